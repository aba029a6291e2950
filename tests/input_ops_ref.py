"""fp64 numpy restatement of the input phase of a step and of a reset (``run_update_ops``, ``run_reset_ops`` and ``apply_frame_wrench`` of
diy_gym_amd/csrc/dg_solver.h): what an action row turns into -- motor targets, joint torques, external wrenches, rotor speeds -- what
one external wrench call adds, and what a reset writes -- respawn jitter from the counter RNG, joint rest positions, randomized
masses and damping, texture parameters, the counters.  Neither the library under test nor the C oracle is called.  Inputs: the env's
models and addons (each addon's ``op`` says where its action columns and its addon state are, ``op.index`` is its RNG stream), the
layout's state offsets, and the state row.  tests/test_input_ops_ref.py pins the pieces (finite-difference Jacobians,
tests/dynamics_ref.py, the moments of the RNG, the two oracle builds) and fixes ``TOL``; tests/test_input_ops_gpu.py holds the
kernels to it.

Kinematics are those of tests/output_ops_ref.py (``_Body``: URDF link frames by ``nphelpers.link_frames``, the reported base by
``base_state_ref``).  A wrench is a force ``F`` at the world point ``P`` and a torque ``T``:

  * LINK_FRAME means the INERTIAL frame of the link (of the base: the reported base): ``F = R f``, ``T = R t``, ``P = p + R pos``;
  * a body with a free base gets ``[F, (P - base origin) x F + T]`` added to its external wrench cells;
  * every movable joint between the link and the base gets ``axis . ((P - joint origin) x F + T)`` (revolute) or ``axis . F``
    (prismatic) added to its torque cell: J^T of the wrench.

``Cells`` is what a call returns: per named state column the expected value of every env, its class, and whether it is exact.  A
class tolerance is absolute up to magnitude 1 and relative to the env's largest reference entry of the class beyond that.
``DG_OP_IK_CONTROL`` is not restated (tests/ik_ref.py owns its targets): its TARGET_POS cells are class 'skip', its TARGET_VEL cells
exact zeros and it adds no torque.

Torque mode of ``joint_controller`` ADDS the action to the torque cell, as ``Backend.apply_joint_torque`` documents and as the
admittance and wrench ops do; with nothing else on the joint the cell is the action's float32 bits (0 + a).
"""
import numpy as np

import base_state_ref as bs
import output_ops_ref as O
from diy_gym_amd.scene import K
from nphelpers import ancestors

F32 = np.float32

# class -> the larger error of the fp64 and the fp32 build of the oracle over the scenes of tests/input_ops_cases.py at 70 envs, as
# tests/test_input_ops_ref.py measures it on this tree (update ops and the wrench entry on the edge states; three resets, hot_start 0),
# rounded up to three significant digits; that test asserts it and names the scene.  The fp64 build stays below 2e-14 everywhere.
# N, N m (external wrench), N m (joint torque), m, rad (angle of the relative rotation), scale, damping.
#                       fp32 build (scene)        fp64 build
MEASURED = {
    'force': 6.53e-7,   # 6.522e-7 (generic)       7.2e-16   LINK-frame forces turned into the world frame and accumulated, relative (tens of N)
    'moment': 1.37e-5,  # 1.360e-5 (drone)         1.7e-15   the ladder 50 m from the origin: (P - base) x F cancels six digits
    'torque': 1.29e-5,  # 1.283e-5 (generic)       5.4e-15   the wrench entry 50 m out: (P - joint) x F cancels; admittance alone 2.14e-6 (pair_adm)
    'rpos': 7.21e-8,    # 7.209e-8 (generic)       1.4e-16
    'rrot': 2.50e-7,    # 2.494e-7 (drone)         1.2e-16
    'mass': 2.73e-7,    # 2.727e-7 (one_arm)       4.4e-17
    'damp': 1.02e-8,    # 1.013e-8 (generic)       0
}
TOL = {k: 4 * v for k, v in MEASURED.items()}

_U = np.uint64


# ---- the counter RNG ----------------------------------------------------------------------------------------------------------
def _mix64(z):
    z = z ^ (z >> _U(30))
    z = z * _U(0xBF58476D1CE4E5B9)
    z = z ^ (z >> _U(27))
    z = z * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def rng_uniform(seed, env, episode, op, comp):
    """u in [0, 1), a multiple of 2^-24 (so exact in float32): the stream (seed, global env index, episode, op index, component).
    Exact integer arithmetic modulo 2^64 in numpy uint64; arguments broadcast."""
    seed, env, episode, op, comp = (np.atleast_1d(np.asarray(v, dtype=np.int64)).astype(_U) for v in (seed, env, episode, op, comp))
    with np.errstate(over='ignore'):
        z = _mix64(seed + _U(0x9E3779B97F4A7C15) * (env + _U(1)))
        z = _mix64(z ^ (episode * _U(0xD1342543DE82EF95) + op * _U(0x2545F4914F6CDD1D) + comp + _U(1)))
    u = (z >> _U(40)).astype(np.float64) / 16777216.0
    return u if u.size > 1 else float(u[0])


def spool_up(w, a, k):
    """``w + (a - w) k`` in float32 with every operation rounded on its own."""
    w, a, k = F32(w), F32(a), F32(k)
    d = F32(a - w)
    p = F32(d * k)
    return F32(w + p)


def qfrom_euler(r, p, y):
    """pybullet's getQuaternionFromEuler, xyzw: Rz(yaw) Ry(pitch) Rx(roll)."""
    cr, sr, cp, sp, cy, sy = np.cos(r / 2), np.sin(r / 2), np.cos(p / 2), np.sin(p / 2), np.cos(y / 2), np.sin(y / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


# ---- what a call returns ---------------------------------------------------------------------------------------------------------
class Cells:
    """``col``: state column -> [class, value [B], exact [B] bool]; ``quats``: first column of a base quaternion -> [B, 4].
    Classes: those of ``TOL``, 'exact', 'spool' (a rotor speed: exact in float32), 'freq' (within one float32 ulp), 'skip' (named,
    not compared)."""
    def __init__(self, B):
        self.B, self.col, self.quats = B, {}, {}

    def put(self, e, col, cls, value, exact=False):
        if col not in self.col:
            self.col[col] = [cls, np.full(self.B, np.nan), np.zeros(self.B, dtype=bool)]
        assert self.col[col][0] == cls, (col, cls, self.col[col][0])
        self.col[col][1][e], self.col[col][2][e] = value, exact or cls == 'exact'

    def quat(self, e, col, q):
        self.quats.setdefault(col, np.zeros((self.B, 4)))[e] = q

    def columns(self):
        """Every state column the call may write."""
        return sorted(set(self.col) | {c + k for c in self.quats for k in range(4)})

    def of_class(self, cls):
        return sorted(c for c, v in self.col.items() if v[0] == cls)


def compare(cells, got, tol=TOL, spool_tol=0.0):
    """``got`` [B, state_dim]: the state read back.  Returns an ``output_ops_ref.Report``: figures per class as a fraction of ``tol``
    (pass ``tol`` of ones for raw errors).  ``spool_tol``: what a rotor speed may differ by from the three float32 operations of
    ``spool_up`` -- 0 for anything that computes in float32; the fp64 build of the oracle does the same three steps in double with
    the rate 0.1 unrounded: three roundings of values below 1 (2^-24 each) and the rate's 1.5e-9, so 2e-7 there."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape[0] == cells.B, (got.shape, cells.B)
    rep = O.Report(cells.B)
    bad_exact = []
    for c, (cls, val, ex) in cells.col.items():
        if cls == 'skip' or not ex.any():
            continue
        same = got[:, c].astype(F32) == val.astype(F32)
        if not same[ex].all():
            bad_exact.append((c, int(np.nonzero(ex & ~same)[0][0])))
    rep.note('exact', np.array([np.inf if bad_exact else 0.0]), 'cells (column, first env) %s' % bad_exact[:8])
    for cls in tol:
        cols = cells.of_class(cls)
        if cls == 'rrot':
            for c, q in sorted(cells.quats.items()):
                ang = np.array([O.geodesic(O.quat_matrix(got[e, c:c + 4]), O.quat_matrix(q[e])) if np.isfinite(got[e, c:c + 4]).all() and np.abs(got[e, c:c + 4]).max() > 0 else np.nan
                                for e in range(cells.B)])
                rep.note(cls, ang / tol[cls], 'rotation of the quaternion at column %d' % c)
                norm = np.abs(np.linalg.norm(got[:, c:c + 4], axis=1) - 1.0)
                rep.note('exact', np.where(norm < 1e-6, 0.0, np.inf), 'norm of the quaternion at column %d' % c)
            continue
        if not cols:
            continue
        ref = np.stack([cells.col[c][1] for c in cols], axis=1)
        ex = np.stack([cells.col[c][2] for c in cols], axis=1)
        mag = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
        frac = np.abs(got[:, cols] - ref) / (tol[cls] * mag)
        rep.note(cls, np.where(ex, 0.0, frac), 'columns %s' % cols)
    for c in cells.of_class('spool'):
        d = np.abs(got[:, c].astype(F32).astype(np.float64) - cells.col[c][1].astype(F32).astype(np.float64))
        rep.note('spool', np.where(d <= spool_tol, 0.0, np.inf), 'rotor speed at column %d (largest difference %.3g)' % (c, d.max()))
    for c in cells.of_class('freq'):
        want = cells.col[c][1].astype(F32)
        d = np.abs(got[:, c].astype(F32).astype(np.float64) - want.astype(np.float64))
        rep.note('freq', d / np.spacing(want).astype(np.float64), 'column %d (in float32 ulps)' % c)
    return rep


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _kind(a):
    return type(a).__name__


UPDATE_KINDS = ('JointController', 'InverseKinematicsController', 'ExternalForce', 'Propellor', 'AdmittanceController')
RESET_KINDS = ('Respawn', 'DynamicsRandomizer', 'VisualRandomizer') + UPDATE_KINDS


class InputRef:
    def __init__(self, env):
        self.env, self.layout = env, env.layout
        L = env.layout
        self.bodies = {m.name: O._Body(env, m) for m in env.models.values()}
        self.g = np.array(env.builder.gravity, dtype=np.float64)
        addons = [a for r in env.receptors.values() for a in r.addons.values() if getattr(a, 'op', None) is not None]
        self.update_addons = sorted((a for a in addons if _kind(a) in UPDATE_KINDS), key=lambda a: a.op.index)
        self.reset_addons = sorted((a for a in addons if _kind(a) in RESET_KINDS), key=lambda a: a.op.index)
        self.all_slots = env._all_slots
        # mass scale cells: model name -> {q_index: state column} (the dynamics_randomizer of the model owns them)
        self.scale_col = {n: {} for n in self.bodies}
        for a in addons:
            if _kind(a) == 'DynamicsRandomizer':
                for k, j in enumerate(a.joint_ids):
                    self.scale_col[a.parent.name][a.parent.robot.joints[j].q_index] = L.addon_off + a.op.state_off + k
        I = L.I
        self.prev_off = {n: int(I[int(I[K.H_OFF_BODY_I]) + b.body * K.BI_STRIDE + K.BI_PREV_OFF]) for n, b in self.bodies.items()}

    # -- columns --
    def ext_col(self, name):
        b = self.bodies[name]
        return self.layout.body_state_off[b.body] + (K.BS_FIXED_END if b.fixed else K.BS_FLOAT_END)

    def joint_col(self, name, q_index, what):
        return self.bodies[name].q_off[q_index] + what

    def scales(self, name, row):
        b = self.bodies[name]
        return np.array([row[self.scale_col[name][q]] if q in self.scale_col[name] else 1.0 for q in range(b.robot.num_dofs)])

    # -- the wrench arithmetic --
    def _wrench(self, b, frame, link_frame, f, pos, t):
        """(ext [6], tau [num_dofs]) of one wrench on frame ``frame`` (pybullet link index, -1 the base) of the body ``b.at(row)``."""
        F, T, P = (np.asarray(v, dtype=np.float64) for v in (f, t, pos))
        if link_frame:
            fr = b.frame(frame, True)
            F, T, P = fr.R @ F, fr.R @ T, fr.p + fr.R @ P
        ext = np.zeros(6)
        if not b.fixed:
            ext[:3], ext[3:] = F, np.cross(P - b.p_l, F) + T
        return ext, (self.jt_wrench(b, frame, P, F, T) if frame >= 0 else {})

    def _open(self, c, e, row, names=None):
        """Names the wrench, torque, target and rotor cells of env ``e`` with the row's own values, exact; returns the accumulators."""
        acc = {}
        for n, b in self.bodies.items():
            if b.frozen or (names is not None and n not in names):
                continue
            eo = self.ext_col(n)
            if not b.fixed:
                for k in range(6):
                    acc[eo + k] = ['force' if k < 3 else 'moment', row[eo + k], True]
            for q in range(b.robot.num_dofs):
                acc[self.joint_col(n, q, K.LS_TORQUE)] = ['torque', row[self.joint_col(n, q, K.LS_TORQUE)], True]
                if names is None:
                    for what in (K.LS_TARGET_POS, K.LS_TARGET_VEL):
                        acc[self.joint_col(n, q, what)] = ['exact', row[self.joint_col(n, q, what)], True]
        return acc

    @staticmethod
    def _add(acc, col, v, exact=False):
        """Adds ``v`` to a cell; the cell stays exact only where ``v`` is a float32 value added to a zero (0 + v)."""
        acc[col][2] = bool(acc[col][2] and exact and acc[col][1] == 0.0)
        acc[col][1] += v

    def _apply(self, acc, name, ext, tau):
        """``ext`` [6] onto the wrench cells of a free body, ``tau`` {q_index: torque} onto the torque cells it names."""
        b = self.bodies[name]
        if not b.fixed:
            for k in range(6):
                self._add(acc, self.ext_col(name) + k, ext[k])
        for q, v in tau.items():
            self._add(acc, self.joint_col(name, q, K.LS_TORQUE), v)

    @staticmethod
    def _close(c, e, acc):
        for col, (cls, v, ex) in acc.items():
            c.put(e, col, cls, v, ex)

    def wrench(self, states, name, frame, link_frame, f=None, pos=None, t=None):
        """One ``apply_external_force / _wrench / _torque`` call on model ``name``: the body's wrench cells and torque cells of
        every env after it (``f``, ``pos``, ``t``: [3], [B, 3] or None = zero)."""
        states = np.atleast_2d(np.asarray(states, dtype=np.float64))
        B = states.shape[0]
        f, pos, t = (np.zeros((B, 3)) if v is None else np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1, 3), (B, 3)) for v in (f, pos, t))
        c = Cells(B)
        for e in range(B):
            b = self.bodies[name].at(states[e])
            acc = self._open(c, e, states[e], names=(name, ))
            self._apply(acc, name, *self._wrench(b, frame, link_frame, f[e], pos[e], t[e]))
            self._close(c, e, acc)
        return c

    # -- update ops --
    def update(self, states, actions, mask=None, real=np.float32):
        """The wrench, torque, target and rotor-speed cells of every env after the update ops selected by ``mask`` (bit = the
        addon's ``op.slot``; None: all) ran on ``states`` [B, state_dim] with ``actions`` [B, act_dim] (float32 values).  ``real``: the
        type the rotor speed lives in -- float32 everywhere but in the fp64 build of the oracle, whose spool-up is the same three
        steps in double (the thrust follows the rotor speed, so the reference of that build has to follow it too)."""
        self.real = real
        states = np.atleast_2d(np.asarray(states, dtype=np.float64))
        B = states.shape[0]
        c = Cells(B)
        if actions is None:
            actions, mask = np.zeros((B, 1)), 0
        actions = np.atleast_2d(np.asarray(actions, dtype=np.float64))
        mask = self.all_slots if mask is None else int(mask)
        for e in range(B):
            row = states[e]
            for b in self.bodies.values():
                b.at(row)
            acc = self._open(c, e, row)
            for a in self.update_addons:
                if _kind(a) == 'Propellor':
                    acc.setdefault(self.layout.addon_off + a.op.state_off, ['spool', row[self.layout.addon_off + a.op.state_off], False])
                if (mask >> a.op.slot) & 1:
                    self._update_op(acc, row, a, actions[e, a.op.io_off:a.op.io_off + a.op.io_dim])
            self._close(c, e, acc)
        return c

    def _update_op(self, acc, row, a, act):
        kind, name = _kind(a), a.parent.name
        b = self.bodies[name]
        if kind == 'JointController':
            for k, j in enumerate(a.joint_ids):
                q = b.robot.joints[j].q_index
                if a.control_mode == K.JC_POSITION:
                    acc[self.joint_col(name, q, K.LS_TARGET_POS)][1], acc[self.joint_col(name, q, K.LS_TARGET_VEL)][1] = act[k], 0.0
                elif a.control_mode == K.JC_VELOCITY:
                    acc[self.joint_col(name, q, K.LS_TARGET_VEL)][1], acc[self.joint_col(name, q, K.LS_TARGET_POS)][1] = act[k], 0.0
                else:
                    self._add(acc, self.joint_col(name, q, K.LS_TORQUE), act[k], exact=True)
        elif kind == 'InverseKinematicsController':
            for j in a.joint_ids:
                q = b.robot.joints[j].q_index
                acc[self.joint_col(name, q, K.LS_TARGET_POS)][0] = 'skip'
                acc[self.joint_col(name, q, K.LS_TARGET_VEL)][1] = 0.0
        elif kind == 'ExternalForce':
            if not b.fixed:
                self._apply(acc, name, *self._wrench(b, -1, False, act[:3], a.xyz, np.zeros(3)))
        elif kind == 'Propellor':
            col = self.layout.addon_off + a.op.state_off
            w = spool_up(row[col], act[0], a.spool_up_rate) if self.real is np.float32 else row[col] + (act[0] - row[col]) * a.spool_up_rate
            acc[col][1] = float(w)
            if not b.fixed:
                self._apply(acc, name, *self._wrench(b, a.frame_id, True, [0.0, 0.0, a.max_thrust * float(w)], np.zeros(3), [0.0, 0.0, a.max_torque * float(w)]))
        elif kind == 'AdmittanceController':
            tau = self.admittance(b, row, a, act)
            for j in a.joint_ids:
                q = b.robot.joints[j].q_index
                self._add(acc, self.joint_col(name, q, K.LS_TORQUE), tau[q])
        else:
            raise NotImplementedError(kind)

    def jt_wrench(self, b, frame, P, F, T):
        """J^T [F; T] for the force ``F`` at the world point ``P`` and the torque ``T`` on the link of joint ``frame``: {q_index: torque}
        over the movable joints between that link and the base."""
        tau = {}
        anc = ancestors(b.robot, b.robot.joints[frame].child)
        for j, o, a in b.joints:
            if j.q_index in anc:
                tau[j.q_index] = a @ F if j.type == 'prismatic' else a @ (np.cross(P - o, F) + T)
        return tau

    def gravity_compensation(self, b, scale):
        """[num_dofs] joint torques that hold ``b.at(row)`` against gravity: minus the gravity torque of each joint's subtree, every
        URDF link weighing ``mass x scale[the movable joint it rides on]``."""
        tau = np.zeros(b.robot.num_dofs)
        for lname, link in b.robot.links.items():
            car = b.carrier[lname]
            if car < 0 or link.mass <= 0:
                continue
            cw = (b.T[lname] * link.inertial_origin).p
            w8 = self.g * link.mass * scale[car]
            anc = ancestors(b.robot, lname)
            for j, o, a in b.joints:
                if j.q_index in anc:
                    tau[j.q_index] -= w8 @ a if j.type == 'prismatic' else w8 @ np.cross(a, cw - o)
        return tau

    def admittance(self, b, row, a, act):
        """[num_dofs] torques of the admittance op: J^T wrench at the offset point of the end effector's inertial frame, gravity
        compensation with the env's mass scales, joint PD towards ``target_pose``."""
        fr = b.frame(a.end_frame, True)
        pw = fr.p + fr.R @ np.asarray(a.offset_admittance_point, dtype=np.float64)
        tau = self.gravity_compensation(b, self.scales(a.parent.name, row))
        for q, v in self.jt_wrench(b, a.end_frame, pw, act[:3], act[3:6]).items():
            tau[q] += v
        target = (list(a.target_pose) + [0.0] * len(a.joint_ids))[:len(a.joint_ids)]
        for k, j in enumerate(a.joint_ids):
            q = b.robot.joints[j].q_index
            tau[q] += a.kp * (target[k] - b.q[q]) - a.kd * b.qd[q]
        return tau

    # -- reset ops --
    def reset(self, states, env_index, seed):
        """Every cell a reset writes, for the envs whose state rows are ``states`` and whose GLOBAL env indices are ``env_index``,
        drawn from each row's own episode counter."""
        states = np.atleast_2d(np.asarray(states, dtype=np.float64))
        B = states.shape[0]
        env_index = np.broadcast_to(np.asarray(env_index, dtype=np.int64), (B, ))
        c = Cells(B)
        self.draws = []   # every u drawn, for the tests of the draws themselves: (addon kind, component, u)
        for e in range(B):
            self._reset_env(c, e, states[e].copy(), int(env_index[e]), int(seed))
        return c

    def _u(self, seed, ge, ep, a, comp):
        u = rng_uniform(seed, ge, ep, a.op.index, comp)
        self.draws.append((_kind(a), comp, u))
        return u

    def _reset_env(self, c, e, row, ge, seed):
        L = self.layout
        episode = int(np.uint64(row[K.ST_EPISODE]))
        for a in self.reset_addons:
            kind, name = _kind(a), a.parent.name
            b = self.bodies[name]
            if kind == 'Respawn':
                ep = 0 if a.once else episode + 1
                u = np.array([self._u(seed, ge, ep, a, k) for k in range(6)]) - 0.5
                p = np.asarray(a.initial_pose[0]) + u[:3] * np.asarray(a.position_range)
                ang = u[3:] * np.asarray(a.rotation_range)
                q = bs.qmul(a.initial_pose[1], qfrom_euler(*ang))[0]
                pl, ql, _, _ = (v[0] for v in bs.stored_from_report(L, b.body, p, q))
                so = L.body_state_off[b.body]
                for k in range(3):
                    c.put(e, so + k, 'rpos', pl[k])
                    row[so + k] = pl[k]
                c.quat(e, so + K.BS_QUAT, ql)
                row[so + K.BS_QUAT:so + K.BS_QUAT + 4] = ql
                if not b.fixed:
                    for k in range(6):
                        c.put(e, so + K.BS_LINVEL + k, 'exact', 0.0)
                        row[so + K.BS_LINVEL + k] = 0.0
            elif kind in UPDATE_KINDS:
                if not hasattr(a, 'rest_position'):
                    continue
                for j, rest in zip(a.joint_ids, a.rest_position):   # (zip: a rest_position shorter than the joint list resets its first joints)
                    q = b.robot.joints[j].q_index
                    c.put(e, self.joint_col(name, q, K.LS_Q), 'exact', float(F32(rest)))
                    c.put(e, self.joint_col(name, q, K.LS_QD), 'exact', 0.0)
                    row[self.joint_col(name, q, K.LS_Q)], row[self.joint_col(name, q, K.LS_QD)] = float(F32(rest)), 0.0
            elif kind == 'VisualRandomizer':
                so = L.addon_off + a.op.state_off
                u = [self._u(seed, ge, episode + 1, a, k) for k in range(K.TX_STRIDE)]
                for k in range(6):
                    c.put(e, so + k, 'exact', u[k])
                c.put(e, so + K.TX_FREQ, 'freq', 2.0 + 14.0 * u[6])
                kind32, kind64 = int(F32(3.0) * F32(u[7])), int(np.floor(3.0 * u[7]))
                assert kind32 == kind64, ('the float32 and the fp64 floor of 3 u differ', u[7])
                c.put(e, so + K.TX_KIND, 'exact', 1.0 + kind64)
            elif kind == 'DynamicsRandomizer':
                so, n = L.addon_off + a.op.state_off, len(a.joint_ids)
                damping = [b.robot.joints[j].damping for j in a.joint_ids]
                damp = row[so + n]
                for rnd in ((0, 1) if episode == 0 else (1, )):   # two rounds at an env's first reset
                    ep = 0 if rnd == 0 else episode + 1
                    for k in range(n):
                        um = a.mass_range[0] + (a.mass_range[1] - a.mass_range[0]) * self._u(seed, ge, ep, a, 2 * k)
                        row[so + k] = min(max(row[so + k] * abs(np.log(um)), a.mass_scale_limits[0]), a.mass_scale_limits[1])
                        ud = a.damping_range[0] + (a.damping_range[1] - a.damping_range[0]) * self._u(seed, ge, ep, a, 2 * k + 1)
                        damp = max(np.log(ud) * damping[k], 0.0)   # body-wide: the last joint's draw of the last round stays
                for k in range(n):
                    c.put(e, so + k, 'mass', row[so + k])
                c.put(e, so + n, 'damp', damp)
        for n, b in self.bodies.items():   # the velocities a force/torque sensor differences: none across a reset
            po = self.prev_off[n]
            if po < 0 or b.frozen:
                continue
            first, nl = L.body_first_link[b.body], L.body_n_links[b.body]
            for i in range(nl):
                c.put(e, po + i, 'exact', row[L.link_state_off[first + i] + K.LS_QD])
            if not b.fixed:
                so = L.body_state_off[b.body]
                for k in range(6):
                    c.put(e, po + nl + k, 'exact', row[so + K.BS_LINVEL + k])
        if L.warm_off >= 0:
            c.put(e, L.warm_off, 'exact', 0.0)
        c.put(e, K.ST_STEP, 'exact', 0.0)
        c.put(e, K.ST_EPISODE, 'exact', float(F32(episode + 1)))   # a float32 cell: beyond 2^24 the counter no longer advances
