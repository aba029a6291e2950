"""fp64 numpy restatement of the output phase of a step (``run_output_ops`` of diy_gym_amd/csrc/dg_solver.h): observation columns,
reward columns, terminal bytes, the collapsed reward and the collapsed terminal flag, from ONE state row.  Neither the library under
test nor the C oracle is called.  Inputs: the env's models and addons (each addon's ``op.io_off`` / ``rew_op`` / ``term_op`` say where
its columns are), the layout's state offsets and the state row.  tests/test_output_ops_ref.py pins the pieces (scipy, finite
differences, the fp64 oracle build) and fixes ``TOL``; tests/test_output_ops_gpu.py holds the kernels to it.

Kinematics: URDF link frames by ``nphelpers.link_frames`` from the parsed URDF tree (as tests/dynamics_ref.py); the base LINK pose is
what the state stores, the REPORTED base (inertial frame) comes from ``base_state_ref.report_from_stored``; the twist of a frame is
the base twist carried to the frame's origin plus one column per joint on its path (revolute ``axis x r`` and ``axis``, prismatic
``axis``).  Which frame an op reads:

  * ``object_state_sensor``: inertial frames (of the link, or the reported base);
  * ``reach_target``: URDF link frames, and the reported base where it names no frame;
  * ``fell_over``: the reported base.

Rotations are compared as rotations: the matrix rebuilt from the three reported fixed-axis XYZ angles against the reference
rotation, by geodesic angle.  In its two gimbal branches (``|sarg| >= 0.99999``) pybullet's Euler formula is itself approximate
(up to 6.3e-3 rad of rebuilt rotation at the threshold); the reference applies the same formula to its own quaternion and reports
that rebuilt error per env: it is the allowance such an env gets on top of the tolerance, no constant.  An env whose ``|sarg|`` is
within one rotation tolerance of the threshold may take either branch in fp32 and gets the larger of the two formulas' errors.

Discontinuities: per env and terminal column ``term_margin`` is the distance of the fp64 quantity (tilt angle, reach distance) from
its threshold; a byte is compared exactly unless that distance is within the quantity's own tolerance.

Force/torque columns (tests/joint_wrench_ref.py owns them) are NaN in ``obs`` and left out of every comparison.

``TOL`` -- absolute, per quantity class, except ``elec`` which is relative to the reward -- is 4 x the larger error of the two CPU
builds of the oracle on the edge states of tests/output_ops_cases.py, measured in tests/test_output_ops_ref.py, where both builds
must stay below TOL / 4, and that test also asserts that every entry IS 4 x the measured maximum; it is never taken from what the
kernels give.  No term is added for the kernels' hardware sine and cosine (``rot_axis`` in dg_device.h, about 1e-6 absolute against
the fp32 oracle's libm): the kernels meet the bare table in every form (DESIGN.md "Output ops against fp64" has the figures).
"""
import numpy as np

import base_state_ref as bs
from diy_gym_amd.mathx import Transform
from diy_gym_amd.scene import K
from dynamics_ref import carrier
from nphelpers import ancestors, link_frames

GIMBAL = 0.99999     # |sarg| from which pybullet's getEulerFromQuaternion takes its gimbal branches
COMPONENTS = 0.99    # angles are also compared one by one below this |sarg|
F32_EPS = 2.0 ** -23

# class -> the larger error of the fp64 and the fp32 build of the oracle over the eight scenes of output_ops_cases at 70 envs, edge
# states and the three seeded steps after them, as tests/test_output_ops_ref.py measures it on this tree, rounded up to three
# significant digits (that test asserts it, and names the scene).  The fp64 build stays below 4e-15 in every class.
# Absolute (m, rad, m/s, rad/s) up to magnitude 1, see compare(); elec relative to the reward.
#                      fp32 build (scene)     fp64 build
MEASURED = {
    'pos': 2.12e-7,    # 2.111e-7 (pair_ik)     5.0e-16
    'rot': 4.72e-7,    # 4.716e-7 (arms)        5.9e-16   rebuilt rotation beyond the formula's own terms
    'lin': 5.49e-7,    # 5.482e-7 (generic)     1.5e-15
    'ang': 4.58e-7,    # 4.574e-7 (one_arm)     3.1e-15
    'reach': 2.24e-7,  # 2.232e-7 (arms)        5.5e-16
    'elec': 2.09e-7,   # 2.089e-7 (arms_ik)     2.4e-16   relative
    'tilt': 2.9e-7,    # 2.899e-7 (arms_ik)     1.3e-15   the angle in the build's precision from its reported quaternion
}
TOL = {k: 4 * v for k, v in MEASURED.items()}


# ---- rotations ----------------------------------------------------------------------------------------------------------------
def quat_matrix(q):
    """R of the quaternion xyzw of any positive norm."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


BRANCHES = ('trace', 'x', 'y', 'z')


def matrix_quat(R):
    """``(q xyzw, branch)``: the four-branch conversion every link-frame quaternion goes through; branch as ``BRANCHES``."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q, br = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s], 0
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q, br = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s], 1
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q, br = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s], 2
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q, br = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s], 3
    q = np.array(q)
    return q / np.linalg.norm(q), br


def sarg_of(q):
    x, y, z, w = q
    return -2.0 * (x * z - w * y)


def euler_plain(q):
    """pybullet's getEulerFromQuaternion outside its gimbal branches (fixed-axis XYZ: R = Rz(yaw) Ry(pitch) Rx(roll))."""
    x, y, z, w = q
    return np.array([np.arctan2(2.0 * (y * z + w * x), w * w - x * x - y * y + z * z), np.arcsin(np.clip(sarg_of(q), -1.0, 1.0)),
                     np.arctan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z)])


def euler_gimbal(q):
    """Its gimbal branches: roll 0, pitch -+pi/2, all of the rest in yaw."""
    x, y, z, w = q
    return np.array([0.0, -np.pi / 2, 2.0 * np.arctan2(x, -y)]) if sarg_of(q) < 0.0 else np.array([0.0, np.pi / 2, 2.0 * np.arctan2(-x, y)])


def euler_pybullet(q):
    return euler_gimbal(q) if abs(sarg_of(q)) >= GIMBAL else euler_plain(q)


def euler_matrix(rpy):
    r, p, y = (float(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr], [-sp, cp * sr, cp * cr]])


def geodesic(Ra, Rb):
    """Angle of Ra^T Rb by the chord ``|Ra - Rb|_F = 2 sqrt(2) sin(angle / 2)``: no cancellation at small angles."""
    return 2.0 * np.arcsin(min(1.0, np.linalg.norm(np.asarray(Ra) - np.asarray(Rb)) / (2.0 * np.sqrt(2.0))))


def wrap(a):
    return (np.asarray(a) + np.pi) % (2.0 * np.pi) - np.pi


# ---- kinematics of one body in one env -----------------------------------------------------------------------------------------
class _Frame:
    __slots__ = ('p', 'R', 'v', 'w', 'branch')


class _Body:
    def __init__(self, env, model):
        self.layout, self.model, self.robot, self.body = env.layout, model, model.robot, model.uid
        if model.uid in env.layout.aliases:
            raise NotImplementedError('output_ops_ref: a model merged into its parent has no body of its own')
        if self.robot.num_dofs and model.flat.scale != 1.0:
            raise NotImplementedError('output_ops_ref: a scaled body with joints')
        I, F = env.layout.I, env.layout.F
        flags = int(I[int(I[K.H_OFF_BODY_I]) + self.body * K.BI_STRIDE + K.BI_FLAGS])
        self.frozen = bool(flags & K.BODY_FROZEN)
        self.fixed = env.layout.body_fixed[self.body]
        row = F[int(I[K.H_OFF_BODY_F]) + self.body * K.BF_STRIDE:][:K.BF_STRIDE]
        self.init = np.array(row[K.BF_INIT_POS:K.BF_INIT_POS + 3], dtype=np.float64), np.array(row[K.BF_INIT_QUAT:K.BF_INIT_QUAT + 4], dtype=np.float64)
        first = env.layout.body_first_link[self.body]
        self.q_off = [env.layout.link_state_off[first + i] for i in range(self.robot.num_dofs)]
        self.carrier = carrier(self.robot)
        self.by_q = {j.q_index: j for j in self.robot.joints if j.movable}

    def at(self, row):
        """The body in the env whose state row is ``row``: sets the base, the joint values and every URDF link frame."""
        row = np.asarray(row, dtype=np.float64)
        if self.frozen:
            self.p_l, q_l = self.init
        else:
            so = self.layout.body_state_off[self.body]
            self.p_l, q_l = row[so:so + 3], row[so + K.BS_QUAT:so + K.BS_QUAT + 4]
        self.q_l = q_l / np.linalg.norm(q_l)
        self.v_l, self.w_l = np.zeros(3), np.zeros(3)
        if not self.fixed:
            self.v_l, self.w_l = row[so + K.BS_LINVEL:so + K.BS_LINVEL + 3], row[so + K.BS_ANGVEL:so + K.BS_ANGVEL + 3]
        self.q = np.array([row[o + K.LS_Q] for o in self.q_off])
        self.qd = np.array([row[o + K.LS_QD] for o in self.q_off])
        self.applied = np.array([row[o + K.LS_APPLIED] for o in self.q_off])
        self.T, self.joints = link_frames(self.robot, self.q, Transform(quat_matrix(self.q_l), self.p_l))
        return self

    def frame(self, fr, com):
        """Pose and twist of frame ``fr`` (the pybullet link index; -1 the base): the inertial frame with
        ``com``, else the URDF link frame."""
        f = _Frame()
        f.branch = None
        if fr < 0:
            if com:
                p, q, v, w = (a[0] for a in bs.report_from_stored(self.layout, self.body, self.p_l, self.q_l, self.v_l, self.w_l))
                f.p, f.R, f.v, f.w = p, quat_matrix(q), v, w
            else:
                f.p, f.R, f.v, f.w = self.p_l.copy(), quat_matrix(self.q_l), self.v_l.copy(), self.w_l.copy()
            return f
        link = self.robot.joints[fr].child
        T = self.T[link] * self.robot.links[link].inertial_origin if com else self.T[link]
        anc = ancestors(self.robot, link)
        w = self.w_l.copy()
        v = self.v_l + np.cross(self.w_l, T.p - self.p_l)
        for j, o, a in self.joints:
            if j.q_index not in anc:
                continue
            qd = self.qd[j.q_index]
            if j.type == 'prismatic':
                v = v + a * qd
            else:
                v = v + np.cross(a, T.p - o) * qd
                w = w + a * qd
        f.p, f.R, f.v, f.w = T.p, T.R, v, w
        c = self.carrier[link]
        if c >= 0:   # the rotation the kernels convert is that of the moving link the frame rides on
            f.branch = matrix_quat(self.T[self.by_q[c].child].R)[1]
        return f


# ---- the ops -------------------------------------------------------------------------------------------------------------------
class Result:
    """What ``OutputRef.evaluate`` returns; every array has one row per env.

    obs [B, obs_dim] (NaN: force/torque), rew, term (uint8), rew_sum, term_flag; ``obs_class`` / ``rew_class`` / ``term_class``
    name each column's class ('exact', 'pos', 'lin', 'ang', 'rot', 'ft' | 'reach', 'elec', 'exact' | 'reach', 'tilt', 'timer');
    ``rew_scale`` the multiplier of a
    reach reward; ``rots`` one entry per rotation triple: dict(off, R [B, 3, 3], sarg [B], own_error [B], other_error [B]);
    ``term_margin`` [B, term_dim] distance of the quantity from its threshold (inf for the timer); ``term_value`` the quantity;
    ``branches`` {(model name, frame): [B] index into BRANCHES} for every observed link frame on a moving link."""


def _kind(addon):
    return type(addon).__name__


class OutputRef:
    def __init__(self, env):
        self.env, self.layout = env, env.layout
        self.bodies = {}
        for m in env.models.values():
            self.bodies[m.name] = _Body(env, m)
        self.obs_dim, self.rew_dim, self.term_dim = env.layout.obs_dim, env.layout.rew_dim, env.layout.term_dim
        # (receptor, addon) in any order: every output column is addressed by the addon's own offsets
        self.addons = [(r, a) for r in env.receptors.values() for a in r.addons.values()]
        self.collapse_all = env.collapse_terminals_func is all

    def _body(self, model):
        return self.bodies[model.name]

    def evaluate(self, states):
        states = np.atleast_2d(np.asarray(states, dtype=np.float64))
        B = states.shape[0]
        r = Result()
        r.obs = np.full((B, max(self.obs_dim, 1)), np.nan)
        r.rew = np.zeros((B, max(self.rew_dim, 1)))
        r.term = np.zeros((B, max(self.term_dim, 1)), dtype=np.uint8)
        r.obs_class, r.rew_class, r.term_class = [None] * self.obs_dim, [None] * self.rew_dim, [None] * self.term_dim
        r.rew_scale = np.ones(max(self.rew_dim, 1))
        r.term_margin, r.term_value = np.full(r.term.shape, np.inf), np.zeros(r.term.shape)
        r.term_group = [None] * self.term_dim
        r.rots, r.branches = {}, {}
        r.rew_sum, r.term_flag = np.zeros(B), np.zeros(B, dtype=np.uint8)
        for e in range(B):
            row = states[e]
            for b in self.bodies.values():
                b.at(row)
            for receptor, a in self.addons:
                self._addon(r, e, B, row, receptor, a)
            if self.env._timer_op is not None:
                k = self.env._timer_op.io_off
                r.term_class[k], r.term_group[k] = 'timer', id(self.env)
                r.term_value[e, k] = row[K.ST_STEP]
                r.term[e, k] = row[K.ST_STEP] >= float(self.env._max_episode_steps)
            r.rew_sum[e] = r.rew[e, :self.rew_dim].sum()
        assert None not in r.obs_class and None not in r.rew_class and None not in r.term_class, 'an output column no restated op writes'
        r.term_flag = self.collapse(r.term, r.term_group)
        r.rots = list(r.rots.values())
        return r

    def collapse(self, term, groups):
        """The collapsed flag of terminal bytes ``term`` [B, term_dim]: any byte, or under terminal_if_all a byte in every group."""
        term = np.asarray(term)[:, :self.term_dim] != 0
        if not self.collapse_all:
            return term.any(axis=1).astype(np.uint8)
        out = np.ones(term.shape[0], dtype=bool) if self.term_dim else np.zeros(term.shape[0], dtype=bool)
        for g in set(groups):
            out &= term[:, [k for k, gk in enumerate(groups) if gk == g]].any(axis=1)
        return out.astype(np.uint8)

    def _cols(self, r, e, k, values, cls):
        for i, v in enumerate(values):
            r.obs[e, k + i], r.obs_class[k + i] = v, cls

    def _reach(self, a):
        t = self._body(a.target_model).frame(a.target_frame_id, a.target_frame_id < 0)
        s = self._body(a.source_model).frame(a.source_frame_id, a.source_frame_id < 0)
        return np.linalg.norm(t.p - s.p)

    def _addon(self, r, e, B, row, receptor, a):
        kind = _kind(a)
        if kind == 'JointStateSensor':
            b, k, n = self._body(a.parent), a.op.io_off, len(a.joint_ids)
            qi = [b.robot.joints[j].q_index for j in a.joint_ids]
            self._cols(r, e, k, b.q[qi], 'exact')
            k += n
            if a.include_velocity:
                self._cols(r, e, k, b.qd[qi], 'exact')
                k += n
            if a.include_effort:
                self._cols(r, e, k, b.applied[qi], 'exact')
        elif kind == 'ObjectStateSensor':
            t = self._body(a.target_model).frame(a.target_frame_id, True)
            p, R, v, w = t.p, t.R, t.v, t.w
            key = (a.target_model.name, a.target_frame_id)
            if t.branch is not None:
                r.branches.setdefault(key, np.zeros(B, dtype=int))[e] = t.branch
            if a.source_model is not None:
                s = self._body(a.source_model).frame(a.source_frame_id, True)
                # the kept quirk: world-frame differences, and q_source (x) q_target for the rotation
                p, R, v, w = p - s.p, s.R @ R, v - s.v, w - s.w
                if s.branch is not None:
                    r.branches.setdefault((a.source_model.name, a.source_frame_id), np.zeros(B, dtype=int))[e] = s.branch
            k = a.op.io_off
            self._cols(r, e, k, p, 'pos')
            k += 3
            if a.include_velocity:
                self._cols(r, e, k, v, 'lin')
                k += 3
            if a.include_rotation:
                q = matrix_quat(R)[0]
                sarg = sarg_of(q)
                own, other = (euler_gimbal, euler_plain) if abs(sarg) >= GIMBAL else (euler_plain, euler_gimbal)
                self._cols(r, e, k, own(q), 'rot')
                rot = r.rots.setdefault(k, dict(off=k, R=np.zeros((B, 3, 3)), sarg=np.zeros(B), own_error=np.zeros(B), other_error=np.zeros(B)))
                rot['R'][e], rot['sarg'][e] = R, sarg
                rot['own_error'][e], rot['other_error'][e] = geodesic(euler_matrix(own(q)), R), geodesic(euler_matrix(other(q)), R)
                k += 3
                if a.include_velocity:
                    self._cols(r, e, k, w, 'ang')
        elif kind == 'Propellor':
            self._cols(r, e, a.obs_op.io_off, [row[self.layout.addon_off + a.op.state_off]], 'exact')
        elif kind == 'ForceTorqueSensor':
            self._cols(r, e, a.op.io_off, [np.nan] * 6, 'ft')
        elif kind == 'ReachTarget':
            d = self._reach(a)
            k = a.rew_op.io_off
            r.rew[e, k], r.rew_class[k], r.rew_scale[k] = -d * a.multiplier, 'reach', abs(a.multiplier)
            k = a.term_op.io_off
            r.term[e, k], r.term_class[k], r.term_group[k] = d < a.tolerance, 'reach', id(receptor)
            r.term_value[e, k], r.term_margin[e, k] = d, abs(d - a.tolerance)
        elif kind == 'ElectricityCost':
            b, k = self._body(a.parent), a.rew_op.io_off
            r.rew[e, k], r.rew_class[k] = -np.abs(b.applied * b.qd).sum() * a.multiplier, 'elec'
        elif kind == 'TimePenalty':
            k = a.rew_op.io_off
            r.rew[e, k], r.rew_class[k] = a.penalty, 'exact'
        elif kind == 'FellOver':
            b, k = self._body(a.parent), a.term_op.io_off
            q = matrix_quat(b.frame(-1, True).R)[0]
            tilt = 2.0 * np.arctan2(np.linalg.norm(q[:3]), abs(q[3]))   # any rotation away from the load pose, yaw included
            r.term[e, k], r.term_class[k], r.term_group[k] = tilt > a.max_tilt, 'tilt', id(receptor)
            r.term_value[e, k], r.term_margin[e, k] = tilt, abs(tilt - a.max_tilt)
        elif any(getattr(a, n, None) is not None for n in ('rew_op', 'term_op', 'obs_op')) or getattr(getattr(a, 'op', None), 'kind', None) in ('obs', 'rew', 'term'):
            raise NotImplementedError('output_ops_ref: no restatement of %s' % kind)


# ---- comparison ----------------------------------------------------------------------------------------------------------------
class Report:
    """``figures``: class -> largest error as a fraction of what the class allows; ``bad``: what exceeded it; ``near`` [B]: envs
    whose terminal bytes the reference places within one tolerance of a threshold (left out of the exact byte comparison)."""
    def __init__(self, B):
        self.figures, self.bad, self.near = {}, [], np.zeros(B, dtype=bool)

    def note(self, cls, frac, what):
        frac = np.asarray(frac, dtype=np.float64)
        worst = float(frac.max()) if frac.size else 0.0
        self.figures[cls] = max(self.figures.get(cls, 0.0), worst)
        if not worst <= 1.0:   # (a NaN fails)
            e = int(np.argmax(np.where(np.isnan(frac.reshape(frac.shape[0], -1)), np.inf, frac.reshape(frac.shape[0], -1)).max(axis=1)))
            self.bad.append('%s %s: %.4g of the allowance, env %d' % (cls, what, worst, e))

    @property
    def ok(self):
        return not self.bad


def margin_unit(ref, k, tol=TOL):
    """[B] the tolerance of the quantity behind terminal column ``k`` (a tilt angle, a reach distance): one margin."""
    mag = np.maximum(1.0, ref.term_value[:, k]) if ref.term_class[k] == 'reach' else 1.0
    return tol[ref.term_class[k]] * mag + np.zeros(ref.term.shape[0])


def near_threshold(ref, tol=TOL, slack=1.0):
    """[B, term_dim] bool: the fp64 quantity is within its own tolerance of the threshold."""
    out = np.zeros(ref.term.shape, dtype=bool)
    for k, cls in enumerate(ref.term_class):
        if cls != 'timer':
            out[:, k] = ref.term_margin[:, k] <= slack * margin_unit(ref, k, tol)
    return out


def euler_conditioning(sarg):
    """What fp32 costs pybullet's Euler formula outside its gimbal branches, as rebuilt rotation: roll and yaw are atan2 of two
    sums of quaternion products whose length is cos(pitch), pitch the asin of a third; each sum of magnitude <= 1 carries up to
    2^-22 of rounding, so each angle is off by up to sqrt(2) 2^-22 / cos(pitch): 4 x 2^-22 / cos(pitch) in all.  The class tolerance
    is measured where cos(pitch) is of order 1, so only the amplification beyond that is returned: 4 x 2^-22 (1 / cos(pitch) - 1).
    (At the threshold cos(pitch) is 4.5e-3 and the term 2.1e-4; it is what the kept formula costs in single precision, not a
    fault of a kernel.)"""
    return 4.0 * 2.0 ** -22 * (1.0 / np.sqrt(np.maximum(1.0 - np.asarray(sarg) ** 2, 2e-5)) - 1.0)


def compare(ref, got, tol=TOL, slack=1.0):
    """``ref``: a Result; ``got``: dict(obs, rew, term, rew_sum, term_flag) of arrays with one row per env -- another Result's, an
    oracle build's or the kernels'.  ``slack`` scales every allowance (2 for step against observe: each is within one of fp64).

    A class tolerance is absolute up to magnitude 1 and relative to the env's largest reference entry of the class beyond (a body
    a contact has thrown at 100 m/s is known to 1e-5, not 1e-6)."""
    if isinstance(got, Result):
        got = got.__dict__
    obs, rew = np.asarray(got['obs'], dtype=np.float64), np.asarray(got['rew'], dtype=np.float64)
    B = obs.shape[0]
    rep = Report(B)
    cls = np.array(ref.obs_class)
    ex = np.nonzero(cls == 'exact')[0]
    if ex.size:
        same = obs[:, ex].astype(np.float32) == ref.obs[:, ex].astype(np.float32)
        rep.note('exact', np.where(same, 0.0, np.inf), 'observation columns %s' % ex[~same.all(axis=0)].tolist())
    for c in ('pos', 'lin', 'ang'):
        k = np.nonzero(cls == c)[0]
        if k.size:
            mag = np.maximum(1.0, np.abs(ref.obs[:, k]).max(axis=1, keepdims=True))
            rep.note(c, np.abs(obs[:, k] - ref.obs[:, k]) / (slack * tol[c] * mag), 'columns')
    for rot in ref.rots:
        k = rot['off']
        allow = slack * tol['rot'] * np.ones(B)
        gimbal = np.abs(rot['sarg']) >= GIMBAL
        either = np.abs(np.abs(rot['sarg']) - GIMBAL) <= allow
        cond = slack * euler_conditioning(rot['sarg'])
        formula = np.where(either, np.maximum(rot['own_error'], rot['other_error']), rot['own_error']) + np.where(gimbal & ~either, 0.0, cond)
        ang = np.array([geodesic(euler_matrix(obs[e, k:k + 3]), rot['R'][e]) if np.isfinite(obs[e, k:k + 3]).all() else np.nan for e in range(B)])
        rep.note('rot', np.maximum(ang - formula, 0.0) / allow, 'rebuilt rotation of columns %d..%d' % (k, k + 2))
        plain = np.abs(rot['sarg']) < COMPONENTS
        if plain.any():   # each angle's sensitivity to a rotation error grows like 1 / cos(pitch)
            cosp = np.sqrt(np.maximum(1.0 - rot['sarg'] ** 2, 0.0))
            d = np.abs(wrap(obs[plain, k:k + 3] - ref.obs[plain, k:k + 3])) * cosp[plain, None]
            rep.note('rot', np.maximum(d - (cond * cosp)[plain, None], 0.0) / allow[plain, None], 'angles of columns %d..%d' % (k, k + 2))
    nr = len(ref.rew_class)
    allowed = np.zeros_like(ref.rew)
    for k, c in enumerate(ref.rew_class):
        d = np.abs(rew[:, k] - ref.rew[:, k])
        if c == 'exact':
            rep.note('exact', np.where(rew[:, k].astype(np.float32) == ref.rew[:, k].astype(np.float32), 0.0, np.inf), 'reward column %d' % k)
        elif c == 'reach':
            dist = np.abs(ref.rew[:, k]) / ref.rew_scale[k]
            allowed[:, k] = slack * ref.rew_scale[k] * tol['reach'] * np.maximum(1.0, dist) + F32_EPS * np.abs(ref.rew[:, k])
            rep.note('reach', d / allowed[:, k], 'reward column %d' % k)
        else:
            allowed[:, k] = slack * tol['elec'] * np.abs(ref.rew[:, k])
            rep.note('elec', np.where(ref.rew[:, k] == 0.0, np.where(rew[:, k] == 0.0, 0.0, np.inf), d / np.maximum(allowed[:, k], 1e-300)), 'reward column %d' % k)
    if nr:
        total = allowed[:, :nr].sum(axis=1) + nr * F32_EPS * np.abs(ref.rew[:, :nr]).sum(axis=1)
        d = np.abs(np.asarray(got['rew_sum'], dtype=np.float64) - ref.rew_sum)
        rep.note('rew_sum', np.where(d == 0.0, 0.0, d / np.maximum(total, 1e-300)), 'collapsed reward')
    nt = len(ref.term_class)
    near = near_threshold(ref, tol, slack)
    rep.near = near.any(axis=1)
    if nt:
        wrong = (np.asarray(got['term'])[:, :nt] != ref.term[:, :nt]) & ~near[:, :nt]
        rep.note('term', np.where(wrong, np.inf, 0.0), 'terminal bytes, columns %s' % np.nonzero(wrong.any(axis=0))[0].tolist())
    flag = np.asarray(got['term_flag']).astype(np.uint8)
    rep.note('term', np.where((flag != ref.term_flag) & ~rep.near, np.inf, 0.0), 'collapsed terminal flag')
    return rep


def outputs_of(sim, rows=None):
    """``got`` of a backend's output tensors (an oracle build's in its own precision)."""
    if hasattr(sim, 'obs64'):
        got = dict(obs=sim.obs64.copy(), rew=sim.rew64.copy(), term=sim.term8.copy(), rew_sum=sim.rsum64.copy(), term_flag=sim.tflag8.copy())
        return got if rows is None else {k: v[rows] for k, v in got.items()}
    f = lambda t: np.array(t.detach().cpu().numpy())
    got = dict(obs=f(sim.obs), rew=f(sim.rew), term=f(sim.term), rew_sum=f(sim.rew_sum), term_flag=f(sim.term_flag))
    return got if rows is None else {k: v[rows] for k, v in got.items()}


def f32_sum_in_order(rew, n):
    """The float32 sum of reward columns 0 .. n-1, left to right from 0: what the collapsed reward must equal bit for bit."""
    acc = np.zeros(rew.shape[0], dtype=np.float32)
    for k in range(n):
        acc = (acc + rew[:, k].astype(np.float32)).astype(np.float32)
    return acc
