"""Scenes and edge states of the output-op tests (tests/test_output_ops_ref.py on the CPU, tests/test_output_ops_gpu.py on the
kernels): one state row per env, written so that every observe / reward / terminal op is evaluated at its edges by ONE launch.

Scenes (tests/golden/output_ops/, variants by tree edit):
  generic      floating cart_tree + marble over a plane (step_kernel<L>); generic_all: the same under terminal_if_all (3 groups)
  joints       the 17-joint UR5 + three-finger gripper, joint_state_sensor subsets
  drone        examples/drone_pilot/drone_pilot.yaml: the addon-state observation and the natural fell_over
  arms         two UR5 + a floating marble under joint_controller (the four-wavefront kernel: helper wave, split sweeps); arms_ik:
               under ik_controller; pair_ik: under ik_controller without the marble -- the planner starts the dynamics early and
               splits the narrow phase (early_dyn, coll_split: the pose hand-over form) only where every moving body is a register
               chain, which a free body is not; one_arm: the right arm removed (arm and free body)

Ladders (env e takes entry e % 70, so a single env gets env 0's):
  gimbal    pitch = +-(pi/2 - d), d in DELTAS, random roll and yaw, half of the envs with -q; on a floating base and, by a joint
            angle, on a link frame (the cart's hinge_a with the base turned so that the link's pitch is the joint angle)
  qfrom_mat joint angles (and free base angles) drawn until an observed moving link's rotation lies clearly inside the wanted
            branch, cycling through the branches; rotations by exactly pi about x, y and z
  tilt      rotation angle max_tilt +- {10, 100} margins, 0 and pi, about random axes and about z (pure yaw), q and -q
  reach     distance tolerance +- {10, 100} margins, and 0
  timer     step counter max - 1, max, max + 1
  electricity  every sign combination of qd and applied effort of the first joint, zeros included
  limits    joints at both limits
A margin is the tolerance of the quantity (``LADDER_MARGIN``: between 1 and 1.5 x output_ops_ref.TOL): ladder envs sit 10 margins from every
threshold by construction, up to the rounding of the state to fp32.
"""
import os

import numpy as np

import base_state_ref as bs
import diy_gym_amd.examples  # noqa: F401  (registers propellor and fell_over)
import output_ops_ref as R
from diy_gym_amd import Configuration, DIYGym
from diy_gym_amd.scene import K
from dynamics_ref import joint_limits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'output_ops')
P = 70
DELTAS = (0.0, 1e-4, 1e-3, 3e-3, 4.3e-3, 4.7e-3, 1e-2, 0.1)
OFFSETS = (10.0, -10.0, 100.0, -100.0)
REST = [-0.17, -0.73, -1.93, -0.36, -0.03, -0.06]


def _all_groups(t):
    del t['terminal_if_any']
    t['terminal_if_all'] = True


def _ik(t):
    for m in ('ur5_l', 'ur5_r'):
        t[m]['controller'] = {'addon': 'ik_controller', 'end_effector': 'ee_fixed_joint', 'use_orientation': True, 'rest_position': list(REST)}


def _one_arm(t):
    for k in ('ur5_r', 'l_from_r', 'r_from_l', 'reach_a'):
        del t[k]
    t['reach_b']['source_model'] = 'ur5_l'


def _pair_ik(t):
    _ik(t)
    for k in ('marble', 'reach_b'):
        del t[k]


SCENES = {
    'generic': (os.path.join(GOLDEN, 'generic.yaml'), None), 'generic_all': (os.path.join(GOLDEN, 'generic.yaml'), _all_groups),
    'joints': (os.path.join(GOLDEN, 'joints.yaml'), None), 'drone': (os.path.join(ROOT, 'examples', 'drone_pilot', 'drone_pilot.yaml'), None),
    'arms': (os.path.join(GOLDEN, 'arms.yaml'), None), 'arms_ik': (os.path.join(GOLDEN, 'arms.yaml'), _ik), 'one_arm': (os.path.join(GOLDEN, 'arms.yaml'), _one_arm),
    'pair_ik': (os.path.join(GOLDEN, 'arms.yaml'), _pair_ik),
}


def make_env(scene, B, backend_factory=None, device=None, seed=5):
    path, edit = SCENES[scene]
    cfg = Configuration.from_file(path)
    if edit is not None:
        edit(cfg.node)
    kw = dict(backend_factory=backend_factory) if backend_factory is not None else dict(device=device)
    return DIYGym(cfg, num_envs=B, seed=seed, **kw)


def action_bounds(env):
    """(low, high) of the flat action row."""
    import torch
    from diy_gym_amd.utils import flatten, get_bounds_for_space
    return tuple(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, low)), dtype=torch.float32) for low in (True, False))


def seeded_actions(env, gen):
    """One row of uniform random actions per env from the torch generator ``gen``."""
    import torch
    lo, hi = action_bounds(env)
    return lo + (hi - lo) * torch.rand((env.num_envs, lo.numel()), generator=gen)


# ---- small rotation helpers ---------------------------------------------------------------------------------------------------
def quat_axis_angle(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    return np.append(axis / np.linalg.norm(axis) * np.sin(angle / 2.0), np.cos(angle / 2.0))


def quat_rpy(r, p, y):
    return R.matrix_quat(R.euler_matrix((r, p, y)))[0]


def random_axis(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def clear_branch(M, clear=0.05):
    """Branch of ``matrix_quat`` for M if every comparison deciding it has ``clear`` to spare (fp32 cannot flip it), else None."""
    tr, d = np.trace(M), np.diag(M)
    if tr > clear:
        return 0
    if tr > -clear:
        return None
    top = np.sort(d)
    return None if top[2] - top[1] < clear else 1 + int(np.argmax(d))


# ---- writing states --------------------------------------------------------------------------------------------------------------
class States:
    """[B, state_dim] float32 rows, begun as copies of the rows a reset leaves (targets, caches and addon state stay valid)."""
    def __init__(self, env, ref, B):
        self.env, self.ref, self.layout = env, ref, env.layout
        self.rows = np.array(np.asarray(env.sim.get_state(), dtype=np.float32)[np.arange(B) % env.num_envs])

    def base(self, name, e, pos=None, orn=None, lin=None, ang=None):
        """Reported (inertial-frame) pose and twist of the base of model ``name`` in env ``e``; what is None stays."""
        m, L = self.env.models[name], self.layout
        so, fixed = L.body_state_off[m.uid], L.body_fixed[m.uid]
        row = self.rows[e].astype(np.float64)
        cur = [a[0] for a in bs.report_from_stored(L, m.uid, row[so:so + 3], row[so + 3:so + 7], None if fixed else row[so + 7:so + 10], None if fixed else row[so + 10:so + 13])]
        pos, orn, lin, ang = (c if v is None else np.asarray(v, dtype=np.float64) for v, c in zip((pos, orn, lin, ang), cur))
        p, q, v, w = (a[0] for a in bs.stored_from_report(L, m.uid, pos, orn, lin, ang))
        self.rows[e, so:so + 7] = np.concatenate([p, q])
        if not fixed:
            self.rows[e, so + 7:so + 13] = np.concatenate([v, w])

    def joints(self, name, e, q=None, qd=None, applied=None):
        b = self.ref.bodies[name]
        for vals, col in ((q, K.LS_Q), (qd, K.LS_QD), (applied, K.LS_APPLIED)):
            if vals is not None:
                self.rows[e, [o + col for o in b.q_off]] = vals

    def step(self, e, n):
        self.rows[e, K.ST_STEP] = n

    def frame(self, name, e, fr, com):
        """fp64 frame of model ``name`` for the row as it stands (rounded to fp32, as every backend gets it)."""
        return self.ref.bodies[name].at(self.rows[e]).frame(fr, com)


def gimbal_entry(i, rng):
    """Entry i of 16: (roll, pitch, yaw, negate)."""
    pitch = (np.pi / 2 - DELTAS[i // 2]) * (1.0 if i % 2 == 0 else -1.0)
    return rng.uniform(-np.pi, np.pi), pitch, rng.uniform(-np.pi, np.pi), bool((i >> 2) & 1)


def tilt_entry(i, max_tilt, margin, rng):
    """Entry i of 20 of a tilt ladder: 16 around the threshold, then angle 0 (q, -q) and pi (q, -q); a quaternion."""
    if i < 16:
        q = quat_axis_angle(random_axis(rng) if (i // 4) % 2 == 0 else [0.0, 0.0, 1.0], max_tilt + OFFSETS[i % 4] * margin)
        return -q if i >= 8 else q
    q = quat_axis_angle(random_axis(rng), 0.0 if i < 18 else np.pi)
    return -q if i % 2 else q


def reach_distance(i, tolerance, margin):
    return 0.0 if i % 5 == 4 else tolerance + OFFSETS[i % 5] * margin


def motor_signs(i, rng, n):
    """qd and applied effort of n joints: random, the first joint's pair running through every sign combination and zero."""
    qd, ap = rng.uniform(-2.0, 2.0, n), rng.uniform(-20.0, 20.0, n)
    qd[0], ap[0] = abs(qd[0]) * (i % 3 - 1), abs(ap[0]) * ((i // 3) % 3 - 1)
    return qd, ap


def _limits_entry(i, lo, lim, q):
    """Envs lo .. lo+5: every joint at its lower (even) or upper (odd) limit."""
    return lim[:, (i - lo) % 2].copy() if lo <= i < lo + 6 else q


def _tilt_of(env, name):
    return env.models[name].addons['upright' if 'upright' in env.models[name].addons else 'fell_over'].max_tilt


def _draw_branch(rng, want, rotation_of, draw, tries=20000):
    for _ in range(tries):
        x = draw()
        if clear_branch(rotation_of(x)) == want:
            return x
    raise RuntimeError('no draw reached branch %d' % want)


# The margin the ladders are built with, per thresholded quantity (rad, m).  A constant at or a little above the quantity's
# tolerance, not the tolerance itself: the table is measured on these very states, and the stepped states go through contacts -- a
# ladder shifted by 1e-8 m gives another trajectory and other maxima, so with the exact tolerance table and states chase each other
# without settling.  tests/test_output_ops_ref.py asserts TOL <= LADDER_MARGIN <= 1.5 x TOL: a rung "10 margins" from a threshold
# is 10 to 15 tolerances from it.
LADDER_MARGIN = {'tilt': 1.2e-6, 'reach': 1.2e-6}


def edge_states(scene, env, ref, B, seed=0):
    """float32 [B, state_dim]: the edge states of ``scene`` (see the module docstring)."""
    rng = np.random.default_rng(seed)
    S = States(env, ref, B)
    tol = LADDER_MARGIN
    for e in range(B):
        i = e % P
        if env._max_episode_steps is not None:
            S.step(e, env._max_episode_steps + i % 3 - 1)
        if scene.startswith('generic'):
            _generic(S, e, i, rng, tol)
        elif scene == 'joints':
            lim = joint_limits(env.models['arm'].robot)
            q = _limits_entry(i, 10, lim, rng.uniform(lim[:, 0], lim[:, 1]))
            qd, ap = motor_signs(i, rng, len(q))
            S.joints('arm', e, q, qd, ap)
        elif scene == 'drone':
            _drone(S, e, i, rng, tol)
        else:
            _arms(S, e, i, rng, tol, scene)
    return S.rows


def _generic(S, e, i, rng, tol):
    env = S.env
    lim = joint_limits(env.models['cart'].robot)
    q = _limits_entry(i, 60, lim, rng.uniform(lim[:, 0], lim[:, 1]))
    qd, ap = motor_signs(i, rng, 3)
    origin_b = R.euler_matrix((0.0, 0.0, 0.5))   # hinge_b's origin rotation: arm_b turns by Rz(0.5) Rx(q[2]) in the base
    arm_b = lambda Rb, th: Rb @ origin_b @ R.euler_matrix((th, 0.0, 0.0))
    want = 1 + i % 3   # the non-trace branch arm_b's rotation is steered into where the ladder leaves angles free
    if i < 16:     # gimbal on the base; roll, yaw and hinge_b drawn until arm_b lies in the wanted branch
        _, pitch, _, neg = gimbal_entry(i, rng)
        r, y, th = _draw_branch(rng, want, lambda x: arm_b(R.euler_matrix((x[0], pitch, x[1])), x[2]),
                                lambda: (rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi), rng.uniform(lim[2, 0], lim[2, 1])))
        orn, q[2] = quat_rpy(r, pitch, y) * (-1.0 if neg else 1.0), th
    elif i < 32:   # gimbal on a link: base Rz(yaw) Rx(-0.3) undoes hinge_a's origin, so arm_a's (and the tip's) pitch is the joint angle
        _, pitch, yaw, neg = gimbal_entry(i - 16, rng)
        orn = R.matrix_quat(R.euler_matrix((0.0, 0.0, yaw)) @ R.euler_matrix((-0.3, 0.0, 0.0)))[0] * (-1.0 if neg else 1.0)
        q[1] = pitch
    elif i < 38:   # exactly pi about x, y, z: w = 0
        orn = np.zeros(4)
        orn[(i - 32) % 3] = 1.0 if i < 35 else -1.0
    elif i < 58:   # the cart's tilt ladder
        orn = tilt_entry(i - 38, _tilt_of(env, 'cart'), tol['tilt'], rng)
    else:          # a base orientation that puts arm_b into the wanted branch
        th = rng.uniform(lim[2, 0], lim[2, 1])
        Rt = _draw_branch(rng, want, lambda M: M, lambda: R.quat_matrix(quat_axis_angle(np.eye(3)[want - 1] + 0.3 * rng.normal(size=3), np.pi - rng.uniform(0.0, 0.6))))
        orn, q[2] = R.matrix_quat(Rt @ arm_b(np.eye(3), th).T)[0], th
    S.base('cart', e, pos=[rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(1.2, 1.8)], orn=orn, lin=rng.uniform(-1, 1, 3), ang=rng.uniform(-2, 2, 3))
    S.joints('cart', e, q, qd, ap)
    # the marble: its own tilt ladder (shifted against the cart's so that the groups fire in every combination), gimbal poses with
    # no angular velocity (they survive a step of free fall), then random
    m = (i + 35) % P
    if m < 20:
        orn, ang = tilt_entry(m, _tilt_of(env, 'marble'), tol['tilt'], rng), rng.uniform(-2, 2, 3)
    elif m < 36:
        r, p, y, neg = gimbal_entry(m - 20, rng)
        orn, ang = quat_rpy(r, p, y) * (-1.0 if neg else 1.0), np.zeros(3)
    else:
        orn, ang = quat_axis_angle(random_axis(rng), rng.uniform(0.0, 0.15 if m % 2 else np.pi)), rng.uniform(-2, 2, 3)
    near = env.addons['near']
    tip = S.frame('cart', e, near.source_frame_id, False)
    d = reach_distance(i, near.tolerance, tol['reach'])
    S.base('marble', e, pos=tip.p + random_axis(rng) * d, orn=orn, lin=rng.uniform(-1, 1, 3), ang=ang)


def _drone(S, e, i, rng, tol):
    env = S.env
    if i < 20:
        orn = tilt_entry(i, _tilt_of(env, 'drone'), tol['tilt'], rng)
    elif i < 36:
        r, p, y, neg = gimbal_entry(i - 20, rng)
        orn = quat_rpy(r, p, y) * (-1.0 if neg else 1.0)
    else:
        orn = quat_axis_angle(random_axis(rng), rng.uniform(0.0, 0.15 if i % 2 else np.pi))
    pos = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(1, 3)])
    S.base('drone', e, pos=pos, orn=orn, lin=rng.uniform(-1, 1, 3), ang=rng.uniform(-2, 2, 3))
    goal = env.addons['reach_goal']
    S.base('target', e, pos=S.frame('drone', e, -1, True).p + random_axis(rng) * reach_distance(i, goal.tolerance, tol['reach']),
           orn=quat_axis_angle(random_axis(rng), rng.uniform(0.0, np.pi)))
    for a in env.models['drone'].addons.values():   # rotor speeds
        if hasattr(a, 'obs_op'):
            S.rows[e, env.layout.addon_off + a.op.state_off] = rng.uniform(0.0, 1.0)


def _arms(S, e, i, rng, tol, scene):
    env = S.env
    arms = [n for n in ('ur5_l', 'ur5_r') if n in env.models]
    robot = env.models['ur5_l'].robot
    lim = joint_limits(robot)
    for n in arms:
        q = _limits_entry(i, 60, lim, rng.uniform(lim[:, 0], lim[:, 1]))
        if n == 'ur5_l' and not 60 <= i < 66:
            # joint angles until the rotation of the wrist_2 link (what l_from_r observes) lies clearly inside branch i % 4
            b = S.ref.bodies[n]
            fr = robot.joint_names.index('wrist_2_joint')

            def rot(x):
                S.joints(n, e, x)
                return b.at(S.rows[e]).T[robot.joints[fr].child].R
            q = _draw_branch(rng, i % 4, rot, lambda: rng.uniform(lim[:, 0], lim[:, 1]))
        qd, ap = motor_signs(i if n == 'ur5_l' else i // 9, rng, 6)
        S.joints(n, e, q, qd, ap * 5.0)
    if 'reach_a' in env.addons:   # the right arm's base is moved so that the two end effectors are a ladder distance apart
        a = env.addons['reach_a']
        src, tgt = S.frame(a.source_model.name, e, a.source_frame_id, False), S.frame(a.target_model.name, e, a.target_frame_id, False)
        d = reach_distance(i, a.tolerance, tol['reach'])
        base = S.frame(a.target_model.name, e, -1, True)
        S.base(a.target_model.name, e, pos=base.p + (src.p + random_axis(rng) * d - tgt.p))
    if 'marble' not in env.models:
        return
    m = (i + 35) % P
    if m < 20:
        orn, ang = tilt_entry(m, _tilt_of(env, 'marble'), tol['tilt'], rng), rng.uniform(-2, 2, 3)
    elif m < 36:
        r, p, y, neg = gimbal_entry(m - 20, rng)
        orn, ang = quat_rpy(r, p, y) * (-1.0 if neg else 1.0), np.zeros(3)
    elif m < 42:
        orn, ang = np.zeros(4), rng.uniform(-2, 2, 3)
        orn[(m - 36) % 3] = 1.0 if m < 39 else -1.0
    else:
        orn, ang = quat_axis_angle(random_axis(rng), rng.uniform(0.0, 0.15 if m % 2 else np.pi)), rng.uniform(-2, 2, 3)
    b = env.addons['reach_b']
    src = S.frame(b.source_model.name, e, b.source_frame_id, False)
    d = reach_distance(i // 5, b.tolerance, tol['reach'])
    S.base('marble', e, pos=src.p + random_axis(rng) * d, orn=orn, lin=rng.uniform(-1, 1, 3), ang=ang)
