"""Closed-form known-answer cases that run on ANY backend: the fp64 oracle, its fp32 build, or the HIP kernels.

tests/test_oracle_kat.py pins the oracle with closed forms, and the GPU suite pins the kernels to the oracle -- so a physics
error restated in both, or one that only shows in lane 63, in the partial tail wavefront or in one workspace mode, passes
both.  The cases here check the physics on whichever backend ``make_env`` binds, for B envs at once, each env with a parameter
of its own, so an indexing error is a wrong answer in particular envs.

A case is ``case(make_env, B) -> Result``: a dict ``{quantity: worst error over the B envs}`` (``.env[quantity]`` the env it
occurred in, ``.same`` per-env answers for comparing two batch sizes).  ``make_env(cfg_path_or_tree, B, **engine)`` builds the
DIYGym.  Cases use only what HipBackend and OracleBackend share (get_state, set_state, set_motor_cfg, motor_cfg, sim.step,
env.step, observe, frame_state, reset), and every expected value is a formula or a numpy fp64 recursion written in the case --
never the oracle.  The one exception is the normal force of case 2: the kernels report it through ``net_contact_forces``,
which the oracle does not have; there it is read from the oracle's last contact list (``_plane_normal_forces``).

Env e of a batch takes parameter ``e % 70`` of a fixed grid of 70 values: env 0 of a 70-env batch and the single env of a
1-env batch solve the same problem.

``TOL[case][quantity]``: 4 x max(error of the fp64 oracle, error of the fp32 oracle) at B = 70, rounded up to one significant
digit.  The fp64 error is how far the discrete model is from the formula, the fp32 error what rounding costs a correct
single-precision implementation of the same recursion; the factor 4 covers the kernels' own summation orders per mode and the
hardware sine, cosine and reciprocal.  tests/test_kat_ref.py asserts both oracle builds stay below TOL / 4, so the table cannot
be loosened without that test failing; tests/test_kat_gpu.py asserts the kernels stay below TOL.  Where the rule has nothing to
work with the table says what stands in for it: a quantity both builds get exactly right (error 0) takes 4 x one fp32 rounding
of the magnitude involved; the joint-limit excess keeps the 2e-3 of tests/test_oracle_kat.py; the two cases that add whole turns
to a joint angle report their errors in units of a per-env scale that grows with the fp32 spacing of the angle (``turn_scale``,
``FK_BASE``), whose constants follow the same 4 x rule.
"""
import copy
import os

import numpy as np
import torch

from diy_gym_amd import DIYGym
from diy_gym_amd.config import Configuration
from diy_gym_amd.mathx import Transform
from diy_gym_amd.scene import K
from diy_gym_amd.urdf import UrdfRobot
from nphelpers import link_frames, mass_matrix_and_gravity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
URDF = os.path.join(GOLDEN, 'urdf')
NODAMP = dict(linear_damping=0.0, angular_damping=0.0)
H = 1.0 / 480.0   # substep: fixedTimeStep 1/240, numSubSteps 2
GRAV = 9.81
P = 70            # size of every parameter grid


class Result(dict):
    """{quantity: worst error}; ``env``: {quantity: the env with that error}; ``same``: {quantity: per-env answers in
    the units of that quantity's error}, for comparing env 0 of two batch sizes; ``answers``: per-env figures worth printing."""
    def __init__(self):
        super().__init__()
        self.env, self.answers, self.same = {}, {}, {}

    def put(self, quantity, err):
        """``err``: one error per env (anything that broadcasts to [B, ...]; reduced over the trailing axes)."""
        err = np.abs(np.asarray(err, dtype=np.float64))
        err = np.where(np.isfinite(err), err, np.inf)   # a NaN is the worst answer, not one that passes every comparison
        err = err.reshape(err.shape[0], -1).max(axis=1)
        self[quantity], self.env[quantity] = float(err.max()), int(err.argmax())
        return self


def make_env_factory(backend_factory=None, device=None):
    """The ``make_env`` of a backend: ``backend_factory`` an OracleBackend (sub)class, or ``device`` for the HIP kernels."""
    def make_env(cfg, B, **engine):
        if isinstance(cfg, dict):
            cfg = Configuration.from_dict('kat', copy.deepcopy(cfg))
        elif not os.path.isabs(cfg):
            cfg = os.path.join(GOLDEN, cfg)
        kw = dict(backend_factory=backend_factory) if backend_factory is not None else dict(device=device)
        return DIYGym(cfg, num_envs=B, engine=engine or None, **kw)
    return make_env


def grid(lo, hi, B):
    """Env e's parameter: value ``e % 70`` of 70 evenly spaced ones in [lo, hi]."""
    return np.linspace(lo, hi, P)[np.arange(B) % P]


def link_q(env, body, dof):
    return env.layout.link_state_off[env.layout.body_first_link[body] + dof]


def state(env):
    return np.asarray(env.sim.get_state(), dtype=np.float64)


def frames(env, body, frame, com=False):
    return env.sim.frame_state(body, frame, com).detach().cpu().numpy().astype(np.float64)


def act(env, rows):
    return torch.as_tensor(np.asarray(rows, dtype=np.float32), device=env.sim.device)


def f32(x):
    """What a value becomes in the fp32 state of the kernels and of the fp32 oracle (expected values start from it)."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def quat_exp(rotvec):
    ang = np.linalg.norm(rotvec, axis=-1, keepdims=True)
    return np.concatenate([rotvec * np.sinc(ang / 2 / np.pi) / 2, np.cos(ang / 2)], axis=-1)


def quat_dist(a, b):
    """Distance of two unit quaternions xyzw up to sign (= half the rotation angle between them, for small angles)."""
    return np.minimum(np.abs(a - b).max(axis=-1), np.abs(a + b).max(axis=-1))


# ---------------------------------------------------------------------------------------------------------------- 1
def free_fall(make_env, B):
    """sphere2.urdf dropped without damping, 50 steps = k = 100 substeps of symplectic Euler: z = z0 - g h^2 k (k + 1) / 2,
    v = -g h k, x = x0 + v0 t, the spin stays (isotropic inertia) and turns the ball by exp(omega t)."""
    env = make_env({'render': False, 'hot_start': 0, 'ball': {'model': 'sphere2.urdf', 'xyz': [0.0, 0.0, 10.0]}}, B, **NODAMP)
    z0 = f32(grid(2.0, 12.0, B))
    e = np.arange(B) % P
    v0 = f32(np.stack([0.3 + 0.01 * e, -0.5 + 0.02 * e], axis=1))
    w0 = f32(np.stack([0.2 + 0.01 * e, -0.4 + 0.005 * e, 0.1 * (1 + e % 7)], axis=1))
    so = env.layout.body_state_off[0]
    st = state(env)
    st[:, so + 2] = z0
    st[:, so + K.BS_LINVEL:so + K.BS_LINVEL + 2] = v0
    st[:, so + K.BS_ANGVEL:so + K.BS_ANGVEL + 3] = w0
    env.sim.set_state(st)
    n = 50
    for _ in range(n):
        env.sim.step(0)
    st = state(env)
    k = 2 * n
    t = k * H
    r = Result()
    r.put('z', st[:, so + 2] - (z0 - GRAV * H * H * k * (k + 1) / 2))
    r.put('vz', st[:, so + K.BS_LINVEL + 2] - (-GRAV * H * k))
    r.put('xy', st[:, so:so + 2] - v0 * t)
    r.put('vxy', st[:, so + K.BS_LINVEL:so + K.BS_LINVEL + 2] - v0)
    r.put('spin', st[:, so + K.BS_ANGVEL:so + K.BS_ANGVEL + 3] - w0)
    r.put('orientation', quat_dist(st[:, so + K.BS_QUAT:so + K.BS_QUAT + 4], quat_exp(w0 * t)))
    assert np.all(st[:, K.ST_STEP] == n)
    r.same['z'] = st[:, so + 2]
    return r


# ---------------------------------------------------------------------------------------------------------------- 3
PEND_M, PEND_L, PEND_I = 1.0, 0.5, 1.0 * 0.5**2 + 1e-6   # tests/golden/urdf/pendulum.urdf: the bob's own 1e-6 kg m^2 added to m L^2


def _free_pendulum(make_env, B, q0, cfg='pendulum.yaml'):
    env = make_env(cfg, B, **NODAMP)
    mc = env.sim.motor_cfg(); mc[:, 2] = 0.0; env.sim.set_motor_cfg(mc)   # motor force 0: a free joint (pybullet idiom)
    qo = link_q(env, 0, 0)
    st = state(env); st[:, qo] = q0; st[:, qo + 1] = 0.0; env.sim.set_state(st)
    return env, qo


def pendulum_period(make_env, B):
    """A free pendulum released at amplitude a: period 2 pi sqrt(L / g) (1 + a^2 / 16) from the upward zero crossings of
    720 steps (three periods), and the energy of symplectic Euler oscillates without drifting."""
    a = f32(grid(0.02, 0.08, B))
    env, qo = _free_pendulum(make_env, B, a)
    qs, es = [], []
    for _ in range(720):
        env.sim.step(0)
        s = state(env)
        qs.append(s[:, qo]); es.append(0.5 * PEND_I * s[:, qo + 1]**2 + PEND_M * GRAV * PEND_L * (1 - np.cos(s[:, qo])))
    qs, es = np.array(qs), np.array(es)
    want = 2 * np.pi * np.sqrt(PEND_L / GRAV) * (1 + a * a / 16)
    period = np.full(B, np.nan)
    for b in range(B):
        q = qs[:, b]
        ups = np.nonzero((q[:-1] < 0) & (q[1:] >= 0))[0]
        if len(ups) >= 2:
            t = (ups + (-q[ups]) / (q[ups + 1] - q[ups])) / 240.0
            period[b] = np.mean(np.diff(t))
    r = Result()
    r.put('period_rel', (period - want) / want)
    r.put('energy_osc', (es.max(axis=0) - es.min(axis=0)) / es.max(axis=0))
    r.same['period_rel'] = period / want
    return r


# ---------------------------------------------------------------------------------------------------------------- 4
DP = dict(m1=1.5, m2=0.7, l1=0.4, l2=0.3)   # tests/golden/urdf/double_pendulum.urdf


def double_pendulum_acc(q1, q2, w1, w2, coriolis=1.0):
    """Joint accelerations of the planar double pendulum, Lagrangian closed form (absolute angles t, rates o)."""
    m1, m2, l1, l2, g = DP['m1'], DP['m2'], DP['l1'], DP['l2'], GRAV
    t1, t2, o1, o2 = q1, q1 + q2, w1, w1 + w2
    den = 2 * m1 + m2 - m2 * np.cos(2 * t1 - 2 * t2)
    a1 = (-g * (2 * m1 + m2) * np.sin(t1) - m2 * g * np.sin(t1 - 2 * t2) - coriolis * 2 * np.sin(t1 - t2) * m2 * (o2**2 * l2 + o1**2 * l1 * np.cos(t1 - t2))) / (l1 * den)
    a2 = (2 * np.sin(t1 - t2) * (coriolis * o1**2 * l1 * (m1 + m2) + g * (m1 + m2) * np.cos(t1) + coriolis * o2**2 * l2 * m2 * np.cos(t1 - t2))) / (l2 * den)
    return a1, a2 - a1


def double_pendulum(make_env, B):
    """Free double pendulum from (q1, q2, w1, w2) in [-1.5, 1.5]^4: after each of 60 steps the state is two substeps of
    ``w += h acc(q, w); q += h w`` with the Lagrangian closed form for acc (gravity, centrifugal and Coriolis terms)."""
    env = make_env('double_pendulum.yaml', B, **NODAMP)
    mc = env.sim.motor_cfg(); mc[:, 2] = 0.0; env.sim.set_motor_cfg(mc)
    x = f32(np.random.default_rng(3).uniform(-1.5, 1.5, (P, 4)))[np.arange(B) % P]
    q1, q2, w1, w2 = x.T.copy()
    o1, o2 = link_q(env, 0, 0), link_q(env, 0, 1)
    st = state(env)
    st[:, o1], st[:, o1 + 1], st[:, o2], st[:, o2 + 1] = q1, w1, q2, w2
    env.sim.set_state(st)
    worst = np.zeros(B)
    for _ in range(60):
        env.sim.step(0)
        for _ in range(2):
            a1, a2 = double_pendulum_acc(q1, q2, w1, w2)
            w1, w2 = w1 + H * a1, w2 + H * a2
            q1, q2 = q1 + H * w1, q2 + H * w2
        s = state(env)
        worst = np.maximum(worst, np.abs(np.stack([s[:, o1] - q1, s[:, o1 + 1] - w1, s[:, o2] - q2, s[:, o2 + 1] - w2])).max(axis=0))
    r = Result()
    r.put('state', worst)
    r.same['state'] = s[:, [o1, o1 + 1, o2, o2 + 1]]
    return r


# ---------------------------------------------------------------------------------------------------------------- 5
def velocity_motor_hold(make_env, B):
    """Every joint gets a velocity motor (target 0) at load: a pendulum released at q does not swing, and the effort the motor
    reports is the gravity torque m g L sin q it resists.  With max force 2.0 a motor that needs more reports exactly 2.0."""
    q0 = f32(grid(0.2, 1.4, B))
    env = make_env('pendulum.yaml', B, **NODAMP)
    qo = link_q(env, 0, 0)
    st = state(env); st[:, qo] = q0; env.sim.set_state(st)
    for _ in range(100):
        env.sim.step(0)
    s = state(env)
    r = Result()
    r.put('hold_q', s[:, qo] - q0)
    r.put('hold_qd', s[:, qo + 1])
    r.put('effort', np.abs(s[:, qo + K.LS_APPLIED]) - PEND_M * GRAV * PEND_L * np.sin(s[:, qo]))
    mc = env.sim.motor_cfg(); mc[:, 2] = 2.0; env.sim.set_motor_cfg(mc)
    env.sim.step(0)
    s2 = state(env)
    need = PEND_M * GRAV * PEND_L * np.sin(s[:, qo])
    assert B < P or ((need > 2.0).any() and (need < 2.0).any())   # both sides of the clamp are in the grid
    r.put('clamp', np.abs(s2[:, qo + K.LS_APPLIED]) - np.minimum(need, 2.0))
    r.same['effort'] = s[:, qo + K.LS_APPLIED]
    return r


# ---------------------------------------------------------------------------------------------------------------- 12
TURNS = np.array([0, 1, -1, 16, -16, 100, -100, 250, -250, 300, -300])
# per-env tolerance scale of the cases that add whole turns to a joint angle: BASE + C x spacing(fp32, |q|) x (substeps + 1).
# The stored angle is rounded to its fp32 spacing once when it is set and once per substep; a correct fp32 implementation
# cannot do better, and the constants are fixed on the fp32 oracle (tests/test_kat_ref.py).
def turn_scale(base, c, q, substeps):
    return base + c * np.spacing(np.abs(q).astype(np.float32)).astype(np.float64) * (substeps + 1)


def pendulum_whole_turns(make_env, B):
    """The free pendulum released at 0.7 rad + n whole turns, n up to +-300 (past the +-256 revolutions the hardware sine
    takes): (q, qd) and the bob's position after 60 steps against ``qd += h (-(m g L / I) sin q); q += h qd`` in fp64 from
    the fp32-rounded start angle.  Errors are reported in units of ``turn_scale``."""
    n = TURNS[np.arange(B) % len(TURNS)]
    q = f32(0.7 + 2 * np.pi * n)
    env, qo = _free_pendulum(make_env, B, q)
    q0 = q.copy()
    qd = np.zeros(B)
    steps = 60
    for _ in range(steps):
        env.sim.step(0)
    for _ in range(2 * steps):
        qd = qd + H * (-(PEND_M * GRAV * PEND_L / PEND_I) * np.sin(q))
        q = q + H * qd
    s = state(env)
    fr = frames(env, 0, env.models['pend'].get_frame_id('hinge'), com=True)
    bob = np.stack([-PEND_L * np.sin(q), np.zeros(B), 1.0 - PEND_L * np.cos(q)], axis=1)
    r = Result()
    r.put('q', np.abs(s[:, qo] - q) / turn_scale(WT_BASE['q'], WT_C['q'], q0, 2 * steps))
    r.put('qd', np.abs(s[:, qo + 1] - qd) / turn_scale(WT_BASE['qd'], WT_C['qd'], q0, 2 * steps))
    r.put('bob', np.abs(fr[:, :3] - bob) / turn_scale(WT_BASE['bob'], WT_C['bob'], q0, 2 * steps)[:, None])
    r.answers['raw'] = np.stack([np.abs(s[:, qo] - q), np.abs(s[:, qo + 1] - qd), np.abs(fr[:, :3] - bob).max(axis=1)], axis=1)
    r.answers['turns'] = n
    r.same['q'] = s[:, qo] / turn_scale(WT_BASE['q'], WT_C['q'], q0, 2 * steps)
    return r


# BASE: 4 x the error of the envs WITHOUT added turns, C: 4 x the largest error / (spacing x (substeps + 1)) of the others, both
# on the fp32 oracle (the fp64 one is exact to 1e-12 here, 3e-8 through the fp32 frame_state), rounded up to one digit.
# Measured fp32: n = 0: q 1.9e-7, qd 5.8e-7, bob 8.7e-8; ratios at most q 0.019 (n = 1), qd 0.029 (n = 16), bob 0.009 (n = 1).
WT_BASE = {'q': 8e-7, 'qd': 3e-6, 'bob': 4e-7}
WT_C = {'q': 0.08, 'qd': 0.12, 'bob': 0.04}


def npy(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- 6
def rolling_marble(make_env, B):
    """A constant horizontal force F through the centre of a sphere resting on a frictional plane: the contact's friction rows
    supply exactly the torque that keeps v = omega r, so v = F t / (m + I / r^2) (10 kg, I = 1, r = 0.5: F t / 14, far from
    the frictionless F t / 10), omega = v / r, and nothing moves sideways."""
    cfg = {'render': False, 'plane': {'model': 'grass/plane.urdf'},
           'ball': {'model': 'sphere2.urdf', 'xyz': [0.0, 0.0, 0.5],
                    'push': {'addon': 'external_force', 'xyz': [0.0, 0.0, 0.5]},   # the force acts at this WORLD point
                    'state': {'addon': 'object_state_sensor', 'include_rotation': True, 'include_velocity': True}}}
    env = make_env(cfg, B, **NODAMP)
    F = f32(grid(2.0, 12.0, B))
    zero = act(env, np.zeros((B, 3)))
    for _ in range(120):                       # settle
        env.step({'ball': {'push': zero}})
    push = act(env, np.stack([F, 0 * F, 0 * F], axis=1))
    steps = 60                                 # 0.25 s: the ball moves centimetres, the push point stays (almost) at its centre
    for _ in range(steps):
        o, _, _, _ = env.step({'ball': {'push': push}})
    v, w = npy(o['ball']['state']['velocity']), npy(o['ball']['state']['angular_velocity'])
    want = F * (steps / 240.0) / (10.0 + 1.0 / 0.25)
    r = Result()
    r.put('v_rel', (v[:, 0] - want) / want)
    r.put('omega_rel', (w[:, 1] - want / 0.5) / (want / 0.5))
    r.put('side', np.stack([v[:, 1], w[:, 0], w[:, 2]], axis=1))
    r.same['v_rel'] = v[:, 0] / want
    return r


# ---------------------------------------------------------------------------------------------------------------- 7
def inelastic_collision(make_env, B):
    """No gravity, no plane: a 10 kg sphere pushed with F for 24 steps (v0 = F 0.1 / 10) runs into an identical one at rest.
    The contact row removes the approach velocity and never pulls (restitution 0): afterwards v_a + v_b = v0, both v0 / 2,
    and b is never slower than a."""
    ball = lambda x, **kw: dict({'model': 'sphere2.urdf', 'xyz': [x, 0.0, 0.0], 'state': {'addon': 'object_state_sensor', 'include_velocity': True}}, **kw)
    cfg = {'render': False, 'gravity': [0.0, 0.0, 0.0], 'a': ball(-1.0, push={'addon': 'external_force', 'xyz': [-1.0, 0.0, 0.0]}), 'b': ball(0.6)}
    env = make_env(cfg, B, **NODAMP)
    F = f32(grid(60.0, 140.0, B))
    push, zero = act(env, np.stack([F, 0 * F, 0 * F], axis=1)), act(env, np.zeros((B, 3)))
    for _ in range(24):
        o, _, _, _ = env.step({'a': {'push': push}})
    v0 = F * 0.1 / 10.0
    r = Result()
    r.put('push_rel', (npy(o['a']['state']['velocity'])[:, 0] - v0) / v0)
    for _ in range(360):
        o, _, _, _ = env.step({'a': {'push': zero}})
    va, vb = npy(o['a']['state']['velocity'])[:, 0], npy(o['b']['state']['velocity'])[:, 0]
    assert np.all(vb > 0.25 * v0), 'the spheres of env %d never met' % int(np.argmin(vb / v0))
    r.put('momentum_rel', (va + vb - v0) / v0)
    r.put('common_rel', np.stack([va - v0 / 2, vb - v0 / 2], axis=1) / v0[:, None])
    r.put('approach_rel', np.maximum(va - vb, 0.0) / v0)
    r.same['common_rel'] = vb / v0
    return r


# ---------------------------------------------------------------------------------------------------------------- 9
def joint_limits(make_env, B):
    """cart_tree's pole joints carry limits: driven hard against them by the top of the action range for 300 steps, every
    limited joint stays within 2e-3 of its range (velocity-level limit row with ERP).  The envs differ by their respawn draws only."""
    from diy_gym_amd.utils import flatten, get_bounds_for_space
    env = make_env('cart_tree.yaml', B)
    robot = env.models['cart'].robot
    lim = [(j.q_index, j.lower, j.upper) for j in robot.joints if j.q_index > -1 and j.lower <= j.upper]
    assert lim, 'fixture has no limited joint'
    top = np.asarray(flatten(get_bounds_for_space(env.action_space, False)), dtype=np.float32)
    a = act(env, np.tile(top, (B, 1)))
    body = list(env.models).index('cart')
    worst = np.zeros(B)
    for i in range(300):
        env.sim.step(env._all_slots, a)
        if i % 10 == 9:
            st = state(env)
            for qi, lo, up in lim:
                q = st[:, link_q(env, body, qi)]
                worst = np.maximum(worst, np.maximum(np.maximum(lo - q, q - up), 0.0))
                worst = np.where(np.isfinite(q), worst, np.inf)
    r = Result()
    r.put('excess', worst)
    return r


# ---------------------------------------------------------------------------------------------------------------- 13
UR_REST = np.array([-0.17, -0.73, -1.93, -0.36, -0.03, -0.06])
UR_BASES = (([-0.55, 0.4, 0.0], -1.57), ([0.55, 0.4, 0.0], 1.57))   # examples/ur_high_5/ur_high_5_joint.yaml
UR_YAML = os.path.join(ROOT, 'examples', 'ur_high_5', 'ur_high_5_joint.yaml')


def ur5():
    return UrdfRobot(os.path.join(ROOT, 'diy_gym_amd', 'data', 'ur5', 'ur5_robot.urdf'))


def _ur_tree():
    import yaml
    tree = yaml.safe_load(open(UR_YAML))
    for arm in ('ur5_l', 'ur5_r'):
        tree[arm]['model'] = os.path.join(ROOT, 'diy_gym_amd', 'data', 'ur5', 'ur5_robot.urdf')
        tree[arm]['joint_state']['include_effort'] = True
    return tree


def arms_hold_against_gravity(make_env, B):
    """Two UR5s under position motors, each env holding a target of its own (rest + U(-0.3, 0.3)^12) for 480 steps: the arms
    settle on the target, and the effort every motor reports -- in the state and through joint_state_sensor -- is the gravity
    torque -G(q) of the arm at its own base transform, from the URDF tree in numpy."""
    env = make_env(_ur_tree(), B)
    target = f32(np.tile(UR_REST, 2) + np.random.default_rng(1).uniform(-0.3, 0.3, (P, 12)))[np.arange(B) % P]
    a = act(env, target)
    for _ in range(480):
        env.sim.step(env._all_slots, a)
    st = state(env)
    obs = env.observe()
    robot = ur5()
    r = Result()
    e_state, e_obs, dq, qd = [np.zeros((B, 12)) for _ in range(4)]
    for b, (xyz, yaw) in enumerate(UR_BASES):
        Tb = Transform.from_xyz_rpy(xyz, [0, 0, yaw])
        off = [link_q(env, b, i) for i in range(6)]
        q = st[:, off]
        eff = npy(obs[('ur5_l', 'ur5_r')[b]]['joint_state']['effort'])
        for e in range(B):
            _, Gv = mass_matrix_and_gravity(robot, q[e], T_base=Tb)
            e_state[e, 6 * b:6 * b + 6] = st[e, [o + K.LS_APPLIED for o in off]] + Gv
            e_obs[e, 6 * b:6 * b + 6] = eff[e] + Gv
        dq[:, 6 * b:6 * b + 6] = q - target[:, 6 * b:6 * b + 6]
        qd[:, 6 * b:6 * b + 6] = st[:, [o + 1 for o in off]]
    r.put('effort', e_state)
    r.put('effort_sensor', e_obs)
    r.put('q_target', dq)
    r.put('qd', qd)
    r.same['effort'] = st[:, [link_q(env, 0, i) + K.LS_APPLIED for i in range(6)]]
    return r


# ---------------------------------------------------------------------------------------------------------------- 14
FK_TURNS = np.array([0, 16, -16, 250, -250])


def arm_end_effector_pose(make_env, B):
    """The UR5's end-effector frame through ``frame_state`` right after ``set_state``: q in [-2, 2]^6 per env, four envs in five
    with whole turns (+-16, +-250) added to the shoulder-lift joint, against the URDF tree chained in numpy.  The tolerance of
    an env grows by ONE fp32 spacing of its largest stored angle, times the lever of the end effector about that joint (half
    of it on the quaternion): an implementation may not disturb an angle by more than the format resolves."""
    env = make_env(_ur_tree(), B)
    e = np.arange(B) % P
    n = FK_TURNS[e % len(FK_TURNS)]
    q = np.random.default_rng(14).uniform(-2.0, 2.0, (P, 6))[e]
    q[:, 1] += 2 * np.pi * n
    q = f32(q)
    st = state(env)
    for b in range(2):
        for i in range(6):
            st[:, link_q(env, b, i)] = q[:, i]; st[:, link_q(env, b, i) + 1] = 0.0
    env.sim.set_state(st)
    robot = ur5()
    r = Result()
    pos, rot = np.zeros((B, 2)), np.zeros((B, 2))
    for b, (xyz, yaw) in enumerate(UR_BASES):
        fr = frames(env, b, env.models[('ur5_l', 'ur5_r')[b]].get_frame_id('ee_fixed_joint'))
        Tb = Transform.from_xyz_rpy(xyz, [0, 0, yaw])
        for k in range(B):
            T, joints = link_frames(robot, q[k], Tb)
            lever = np.linalg.norm(np.cross(joints[1][2], T['ee_link'].p - joints[1][1]))
            ulp = float(np.spacing(np.float32(np.abs(q[k, 1]))))
            pos[k, b] = np.abs(fr[k, :3] - T['ee_link'].p).max() / (FK_BASE['pos'] + ulp * lever)
            rot[k, b] = quat_dist(fr[k, 3:7], np.asarray(T['ee_link'].quat)) / (FK_BASE['rot'] + 0.5 * ulp)
    r.put('pos', pos)
    r.put('rot', rot)
    r.same['pos'] = fr[:, :3] / (FK_BASE['pos'] + float(np.spacing(np.float32(np.abs(q[0, 1])))))
    return r


# 4 x the error of the two oracle builds (both report through the fp32 frame_state): pos 4.6e-8 / 1.3e-7 m, rot 2.8e-8 / 8.5e-8
FK_BASE = {'pos': 6e-7, 'rot': 4e-7}


# ---------------------------------------------------------------------------------------------------------------- 2
def _plane_normal_forces(env, marbles, plane):
    """[B, n] normal force the plane exerts on each marble after the last step.  The kernels report it through
    ``net_contact_forces``; the oracle keeps the contact list of its last substep (normal impulse / h), which is all it has."""
    sim = env.sim
    if hasattr(sim, 'net_contact_forces'):
        return np.stack([npy(sim.net_contact_forces(m, None, body_b=plane, want=('force', ))[0])[:, 0, 2] for m in marbles], axis=1)
    st = state(env)
    out = np.full((sim.num_envs, len(marbles)), np.nan)
    for e in range(sim.num_envs):
        for k in range(sim.contacts(e)):
            c = sim.contact(e, k)
            if abs(c[5]) > 0.9:   # the plane's normal; the two marbles that touch each other meet along x
                xy = np.array([st[e, [env.layout.body_state_off[m], env.layout.body_state_off[m] + 1]] for m in marbles])
                out[e, int(np.argmin(np.linalg.norm(xy - c[:2], axis=1)))] = c[7] / H
    return out


def marbles_at_rest(make_env, B):
    """Three 10 kg marbles on the plane for 240 steps: each rests at z = r = 0.5, nothing moves, the plane carries each with
    m g, and B identical envs give one answer."""
    env = make_env('basic_env_nocam.yaml', B)
    for _ in range(240):
        env.sim.step(0)
    st = state(env)
    marbles = [env.models[n].uid for n in ('red_marble', 'green_marble', 'blue_marble')]
    so = [env.layout.body_state_off[m] for m in marbles]
    r = Result()
    r.put('z', np.stack([st[:, o + 2] - 0.5 for o in so], axis=1))
    r.put('velocity', np.stack([st[:, o + K.BS_LINVEL:o + K.BS_LINVEL + 6] for o in so], axis=1))
    N = _plane_normal_forces(env, marbles, env.models['plane'].uid)
    r.put('normal_force_rel', (N - 10.0 * GRAV) / (10.0 * GRAV))
    phys = np.concatenate([st[:, o:o + 13] for o in so], axis=1)
    r.put('spread', phys - phys[:1])
    r.same['z'] = st[:, so[0] + 2]
    return r


# ---------------------------------------------------------------------------------------------------------------- 8
def fixed_constraint_pair(make_env, B):
    """``attach: constraint`` (six solver rows), no gravity: a 10 kg sphere carries a second one on a 0.5 m offset.  Pushed with F
    for 24 steps through the pair's common centre of mass both end up at F t / (m_a + m_b), without spin, the offset kept;
    pushed through the parent's own centre the pair also turns: angular momentum about the common centre = lever x impulse,
    with the pair's inertia 2 I + 2 m (d / 2)^2, and the child stays 0.5 m from the parent."""
    F = f32(grid(60.0, 140.0, B))
    v = F * 0.1 / 20.0
    r = Result()

    def run(push_at):
        cfg = {'render': False, 'gravity': [0.0, 0.0, 0.0],
               'a': {'model': 'sphere2.urdf', 'xyz': [0.0, 0.0, 0.0], 'push': {'addon': 'external_force', 'xyz': push_at},
                     'b': {'model': 'sphere2.urdf', 'attach': 'constraint', 'xyz': [0.0, 0.5, 0.0], 'constraint_max_force': 1e5}}}
        env = make_env(cfg, B, **NODAMP)
        assert env.layout.n_bodies == 2
        push, zero = act(env, np.stack([F, 0 * F, 0 * F], axis=1)), act(env, np.zeros((B, 3)))
        for _ in range(24):
            env.step({'a': {'push': push}})
        for _ in range(60):
            env.step({'a': {'push': zero}})
        return frames(env, env.models['a'].uid, -1, com=True), frames(env, env.models['a'].models['b'].uid, -1, com=True)

    a, b = run([0.0, 0.25, 0.0])           # through the common centre of mass
    r.put('straight_v_rel', np.stack([a[:, 7] - v, b[:, 7] - v], axis=1) / v[:, None])
    r.put('straight_spin', np.concatenate([a[:, 10:13], b[:, 10:13]], axis=1))
    r.put('straight_offset', b[:, :3] - a[:, :3] - np.array([0.0, 0.5, 0.0]))
    r.same['straight_v_rel'] = a[:, 7] / v
    a, b = run([0.0, 0.0, 0.0])            # through the parent's centre: 0.25 m beside the common one
    I_pair = 2 * 1.0 + 2 * 10.0 * 0.25**2   # sphere2.urdf: izz = 1
    wz = 0.25 * F * 0.1 / I_pair
    r.put('turning_v_rel', (np.linalg.norm(0.5 * (a[:, 7:10] + b[:, 7:10]), axis=1) - v) / v)   # linear momentum / 20 kg
    r.put('turning_length', np.linalg.norm(b[:, :3] - a[:, :3], axis=1) - 0.5)
    r.put('turning_spin_rel', np.stack([np.abs(a[:, 12]) - wz, np.abs(b[:, 12]) - wz], axis=1) / wz[:, None])
    return r


# ---------------------------------------------------------------------------------------------------------------- 10
def drone_thrust(make_env, B):
    """drone_pilot's 8 kg quadrotor released at z = 0.5 with all four rotors commanded to one level per env.  A rotor spools up
    by a tenth of what is missing per step, so the thrust during step n is 80 N x level x (1 - 0.9^n).  Envs whose closed-form
    trajectory never comes near the ground follow it: ``v += h (T_n / m - g); z += h v`` per substep.  Envs with
    80 N x level <= m g come down and stay down: no vertical speed at the end, all at one height.  (The envs in between land and
    take off again; they are not judged.)"""
    import diy_gym_amd.examples  # noqa: F401  (registers propellor and fell_over)
    env = make_env(os.path.join(ROOT, 'examples', 'drone_pilot', 'drone_pilot.yaml'), B, **NODAMP)
    level = f32(grid(0.9, 1.2, B))
    if B < P:   # one of each kind at the head of the grid, so that a small batch judges both
        level[:2] = f32([0.9, 1.2])[:B]
    a = act(env, np.repeat(level[:, None], 4, axis=1))
    so = env.layout.body_state_off[env.models['drone'].uid]
    m, steps = 8.0, 300
    st = state(env)   # (the reset's hot start has already let it fall for one step, rotors still)
    z, v = st[:, so + 2], st[:, so + K.BS_LINVEL + 2]
    assert np.all(np.abs(z - 0.5) < 1e-3) and np.all(np.abs(v) < 0.1)
    zs, vs, lowest = [], [], z.copy()
    for n in range(1, steps + 1):
        env.sim.step(env._all_slots, a)
        for _ in range(2):
            v = v + H * (80.0 * level * (1 - 0.9**n) / m - GRAV)
            z = z + H * v
        lowest = np.minimum(lowest, z)
        if n % 50 == 0:
            st = state(env)
            zs.append(st[:, so + 2] - z); vs.append(st[:, so + K.BS_LINVEL + 2] - v)
    flying, grounded = lowest > 0.3, 80.0 * level <= m * GRAV   # (the hull touches the plane at z = 0.20)
    assert B < P or (flying.sum() >= 10 and grounded.sum() >= 10), (flying.sum(), grounded.sum())
    r = Result()
    r.put('flying_z', np.where(flying[:, None], np.array(zs).T, 0.0))
    r.put('flying_vz', np.where(flying[:, None], np.array(vs).T, 0.0))
    r.put('flying_drift', np.where(flying[:, None], np.concatenate([st[:, so:so + 2], st[:, so + K.BS_LINVEL:so + K.BS_LINVEL + 2], st[:, so + K.BS_ANGVEL:so + K.BS_ANGVEL + 3]], axis=1), 0.0))
    r.put('grounded_vz', np.where(grounded, st[:, so + K.BS_LINVEL + 2], 0.0))
    zg = st[:, so + 2]
    r.put('grounded_z', np.where(grounded, zg - (np.median(zg[grounded]) if grounded.any() else 0.0), 0.0))
    assert not grounded.any() or 0.15 < np.median(zg[grounded]) < 0.25
    r.same['flying_z'] = np.where(flying, st[:, so + 2], 0.0)
    return r


# ---------------------------------------------------------------------------------------------------------------- 11
def _pendulum_tool(make_env, B, extra=None):
    """tests/golden/urdf/pendulum_tool.urdf: rod 1 kg at 0.5 m (0.02 kg m^2), tool 0.3 kg at 1.1 m (0.001 kg m^2) behind a fixed joint."""
    cfg = dict(extra or {})
    cfg.update({'render': False, 'pend': {'model': os.path.join(URDF, 'pendulum_tool.urdf'), 'xyz': [0, 0, 0],
                                            'wrist': {'addon': 'force_torque_sensor', 'frame': 'mount'},
                                            'shoulder': {'addon': 'force_torque_sensor', 'frame': 'hinge'}}})
    env = make_env(cfg, B, **NODAMP)
    return env, env.models['pend'].uid


def _to_link(q, v):
    """World vectors [B, 3] in the axes of a link turned by q about y."""
    c, s = np.cos(q), np.sin(q)
    return np.stack([c * v[:, 0] - s * v[:, 2], v[:, 1], s * v[:, 0] + c * v[:, 2]], axis=1)


def _to_world(q, v):
    return _to_link(-q, v)


def force_torque_sensor(make_env, B):
    """The joint force-torque sensors of a two-part pendulum against Newton-Euler in closed form: held still by a strong motor
    (the weight at the right lever arm), swinging freely for 60 steps (inertial and centripetal terms), and leaning on a prop
    with its tool (the wrist carries the tool's weight minus the support)."""
    g = GRAV
    r = Result()
    # -- static hold at an angle per env
    q0 = f32(grid(0.3, 1.3, B))
    env, body = _pendulum_tool(make_env, B)
    qo = link_q(env, body, 0)
    st = state(env); st[:, qo] = q0; env.sim.set_state(st)
    mc = env.sim.motor_cfg(); mc[:, 2] = 1e4; env.sim.set_motor_cfg(mc)
    for _ in range(30):
        env.sim.step(0)
    obs = env.observe()['pend']
    s = state(env)
    q = s[:, qo]
    up = np.tile([0.0, 0.0, 1.0], (B, 1))
    r.put('hold_wrist_force', npy(obs['wrist']['force']) - _to_link(q, 0.3 * g * up))
    r.put('hold_wrist_torque', npy(obs['wrist']['torque']))
    r.put('hold_shoulder_force', npy(obs['shoulder']['force']) - _to_link(q, 1.3 * g * up))
    r.put('hold_shoulder_torque', npy(obs['shoulder']['torque']) - np.stack([0 * q, 0.6 * np.sin(q) * 0.3 * g, 0 * q], axis=1))
    r.put('hold_effort', np.abs(s[:, qo + K.LS_APPLIED]) - (0.5 * 1.0 + 1.1 * 0.3) * g * np.sin(q))
    r.same['hold_shoulder_force'] = npy(obs['shoulder']['force'])
    # -- free swing from an angle per env
    q0 = f32(grid(0.8, 1.4, B))
    env, body = _pendulum_tool(make_env, B)
    qo = link_q(env, body, 0)
    st = state(env); st[:, qo] = q0; env.sim.set_state(st)
    mc = env.sim.motor_cfg(); mc[:, 2] = 0.0; env.sim.set_motor_cfg(mc)
    for _ in range(60):
        env.sim.step(0)
    obs = env.observe(_refresh=False)['pend']
    s = state(env)
    q, qd = s[:, qo], s[:, qo + 1]
    I_h = (0.02 + 1.0 * 0.5**2) + (0.001 + 0.3 * 1.1**2)
    qdd = -(1.0 * 0.5 + 0.3 * 1.1) * g * np.sin(q) / I_h

    def part(m, L):   # the force that moves a point mass on the rod at distance L, minus gravity (world x, z)
        t = np.stack([-np.cos(q), 0 * q, np.sin(q)], axis=1) * L   # d(position)/dq for position = (-L sin q, 0, 1 - L cos q)
        n = np.stack([np.sin(q), 0 * q, np.cos(q)], axis=1) * L    # centripetal direction
        return m * (t * qdd[:, None] + n * (qd * qd)[:, None] + g * up)
    Fw = part(1.0, 0.5) + part(0.3, 1.1)
    scale = np.linalg.norm(Fw, axis=1)[:, None]
    r.put('swing_shoulder_rel', (npy(obs['shoulder']['force']) - _to_link(q, Fw)) / scale)
    r.put('swing_wrist_rel', (npy(obs['wrist']['force']) - _to_link(q, part(0.3, 1.1))) / scale)
    # -- leaning on the prop's top face with the tool sphere, motor off
    q0 = f32(grid(0.93, 0.97, B))
    env, body = _pendulum_tool(make_env, B, extra={'prop': {'model': os.path.join(URDF, 'ft_prop.urdf'), 'use_fixed_base': True, 'xyz': [-0.7, 0, 0.0]}})
    qo = link_q(env, body, 0)
    st = state(env); st[:, qo] = q0; env.sim.set_state(st)
    mc = env.sim.motor_cfg(); mc[:, 2] = 0.0; env.sim.set_motor_cfg(mc)
    for _ in range(400):
        env.sim.step(0)
    s = state(env)
    q, qd = s[:, qo], s[:, qo + 1]
    obs = env.observe(_refresh=False)['pend']
    # moment balance about the hinge: N x_contact = (m_rod x_rod + m_tool x_tool) g with a vertical support force
    x_rod, x_tool = 0.5 * np.sin(q), 1.1 * np.sin(q)
    N = (1.0 * x_rod + 0.3 * x_tool) * g / x_tool
    Fwr, Fsh = _to_world(q, npy(obs['wrist']['force'])), _to_world(q, npy(obs['shoulder']['force']))
    r.put('lean_qd', qd)
    r.put('lean_wrist_rel', np.stack([Fwr[:, 2] - (0.3 * g - N), Fwr[:, 0]], axis=1) / N[:, None])
    r.put('lean_shoulder_rel', (Fsh[:, 2] - (1.3 * g - N)) / N)
    return r


CASES = {   # numbered 1 .. 14 in the section comments above
    'free_fall': free_fall,
    'marbles_at_rest': marbles_at_rest,
    'pendulum_period': pendulum_period,
    'double_pendulum': double_pendulum,
    'velocity_motor_hold': velocity_motor_hold,
    'rolling_marble': rolling_marble,
    'inelastic_collision': inelastic_collision,
    'fixed_constraint_pair': fixed_constraint_pair,
    'joint_limits': joint_limits,
    'drone_thrust': drone_thrust,
    'force_torque_sensor': force_torque_sensor,
    'pendulum_whole_turns': pendulum_whole_turns,
    'arms_hold_against_gravity': arms_hold_against_gravity,
    'arm_end_effector_pose': arm_end_effector_pose,
}

# quantity: tolerance   # measured fp64 oracle / fp32 oracle at B = 70; tolerance = 4 x the larger, rounded up to one digit
TOL = {
    'free_fall': {
        'z': 3e-6,             # 3.6e-15 / 6.5e-7
        'vz': 6e-6,            # 4.4e-15 / 1.4e-6
        'xy': 1e-6,            # 3.6e-16 / 2.5e-7
        'vxy': 2e-8,           # 1.9e-17 / 2.9e-9
        'spin': 2e-7,          # 6.3e-17 / 3.0e-8
        'orientation': 4e-7,   # 1.9e-16 / 9.3e-8
    },
    'marbles_at_rest': {
        'z': 5e-5,                  # 1.0e-5 / 1.0e-5: the contact's resting depth, not rounding
        'velocity': 3e-6,           # 2.0e-14 / 5.2e-7: determined only to the sweeps' residual threshold
        'normal_force_rel': 3e-7,   # 9.9e-12 / 6.7e-8
        'spread': 3e-7,             # 0 / 0: identical envs.  One fp32 rounding of the largest coordinate (1 m), x 4
    },
    'fixed_constraint_pair': {
        'straight_v_rel': 3e-6,     # 5.3e-8 / 7.0e-7
        'straight_spin': 8e-7,      # 6.5e-16 / 1.9e-7
        'straight_offset': 6e-8,    # 0 / 1.49e-8
        'turning_v_rel': 4e-6,      # 4.8e-8 / 8.5e-7
        'turning_length': 7e-5,     # 1.59e-5 / 1.59e-5: the ERP of the constraint rows, not rounding
        'turning_spin_rel': 3e-4,   # 5.84e-5 / 5.88e-5: the lever turns with the pair during the push
    },
    'drone_thrust': {
        'flying_z': 2e-5,           # 2.2e-15 / 4.4e-6
        'flying_vz': 6e-5,          # 3.3e-15 / 1.3e-5
        'flying_drift': 3e-7,       # 0 / 0: the rotors' torques and levers cancel.  One fp32 rounding of a unit quantity, x 4
        'grounded_vz': 9e-4,        # 9.4e-5 / 2.2e-4: a resting contact's velocity is determined to the residual threshold
        'grounded_z': 2e-4,         # 3.8e-5 / 4.6e-5
    },
    'force_torque_sensor': {
        'hold_wrist_force': 3e-6,       # 1.2e-7 / 5.7e-7 N
        'hold_wrist_torque': 4e-9,      # 1.7e-18 / 8.9e-10 N m
        'hold_shoulder_force': 7e-6,    # 4.8e-7 / 1.66e-6 N
        'hold_shoulder_torque': 2e-6,   # 5.9e-8 / 4.4e-7 N m
        'hold_effort': 6e-6,            # 1.8e-15 / 1.27e-6 N m
        'swing_shoulder_rel': 2e-2,     # 2.84e-3 / 2.84e-3: accelerations over one substep against the formula at its end
        'swing_wrist_rel': 5e-3,        # 1.13e-3 / 1.13e-3
        'lean_qd': 8e-9,                # 3.5e-18 / 1.9e-9 rad/s
        'lean_wrist_rel': 0.08,         # 1.90e-2 / 1.84e-2: the support is not quite vertical (contact depth, friction)
        'lean_shoulder_rel': 0.07,      # 1.68e-2 / 1.63e-2
    },
    'pendulum_period': {
        'period_rel': 7e-6,   # 1.56e-6 / 1.69e-6: the discretisation, not rounding
        'energy_osc': 0.04,    # 9.19e-3 / 9.19e-3: the oscillation of symplectic Euler, ~ h omega
    },
    'double_pendulum': {'state': 2e-5},   # 2.1e-7 / 4.8e-6 (|w| reaches 12 rad/s)
    'velocity_motor_hold': {
        # 0 / 0 on both builds: the motor row cancels the gravity kick of a substep, h (g / L) sin q <= 0.041 rad/s, exactly.  A
        # correct fp32 implementation may leave one rounding of that kick, 0.041 x 6e-8 = 2.4e-9 rad/s, which never moves q
        # (h x 2.4e-9 is far below the spacing 1.2e-7 of q); x 4 as everywhere: 1e-8 rad/s, and one spacing x 4 on q.
        'hold_q': 5e-7,
        'hold_qd': 1e-8,
        'effort': 4e-6,        # 8.9e-16 / 8.2e-7
        'clamp': 7e-7,         # 0 / 1.6e-7
    },
    # errors in units of turn_scale (constants above, fixed so that the fp32 oracle stays below 1/4)
    'pendulum_whole_turns': {'q': 1.0, 'qd': 1.0, 'bob': 1.0},
    'rolling_marble': {
        'v_rel': 7e-5,         # 1.43e-5 / 1.58e-5: the push point stays behind the rolling centre, not rounding
        'omega_rel': 2e-4,     # 2.43e-5 / 2.57e-5
        # 0 / 0: nothing pushes sideways.  One fp32 rounding of the largest rate involved (omega = 0.43 rad/s), x 4
        'side': 1e-7,
    },
    'inelastic_collision': {
        'push_rel': 3e-6,      # 5.3e-8 / 7.2e-7
        'momentum_rel': 3e-6,  # 5.3e-8 / 7.2e-7
        'common_rel': 4e-5,    # 2.6e-8 / 8.5e-6: the sweep leaves at the residual threshold
        'approach_rel': 3e-7,  # 0 / 0: one fp32 rounding of v0, x 4
    },
    'joint_limits': {'excess': 2e-3},     # 2.4e-6 / 2.4e-6; the bound is the solver's slop, as tests/test_oracle_kat.py has it
    'arms_hold_against_gravity': {
        'effort': 6e-4,        # 1.27e-4 / 1.12e-4 N m: the slowest env is still settling (|qd| 4e-6 rad/s on the fp64 build)
        'effort_sensor': 6e-4, # 1.29e-4 / 1.12e-4
        'q_target': 2e-5,      # 2.5e-7 / 3.8e-6
        'qd': 3e-4,            # 3.7e-6 / 5.5e-5
    },
    # errors in units of FK_BASE + one fp32 spacing of the turned angle x lever
    'arm_end_effector_pose': {'pos': 1.0, 'rot': 1.0},
}
