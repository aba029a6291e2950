"""env.sim.calculate_forward_dynamics and env.sim.rollout_joint_dynamics (dg_world_forward_dynamics / forward_dynamics_kernel,
dg_world_rollout / rollout_kernel) on the GPU against the fp64 reference of tests/fd_ref.py (itself pinned by tests/test_fd_ref.py).

Scenes, as tests/test_task_space_gpu.py: a pendulum, a double pendulum, the branching cart bolted down (prismatic joint, two
branches), a UR5 (also with DG_MAX_LANES 4 and 1, which put it in the global-workspace mode, Lane<0>), the UR5s whose link masses
a dynamics_randomizer scales per env, and the twelve-joint UR5 + gripper tree in its one-env-per-wavefront mode.  Batches of 1, 3
and 70 envs.  Per-env q in [-pi, pi] and inside the joint limits, qd in [-2, 2], tau in [-3, 3]; the rollouts' torques are those of
accelerations in [-3, 3] at the start state (inverse dynamics in fp64, rounded to fp32).  Rollouts (K, T) of (1, 1), (5, 8) and
(50, 2) at dt = the scene's substep: with B = 3 and K = 50 the 150 items straddle wavefronts and leave a ragged tail;
with B = 70, K = 5 and DG_MAX_LANES 4 the grid cap of the global-workspace mode (two workgroups for 350 items) makes every lane
stride through the item list several times (test_the_capped_grid_of_the_global_workspace_mode_strides).

Error measures.  qdd: per env, max |gpu - reference| divided by that env's largest |reference| entry and by the fp64 cond(M); no
env is left out (M is always SPD) and singular == 0 everywhere.  The round trip on the kernels themselves,
calculate_forward_dynamics(q, qd, calculate_inverse_dynamics(q, qd, a)) against a, is measured the same way.  Rollout q, qd, pos:
per item (env, sample), max |gpu - reference| over the trajectory divided by the largest |reference| entry of that trajectory.
The figure of a case is the largest over its envs / items.  The bounds are 8 x the largest figure measured over all cases of this
file on an MI355X, in two groups as in the task-space file ('short': pendulum, double pendulum, cart; 'arms': the six-axis arms
and the gripper tree); DESIGN.md "Forward dynamics and rollouts" has the table.  The margin is for other draws and batches and a
compiler that contracts multiply-adds differently, not for bugs.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import dynamics_ref as D
import fd_ref as FD
from diy_gym_amd import DIYGym
from diy_gym_amd.backend import JointRollout
from diy_gym_amd.scene import K as KC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda:0'
# measured maxima (MI355X, all cases of this file) and the bounds 8 x them.  'step': the rollout against env.step on ur_admittance
# (test_the_rollout_follows_the_real_step): 'step_ref' is the rollout's error against fp64 at that T (K = 1, T = 10), in radians;
# 'step_diff' the measured difference between the two, recorded, not a bound.
MEASURED = {
    # qdd, round_trip: ur_admittance x70, ur_randomized x70; q, pos: ur_admittance x70 K=5 T=8 (every mode the same figures); qd: ur5_gripper x3 K=5 T=8
    'arms': {'qdd': 5.92e-8, 'round_trip': 1.32e-7, 'q': 2.39e-7, 'qd': 2.40e-6, 'pos': 2.93e-6},
    # qdd, round_trip: pendulum x70 (an env whose tau - h nearly cancels: a small largest entry); q, qd: double_pendulum x3 K=5 T=8; pos: cart_tree x3 K=5 T=8
    'short': {'qdd': 4.52e-6, 'round_trip': 9.00e-6, 'q': 2.08e-7, 'qd': 3.50e-7, 'pos': 3.16e-7},
    'step': {'step_ref': 2.43e-7, 'step_diff': 0.0},   # (the joint angles of the five steps and of the rollout: the same bits; velocities 1.79e-7 rad/s apart)
}
BOUND = {g: {k: 8 * v for k, v in row.items()} for g, row in MEASURED.items()}
PARITY_Q_TOL = 2e-4   # rad: what tests/test_parity_gpu.py grants the step's joint angles against the checker
GROUP = {'pendulum': 'short', 'double_pendulum': 'short', 'cart_tree': 'short', 'ur_admittance': 'arms', 'ur_randomized': 'arms', 'ur5_gripper': 'arms'}
MODE = {'4': 0, '1': 0}   # DG_MAX_LANES -> the mode ur_admittance gets (sim.lanes)
LOCAL = (0.03, -0.02, 0.05)
G = (0.0, 0.0, -9.81)
SCENES = {
    'pendulum': ('pendulum.yaml', 'pend', 'hinge'), 'double_pendulum': ('double_pendulum.yaml', 'dp', 'j2'), 'cart_tree': ('cart_tree_fixed.yaml', 'cart', 'tip_joint'),
    'ur_admittance': ('ur_admittance.yaml', 'arm', 'ee_fixed_joint'), 'ur_randomized': ('ur_randomized.yaml', 'ur5_r', 'ee_fixed_joint'),
    'ur5_gripper': ('ur5_gripper.yaml', 'arm', 'ee_fixed_joint'),
}
FD_CASES = [(s, B, None) for s in SCENES for B in (1, 3, 70)] + [('ur_admittance', B, lanes) for lanes in ('4', '1') for B in (1, 3, 70)]
# rollouts: every scene at (B, K, T) = (1, 1, 1), (3, 50, 2), (3, 5, 8); the UR5 also at 70 envs, and in the two narrow modes
ROLL_CASES = ([(s, B, K, T, None) for s in SCENES for B, K, T in ((1, 1, 1), (3, 50, 2), (3, 5, 8))] + [('ur_admittance', 70, 5, 8, None)]
              + [('ur_admittance', B, K, T, lanes) for lanes in ('4', '1') for B, K, T in ((1, 1, 1), (3, 50, 2), (70, 5, 8))])
_ENVS, _FD_REFS, _ROLL_REFS = {}, {}, {}


def make(scene, B, lanes, monkeypatch, **kw):
    """The env of a case, built once per session; ``lanes``: DG_MAX_LANES while the world is created."""
    key = (scene, B, lanes, tuple(sorted(kw)))
    if key not in _ENVS:
        if lanes:
            monkeypatch.setenv('DG_MAX_LANES', lanes)
        env = DIYGym(os.path.join(GOLDEN, SCENES[scene][0]), num_envs=B, device=DEV, seed=5, **kw)
        if lanes:
            assert env.sim.lanes == MODE[lanes]
        _ENVS[key] = env
    env = _ENVS[key]
    return env, env.models[SCENES[scene][1]]


def draws(robot, B, seed, shape=()):
    """Per-env q in [-pi, pi] and inside the joint limits, qd, tau (``shape``: the axes between env and joint) -- fp32 values, as
    the kernel gets them."""
    rng = np.random.default_rng(seed)
    lim = D.joint_limits(robot)
    lo, hi = np.maximum(lim[:, 0], -np.pi), np.minimum(lim[:, 1], np.pi)
    n = robot.num_dofs
    return (rng.uniform(lo, hi, (B, n)).astype(np.float32), rng.uniform(-2.0, 2.0, (B, n)).astype(np.float32),
            rng.uniform(-3.0, 3.0, (B, ) + tuple(shape) + (n, )).astype(np.float32))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def frame_of(robot, name):
    return [j.name for j in robot.joints].index(name)


def fd_reference(scene, B, env, model):
    """(inputs, qdd [B, n] fp64 without and with joint damping, cond(M) [B]) of a scene at a batch size, computed once (the lane
    modes of a scene share it: the draws and the state are the same)."""
    key = (scene, B)
    if key not in _FD_REFS:
        robot, uid = model.robot, model.uid
        Tb, scales = D.base_transforms(env, uid), D.mass_scales(env, uid)
        q, qd, tau = draws(robot, B, 2000 * B + 1)
        ref = [np.stack([FD.fd(robot, q[e].astype(np.float64), qd[e], tau[e], damping, G, Tb[e], scales[e]) for e in range(B)]) for damping in (False, True)]
        cond = np.array([np.linalg.cond(D.mass_matrix(robot, q[e].astype(np.float64), Tb[e], scales[e])) for e in range(B)])
        _FD_REFS[key] = ((q, qd, tau), ref[0], ref[1], cond)
    return _FD_REFS[key]


def roll_reference(scene, B, K, T, env, model):
    """(inputs, q, qd [B, K, T, n], pos [B, K, T, 3]) in fp64, joint damping on, dt = the substep; computed once."""
    key = (scene, B, K, T)
    if key not in _ROLL_REFS:
        robot, uid = model.robot, model.uid
        Tb, scales = D.base_transforms(env, uid), D.mass_scales(env, uid)
        q0, qd0, acc = draws(robot, B, 3000 * B + 10 * K + T, (K, T))
        n, frame = robot.num_dofs, frame_of(robot, SCENES[scene][2])
        # torques a controller would ask for: those of accelerations in [-3, 3] at the start state.  (Uniform torques would spin
        # the gripper's fingers -- inertias of 1e-6 kg m^2 -- through thousands of radians in eight steps: a trajectory that no two
        # precisions share.)
        tau = np.stack([[[D.inverse_dynamics(robot, q0[e].astype(np.float64), qd0[e], acc[e, k, t], G, Tb[e], scales[e]) for t in range(T)] for k in range(K)]
                        for e in range(B)]).astype(np.float32)
        q, qd, pos = np.zeros((B, K, T, n)), np.zeros((B, K, T, n)), np.zeros((B, K, T, 3))
        for e in range(B):
            for k in range(K):
                q[e, k], qd[e, k], pos[e, k] = FD.rollout(robot, q0[e], qd0[e], tau[e, k], env.layout.dt, True, frame, LOCAL, G, Tb[e], scales[e])
        _ROLL_REFS[key] = ((q0, qd0, tau), q, qd, pos)
    return _ROLL_REFS[key]


def per_row(gpu, ref):
    """max |gpu - ref| / max |ref| over everything behind the first axis; a reference that is all zero in a row must be met exactly."""
    gpu, ref = gpu.reshape(gpu.shape[0], -1).astype(np.float64), ref.reshape(ref.shape[0], -1)
    scale, err = np.abs(ref).max(axis=1), np.abs(gpu - ref).max(axis=1)
    assert (err[scale == 0] == 0).all()
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0)


def check(scene, worst):
    for k, v in worst.items():
        assert v < BOUND[GROUP[scene]][k], (scene, k, v, BOUND[GROUP[scene]][k])


@pytest.mark.parametrize('scene,B,lanes', FD_CASES)
def test_forward_dynamics_matches_the_reference_and_inverts_inverse_dynamics(scene, B, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    scales = D.mass_scales(env, uid)
    if scene == 'ur_randomized':
        assert np.abs(scales - scales[0]).max() > 0.05 if B > 1 else np.abs(scales - 1.0).max() > 0.05   # (scales ignored cannot pass)
    (q, qd, tau), ref, ref_damped, cond = fd_reference(scene, B, env, model)
    qdd, sing = sim.calculate_forward_dynamics(uid, dev(q), dev(qd), dev(tau), return_singular=True)
    assert qdd.shape == (B, n) and qdd.dtype == torch.float32 and sing.shape == (B, ) and sing.dtype == torch.int32
    assert bool((sing == 0).all()) and bool(torch.isfinite(qdd).all())
    worst = {'qdd': float((per_row(qdd.cpu().numpy(), ref) / cond).max())}
    damped = sim.calculate_forward_dynamics(uid, dev(q), dev(qd), dev(tau), joint_damping=True)
    assert damped.data_ptr() == qdd.data_ptr()   # the buffer is reused
    worst['qdd'] = max(worst['qdd'], float((per_row(damped.cpu().numpy(), ref_damped) / cond).max()))
    if np.abs(FD.joint_damping(robot)).max() > 0:
        assert np.abs(ref - ref_damped).max() > 0
    # the round trip on the kernels themselves
    a = dev(draws(robot, B, 77)[2])
    back = sim.calculate_forward_dynamics(uid, dev(q), dev(qd), sim.calculate_inverse_dynamics(uid, dev(q), dev(qd), a).clone())
    worst['round_trip'] = float((per_row(back.cpu().numpy(), a.cpu().numpy().astype(np.float64)) / cond).max())
    print('%s x%d lanes=%s: %s (cond M up to %.3g)' % (scene, B, sim.lanes, ' '.join('%s %.4g' % kv for kv in worst.items()), cond.max()))
    check(scene, worst)


@pytest.mark.parametrize('scene,B,K,T,lanes', ROLL_CASES)
def test_rollout_matches_the_reference(scene, B, K, T, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n, frame = robot.num_dofs, frame_of(robot, SCENES[scene][2])
    (q0, qd0, tau), q, qd, pos = roll_reference(scene, B, K, T, env, model)
    r = sim.rollout_joint_dynamics(uid, dev(tau), dev(q0), dev(qd0), frame=frame, local_pos=LOCAL, joint_damping=True, want=('q', 'qd', 'pos', 'singular'))
    assert isinstance(r, JointRollout)
    assert r.q.shape == (B, K, T, n) and r.qd.shape == (B, K, T, n) and r.pos.shape == (B, K, T, 3) and r.singular.shape == (B, K) and r.singular.dtype == torch.int32
    assert bool((r.singular == 0).all()) and all(bool(torch.isfinite(t).all()) for t in (r.q, r.qd, r.pos))
    items = lambda a: a.reshape((B * K, ) + a.shape[2:])
    worst = {k: float(per_row(items(getattr(r, k).cpu().numpy()), items(ref)).max()) for k, ref in (('q', q), ('qd', qd), ('pos', pos))}
    print('%s x%d K=%d T=%d lanes=%s grid=%d: %s' % (scene, B, K, T, sim.lanes, sim.rollout_grid(K), ' '.join('%s %.4g' % kv for kv in worst.items())))
    check(scene, worst)


def test_the_capped_grid_of_the_global_workspace_mode_strides(monkeypatch):
    """70 envs x 5 samples in the global-workspace mode: the workspace holds the STEP's grid (two workgroups of 64 lanes), so 350
    items run as a grid-stride loop -- three trips for most lanes, two at the tail -- and still match the reference item by item
    (test_rollout_matches_the_reference has the figures); the LDS mode takes a workgroup per 16 items."""
    env, model = make('ur_admittance', 70, '4', monkeypatch)
    sim = env.sim
    assert sim.lanes == 0
    step_grid = (70 + 63) // 64
    assert sim.rollout_grid(5) == step_grid < (70 * 5 + 63) // 64   # capped
    assert sim.rollout_grid(1) == step_grid
    wide, _ = make('ur_admittance', 70, None, monkeypatch)
    per = wide.sim.lanes
    assert per > 0 and wide.sim.rollout_grid(5) == (70 * 5 + per - 1) // per > (70 + per - 1) // per   # an LDS mode: one item per lane
    (q0, qd0, tau), q, qd, pos = roll_reference('ur_admittance', 70, 5, 8, env, model)
    r = sim.rollout_joint_dynamics(model.uid, dev(tau), dev(q0), dev(qd0), joint_damping=True, want=('q', ))
    err = per_row(r.q.cpu().numpy().reshape(350, -1), q.reshape(350, -1))
    assert err.max() < BOUND['arms']['q'] and err[300:].max() > 0   # the last stride's items were computed too (fp32 never meets fp64 exactly)


@pytest.mark.parametrize('scene,B,lanes', [('cart_tree', 3, None), ('ur_randomized', 70, None), ('ur_admittance', 70, '4'), ('ur5_gripper', 3, None)])
def test_current_state_equals_the_explicit_call_in_bits(scene, B, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    L, n = env.layout, robot.num_dofs
    q0, qd0, tau = draws(robot, B, 7, (4, 3))
    st = sim.get_state()
    first = L.body_first_link[L.resolve_frame(uid, -1)[0]]
    for i in range(n):
        st[:, L.link_state_off[first + i] + KC.LS_Q] = 0.5 * q0[:, i]; st[:, L.link_state_off[first + i] + KC.LS_QD] = 0.2 * qd0[:, i]
    sim.set_state(st)
    q, qd = (t.clone() for t in sim.joint_states(uid))
    assert float(q.abs().max()) > 0 and torch.equal(q, dev(0.5 * q0))
    t1 = dev(tau[:, 0, 0])
    for damping in (False, True):
        implicit = sim.calculate_forward_dynamics(uid, tau=t1, joint_damping=damping).clone()
        assert torch.equal(implicit, sim.calculate_forward_dynamics(uid, q, qd, t1, joint_damping=damping))
    # tau = None is zero torque; one [nv] vector stands for every env
    assert torch.equal(sim.calculate_forward_dynamics(uid).clone(), sim.calculate_forward_dynamics(uid, q, qd, torch.zeros_like(q)))
    one = sim.calculate_forward_dynamics(uid, q[0].clone(), qd[0].clone(), t1[0].clone()).clone()
    rows = lambda t: t[0:1].expand(B, n).contiguous()
    assert torch.equal(one, sim.calculate_forward_dynamics(uid, rows(q), rows(qd), rows(t1)))
    frame = frame_of(robot, SCENES[scene][2])
    implicit = [t.clone() for t in sim.rollout_joint_dynamics(uid, dev(tau), frame=frame, local_pos=LOCAL, want=('q', 'qd', 'pos', 'singular'))]
    explicit = sim.rollout_joint_dynamics(uid, dev(tau), q, qd, frame=frame, local_pos=LOCAL, want=('q', 'qd', 'pos', 'singular'))
    assert all(torch.equal(a, b) for a, b in zip(implicit, explicit))
    assert np.array_equal(sim.get_state(), st.astype(np.float32))   # the rollout wrote no state


@pytest.mark.parametrize('scene,B,lanes', [('double_pendulum', 3, None), ('cart_tree', 70, None), ('ur_admittance', 3, None), ('ur_admittance', 3, '1'), ('ur5_gripper', 3, None)])
def test_one_step_of_one_sample_is_the_forward_dynamics_call_integrated(scene, B, lanes, monkeypatch):
    """K = 1, T = 1 equals q + dt (qd + dt qdd) of calculate_forward_dynamics within that call's bound (the two kernels inline the
    same passes, but not necessarily to the same bits)."""
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    q0, qd0, tau = draws(robot, B, 11, (1, 1))
    dt = 0.01
    Tb, scales = D.base_transforms(env, uid), D.mass_scales(env, uid)
    cond = np.array([np.linalg.cond(D.mass_matrix(robot, q0[e].astype(np.float64), Tb[e], scales[e])) for e in range(B)])
    for damping in (False, True):
        qdd = sim.calculate_forward_dynamics(uid, dev(q0), dev(qd0), dev(tau[:, 0, 0]), joint_damping=damping).cpu().numpy().astype(np.float64)
        r = sim.rollout_joint_dynamics(uid, dev(tau), dev(q0), dev(qd0), dt=dt, joint_damping=damping)
        assert r.pos is None and r.singular is None
        qd1 = qd0 + dt * qdd
        # the rollout's qdd, recovered from its velocity row, against the call's: the call's own measure and bound
        got = (r.qd.cpu().numpy()[:, 0, 0].astype(np.float64) - qd0) / dt
        fig = float((per_row(got, qdd) / cond).max())
        slack = float((np.abs(qd0).max(axis=1) * 2.0 ** -23 / dt / np.abs(qdd).max(axis=1) / cond).max())   # rounding of the fp32 velocity row itself
        print('%s x%d lanes=%s damping=%s: rollout qdd against the call %.3g (+ %.3g for the velocity row)' % (scene, B, sim.lanes, damping, fig, slack))
        assert fig < BOUND[GROUP[scene]]['qdd'] + slack
        assert np.abs(r.q.cpu().numpy()[:, 0, 0] - (q0 + dt * qd1)).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(q0).max()) + dt * dt * np.abs(qdd).max() * 1e-3


@pytest.mark.parametrize('scene,lanes', [('ur_admittance', None), ('ur_admittance', '4'), ('cart_tree', None), ('ur5_gripper', None)])
def test_a_sample_of_many_is_the_single_sample_call_in_bits(scene, lanes, monkeypatch):
    """No lane depends on its neighbours, on its position in the wavefront or on the trips it made before."""
    B, K, T = 3, 50, 2
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    frame = frame_of(robot, SCENES[scene][2])
    (q0, qd0, tau), _, _, _ = roll_reference(scene, B, K, T, env, model)
    many = [t.clone() for t in sim.rollout_joint_dynamics(uid, dev(tau), dev(q0), dev(qd0), frame=frame, local_pos=LOCAL, joint_damping=True,
                                                          want=('q', 'qd', 'pos', 'singular'))]
    for k in (0, 21, 49):
        one = sim.rollout_joint_dynamics(uid, dev(tau[:, k:k + 1]), dev(q0), dev(qd0), frame=frame, local_pos=LOCAL, joint_damping=True, want=('q', 'qd', 'pos', 'singular'))
        assert all(torch.equal(a[:, k:k + 1], b) for a, b in zip(many, one)), k


def test_want_selects_the_outputs_and_buffers_are_reused(monkeypatch):
    env, model = make('ur_admittance', 3, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    frame = frame_of(robot, 'ee_fixed_joint')
    q0, qd0, tau = draws(robot, 3, 5, (5, 8))
    full = JointRollout(*[t.clone() for t in sim.rollout_joint_dynamics(uid, dev(tau), dev(q0), dev(qd0), frame=frame, local_pos=LOCAL, want=('q', 'qd', 'pos', 'singular'))])
    default = sim.rollout_joint_dynamics(uid, dev(tau), dev(q0), dev(qd0))
    assert default.pos is None and default.singular is None and torch.equal(default.q, full.q) and torch.equal(default.qd, full.qd)
    for want in (('q', ), ('qd', ), ('pos', ), ('singular', ), ('qd', 'pos')):
        sub = sim.rollout_joint_dynamics(uid, dev(tau), dev(q0), dev(qd0), frame=frame, local_pos=LOCAL, want=want)
        for f in JointRollout._fields:
            assert (getattr(sub, f) is None) == (f not in want)
            assert getattr(sub, f) is None or torch.equal(getattr(sub, f), getattr(full, f)), (want, f)
    a = sim.rollout_joint_dynamics(uid, dev(tau), dev(q0), dev(qd0))
    b = sim.rollout_joint_dynamics(uid, dev(tau * 0.5), dev(q0), dev(qd0))
    assert a.q.data_ptr() == b.q.data_ptr() and a.qd.data_ptr() == b.qd.data_ptr()   # kept per (want, K, T) and reused
    c = sim.rollout_joint_dynamics(uid, dev(tau[:, :2]), dev(q0), dev(qd0))
    assert c.q.data_ptr() != a.q.data_ptr() and c.q.shape == (3, 2, 8, 6)
    # dt: None is the substep
    assert torch.equal(sim.rollout_joint_dynamics(uid, dev(tau), dev(q0), dev(qd0)).q.clone(), sim.rollout_joint_dynamics(uid, dev(tau), dev(q0), dev(qd0), dt=env.layout.dt).q)


def test_the_rollout_follows_the_real_step(monkeypatch):
    """ur_admittance with the engine's link damping 0 and the motors off, B = 3: N = 5 steps of env.step with a fixed
    apply_joint_torque each step, against ONE rollout with K = 1, T = substeps x N and the torque repeated per substep.  The two
    are different algorithms in fp32 (the step's articulated-body pass, the rollout's M^-1), so: bound = 8 x the rollout's measured
    error against fp64 at that T (MEASURED['step']['step_ref'], radians) + the joint-angle tolerance the parity tests grant the
    step against the checker."""
    N, B = 5, 3
    env, model = make('ur_admittance', B, None, monkeypatch, engine={'linear_damping': 0.0, 'angular_damping': 0.0})
    sim, robot, uid, L = env.sim, model.robot, model.uid, env.layout
    n = robot.num_dofs
    cfg = sim.motor_cfg(); cfg[:, 2] = 0.0; sim.set_motor_cfg(cfg)
    rng = np.random.default_rng(23)
    q0 = (np.array([0.3, -1.0, 1.2, -0.5, 0.4, 0.1]) + rng.uniform(-0.2, 0.2, (B, n))).astype(np.float32)
    qd0 = rng.uniform(-0.3, 0.3, (B, n)).astype(np.float32)
    torque = rng.uniform(-2.0, 2.0, (B, n)).astype(np.float32)
    sim.reset_joint_state(uid, dev(q0), dev(qd0))
    T = L.substeps * N
    tau = np.ascontiguousarray(np.broadcast_to(torque[:, None, None, :], (B, 1, T, n)))
    roll = JointRollout(*[None if t is None else t.clone() for t in sim.rollout_joint_dynamics(uid, dev(tau), joint_damping=True)])
    Tb = D.base_transforms(env, uid)
    ref = np.stack([FD.rollout(robot, q0[e], qd0[e], tau[e, 0], L.dt, True, None, LOCAL, G, Tb[e])[0] for e in range(B)])
    ref_err = float(np.abs(roll.q.cpu().numpy()[:, 0].astype(np.float64) - ref).max())
    for _ in range(N):
        sim.apply_joint_torque(uid, dev(torque))
        sim.step(0)
    q_step, _ = sim.joint_states(uid)
    assert float((q_step - dev(q0)).abs().max()) > 1e-3   # it moved
    q_step, qd_step = sim.joint_states(uid)
    diff = float((q_step - roll.q[:, 0, T - 1]).abs().max())
    print('ur_admittance x%d: rollout against fp64 at T = %d: %.3g rad; %d steps against the rollout: %.3g rad (velocities: %.3g rad/s)'
          % (B, T, ref_err, N, diff, float((qd_step - roll.qd[:, 0, T - 1]).abs().max())))
    assert ref_err < BOUND['step']['step_ref']
    assert diff < BOUND['step']['step_ref'] + PARITY_Q_TOL


def test_refusals_raise_value_error_with_the_entrys_text_and_launch_nothing(monkeypatch):
    env, model = make('cart_tree', 3, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    q, qd, tau = (dev(a) for a in draws(robot, 3, 1, (2, 4)))
    tip = frame_of(robot, 'tip_joint')
    kept = [t for t in sim.rollout_joint_dynamics(uid, tau, q, qd, frame=tip, want=('q', 'qd', 'pos', 'singular'))] + [sim.calculate_forward_dynamics(uid, q, qd)]
    before = [t.clone() for t in kept]
    floating = DIYGym(os.path.join(GOLDEN, 'cart_tree.yaml'), num_envs=3, device=DEV)   # a floating TREE: refused
    plane = DIYGym(os.path.join(GOLDEN, 'ur5_gripper.yaml'), num_envs=3, device=DEV)
    F, R = 'dg_world_forward_dynamics: ', 'dg_world_rollout: '
    fuid, puid = floating.models['cart'].uid, plane.models['plane'].uid
    bad = [(lambda: floating.sim.calculate_forward_dynamics(fuid), 'fixed-base'),
           (lambda: plane.sim.calculate_forward_dynamics(puid), 'fixed-base'),
           (lambda: sim.calculate_forward_dynamics(99), 'out of range'),
           (lambda: sim.calculate_forward_dynamics(uid, q[:, :2].contiguous()), 'shape'),
           (lambda: sim.calculate_forward_dynamics(uid, q.double()), 'float32'),
           (lambda: sim.calculate_forward_dynamics(uid, tau=q.cpu()), 'cpu'),
           (lambda: floating.sim.rollout_joint_dynamics(fuid, tau), 'fixed-base'),
           (lambda: plane.sim.rollout_joint_dynamics(puid, tau), 'fixed-base'),
           (lambda: sim.rollout_joint_dynamics(99, tau), 'out of range'),
           (lambda: sim.rollout_joint_dynamics(uid, None), R + 'tau is NULL'),
           (lambda: sim.rollout_joint_dynamics(uid, tau[:, :0].contiguous()), R + 'K must be >= 1, got 0'),
           (lambda: sim.rollout_joint_dynamics(uid, tau[:, :, :0].contiguous()), R + 'T must be >= 1, got 0'),
           (lambda: sim.rollout_joint_dynamics(uid, tau, dt=0.0), R + 'dt must be finite and > 0, got 0'),
           (lambda: sim.rollout_joint_dynamics(uid, tau, dt=-0.01), R + 'dt must be finite and > 0, got -0.01'),
           (lambda: sim.rollout_joint_dynamics(uid, tau, dt=float('nan')), R + 'dt must be finite and > 0, got nan'),
           (lambda: sim.rollout_joint_dynamics(uid, tau, dt=float('inf')), R + 'dt must be finite and > 0, got inf'),
           (lambda: sim.rollout_joint_dynamics(uid, tau, want=()), R + 'every output is NULL'),
           (lambda: sim.rollout_joint_dynamics(uid, tau, want=('pos', )), "'pos' in want needs frame"),
           (lambda: sim.rollout_joint_dynamics(uid, tau, frame=len(robot.joints), want=('pos', )), R + 'body %d has no frame %d' % (uid, len(robot.joints))),
           (lambda: sim.rollout_joint_dynamics(uid, tau, frame=-1, want=('pos', )), 'frame'),
           (lambda: sim.rollout_joint_dynamics(uid, tau, frame=tip, local_pos=(0.0, 0.0), want=('pos', )), 'local_pos'),
           (lambda: sim.rollout_joint_dynamics(uid, tau, want=('torque', )), 'want'),
           (lambda: sim.rollout_joint_dynamics(uid, tau[:, :, :, :2].contiguous()), 'shape'),
           (lambda: sim.rollout_joint_dynamics(uid, tau[:2].contiguous()), 'shape'),
           (lambda: sim.rollout_joint_dynamics(uid, tau[0]), 'shape'),
           (lambda: sim.rollout_joint_dynamics(uid, tau.double()), 'float32'),
           (lambda: sim.rollout_joint_dynamics(uid, tau.cpu()), 'cpu'),
           (lambda: sim.rollout_joint_dynamics(uid, tau, q0=q[:, :2].contiguous()), 'shape')]
    for fn, text in bad:
        with pytest.raises(ValueError) as info:
            fn()
        assert text in str(info.value), (text, str(info.value))
    # the C entries themselves: DG_ERR_ARG with their text, nothing launched
    lib, st = sim.lib, ctypes.c_void_p(sim.state.data_ptr())
    out = torch.full((3, 256), 7.0, device=DEV)
    o, lp, t = ctypes.c_void_p(out.data_ptr()), (ctypes.c_float * 3)(*LOCAL), ctypes.c_void_p(tau.data_ptr())
    fst = ctypes.c_void_p(floating.sim.state.data_ptr())
    big = 2 ** 31 - 1
    for args, text in (((sim.handle, st, uid, tip, lp, 0, 4, 0.01, 0, None, None, t, o, o, o, o), 'K must be >= 1, got 0'),
                       ((sim.handle, st, uid, tip, lp, 2, -1, 0.01, 0, None, None, t, o, o, o, o), 'T must be >= 1, got -1'),
                       ((sim.handle, st, uid, tip, lp, 2, 4, 0.0, 0, None, None, t, o, o, o, o), 'dt must be finite and > 0, got 0'),
                       ((sim.handle, st, uid, tip, lp, 2, 4, float('inf'), 0, None, None, t, o, o, o, o), 'dt must be finite and > 0, got inf'),
                       ((sim.handle, st, uid, tip, lp, 2, 4, 0.01, 0, None, None, None, o, o, o, o), 'tau is NULL'),
                       ((sim.handle, st, uid, tip, lp, 2, 4, 0.01, 0, None, None, t, None, None, None, None), 'every output is NULL'),
                       ((sim.handle, st, uid, tip, lp, big, big, 0.01, 0, None, None, t, o, o, o, o), '3 envs x K %d x T %d x 3 joints is beyond INT64_MAX / 4 values' % (big, big)),
                       ((sim.handle, st, uid, tip, None, 2, 4, 0.01, 0, None, None, t, o, o, o, o), 'local_pos is NULL (three host floats)'),
                       ((sim.handle, st, uid, -1, lp, 2, 4, 0.01, 0, None, None, t, o, o, o, o), 'frame -1 out of range (the base of a fixed body does not move)'),
                       ((sim.handle, st, uid, 40, lp, 2, 4, 0.01, 0, None, None, t, o, o, o, o), 'body %d has no frame 40' % uid),
                       ((sim.handle, st, 99, tip, lp, 2, 4, 0.01, 0, None, None, t, o, o, o, o), 'body 99 out of range'),
                       ((sim.handle, None, uid, tip, lp, 2, 4, 0.01, 0, None, None, t, o, o, o, o), 'null argument'),
                       ((floating.sim.handle, fst, fuid, 0, lp, 2, 4, 0.01, 0, None, None, t, o, o, o, o),
                        'body %d has a floating base; the dynamics queries take fixed-base bodies only' % fuid)):
        assert lib.dg_world_rollout(*args, None) == -4
        assert lib.dg_last_error().decode() == R + text
    for args, text in (((sim.handle, st, uid, None, None, None, 0, None, None), 'qdd and singular are both NULL'),
                       ((sim.handle, st, 99, None, None, None, 0, o, o), 'body 99 out of range'),
                       ((sim.handle, None, uid, None, None, None, 0, o, o), 'null argument'),
                       ((floating.sim.handle, fst, fuid, None, None, None, 0, o, o),
                        'body %d has a floating base; the dynamics queries take fixed-base bodies only' % fuid)):
        assert lib.dg_world_forward_dynamics(*args, None) == -4
        assert lib.dg_last_error().decode() == F + text
    # a static body (the gripper scene's plane): frozen into the static world, or a fixed base without joints -- whichever the scene made it
    pst = ctypes.c_void_p(plane.sim.state.data_ptr())
    static = ('body %d is part of the frozen static world: it has no joints' % puid, 'body %d has no joints' % puid)
    assert lib.dg_world_rollout(plane.sim.handle, pst, puid, 0, lp, 2, 4, 0.01, 0, None, None, t, o, o, o, o, None) == -4
    assert lib.dg_last_error().decode() in [R + s for s in static]
    assert lib.dg_world_forward_dynamics(plane.sim.handle, pst, puid, None, None, None, 0, o, o, None) == -4
    assert lib.dg_last_error().decode() in [F + s for s in static]
    # a frame is ignored without pos_out
    flags = torch.full((3, 2), 7, dtype=torch.int32, device=DEV)
    assert lib.dg_world_rollout(sim.handle, st, uid, 40, None, 2, 4, 0.01, 0, None, None, t, None, None, None, ctypes.c_void_p(flags.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((flags == 0).all())
    assert all(torch.equal(a, b) for a, b in zip(kept, before))
