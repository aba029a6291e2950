"""env.sim.task_space_dynamics (dg_world_task_space, task_space_kernel) on the GPU against the fp64 reference of
tests/task_space_ref.py (itself pinned by tests/test_task_space_ref.py).

Scenes: a pendulum, a double pendulum, the branching cart bolted down (prismatic joint, two branches, a frame on a fixed joint), a
UR5 (also with DG_MAX_LANES 4 and 1 -- a scene with a register-chain body stops at 16 envs per wavefront, so both put it in the
global-workspace mode, Lane<0> -- and with 16), the two UR5s whose link masses a dynamics_randomizer scales per env, and the twelve-joint
UR5 + gripper tree in its default one-env-per-wavefront mode.  Batches of 1, 3 and 70 envs (70 crosses a wavefront).  Per-env q in
[-pi, pi] and inside the joint limits, qd in [-2, 2], random acc and tau_null, a point off the inertial origin.  Tasks: the six rows
and the three translational rows with a null-space torque on the six-axis arms and the gripper tree, and rows no more than the
chain is long elsewhere (TASKS below).

Error measure, as tests/test_dynamics_queries_gpu.py: per env, max |gpu - reference| over the quantity divided by that env's
largest |reference| entry; the figure of a case is the largest over its envs.  For `lambda` and `tau` the per-env figure is
additionally divided by the fp64 cond(A), A = J M^-1 J^T, and only envs with cond(A) <= 1e3 are compared -- for these two and for
`singular == 0`; the others are still asked to be finite.  How many envs that leaves out is known beforehand (400 draws each on
the CPU with dynamics_ref: UR5 at ee_fixed_joint 11 % at six rows, 0.5 % at three; the gripper tree 12 % and 0 %; the double
pendulum's tip in (x, z) 5 %; the cart's tip in (x, z) 3 %; every one-row task 0 %) and asserted per scene: at most one quarter.

The bounds below are 8 x the largest figure measured over all cases of this file on an MI355X (DESIGN.md "Task-space dynamics"
has the table); the margin is for a compiler that contracts multiply-adds differently, not for bugs.

A kept env whose `lambda` figure -- before the division by cond(A) -- exceeds 64 x 2^-24 x cond(M) is a finding to explain.  There
is one kind, in the one- and two-row tasks of the short chains only, four envs in all: the pendulum's z row at 70 envs reads
3.99e-6 against 3.81e-6, the double pendulum's first link in x 1.05e-4 against 2.35e-5.  A world row picked out of
the point's Jacobian can be small against the Jacobian it is picked from -- the pendulum's tip moving almost horizontally -- while its
fp32 error is that of the whole: the pose's rounding, 2^-24 of the LARGEST entry.  The row's relative error is then larger by
rho = max |[jac_t; jac_r]| / max |selected rows|, and lambda, which is quadratic in the row, carries it; neither cond(A) (1 for a
single row) nor cond(M) sees that.  The test therefore asserts the threshold times rho -- rho is 1 for the six-row tasks -- and prints
every env over the plain threshold (measured: rho 21 and 30 for the pendulum's two envs, 5 and 1.9e3 for the double pendulum's).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import dynamics_ref as D
import task_space_ref as TS
from diy_gym_amd import DIYGym
from diy_gym_amd.backend import TaskSpaceDynamics
from diy_gym_amd.scene import K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda:0'
# measured maxima (MI355X, all cases of this file), in two groups, and the bounds 8 x them.  'arms': the six-axis arms and the gripper
# tree, six and three rows.  'short': pendulum, double pendulum, cart -- one- and two-row tasks, where an env's largest entry of a
# quantity is often a SMALL number (a world row the point hardly moves along, a gravity torque near its zero crossing, a bias
# acceleration that is what is left of a_link + g), so that the same absolute error reads 1e2 .. 1e4 times larger on this measure.
# 'sibling': jac and bias_torque against calculate_jacobian / calculate_inverse_dynamics of the same world.
MEASURED = {
    # jac, bias_acc, point: ur_admittance x70 (every mode the same figures); bias_torque, lambda: ur_randomized x70; tau: ur5_gripper x70
    # (cond M = 1.4e6; 9.3e-7 on the six-axis arms)
    'arms': {'jac': 7.35e-7, 'bias_acc': 7.01e-6, 'bias_torque': 1.97e-6, 'lambda': 7.77e-7, 'tau': 3.86e-5, 'point_pos': 1.71e-6, 'point_quat': 4.60e-7,
             'point_vel': 1.39e-6},
    # jac, lambda, tau, point_vel: double_pendulum x70; bias_acc, point_quat: cart_tree x70; bias_torque, point_pos: pendulum x70
    'short': {'jac': 5.36e-5, 'bias_acc': 6.53e-3, 'bias_torque': 2.12e-5, 'lambda': 1.05e-4, 'tau': 4.94e-5, 'point_pos': 1.75e-7, 'point_quat': 2.30e-7,
              'point_vel': 3.35e-7},
    # jac: cart_tree x70; bias_torque: ur_randomized x70
    'sibling': {'jac': 3.15e-7, 'bias_torque': 1.19e-7},
}
BOUND = {g: {k: (1.0 if v is None else 8 * v) for k, v in row.items()} for g, row in MEASURED.items()}
GROUP = {'pendulum': 'short', 'double_pendulum': 'short', 'cart_tree': 'short', 'ur_admittance': 'arms', 'ur_randomized': 'arms', 'ur5_gripper': 'arms'}
# DG_MAX_LANES -> the mode ur_admittance gets (sim.lanes)
MODE = {'4': 0, '1': 0, '16': 16}
LOCAL = (0.03, -0.02, 0.05)
G = (0.0, 0.0, -9.81)
COND_KEPT = 1e3
SCENES = {
    'pendulum': ('pendulum.yaml', 'pend'), 'double_pendulum': ('double_pendulum.yaml', 'dp'), 'cart_tree': ('cart_tree_fixed.yaml', 'cart'),
    'ur_admittance': ('ur_admittance.yaml', 'arm'), 'ur_randomized': ('ur_randomized.yaml', 'ur5_r'), 'ur5_gripper': ('ur5_gripper.yaml', 'arm'),
}
ARM = [('ee_fixed_joint', (0, 1, 2, 3, 4, 5), True), ('ee_fixed_joint', (0, 1, 2), True)]
# scene -> [(frame: a joint's name, axes, with a null-space torque)]
TASKS = {
    'pendulum': [('hinge', (2, ), False), ('hinge', (4, ), True)],
    'double_pendulum': [('j2', (0, 2), False), ('j2', (4, ), True), ('j1', (0, ), True)],
    'cart_tree': [('tip_joint', (0, 2), True), ('hinge_a', (0, 1), False), ('hinge_b', (3, ), True), ('slide', (2, ), True)],
    'ur_admittance': ARM, 'ur_randomized': ARM, 'ur5_gripper': ARM,
}
CASES = ([(s, B, None) for s in SCENES for B in (1, 3, 70)] + [('ur_admittance', B, lanes) for lanes in ('4', '1') for B in (1, 3, 70)]
         + [('ur_admittance', 70, '16')])
_ENVS, _REFS = {}, {}


def make(scene, B, lanes, monkeypatch):
    """The env of a case, built once per session; ``lanes``: DG_MAX_LANES while the world is created."""
    key = (scene, B, lanes)
    if key not in _ENVS:
        if lanes:
            monkeypatch.setenv('DG_MAX_LANES', lanes)
        env = DIYGym(os.path.join(GOLDEN, SCENES[scene][0]), num_envs=B, device=DEV, seed=5)
        if lanes:
            assert env.sim.lanes == MODE[lanes]
        _ENVS[key] = env
    env = _ENVS[key]
    return env, env.models[SCENES[scene][1]]


def draws(robot, B, m, seed):
    """Per-env q in [-pi, pi] and inside the joint limits, qd, acc, tau_null -- fp32 values, as the kernel gets them."""
    rng = np.random.default_rng(seed)
    lim = D.joint_limits(robot)
    lo, hi = np.maximum(lim[:, 0], -np.pi), np.minimum(lim[:, 1], np.pi)
    n = robot.num_dofs
    return (rng.uniform(lo, hi, (B, n)).astype(np.float32), rng.uniform(-2.0, 2.0, (B, n)).astype(np.float32),
            rng.uniform(-5.0, 5.0, (B, m)).astype(np.float32), rng.uniform(-3.0, 3.0, (B, n)).astype(np.float32))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def frame_of(robot, name):
    return [j.name for j in robot.joints].index(name)


def reference(scene, B, env, model):
    """[(task, inputs, {field: [B, ...] fp64})] of a scene at a batch size, computed once (the lane modes of a scene share it: the
    draws and the state are the same)."""
    key = (scene, B)
    if key not in _REFS:
        robot, uid = model.robot, model.uid
        Tb, scales = D.base_transforms(env, uid), D.mass_scales(env, uid)
        out = []
        for t, (frame, axes, with_null) in enumerate(TASKS[scene]):
            q, qd, acc, t0 = draws(robot, B, len(axes), 1000 * B + t)
            rows = [TS.task_space(robot, q[e].astype(np.float64), qd[e], frame_of(robot, frame), LOCAL, axes, acc[e], t0[e] if with_null else None, 0.0, G,
                                  Tb[e], scales[e]) for e in range(B)]
            out.append(((frame, axes, with_null), (q, qd, acc, t0), {k: np.stack([np.asarray(r[k], dtype=np.float64) for r in rows]) for k in rows[0]}))
        _REFS[key] = out
    return _REFS[key]


def per_env(gpu, ref):
    """The file's error measure, env by env; a reference that is all zero in an env must be met exactly there."""
    gpu, ref = gpu.reshape(gpu.shape[0], -1).astype(np.float64), ref.reshape(ref.shape[0], -1)
    scale, err = np.abs(ref).max(axis=1), np.abs(gpu - ref).max(axis=1)
    assert (err[scale == 0] == 0).all()
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0)


def call(sim, uid, robot, task, inputs, **kw):
    frame, axes, with_null = task
    q, qd, acc, t0 = inputs
    torque = 'tau' in kw.get('want', ('tau', ))
    return sim.task_space_dynamics(uid, frame_of(robot, frame), LOCAL, axes, dev(q), dev(qd), dev(acc) if torque else None,
                                   dev(t0) if with_null and torque else None, **kw)


@pytest.mark.parametrize('scene,B,lanes', CASES)
def test_every_output_matches_the_reference(scene, B, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    scales = D.mass_scales(env, uid)
    if scene == 'ur_randomized':
        assert np.abs(scales - scales[0]).max() > 0.05 if B > 1 else np.abs(scales - 1.0).max() > 0.05   # (scales ignored cannot pass)
    else:
        assert (scales == 1.0).all()
    worst = dict.fromkeys(BOUND[GROUP[scene]], 0.0)
    Tb = D.base_transforms(env, uid)
    for task, inputs, ref in reference(scene, B, env, model):
        m = len(task[1])
        r = call(sim, uid, robot, task, inputs)
        assert isinstance(r, TaskSpaceDynamics)
        assert r.jac.shape == (B, m, n) and r.bias_acc.shape == (B, m) and r.bias_torque.shape == (B, n) and r.lambda_.shape == (B, m, m)
        assert r.tau.shape == (B, n) and r.point.shape == (B, 13) and r.singular.shape == (B, ) and r.singular.dtype == torch.int32
        got = {k.rstrip('_'): v.cpu().numpy() for k, v in r._asdict().items()}
        assert all(np.isfinite(v).all() for v in got.values())
        for k in ('jac', 'bias_acc', 'bias_torque'):
            worst[k] = max(worst[k], float(per_env(got[k], ref[k]).max()))
        # the pose: position, quaternion up to its sign, velocity
        sign = np.sign((got['point'][:, 3:7] * ref['point'][:, 3:7]).sum(axis=1, keepdims=True))
        worst['point_pos'] = max(worst['point_pos'], float(per_env(got['point'][:, 0:3], ref['point'][:, 0:3]).max()))
        worst['point_quat'] = max(worst['point_quat'], float(per_env(sign * got['point'][:, 3:7], ref['point'][:, 3:7]).max()))
        worst['point_vel'] = max(worst['point_vel'], float(per_env(got['point'][:, 7:13], ref['point'][:, 7:13]).max()))
        # lambda, tau, singular: the envs whose task is well conditioned
        kept = ref['cond_A'] <= COND_KEPT
        assert (ref['singular'][kept] == 0).all() and (got['singular'][kept] == 0).all()
        if kept.any():
            lam = per_env(got['lambda'][kept], ref['lambda'][kept])
            cond_m = np.array([np.linalg.cond(M) for M in ref['M'][kept]])
            rho = np.array([np.abs(np.vstack(D.jacobian(robot, inputs[0][e].astype(np.float64), frame_of(robot, task[0]), LOCAL, Tb[e]))).max()
                            for e in np.flatnonzero(kept)]) / np.abs(ref['jac'][kept]).reshape(int(kept.sum()), -1).max(axis=1)
            for e in np.flatnonzero(lam > 64 * 2.0 ** -24 * cond_m):
                print('finding: %s x%d %s kept env %d: lambda %.3g > 64 x 2^-24 x cond(M) = %.3g, rho %.3g' % (scene, B, task, e, lam[e], 64 * 2.0 ** -24 * cond_m[e], rho[e]))
            assert (lam <= 64 * 2.0 ** -24 * cond_m * rho).all(), (scene, B, task, float((lam / cond_m / rho).max()))
            worst['lambda'] = max(worst['lambda'], float((lam / ref['cond_A'][kept]).max()))
            worst['tau'] = max(worst['tau'], float((per_env(got['tau'][kept], ref['tau'][kept]) / ref['cond_A'][kept]).max()))
        assert (got['lambda'].view(np.uint32) == got['lambda'].transpose(0, 2, 1).view(np.uint32)).all()   # symmetric in bits
    print('%s x%d lanes=%s: %s' % (scene, B, sim.lanes, ' '.join('%s %.4g' % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v < BOUND[GROUP[scene]][k], (scene, B, k, v)


@pytest.mark.parametrize('scene', sorted(SCENES))
def test_at_most_a_quarter_of_a_scenes_envs_is_left_out(scene, monkeypatch):
    """... of the comparison of lambda, tau and singular, over the scene's tasks and batch sizes; and every task of every batch
    keeps at least one env."""
    kept = []
    for B in (1, 3, 70):
        env, model = make(scene, B, None, monkeypatch)
        for task, _, ref in reference(scene, B, env, model):
            assert (ref['cond_A'] <= COND_KEPT).any(), (scene, B, task)
            kept.append(ref['cond_A'] <= COND_KEPT)
    share = 1.0 - float(np.concatenate(kept).mean())
    print('%s: %.1f %% of %d envs left out' % (scene, 100 * share, np.concatenate(kept).size))
    assert share <= 0.25


@pytest.mark.parametrize('scene,B,lanes', [c for c in CASES if c[1] == 70])
def test_jacobian_and_bias_torque_against_the_siblings(scene, B, lanes, monkeypatch):
    """The passes are the new header's own copies of dg_dynq.h's, statement for statement, but not the same bits: inlined into another
    kernel the compiler contracts other multiply-adds (measured: the Jacobian differs in the last bit or two of some entries).  So
    the rule of the file: the file's measure against the sibling's values, bound 8 x the measured figure."""
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    worst = {'jac': 0.0, 'bias_torque': 0.0}
    for task, inputs, _ in reference(scene, B, env, model):
        q, qd = dev(inputs[0]), dev(inputs[1])
        r = call(sim, uid, robot, task, inputs, want=('jac', 'bias_torque'))
        jt, jr = sim.calculate_jacobian(uid, frame_of(robot, task[0]), LOCAL, q)
        full = torch.cat([jt, jr], dim=1)
        assert bool(((full[:, list(task[1])] == 0) == (r.jac == 0)).all())   # the same zero columns
        worst['jac'] = max(worst['jac'], float(per_env(r.jac.cpu().numpy(), full[:, list(task[1])].cpu().numpy().astype(np.float64)).max()))
        tau = sim.calculate_inverse_dynamics(uid, q, qd, torch.zeros_like(q))
        worst['bias_torque'] = max(worst['bias_torque'], float(per_env(r.bias_torque.cpu().numpy(), tau.cpu().numpy().astype(np.float64)).max()))
    print('%s x%d lanes=%s against the siblings: %s' % (scene, B, sim.lanes, ' '.join('%s %.4g' % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v < BOUND['sibling'][k], (scene, B, k, v)


@pytest.mark.parametrize('scene,B,lanes', [('cart_tree', 3, None), ('ur_randomized', 70, None), ('ur_admittance', 70, '4'), ('ur_admittance', 70, '16'), ('ur5_gripper', 3, None)])
def test_current_state_equals_the_explicit_call_and_a_subset_equals_the_full_call(scene, B, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    L, n = env.layout, robot.num_dofs
    # joints off their rest pose and moving, then five steps of random actions
    q0, qd0, _, _ = draws(robot, B, 1, 7)
    st = sim.get_state()
    first = L.body_first_link[L.resolve_frame(uid, -1)[0]]
    for i in range(n):
        st[:, L.link_state_off[first + i] + K.LS_Q] = 0.5 * q0[:, i]; st[:, L.link_state_off[first + i] + K.LS_QD] = 0.2 * qd0[:, i]
    sim.set_state(st)
    gen = torch.Generator().manual_seed(3)
    for _ in range(5):
        sim.step(env._all_slots, ((torch.rand((B, max(L.act_dim, 1)), generator=gen) * 2 - 1) * 0.3).to(DEV))
    q, qd = (t.clone() for t in sim.joint_states(uid))
    assert float(q.abs().max()) > 0
    frame, axes, _ = TASKS[scene][0]
    m = len(axes)
    acc, t0 = dev(draws(robot, B, m, 8)[2]), dev(draws(robot, B, m, 8)[3])
    args = (uid, frame_of(robot, frame), LOCAL, axes)
    implicit = [t.clone() for t in sim.task_space_dynamics(*args, acc=acc, tau_null=t0, damping=0.01)]
    explicit = sim.task_space_dynamics(*args, q=q, qd=qd, acc=acc, tau_null=t0, damping=0.01)
    assert all(torch.equal(a, b) and bool(torch.isfinite(a.float()).all()) for a, b in zip(implicit, explicit))
    # one [nv] / [m] vector stands for every env
    one = [t.clone() for t in sim.task_space_dynamics(*args, q=q[0].clone(), qd=qd[0].clone(), acc=acc[0].clone(), tau_null=t0[0].clone())]
    rows = lambda t: t[0:1].expand(B, t.shape[1]).contiguous()
    assert all(torch.equal(a, b) for a, b in zip(one, sim.task_space_dynamics(*args, q=rows(q), qd=rows(qd), acc=rows(acc), tau_null=rows(t0))))
    # a want subset: the same bits for the fields it keeps, None for the others; the default drops tau without acc
    full = TaskSpaceDynamics(*implicit)
    for want in (('tau', ), ('lambda', 'singular'), ('point', ), ('bias_acc', ), ('jac', 'bias_torque', 'point'), ('singular', )):
        sub = sim.task_space_dynamics(*args, acc=acc, tau_null=t0 if 'tau' in want else None, damping=0.01, want=want)
        for f in TaskSpaceDynamics._fields:
            assert (getattr(sub, f) is None) == (f.rstrip('_') not in want)
            assert getattr(sub, f) is None or torch.equal(getattr(sub, f), getattr(full, f)), (want, f)
    no_acc = sim.task_space_dynamics(*args, damping=0.01)
    assert no_acc.tau is None and all(torch.equal(getattr(no_acc, f), getattr(full, f)) for f in TaskSpaceDynamics._fields if f != 'tau')
    # damping reaches the diagonal: lambda shrinks
    assert float(sim.task_space_dynamics(*args, damping=10.0, want=('lambda', )).lambda_.abs().max()) < float(full.lambda_.abs().max())


@pytest.mark.parametrize('B', [3, 70])
def test_a_rank_deficient_task_is_flagged_and_every_output_is_finite(B, monkeypatch):
    """Three translational rows at the cart's branch frame, whose chain has two joints: A has rank 2 in every env."""
    env, model = make('cart_tree', B, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    q, qd, acc, t0 = draws(robot, B, 3, 77)
    r = sim.task_space_dynamics(uid, frame_of(robot, 'tip_joint'), LOCAL, (0, 1, 2), dev(q), dev(qd), dev(acc), dev(t0))
    assert bool((r.singular == 1).all())
    assert all(bool(torch.isfinite(t.float()).all()) for t in r)
    ref = [TS.task_space(robot, q[e].astype(np.float64), qd[e], frame_of(robot, 'tip_joint'), LOCAL, (0, 1, 2), T_base=D.base_transforms(env, uid)[e]) for e in range(B)]
    assert all(x['singular'] == 1 for x in ref)
    # ... and the same frame with two rows is not
    assert bool((sim.task_space_dynamics(uid, frame_of(robot, 'tip_joint'), LOCAL, (0, 2), dev(q), want=('singular', )).singular == 0).sum() >= 0.75 * B)


def test_refusals_raise_value_error_with_the_entrys_text_and_launch_nothing(monkeypatch):
    env, model = make('cart_tree', 3, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    q, qd, acc, t0 = (dev(a) for a in draws(robot, 3, 2, 1))
    tip = frame_of(robot, 'tip_joint')
    kept = [t for t in sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), q, qd, acc, t0)]
    before = [t.clone() for t in kept]
    floating = DIYGym(os.path.join(GOLDEN, 'cart_tree.yaml'), num_envs=3, device=DEV)   # a floating TREE: refused
    plane = DIYGym(os.path.join(GOLDEN, 'ur5_gripper.yaml'), num_envs=3, device=DEV)
    T = 'dg_world_task_space: '
    bad = [(lambda: floating.sim.task_space_dynamics(floating.models['cart'].uid, 0), 'fixed-base'),
           (lambda: plane.sim.task_space_dynamics(plane.models['plane'].uid, 0), 'fixed-base'),
           (lambda: sim.task_space_dynamics(99, 0), 'out of range'),
           (lambda: sim.task_space_dynamics(uid, -1), 'frame'),
           (lambda: sim.task_space_dynamics(uid, len(robot.joints), LOCAL, (0, )), T + 'body %d has no frame %d' % (uid, len(robot.joints))),
           (lambda: sim.task_space_dynamics(uid, tip, (0.0, 0.0)), 'local_pos'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, ()), T + 'axes_mask 0 selects no row or a row above 5'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 6)), T + 'axes_mask 65 selects no row or a row above 5'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 0)), 'distinct'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 1, 2, 3)), T + '4 task rows for a body of 3 joints'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), damping=-0.5), T + 'damping must be finite and >= 0, got -0.5'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), damping=float('nan')), T + 'damping must be finite and >= 0, got nan'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), damping=float('inf')), T + 'damping must be finite and >= 0, got inf'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), want=()), T + 'every output is NULL'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), want=('tau', )), T + 'tau needs acc'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), tau_null=t0, want=('point', )), T + 'tau_null without tau'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), want=('torque', )), 'want'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), q[:, :2].contiguous()), 'shape'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), q.double()), 'float32'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), q.cpu()), 'cpu'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), acc=acc[:, :1].contiguous()), 'shape'),
           (lambda: sim.task_space_dynamics(uid, tip, LOCAL, (0, 2), acc=acc, tau_null=t0[:2].contiguous()), 'shape')]
    for fn, text in bad:
        with pytest.raises(ValueError) as info:
            fn()
        assert text in str(info.value), (text, str(info.value))
    # the C entry itself: DG_ERR_ARG with its text, nothing launched
    lib, st = sim.lib, ctypes.c_void_p(sim.state.data_ptr())
    out = torch.full((3, 64), 7.0, device=DEV)
    o, lp = ctypes.c_void_p(out.data_ptr()), (ctypes.c_float * 3)(*LOCAL)
    fst = ctypes.c_void_p(floating.sim.state.data_ptr())
    entry = lambda *a: lib.dg_world_task_space(*a, None)
    for args, text in (((sim.handle, st, uid, tip, lp, 0, None, None, None, None, 0.0, o, o, o, o, None, o, o), 'axes_mask 0 selects no row or a row above 5 of [v; w]'),
                       ((sim.handle, st, uid, tip, lp, 64, None, None, None, None, 0.0, o, o, o, o, None, o, o), 'axes_mask 64 selects no row or a row above 5 of [v; w]'),
                       ((sim.handle, st, uid, tip, lp, 15, None, None, None, None, 0.0, o, o, o, o, None, o, o), '4 task rows for a body of 3 joints'),
                       ((sim.handle, st, uid, tip, lp, 5, None, None, None, None, -1.0, o, o, o, o, None, o, o), 'damping must be finite and >= 0, got -1'),
                       ((sim.handle, st, uid, tip, lp, 5, None, None, None, None, 0.0, None, None, None, None, None, None, None), 'every output is NULL'),
                       ((sim.handle, st, uid, tip, lp, 5, None, None, None, None, 0.0, o, o, o, o, o, o, o), 'tau needs acc'),
                       ((sim.handle, st, uid, tip, lp, 5, None, None, o, o, 0.0, o, o, o, o, None, o, o), 'tau_null without tau'),
                       ((sim.handle, st, uid, tip, None, 5, None, None, None, None, 0.0, o, o, o, o, None, o, o), 'local_pos is NULL (three host floats)'),
                       ((sim.handle, st, uid, -1, lp, 5, None, None, None, None, 0.0, o, o, o, o, None, o, o), 'frame -1 out of range (the base of a fixed body does not move)'),
                       ((sim.handle, st, uid, 40, lp, 5, None, None, None, None, 0.0, o, o, o, o, None, o, o), 'body %d has no frame 40' % uid),
                       ((sim.handle, st, 99, tip, lp, 5, None, None, None, None, 0.0, o, o, o, o, None, o, o), 'body 99 out of range'),
                       ((sim.handle, None, uid, tip, lp, 5, None, None, None, None, 0.0, o, o, o, o, None, o, o), 'null argument'),
                       ((floating.sim.handle, fst, floating.models['cart'].uid, 0, lp, 1, None, None, None, None, 0.0, o, o, o, o, None, o, o),
                        'body %d has a floating base; the dynamics queries take fixed-base bodies only' % floating.models['cart'].uid)):
        assert entry(*args) == -4
        assert lib.dg_last_error().decode() == T + text
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert all(torch.equal(a, b) for a, b in zip(kept, before))
