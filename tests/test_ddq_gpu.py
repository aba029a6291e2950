"""env.sim.forward_dynamics_derivatives (dg_world_dynamics_derivatives / dynamics_derivatives_kernel) on the GPU against the fp64
reference of tests/ddq_ref.py (itself pinned by tests/test_ddq_ref.py): the kernel's derivatives are analytic, the reference's are
central differences of the fp64 model.

Scenes, as tests/test_fd_gpu.py: a pendulum, a double pendulum, the branching cart bolted down (prismatic joint, two branches), a
UR5 (also with DG_MAX_LANES 4 and 1: the global-workspace mode), the UR5s whose link masses a dynamics_randomizer scales per env,
and the twelve-joint UR5 + gripper tree in its one-env-per-wavefront mode.  (B, P) of (1, 1), (3, 5), (3, 50) and (70, 5): with
(3, 50) the 150 items leave a ragged tail; with (70, 5) and DG_MAX_LANES 4 the capped grid (two workgroups for 350 items) makes every
lane stride.  The points are rows of ONE pool per scene drawn as test_fd_gpu.draws draws them (q in [-pi, pi] and inside the limits,
qd in [-2, 2], tau in [-3, 3]); item i of a case takes row i modulo the pool's size, so the reference of a row is computed once per
session for every case and lane mode that shares it.  The pool has 350 rows for the short chains, 60 for the six-axis arms and 24 for
the twelve-joint tree, whose fp64 reference costs 0.07 s and 0.36 s a point (8 n evaluations of the model): every item of every
case is still launched and checked against its own reference, on fewer DISTINCT points (ur_randomized keeps a reference per env and
point, its masses differing per env).  Joint damping is on.

Error measure per item and matrix: max |gpu - ref| / max |ref| of that matrix; the dqdd_* figures and qdd are also divided by the fp64
cond(M).  No item is left out; singular == 0 everywhere.  A matrix whose reference is identically zero (below 1e-9, the noise of the
reference's differences: the pendulum's velocity terms) must be met to 1e-6 absolute.

Ceilings, fixed before anything was measured: dtau_* below 1e-4 (what tests/test_dynamics_queries_gpu.py states for twelve links in
fp32); qdd and dqdd_* below 16 x the qdd figure tests/test_fd_gpu.py records for the group (5.92e-8 arms, 4.52e-6 short chains):
twice that file's margin, because the right-hand sides now come from a second pass of the same length.  The working bounds are 8 x
the largest figure measured on an MI355X (MEASURED; DESIGN.md "Dynamics derivatives" has the table), never above a ceiling.

The point of evaluation.  dtau_dq is taken at FIXED qdd, and the qdd output is fq_solve's fp32 result, which for the twelve-joint
gripper tree is 2.7e-4 off relative to its largest entry (cond M 1.45e6: composite inertias about the base origin cost the fingers,
1e-6 kg m^2 a metre out, digits by cancellation).  At torques of +-3 N m the fingers' qdd reaches 3.7e5 rad/s^2, so dtau_dq there is
d(M qdd)/dq almost alone and would carry that error undivided: taken at fq_solve's qdd it measured 1.59e-4 (on a pool of 350 points),
above its ceiling.  The kernel therefore refines qdd once against the Newton-Euler residual before the sweeps (dg_ddq.h, phase B0;
the qdd output is untouched), which brought the tree's dtau_dq to 1.28e-6 and the arms' from 1.76e-5 to 2.83e-6 on those points.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import ddq_ref as DD
import dynamics_ref as D
import fd_ref as FD
import test_fd_gpu as TF
from diy_gym_amd import DIYGym
from diy_gym_amd.backend import DynamicsDerivatives
from diy_gym_amd.scene import K as KC
from test_fd_gpu import DEV, G, GOLDEN, GROUP, SCENES, dev, make

pytestmark = pytest.mark.gpu
MATS = ('dqdd_dq', 'dqdd_dqd', 'dqdd_dtau', 'dtau_dq', 'dtau_dqd')
FIELDS = ('qdd', ) + MATS
BY_COND = ('qdd', 'dqdd_dq', 'dqdd_dqd', 'dqdd_dtau')
CEILING = {g: dict({k: 16 * TF.MEASURED[g]['qdd'] for k in BY_COND}, dtau_dq=1e-4, dtau_dqd=1e-4) for g in ('arms', 'short')}
# measured maxima (MI355X, all cases of this file, every lane mode of ur_admittance the same figures) and the bounds 8 x them
MEASURED = {
    # qdd, dqdd_dtau, dtau_dq: ur_randomized x70 P=5; dqdd_dq, dqdd_dqd: ur_randomized x3 P=50; dtau_dqd: ur_admittance x3 P=5 (ur5_gripper: dtau_dq 1.11e-6, dtau_dqd 2.23e-6,
    # the others below 1.2e-10 after the division by cond M)
    'arms': {'qdd': 6.82e-8, 'dqdd_dq': 6.99e-8, 'dqdd_dqd': 5.70e-8, 'dqdd_dtau': 8.60e-8, 'dtau_dq': 3.90e-6, 'dtau_dqd': 3.32e-6},
    # qdd, dqdd_dq, dtau_dq: the pendulum (1 x 1 matrices: an item whose cos q nearly vanishes has a small largest entry); the others: double_pendulum
    'short': {'qdd': 1.52e-5, 'dqdd_dq': 1.41e-5, 'dqdd_dqd': 4.64e-6, 'dqdd_dtau': 1.96e-6, 'dtau_dq': 1.38e-5, 'dtau_dqd': 2.01e-5},
}
BOUND = {g: {k: min(8 * v, CEILING[g][k]) for k, v in row.items()} for g, row in MEASURED.items()}
ZERO_REF, ZERO_TOL = 1e-9, 1e-6
BP = ((1, 1), (3, 5), (3, 50), (70, 5))
POOL = {'ur_admittance': 60, 'ur_randomized': 60, 'ur5_gripper': 24}   # distinct points per scene; the others: 350
CASES = [(s, B, P, None) for s in SCENES for B, P in BP] + [('ur_admittance', B, P, lanes) for lanes in ('4', '1') for B, P in BP]
_POOLS, _REFS = {}, {}


def pool(scene, robot):
    """The scene's POOL points: q, qd, tau [POOL, n] fp32."""
    if scene not in _POOLS:
        _POOLS[scene] = TF.draws(robot, POOL.get(scene, 350), 4000 + sorted(SCENES).index(scene))
    return _POOLS[scene]


def pool_rows(scene, B, P):
    """[B, P] pool rows of a case's items."""
    return (np.arange(B * P) % POOL.get(scene, 350)).reshape(B, P)


def points(scene, robot, B, P):
    return tuple(np.ascontiguousarray(a[pool_rows(scene, B, P)]) for a in pool(scene, robot))


def reference(scene, B, P, env, model):
    """Per item: (Derivs in fp64 with joint damping on, cond(M)); [B][P] lists.  A row of the pool whose env has the same base
    frame and mass scales as an earlier one's is not computed again."""
    robot, uid = model.robot, model.uid
    Tb, scales = D.base_transforms(env, uid), D.mass_scales(env, uid)
    q, qd, tau = points(scene, robot, B, P)
    idx = pool_rows(scene, B, P)
    out = []
    for e in range(B):
        row = []
        for p in range(P):
            key = (scene, int(idx[e, p]), np.round(Tb[e].p, 9).tobytes(), np.asarray(Tb[e].R).tobytes(), scales[e].tobytes())
            if key not in _REFS:
                d = DD.derivatives(robot, q[e, p].astype(np.float64), qd[e, p], tau[e, p], True, G, Tb[e], scales[e])
                _REFS[key] = (d, float(np.linalg.cond(D.mass_matrix(robot, q[e, p].astype(np.float64), Tb[e], scales[e]))))
            row.append(_REFS[key])
        out.append(row)
    return (q, qd, tau), out


def figure(gpu, ref):
    """max |gpu - ref| / max |ref|; a reference that is identically zero is met to ZERO_TOL absolute (figure 0)."""
    scale, err = np.abs(ref).max(), np.abs(gpu.astype(np.float64) - ref).max()
    if scale < ZERO_REF:
        assert err <= ZERO_TOL, (err, scale)
        return 0.0
    return err / scale


def check(scene, worst):
    for k, v in worst.items():
        assert v < BOUND[GROUP[scene]][k], (scene, k, v, BOUND[GROUP[scene]][k])


def call(sim, uid, q, qd, tau, damping=True, want=FIELDS + ('singular', )):
    return sim.forward_dynamics_derivatives(uid, dev(q), dev(qd), dev(tau), joint_damping=damping, want=want)


@pytest.mark.parametrize('scene,B,P,lanes', CASES)
def test_derivatives_match_the_reference(scene, B, P, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    if scene == 'ur_randomized':
        scales = D.mass_scales(env, uid)
        assert np.abs(scales - scales[0]).max() > 0.05 if B > 1 else np.abs(scales - 1.0).max() > 0.05   # (scales ignored cannot pass)
    (q, qd, tau), ref = reference(scene, B, P, env, model)
    before = sim.get_state()
    d = call(sim, uid, q, qd, tau)
    assert isinstance(d, DynamicsDerivatives)
    assert d.qdd.shape == (B, P, n) and d.singular.shape == (B, P) and d.singular.dtype == torch.int32 and all(getattr(d, f).shape == (B, P, n, n) for f in MATS)
    assert bool((d.singular == 0).all()) and all(bool(torch.isfinite(getattr(d, f)).all()) for f in FIELDS)
    got = {f: getattr(d, f).cpu().numpy() for f in FIELDS}
    assert np.array_equal(sim.get_state(), before)   # the state is never written
    worst = dict.fromkeys(FIELDS, 0.0)
    for e in range(B):
        for p in range(P):   # no item is left out
            r, cond = ref[e][p]
            for f in FIELDS:
                worst[f] = max(worst[f], figure(got[f][e, p], getattr(r, f)) / (cond if f in BY_COND else 1.0))
    print('%s x%d P=%d lanes=%s grid=%d: %s (cond M up to %.3g)' % (scene, B, P, sim.lanes, sim.rollout_grid(P), ' '.join('%s %.4g' % kv for kv in worst.items()),
                                                                     max(c for row in ref for _, c in row)))
    check(scene, worst)
    if P == 5:
        # M^-1 M = I with the mass-matrix query, and the qdd field is calculate_forward_dynamics
        bound_fd = TF.BOUND[GROUP[scene]]['qdd']
        Minv, qdd = d.dqdd_dtau.clone(), d.qdd.clone()
        for p in range(P):
            M = sim.calculate_mass_matrix(uid, dev(q[:, p])).double()
            cond = np.array([ref[e][p][1] for e in range(B)])
            eye = (Minv[:, p].double() @ M - torch.eye(n, device=DEV, dtype=torch.float64)).abs().amax(dim=(1, 2)).cpu().numpy()
            assert (eye < BOUND[GROUP[scene]]['qdd'] * cond).all(), (scene, p, (eye / cond).max())
            fd = sim.calculate_forward_dynamics(uid, dev(q[:, p]), dev(qd[:, p]), dev(tau[:, p]), joint_damping=True)
            assert (TF.per_row(qdd[:, p].cpu().numpy(), fd.cpu().numpy().astype(np.float64)) / cond).max() < bound_fd


def test_the_capped_grid_of_the_global_workspace_mode_strides(monkeypatch):
    """70 envs x 5 points in the global-workspace mode: the workspace holds the STEP's grid, so the 350 items run as a grid-stride
    loop; the LDS mode takes a workgroup per lanes items (test_derivatives_match_the_reference has the figures of both)."""
    env, model = make('ur_admittance', 70, '4', monkeypatch)
    sim = env.sim
    assert sim.lanes == 0
    step_grid = (70 + 63) // 64
    assert sim.rollout_grid(5) == step_grid < (70 * 5 + 63) // 64
    (q, qd, tau), ref = reference('ur_admittance', 70, 5, env, model)
    d = call(sim, model.uid, q, qd, tau, want=('dqdd_dq', ))
    got = d.dqdd_dq.cpu().numpy().reshape(350, 6, 6)
    errs = np.array([figure(got[i], ref[i // 5][i % 5][0].dqdd_dq) / ref[i // 5][i % 5][1] for i in range(350)])
    assert errs.max() < BOUND['arms']['dqdd_dq'] and errs[300:].max() > 0   # the last stride's items were computed too


@pytest.mark.parametrize('scene,B,lanes', [('cart_tree', 3, None), ('ur_randomized', 70, None), ('ur_admittance', 70, '4'), ('ur5_gripper', 3, None)])
def test_none_inputs_equal_the_explicit_call_in_bits(scene, B, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    L, n = env.layout, robot.num_dofs
    q0, qd0, tau = TF.draws(robot, B, 7, (4, ))
    st = sim.get_state()
    first = L.body_first_link[L.resolve_frame(uid, -1)[0]]
    for i in range(n):
        st[:, L.link_state_off[first + i] + KC.LS_Q] = 0.5 * q0[:, i]; st[:, L.link_state_off[first + i] + KC.LS_QD] = 0.2 * qd0[:, i]
    sim.set_state(st)
    q, qd = (t.clone() for t in sim.joint_states(uid))
    assert float(q.abs().max()) > 0
    want = FIELDS + ('singular', )
    for damping in (False, True):
        implicit = [t.clone() for t in sim.forward_dynamics_derivatives(uid, joint_damping=damping, want=want)]
        assert implicit[1].shape == (B, n, n) and implicit[0].shape == (B, n) and implicit[6].shape == (B, )
        explicit = sim.forward_dynamics_derivatives(uid, q, qd, torch.zeros_like(q), joint_damping=damping, want=want)
        assert all(torch.equal(a, b) for a, b in zip(implicit, explicit))
        # P points of torque at the env's own state: q, qd = None stands for every point of the env
        implicit = [t.clone() for t in sim.forward_dynamics_derivatives(uid, tau=dev(tau), joint_damping=damping, want=want)]
        rows = lambda t: t[:, None, :].expand(B, 4, n).contiguous()
        explicit = sim.forward_dynamics_derivatives(uid, rows(q), rows(qd), dev(tau), joint_damping=damping, want=want)
        assert implicit[1].shape == (B, 4, n, n) and all(torch.equal(a, b) for a, b in zip(implicit, explicit))
    # one [nv] vector stands for every env; [B, nv] is the P = 1 call without its axis
    one = [t.clone() for t in sim.forward_dynamics_derivatives(uid, q[0].clone(), qd[0].clone(), want=want)]
    flat = lambda t: t[0:1].expand(B, n).contiguous()
    assert all(torch.equal(a, b) for a, b in zip(one, sim.forward_dynamics_derivatives(uid, flat(q), flat(qd), want=want)))
    two = [t.clone() for t in sim.forward_dynamics_derivatives(uid, q, qd, dev(tau[:, 0]), want=want)]
    three = sim.forward_dynamics_derivatives(uid, q[:, None].contiguous(), qd[:, None].contiguous(), dev(tau[:, 0:1]), want=want)
    assert all(torch.equal(a, b[:, 0]) for a, b in zip(two, three))
    assert np.array_equal(sim.get_state(), st.astype(np.float32))   # the state is never written


@pytest.mark.parametrize('scene,lanes', [('ur_admittance', None), ('ur_admittance', '4'), ('cart_tree', None), ('ur5_gripper', None)])
def test_a_point_of_many_is_the_single_point_call_in_bits(scene, lanes, monkeypatch):
    """No lane depends on its neighbours, on its position in the wavefront or on the trips it made before."""
    B, P = 3, 50
    env, model = make(scene, B, lanes, monkeypatch)
    sim, uid = env.sim, model.uid
    q, qd, tau = points(scene, model.robot, B, P)
    many = [t.clone() for t in call(sim, uid, q, qd, tau)]
    for p in (0, 21, 49):
        one = call(sim, uid, q[:, p:p + 1], qd[:, p:p + 1], tau[:, p:p + 1])
        assert all(torch.equal(a[:, p:p + 1], b) for a, b in zip(many, one)), p


def test_want_selects_the_fields_and_buffers_are_reused(monkeypatch):
    env, model = make('ur_admittance', 3, None, monkeypatch)
    sim, uid = env.sim, model.uid
    q, qd, tau = points('ur_admittance', model.robot, 3, 5)
    every = FIELDS + ('singular', )
    full = DynamicsDerivatives(*[t.clone() for t in call(sim, uid, q, qd, tau, want=every)])
    default = sim.forward_dynamics_derivatives(uid, dev(q), dev(qd), dev(tau), joint_damping=True)
    assert [f for f in DynamicsDerivatives._fields if getattr(default, f) is not None] == ['dqdd_dq', 'dqdd_dqd', 'dqdd_dtau']
    # every subset gives the same bits: the raw columns go through dtau_* or through dqdd_* itself
    for want in (('qdd', ), ('singular', ), ('dqdd_dq', ), ('dqdd_dqd', ), ('dqdd_dtau', ), ('dtau_dq', ), ('dtau_dqd', ), ('dqdd_dq', 'dtau_dq'), ('dqdd_dqd', 'dtau_dqd'),
                 ('dqdd_dq', 'dqdd_dqd', 'dqdd_dtau'), ('qdd', 'dtau_dq', 'dqdd_dqd')):
        sub = call(sim, uid, q, qd, tau, want=want)
        for f in DynamicsDerivatives._fields:
            assert (getattr(sub, f) is None) == (f not in want)
            assert getattr(sub, f) is None or torch.equal(getattr(sub, f), getattr(full, f)), (want, f)
    a = call(sim, uid, q, qd, tau, want=('dqdd_dq', ))
    b = call(sim, uid, q, qd, 0.5 * tau, want=('dqdd_dq', ))
    assert a.dqdd_dq.data_ptr() == b.dqdd_dq.data_ptr()   # kept per (body, want, P) and reused
    c = call(sim, uid, q[:, :2], qd[:, :2], tau[:, :2], want=('dqdd_dq', ))
    assert c.dqdd_dq.data_ptr() != a.dqdd_dq.data_ptr() and c.dqdd_dq.shape == (3, 2, 6, 6)
    e = call(sim, uid, q, qd, tau, want=('dqdd_dq', 'qdd'))
    assert e.dqdd_dq.data_ptr() != a.dqdd_dq.data_ptr()


@pytest.mark.parametrize('scene', ['ur_admittance', 'cart_tree', 'ur5_gripper'])
def test_joint_damping_shifts_the_diagonal_of_dtau_dqd_by_the_urdf_damping(scene, monkeypatch):
    env, model = make(scene, 3, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    damping = FD.joint_damping(robot)
    assert (damping.max() > 0) == (scene == 'cart_tree')   # (the UR5's URDF has none: the shift is zero and the two calls are the same bits)
    q, qd, tau = points(scene, robot, 3, 5)
    off = {f: getattr(call(sim, uid, q, qd, tau, damping=False, want=('dtau_dq', 'dtau_dqd', 'dqdd_dtau')), f).clone() for f in ('dtau_dq', 'dtau_dqd', 'dqdd_dtau')}
    on = call(sim, uid, q, qd, tau, damping=True, want=('dtau_dq', 'dtau_dqd', 'dqdd_dtau'))
    assert torch.equal(on.dqdd_dtau, off['dqdd_dtau'])
    shift = (on.dtau_dqd - off['dtau_dqd']).cpu().numpy().astype(np.float64)
    scale = float(off['dtau_dqd'].abs().max())
    assert np.abs(shift - np.diag(damping)).max() <= 4 * 2.0 ** -23 * max(scale, damping.max())   # one fp32 addition on the diagonal, nothing elsewhere
    # dtau_dq at fixed qdd changes only through qdd (the damping moves it)
    assert torch.equal(on.dtau_dq, off['dtau_dq']) == (damping.max() == 0)


def test_refusals_raise_value_error_with_the_entrys_text_and_launch_nothing(monkeypatch):
    env, model = make('cart_tree', 3, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    q, qd, tau = (dev(a) for a in points('cart_tree', robot, 3, 4))
    every = FIELDS + ('singular', )
    kept = list(sim.forward_dynamics_derivatives(uid, q, qd, tau, want=every))
    before = [t.clone() for t in kept]
    floating = DIYGym(os.path.join(GOLDEN, 'cart_tree.yaml'), num_envs=3, device=DEV)   # a floating TREE: refused
    plane = DIYGym(os.path.join(GOLDEN, 'ur5_gripper.yaml'), num_envs=3, device=DEV)
    E = 'dg_world_dynamics_derivatives: '
    fuid, puid = floating.models['cart'].uid, plane.models['plane'].uid
    f = sim.forward_dynamics_derivatives
    bad = [(lambda: floating.sim.forward_dynamics_derivatives(fuid), 'fixed-base'),
           (lambda: plane.sim.forward_dynamics_derivatives(puid), 'fixed-base'),
           (lambda: f(99), 'out of range'),
           (lambda: f(uid, q, qd, tau, want=()), E + 'every output is NULL'),
           (lambda: f(uid, q, qd, tau, want=('jac', )), 'want'),
           (lambda: f(uid, q[:, :0].contiguous(), qd[:, :0].contiguous(), tau[:, :0].contiguous()), E + 'P must be >= 1, got 0'),
           (lambda: f(uid, q, qd[:, :2].contiguous(), tau), 'agree on the points per env'),
           (lambda: f(uid, q, qd[:, 0].contiguous(), tau), 'agree on the points per env'),
           (lambda: f(uid, q[:, :, :2].contiguous()), 'shape'),
           (lambda: f(uid, q[:2].contiguous()), 'shape'),
           (lambda: f(uid, q[:, 0, :2].contiguous()), 'shape'),
           (lambda: f(uid, q.double()), 'float32'),
           (lambda: f(uid, tau=tau.cpu()), 'cpu'),
           (lambda: f(uid, q.transpose(0, 1)), 'shape'),
           (lambda: f(uid, [0.0, 0.0, 0.0]), 'torch.Tensor')]
    for fn, text in bad:
        with pytest.raises(ValueError) as info:
            fn()
        assert text in str(info.value), (text, str(info.value))
    # the C entry itself: DG_ERR_ARG with its text, nothing launched
    lib, st = sim.lib, ctypes.c_void_p(sim.state.data_ptr())
    out = torch.full((3, 4096), 7.0, device=DEV)
    o, fst, pst = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(floating.sim.state.data_ptr()), ctypes.c_void_p(plane.sim.state.data_ptr())
    outs = (o, o, o, o, o, o, o)
    for args, text in (((sim.handle, st, uid, 0, None, None, None, 0) + outs, 'P must be >= 1, got 0'),
                       ((sim.handle, st, uid, -3, None, None, None, 0) + outs, 'P must be >= 1, got -3'),
                       ((sim.handle, st, uid, 2, None, None, None, 0) + (None, ) * 7, 'every output is NULL'),
                       ((sim.handle, st, 99, 2, None, None, None, 0) + outs, 'body 99 out of range'),
                       ((sim.handle, None, uid, 2, None, None, None, 0) + outs, 'null argument'),
                       ((floating.sim.handle, fst, fuid, 2, None, None, None, 0) + outs,
                        'body %d has a floating base; the dynamics queries take fixed-base bodies only' % fuid)):
        assert lib.dg_world_dynamics_derivatives(*args, None) == -4
        assert lib.dg_last_error().decode() == E + text
    static = ('body %d is part of the frozen static world: it has no joints' % puid, 'body %d has no joints' % puid)
    assert lib.dg_world_dynamics_derivatives(plane.sim.handle, pst, puid, 2, None, None, None, 0, *outs, None) == -4
    assert lib.dg_last_error().decode() in [E + s for s in static]
    # (the entry's last guard, B P n n beyond INT64_MAX / 4, cannot be reached from here: P is an int32, so it takes B n n > 2^30)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert all(torch.equal(a, b) for a, b in zip(kept, before))
