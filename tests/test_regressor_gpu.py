"""env.sim.inertial_parameters and env.sim.inverse_dynamics_regressor (dg_world_inertial_parameters / inertial_params_kernel,
dg_world_id_regressor / id_regressor_kernel) on the GPU against the fp64 reference of tests/regressor_ref.py (itself pinned by
tests/test_regressor_ref.py).

Scenes and lane modes, as tests/test_fd_gpu.py: a pendulum, a double pendulum, the branching cart bolted down (prismatic joint, two
branches), a UR5 (also with DG_MAX_LANES 4 and 1, which put it in the global-workspace mode, Lane<0>), the UR5s whose link masses a
dynamics_randomizer scales per env, and the twelve-joint UR5 + gripper tree.  (B, P) of (1, 1), (3, 5), (3, 50) and (70, 5): with
B = 3 and P = 50 the 150 items straddle wavefronts and leave a ragged tail, and with B = 70, P = 5 and DG_MAX_LANES 4 the grid cap of
the global-workspace mode makes every lane stride through the item list.  Inputs: test_fd_gpu's draws (q in [-pi, pi] and inside the
joint limits, qd in [-2, 2], qdd in [-3, 3]), q and qd per point around them, a qd_ref drawn like qd, a theta_hat within +-50 % of
the truth, s in [-1, 1].

Error measure, per item (env, point): max |gpu - reference| / max |reference| over the item's output (Y: the whole [nv, 10 nv]
matrix; tau; grad).  No item is left out.  Blocks of Y that belong to links a joint does not carry must be exactly 0.  The figure of
a case is the largest over its items, in the plain form and with qd_ref.  Ceiling, fixed before anything was measured: 1e-4, what
tests/test_dynamics_queries_gpu.py grants fp32 inverse dynamics on twelve links.  The working bounds are 8 x the largest figure
measured over all cases of this file on an MI355X per group ('short': pendulum, double pendulum, cart; 'arms': the six-axis arms and
the gripper tree), never above the ceiling; DESIGN.md "Inverse-dynamics regressor" has the table.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import dynamics_ref as D
import regressor_ref as RR
import test_fd_gpu as TF
from diy_gym_amd.backend import DynamicsRegressor

pytestmark = pytest.mark.gpu
DEV = TF.DEV
G = TF.G
CEILING = 1e-4
# measured maxima (MI355X, all cases of this file, the plain form and the one with qd_ref) and the bounds: 8 x them, never above the ceiling
MEASURED = {
    # Y, grad: ur5_gripper x70 P=5; tau: ur_admittance x70 P=5 (every mode the same figures)
    'arms': {'Y': 3.62e-6, 'tau': 2.07e-6, 'grad': 3.97e-6},
    # Y: double_pendulum x3 P=50; grad: double_pendulum x70 P=5; tau: double_pendulum x70 P=5 and pendulum x70 P=5 (2.15e-5) -- items whose
    # inertial and gravity torques nearly cancel under the random theta_hat, so the item's largest |reference| entry is small; 8 x is
    # above the ceiling, which therefore is the bound
    'short': {'Y': 5.35e-7, 'tau': 2.48e-5, 'grad': 5.63e-7},
}
BOUND = {g: {k: min(8 * v, CEILING) for k, v in row.items()} for g, row in MEASURED.items()}
ID_BOUND = 1e-4   # what tests/test_dynamics_queries_gpu.py grants calculate_inverse_dynamics
BP = [(1, 1), (3, 5), (3, 50), (70, 5)]
CASES = [(s, B, P, None) for s in TF.SCENES for B, P in BP] + [('ur_admittance', B, P, lanes) for lanes in ('4', '1') for B, P in BP]
_REFS = {}
dev = TF.dev


def inputs(robot, B, P, seed):
    """fp32 q, qd, qdd, qd_ref, s [B, P, n] and the +-50 % factors of theta_hat [B, n, 10]."""
    n = robot.num_dofs
    q0, qd0, qdd = TF.draws(robot, B, seed, (P, ))
    rng = np.random.default_rng(seed + 7)
    q = (q0[:, None, :] + rng.uniform(-0.3, 0.3, (B, P, n))).astype(np.float32)
    qd = (qd0[:, None, :] * rng.uniform(0.5, 1.0, (B, P, n))).astype(np.float32)
    qd_ref = rng.uniform(-2.0, 2.0, (B, P, n)).astype(np.float32)
    s = rng.uniform(-1.0, 1.0, (B, P, n)).astype(np.float32)
    return q, qd, qdd, qd_ref, s, rng.uniform(0.5, 1.5, (B, n, 10))


def reference(scene, B, P, env, model):
    """(inputs, theta_true [B, n, 10], theta_hat fp32 [B, 10 n], Y plain and with qd_ref [B, P, n, 10 n]) in fp64, computed once (the
    lane modes of a scene share it: the draws and the state are the same)."""
    key = (scene, B, P)
    if key not in _REFS:
        robot, uid = model.robot, model.uid
        Tb, scales = D.base_transforms(env, uid), D.mass_scales(env, uid)
        q, qd, qdd, qd_ref, s, factor = inputs(robot, B, P, 4000 * B + P)
        theta = np.stack([RR.theta(robot, scales[e]) for e in range(B)])
        theta_hat = (theta * factor).reshape(B, -1).astype(np.float32)
        Y = np.stack([[RR.regressor(robot, q[e, p].astype(np.float64), qd[e, p], qdd[e, p], None, G, Tb[e]) for p in range(P)] for e in range(B)])
        Yr = np.stack([[RR.regressor(robot, q[e, p].astype(np.float64), qd[e, p], qdd[e, p], qd_ref[e, p], G, Tb[e]) for p in range(P)] for e in range(B)])
        _REFS[key] = ((q, qd, qdd, qd_ref, s), theta, theta_hat, Y, Yr)
    return _REFS[key]


def carried(robot):
    """[n, n] bool: joint i carries link j (i is j or an ancestor of j)."""
    n = robot.num_dofs
    out = np.zeros((n, n), dtype=bool)
    for j, name in RR.carrier_links(robot).items():
        out[sorted(RR.ancestors(robot, name)), j] = True
    return out


def items(a, B, P):
    return a.reshape((B * P, ) + a.shape[2:])


@pytest.mark.parametrize('scene,B,P,lanes', CASES)
def test_regressor_matches_the_reference(scene, B, P, lanes, monkeypatch):
    env, model = TF.make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    (q, qd, qdd, qd_ref, s), theta, theta_hat, Y, Yr = reference(scene, B, P, env, model)
    mask = np.repeat(carried(robot), 10, axis=1)   # [n, 10 n]
    worst = {'Y': 0.0, 'tau': 0.0, 'grad': 0.0}
    for ref, ref_arg in ((Y, None), (Yr, dev(qd_ref))):
        r = sim.inverse_dynamics_regressor(uid, dev(q), dev(qd), dev(qdd), qd_ref=ref_arg, theta=dev(theta_hat), s=dev(s), want=('Y', 'tau', 'grad'))
        assert isinstance(r, DynamicsRegressor)
        assert r.Y.shape == (B, P, n, 10 * n) and r.tau.shape == (B, P, n) and r.grad.shape == (B, P, 10 * n)
        assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in r)
        gY, gtau, ggrad = (t.cpu().numpy() for t in r)
        assert (gY[:, :, ~mask] == 0).all() and (ref[:, :, ~mask] == 0).all()   # blocks of links a joint does not carry: exactly zero
        tau_ref = np.einsum('bpij,bj->bpi', ref, theta_hat.astype(np.float64))
        grad_ref = np.einsum('bpij,bpi->bpj', ref, s.astype(np.float64))
        for k, g, want in (('Y', gY, ref), ('tau', gtau, tau_ref), ('grad', ggrad, grad_ref)):
            worst[k] = max(worst[k], float(TF.per_row(items(g, B, P), items(want, B, P)).max()))
    print('%s x%d P=%d lanes=%s grid=%d: %s' % (scene, B, P, sim.lanes, sim.rollout_grid(P), ' '.join('%s %.4g' % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v < BOUND[TF.GROUP[scene]][k], (scene, k, v, BOUND[TF.GROUP[scene]][k])


@pytest.mark.parametrize('scene,B,lanes', [(s, B, None) for s in TF.SCENES for B in (3, 70)] + [('ur_admittance', 70, '4')])
def test_the_defaults_and_one_point_shapes(scene, B, lanes, monkeypatch):
    """[B, nv] inputs give [B, nv, 10 nv]; q, qd = None are the env's own, qdd = None is zero, qd_ref = None is qd: the same bits as the
    call given those numbers; a [nv] vector is every env's."""
    env, model = TF.make(scene, B, lanes, monkeypatch)
    sim, uid, n = env.sim, model.uid, model.robot.num_dofs
    q, qd = (t.clone() for t in sim.joint_states(uid))
    a = sim.inverse_dynamics_regressor(uid).Y
    assert a.shape == (B, n, 10 * n)
    a = a.clone()
    b = sim.inverse_dynamics_regressor(uid, q, qd, torch.zeros_like(q), qd_ref=qd).Y
    assert torch.equal(a, b)
    one = torch.linspace(-1.0, 1.0, n, device=DEV)
    c = sim.inverse_dynamics_regressor(uid, q, qd, one).Y.clone()
    d = sim.inverse_dynamics_regressor(uid, q, qd, one.expand(B, n).contiguous()).Y
    assert torch.equal(c, d) and not torch.equal(c, a)


@pytest.mark.parametrize('scene', ['ur_randomized', 'ur5_gripper'])
def test_inertial_parameters_are_the_urdfs_with_the_envs_scales(scene, monkeypatch):
    B = 70
    env, model = TF.make(scene, B, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    scales = D.mass_scales(env, uid)
    if scene == 'ur_randomized':
        assert np.abs(scales - scales[0]).max() > 0.05   # (scales ignored cannot pass)
    theta = sim.inertial_parameters(uid)
    assert theta.shape == (B, n, 10) and theta.dtype == torch.float32
    got = theta.cpu().numpy().astype(np.float64)
    nominal = sim.inertial_parameters(uid, nominal=True)
    assert nominal.data_ptr() != theta.data_ptr() and sim.inertial_parameters(uid).data_ptr() == theta.data_ptr()   # kept per (body, nominal)
    ref0 = RR.theta(robot)
    for e in range(B):
        ref = RR.theta(robot, scales[e])
        assert np.abs(got[e] - ref).max() <= 1e-6 * np.abs(ref).max(), (scene, e)
    got0 = nominal.cpu().numpy().astype(np.float64)
    assert np.abs(got0 - ref0[None]).max() <= 1e-6 * np.abs(ref0).max()
    assert (got0 == got0[0]).all()


@pytest.mark.parametrize('scene,B', [('ur_randomized', 70), ('ur5_gripper', 3), ('cart_tree', 3)])
def test_y_times_the_true_parameters_is_the_inverse_dynamics_kernel(scene, B, monkeypatch):
    """Y @ theta_true (fp64 product on the host, theta from the device query) against calculate_inverse_dynamics, which uses each env's
    own masses: within the sum of the two bounds."""
    env, model = TF.make(scene, B, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    q, qd, qdd = (dev(a) for a in TF.draws(robot, B, 91))
    tau = sim.calculate_inverse_dynamics(uid, q, qd, qdd).cpu().numpy().astype(np.float64)
    Y = sim.inverse_dynamics_regressor(uid, q, qd, qdd).Y.cpu().numpy().astype(np.float64)
    theta = sim.inertial_parameters(uid).cpu().numpy().astype(np.float64).reshape(B, -1)
    prod = np.einsum('bij,bj->bi', Y, theta)
    err = TF.per_row(prod, tau)
    print('%s x%d: Y theta against calculate_inverse_dynamics %.4g' % (scene, B, err.max()))
    assert err.max() < BOUND[TF.GROUP[scene]]['Y'] + ID_BOUND


def test_want_subsets_give_none_fields_and_the_same_bits(monkeypatch):
    env, model = TF.make('ur_admittance', 3, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    (q, qd, qdd, qd_ref, s), theta, theta_hat, _, _ = reference('ur_admittance', 3, 5, env, model)
    args = dict(q=dev(q), qd=dev(qd), qdd=dev(qdd), qd_ref=dev(qd_ref), theta=dev(theta_hat), s=dev(s))
    full = DynamicsRegressor(*[t.clone() for t in sim.inverse_dynamics_regressor(uid, want=('Y', 'tau', 'grad'), **args)])
    for want in (('Y', ), ('tau', ), ('grad', ), ('tau', 'grad'), ('Y', 'grad')):
        r = sim.inverse_dynamics_regressor(uid, want=want, **args)
        for f in DynamicsRegressor._fields:
            if f in want:
                assert torch.equal(getattr(r, f), getattr(full, f)), (want, f)
            else:
                assert getattr(r, f) is None, (want, f)
        assert sim.inverse_dynamics_regressor(uid, want=want, **args) is r   # buffers kept per (body, want, P)
    # theta [B, nv, 10] and [10 nv] are the same parameters
    n = robot.num_dofs
    r3 = sim.inverse_dynamics_regressor(uid, want=('tau', ), **dict(args, theta=dev(theta_hat.reshape(3, n, 10)))).tau
    assert torch.equal(r3, full.tau)
    every = np.tile(theta_hat[:1], (3, 1))
    a = sim.inverse_dynamics_regressor(uid, want=('tau', ), **dict(args, theta=dev(every))).tau.clone()
    b = sim.inverse_dynamics_regressor(uid, want=('tau', ), **dict(args, theta=dev(theta_hat[0]))).tau
    assert torch.equal(a, b)


def test_refusals(monkeypatch):
    env, model = TF.make('ur_admittance', 3, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    z = torch.zeros((3, n), device=DEV)
    with pytest.raises(ValueError, match="'tau' in want needs theta"):
        sim.inverse_dynamics_regressor(uid, want=('tau', ))
    with pytest.raises(ValueError, match="'grad' in want needs s"):
        sim.inverse_dynamics_regressor(uid, want=('grad', ))
    with pytest.raises(ValueError, match='want must name some of'):
        sim.inverse_dynamics_regressor(uid, want=('M', ))
    with pytest.raises(ValueError, match='must agree on the points per env'):
        sim.inverse_dynamics_regressor(uid, q=z, qd=torch.zeros((3, 4, n), device=DEV))
    with pytest.raises(ValueError, match='theta must have shape'):
        sim.inverse_dynamics_regressor(uid, theta=torch.zeros((3, 10 * n + 1), device=DEV), want=('tau', ))
    # the entry's own refusals, with their texts, before any launch
    lib, st = sim.lib, ctypes.c_void_p(sim.state.data_ptr())
    body = sim._dyn_body(uid)[0]
    out = torch.full((3, n, 10 * n), 7.0, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(P=1, theta_hat=None, s=None, Y=None, tau=None, grad=None, b=body, state=st):
        return lib.dg_world_id_regressor(sim.handle, state, b, P, None, None, None, None, p(theta_hat), p(s), p(Y), p(tau), p(grad), None)
    for kw, text in ((dict(state=None, Y=out), 'dg_world_id_regressor: null argument'),
                     (dict(P=0, Y=out), 'dg_world_id_regressor: P must be >= 1, got 0'),
                     (dict(), 'dg_world_id_regressor: every output is NULL'),
                     (dict(tau=z), 'dg_world_id_regressor: tau needs theta_hat'),
                     (dict(grad=out), 'dg_world_id_regressor: grad needs s'),
                     (dict(Y=out.view(-1)[1:]), 'dg_world_id_regressor: Y and grad must be 8-byte aligned'),
                     (dict(grad=out.view(-1)[1:], s=z), 'dg_world_id_regressor: Y and grad must be 8-byte aligned'),
                     (dict(b=99, Y=out), 'dg_world_id_regressor: body 99 out of range')):
        assert call(**kw) == -4 and lib.dg_last_error().decode() == text, (kw, lib.dg_last_error())
    assert lib.dg_world_inertial_parameters(sim.handle, st, body, 0, None, None) == -4
    assert lib.dg_last_error().decode() == 'dg_world_inertial_parameters: theta is NULL'
    assert lib.dg_world_inertial_parameters(sim.handle, None, body, 0, p(out), None) == -4
    assert lib.dg_last_error().decode() == 'dg_world_inertial_parameters: null argument'
    assert lib.dg_world_inertial_parameters(sim.handle, st, body, 0, p(out.view(-1)[1:]), None) == -4
    assert lib.dg_last_error().decode() == 'dg_world_inertial_parameters: theta must be 8-byte aligned'
    assert lib.dg_world_inertial_parameters(sim.handle, st, 99, 0, p(out), None) == -4
    assert lib.dg_last_error().decode() == 'dg_world_inertial_parameters: body 99 out of range'
    # dynq_check's bodies, as tests/test_fd_gpu.py has them: a floating TREE (cart_tree.yaml) and a static body (the gripper scene's
    # plane: frozen into the static world, or a fixed base without joints -- whichever the scene made it).  Python's own guard first,
    # then the C entries themselves through the library, with their texts
    floating = TF.DIYGym(os.path.join(TF.GOLDEN, 'cart_tree.yaml'), num_envs=3, device=DEV)
    plane = TF.DIYGym(os.path.join(TF.GOLDEN, 'ur5_gripper.yaml'), num_envs=3, device=DEV)
    fuid, puid = floating.models['cart'].uid, plane.models['plane'].uid
    for other, b in ((floating, fuid), (plane, puid)):
        with pytest.raises(ValueError, match='fixed-base'):
            other.sim.inverse_dynamics_regressor(b)
        with pytest.raises(ValueError, match='fixed-base'):
            other.sim.inertial_parameters(b)
    R, T = 'dg_world_id_regressor: ', 'dg_world_inertial_parameters: '
    fst, pst = ctypes.c_void_p(floating.sim.state.data_ptr()), ctypes.c_void_p(plane.sim.state.data_ptr())
    text = 'body %d has a floating base; the dynamics queries take fixed-base bodies only' % fuid
    assert lib.dg_world_id_regressor(floating.sim.handle, fst, fuid, 1, None, None, None, None, None, None, p(out), None, None, None) == -4
    assert lib.dg_last_error().decode() == R + text
    assert lib.dg_world_inertial_parameters(floating.sim.handle, fst, fuid, 0, p(out), None) == -4
    assert lib.dg_last_error().decode() == T + text
    static = ('body %d is part of the frozen static world: it has no joints' % puid, 'body %d has no joints' % puid)
    assert lib.dg_world_id_regressor(plane.sim.handle, pst, puid, 1, None, None, None, None, None, None, p(out), None, None, None) == -4
    assert lib.dg_last_error().decode() in [R + s for s in static]
    assert lib.dg_world_inertial_parameters(plane.sim.handle, pst, puid, 0, p(out), None) == -4
    assert lib.dg_last_error().decode() in [T + s for s in static]
    # slots_refusal cannot be made to fire from a scene: the planner gives every fixed-base body 12 + 32 n slots of transient region and
    # the pass takes 23 n (tests/test_regressor_cabi.py checks both, and every scene's plan); it is the last check in front of the launch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())   # nothing was launched


def test_identification_of_the_mass_scales_by_least_squares(monkeypatch):
    """ur_randomized, 3 envs, 16 points: tau from 16 calculate_inverse_dynamics calls (each env's own masses), Phi [16 nv, nv] from Y and
    the nominal theta0 (column l: Y's block of link l times theta0_l), s_est by least squares in fp64.  The first-order perturbation
    bound |s_est - s_true| <= 2 (|tau_gpu - tau_ref| + |(Phi_gpu - Phi_ref) s_true|) / sigma_min(Phi_ref) must hold, below 0.05."""
    B, P = 3, 16
    env, model = TF.make('ur_randomized', B, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    Tb, scales = D.base_transforms(env, uid), D.mass_scales(env, uid)
    q, qd, qdd, _, _, _ = inputs(robot, B, P, 555)
    tau_gpu = np.stack([sim.calculate_inverse_dynamics(uid, dev(q[:, p]), dev(qd[:, p]), dev(qdd[:, p])).cpu().numpy() for p in range(P)], axis=1).astype(np.float64)
    Y = sim.inverse_dynamics_regressor(uid, dev(q), dev(qd), dev(qdd)).Y.cpu().numpy().astype(np.float64)
    theta0_gpu = sim.inertial_parameters(uid, nominal=True).cpu().numpy().astype(np.float64)
    theta0 = RR.theta(robot)
    phi = lambda Ye, th: np.einsum('pilk,lk->pil', Ye.reshape(P, n, n, 10), th).reshape(P * n, n)
    for e in range(B):
        Y_ref = np.stack([RR.regressor(robot, q[e, p].astype(np.float64), qd[e, p], qdd[e, p], None, G, Tb[e]) for p in range(P)])
        Phi_ref, Phi_gpu = phi(Y_ref, theta0), phi(Y[e], theta0_gpu[e])
        tau_ref = Phi_ref @ scales[e]
        sigma = np.linalg.svd(Phi_ref, compute_uv=False)
        assert sigma[-1] >= 0.01, sigma
        s_est = torch.linalg.lstsq(torch.as_tensor(Phi_gpu), torch.as_tensor(tau_gpu[e].reshape(-1, 1))).solution[:, 0].numpy()
        bound = 2.0 * (np.linalg.norm(tau_gpu[e].reshape(-1) - tau_ref) + np.linalg.norm((Phi_gpu - Phi_ref) @ scales[e])) / sigma[-1]
        err = np.linalg.norm(s_est - scales[e])
        print('env %d: |s_est - s_true| %.3g, bound %.3g, sigma_min %.3g, cond %.3g' % (e, err, bound, sigma[-1], sigma[0] / sigma[-1]))
        assert err <= bound and err < 0.05 and bound < 0.05, (e, err, bound)
