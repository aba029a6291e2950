"""env.sim.joint_states / calculate_jacobian / calculate_inverse_dynamics / calculate_mass_matrix / apply_joint_torque on the GPU
against the fp64 reference of tests/dynamics_ref.py (itself pinned by tests/test_dynamics_ref.py).

Scenes: a pendulum, a double pendulum, the branching cart (prismatic joint, two branches, a frame on a fixed joint; the URDF of
cart_tree.yaml with its base bolted down -- the queries take fixed-base bodies, and cart_tree.yaml's own floating cart is one of
the bodies test_errors sees refused), a UR5, the twelve-joint UR5 + gripper tree (also in the 4-envs-per-wavefront workspace
mode) and the two UR5s whose link masses a dynamics_randomizer scales per env.  Batches of 1, 3 and 70 envs (70 crosses a
wavefront).

Error measure: per env, max |gpu - reference| over the quantity divided by that env's largest |reference| entry; the figure of a
case is the largest over its envs.  The bounds below are 8 x the largest figure measured over all cases of this file on an MI355X
(DESIGN.md "Dynamics queries" has the table); the margin is for a compiler that contracts multiply-adds differently, not for bugs.
Nothing here may exceed 1e-4: twelve links in fp32 give 1e-6 .. 1e-5.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import dynamics_ref as D
from diy_gym_amd import DIYGym
from diy_gym_amd.scene import K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda:0'
# measured maxima (MI355X, all cases of this file): jac_t 1.02e-6 (ur5_gripper x70), jac_r 8.13e-7 (ur5_gripper x70, 4 envs per
# wavefront), M 5.73e-6 (double_pendulum x70), tau 1.92e-6 (ur_admittance x70); Mqdd -- (ID(q, 0, qdd) - ID(q, 0, 0)) - M qdd with the
# kernel's own M, per env over the larger of that env's two torque vectors -- 1.51e-6 (double_pendulum x70)
BOUND = {'jac_t': 8 * 1.02e-6, 'jac_r': 8 * 8.13e-7, 'M': 8 * 5.73e-6, 'tau': 8 * 1.92e-6, 'Mqdd': 8 * 1.51e-6}
assert max(BOUND.values()) < 1e-4
LOCAL = (0.03, -0.02, 0.05)
G = (0.0, 0.0, -9.81)
# scene -> (config, model); every scene at 1, 3 and 70 envs, ur5_gripper also with DG_MAX_LANES=4
SCENES = {
    'pendulum': ('pendulum.yaml', 'pend'), 'double_pendulum': ('double_pendulum.yaml', 'dp'), 'cart_tree': ('cart_tree_fixed.yaml', 'cart'),
    'ur_admittance': ('ur_admittance.yaml', 'arm'), 'ur5_gripper': ('ur5_gripper.yaml', 'arm'), 'ur_randomized': ('ur_randomized.yaml', 'ur5_r'),
}
CASES = [(s, B, None) for s in SCENES for B in (1, 3, 70)] + [('ur5_gripper', B, '4') for B in (1, 3, 70)]
_ENVS = {}


def make(scene, B, lanes, monkeypatch):
    """The env of a case, built once per session; ``lanes``: DG_MAX_LANES while the world is created."""
    key = (scene, B, lanes)
    if key not in _ENVS:
        if lanes:
            monkeypatch.setenv('DG_MAX_LANES', lanes)
        env = DIYGym(os.path.join(GOLDEN, SCENES[scene][0]), num_envs=B, device=DEV, seed=5)
        if lanes:
            assert env.sim.envs_per_wave == int(lanes)
        _ENVS[key] = env
    env = _ENVS[key]
    return env, env.models[SCENES[scene][1]]


def draws(robot, B, seed):
    """Per-env q inside the joint limits, qd, qdd -- fp32 values, as the kernels get them."""
    rng = np.random.default_rng(seed)
    lim = D.joint_limits(robot)
    n = robot.num_dofs
    return (rng.uniform(lim[:, 0], lim[:, 1], (B, n)).astype(np.float32), rng.uniform(-2.0, 2.0, (B, n)).astype(np.float32),
            rng.uniform(-5.0, 5.0, (B, n)).astype(np.float32))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def figure(gpu, ref):
    """The file's error measure; a reference that is all zero in an env must be met exactly there."""
    gpu, ref = gpu.reshape(gpu.shape[0], -1).astype(np.float64), ref.reshape(ref.shape[0], -1)
    scale = np.abs(ref).max(axis=1)
    err = np.abs(gpu - ref).max(axis=1)
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0


def frames_of(robot, B):
    every = list(range(len(robot.joints)))
    return every if len(every) <= 6 or B <= 3 else every[2::3]   # (the twelve-joint tree at 70 envs: every third frame)


@pytest.mark.parametrize('scene,B,lanes', CASES)
def test_queries_match_the_reference(scene, B, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    q, qd, qdd = draws(robot, B, 100 + B)
    Tb = D.base_transforms(env, uid)
    scales = D.mass_scales(env, uid)
    if scene == 'ur_randomized':
        assert np.abs(scales - scales[0]).max() > 0.05 if B > 1 else np.abs(scales - 1.0).max() > 0.05   # (scales ignored cannot pass)
    else:
        assert (scales == 1.0).all()
    worst = dict.fromkeys(('jac_t', 'jac_r', 'M', 'tau'), 0.0)
    # ---- Jacobians: every frame (fixed joints included), a point off the inertial origin
    for frame in frames_of(robot, B):
        jt, jr = sim.calculate_jacobian(uid, frame, LOCAL, dev(q))
        assert jt.shape == (B, 3, n) and jr.shape == (B, 3, n)
        jt, jr = jt.cpu().numpy(), jr.cpu().numpy()
        ref = [D.jacobian(robot, q[e].astype(np.float64), frame, LOCAL, Tb[e]) for e in range(B)]
        rt, rr = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
        anc = D.ancestors(robot, robot.joints[frame].child)
        off = [k for k in range(n) if k not in anc]
        assert (jt[:, :, off] == 0).all() and (jr[:, :, off] == 0).all(), (scene, frame)   # not ancestors: exactly zero
        worst['jac_t'] = max(worst['jac_t'], figure(jt, rt)); worst['jac_r'] = max(worst['jac_r'], figure(jr, rr))
    # ---- mass matrix
    M = sim.calculate_mass_matrix(uid, dev(q)).cpu().numpy()
    assert M.shape == (B, n, n) and (M.view(np.uint32) == M.transpose(0, 2, 1).view(np.uint32)).all()   # symmetric in bits
    worst['M'] = figure(M, np.stack([D.mass_matrix(robot, q[e].astype(np.float64), Tb[e], scales[e]) for e in range(B)]))
    # ---- inverse dynamics: the full call, gravity compensation alone, and M qdd as a difference of two calls
    zero = np.zeros_like(q)
    for a, b, c in ((q, qd, qdd), (q, zero, zero), (q, zero, qdd)):
        tau = sim.calculate_inverse_dynamics(uid, dev(a), dev(b), dev(c)).cpu().numpy()
        ref = np.stack([D.inverse_dynamics(robot, a[e].astype(np.float64), b[e], c[e], G, Tb[e], scales[e]) for e in range(B)])
        worst['tau'] = max(worst['tau'], figure(tau, ref))
    t_acc = sim.calculate_inverse_dynamics(uid, dev(q), dev(zero), dev(qdd)).cpu().numpy().astype(np.float64)
    t_rest = sim.calculate_inverse_dynamics(uid, dev(q), dev(zero), None).cpu().numpy().astype(np.float64)   # (qdd None: zero)
    Mqdd = np.einsum('bij,bj->bi', M.astype(np.float64), qdd.astype(np.float64))
    # per env, over that env's own scale: the larger of its two torque vectors (what the difference is a difference of)
    scale = np.maximum(np.abs(t_acc).max(axis=1), np.abs(t_rest).max(axis=1))
    worst['Mqdd'] = float((np.abs((t_acc - t_rest) - Mqdd).max(axis=1) / scale).max())
    print('%s x%d lanes=%s: %s' % (scene, B, sim.lanes, ' '.join('%s %.4g' % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v < BOUND[k], (scene, B, k, v)


@pytest.mark.parametrize('scene,B,lanes', CASES)
def test_current_state_equals_the_explicit_call_bit_for_bit(scene, B, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    L, n = env.layout, robot.num_dofs
    # joints off their rest pose and moving, then five steps of random actions
    q0, qd0, _ = draws(robot, B, 7)
    st = sim.get_state()
    first = L.body_first_link[uid]
    for i in range(n):
        st[:, L.link_state_off[first + i] + K.LS_Q] = 0.5 * q0[:, i]; st[:, L.link_state_off[first + i] + K.LS_QD] = 0.2 * qd0[:, i]
    sim.set_state(st)
    gen = torch.Generator().manual_seed(3)
    for _ in range(5):
        sim.step(env._all_slots, ((torch.rand((B, max(L.act_dim, 1)), generator=gen) * 2 - 1) * 0.3).to(DEV))
    q, qd = (t.clone() for t in sim.joint_states(uid))
    st = sim.get_state()
    for i in range(n):
        assert (q[:, i].cpu().numpy() == st[:, L.link_state_off[first + i] + K.LS_Q]).all() and (qd[:, i].cpu().numpy() == st[:, L.link_state_off[first + i] + K.LS_QD]).all()
    assert float(q.abs().max()) > 0   # (off the zero pose; the default velocity motors may well have stopped the joints)
    frame = len(robot.joints) - 1
    for implicit, explicit in ((lambda: sim.calculate_jacobian(uid, frame, LOCAL), lambda: sim.calculate_jacobian(uid, frame, LOCAL, q)),
                               (lambda: (sim.calculate_mass_matrix(uid), ), lambda: (sim.calculate_mass_matrix(uid, q), )),
                               (lambda: (sim.calculate_inverse_dynamics(uid), ), lambda: (sim.calculate_inverse_dynamics(uid, q, qd, torch.zeros_like(q)), )),
                               (lambda: (sim.calculate_inverse_dynamics(uid, qd=torch.zeros_like(q)), ), lambda: (sim.calculate_inverse_dynamics(uid, q, torch.zeros_like(q)), ))):
        a = [t.clone() for t in implicit()]
        b = explicit()
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(bool(torch.isfinite(x).all()) for x in a)
    # one [nv] vector stands for every env
    one = sim.calculate_inverse_dynamics(uid, q[0].clone(), qd[0].clone()).clone()
    assert torch.equal(one, sim.calculate_inverse_dynamics(uid, q[0:1].expand(B, n).contiguous(), qd[0:1].expand(B, n).contiguous()))
    assert torch.equal(one[0], sim.calculate_inverse_dynamics(uid)[0])   # (env 0's own state)


@pytest.mark.parametrize('scene,B', [('cart_tree', 3), ('ur_randomized', 70), ('ur5_gripper', 70)])
def test_apply_joint_torque_round_trip(scene, B, monkeypatch):
    env, model = make(scene, B, None, monkeypatch)
    sim, L, uid = env.sim, env.layout, model.uid
    n, first = model.robot.num_dofs, L.body_first_link[uid]
    sim.step(0)   # (whatever earlier tests applied is consumed)
    cols = [L.link_state_off[l] + K.LS_TORQUE for l in range(L.n_links)]
    mine = cols[first:first + n]
    assert (sim.get_state()[:, cols] == 0).all()
    tau = dev(np.random.default_rng(2).uniform(-3.0, 3.0, (B, n)).astype(np.float32))
    sim.apply_joint_torque(uid, tau)
    st = sim.get_state()
    assert (st[:, mine] == tau.cpu().numpy()).all()
    assert (st[:, [c for c in cols if c not in mine]] == 0).all()   # the other body's joints: untouched
    sim.apply_joint_torque(uid, tau)
    assert (sim.get_state()[:, mine] == (tau + tau).cpu().numpy()).all()   # a second call adds
    sim.apply_joint_torque(uid, tau[0].clone())   # one [nv] vector for every env
    assert (sim.get_state()[:, mine] == ((tau + tau) + tau[0:1]).cpu().numpy()).all()
    sim.step(0)
    assert (sim.get_state()[:, cols] == 0).all()   # consumed by one step


def test_errors_raise_and_leave_the_outputs_alone(monkeypatch):
    env, model = make('ur5_gripper', 3, None, monkeypatch)
    sim, uid, n = env.sim, model.uid, model.robot.num_dofs
    q = dev(draws(model.robot, 3, 1)[0])
    kept = [t for t in (*sim.calculate_jacobian(uid, 3, LOCAL, q), sim.calculate_mass_matrix(uid, q), sim.calculate_inverse_dynamics(uid, q), *sim.joint_states(uid))]
    before = [t.clone() for t in kept]
    plane = env.models['plane'].uid   # frozen into the static world
    floating = DIYGym(os.path.join(GOLDEN, 'box_stack.yaml'), num_envs=3, device=DEV)
    cart = DIYGym(os.path.join(GOLDEN, 'cart_tree.yaml'), num_envs=3, device=DEV)   # a floating TREE: out of scope, refused
    calls = lambda s, b, nv: [lambda: s.joint_states(b), lambda: s.calculate_jacobian(b, 0), lambda: s.calculate_inverse_dynamics(b),
                              lambda: s.calculate_mass_matrix(b), lambda: s.apply_joint_torque(b, torch.zeros((3, nv), device=DEV))]
    for s, b, nv in ((sim, plane, 1), (floating.sim, floating.models['lower'].uid, 1), (floating.sim, floating.models['upper'].uid, 1),
                     (cart.sim, cart.models['cart'].uid, 3), (sim, 99, 1)):
        for call in calls(s, b, nv):
            with pytest.raises(ValueError):
                call()
    bad = [lambda: sim.calculate_jacobian(uid, 3, LOCAL, q[:, :n - 1].contiguous()),                     # wrong shape
           lambda: sim.calculate_jacobian(uid, 3, LOCAL, q.double()),                                    # wrong dtype
           lambda: sim.calculate_jacobian(uid, 3, LOCAL, q.cpu()),                                       # wrong device
           lambda: sim.calculate_jacobian(uid, 3, (0.0, 0.0)),                                           # local_pos
           lambda: sim.calculate_jacobian(uid, len(model.robot.joints), LOCAL, q),                       # frame out of range
           lambda: sim.calculate_jacobian(uid, -1, LOCAL, q),                                            # the base
           lambda: sim.calculate_inverse_dynamics(uid, q, q[:2].contiguous()), lambda: sim.calculate_inverse_dynamics(uid, q, None, q.half()),
           lambda: sim.calculate_mass_matrix(uid, q.reshape(-1)), lambda: sim.calculate_mass_matrix(uid, [0.0] * n),
           lambda: sim.apply_joint_torque(uid, q.double()), lambda: sim.apply_joint_torque(uid, q[:, :3].contiguous()), lambda: sim.apply_joint_torque(uid, None)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    # the C entries themselves: DG_ERR_ARG, nothing launched
    lib, st = sim.lib, ctypes.c_void_p(floating.sim.state.data_ptr())
    out = torch.full((3, 64), 7.0, device=DEV)
    o = ctypes.c_void_p(out.data_ptr())
    lp = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    fb = floating.models['lower'].uid
    assert lib.dg_world_joint_state(floating.sim.handle, st, fb, o, o, None) == -4
    assert lib.dg_world_jacobian(floating.sim.handle, st, fb, 0, lp, None, o, o, None) == -4
    assert lib.dg_world_inverse_dynamics(floating.sim.handle, st, fb, None, None, None, o, None) == -4
    assert lib.dg_world_mass_matrix(floating.sim.handle, st, fb, None, o, None) == -4
    assert lib.dg_world_apply_joint_torque(floating.sim.handle, st, fb, o, None) == -4 and b'floating' in lib.dg_last_error()
    assert lib.dg_world_jacobian(sim.handle, ctypes.c_void_p(sim.state.data_ptr()), uid, 40, lp, None, o, o, None) == -4 and b'frame' in lib.dg_last_error()
    # (the frozen plane reaches the C check only this way: Python refuses it first)
    for call in (lambda: lib.dg_world_joint_state(sim.handle, ctypes.c_void_p(sim.state.data_ptr()), plane, o, o, None),
                 lambda: lib.dg_world_inverse_dynamics(sim.handle, ctypes.c_void_p(sim.state.data_ptr()), plane, None, None, None, o, None),
                 lambda: lib.dg_world_apply_joint_torque(sim.handle, ctypes.c_void_p(sim.state.data_ptr()), plane, o, None)):
        assert call() == -4 and b'frozen' in lib.dg_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert all(torch.equal(a, b) for a, b in zip(kept, before))
