"""env.sim.calculate_inverse_kinematics / set_joint_motor_targets / reset_joint_state on the GPU.

1. The query against the fp64 reference of tests/ik_ref.py (itself pinned by tests/test_ik_ref.py), in worlds built with
   ``engine={'ik_residual': 0.0}``: both sides then run exactly ``ik_iterations`` iterations and no fp32 / fp64 flip of the early
   exit can enter.  Scenes and frames: the UR5 of ur_ik.yaml at ee_fixed_joint, the Jaco of jaco_ik.yaml at its end effector (ten
   joints, a branching tree, the end effector mid-tree) and the cart of cart_tree_fixed.yaml at the frame on its slider's arm, where
   hinge_b -- no ancestor of that frame -- moves only through the null-space term (the lists put its lower limit above its rest
   angle).  With and without an orientation target, with and without the four lists, the start given and taken from the env's
   state; 3 and 70 envs (one partial wavefront, one wavefront boundary crossed) and the Jaco once in the one-env-per-wavefront
   workspace mode.  Targets: the forward kinematics of rest + U(-0.2, 0.2) per env.
   The lists are the URDF's limits but for the cart's slider, which gets (-1, 1): beyond a limit the recursion multiplies the
   excess by 1 - ik_null_limit_gain / range per iteration, and the slider's own range of 0.4 m makes that -24.  Targets that hold
   the slider at its limit then turn the recursion ITSELF into an amplifier -- the fp64 reference maps a 1e-7 change of the start
   to 7e-4 in 2 of the 70 envs, measured on the host -- and a comparison of two precisions measures that, not the kernel.  With
   the lists used here the reference maps a 1e-7 change of the start to at most 4e-7, but for the Jaco with orientation and
   lists at 70 envs (6e-6: joints past their limits), which is also where the largest error below is.
   Error measure: per env, max |q_gpu - q_ref| over the joints (radians, metres for the cart's slider); the figure of a case is the
   largest over its envs.  BOUND_Q is 8 x the largest figure measured over all cases on an MI355X (DESIGN.md "Inverse-kinematics
   query"); the margin is for a compiler that contracts multiply-adds differently, not for bugs.  It may not exceed 1e-4.
   Measured maxima (MI355X): ur_ik 3.43e-7 (x3) / 6.91e-7 (x70), jaco_ik 1.86e-6 / 8.76e-6 (1.98e-6 at one env per wavefront),
   cart_tree 1.42e-7 / 2.12e-7.
2. The early exit with the default ``ik_residual``, in worlds with ``ik_iterations`` = EARLY_ITERS: the reference exits in every
   case of EARLY_CASES with at least two iterations to spare (asserted here on its own iteration counts), every env reports fewer
   iterations than the world allows, and the joints the query returned put the frame within ik_residual + 1e-6 of the target.
3. The two push entries write exactly the selected joints' slots of exactly the selected envs -- every other column of the state is
   the same bits -- and the calls refuse what they cannot take.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import dynamics_ref as D
import ik_ref as R
from diy_gym_amd import DIYGym
from diy_gym_amd.mathx import quat_from_mat
from diy_gym_amd.scene import DEFAULTS, K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda:0'
MEASURED_Q = 8.77e-6   # largest max |q_gpu - q_ref| over all cases of test_query_matches_the_reference (jaco_ik x70, orientation + lists)
BOUND_Q = 8 * MEASURED_Q
assert BOUND_Q <= 1e-4
# scene -> (config, model, frame name, rest position over the body's joints)
SCENES = {
    'ur_ik': ('ur_ik.yaml', 'arm', 'ee_fixed_joint', [0.3, -1.0, 1.2, -0.5, 0.4, 0.1]),
    'jaco_ik': ('jaco_ik.yaml', 'robot', 'j2s7s300_joint_end_effector', [0.0, 2.9, 0.0, 1.3, 4.2, 1.4, 0.0, 1.0, 1.0, 1.0]),
    'cart_tree': ('cart_tree_fixed.yaml', 'cart', 'tip_joint', [0.05, 0.2, -0.1]),
}
CASES = [(s, B, None) for s in SCENES for B in (3, 70)] + [('jaco_ik', 3, '1')]   # (the Jaco's scene holds the one-env-per-wavefront mode)
EARLY_ITERS = 80   # (the reference needs at most 60: the UR5 with its orientation at 70 envs; at most 22 elsewhere)
EARLY_CASES = [(s, B) for s in ('ur_ik', 'jaco_ik') for B in (3, 70)]
_ENVS = {}


def make(scene, B, lanes, monkeypatch, **engine):
    """The env of a case, built once per session; ``lanes``: DG_MAX_LANES while the world is created."""
    key = (scene, B, lanes, tuple(sorted(engine.items())))
    if key not in _ENVS:
        if lanes:
            monkeypatch.setenv('DG_MAX_LANES', lanes)
        env = DIYGym(os.path.join(GOLDEN, SCENES[scene][0]), num_envs=B, device=DEV, seed=5, engine=engine)
        if lanes:
            assert env.sim.envs_per_wave == int(lanes)
        _ENVS[key] = env
    env = _ENVS[key]
    model = env.models[SCENES[scene][1]]
    return env, model, model.get_frame_id(SCENES[scene][2])


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def lists_of(robot, scene):
    """(rest, lower, upper, range) as the fp32 values both sides use."""
    lim = D.joint_limits(robot).astype(np.float32)
    if scene == 'cart_tree':
        lim[2] = (0.0, 2.0)   # hinge_b rests at -0.1, below this limit: the limit term of the null-space velocity pushes it
        lim[0] = (-1.0, 1.0)  # the slider: out of reach of every target (see the docstring on the URDF's own range)
    rest = np.asarray(SCENES[scene][3], dtype=np.float32)
    return rest, lim[:, 0], lim[:, 1], (lim[:, 1] - lim[:, 0]).astype(np.float32)


def targets(robot, scene, frame, Tb, B, seed):
    """Per env: the pose of the frame at rest + U(-0.2, 0.2), and a start near rest -- fp32 values, as the kernel gets them."""
    rng = np.random.default_rng(seed)
    rest = np.asarray(SCENES[scene][3], dtype=np.float64)
    pos, orn = np.zeros((B, 3), dtype=np.float32), np.zeros((B, 4), dtype=np.float32)
    for e in range(B):
        p, Rm = R.forward(robot, rest + rng.uniform(-0.2, 0.2, rest.size), frame, Tb[e])
        pos[e], orn[e] = p, quat_from_mat(Rm)
    q0 = (rest + rng.uniform(-0.05, 0.05, (B, rest.size))).astype(np.float32)
    return pos, orn, q0


@pytest.mark.parametrize('scene,B,lanes', CASES)
def test_query_matches_the_reference(scene, B, lanes, monkeypatch):
    env, model, frame = make(scene, B, lanes, monkeypatch, ik_residual=0.0)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    p = R.params(ik_residual=0.0)
    Tb = D.base_transforms(env, uid)
    pos, orn, q0 = targets(robot, scene, frame, Tb, B, 300 + B)
    lists = lists_of(robot, scene)
    current = sim.joint_states(uid)[0].cpu().numpy()
    worst = 0.0
    for use_orn in (False, True):
        for use_lists in (False, True):
            for given in (True, False):
                kw = dict(zip(('rest', 'lower', 'upper', 'ranges'), (v.tolist() for v in lists))) if use_lists else {}
                q, it = sim.calculate_inverse_kinematics(uid, frame, dev(pos), dev(orn) if use_orn else None, q0=dev(q0) if given else None, return_iters=True, **kw)
                assert q.shape == (B, n) and it.shape == (B, ) and it.dtype == torch.int32
                q, it = q.cpu().numpy(), it.cpu().numpy()
                assert (it == p['ik_iterations']).all()
                start = q0 if given else current
                ref = np.stack([R.solve(robot, frame, pos[e], orn[e] if use_orn else None, start[e], lists if use_lists else None, Tb[e], p)[0] for e in range(B)])
                assert np.abs(ref - start).max() > 1e-2   # (the solve went somewhere)
                if scene == 'cart_tree':   # hinge_b is no ancestor of the frame: the null-space term alone moves it
                    moved = np.abs(q[:, 2] - start[:, 2])
                    assert (moved > 1e-2).all() if use_lists else (moved == 0).all()
                err = float(np.abs(q - ref).max(axis=1).max())
                print('%s x%d lanes=%s orn=%d lists=%d q0=%d: max |q_gpu - q_ref| %.3g' % (scene, B, sim.lanes, use_orn, use_lists, given, err))
                worst = max(worst, err)
    assert np.array_equal(sim.joint_states(uid)[0].cpu().numpy(), current)   # the state is not written
    print('%s x%d lanes=%s: worst %.3g' % (scene, B, sim.lanes, worst))
    assert worst < BOUND_Q, (scene, B, worst)


@pytest.mark.parametrize('scene,B', EARLY_CASES)
def test_early_exit_reports_its_iterations_and_reaches_the_target(scene, B, monkeypatch):
    env, model, frame = make(scene, B, None, monkeypatch, ik_iterations=EARLY_ITERS)
    sim, robot, uid = env.sim, model.robot, model.uid
    p = R.params(ik_iterations=EARLY_ITERS)
    assert p['ik_residual'] == DEFAULTS['ik_residual'] > 0
    Tb = D.base_transforms(env, uid)
    pos, orn, q0 = targets(robot, scene, frame, Tb, B, 500 + B)
    for use_orn in (False, True):
        ref_iters = [R.solve(robot, frame, pos[e], orn[e] if use_orn else None, q0[e], None, Tb[e], p)[1] for e in range(B)]
        assert 2 <= min(ref_iters) and max(ref_iters) <= EARLY_ITERS - 2, (scene, use_orn, max(ref_iters))   # two iterations to spare
        q, it = sim.calculate_inverse_kinematics(uid, frame, dev(pos), dev(orn) if use_orn else None, q0=dev(q0), return_iters=True)
        it = it.cpu().numpy()
        print('%s x%d orn=%d: iterations gpu %d..%d, reference %d..%d' % (scene, B, use_orn, it.min(), it.max(), min(ref_iters), max(ref_iters)))
        assert (it >= 1).all() and (it < EARLY_ITERS).all()
        sim.reset_joint_state(uid, q)
        reached = sim.frame_state(uid, frame, com=True)[:, 0:3].cpu().numpy().astype(np.float64)
        dist = np.linalg.norm(reached - pos.astype(np.float64), axis=1)
        assert (dist < p['ik_residual'] + 1e-6).all(), (scene, use_orn, dist.max())
    env.reset()


def columns(env, body, field):
    L = env.layout
    return [L.link_state_off[L.body_first_link[body] + i] + field for i in range(L.body_n_links[body])]


@pytest.mark.parametrize('B', [3, 70])
def test_targets_and_reset_write_the_selected_slots_only(B):
    env = DIYGym(os.path.join(GOLDEN, 'ur_arms_touching_ik.yaml'), num_envs=B, device=DEV, seed=5)   # two arms, colliding forearms: pairs
    sim, L = env.sim, env.layout
    uid, other = env.models['ur5_l'].uid, env.models['ur5_r'].uid
    n = L.body_n_links[uid]
    warm = int(L.I[K.H_WARM_OFF])
    assert warm >= 0
    for _ in range(3):
        sim.step(0)
    rng = np.random.default_rng(B)
    draw = lambda: dev(rng.uniform(-1.0, 1.0, (B, n)).astype(np.float32))
    tp, tv, tq, tqd = (columns(env, uid, f) for f in (K.LS_TARGET_POS, K.LS_TARGET_VEL, K.LS_Q, K.LS_QD))

    def changed(before, after):
        """columns whose bits differ anywhere, and the envs in which they do"""
        diff = before.view(np.uint32) != after.view(np.uint32)
        return sorted(np.nonzero(diff.any(axis=0))[0].tolist()), sorted(np.nonzero(diff.any(axis=1))[0].tolist())

    # ---- POSITION_CONTROL on joints 1, 3, 4: their position targets, velocity targets = vel
    joints = [1, 3, 4]
    pos, vel = draw(), draw()
    s0 = sim.get_state()
    sim.set_joint_motor_targets(uid, positions=pos, velocities=vel, joints=joints)
    s1 = sim.get_state()
    assert changed(s0, s1)[0] == sorted([tp[j] for j in joints] + [tv[j] for j in joints])
    assert (s1[:, [tp[j] for j in joints]] == pos.cpu().numpy()[:, joints]).all() and (s1[:, [tv[j] for j in joints]] == vel.cpu().numpy()[:, joints]).all()
    # ... without velocities: zero velocity targets; every joint when none is named
    sim.set_joint_motor_targets(uid, positions=pos)
    s2 = sim.get_state()
    assert (s2[:, tp] == pos.cpu().numpy()).all() and (s2[:, tv] == 0).all()
    assert set(changed(s1, s2)[0]) <= set(tp + tv)
    # ---- VELOCITY_CONTROL: the velocity-only form writes a zero position target
    sim.set_joint_motor_targets(uid, velocities=vel, joints=[0, 5])
    s3 = sim.get_state()
    assert (s3[:, [tv[0], tv[5]]] == vel.cpu().numpy()[:, [0, 5]]).all() and (s3[:, [tp[0], tp[5]]] == 0).all()
    assert set(changed(s2, s3)[0]) <= {tp[0], tp[5], tv[0], tv[5]}
    assert (s3[:, columns(env, other, K.LS_TARGET_POS)] == s0[:, columns(env, other, K.LS_TARGET_POS)]).all()
    # ---- reset_joint_state under an env mask: q, qd of the selected joints of the selected envs, their contact cache count
    for _ in range(2):
        sim.step(0)
    s4 = sim.get_state()
    assert (s4[:, warm] > 0).all()   # (the forearms touch: every env has cached impulses)
    mask = torch.zeros(B, dtype=torch.bool)
    mask[::2] = True
    q, qd = draw(), draw()
    sim.reset_joint_state(uid, q, qd, joints=[2, 5], mask=mask)
    s5 = sim.get_state()
    cols, envs = changed(s4, s5)
    sel = np.nonzero(mask.numpy())[0]
    assert cols == sorted([tq[2], tq[5], tqd[2], tqd[5], warm]) and envs == sel.tolist()
    assert (s5[sel][:, [tq[2], tq[5]]] == q.cpu().numpy()[sel][:, [2, 5]]).all() and (s5[sel][:, [tqd[2], tqd[5]]] == qd.cpu().numpy()[sel][:, [2, 5]]).all()
    assert (s5[sel, warm] == 0).all() and (s5[~mask.numpy(), warm] == s4[~mask.numpy(), warm]).all()
    # ... qd None: zero; no mask: every env; one [nv] row for every env
    sim.reset_joint_state(uid, q[0].clone())
    s6 = sim.get_state()
    assert (s6[:, tq] == q[0].cpu().numpy()).all() and (s6[:, tqd] == 0).all() and (s6[:, warm] == 0).all()
    assert set(changed(s5, s6)[0]) <= set(tq + tqd + [warm])
    assert (s6[:, tp] == s3[:, tp]).all() and (s6[:, tv] == s3[:, tv]).all()   # the targets are left alone


def test_errors_raise_and_launch_nothing(monkeypatch):
    env, model, frame = make('ur_ik', 3, None, monkeypatch, ik_residual=0.0)
    sim, uid, n = env.sim, model.uid, model.robot.num_dofs
    pos, q = torch.zeros((3, 3), device=DEV), torch.zeros((3, n), device=DEV)
    lists = dict(zip(('rest', 'lower', 'upper', 'ranges'), (v.tolist() for v in lists_of(model.robot, 'ur_ik'))))
    kept = sim.calculate_inverse_kinematics(uid, frame, pos, **lists)
    before, state = kept.clone(), sim.state.clone()
    floating = DIYGym(os.path.join(GOLDEN, 'box_stack.yaml'), num_envs=3, device=DEV)
    static = DIYGym(os.path.join(GOLDEN, 'ur5_gripper.yaml'), num_envs=3, device=DEV)
    plane = static.models['plane'].uid   # frozen into the static world
    calls = lambda s, b: [lambda: s.calculate_inverse_kinematics(b, 0, pos), lambda: s.set_joint_motor_targets(b, positions=torch.zeros((3, 1), device=DEV)),
                          lambda: s.reset_joint_state(b, torch.zeros((3, 1), device=DEV))]
    for s, b in ((floating.sim, floating.models['lower'].uid), (static.sim, plane), (sim, 99)):
        for call in calls(s, b):
            with pytest.raises(ValueError):
                call()
    bad = [lambda: sim.calculate_inverse_kinematics(uid, -1, pos),                                           # the base
           lambda: sim.calculate_inverse_kinematics(uid, len(model.robot.joints), pos),                      # frame out of range
           lambda: sim.calculate_inverse_kinematics(uid, frame, pos[:, :2].contiguous()),                    # wrong shapes
           lambda: sim.calculate_inverse_kinematics(uid, frame, pos, torch.zeros((3, 3), device=DEV)),
           lambda: sim.calculate_inverse_kinematics(uid, frame, pos, q0=q[:, :n - 1].contiguous()),
           lambda: sim.calculate_inverse_kinematics(uid, frame, pos.double()), lambda: sim.calculate_inverse_kinematics(uid, frame, pos.cpu()),
           lambda: sim.calculate_inverse_kinematics(uid, frame, None),
           lambda: sim.calculate_inverse_kinematics(uid, frame, pos, lower=lists['lower'], upper=lists['upper']),   # a partial list set
           lambda: sim.calculate_inverse_kinematics(uid, frame, pos, **dict(lists, rest=lists['rest'][:n - 1])),   # a list of another length
           lambda: sim.set_joint_motor_targets(uid), lambda: sim.set_joint_motor_targets(uid, positions=q[:2].contiguous()),
           lambda: sim.set_joint_motor_targets(uid, positions=q, joints=[n]), lambda: sim.set_joint_motor_targets(uid, velocities=q.double()),
           lambda: sim.reset_joint_state(uid, None), lambda: sim.reset_joint_state(uid, q, q[:, :2].contiguous()),
           lambda: sim.reset_joint_state(uid, q, joints=[-1]), lambda: sim.reset_joint_state(uid, q, mask=torch.ones(2, dtype=torch.bool))]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    # the C entries themselves: DG_ERR_ARG, nothing launched
    lib, st = sim.lib, ctypes.c_void_p(sim.state.data_ptr())
    out = torch.full((3, 64), 7.0, device=DEV)
    o, fst, fb = ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(floating.sim.state.data_ptr()), floating.models['lower'].uid
    assert lib.dg_world_inverse_kinematics(floating.sim.handle, fst, fb, 0, o, None, None, None, o, None, None) == -4 and b'floating' in lib.dg_last_error()
    assert lib.dg_world_set_joint_targets(floating.sim.handle, fst, fb, ctypes.c_uint64(1), o, None, None) == -4
    assert lib.dg_world_reset_joint_state(floating.sim.handle, fst, fb, ctypes.c_uint64(1), o, None, None, None) == -4
    assert lib.dg_world_inverse_kinematics(sim.handle, st, uid, 40, o, None, None, None, o, None, None) == -4 and b'frame' in lib.dg_last_error()
    assert lib.dg_world_inverse_kinematics(sim.handle, st, uid, frame, None, None, None, None, o, None, None) == -4
    assert lib.dg_world_inverse_kinematics(sim.handle, st, uid, frame, o, None, None, None, None, None, None) == -4 and b'q_out' in lib.dg_last_error()
    assert lib.dg_world_set_joint_targets(sim.handle, st, uid, ctypes.c_uint64(1), None, None, None) == -4
    assert lib.dg_world_reset_joint_state(sim.handle, st, uid, ctypes.c_uint64(1), None, None, None, None) == -4
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(kept, before) and torch.equal(sim.state, state)
