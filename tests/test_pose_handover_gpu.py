"""The opening pose hand-over of the helper-wave step kernel (dg_step_par_body.inc, `pose_ho`; Handover in dg_solver.h): in a scene
with `early_dyn` and `coll_split` the two narrow-phase wavefronts compute the arms' opening poses, and the two inverse-kinematics
wavefronts start their solve at once and pass the workgroup barrier B0 from inside it -- between its set-up and its first forward
kinematics --, or in the kernel body if no register-chain solve ran.  DG_NO_EARLY_DYNAMICS=1 and DG_NO_COLLIDE_SPLIT=1 are its
off switches.  A barrier count that differed between the wavefronts on any of these paths would be a hang, so every case below
runs under a wall-clock limit that ends the process.

67 envs unless said otherwise: one full workgroup and one with three real envs.

Tolerances are those of tests/test_parity_gpu.py for these scenes: 5e-4 on observations and on the kinematic columns of the
state, |difference| / (1 + |oracle|) < 5e-3 on efforts (the applied-torque columns); ur_arms_touching 3e-3 on observations,
ur_arms_touching_ik 5e-3."""
import faulthandler
import os

import numpy as np
import pytest
import torch

from test_parity_gpu import CONFIGS, action_bounds, make_pair, phys_state
from test_fused_free_substep_gpu import obs_errors, state_errors

pytestmark = pytest.mark.gpu

B = 67
OBS_TOL, EFFORT_REL_TOL = 5e-4, 5e-3
WALL_CLOCK_LIMIT = 120   # seconds per test; a case takes a few (most of it world creation and the oracle)


@pytest.fixture(autouse=True)
def wall_clock_limit():
    """A watchdog thread: it fires even while the main thread waits inside a device synchronise, dumps the stacks and exits."""
    faulthandler.dump_traceback_later(WALL_CLOCK_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def world_under(switches, name='ur_ik', num_envs=B, **engine):
    """A HIP world of `name` created with the environment switches of `switches` set to 1 (make_pair's seed)."""
    from diy_gym_amd import DIYGym
    for s in switches:
        os.environ[s] = '1'
    try:
        return DIYGym(CONFIGS[name], num_envs=num_envs, device='cuda:0', seed=5, engine=engine)
    finally:
        for s in switches:
            del os.environ[s]


def plan_under(env, switches):
    from diy_gym_amd.backend import debug_plan
    for s in switches:
        os.environ[s] = '1'
    try:
        return debug_plan(env.layout, env.num_envs)
    finally:
        for s in switches:
            del os.environ[s]


def random_actions(env, gen, n=None, scale=1.0):
    lo, hi = action_bounds(env)
    return (lo + (hi - lo) * torch.rand((n or env.num_envs, lo.numel()), generator=gen)) * scale


def check_against_oracle(gpu, cpu, what):
    o, oe = obs_errors(gpu, cpu)
    k, e = state_errors(phys_state(gpu), phys_state(cpu), gpu)
    print('%s: obs %.3g, obs efforts (relative) %.3g, state %.3g, state efforts (relative) %.3g' % (what, o, oe, k, e))
    assert o < OBS_TOL and oe < EFFORT_REL_TOL and k < OBS_TOL and e < EFFORT_REL_TOL, (what, o, oe, k, e)


def test_against_the_oracle_and_the_two_off_switches():
    """12 seeded random steps of ur_ik in four worlds: default (the hand-over), the oracle, DG_NO_EARLY_DYNAMICS=1 and
    DG_NO_COLLIDE_SPLIT=1 (each: the plain order, every wavefront's own pose pass and then B0).  Full state and observations
    after every step.  Whether the three HIP worlds agree bit for bit is printed, not asserted (the base rotation is stored from
    a second copy of qmat(), which may contract into FMAs differently).  Measured: they agree in every bit of state and
    observations over the 12 steps; against the oracle 4.1e-6 on observations and state, 2.6e-3 relative on efforts."""
    gpu, cpu = make_pair('ur_ik', B)
    off = {sw: world_under([sw]) for sw in ('DG_NO_EARLY_DYNAMICS', 'DG_NO_COLLIDE_SPLIT')}
    for sw, env in [(None, gpu)] + list(off.items()):
        plan = plan_under(env, [sw] if sw else [])
        assert env.sim.lanes == 64 and env.sim.par, sw
        assert bool(plan['early_dyn']) == (sw != 'DG_NO_EARLY_DYNAMICS'), (sw, plan['early_dyn'])
        assert bool(plan['coll_split']) == (sw != 'DG_NO_COLLIDE_SPLIT'), (sw, plan['coll_split'])
        assert plan['reg_body0'] >= 0 and plan['helper_body'] >= 0 and plan['reg_body0'] != plan['helper_body'], sw
    gen = torch.Generator().manual_seed(11)
    bitwise = {sw: True for sw in off}
    for i in range(12):
        act = random_actions(gpu, gen)
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); cpu.sim.step(cpu._all_slots, act)
        check_against_oracle(gpu, cpu, 'step %d, default' % i)
        full_g = np.asarray(gpu.sim.get_state())
        for sw, env in off.items():
            env.sim.step(env._all_slots, act.to(env.device))
            check_against_oracle(env, cpu, 'step %d, %s' % (i, sw))
            k, e = state_errors(phys_state(gpu), phys_state(env), gpu)
            assert k < OBS_TOL and e < EFFORT_REL_TOL and float((gpu.sim.obs - env.sim.obs).abs().max()) < OBS_TOL, (sw, k, e)
            bitwise[sw] = bitwise[sw] and np.array_equal(full_g.view(np.uint32), np.asarray(env.sim.get_state()).view(np.uint32)) \
                and torch.equal(gpu.sim.obs, env.sim.obs)
    print('state and observations bit for bit equal to the default world over 12 steps: %s' % bitwise)


def test_general_register_ik_takes_the_hand_over():
    """DG_NO_FULL_IK=1: the arms' solves are run_ik_chain<6>, the general register-resident form, with the same hand-over."""
    cpu = make_pair('ur_ik', B)[1]
    gpu = world_under(['DG_NO_FULL_IK'])
    plan = plan_under(gpu, ['DG_NO_FULL_IK'])
    assert gpu.sim.lanes == 64 and gpu.sim.par and plan['early_dyn'] and plan['coll_split']
    gen = torch.Generator().manual_seed(12)
    for i in range(6):
        act = random_actions(gpu, gen)
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); cpu.sim.step(cpu._all_slots, act)
        check_against_oracle(gpu, cpu, 'DG_NO_FULL_IK, step %d' % i)


def test_ik_op_masked_out():
    """Steps whose slot mask leaves one arm's controller out (each arm in turn), then both: the wavefront whose op is masked
    out passes B0 in the kernel body, behind run_update_ops.  The call returns and the state follows the oracle."""
    gpu, cpu = make_pair('ur_ik', B)
    assert gpu.layout.n_slots == 2 and gpu._all_slots == 3
    gen = torch.Generator().manual_seed(13)
    for i, slots in enumerate([3, 1, 2, 0, 3, 2, 0, 1]):
        act = random_actions(gpu, gen)
        gpu.sim.step(slots, act.to(gpu.device)); cpu.sim.step(slots, act)
        torch.cuda.synchronize()
        check_against_oracle(gpu, cpu, 'slot mask %d, step %d' % (slots, i))


def test_masked_reset_through_the_reset_kernel():
    """reset(mask) of envs 1, 40 and 65 after 4 steps: reset_kernel_par's hot-start step has no actions, so both
    inverse-kinematics wavefronts pass B0 in the kernel body.  Untouched envs keep every bit, reset envs follow the oracle, and
    an all-zero mask (every wavefront leaves before the first barrier) returns with nothing changed."""
    gpu, cpu = make_pair('ur_ik', B)
    gen = torch.Generator().manual_seed(3)
    for _ in range(4):
        act = random_actions(gpu, gen)
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); cpu.sim.step(cpu._all_slots, act)
    mask = torch.zeros(B, dtype=torch.uint8); mask[[1, 40, 65]] = 1
    before = np.array(gpu.sim.get_state())
    gpu.sim.reset(mask.to(gpu.device)); cpu.sim.reset(mask)
    after = np.array(gpu.sim.get_state())
    keep = (mask == 0).numpy()
    assert np.array_equal(before[keep].view(np.uint32), after[keep].view(np.uint32))
    assert not np.array_equal(before[~keep], after[~keep])
    k, e = state_errors(phys_state(gpu)[~keep], phys_state(cpu)[~keep], gpu)
    print('masked reset, reset envs against the oracle: kinematic %.3g, efforts (relative) %.3g' % (k, e))
    assert k < OBS_TOL and e < EFFORT_REL_TOL, (k, e)
    obs_before = gpu.sim.obs.clone()
    gpu.sim.reset(torch.zeros(B, dtype=torch.uint8, device=gpu.device))
    torch.cuda.synchronize()
    assert np.array_equal(after.view(np.uint32), np.array(gpu.sim.get_state()).view(np.uint32))
    assert torch.equal(obs_before, gpu.sim.obs)
    # and the worlds go on in step
    act = random_actions(gpu, gen)
    gpu.sim.step(gpu._all_slots, act.to(gpu.device)); cpu.sim.step(cpu._all_slots, act)
    check_against_oracle(gpu, cpu, 'the step after the resets')


@pytest.mark.parametrize('name,scale,tol', [('touching', 0.3, 3e-3), ('touching_ik', 1.0, 5e-3)])
def test_arms_in_contact(name, scale, tol):
    """37 envs, 20 steps, the arms start with crossed forearms: contacts in the step's first substep.  ur_arms_touching (capsule
    narrow phase, hull_contacts = 0, as the other tests run it) is under joint_controller: no inverse-kinematics op, early_dyn == 0,
    so it pins that such a scene keeps the plain order.  ur_arms_touching_ik is the same pose under ik_controller: the hand-over
    with contacts in the early narrow phase that consumes the handed-over poses (tolerance: test_parity_gpu's for that scene)."""
    n = 37
    gpu, cpu = make_pair(name, n)
    plan = plan_under(gpu, [])
    assert gpu.sim.lanes == 64 and gpu.sim.par
    assert bool(plan['early_dyn']) == (name == 'touching_ik') and plan['coll_split'], (plan['early_dyn'], plan['coll_split'])
    d = gpu.sim.enable_diagnostics()
    gen = torch.Generator().manual_seed(0)
    worst = 0.0; term_mismatch = 0; first_substep_contacts = 0
    for _ in range(20):
        act = random_actions(gpu, gen, n, scale)
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); cpu.sim.step(cpu._all_slots, act)
        worst = max(worst, float((gpu.sim.obs.cpu() - cpu.sim.obs).abs().max()))
        term_mismatch += int((gpu.sim.term.cpu() != cpu.sim.term).sum())
        first_substep_contacts += int(d[:, 3].max() > 0)   # DIAG_CONTACTS_FIRST
    print('%s: obs %.3g, steps with a contact in the first substep %d of 20' % (name, worst, first_substep_contacts))
    assert worst < tol and term_mismatch == 0, (worst, term_mismatch)
    assert first_substep_contacts > 0
