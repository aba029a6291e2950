"""Substeps without narrow phase and pose pass (sc.np_skip; substep_np_skip in dg_solver.h, the four-wavefront kernel body in
dg_step_par_body.inc): while the clearance the previous narrow phase measured exceeds what the two arms can have moved since, a
substep k >= 1 leaves out its narrow phase -- which would find nothing -- and the pose pass in front of it, whose only reader the
narrow phase is in a contact-free substep.  Nothing the step computes changes, so the yardstick is bit-for-bit equality, state
and observations, with a world created under DG_NO_NP_SKIP=1 (the off switch: every substep runs both), next to the usual
comparison with the fp64 checker; `dg_world_set_skip_counter` reports per env how many substeps of the last step were skipped
(the decision is the workgroup's: 64 envs report the same number).

Every wavefront of the workgroup takes the decision on its own from the same LDS values; a disagreement would be a barrier
miscount, i.e. a hang, so every case runs under the wall-clock watchdog of tests/test_pose_handover_gpu.py.

67 envs unless said otherwise: one full workgroup and one with three real envs.  Tolerances against the checker are those of
tests/test_parity_gpu.py for these scenes (test_pose_handover_gpu.check_against_oracle: 5e-4 on observations and the kinematic
state, 5e-3 relative on efforts; ur_arms_touching_ik 5e-3 on observations)."""
import os

import numpy as np
import pytest
import torch

from test_parity_gpu import CONFIGS, make_pair
from test_pose_handover_gpu import check_against_oracle, plan_under, random_actions, wall_clock_limit, world_under  # noqa: F401  (the watchdog is an autouse fixture)

pytestmark = pytest.mark.gpu

B = 67
OFF = 'DG_NO_NP_SKIP'


def bits(env):
    return np.asarray(env.sim.get_state()).view(np.uint32)


def assert_same_bits(a, b, what):
    assert np.array_equal(bits(a), bits(b)), ('state', what)
    assert torch.equal(a.sim.obs, b.sim.obs), ('observations', what)
    assert torch.equal(a.sim.rew, b.sim.rew) and torch.equal(a.sim.term, b.sim.term), ('rewards / terminals', what)


def plans(gpu, off):
    p, q = plan_under(gpu, []), plan_under(off, [OFF])
    assert p['np_skip'] == 1 and q['np_skip'] == 0
    assert gpu.sim.lanes == 64 and gpu.sim.par and off.sim.lanes == 64 and off.sim.par
    return p


@pytest.mark.parametrize('name,steps', [('ur_ik', 12), ('ur_joint', 6)])
def test_free_arms_skip_every_second_substep(name, steps):
    """Seeded random steps in three worlds: default, DG_NO_NP_SKIP=1 and the checker.  The two HIP worlds agree in every bit after
    every step, both follow the checker, and every env reports a skipped substep at every step (the arms of ur_high_5 start a
    metre apart).  ur_ik takes the clearance from the early narrow phase of the update phase, ur_joint (no inverse-kinematics
    op: early_dyn == 0) from the narrow phase of substep 0 inside the loop."""
    gpu, cpu = make_pair(name, B)
    off = world_under([OFF], name)
    p = plans(gpu, off)
    assert bool(p['early_dyn']) == (name == 'ur_ik')
    skipped, skipped_off = gpu.sim.enable_skip_counter(), off.sim.enable_skip_counter()
    gen = torch.Generator().manual_seed(11)
    for i in range(steps):
        act = random_actions(gpu, gen)
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); off.sim.step(off._all_slots, act.to(off.device)); cpu.sim.step(cpu._all_slots, act)
        torch.cuda.synchronize()
        print('%s step %d: skipped substeps per env %d .. %d' % (name, i, int(skipped.min()), int(skipped.max())))
        assert_same_bits(gpu, off, (name, i))
        check_against_oracle(gpu, cpu, '%s step %d, default' % (name, i))
        check_against_oracle(off, cpu, '%s step %d, %s' % (name, i, OFF))
        assert int(skipped.min()) > 0 and int(skipped.max()) <= 1, (i, skipped.tolist())
        assert int(skipped_off.max()) == 0


# Shoulder increments of make_vectors.press_actions (0.06 .. 0.14 rad over the 16 envs) are scaled per leg: see the test's docstring.
AWAY, STEPS_AWAY, BACK, STEPS_BACK = -3.5, 18, 1.0, 22


def test_arms_meeting_in_a_second_substep():
    """The scene and actions of test_arms_pressed_together_follow_the_checker_free_running (tests/test_hull_contacts.py), 16
    envs: crossed forearms, hulls 4.5 mm apart, one shoulder turning.  The default world equals the off-switch world in every bit,
    contact counts are the checker's at every step, and the counter shows skipped as well as refused steps.  Premise, asserted on
    the off-switch world alone: at some (env, step) the step's first substep is free of contacts and its last is not -- a first
    contact made in a second substep, which a wrong skip would have missed.

    The shoulder rate is scaled, as the premise needs it.  With the actions as they are the hulls are inside the contact margin
    from the first step on: 3 contacts in every env in both substeps of all 30 steps, no step skipped, premise 0.  Measured on
    the off-switch world for scales -200 .. 200 (1, 3, 10, 30, 60, 100, 200, their negatives, -1.2 .. -2.8 in steps of 0.2, -3.5,
    -4, -5, -7), 30 steps each: a positive scale keeps 3 contacts throughout; a negative one turns the shoulder away, the contacts
    go 3 -> 2 -> 1 -> 0 between steps 12 and 29 (always last substep first: '1 / 0') and never come back, 0 - 7 steps skipped near
    the end: no single scale makes the arms MEET.  So the rollout has two legs: 18 steps at scale -3.5 (apart by step 14, the
    clearance then grows past the bound: skipped steps) and 22 steps at scale 1, the test's own actions, which bring the forearms
    back together -- the approach in which contacts appear.  Measured: 3 steps skipped, 37 refused, 2 (env, step) with the first
    contact in the second substep."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    import make_vectors
    import oracle_backend
    from diy_gym_amd import DIYGym
    n = 16
    cfg = CONFIGS['touching']

    def world(switches=()):
        for s in switches:
            os.environ[s] = '1'
        try:
            return DIYGym(cfg, num_envs=n, device='cuda:0', seed=5)
        finally:
            for s in switches:
                del os.environ[s]
    gpu, off = world(), world([OFF])
    cpu = DIYGym(cfg, num_envs=n, seed=5, backend_factory=oracle_backend.OracleBackend)
    plans(gpu, off)
    d, d_off = gpu.sim.enable_diagnostics(), off.sim.enable_diagnostics()
    skipped = gpu.sim.enable_skip_counter()
    steps = STEPS_AWAY + STEPS_BACK
    held = torch.tensor(make_vectors.CROSSED * 2, dtype=torch.float32)[None, None]   # the crossed pose, held
    turn = make_vectors.press_actions(gpu, steps) - held
    scale = torch.tensor([AWAY] * STEPS_AWAY + [BACK] * STEPS_BACK)[:, None, None]
    acts = held + turn * scale
    n_skipped = n_refused = first_contact_in_second = 0
    for step in range(steps):
        for env in (gpu, off):
            env.sim.step(env._all_slots, acts[step].to('cuda:0'))
        cpu.sim.step(cpu._all_slots, acts[step])
        torch.cuda.synchronize()
        s = int(skipped.max())
        print('step %2d: skipped %d, contacts first / last substep %s / %s' % (step, s, d_off[:, 3].tolist(), d_off[:, 0].tolist()))
        assert_same_bits(gpu, off, step)
        assert torch.equal(d, d_off), step
        assert d[:, 0].tolist() == [cpu.sim.contacts(e) for e in range(n)], step
        assert int(skipped.min()) == s   # one workgroup: one verdict
        n_skipped += s > 0; n_refused += s == 0
        first_contact_in_second += int(((d_off[:, 3] == 0) & (d_off[:, 0] > 0)).sum())   # DG_DIAG_CONTACTS_FIRST, DG_DIAG_CONTACTS
    print('steps skipped %d, refused %d; (env, step) with the first contact in the second substep %d' % (n_skipped, n_refused, first_contact_in_second))
    assert first_contact_in_second > 0
    assert n_skipped > 0 and n_refused > 0, (n_skipped, n_refused)


def test_arms_in_contact_under_ik_control():
    """ur_arms_touching_ik, 37 envs, 20 steps (test_pose_handover_gpu.test_arms_in_contact): contacts in the early narrow phase.
    Bit for bit the off-switch world; no substep is skipped in a step in which the workgroup holds a contact."""
    n = 37
    gpu, cpu = make_pair('touching_ik', n)
    off = world_under([OFF], 'touching_ik', n)
    plans(gpu, off)
    d = gpu.sim.enable_diagnostics(); skipped = gpu.sim.enable_skip_counter()
    gen = torch.Generator().manual_seed(0)
    with_contact = worst = 0
    for i in range(20):
        act = random_actions(gpu, gen, n)
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); off.sim.step(off._all_slots, act.to(off.device)); cpu.sim.step(cpu._all_slots, act)
        torch.cuda.synchronize()
        assert_same_bits(gpu, off, i)
        worst = max(worst, float((gpu.sim.obs.cpu() - cpu.sim.obs).abs().max()))
        contact = int(d[:, 0].max()) > 0 or int(d[:, 3].max()) > 0
        with_contact += contact
        print('step %2d: workgroup holds a contact %s, skipped %d .. %d' % (i, contact, int(skipped.min()), int(skipped.max())))
        if contact:
            assert int(skipped.max()) == 0, i
    print('touching_ik: obs %.3g, steps with a contact in the workgroup %d of 20' % (worst, with_contact))
    assert worst < 5e-3, worst
    assert with_contact > 0


def test_masked_reset_and_slot_masks():
    """After 4 steps: reset(mask) of envs 1, 40 and 65 (reset_kernel_par shares the step's body: its hot-start step decides and
    skips like any other), a reset with an all-zero mask, then steps under the slot masks 1, 2 and 0.  Untouched envs keep every
    bit across the resets, and the default world stays bit for bit the off-switch world throughout."""
    gpu, cpu = make_pair('ur_ik', B)
    off = world_under([OFF])
    plans(gpu, off)
    gen = torch.Generator().manual_seed(3)

    def step(slots, what):
        act = random_actions(gpu, gen)
        gpu.sim.step(slots, act.to(gpu.device)); off.sim.step(slots, act.to(off.device)); cpu.sim.step(slots, act)
        torch.cuda.synchronize()
        assert_same_bits(gpu, off, what)
        check_against_oracle(gpu, cpu, what)
    for i in range(4):
        step(gpu._all_slots, 'step %d' % i)
    mask = torch.zeros(B, dtype=torch.uint8); mask[[1, 40, 65]] = 1
    keep = (mask == 0).numpy()
    before = bits(gpu).copy()
    gpu.sim.reset(mask.to(gpu.device)); off.sim.reset(mask.to(off.device)); cpu.sim.reset(mask)
    torch.cuda.synchronize()
    after = bits(gpu).copy()
    assert np.array_equal(before[keep], after[keep]) and not np.array_equal(before[~keep], after[~keep])
    assert_same_bits(gpu, off, 'masked reset')
    for env in (gpu, off):
        env.sim.reset(torch.zeros(B, dtype=torch.uint8, device=env.device))
    torch.cuda.synchronize()
    assert np.array_equal(after, bits(gpu))
    assert_same_bits(gpu, off, 'all-zero mask')
    for slots in (1, 2, 0):
        step(slots, 'slot mask %d' % slots)
