"""The fused contact-free substep of the helper-wave step kernel (fused_free_halves, dg_solver.h): motor / limit rows,
sweeps and joint integration of both arms in the arm-per-half-wavefront lane mapping, for substeps in which no env of the
workgroup has a contact.  DG_NO_SPLIT_SWEEPS=1 is its off switch (split_pgs == 0: the main wave does everything).

67 envs throughout: one full workgroup and one with three real envs, so the store predicate of the new lane mapping is
exercised in both halves of both wavefronts and lanes without an env exist.

Tolerances are those of tests/test_parity_gpu.py for these scenes: 5e-4 on observations and on the kinematic columns of
the state (the same quantities), |difference| / (1 + |oracle|) < 5e-3 on efforts (the applied-torque columns: O(100) N m,
determined to the solver's residual early-out)."""
import os

import numpy as np
import pytest
import torch

from test_parity_gpu import CONFIGS, action_bounds, effort_columns, make_pair, phys_state

pytestmark = pytest.mark.gpu

B = 67
OBS_TOL, EFFORT_REL_TOL = 5e-4, 5e-3


def unfused_world(name, num_envs=B, **engine):
    from diy_gym_amd import DIYGym
    os.environ['DG_NO_SPLIT_SWEEPS'] = '1'
    try:
        return DIYGym(CONFIGS[name], num_envs=num_envs, device='cuda:0', seed=5, engine=engine)   # (make_pair's seed)
    finally:
        del os.environ['DG_NO_SPLIT_SWEEPS']


def columns(env):
    """(kinematic, applied-torque) columns of the physical state."""
    eff = [o + 5 for o in env.layout.link_state_off]   # DG_LS_APPLIED
    return [c for c in range(env.layout.physical_dim) if c not in eff], eff


def state_errors(a, b, env):
    """(largest kinematic difference, largest relative effort difference) of two [B, physical_dim] states, b the reference."""
    kin, eff = columns(env)
    return float(np.abs(a[:, kin] - b[:, kin]).max()), float((np.abs(a[:, eff] - b[:, eff]) / (1.0 + np.abs(b[:, eff]))).max())


def obs_errors(gpu, cpu):
    eo, _ = effort_columns(gpu)
    d = (gpu.sim.obs.cpu() - cpu.sim.obs).abs()
    keep = torch.ones(d.shape[1], dtype=torch.bool); keep[eo] = False
    rel = float((d[:, eo] / (1.0 + cpu.sim.obs[:, eo].abs())).max()) if eo else 0.0
    return float(d[:, keep].max()), rel


@pytest.mark.parametrize('name', ['ur_ik', 'ur_joint'])
def test_fused_path_against_the_oracle_and_the_unfused_path(name):
    """12 steps of seeded random actions in three worlds: default (fused), DG_NO_SPLIT_SWEEPS=1 (the main wave sets up,
    sweeps and integrates both arms) and the oracle.  Full state, observations and the applied efforts of all twelve
    joints after every step.  Between the two HIP worlds the largest difference is printed and held to the same tolerance;
    whether the impulses still agree bit for bit is printed, not asserted (two copies of one expression may contract into
    FMAs differently).  Measured: against the oracle 4.1e-6 on observations and state, 2.6e-3 relative on efforts (ur_ik);
    between the two HIP worlds 0 in every column of the state, efforts included."""
    gpu, cpu = make_pair(name, B)
    off = unfused_world(name)
    assert gpu.sim.lanes == 64 and off.sim.lanes == 64
    assert len(gpu.layout.link_state_off) == 12
    lo, hi = action_bounds(gpu)
    gen = torch.Generator().manual_seed(11)
    worst = dict(obs=0.0, obs_eff=0.0, kin=0.0, eff=0.0, hip_obs=0.0, hip_kin=0.0, hip_eff=0.0, hip_state_abs=0.0)
    bitwise_efforts = True
    _, eff = columns(gpu)
    for _ in range(12):
        act = lo + (hi - lo) * torch.rand((B, lo.numel()), generator=gen)
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); off.sim.step(off._all_slots, act.to(off.device)); cpu.sim.step(cpu._all_slots, act)
        o, oe = obs_errors(gpu, cpu)
        g, u, c = phys_state(gpu), phys_state(off), phys_state(cpu)
        k, e = state_errors(g, c, gpu)
        hk, he = state_errors(g, u, gpu)
        full_g, full_u = np.asarray(gpu.sim.get_state()), np.asarray(off.sim.get_state())
        worst['obs'] = max(worst['obs'], o); worst['obs_eff'] = max(worst['obs_eff'], oe)
        worst['kin'] = max(worst['kin'], k); worst['eff'] = max(worst['eff'], e)
        worst['hip_obs'] = max(worst['hip_obs'], float((gpu.sim.obs - off.sim.obs).abs().max()))
        worst['hip_kin'] = max(worst['hip_kin'], hk); worst['hip_eff'] = max(worst['hip_eff'], he)
        worst['hip_state_abs'] = max(worst['hip_state_abs'], float(np.abs(full_g - full_u).max()))
        bitwise_efforts = bitwise_efforts and np.array_equal(g[:, eff], u[:, eff])
        assert np.array_equal(full_g[:, gpu.layout.physical_dim:], full_u[:, gpu.layout.physical_dim:])   # (contact impulse cache: empty in both)
    print('%s fused vs oracle / fused vs unfused: %s; applied efforts bitwise equal to the unfused path: %s' % (name, worst, bitwise_efforts))
    assert worst['obs'] < OBS_TOL and worst['obs_eff'] < EFFORT_REL_TOL, worst
    assert worst['kin'] < OBS_TOL and worst['eff'] < EFFORT_REL_TOL, worst
    assert worst['hip_obs'] < OBS_TOL and worst['hip_kin'] < OBS_TOL and worst['hip_eff'] < EFFORT_REL_TOL, worst


def test_active_limit_rows_and_pinning_on_the_fused_path():
    """Both elbows start a hair inside their lower limit (the set-up of
    test_motors_pushing_into_joint_limits_start_at_their_fixed_point): active limit rows, pinned limit impulses and the
    limit copy of the sweep loop inside the fused path.  10 random IK steps against the oracle."""
    gpu, cpu = make_pair('ur_ik', B)
    L = gpu.layout
    st = np.array(cpu.sim.get_state())
    for arm in range(2):
        o = L.link_state_off[6 * arm + 2]
        st[:, o] = -np.pi + 1e-4 * (1 + np.arange(B) % 5); st[:, o + 1] = 0.0
    gpu.sim.set_state(st); cpu.sim.set_state(st)
    d = gpu.sim.enable_diagnostics()
    lo, hi = action_bounds(gpu)
    gen = torch.Generator().manual_seed(7)
    worst_obs = 0.0; worst_it = most_it = saturated = 0
    for _ in range(10):
        act = lo + (hi - lo) * torch.rand((B, lo.numel()), generator=gen)
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); cpu.sim.step(cpu._all_slots, act)
        worst_obs = max(worst_obs, float((gpu.sim.obs.cpu() - cpu.sim.obs).abs().max()))
        itc = np.array([cpu.sim.iterations(e) for e in range(B)]); itg = d[:, 1].cpu().numpy()
        worst_it = max(worst_it, int(np.abs(itg - itc).max())); most_it = max(most_it, int(itc.max()), int(itg.max()))
        a = np.asarray(cpu.sim.get_state()); g = np.asarray(gpu.sim.get_state())
        for arm in range(2):
            o = L.link_state_off[6 * arm + 2] + 5   # DG_LS_APPLIED of the elbow
            sat = np.abs(np.abs(a[:, o]) - 150.0) < 1e-3
            saturated += int(sat.sum())
            assert np.abs(g[sat, o] - a[sat, o]).max(initial=0.0) < 1e-2   # the same elbows are pinned, at the same (saturated) effort
    print('limit rows on the fused path: obs %.3g, iterations off by %d, most %d, saturated elbow-steps %d' % (worst_obs, worst_it, most_it, saturated))
    assert worst_obs < OBS_TOL, worst_obs
    assert saturated >= 1, saturated          # pinning happened
    assert worst_it <= 3 and most_it < 60, (worst_it, most_it)   # (the cap is 150 sweeps)


def test_masked_reset_through_the_reset_kernel():
    """reset(mask) of envs 1, 40 and 65 -- a lane below 32, a lane above 32 and the partial workgroup: the hot-start step of
    reset_kernel_par takes the fused path with its stores predicated on the reset mask of the lane's own env."""
    gpu, cpu = make_pair('ur_ik', B)
    lo, hi = action_bounds(gpu)
    gen = torch.Generator().manual_seed(3)
    for _ in range(4):
        act = lo + (hi - lo) * torch.rand((B, lo.numel()), generator=gen)
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); cpu.sim.step(cpu._all_slots, act)
    mask = torch.zeros(B, dtype=torch.uint8); mask[[1, 40, 65]] = 1
    before = np.array(gpu.sim.get_state())
    gpu.sim.reset(mask.to(gpu.device)); cpu.sim.reset(mask)
    after = np.array(gpu.sim.get_state())
    keep = (mask == 0).numpy()
    assert np.array_equal(before[keep].view(np.uint32), after[keep].view(np.uint32))   # every other env: not a bit changed
    assert not np.array_equal(before[~keep], after[~keep])
    k, e = state_errors(phys_state(gpu)[~keep], phys_state(cpu)[~keep], gpu)
    print('masked reset, reset envs against the oracle: kinematic %.3g, efforts (relative) %.3g' % (k, e))
    assert k < OBS_TOL and e < EFFORT_REL_TOL, (k, e)


def test_switching_between_the_fused_and_the_contact_path():
    """ur_arms_touching (capsule narrow phase, as the other tests run it): the arms start in contact and separate, so the
    workgroup changes between the contact path and the fused path from substep to substep."""
    n = 37
    gpu, cpu = make_pair('touching', n)
    d = gpu.sim.enable_diagnostics()
    lo, hi = action_bounds(gpu)
    gen = torch.Generator().manual_seed(0)
    worst = 0.0; term_mismatch = 0; with_contact = free = 0
    for _ in range(30):
        act = (lo + (hi - lo) * torch.rand((n, lo.numel()), generator=gen)) * 0.3
        gpu.sim.step(gpu._all_slots, act.to(gpu.device)); cpu.sim.step(cpu._all_slots, act)
        worst = max(worst, float((gpu.sim.obs.cpu() - cpu.sim.obs).abs().max()))
        term_mismatch += int((gpu.sim.term.cpu() != cpu.sim.term).sum())
        for col in (0, 3):   # contacts of the step's last and first substep; one workgroup: it is contact-free when every env is
            if int(d[:, col].max()) > 0:
                with_contact += 1
            else:
                free += 1
    print('touching: obs %.3g, substeps with a contact in the workgroup %d, without %d' % (worst, with_contact, free))
    assert worst < 3e-3 and term_mismatch == 0, (worst, term_mismatch)
    assert with_contact > 0 and free > 0, (with_contact, free)
