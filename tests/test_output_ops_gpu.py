"""The observe, reward and terminal ops of the HIP kernels against the fp64 restatement of tests/output_ops_ref.py, in every kernel
form a scene can take: what a trainer sees -- observation columns, reward columns, terminal bytes, the collapsed reward and the
collapsed terminal flag -- at the edges the shipped scenes never visit (tests/output_ops_cases.py has the scenes and ladders).

70 envs: one full wavefront plus a tail of 6, every env with a state of its own; one run at 1 env.  Each world is created under the
form's DG_* switches and the run asserts the form taken (``debug_plan`` under the same switches, ``sim.lanes``, ``sim.par``,
``sim.kernel_name``).  Tolerances are ``output_ops_ref.TOL``, fixed on the CPU from the two oracle builds
(tests/test_output_ops_ref.py), plus the two terms of the Euler formula written there; never from what the kernels give.

A  edge states written into ``sim.state``, one ``observe()`` launch;
B  three seeded steps from the edge states: a step's outputs equal ``observe()`` of the state it leaves (within 2 x tolerance: each
   is within one of fp64) and both equal fp64 on the state read back; terminal bytes exact but for envs within one margin of a
   threshold, at most 5 % of a run (0 % in A);
C  in both: every column of every real env is overwritten (force/torque columns included), ``rew_sum`` is bit for bit the float32
   sum of the reward columns in op order, ``term_flag`` is the collapse of the bytes written;
D  ``reset(mask)``: masked rows equal ``observe()``, unmasked rows keep their bits (``reset_kernel<L>`` used to rewrite every row of
   a wavefront that held a reset env; fixed with this test).

Measured on an MI355X (DESIGN.md "Output ops against fp64" has the table per form): the generic scenes stay below 0.3 of the table
against fp64, the arm scenes reach 0.90 (rebuilt rotation) and, in one env of one_arm, 0.996 (angular velocity of an arm link); a
step against ``observe()`` at most 0.15 of twice the table; no env near a threshold after a step.  No allowance is made for the
kernels' hardware sine and cosine: nothing exceeds the bare table.
"""
import numpy as np
import pytest
import torch

import output_ops_cases as C
import output_ops_ref as R
from diy_gym_amd.backend import debug_plan

pytestmark = pytest.mark.gpu

B = 70
SENTINEL, SENTINEL_BYTE = -12345.678, 0xAB
LANES = [({}, 64), ({'DG_MAX_LANES': '32'}, 32), ({'DG_MAX_LANES': '16'}, 16), ({'DG_MAX_LANES': '8'}, 8), ({'DG_MAX_LANES': '4'}, 4), ({'DG_MAX_LANES': '1'}, 1)]
# (scene, switches, envs, form): form = lanes of step_kernel<lanes> (0: the global workspace), or the plan fields of step_kernel_par
PAR = dict(par=1, split_pgs=1, coll_wave=0, early_dyn=0, coll_split=0)            # two arms and a free body: helper wave, split sweeps
HANDOVER = dict(par=1, split_pgs=2, coll_wave=1, early_dyn=1, coll_split=1)       # two arms alone under ik_controller
ONE_ARM = dict(par=1, split_pgs=0, coll_wave=0, early_dyn=0, coll_split=0)
OBSERVE = ([('generic', sw, B, lanes) for sw, lanes in LANES] + [('generic', {}, 1, 64), ('generic_all', {}, B, 64), ('generic_all', {'DG_MAX_LANES': '4'}, B, 4),
           ('joints', {}, B, 1), ('joints', {'DG_MAX_LANES': '16'}, B, 16), ('drone', {}, B, 64), ('drone', {'DG_MAX_LANES': '4'}, B, 4),
           ('arms', {}, B, PAR), ('arms', {}, 1, PAR), ('arms', {'DG_MAX_LANES': '16'}, B, 16), ('arms', {'DG_MAX_LANES': '4'}, B, 0),
           ('arms_ik', {}, B, PAR), ('pair_ik', {}, B, HANDOVER), ('one_arm', {}, B, ONE_ARM)])
STEPS = ([('generic', sw, B, lanes) for sw, lanes in LANES] + [('generic_all', {}, B, 64),
         ('arms', {}, B, PAR), ('arms', {'DG_NO_HELPER_WAVE': '1'}, B, 64), ('arms', {'DG_NO_SPLIT_SWEEPS': '1'}, B, dict(PAR, split_pgs=0)),
         ('arms', {'DG_MAX_LANES': '4'}, B, 0), ('arms_ik', {}, B, PAR), ('one_arm', {}, B, ONE_ARM),
         ('pair_ik', {}, B, HANDOVER), ('pair_ik', {'DG_NO_HELPER_WAVE': '1'}, B, 64), ('pair_ik', {'DG_NO_SPLIT_SWEEPS': '1'}, B, dict(HANDOVER, split_pgs=0)),
         ('pair_ik', {'DG_NO_EARLY_DYNAMICS': '1'}, B, dict(HANDOVER, early_dyn=0)), ('pair_ik', {'DG_NO_COLLIDE_SPLIT': '1'}, B, dict(HANDOVER, coll_split=0)),
         ('pair_ik', {'DG_NO_SPLIT_CONTACTS': '1'}, B, dict(HANDOVER, split_pgs=1))])
RESETS = [('generic', {'DG_MAX_LANES': '4'}, 4), ('generic', {}, 64), ('arms', {}, PAR), ('arms', {'DG_NO_PAR_RESET': '1'}, PAR), ('pair_ik', {}, HANDOVER)]


def _id(run):
    return '%s-%s-x%s' % (run[0], '_'.join('%s=%s' % kv for kv in run[1].items()) or 'default', run[2] if len(run) == 4 else 134)


def world(scene, sw, n, form, monkeypatch):
    """The HIP world of ``scene`` created under the switches ``sw``; asserts the kernel form."""
    with monkeypatch.context() as m:   # the switches are read while the world is created
        for k, v in sw.items():
            m.setenv(k, v)
        env = C.make_env(scene, n, device='cuda:0')
        plan = debug_plan(env.layout, n)
    sim = env.sim
    what = (scene, sw, n, sim.lanes, sim.kernel_name, {k: plan[k] for k in ('lanes', 'par', 'split_pgs', 'coll_wave', 'early_dyn', 'coll_split')})
    assert sim.lanes == plan['lanes'] and bool(plan['par']) == sim.par, what
    if isinstance(form, dict):
        assert sim.par and sim.lanes == 64 and sim.kernel_name.startswith('step_kernel_par'), what
        assert all(plan[k] == v for k, v in form.items()), what
    else:
        assert not sim.par and sim.lanes == form and sim.kernel_name == 'step_kernel<%d>' % form, what
    return env


def prefill(sim):
    sim.obs.fill_(SENTINEL)
    sim.rew.fill_(SENTINEL)
    sim.term.fill_(SENTINEL_BYTE)
    sim.rew_sum.fill_(SENTINEL)
    sim.term_flag.fill_(SENTINEL_BYTE)


def check_invariants(ref, res, got, what):
    """C: nothing left unwritten, the collapsed outputs follow from the columns written."""
    L = ref.layout
    assert np.isfinite(got['obs'][:, :L.obs_dim]).all() and (got['obs'][:, :L.obs_dim] != np.float32(SENTINEL)).all(), (what, 'an observation column kept the sentinel')
    assert L.rew_dim == 0 or (got['rew'][:, :L.rew_dim] != np.float32(SENTINEL)).all(), (what, 'a reward column kept the sentinel')
    assert np.isin(got['term'][:, :L.term_dim], (0, 1)).all() and np.isin(got['term_flag'], (0, 1)).all(), (what, 'a terminal byte kept the sentinel')
    want = R.f32_sum_in_order(got['rew'], L.rew_dim)
    assert np.array_equal(want.view(np.uint32), got['rew_sum'].astype(np.float32).view(np.uint32)), (what, 'rew_sum is not the float32 sum of its columns',
                                                                                                    np.nonzero(want != got['rew_sum'])[0][:8])
    assert np.array_equal(ref.collapse(got['term'], res.term_group), got['term_flag']), (what, 'term_flag is not the collapse of the bytes written')


def as_reference(res, got):
    """``res`` with the continuous values (and rebuilt rotations) of ``got`` in place of fp64's: the reference of step against observe."""
    import copy
    r = copy.copy(res)
    r.obs, r.rew, r.term, r.rew_sum = np.where(np.isnan(res.obs), np.nan, got['obs'].astype(np.float64)), got['rew'].astype(np.float64), got['term'], got['rew_sum'].astype(np.float64)
    r.term_flag = got['term_flag']
    r.rots = [dict(rot, R=np.stack([R.euler_matrix(got['obs'][e, rot['off']:rot['off'] + 3]) for e in range(got['obs'].shape[0])])) for rot in res.rots]
    return r


def show(what, rep):
    print('%s: %s; near a threshold %d' % (what, ' '.join('%s %.3g' % kv for kv in sorted(rep.figures.items())), int(rep.near.sum())))


@pytest.mark.parametrize('run', OBSERVE, ids=_id)
def test_edges_through_observe(run, monkeypatch):
    scene, sw, n, form = run
    env = world(scene, sw, n, form, monkeypatch)
    sim, ref = env.sim, R.OutputRef(env)
    states = C.edge_states(scene, env, ref, n, seed=0)
    sim.set_state(states)
    prefill(sim)
    sim.observe()
    got = R.outputs_of(sim)
    res = ref.evaluate(states)
    what = (scene, sw, n, sim.kernel_name)
    check_invariants(ref, res, got, what)
    rep = R.compare(res, got)
    show('observe %s %s x%d %s (fractions of the tolerance)' % (scene, sw, n, sim.kernel_name), rep)
    assert rep.ok, (what, rep.bad)
    assert rep.near.sum() == 0, (what, 'a ladder env within a margin of a threshold', np.nonzero(rep.near)[0])
    if n == B and scene in ('generic', 'arms'):   # the ladders as the kernels got them: every branch of the matrix conversion, both gimbal branches
        frame = {'generic': ('cart', 'hinge_b'), 'arms': ('ur5_l', 'wrist_2_joint')}[scene]
        count = np.bincount(res.branches[frame[0], env.models[frame[0]].get_frame_id(frame[1])], minlength=4)
        assert (count >= 8).all(), (what, count)
        assert max(int((np.abs(rot['sarg']) >= R.GIMBAL).sum()) for rot in res.rots) >= 10, what


@pytest.mark.parametrize('run', STEPS, ids=_id)
def test_a_step_writes_what_observe_sees_in_the_state_it_leaves(run, monkeypatch):
    scene, sw, n, form = run
    env = world(scene, sw, n, form, monkeypatch)
    sim, ref = env.sim, R.OutputRef(env)
    sim.set_state(C.edge_states(scene, env, ref, n, seed=0))
    gen = torch.Generator().manual_seed(7)
    what = (scene, sw, n, sim.kernel_name)
    for step in range(3):
        act = C.seeded_actions(env, gen).to(sim.device)
        prefill(sim)
        sim.step(env._all_slots, act)
        stepped = R.outputs_of(sim)
        back = np.asarray(sim.get_state(), dtype=np.float64)
        prefill(sim)
        sim.observe()
        observed = R.outputs_of(sim)
        assert np.array_equal(back.astype(np.float32).view(np.uint32), np.asarray(sim.get_state(), dtype=np.float32).view(np.uint32)), (what, 'observe() touched the state')
        res = ref.evaluate(back)
        for name, got in (('step', stepped), ('observe', observed)):
            check_invariants(ref, res, got, what + (step, name))
            rep = R.compare(res, got)
            show('%s %d of %s %s %s against fp64' % (name, step, scene, sw, sim.kernel_name), rep)
            assert rep.ok, (what, step, name, rep.bad)
            assert rep.near.sum() <= 0.05 * n, (what, step, 'more than 5 % of the envs within a margin of a threshold', int(rep.near.sum()))
        pair = R.compare(as_reference(res, observed), stepped, slack=2.0)
        show('step %d against observe of %s %s %s (fractions of twice the tolerance)' % (step, scene, sw, sim.kernel_name), pair)
        assert pair.ok, (what, step, 'step against observe', pair.bad)
        if 'marble' in env.models:
            # the marble's gimbal poses (10 envs) carry no angular velocity: free fall keeps them, so the step's own output phase meets
            # the branch.  Beside the arms the marble falls free; in the generic scene the cart's links reach some of them.
            pose = [rot for rot in res.rots if rot['off'] == env.models['marble'].addons['pose'].op.io_off + 6][0]
            kept = int((np.abs(pose['sarg']) >= R.GIMBAL).sum())
            print('step %d of %s: marble envs still in a gimbal branch %d' % (step, scene, kept))
            assert kept >= (4 if scene.startswith("generic") else 6), (what, step, kept)


@pytest.mark.parametrize('run', RESETS, ids=_id)
def test_masked_reset_writes_the_masked_rows_only(run, monkeypatch):
    """134 envs (at 64 per workgroup: two full workgroups and a tail of 6); the mask names envs 15, 16, 63, 64 and 65 -- both sides of
    the boundaries of a workgroup of 16 and of 64, every rung of the timer ladder -- and leaves the last workgroup (and at 16 or 4 per workgroup most of them)
    without any."""
    scene, sw, form = run
    n = 134
    env = world(scene, sw, n, form, monkeypatch)
    assert env.hot_start == 1   # reset_kernel_par (or, without it, reset_kernel<L>) with its one hot-start step: with 0 every scene takes reset_kernel<L>
    sim, ref = env.sim, R.OutputRef(env)
    sim.set_state(C.edge_states(scene, env, ref, n, seed=0))
    sim.observe()
    before = sim.obs.clone()
    rows = [15, 16, 63, 64, 65]
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[rows] = 1
    sim.reset(mask.to(sim.device))
    after = sim.obs.clone()
    keep = (mask == 0).numpy()
    assert np.array_equal(before.cpu().numpy()[keep].view(np.uint32), after.cpu().numpy()[keep].view(np.uint32)), (run, 'an unmasked row changed')
    state = np.asarray(sim.get_state(), dtype=np.float64)
    sim.observe()
    observed = R.outputs_of(sim, rows)
    reset = dict(observed, obs=after.cpu().numpy()[rows])
    res = ref.evaluate(state[rows])
    for name, got in (('reset', reset), ('observe', observed)):
        rep = R.compare(res, got)
        show('%s of %s %s %s against fp64' % (name, scene, sw, sim.kernel_name), rep)
        assert rep.ok, (run, name, rep.bad)
    pair = R.compare(as_reference(res, observed), reset, slack=2.0)
    assert pair.ok, (run, 'reset against observe', pair.bad)
