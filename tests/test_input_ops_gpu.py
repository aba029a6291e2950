"""The update ops, the reset ops and the external wrench entry of the HIP kernels against the fp64 restatement of
tests/input_ops_ref.py, in every kernel form a scene can take: what an action row, a wrench call and a reset write into the state
(tests/input_ops_cases.py has the scenes and ladders).

70 envs: one full wavefront plus a tail of 6, every env with a state of its own; one run at 1 env; the resets at 134.  Worlds are
created, and their forms asserted, by ``world()`` of tests/test_output_ops_gpu.py with its ``LANES``, ``PAR``, ``HANDOVER`` and
``ONE_ARM`` tables.  Tolerances are ``input_ops_ref.TOL``, fixed on the CPU from the two oracle builds
(tests/test_input_ops_ref.py), with no term for the kernels' hardware sine and cosine; never from what the kernels give.

A  ``sim.apply_external_force / _wrench / _torque`` (device rows, host rows, one vector for all envs) on the edge states: the base, every frame of the cart (prismatic and revolute
   ancestors, a frame on a massless link, a frame bolted to the base), the marble, a UR5 wrist; WORLD and LINK frame; one row per
   env and one 3-vector for all; the calls accumulate; no cell outside the body's wrench and its joints' torques changes a bit;
B  one ``sim.step`` under DG_DEBUG_KEEP_EXT=1: the wrench, torque, target and rotor cells read back equal ``InputRef.update`` of
   the pre-step state -- with a wrench and joint torques applied from Python before the step still there, on torque-mode joints
   too -- in every form of the step kernel and each ablation of the four-wavefront kernel (an op that ran on two wavefronts or
   on none shows: the adding ops double or vanish); with half of the slots masked; with no slot; from the staged action buffer;
C  hot_start 0: three successive resets of 134 envs, then a masked reset of envs 15, 16, 63, 64, 65: every cell the reference
   names, unmasked rows bit for bit; the envs whose episode counter stands at 2^24 repeat their draws; a shard draws what its envs
   draw in the whole batch;
D  hot_start 1: the cells one physics step cannot touch (addon state, counters, the pose of a fixed base).

The reset kernel follows the world's form (``reset_kernel<L>`` with the step kernel's lanes, ``<0>`` in the global workspace,
``reset_kernel_par`` for a four-wavefront scene with a hot start unless DG_NO_PAR_RESET); the step form and ``hot_start`` are asserted.

Measured on an MI355X (DESIGN.md "Update and reset ops against fp64" has the table per form): the wrench entry stays below 0.25 of the
table, a step below 0.21 (the drone's moments), the resets below 0.39 (damping) -- the same figures in every form of a scene.
Found with these tests and fixed: torque mode overwrote the torque cell (nine runs of B fail against the parent's library), and
``apply_external_force / _wrench`` read force, point and torque from one block whenever they had to convert their arguments.
"""
import numpy as np
import pytest
import torch

import input_ops_cases as C
import input_ops_ref as R
import test_output_ops_gpu as G
from diy_gym_amd.scene import K
from test_output_ops_gpu import HANDOVER, LANES, ONE_ARM, PAR

pytestmark = pytest.mark.gpu

B, SEED = 70, 5
KEEP = {'DG_DEBUG_KEEP_EXT': '1'}
PAIR_ADM = dict(par=1, split_pgs=2, coll_wave=1, early_dyn=0, coll_split=1)   # two arms alone with a torque op: no early dynamics
WRENCH = [('generic', sw, B, lanes) for sw, lanes in LANES] + [('generic', {}, 1, 64), ('arms', {}, B, PAR), ('arms', {'DG_MAX_LANES': '16'}, B, 16), ('arms', {'DG_MAX_LANES': '4'}, B, 0)]
STEPS = ([('generic', sw, B, lanes) for sw, lanes in LANES] + [('generic', {}, 1, 64), ('generic_vel', {}, B, 64), ('generic_torque', {}, B, 64), ('generic_torque', {'DG_MAX_LANES': '4'}, B, 4),
         ('drone', {}, B, 64), ('drone', {'DG_MAX_LANES': '4'}, B, 4),
         ('arms', {}, B, PAR), ('arms', {'DG_NO_HELPER_WAVE': '1'}, B, 64), ('arms', {'DG_NO_SPLIT_SWEEPS': '1'}, B, dict(PAR, split_pgs=0)),
         ('arms', {'DG_MAX_LANES': '4'}, B, 0), ('one_arm', {}, B, ONE_ARM),
         ('pair', {}, B, HANDOVER), ('pair', {'DG_NO_HELPER_WAVE': '1'}, B, 64), ('pair', {'DG_NO_SPLIT_SWEEPS': '1'}, B, dict(HANDOVER, split_pgs=0)),
         ('pair', {'DG_NO_EARLY_DYNAMICS': '1'}, B, dict(HANDOVER, early_dyn=0)), ('pair', {'DG_NO_COLLIDE_SPLIT': '1'}, B, dict(HANDOVER, coll_split=0)),
         ('pair', {'DG_NO_SPLIT_CONTACTS': '1'}, B, dict(HANDOVER, split_pgs=1)),
         ('pair_adm', {}, B, PAIR_ADM), ('pair_adm', {'DG_NO_COLLIDE_SPLIT': '1'}, B, dict(PAIR_ADM, coll_split=0)), ('pair_adm', {'DG_NO_SPLIT_CONTACTS': '1'}, B, dict(PAIR_ADM, split_pgs=1))])
RESETS0 = ([('generic', sw, lanes) for sw, lanes in LANES] + [('generic', {'DG_NO_SLICED_RESET': '1'}, 64), ('generic_vel', {}, 64), ('drone', {}, 64),
           ('arms', {}, PAR), ('arms', {'DG_MAX_LANES': '16'}, 16), ('arms', {'DG_MAX_LANES': '4'}, 0), ('arms', {'DG_NO_SLICED_RESET': '1'}, PAR), ('pair', {}, HANDOVER)])
RESETS1 = [('arms', {}, PAR), ('arms', {'DG_NO_PAR_RESET': '1'}, PAR), ('generic', {'DG_MAX_LANES': '4'}, 4), ('generic', {}, 64), ('pair', {}, HANDOVER)]
MASKED = [15, 16, 63, 64, 65]


def world(scene, sw, n, form, monkeypatch, hot_start=0, env_index_base=0):
    """``world()`` of the output-op tests over the scenes of tests/input_ops_cases.py: creates the HIP world under the switches and
    asserts the form taken."""
    class Cases:
        make_env = staticmethod(lambda s, b, device=None: C.make_env(s, b, hot_start=hot_start, device=device, seed=SEED, env_index_base=env_index_base))
    with monkeypatch.context() as m:
        m.setattr(G, 'C', Cases)
        env = G.world(scene, sw, n, form, monkeypatch)
    assert env.hot_start == hot_start
    return env


def state_of(sim):
    return np.array(np.asarray(sim.get_state(), dtype=np.float32))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def show(what, rep):
    print('%s: %s' % (what, ' '.join('%s %.3g' % kv for kv in sorted(rep.figures.items()))))


def untouched(cells, before, after, what):
    others = np.setdiff1d(np.arange(before.shape[1]), cells.columns())
    diff = before[:, others].view(np.uint32) != after[:, others].view(np.uint32)
    assert not diff.any(), (what, 'a cell the reference does not name changed: columns', others[diff.any(axis=0)][:8], 'envs', np.nonzero(diff.any(axis=1))[0][:8])


# ---- A: the wrench entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', WRENCH, ids=G._id)
def test_wrench_entry(run, monkeypatch):
    scene, sw, n, form = run
    env = world(scene, sw, n, form, monkeypatch)
    sim, ref = env.sim, R.InputRef(env)
    sim.set_state(C.edge_states(scene, env, ref, n, seed=0))
    rng = np.random.default_rng(11)
    worst = {}
    for name, frame_name in C.wrench_targets(scene):
        m = env.models[name]
        fr = -1 if frame_name is None else m.get_frame_id(frame_name)
        for flags in (sim.WORLD_FRAME, sim.LINK_FRAME):
            link = flags == sim.LINK_FRAME
            before = state_of(sim)
            f, p, t, one = (torch.tensor(v, dtype=torch.float32) for v in C.wrench_rows(ref, before, name, rng, not link))
            calls = [('force rows', lambda: sim.apply_external_force(m.uid, fr, f.to(sim.device), p.to(sim.device), flags), dict(f=f.numpy(), pos=p.numpy())),
                     ('wrench one vector', lambda: sim.apply_external_wrench(m.uid, fr, one, p[0], -one, flags), dict(f=one.numpy(), pos=p[0].numpy(), t=-one.numpy())),
                     ('torque rows', lambda: sim.apply_external_torque(m.uid, fr, t.to(sim.device), flags), dict(t=t.numpy())),
                     # (host rows: each of the three is converted into a device temporary of its own)
                     ('wrench host rows', lambda: sim.apply_external_wrench(m.uid, fr, t, p, f, flags), dict(f=t.numpy(), pos=p.numpy(), t=f.numpy()))]
            for label, call, kw in calls:   # (the three accumulate: each is compared on top of the state the one before left)
                cells = ref.wrench(before, name, fr, link, **kw)
                call()
                after = state_of(sim)
                what = (scene, sw, n, sim.kernel_name, name, frame_name, 'LINK' if link else 'WORLD', label)
                rep = R.compare(cells, after)
                assert rep.ok, '%s %s' % (what, rep.bad)
                untouched(cells, before, after, str(what))
                for k, v in rep.figures.items():
                    worst[k] = max(worst.get(k, 0.0), v)
                before = after
    print('wrench entry %s %s x%d %s (fractions of the tolerance): %s' % (scene, sw, n, sim.kernel_name, ' '.join('%s %.3g' % kv for kv in sorted(worst.items()))))


# ---- B: the update ops through a step ----------------------------------------------------------------------------------------------
def python_side(env, sim, ref, rng, n):
    """What a Python addon does before a step: a wrench on every free body (on the last link of a jointed one, so that its joints'
    torque cells are loaded too) and joint torques on every fixed-base arm, the torque-mode ones included."""
    rows = lambda lim, k=3: torch.tensor(rng.uniform(-lim, lim, (n, k)), dtype=torch.float32)
    for name, b in ref.bodies.items():
        m = env.models[name]
        if b.frozen:
            continue
        if not b.fixed:
            fr = len(m.robot.joints) - 2 if m.robot.num_dofs else -1   # (the cart: tip_joint, on the slider-and-hinge branch)
            sim.apply_external_wrench(m.uid, fr, rows(3.0), rows(0.2), rows(1.0), sim.LINK_FRAME)
            if m.robot.num_dofs:
                sim.apply_external_torque(m.uid, m.get_frame_id('hinge_b'), rows(1.0), sim.WORLD_FRAME)
        elif m.robot.num_dofs:
            sim.apply_joint_torque(m.uid, rows(2.0, m.robot.num_dofs).to(sim.device))


@pytest.mark.parametrize('run', STEPS, ids=G._id)
def test_update_ops_through_a_step(run, monkeypatch):
    scene, sw, n, form = run
    env = world(scene, dict(sw, **KEEP), n, form, monkeypatch)
    sim, ref = env.sim, R.InputRef(env)
    states = C.edge_states(scene, env, ref, n, seed=0)
    act = C.actions(env, n)
    half = sum(1 << a.op.slot for a in ref.update_addons[::2])
    rng = np.random.default_rng(13)
    for label, mask, python, staged in (('all slots', env._all_slots, False, False), ('all slots on top of Python-side torques', env._all_slots, True, False),
                                        ('half of the slots', half, True, False), ('no slot', 0, True, False), ('the staged action buffer', env._all_slots, False, True)):
        sim.set_state(states)
        if python:
            python_side(env, sim, ref, rng, n)
        pre = state_of(sim)
        if python:
            assert not same_bits(pre, states), 'the Python-side calls left no trace'
        if staged:
            sim.act.copy_(act.to(sim.device))
            sim.step(mask)
        else:
            sim.step(mask, act.to(sim.device))
        post = state_of(sim)
        cells = ref.update(pre, act.numpy(), mask)
        rep = R.compare(cells, post)
        what = (scene, sw, n, sim.kernel_name, label)
        show('update ops %s %s x%d %s, %s (fractions of the tolerance)' % (scene, sw, n, sim.kernel_name, label), rep)
        assert rep.ok, (what, rep.bad)
        if mask == 0:   # nothing applied: every named cell keeps its bits
            cols = [c for c in cells.columns() if cells.col[c][0] != 'skip']
            assert same_bits(pre[:, cols], post[:, cols]), what


# ---- C, D, E: the reset ops --------------------------------------------------------------------------------------------------------
def stable(cells, env, ref):
    """The cells one physics step cannot touch: addon state that no sensor rewrites (mass scales, damping, texture), the counters,
    the pose of a fixed base."""
    keep = R.Cells(cells.B)
    fixed = [env.layout.body_state_off[b.body] for b in ref.bodies.values() if b.fixed and not b.frozen]
    for c, v in cells.col.items():
        if v[0] in ('mass', 'damp', 'freq') or c in (K.ST_STEP, K.ST_EPISODE) or any(so <= c < so + 3 for so in fixed) or \
                any(type(a).__name__ == 'VisualRandomizer' and 0 <= c - env.layout.addon_off - a.op.state_off < K.TX_STRIDE for a in ref.reset_addons):
            keep.col[c] = v
    keep.quats = {c: q for c, q in cells.quats.items() if c - K.BS_QUAT in fixed}
    return keep


def reset_run(scene, sw, form, monkeypatch, hot_start, n=134, base=0):
    env = world(scene, sw, n, form, monkeypatch, hot_start=hot_start, env_index_base=base)
    sim, ref = env.sim, R.InputRef(env)
    sim.set_state(C.edge_states(scene, env, ref, n, seed=0))
    pick = (lambda c: stable(c, env, ref)) if hot_start else (lambda c: c)
    index = base + np.arange(n)
    history = []
    for ep in range(3):
        pre = state_of(sim)
        cells = pick(ref.reset(pre, index, SEED))
        sim.reset()
        post = state_of(sim)
        rep = R.compare(cells, post)
        what = (scene, sw, n, sim.kernel_name, 'hot_start', hot_start, 'reset', ep)
        show('reset ops %s %s x%d hot_start %d, reset %d (fractions of the tolerance)' % (scene, sw, n, hot_start, ep), rep)
        assert rep.ok, (what, rep.bad)
        if not hot_start:
            untouched(cells, pre, post, what)
        history.append(post)
    pre = state_of(sim)
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[MASKED] = 1
    sim.reset(mask.to(sim.device))
    post = state_of(sim)
    keep = (mask == 0).numpy()
    assert same_bits(pre[keep], post[keep]), (scene, sw, 'an unmasked row changed')
    cells = pick(ref.reset(pre[MASKED], index[MASKED], SEED))
    rep = R.compare(cells, post[MASKED])
    assert rep.ok, (scene, sw, 'masked reset', rep.bad)
    assert not same_bits(pre[MASKED][:, K.ST_EPISODE], post[MASKED][:, K.ST_EPISODE]) or (pre[MASKED][:, K.ST_EPISODE] >= 2 ** 24).all()
    return env, ref, history


@pytest.mark.parametrize('run', RESETS0, ids=G._id)
def test_reset_ops(run, monkeypatch):
    scene, sw, form = run
    env, ref, history = reset_run(scene, sw, form, monkeypatch, 0)
    # E: the episode counter is a float32 cell; at 2^24 it no longer advances and the env repeats the draws of episode 2^24 + 1
    ladder = np.asarray(C.EPISODES)[np.arange(134) % C.P % len(C.EPISODES)]
    top, low = ladder == 2 ** 24, ladder < 1000
    assert (history[0][top, K.ST_EPISODE] == 2 ** 24).all() and (history[2][top, K.ST_EPISODE] == 2 ** 24).all() and (history[2][low, K.ST_EPISODE] == ladder[low] + 3).all()
    jittered = [env.layout.body_state_off[a.parent.uid] for a in ref.reset_addons if type(a).__name__ == 'Respawn' and not a.once]
    assert jittered
    for so in jittered:   # position and quaternion of every respawned base
        assert same_bits(history[1][top, so:so + 7], history[2][top, so:so + 7]) and not same_bits(history[1][low, so:so + 7], history[2][low, so:so + 7]), (run, so)


@pytest.mark.parametrize('run', RESETS1, ids=G._id)
def test_reset_ops_under_a_hot_start(run, monkeypatch):
    scene, sw, form = run
    reset_run(scene, sw, form, monkeypatch, 1)


def test_a_shard_draws_what_its_envs_draw_in_the_whole_batch(monkeypatch):
    """A world created with ``env_index_base`` 64 and 70 envs against envs 64 .. 133 of the whole batch, from the same rows."""
    whole = world('generic', {}, 134, 64, monkeypatch)
    shard = world('generic', {}, B, 64, monkeypatch, env_index_base=64)
    ref = R.InputRef(whole)
    states = C.edge_states('generic', whole, ref, 134, seed=0)
    whole.sim.set_state(states)
    shard.sim.set_state(states[64:])
    for ep in range(2):
        pre = state_of(shard.sim)
        whole.sim.reset()
        shard.sim.reset()
        assert same_bits(state_of(whole.sim)[64:], state_of(shard.sim)), ep
        rep = R.compare(R.InputRef(shard).reset(pre, 64 + np.arange(B), SEED), state_of(shard.sim))
        assert rep.ok, rep.bad
