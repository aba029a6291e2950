"""env.sim.link_states / reset_base_state and the link_state_sensor addon on the GPU.  Worlds of 3 and 70 envs: one partial wavefront,
one wavefront boundary crossed.

1. ``link_states`` against ``frame_state``, row by row, bit for bit (the int32 views are compared: a signed zero counts), after a
   reset and 5 steps of random actions; the state is not written; the buffer is reused.
2. ``reset_base_state`` with the pose a zero-range compiled ``respawn`` holds stores what that op stores, bit for bit, in the masked
   envs and nothing else anywhere -- the contact cache of the masked envs apart, whose count is zero.  cart_tree.yaml is built with
   ``hot_start: 0`` for this: its marble is a floating base, and the reset's hot-start step would move it off the respawn pose.
3. Arbitrary poses and velocities against the fp64 restatement of tests/base_state_ref.py (pinned by tests/test_base_state_ref.py).
   Error measure: the largest absolute difference over the stored base columns and over the 13 columns ``frame_state(uid, -1,
   com=True)`` returns, over the envs.  Poses: positions in [-1, 1]^2 x [1, 3] m, uniformly random orientations handed in with norm
   2, |v| components up to 2 m/s, |w| components up to 3 rad/s.  BOUND is 8 x the largest figure measured over these cases on an
   MI355X (DESIGN.md "Link states and base reset"); the margin is for a compiler that contracts multiply-adds differently, not for
   bugs.  It may not exceed 1e-5.  Measured maxima (MI355X): cart_tree 1.19e-7 (x3) / 3.58e-7 (x70), contacts_marbles 1.62e-8 / 5.24e-8.
4. The step sees the write: a world reset through ``reset_base_state`` and a world whose state was written by hand run to the same
   bits; tests/user_respawn.py respawns a marble from Python under a reset mask.
5. What the calls refuse, in Python and in the C entries themselves: nothing is launched, the state keeps its bits.
6. The link_state_sensor addon reports ``link_states`` of its selectors.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

import base_state_ref as R
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.config import Configuration

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda:0'
MEASURED = 3.58e-7   # largest figure of test_arbitrary_poses_and_velocities over its cases (cart_tree x70; see the docstring)
BOUND = 8 * MEASURED
assert BOUND <= 1e-5
_ENVS = {}


def make(cfg, B, monkeypatch=None, lanes=None, edit=None, tag=None, registry=None):
    """The env of a case, built once per session.  ``lanes``: DG_MAX_LANES while the world is created; ``edit``: a change to the
    config tree (``tag`` names it in the cache); ``registry``: addon classes registered under their names while it is built."""
    key = (cfg, B, lanes, tag)
    if key not in _ENVS:
        if lanes:
            monkeypatch.setenv('DG_MAX_LANES', lanes)
        tree = yaml.safe_load(open(os.path.join(GOLDEN, cfg)))
        if edit:
            edit(tree)
        conf = Configuration.from_dict(os.path.splitext(os.path.basename(cfg))[0], tree)
        conf.source_dir = os.path.dirname(os.path.join(GOLDEN, cfg))
        names = AddonFactory.get().addons
        for name, cls in (registry or {}).items():
            assert name not in names
            AddonFactory.register_addon(name, cls)
        try:
            env = DIYGym(conf, num_envs=B, device=DEV, seed=5)
        finally:
            for name in (registry or {}):
                del names[name]
        if lanes:
            assert env.sim.envs_per_wave == int(lanes)
        _ENVS[key] = env
    return _ENVS[key]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run(env, steps, seed=0, scale=0.01):
    """``steps`` steps of seeded random actions (zeros for a scene without actions)."""
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        act = ((torch.rand((env.sim.num_envs, max(env.layout.act_dim, 1)), generator=gen) * 2 - 1) * scale).to(DEV)
        env.sim.step(env._all_slots, act if env.layout.act_dim else None)


def live(sim):
    """The state of the real envs, [state_dim, B], a copy."""
    return sim.state[:, :sim.num_envs].clone()


def n_frames(model):
    return len(model.flat.frames)


# ------------------------------------------------------------------------------------------------------------ 1. link_states
def selector_lists(env, scene):
    """[(uids, frames)] of a scene: a repeated frame, the base among deep links, 32 selectors, two bodies."""
    m = env.models
    if scene == 'contacts_marbles.yaml':   # all three marbles and the plane (a frozen body) in one call
        uids = [m['red_marble'].uid, m['plane'].uid, m['green_marble'].uid, m['blue_marble'].uid]
        return [(uids, [-1] * 4), (uids[2], [-1, -1])]
    if scene == 'ur5_child_gripper.yaml':   # the merged child by its alias uid, alone and beside its parent
        arm, grip = m['arm'], m['arm'].models['gripper']
        assert grip.uid in env.layout.aliases
        ng, na = n_frames(grip), n_frames(arm)
        assert ng >= 2 and na >= 6
        deep = [(grip.uid, f) for f in range(-1, ng)] + [(arm.uid, f) for f in range(-1, na)]
        wide = (deep * 32)[:32]
        return [(grip.uid, [-1, ng - 1, 0, ng - 1]), ([u for u, _ in deep[:8]] + [arm.uid, grip.uid], [f for _, f in deep[:8]] + [na - 1, -1]),
                ([u for u, _ in wide], [f for _, f in wide])]
    model = m[{'ur_ik.yaml': 'arm', 'jaco_ik.yaml': 'robot', 'cart_tree.yaml': 'cart'}[scene]]
    nf = n_frames(model)
    assert nf >= 3
    out = [(model.uid, [nf - 1, nf - 1, -1, nf // 2, nf - 1]),            # a frame repeated, the base among deep links
           (model.uid, [-1] + list(range(nf - 1, -1, -1))[:31]),          # the base, then every frame from the tip down
           (model.uid, ([-1] + list(range(nf)) * 32)[:32])]               # n = 32
    if scene == 'cart_tree.yaml':   # two bodies and the frozen plane
        out.append(([model.uid, m['marble'].uid, m['plane'].uid, model.uid], [nf - 1, -1, -1, 0]))
    return out


LINK_CASES = [(s, B, None) for s in ('ur_ik.yaml', 'cart_tree.yaml', 'ur5_child_gripper.yaml', 'contacts_marbles.yaml') for B in (3, 70)] + \
             [('jaco_ik.yaml', 3, None), ('jaco_ik.yaml', 3, '1')]


@pytest.mark.parametrize('scene,B,lanes', LINK_CASES)
def test_link_states_equals_frame_state_bit_for_bit(scene, B, lanes, monkeypatch):
    env = make(scene, B, monkeypatch, lanes)
    sim = env.sim
    env.reset()
    run(env, 5, seed=B)
    before = live(sim)
    moving = 0.0
    for uids, frames in selector_lists(env, scene):
        for com in (False, True):
            out = sim.link_states(uids, frames, com=com)
            assert tuple(out.shape) == (B, len(frames), 13) and out.dtype == torch.float32
            got = out.clone()
            for k, f in enumerate(frames):
                b, lf = env.layout.resolve_frame(uids[k] if isinstance(uids, list) else uids, f)
                assert same_bits(got[:, k], sim.frame_state(b, lf, com=com)), (uids, frames, k, com)
            moving = max(moving, float(got[:, :, 7:13].abs().max()))
            again = sim.link_states(uids, list(frames), com=com)
            assert again.data_ptr() == out.data_ptr() and same_bits(again, got)
    assert moving > 0.0   # (velocities were compared on something that moves)
    assert same_bits(live(sim), before)
    assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------------------ 2. the respawn's bits
def _no_hot_start(tree):
    tree['hot_start'] = 0


RESPAWN_CASES = [('np_gem_wedge_respawned.yaml', 'wedge', None), ('cart_tree.yaml', 'marble', _no_hot_start)]


@pytest.mark.parametrize('B', [3, 70])
@pytest.mark.parametrize('scene,name,edit', RESPAWN_CASES)
def test_reset_base_state_writes_what_the_compiled_respawn_writes(scene, name, edit, B):
    env = make(scene, B, edit=edit, tag=edit and edit.__name__)
    sim, model, L = env.sim, env.models[name], env.layout
    uid = model.uid
    assert sim.base_is_movable(uid)
    env.reset()
    cols = R.base_columns(L, uid)
    fresh = live(sim)[cols]
    run(env, 5, seed=1)
    before = live(sim)
    if not L.body_fixed[uid]:
        assert not same_bits(before[cols], fresh)   # (it moved: the call below has something to undo)
    m = (torch.arange(B) % 2 == 0).to(DEV)
    sim.reset_base_state(uid, pos=torch.tensor(model.position, dtype=torch.float64).float(), orn=torch.tensor(model.orientation, dtype=torch.float64).float(), mask=m)
    after = live(sim)
    assert same_bits(after[cols][:, m], fresh[:, m])
    assert same_bits(after[:, ~m], before[:, ~m])
    other = torch.ones(sim.state_dim, dtype=torch.bool, device=DEV)
    other[cols] = False
    if L.warm_off >= 0:
        other[L.warm_off:] = False
        assert float(after[L.warm_off][m].abs().max()) == 0.0
    assert same_bits(after[other], before[other])


# ------------------------------------------------------------------------------------------------------------ 3. the fp64 reference
def draws(B, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.uniform(-1.0, 1.0, (B, 3)) + np.array([0.0, 0.0, 2.0])).astype(np.float32)
    orn = rng.normal(size=(B, 4))
    orn = (2.0 * orn / np.linalg.norm(orn, axis=1, keepdims=True)).astype(np.float32)
    return pos, orn, rng.uniform(-2.0, 2.0, (B, 3)).astype(np.float32), rng.uniform(-3.0, 3.0, (B, 3)).astype(np.float32)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


@pytest.mark.parametrize('B', [3, 70])
@pytest.mark.parametrize('scene,name', [('cart_tree.yaml', 'cart'), ('contacts_marbles.yaml', 'green_marble')])
def test_arbitrary_poses_and_velocities(scene, name, B):
    env = make(scene, B)
    sim, L, uid = env.sim, env.layout, env.models[name].uid
    env.reset()
    run(env, 2, seed=3)
    cols = R.base_columns(L, uid)
    pos, orn, lin, ang = draws(B, 40 + B)
    unit = orn.astype(np.float64) / np.linalg.norm(orn.astype(np.float64), axis=1, keepdims=True)
    stored = lambda: sim.state[cols, :B].t().cpu().numpy()
    report = lambda: sim.frame_state(uid, -1, com=True).cpu().numpy()
    figures = []
    # pose and both velocities
    sim.reset_base_state(uid, pos=dev(pos), orn=dev(orn), lin_vel=dev(lin), ang_vel=dev(ang))
    want = np.concatenate(R.stored_from_report(L, uid, pos, orn, lin, ang), axis=1)
    figures += [err(stored(), want), err(report(), np.concatenate([pos, unit, lin, ang], axis=1))]
    # the pose alone: all six velocity columns are zero
    sim.reset_base_state(uid, pos=dev(pos), orn=dev(orn))
    s = stored()
    assert not s[:, 7:13].any()
    figures += [err(s, np.concatenate(R.stored_from_report(L, uid, pos, orn), axis=1))]
    # the velocities alone: the pose columns keep their bits
    pose_before = sim.state[cols, :B][:7].clone()
    sim.reset_base_state(uid, lin_vel=dev(lin), ang_vel=dev(ang))
    assert same_bits(sim.state[cols, :B][:7], pose_before)
    figures += [err(stored(), want), err(report()[:, 7:13], np.concatenate([lin, ang], axis=1))]
    # one velocity alone: the other keeps its reported value
    sim.reset_base_state(uid, ang_vel=dev(-ang))
    assert same_bits(sim.state[cols, :B][:7], pose_before)
    figures += [err(report()[:, 7:13], np.concatenate([lin, -ang], axis=1))]
    sim.reset_base_state(uid, lin_vel=dev(2 * lin))
    figures += [err(report()[:, 7:13], np.concatenate([2 * lin, -ang], axis=1))]
    print('base_state figures %s x%d: %s (max %.3g)' % (scene, B, ' '.join('%.3g' % f for f in figures), max(figures)))
    assert max(figures) <= BOUND, figures
    env.reset()


# ------------------------------------------------------------------------------------------------------------ 4. the step sees it
@pytest.mark.parametrize('B', [3, 70])
def test_a_world_written_by_hand_runs_to_the_same_bits(B):
    a, b = make('contacts_marbles.yaml', B, tag='twin_a'), make('contacts_marbles.yaml', B, tag='twin_b')   # (no other test resets these: same episode count)
    assert a is not b and a.sim.lanes == b.sim.lanes and a.sim.kernel_name == b.sim.kernel_name
    L, uid = a.layout, a.models['blue_marble'].uid
    for env in (a, b):
        env.reset()
        run(env, 3, seed=2)
    assert same_bits(live(a.sim), live(b.sim))
    rng = np.random.default_rng(B)
    pos = np.array([0.0, 1.0, 0.0], dtype=np.float32) + np.stack([np.zeros(B), np.zeros(B), rng.uniform(0.6, 1.5, B)], axis=1).astype(np.float32)
    orn = np.tile(np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32), (B, 1))
    lin, ang = rng.uniform(-1.0, 1.0, (B, 3)).astype(np.float32), rng.uniform(-2.0, 2.0, (B, 3)).astype(np.float32)
    a.sim.reset_base_state(uid, pos=dev(pos), orn=dev(orn), lin_vel=dev(lin), ang_vel=dev(ang))
    # the marble's inertial frame is its link frame and the orientation is the identity: the stored values are the inputs, exactly
    assert not R.report_offset(L, uid)[0].any()
    want = np.concatenate(R.stored_from_report(L, uid, pos, orn, lin, ang), axis=1).astype(np.float32)
    assert np.array_equal(want, np.concatenate([pos, orn, lin, ang], axis=1))
    st = b.sim.get_state()
    st[:, R.base_columns(L, uid)] = want
    assert L.warm_off >= 0
    st[:, L.warm_off] = 0.0
    b.sim.set_state(st)
    assert torch.equal(live(a.sim), live(b.sim))
    for env in (a, b):
        run(env, 5, seed=7)
    assert same_bits(live(a.sim), live(b.sim))
    height = a.sim.frame_state(uid, -1)[:, 2].cpu().numpy()
    assert np.all(np.abs(height - pos[:, 2]) < 0.2) and np.all(height > 0.55)   # (where it was put, not where it lay)


def test_a_respawn_written_in_python():
    from user_respawn import PyRespawn
    B, rng_ = 70, [0.4, 0.4, 0.2]

    def edit(tree):
        tree['hot_start'] = 0   # (the state after the reset is what the hooks and the reset ops wrote)
        tree['green_marble']['respawn'] = {'addon': 'py_respawn', 'position_range': rng_, 'rotation_range': [0.0, 0.0, 1.0], 'seed': 3}
    env = make('contacts_marbles.yaml', B, edit=edit, tag='py_respawn', registry={'py_respawn': PyRespawn})
    assert len(env._hook_addons) == 1
    sim, model = env.sim, env.models['green_marble']
    env.reset()
    run(env, 3, seed=4)
    before = live(sim)
    m = (torch.arange(B) % 3 == 0).to(DEV)
    env.reset(m)
    after = live(sim)
    assert same_bits(after[:, ~m], before[:, ~m])
    st = sim.frame_state(model.uid, -1, com=True)[m]
    off = (st[:, 0:3].cpu() - torch.tensor(model.position, dtype=torch.float32)).abs()
    assert bool((off <= torch.tensor(rng_) / 2).all())
    assert float(off[:, 0].max()) > 0.05 and float(off[:, 0].min()) < 0.15   # (a spread, not one pose)
    assert float(st[:, 7:13].abs().max()) == 0.0 and float(st[:, 3:5].abs().max()) < 1e-6 and float(st[:, 5].abs().max()) > 0.01   # at rest, turned about z


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals():
    ur, mb, wd = make('ur_ik.yaml', 3), make('contacts_marbles.yaml', 3), make('np_gem_wedge_respawned.yaml', 3)
    p, q, v = torch.zeros(3, device=DEV), torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV), torch.ones(3, device=DEV)
    marble = mb.models['green_marble'].uid
    cases = [
        (ur, 'respawn', lambda s: s.reset_base_state(ur.models['arm'].uid, pos=p, orn=q)),                  # anchored
        (mb, 'respawn', lambda s: s.reset_base_state(mb.models['plane'].uid, pos=p, orn=q)),                # frozen
        (wd, 'no velocity', lambda s: s.reset_base_state(wd.models['wedge'].uid, pos=p, orn=q, lin_vel=v)),  # a velocity on a fixed base
        (wd, 'no velocity', lambda s: s.reset_base_state(wd.models['wedge'].uid, ang_vel=v)),
        (mb, 'both or neither', lambda s: s.reset_base_state(marble, pos=p)),
        (mb, 'both or neither', lambda s: s.reset_base_state(marble, orn=q)),
        (mb, 'nothing to write', lambda s: s.reset_base_state(marble)),
        (mb, 'out of range', lambda s: s.reset_base_state(99, pos=p, orn=q)),
        (mb, 'one element per env', lambda s: s.reset_base_state(marble, pos=p, orn=q, mask=torch.ones(4, dtype=torch.bool, device=DEV))),
        (mb, '3 or 3 x 3', lambda s: s.reset_base_state(marble, pos=torch.zeros((2, 3), device=DEV), orn=q)),
        (ur, '1 .. 32', lambda s: s.link_states(ur.models['arm'].uid, [0] * 33)),
        (ur, 'no frame', lambda s: s.link_states(ur.models['arm'].uid, [0, n_frames(ur.models['arm'])])),
        (ur, 'frame id', lambda s: s.link_states(ur.models['arm'].uid, [-2])),
        (mb, 'not a model', lambda s: s.link_states(99, [-1])),
        (mb, '2 bodies for 1 frames', lambda s: s.link_states([marble, marble], [-1])),
    ]
    for env, text, call in cases:
        before = live(env.sim)
        with pytest.raises(ValueError, match=text):
            call(env.sim)
        assert same_bits(live(env.sim), before), text


def test_the_c_entries_refuse_the_same():
    """The Python layer raises before it calls; the entries themselves answer DG_ERR_ARG, name themselves and launch nothing."""
    ur, mb, wd = make('ur_ik.yaml', 3), make('contacts_marbles.yaml', 3), make('np_gem_wedge_respawned.yaml', 3)
    buf = torch.full((3, 33, 13), 7.0, device=DEV)
    vec, quat = torch.zeros((3, 3), device=DEV), torch.tensor([[0.0, 0.0, 0.0, 1.0]] * 3, device=DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    i32s = lambda v: (ctypes.c_int32 * len(v))(*v)

    def base(env, body, pos=None, orn=None, lin=None, ang=None):
        s = env.sim
        return s.lib.dg_world_reset_base_state(s.handle, ptr(s.state), body, pos, orn, lin, ang, None, s._stream())

    def links(env, bodies, frames, n=None, out=buf):
        s = env.sim
        return s.lib.dg_world_link_states(s.handle, ptr(s.state), i32s(bodies), i32s(frames), len(frames) if n is None else n, 0, out if out is None else ptr(out), s._stream())
    arm, nf = ur.models['arm'].uid, n_frames(ur.models['arm'])
    cases = [
        (ur, b'respawn', lambda: base(ur, arm, ptr(vec), ptr(quat))),
        (mb, b'respawn', lambda: base(mb, mb.models['plane'].uid, ptr(vec), ptr(quat))),
        (wd, b'no velocity', lambda: base(wd, wd.models['wedge'].uid, ptr(vec), ptr(quat), ptr(vec))),
        (mb, b'both or neither', lambda: base(mb, mb.models['green_marble'].uid, ptr(vec))),
        (mb, b'nothing to write', lambda: base(mb, mb.models['green_marble'].uid)),
        (mb, b'out of range', lambda: base(mb, 99, ptr(vec), ptr(quat))),
        (ur, b'1 .. 32', lambda: links(ur, [arm] * 33, [0] * 33)),
        (ur, b'1 .. 32', lambda: links(ur, [arm], [0], n=0)),
        (ur, b'no frame', lambda: links(ur, [arm, arm], [0, nf])),
        (ur, b'out of range', lambda: links(ur, [arm, 99], [0, 0])),
        (ur, b'NULL', lambda: links(ur, [arm], [0], out=None)),
    ]
    for env, text, call in cases:
        before = live(env.sim)
        assert call() == -4, text
        msg = env.sim.lib.dg_last_error()
        assert text in msg and (b'dg_world_reset_base_state' in msg or b'dg_world_link_states' in msg), msg
        assert same_bits(live(env.sim), before)
    assert float(buf.min()) == 7.0 and float(buf.max()) == 7.0   # outputs untouched


# ------------------------------------------------------------------------------------------------------------ 6. the addon
def test_link_state_sensor_reports_link_states():
    env = make(os.path.join('link_state_sensor', 'arm_keypoints.yaml'), 3)
    arm = env.models['arm']
    ids = [arm.get_frame_id('elbow_joint'), -1, arm.get_frame_id('wrist_3_joint')]
    env.reset()
    gen = torch.Generator().manual_seed(1)
    for _ in range(5):
        obs = env.step({'arm': {'controller': ((torch.rand((3, 6), generator=gen) - 0.5) * 0.4).to(DEV)}})[0]
    o = obs['arm']['keypoints']
    want = env.sim.link_states(arm.uid, ids).clone()
    assert same_bits(o['position'], want[:, :, 0:3].reshape(3, 9)) and same_bits(o['orientation'], want[:, :, 3:7].reshape(3, 12))
    assert same_bits(o['velocity'], want[:, :, 7:10].reshape(3, 9)) and same_bits(o['angular_velocity'], want[:, :, 10:13].reshape(3, 9))
    assert float(o['velocity'].abs().max()) > 0.0
    root = env.sim.link_states(arm.uid).clone()
    assert tuple(root.shape) == (3, 1, 13)
    assert same_bits(obs['arm']['root']['position'], root[:, 0, 0:3]) and same_bits(obs['arm']['root']['orientation'], root[:, 0, 3:7])
