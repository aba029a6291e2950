"""Contact forces in full on the GPU: ``dg_world_contact_forces`` / ``env.sim.contact_forces``, ``dg_world_net_contact_wrench`` /
``env.sim.net_contact_forces`` and the ``contact_force_sensor`` addon.

The readout is compared with an independent fp64 restatement of the GPU's own numbers (tests/contact_force_ref.py: the impulse
cache read from the state, the geometry from ``contact_points``): what the kernel copies must match to the bit, what it computes
differs by fp32 rounding of a handful of operations.  Every bound is 8 x the largest error measured on an MI355X over exactly these
scenes and batches (MEASURED; DESIGN.md "Contact forces").  The momentum balance of a pushed marble is independent of the checker."""
import os
import sys

import numpy as np
import pytest

import contact_force_ref as ref
from test_contact_force_ref import PUSHED, SETTLE, marble, push_actions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)   # make_vectors: the pressed-together inputs of the arms
pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 70)   # one lane; a wavefront with a partial tail; more than one wavefront
# largest error per quantity over test_readout_is_the_restatement's nine cases: unit tangents (absolute), force_on_a and net force
# relative to the env's largest contact force, net moment relative to the env's largest force x arm; and the residual of the pushed
# marble's momentum balance relative to m g, and the lateral force of a marble at rest relative to m g
# (MI355X: direction 1.237e-07, force 6.034e-08 and net moment 1.091e-07 on the arms at 70 envs, net force 8.038e-08 on the box stack;
# momentum residual 1.588e-07 at 1 env, 1.855e-07 at 3, 3.277e-07 at 70; a marble at rest reports no lateral force at all)
MEASURED = dict(direction=1.237e-07, force=6.034e-08, net_force=8.038e-08, net_torque=1.091e-07, momentum=3.277e-07, rest_lateral=0.0)
BOUND = {k: 8.0 * v for k, v in MEASURED.items()}
MG = 98.1


def _path(name):
    for p in (os.path.join(GOLDEN, name + '.yaml'), os.path.join(GOLDEN, 'contact_force_sensor', name + '.yaml'), os.path.join(ROOT, 'examples', name, name + '.yaml')):
        if os.path.isfile(p):
            return p
    raise KeyError(name)


def gpu_env(name, B, **kw):
    from diy_gym_amd import DIYGym
    return DIYGym(_path(name), num_envs=B, seed=5, device='cuda:0', **kw)


def run(env, name, steps):
    import torch
    if 'arms' in name:
        import make_vectors
        acts = make_vectors.press_actions(env, steps)
    else:
        acts = torch.zeros((steps, env.num_envs, max(env.layout.act_dim, 1)))
    for s in range(steps):
        env.sim.step(env._all_slots, acts[s].to(env.device))
    return env


def host(t):
    return type(t)(*[None if x is None else x.cpu().numpy().copy() for x in t])


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def link_part(ids):
    return (ids >> 24) - 1


# ------------------------------------------------------------------------------------------ 1. the readout against its restatement
SCENES = {'contacts_marbles': 300, 'contacts_box_stack': 120, 'contacts_arms': 45}


def check_rows(got, want, worst):
    """One env's rows of contact_forces against the reference rows: scalars to the bit, vectors measured."""
    n = len(want); fmax = max([abs(c.normal_force) for c in want] + [1e-30])
    for k, c in enumerate(want):
        assert (got.id_a[k], got.id_b[k]) == (c.id_a, c.id_b)
        for name in ('normal_force', 'lateral_friction1', 'lateral_friction2'):
            assert bits(getattr(got, name)[k]) == bits(np.float32(getattr(c, name))), (name, k)
        assert np.array_equal(bits(got.normal[k]), bits(c.normal.astype(np.float32)))
        worst['direction'] = max(worst['direction'], np.abs(got.lateral_dir1[k] - c.lateral_dir1).max(), np.abs(got.lateral_dir2[k] - c.lateral_dir2).max())
        worst['force'] = max(worst['force'], np.abs(got.force_on_a[k] - c.force_on_a).max() / fmax)
        # the identity the interface promises, from the reported numbers themselves
        g = got.normal_force[k].astype(np.float64) * got.normal[k] + got.lateral_friction1[k].astype(np.float64) * got.lateral_dir1[k] \
            + got.lateral_friction2[k].astype(np.float64) * got.lateral_dir2[k]
        worst['force'] = max(worst['force'], np.abs(got.force_on_a[k] - g).max() / fmax)
        # the friction clamp: each tangent on its own within mu x normal force, one fp32 rounding of the product of slack
        lim = np.float32(c.mu) * np.float32(c.normal_force) * (1.0 + 2.0 ** -23)
        assert abs(got.lateral_friction1[k]) <= lim and abs(got.lateral_friction2[k]) <= lim, (k, c.mu, c.normal_force)
    return n


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('name', sorted(SCENES))
def test_readout_is_the_restatement(name, B):
    """Marbles on the plane (|n.z| > 0.707 and, between two marbles, a horizontal normal: both branches of tangent_basis), a box
    on a box on the ground, two UR5 pressed together (oblique normals): rows, ids and counts are contact_points'; normal force and
    both friction forces are the cache's numbers over the substep, to the bit; tangents, force_on_a and the per-link net wrenches
    follow the fp64 restatement; every tangent force is within the friction cone's box."""
    env = run(gpu_env(name, B), name, SCENES[name]); sim = env.sim
    S = sim.get_state()
    cp = host(sim.contact_points()); cf = host(sim.contact_forces())
    assert cf.count.tolist() == cp.count.tolist() and cp.count.min() > 0
    assert np.array_equal(cf.id_a, cp.id_a) and np.array_equal(cf.id_b, cp.id_b)
    assert np.array_equal(bits(cf.normal), bits(cp.normal)) and np.array_equal(bits(cf.normal_force), bits(cp.normal_force))
    want, found = ref.restate_from_query(cp, S, env.layout)
    worst = dict(direction=0.0, force=0.0, net_force=0.0, net_torque=0.0); nz = []
    for e in range(B):
        n = check_rows(type(cf)(*[None if x is None else x[e] for x in cf]), want[e], worst)
        dead = slice(n, None)
        assert (cf.id_a[e, dead] == -1).all() and not cf.force_on_a[e, dead].any() and not cf.lateral_dir1[e, dead].any() and not cf.lateral_friction2[e, dead].any()
        nz += [abs(c.normal[2]) for c in want[e]]
    if name == 'contacts_marbles':
        assert max(nz) > 0.99 and min(nz) < 0.01
    if name == 'contacts_arms':
        assert any(0.05 < z < 0.95 for z in nz)
    # filtered rows: every body as A, with the swap rule
    for m in env.models.values():
        rows = host(sim.contact_forces(m.uid))
        for e in range(B):
            w = ref.filtered(want[e], m.uid)
            assert rows.count[e] == len(w)
            check_rows(type(rows)(*[None if x is None else x[e] for x in rows]), w, worst)
    # net wrenches: the whole body, its base, and the links its contacts sit on
    for m in env.models.values():
        seen = sorted({int(l) for e in range(B) for c in ref.filtered(want[e], m.uid) for l in [link_part(c.id_a)] if l >= 0})[:3]
        links = [None, -1] + seen
        force, torque, count = (x.cpu().numpy().copy() for x in sim.net_contact_forces(m.uid, links))
        assert force.shape == (B, len(links), 3) and torque.shape == (B, len(links), 3) and count.shape == (B, len(links))
        for s, l in enumerate(links):
            org = sim.frame_state(m.uid, -1 if l is None else l, com=True)[:, :3].cpu().numpy().astype(np.float64)
            for e in range(B):
                F, T, k = ref.net_wrench(want[e], m.uid, l, org[e])
                rows = ref.filtered(want[e], m.uid, l)
                fmax = max([np.linalg.norm(c.force_on_a) for c in rows] + [1e-30]); tmax = max([np.linalg.norm(c.force_on_a) * np.linalg.norm(c.pos_a - org[e]) for c in rows] + [1e-30])
                assert count[e, s] == k
                worst['net_force'] = max(worst['net_force'], np.abs(force[e, s] - F).max() / fmax)
                worst['net_torque'] = max(worst['net_torque'], np.abs(torque[e, s] - T).max() / tmax)
    print('MEASURE readout %s B=%d direction %.3e force %.3e net_force %.3e net_torque %.3e' % (name, B, worst['direction'], worst['force'], worst['net_force'], worst['net_torque']))
    assert np.array_equal(bits(S), bits(sim.get_state()))   # the state is never written
    for k, v in worst.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


# ---------------------------------------------------------------------------------------------------- 2. the identity and the swap
def test_swapped_sides_report_exactly_opposite_forces():
    env = run(gpu_env('contacts_box_stack', 70), 'contacts_box_stack', 120); sim = env.sim
    m = env.models; plane, lower, upper = m['plane'].uid, m['lower'].uid, m['upper'].uid; C = env.layout.max_contacts
    for x, y in ((lower, upper), (plane, lower)):
        xy, yx = host(sim.contact_forces(x, y)), host(sim.contact_forces(y, x))
        assert xy.count.tolist() == yx.count.tolist() and xy.count.min() >= 1
        live = np.arange(C)[None, :] < xy.count[:, None]
        assert np.array_equal(xy.id_a, yx.id_b) and np.array_equal(xy.id_b, yx.id_a)
        for f in ('normal_force', 'lateral_friction1', 'lateral_friction2'):
            assert np.array_equal(bits(getattr(xy, f)), bits(getattr(yx, f))), f
        for f in ('normal', 'lateral_dir1', 'lateral_dir2', 'force_on_a'):
            assert np.array_equal(bits(getattr(xy, f))[live], bits(-getattr(yx, f))[live]), f
        assert np.abs(xy.lateral_friction1[live]).max() > 0   # (the stack carries friction: the swap is not tested on zeros)
    # one contact between the boxes: the net forces of the two sides are exact negatives
    a = sim.net_contact_forces(lower, None, upper)[0].cpu().numpy().copy(); b = sim.net_contact_forces(upper, None, lower)[0].cpu().numpy().copy()
    assert host(sim.contact_forces(lower, upper)).count.tolist() == [1] * 70
    assert np.array_equal(bits(a), bits(-b)) and np.abs(a).max() > 1.0


# -------------------------------------------------------------------------------------------------------- 3. the momentum balance
@pytest.mark.parametrize('B', BATCHES)
def test_momentum_balance_of_a_pushed_marble(B):
    """Independent of the checker: the blue marble rests on the plane and is pushed by its external_force addon with a constant
    horizontal force; over every one of 20 steps (one substep each) m (v1 - v0) / h is gravity + the push + the step's velocity damping
    + net_contact_forces(marble).force read after the step.  The contact set never changes and every contact is in the cache.  Before
    the push the marble reports (0, 0, float32(98.1)) in z to the bit."""
    import torch
    env = gpu_env('contacts_marbles', B); sim = env.sim; layout = env.layout
    b, m, vo = marble(env); h, g = float(layout.dt), ref.gravity(layout)
    zero = torch.zeros((B, layout.act_dim), device=env.device); act, applied = push_actions(env, B); act = act.to(env.device)
    for _ in range(SETTLE):
        sim.step(env._all_slots, zero)
    rest = sim.net_contact_forces(b)[0].cpu().numpy()[:, 0]
    assert np.array_equal(bits(rest[:, 2]), bits(np.full(B, 98.1, dtype=np.float32)))
    lateral = float(np.abs(rest[:, :2]).max()) / MG
    worst = 0.0; first = None
    for _ in range(PUSHED):
        v0 = sim.get_state()[:, vo:vo + 3].astype(np.float64)
        sim.step(env._all_slots, act)
        S = sim.get_state(); v1 = S[:, vo:vo + 3].astype(np.float64)
        force, _, count = sim.net_contact_forces(b)
        total = sim.contact_forces(want=('id', )).count.cpu().numpy()
        assert count[:, 0].tolist() == [1] * B and total.tolist() == S[:, layout.warm_off].astype(np.int64).tolist()
        first = total if first is None else first
        assert total.tolist() == first.tolist()
        fc = force.cpu().numpy()[:, 0].astype(np.float64)
        res = m * (v1 - v0) / h - (m * g + applied + ref.damping_force(layout, m, v0) + fc)
        worst = max(worst, float(np.abs(res).max()) / MG)
        assert (np.abs(fc[:, :2]).max(1) > 0.5).all()
    print('MEASURE momentum B=%d residual / m g %.3e, lateral at rest / m g %.3e' % (B, worst, lateral))
    assert worst <= BOUND['momentum'] and lateral <= BOUND['rest_lateral']


# ------------------------------------------------------------------------------------------------------- 4. every workspace mode
MODES = {
    ('contacts_arms', 70, 45): [({}, 64), ({'DG_MAX_LANES': '16'}, 16), ({'DG_MAX_LANES': '8'}, 0), ({'DG_NO_SLICED_GLOBAL': '1'}, 64)],
    ('contacts_marbles', 3, 60): [({}, 32), ({'DG_MAX_LANES': '16'}, 16), ({'DG_MAX_LANES': '8'}, 8), ({'DG_MAX_LANES': '4'}, 4), ({'DG_MAX_LANES': '1'}, 1)],
    ('from_the_readme', 3, 30): [({}, 1), ({'DG_NO_WAVE_ENV': '1'}, 4), ({'DG_NO_NARROW_MODES': '1'}, -16), ({'DG_NO_NARROW_MODES': '1', 'DG_NO_SLICED_GLOBAL': '1'}, 0)],
}


def both_calls(env):
    out = [x for x in host(env.sim.contact_forces())]
    for m in env.models.values():
        nfr = env.sim._body_n_frames(m.uid)
        out += [x.cpu().numpy().copy() for x in env.sim.net_contact_forces(m.uid, [None, -1] + list(range(min(nfr, 14))))]
    return out


@pytest.mark.parametrize('name,B,steps', sorted(MODES))
def test_every_workspace_mode_gives_the_same_bits(monkeypatch, name, B, steps):
    """Both calls are the same code on another workspace: one state, set into worlds of every mode the scene can run in, gives
    bit-identical answers (pressed arms at 70 envs: helper-wave world, 16 envs per wavefront, global workspace; marbles at 3 envs:
    every LDS mode; from_the_readme at 3 envs: one env per wavefront, four, and both global modes)."""
    import diy_gym_amd.examples  # noqa: F401
    switches = [v for sw, _ in MODES[(name, B, steps)] for v in sw]
    for v in switches:
        monkeypatch.delenv(v, raising=False)
    ref_env = run(gpu_env(name, B), name, steps)
    S = ref_env.sim.get_state(); want = both_calls(ref_env)
    assert want[0].min() > 0 and np.abs(want[4]).max() > 0
    for sw, lanes in MODES[(name, B, steps)]:
        for v in switches:
            monkeypatch.delenv(v, raising=False)
        for k, v in sw.items():
            monkeypatch.setenv(k, v)
        env = gpu_env(name, B)
        assert env.sim.lanes == lanes, (sw, env.sim.lanes)
        env.sim.set_state(S)
        for i, (a, c) in enumerate(zip(want, both_calls(env))):
            assert np.array_equal(bits(a), bits(c)), (sw, i)
        env.close()


# -------------------------------------------------------------------------------------------------- 5. filters, links, merged child
def test_links_of_a_body_with_a_merged_child():
    import torch
    gpu = gpu_env('contacts_child_gripper', 3); sim = gpu.sim
    arm = gpu.models['arm']; plane = gpu.models['plane'].uid
    act = torch.tensor([[0.3, -0.55, 1.22, -1.51, 0.84, 0.1]] * 3, device=gpu.device)   # (presses a finger onto the plane)
    for _ in range(120):
        sim.step(gpu._all_slots, act)
    every = host(sim.contact_forces(arm.uid)); C = gpu.layout.max_contacts
    live = np.arange(C)[None, :] < every.count[:, None]
    finger = int(max(link_part(every.id_a)[live]))   # a link of the gripper that touches the plane (the index its shapes carry)
    assert finger >= 0 and every.count.min() >= 5
    links = [None, -1, finger]
    force, torque, count = (x.cpu().numpy().copy() for x in sim.net_contact_forces(arm.uid, links))
    for s, l in enumerate(links):
        rows = host(sim.contact_forces(arm.uid, None, l)); cp = sim.contact_points(arm.uid, None, l, want=('id', ))
        assert count[:, s].tolist() == rows.count.tolist() == cp.count.cpu().numpy().tolist()
        assert rows.count.min() >= 1 or l == -1   # (the whole body and the finger touch in every env)
        fsum = rows.force_on_a.astype(np.float64).sum(1); fmax = np.linalg.norm(rows.force_on_a, axis=-1).max(1)
        assert (np.abs(force[:, s] - fsum).max(1) <= BOUND['net_force'] * fmax).all()   # the row is the sum of the per-contact forces
    assert np.abs(force[:, 0]).max() > 50.0 and np.abs(torque).max() > 0.0
    only_plane = sim.net_contact_forces(arm.uid, links, plane)[0].cpu().numpy()
    assert np.array_equal(bits(only_plane), bits(force))   # (the arm touches nothing else)
    nfr = sim._body_n_frames(arm.uid)
    for bad in ([nfr], [999], [-2], [0] * 17, []):
        with pytest.raises(ValueError):
            sim.net_contact_forces(arm.uid, bad)


def test_world_without_impulse_cache_refuses_both_calls():
    gpu = run(gpu_env('contacts_marbles', 3, engine={'warmstart': 0, 'warmstart_friction': 0}), 'contacts_marbles', 20)
    assert gpu.layout.warm_off < 0
    with pytest.raises(RuntimeError, match='impulse cache'):
        gpu.sim.contact_forces()
    with pytest.raises(RuntimeError, match='impulse cache'):
        gpu.sim.net_contact_forces(gpu.models['green_marble'].uid)


# ------------------------------------------------------------------------------------------------------------------- 6. the addon
def test_contact_force_sensor_reports_the_net_force_and_leaves_the_state_alone():
    import torch
    env = gpu_env('marbles', 3); plain = gpu_env('marbles', 3)   # (the second one is stepped without ever evaluating its sensors)
    for _ in range(300):
        obs, _, _, _ = env.step({})
        plain.sim.step(plain._all_slots)
    g = obs['green_marble']; green, plane = env.models['green_marble'].uid, env.models['plane'].uid
    assert tuple(g['ground_reaction']['force'].shape) == (3, 3)
    assert torch.equal(g['ground_reaction']['force'], env.sim.net_contact_forces(green, None, plane)[0][:, 0])
    assert torch.equal(g['all_contacts']['force'], env.sim.net_contact_forces(green)[0][:, 0])
    assert np.array_equal(bits(g['ground_reaction']['force'][:, 2].cpu().numpy()), bits(np.full(3, 98.1, dtype=np.float32)))
    # a rollout with the sensors evaluated every step leaves the state bit-identical to one that never launched the query
    assert np.array_equal(bits(env.sim.get_state()), bits(plain.sim.get_state()))
