"""The batched closest-points query on the GPU: ``dg_world_closest`` / ``env.sim.closest_points`` and the ``proximity_sensor`` addon.

Every case (tests/closest_cases.py) is a scene from tests/golden brought to a state by a few seeded steps of the fp64 checker; the
state is set into a GPU world and the query's answer compared, env by env and pair by pair, with the fp64 reference
(tests/closest_ref.py), which tests/test_closest_ref.py pins on the CPU.  No (env, pair) is left out of a comparison: the cases
keep every pair at least CLEAR away from the query's distance, so counts and ids are equal outright.

Every bound is 8 x the largest error measured on an MI355X over exactly these cases and batches (the project's convention for fp32
against fp64; the 8 absorbs state-to-state variation in the conditioning of fp32 GJK); the measured values are in MEASURED and in
DESIGN.md "Closest-points query"."""
import ctypes

import numpy as np
import pytest

import closest_cases as cc

pytestmark = pytest.mark.gpu

# largest |query - reference| per pair type over test_geometry_follows_the_reference, test_capsule_world_uses_the_fitted_capsules and
# test_pruned_pairs_are_reported (MI355X, batches 1 / 3 / 70): signed distance (m), normal (largest component), each witness off
# its own shape (m), and pos_a - pos_b against normal x distance (m)
MEASURED = {
    'round-round': dict(distance=2.035e-07, normal=7.223e-07, witness=1.958e-07, gap=1.150e-07),   # marbles; the arms' fitted capsules
    'round-box': dict(distance=7.405e-08, normal=0.0, witness=1.410e-08, gap=7.823e-08),          # marbles, r2d2's wheels (the ground's normal is exact)
    'hull-box': dict(distance=1.019e-07, normal=5.960e-08, witness=1.144e-08, gap=9.604e-08),      # box on the ground, r2d2's boxes
    'hull-hull': dict(distance=3.073e-07, normal=4.256e-04, witness=2.467e-07, gap=1.420e-07),     # box on box, two UR5 (the normal: fp32 GJK / EPA of pairs 1e-4 m apart)
}
BOUND = {kind: {k: 8.0 * v for k, v in cols.items()} for kind, cols in MEASURED.items()}


def clone(cp):
    return type(cp)(*[None if t is None else t.clone() for t in cp])


def host(cp):
    return type(cp)(*[None if t is None else t.cpu().numpy() for t in cp])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(x, y):
    for f, a, b in zip(x._fields, x, y):
        assert (a is None) == (b is None) and (a is None or np.array_equal(bits(a), bits(b))), f


def world(name, B):
    """A GPU world of the case's scene at the checker's state, and the case's reference."""
    case, r = cc.CASES[name], cc.reference(name, B)
    gpu = cc.gpu_env(case.scene, B, case.engine)
    gpu.sim.set_state(r.state)
    return gpu, r


def compare(got, r, measured, distance, worst):
    """Counts and ids equal in every env; per row the four error columns, accumulated per pair type into ``worst``."""
    rows = cc.rows_of(measured, distance); near = cc.nearest_of(rows)
    K = got.id_a.shape[1]
    assert got.count.tolist() == [len(x) for x in rows]
    assert max(len(x) for x in rows) <= K
    for e, env in enumerate(rows):
        assert got.id_a[e, :len(env)].tolist() == [p.id_a for p in env] and got.id_b[e, :len(env)].tolist() == [p.id_b for p in env]
        assert (got.id_a[e, len(env):] == -1).all() and (got.id_b[e, len(env):] == -1).all()
        assert not got.distance[e, len(env):].any() and not got.pos_a[e, len(env):].any() and not got.normal[e, len(env):].any()
        for k, p in enumerate(env):
            pa, pb, n, d = (got.pos_a[e, k].astype(np.float64), got.pos_b[e, k].astype(np.float64), got.normal[e, k].astype(np.float64),
                            float(got.distance[e, k]))
            w = worst.setdefault(p.kind, dict(distance=0.0, normal=0.0, witness=0.0, gap=0.0))
            w['distance'] = max(w['distance'], abs(d - p.distance))
            w['normal'] = max(w['normal'], float(np.abs(n - p.normal).max()))
            w['witness'] = max(w['witness'], r.ref.off_shape(p.sa, p.sb, r.poses, e, pa), r.ref.off_shape(p.sb, p.sa, r.poses, e, pb))
            w['gap'] = max(w['gap'], float(np.abs((pa - pb) - n * d).max()))
        # the nearest pair: the reference's where it leads the runner-up by more than CLEAR, and always one of the rows' minimum
        ds = sorted(p.distance for p in env)
        if len(ds) == 1 or ds[1] - ds[0] > cc.CLEAR:
            assert (int(got.nearest_id_a[e]), int(got.nearest_id_b[e])) == (near[e].id_a, near[e].id_b)
        k = int(np.argmin(got.distance[e, :len(env)]))   # (first minimum: ties go to the first pair)
        assert bits(got.nearest_distance[e:e + 1])[0] == bits(got.distance[e, k:k + 1])[0]
        assert (int(got.nearest_id_a[e]), int(got.nearest_id_b[e])) == (int(got.id_a[e, k]), int(got.id_b[e, k]))
        assert np.array_equal(bits(got.nearest_pos_a[e]), bits(got.pos_a[e, k])) and np.array_equal(bits(got.nearest_normal[e]), bits(got.normal[e, k]))


def held(worst, label):
    for kind, cols in sorted(worst.items()):
        print('MEASURE closest %s %s distance %.3e normal %.3e witness %.3e gap %.3e' % (label, kind, cols['distance'], cols['normal'], cols['witness'], cols['gap']))
    for kind, cols in worst.items():
        for k, v in cols.items():
            assert v <= BOUND[kind][k], (kind, k, v, BOUND[kind][k])


# ---------------------------------------------------------------------------------------------------------------- 1. geometry
@pytest.mark.parametrize('B', cc.BATCHES)
@pytest.mark.parametrize('name', cc.GEOMETRY)
def test_geometry_follows_the_reference(name, B):
    """Marbles (sphere on sphere, sphere on box), a box on a box on the ground (hull on box through its points, hull on hull), r2d2
    over the plane (capsules and hulls on a box) and two UR5 with crossed forearms (hull on hull, statically pruned pairs among
    them): every query of the case keeps some pairs in and some out; counts and ids are the reference's in every env; distance,
    normal, witnesses on their shapes and pos_a - pos_b = normal x distance are held pair by pair."""
    gpu, r = world(name, B); worst = {}
    for ua, ub, dist, measured in r.answers:
        got = host(gpu.sim.closest_points(ua, ub, dist))
        compare(got, r, measured, dist, worst)
    held(worst, '%s B=%d' % (name, B))


@pytest.mark.parametrize('B', (3, 70))
def test_capsule_world_uses_the_fitted_capsules(B):
    """The arms in a hull_contacts = 0 world: hull against hull is the step's capsule model there, and so is the query's."""
    gpu, r = world('arms_capsules', B); worst = {}
    assert not r.ref.hull_mode
    for ua, ub, dist, measured in r.answers:
        compare(host(gpu.sim.closest_points(ua, ub, dist)), r, measured, dist, worst)
    assert set(worst) == {'round-round'}
    held(worst, 'arms_capsules B=%d' % B)


@pytest.mark.parametrize('name,B', (('two_arms', 3), ('arms', 70)))
def test_pruned_pairs_are_reported(name, B):
    """Pairs the scene's static pruning removed from the step's pair table (``layout.pruned_pairs``: two arm bases bolted too far
    apart to ever touch) are candidates of the query and come back with the reference's distance."""
    gpu, r = world(name, B); worst = {}; pruned = set(map(tuple, r.layout.pruned_pairs)); seen = 0
    assert pruned
    ua, ub, dist, measured = r.answers[-1]
    got = host(gpu.sim.closest_points(ua, ub, dist))
    compare(got, r, measured, dist, worst)
    for e, env in enumerate(cc.rows_of(measured, dist)):
        for k, p in enumerate(env):
            if (min(p.sa, p.sb), max(p.sa, p.sb)) in pruned:
                seen += 1
                assert abs(float(got.distance[e, k]) - p.distance) <= BOUND[p.kind]['distance']
    assert seen >= B
    held(worst, 'pruned %s B=%d' % (name, B))


# ------------------------------------------------------------------------------------------------------------------- 2. culls
@pytest.mark.parametrize('name', sorted(cc.CASES))
def test_no_cull_drops_a_pair(name):
    """Every candidate pair through its primitive (the debug switch) gives the same bits as the culled query: each cull is a lower
    bound of the distance it stands in front of."""
    gpu, r = world(name, 70)
    lib, h = gpu.sim.lib, gpu.sim.handle
    lib.dg_debug_closest_no_cull.restype = ctypes.c_int32
    lib.dg_debug_closest_no_cull.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    for ua, ub, dist, _ in r.answers:
        for d in (dist, 0.0, 0.01):
            culled = host(clone(gpu.sim.closest_points(ua, ub, d)))
            assert lib.dg_debug_closest_no_cull(h, 1) == 0
            brute = host(clone(gpu.sim.closest_points(ua, ub, d)))
            assert lib.dg_debug_closest_no_cull(h, 0) == 0
            same_bits(culled, brute)


# ------------------------------------------------------------------------------------------- 3. agreement with the contact query
@pytest.mark.parametrize('name', ('marbles', 'box_stack', 'arms'))
def test_agrees_with_the_contact_query(name):
    """At one state: every row of contact_points has a closest_points row with the same ids whose distance is the contact's within
    the bound of the pair's type -- or at most the contact's where the step lists several contacts per pair (a hull's corners on a
    box; the query reports the nearest one); and with distance = 0 only penetrating pairs come back."""
    gpu, r = world(name, 3)
    margin = 0.02   # (beyond every scene's contact margin)
    seen = 0
    for ua in sorted(set(r.uids.values())):
        if not r.ref.candidates(ua):
            continue
        ct = host(clone(gpu.sim.contact_points(ua, want=('id', 'distance'))))
        cl = host(clone(gpu.sim.closest_points(ua, None, margin, want=('id', 'distance'))))
        for e in range(3):
            rows = {(int(a), int(b)): float(d) for a, b, d in zip(cl.id_a[e, :cl.count[e]], cl.id_b[e, :cl.count[e]], cl.distance[e, :cl.count[e]])}
            per_pair = {}
            for k in range(ct.count[e]):
                per_pair.setdefault((int(ct.id_a[e, k]), int(ct.id_b[e, k])), []).append(float(ct.distance[e, k]))
            for ids, ds in per_pair.items():
                assert ids in rows, (ids, sorted(rows))
                loosest = max(v['distance'] for v in BOUND.values())
                assert abs(rows[ids] - min(ds)) <= loosest, (ids, rows[ids], ds)
                assert all(rows[ids] <= d + loosest for d in ds)
                seen += 1
        zero = host(clone(gpu.sim.closest_points(ua, None, 0.0, want=('id', 'distance'))))
        for e in range(3):
            assert (zero.distance[e, :zero.count[e]] < 0).all()
            assert zero.count[e] == int((cl.distance[e, :cl.count[e]] < 0).sum())
    assert seen > 0


# --------------------------------------------------------------------------------------------- 4. filters, shape of the answer
def test_swapped_sides_are_the_same_bits_mirrored():
    gpu, r = world('box_stack', 3)
    lower, upper, plane = r.uids['lower'], r.uids['upper'], r.uids['plane']
    for x, y in ((lower, upper), (lower, plane), (upper, plane)):
        a, b = host(clone(gpu.sim.closest_points(x, y, 0.3))), host(clone(gpu.sim.closest_points(y, x, 0.3)))
        assert a.count.tolist() == b.count.tolist() == [1] * 3
        assert np.array_equal(a.id_a, b.id_b) and np.array_equal(a.id_b, b.id_a)
        assert np.array_equal(bits(a.pos_a), bits(b.pos_b)) and np.array_equal(bits(a.pos_b), bits(b.pos_a))
        assert np.array_equal(bits(a.distance), bits(b.distance)) and np.array_equal(bits(a.normal), bits(-b.normal))
        assert (a.id_a[:, 0] & 0xFFFFFF).tolist() == [x] * 3   # the body given as A is side A


def test_link_filters_select_rows():
    gpu, r = world('r2d2', 3)
    robot, plane = r.uids['r2d2'], r.uids['plane']
    every = host(clone(gpu.sim.closest_points(robot, plane, 0.3)))
    links = sorted(set(((every.id_a[0, :every.count[0]] >> 24) - 1).tolist()))
    assert len(links) >= 3
    for lk in links:
        got = host(clone(gpu.sim.closest_points(robot, plane, 0.3, link_a=lk)))
        for e in range(3):
            sel = ((every.id_a[e, :every.count[e]] >> 24) - 1) == lk
            assert got.count[e] == sel.sum()
            assert np.array_equal(bits(got.distance[e, :got.count[e]]), bits(every.distance[e, :every.count[e]][sel]))
        rev = host(clone(gpu.sim.closest_points(plane, robot, 0.3, link_b=lk)))
        assert rev.count.tolist() == got.count.tolist() and np.array_equal(rev.id_b[:, :1], got.id_a[:, :1])
    with pytest.raises(ValueError):
        gpu.sim.closest_points(robot, plane, 0.3, link_a=999)
    with pytest.raises(ValueError):
        gpu.sim.closest_points(robot, None, 0.3, link_b=0)
    with pytest.raises(ValueError):
        gpu.sim.closest_points(None)
    with pytest.raises(ValueError):
        gpu.sim.closest_points(robot, distance=float('nan'))
    with pytest.raises(ValueError):
        gpu.sim.closest_points(robot, distance=-0.1)
    with pytest.raises(ValueError):
        gpu.sim.closest_points(robot, max_points=-1)


def test_alias_of_a_merged_child():
    """A gripper merged into the arm's body: the alias uid selects the whole merged body, with a link the shapes that carry that
    link index in the child's own URDF -- the rows of the unfiltered answer with that link, bit for bit."""
    gpu = cc.gpu_env('contacts_child_gripper', 3)
    arm = gpu.models['arm']; alias = arm.models['gripper'].uid; plane = gpu.models['plane'].uid
    assert alias in gpu.layout.aliases and gpu.layout.aliases[alias][0] == arm.uid
    every = host(clone(gpu.sim.closest_points(arm.uid, plane, 1.0)))
    whole = host(clone(gpu.sim.closest_points(alias, plane, 1.0)))
    same_bits(every, whole)
    assert every.count.min() >= 10
    links = ((every.id_a[0, :every.count[0]] >> 24) - 1)
    for lk in sorted(set(links.tolist())):
        got = host(clone(gpu.sim.closest_points(alias, plane, 1.0, link_a=lk)))
        for e in range(3):
            sel = ((every.id_a[e, :every.count[e]] >> 24) - 1) == lk
            assert got.count[e] == sel.sum() and np.array_equal(bits(got.distance[e, :got.count[e]]), bits(every.distance[e, :every.count[e]][sel]))


def test_truncation_k_zero_sentinel_and_reuse():
    gpu, r = world('r2d2', 70)
    robot = r.uids['r2d2']
    full = host(clone(gpu.sim.closest_points(robot, None, 0.3)))
    assert full.count.min() >= 6 and full.id_a.shape[1] == len(r.ref.candidates(robot))
    # truncated: the first K rows, count still the number found, nearest the global one (it is beyond the first K rows here)
    K = 3
    first = full.distance[:, :K].min(1); assert (full.nearest_distance < first).all()
    gpu.sim.closest_points(robot, None, 0.3, max_points=K)
    key = [k for k in gpu.sim._closest_out if k[3] == K]; assert len(key) == 1
    for t in gpu.sim._closest_out[key[0]]:
        t.fill_(77)   # a sentinel in every slot of every buffer of this call
    cut = host(clone(gpu.sim.closest_points(robot, None, 0.3, max_points=K)))
    assert cut.count.tolist() == full.count.tolist() and (cut.count > K).all() and cut.id_a.shape == (70, K)
    assert np.array_equal(cut.id_a, full.id_a[:, :K]) and np.array_equal(bits(cut.distance), bits(full.distance[:, :K]))
    assert np.array_equal(bits(cut.pos_a), bits(full.pos_a[:, :K])) and np.array_equal(bits(cut.normal), bits(full.normal[:, :K]))
    assert np.array_equal(bits(cut.nearest_distance), bits(full.nearest_distance)) and np.array_equal(cut.nearest_id_a, full.nearest_id_a)
    # every slot behind the rows is written: at 0.03 m only the four wheels (0.0188 m) are rows, fewer than K2 = 6, in buffers
    # full of sentinels
    K2 = 6
    view = gpu.sim.closest_points(robot, None, 0.03, max_points=K2)
    key = [k for k in gpu.sim._closest_out if k[3] == K2]; assert len(key) == 1
    for t in gpu.sim._closest_out[key[0]]:
        t.fill_(77)
    few = host(clone(gpu.sim.closest_points(robot, None, 0.03, max_points=K2)))
    n = few.count
    assert (n < K2).all() and (n > 0).all() and few.id_a.shape == (70, K2)
    for e in range(70):
        assert (few.id_a[e, n[e]:] == -1).all() and (few.id_b[e, n[e]:] == -1).all() and (few.id_a[e, :n[e]] != 77).all()
        assert not few.pos_a[e, n[e]:].any() and not few.pos_b[e, n[e]:].any() and not few.normal[e, n[e]:].any() and not few.distance[e, n[e]:].any()
        assert np.array_equal(bits(few.distance[e, :n[e]]), bits(full.distance[e, :full.count[e]][full.distance[e, :full.count[e]] < 0.03]))
    for t in gpu.sim._closest_out[key[0]]:
        assert not (t == 77).any()
    # the buffers are reused: the same storage comes back, the earlier view now shows the later answer
    again = gpu.sim.closest_points(robot, None, 0.03, max_points=K2)
    assert again.distance.data_ptr() == view.distance.data_ptr() and again.count.data_ptr() == view.count.data_ptr()
    # K = 0: counts and the nearest pair alone
    zero = gpu.sim.closest_points(robot, None, 0.3, max_points=0, want=('nearest', ))
    assert zero.id_a is None and zero.distance is None
    z = host(zero)
    assert z.count.tolist() == full.count.tolist() and np.array_equal(bits(z.nearest_distance), bits(full.nearest_distance))
    assert np.array_equal(bits(z.nearest_normal), bits(full.nearest_normal))
    with pytest.raises(ValueError):
        gpu.sim.closest_points(robot, None, 0.3, max_points=2, want=('nearest', ))


def test_nothing_near_reads_the_distance_itself():
    gpu, r = world('r2d2', 3)
    got = host(gpu.sim.closest_points(r.uids['r2d2'], None, 0.01))
    assert got.count.tolist() == [0] * 3 and (got.nearest_id_a == -1).all() and (got.nearest_id_b == -1).all()
    assert got.nearest_distance.tolist() == [np.float32(0.01)] * 3
    assert not got.nearest_pos_a.any() and not got.nearest_pos_b.any() and not got.nearest_normal.any()
    assert (got.id_a == -1).all() and not got.distance.any()


# ------------------------------------------------------------------------------------------------------- 5. workspace modes
@pytest.mark.parametrize('name,B,modes', (('arms', 70, (({}, 64), ({'DG_MAX_LANES': '16'}, 16), ({'DG_MAX_LANES': '8'}, 0))),
                                          ('marbles', 3, (({}, 32), ({'DG_MAX_LANES': '4'}, 4), ({'DG_MAX_LANES': '1'}, 1)))))
def test_every_workspace_mode_gives_the_same_bits(monkeypatch, name, B, modes):
    """The query kernel uses no workspace; the pose pass in front of it runs in the world's mode.  One state in worlds of several
    modes: identical bits."""
    monkeypatch.delenv('DG_MAX_LANES', raising=False)
    case, r = cc.CASES[name], cc.reference(name, B); ref = None
    for sw, lanes in modes:
        monkeypatch.delenv('DG_MAX_LANES', raising=False)
        for k, v in sw.items():
            monkeypatch.setenv(k, v)
        env = cc.gpu_env(case.scene, B, case.engine)
        assert env.sim.lanes == lanes, (sw, env.sim.lanes)
        env.sim.set_state(r.state)
        ua, ub, dist, _ = r.answers[0]
        got = host(clone(env.sim.closest_points(ua, ub, dist)))
        assert got.count.min() > 0
        if ref is None:
            ref = got
        same_bits(ref, got)
        env.close()


# ------------------------------------------------------------------------------------------------------ 6. proximity_sensor
def test_proximity_sensor_follows_the_reference():
    import torch
    gpu, cpu = cc.gpu_env('marbles', 3), cc.cpu_env('marbles', 3)
    for _ in range(5):
        og, _, _, _ = gpu.step({}); oc, _, _, _ = cpu.step({})
    cpu.sim.set_state(gpu.sim.get_state()); cpu._tick += 1; oc = cpu.observe()
    g, c = og['green_marble'], oc['green_marble']
    loose = BOUND['round-round']
    for name, rng in (('to_red', 0.5), ('to_blue', 0.8), ('to_any', 2.0)):
        assert tuple(g[name]['distance'].shape) == (3, 1) and tuple(g[name]['direction'].shape) == (3, 3)
    # red is 0.1 m away along -x; blue is beyond its range of 0.8 m: the range itself and no direction; anything: the ground
    assert float((g['to_red']['distance'].cpu().double() - c['to_red']['distance'].double()).abs().max()) <= loose['distance']
    assert abs(float(g['to_red']['distance'][0, 0]) - 0.1) < 1e-3
    assert float((g['to_red']['direction'].cpu().double() - c['to_red']['direction'].double()).abs().max()) <= loose['normal']
    assert float((g['to_red']['direction'][:, 0] + 1.0).abs().max()) < 1e-3
    assert g['to_blue']['distance'].tolist() == [[np.float32(0.8)]] * 3 and not g['to_blue']['direction'].any()
    assert float((g['to_any']['distance'].cpu().double() - c['to_any']['distance'].double()).abs().max()) <= BOUND['round-box']['distance']
    assert float((g['to_any']['direction'][:, 2] + 1.0).abs().max()) < 1e-3
    # the observation is the direct reduction of the query
    green, red = gpu.models['green_marble'].uid, gpu.models['red_marble'].uid
    cp = gpu.sim.closest_points(green, red, 0.5, max_points=0, want=('nearest', ))
    assert torch.equal(g['to_red']['distance'][:, 0], cp.nearest_distance) and torch.equal(g['to_red']['direction'], -cp.nearest_normal)


def test_proximity_sensor_terminal_restarts_the_env():
    env = cc.gpu_env('drop_terminal', 3)
    z0 = float(env.observe()['marble']['pose']['position'][0, 2]); fired = None
    for step in range(80):
        obs, _, term, _ = env.step({})
        z = obs['marble']['pose']['position'][:, 2]
        if bool(term.any()):
            fired = step
            assert term.tolist() == [True] * 3
            assert float((z - z0).abs().max()) < 1e-3      # the first observation of the new episode: back at the drop height
            assert float(obs['marble']['clearance']['distance'].min()) > 0.19
            break
        assert float(obs['marble']['clearance']['distance'].min()) >= 0.05
    assert fired is not None and 25 < fired < 60   # (0.15 m of free fall: 0.175 s = 42 steps of 1/240 s)
    obs, _, term, _ = env.step({})
    assert not term.any() and float(obs['marble']['pose']['position'][:, 2].min()) > 0.6
