"""One-shot contact manifold for hull-vs-hull pairs (DIYGym(..., hull_manifold_points=N), DG_HF_HULL_MANIFOLD): up to N points per
pair rebuilt every substep from the pair's GJK / polytope normal (diy_gym_amd/csrc/dg_hull.h hull_manifold).

CPU: the numpy restatement (tests/manifold_ref.py) on closed-form cases, and what the keyword does to the scene blob.
GPU: the device routine against the restatement pose by pose, then what the manifold is for -- a free box resting on another."""
import ctypes
import os
import re

import numpy as np
import pytest

import manifold_ref as mr
import oracle_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STACK = os.path.join(ROOT, 'tests', 'golden', 'box_stack.yaml')
STACK_SWAPPED = os.path.join(ROOT, 'tests', 'golden', 'box_stack_swapped.yaml')
MARGIN, HMG = 0.02, 0.001   # contact_margin, hull_margin defaults


def _cube_on_box(upper_half, lower_half, R_up=np.eye(3), xy=(0.0, 0.0), gap=-0.001):
    """A (upper) resting on B (lower, at the origin, axis aligned): A's lowest point `gap` above B's top face."""
    pa, pb = mr.box_points(upper_half), mr.box_points(lower_half)
    low = (pa @ R_up.T)[:, 2].min()
    ta = np.array([xy[0], xy[1], lower_half[2] - low + gap])
    return pa, R_up, ta, pb, np.eye(3), np.zeros(3)


def _run(pa, RA, ta, pb, RB, tb, n=(0.0, 0.0, 1.0), npts=4):
    ra = float(np.max(np.linalg.norm(pa, axis=1))); rb = float(np.max(np.linalg.norm(pb, axis=1)))
    return mr.manifold(pa, RA, ta, pb, RB, tb, np.array(n), ra, rb, MARGIN, HMG, npts)


# ---- the restatement on closed-form cases ------------------------------------------------------------------------------
def test_offset_cube_on_a_larger_box_gives_the_corners_of_the_overlap():
    pa, RA, ta, pb, RB, tb = _cube_on_box([0.05] * 3, [0.1, 0.1, 0.05], xy=(0.08, 0.03), gap=-0.001)
    res = _run(pa, RA, ta, pb, RB, tb)
    assert res is not None and len(res) == 4
    P = np.array([p for p, _ in res])
    want = {(0.03, -0.02), (0.1, -0.02), (0.1, 0.08), (0.03, 0.08)}
    assert {(round(x, 9), round(y, 9)) for x, y in P[:, :2]} == want
    assert np.allclose(P[:, 2], 0.05 - 0.0005) and np.allclose([d for _, d in res], -0.001 - 2 * HMG)
    # slots counter-clockwise about n from A's x axis: angles about the centroid increase
    c = P[:, :2].mean(0); ang = [mr.pseudo_angle(*(p[:2] - c)) for p in P]
    assert ang == sorted(ang)


def test_cube_turned_45_degrees_on_an_equal_cube_keeps_four_octagon_points():
    pa, RA, ta, pb, RB, tb = _cube_on_box([0.05] * 3, [0.05] * 3, R_up=mr.rot_z(np.pi / 4), gap=-0.0005)
    res = _run(pa, RA, ta, pb, RB, tb)
    assert res is not None and len(res) == 4
    P = np.array([p for p, _ in res])[:, :2]
    # the octagon: B's square clipped by A's diamond
    r = 0.05 * np.sqrt(2); octo = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            octo += [(sx * 0.05, sy * (r - 0.05)), (sx * (r - 0.05), sy * 0.05)]
    octo = np.array(octo)
    for p in P:
        assert np.min(np.linalg.norm(octo - p, axis=1)) < 1e-9
    # chosen by the reduction: deepest (all equal: the first), farthest from it, largest triangle, most added area -- a quad of
    # nearly the largest area any four octagon points span
    def area(Q):
        c = Q.mean(0); Q = Q[np.argsort(np.arctan2(Q[:, 1] - c[1], Q[:, 0] - c[0]))]
        return 0.5 * abs(np.sum(Q[:, 0] * np.roll(Q[:, 1], -1) - np.roll(Q[:, 0], -1) * Q[:, 1]))
    import itertools
    best = max(area(octo[list(s)]) for s in itertools.combinations(range(8), 4))
    assert area(P) > 0.95 * best


def test_edge_on_a_face_gives_two_points():
    pa, RA, ta, pb, RB, tb = _cube_on_box([0.05] * 3, [0.2, 0.2, 0.05], R_up=mr.rot_x(np.pi / 4), gap=-0.001)
    res = _run(pa, RA, ta, pb, RB, tb)
    assert res is not None and len(res) == 2
    P = np.array([p for p, _ in res])
    assert np.allclose(sorted(P[:, 0]), [-0.05, 0.05]) and np.allclose(P[:, 1], 0.0)
    assert np.allclose([d for _, d in res], -0.001 - 2 * HMG)


def test_a_vertex_on_a_face_or_crossed_edges_keep_the_single_contact():
    # a corner pointing down: rotate the body diagonal (1, 1, 1) onto -z
    d = np.array([1.0, 1.0, 1.0]) / np.sqrt(3); t = np.array([0.0, 0.0, -1.0]); k = np.cross(d, t); s, c = np.linalg.norm(k), d @ t
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]]) / s
    R_corner = np.eye(3) + np.sin(np.arccos(c)) * kx + (1 - c) * kx @ kx
    pa, RA, ta, pb, RB, tb = _cube_on_box([0.05] * 3, [0.2, 0.2, 0.05], R_up=R_corner)
    assert _run(pa, RA, ta, pb, RB, tb) is None
    # crossed edges: A's lowest edge along x, B's highest edge along y
    pa, pb = mr.box_points([0.05] * 3), mr.box_points([0.05] * 3)
    RA = mr.rot_x(np.pi / 4)
    RB = np.array([[np.cos(np.pi / 4), 0, np.sin(np.pi / 4)], [0, 1, 0], [-np.sin(np.pi / 4), 0, np.cos(np.pi / 4)]])
    ta = np.array([0.0, 0.0, 2 * 0.05 * np.sqrt(2) - 0.001])
    assert _run(pa, RA, ta, pb, RB, np.zeros(3)) is None


def test_a_gap_below_the_contact_margin_gives_positive_depths_and_beyond_it_none():
    pa, RA, ta, pb, RB, tb = _cube_on_box([0.05] * 3, [0.1, 0.1, 0.05], gap=0.01)
    res = _run(pa, RA, ta, pb, RB, tb)
    assert len(res) == 4 and np.allclose([d for _, d in res], 0.01 - 2 * HMG) and all(d > 0 for _, d in res)
    pa, RA, ta, pb, RB, tb = _cube_on_box([0.05] * 3, [0.1, 0.1, 0.05], gap=0.03)
    assert _run(pa, RA, ta, pb, RB, tb) is None


def test_a_tilted_face_is_measured_as_tilted_whichever_hull_is_a():
    """A cube tilted 0.5 degrees over a flat box, its lowest edge 0.5 mm into it: the corners of its face are 0.5 mm into the box
    and 0.373 mm above it -- with the cube as A (its face is the reference) and with the box as A alike."""
    th = np.radians(0.5); lift = 0.1 * np.sin(th)
    pa, RA, ta, pb, RB, tb = _cube_on_box([0.05] * 3, [0.1, 0.1, 0.05], R_up=mr.rot_x(th), gap=-0.0005)
    want = sorted([-0.0005, -0.0005, -0.0005 + lift, -0.0005 + lift])
    as_a = _run(pa, RA, ta, pb, RB, tb)
    as_b = _run(pb, RB, tb, pa, RA, ta, n=(0.0, 0.0, -1.0))
    for res in (as_a, as_b):
        assert res is not None and len(res) == 4
        assert np.allclose(sorted(d + 2 * HMG for _, d in res), want, atol=2e-6), [d for _, d in res]
    # the same contact points: midway between the box's face and the cube's
    Pa = sorted(tuple(np.round(p, 5)) for p, _ in as_a); Pb = sorted(tuple(np.round(p, 5)) for p, _ in as_b)
    assert np.allclose(Pa, Pb, atol=2e-5)


def test_fewer_points_asked_for():
    pa, RA, ta, pb, RB, tb = _cube_on_box([0.05] * 3, [0.1, 0.1, 0.05], xy=(0.08, 0.03))
    for n in (2, 3):
        assert len(_run(pa, RA, ta, pb, RB, tb, npts=n)) == n


# ---- the keyword and the scene blob ------------------------------------------------------------------------------------
def _env(cfg, **kw):
    from diy_gym_amd import DIYGym
    return DIYGym(cfg, num_envs=2, backend_factory=oracle_backend.OracleBackend, **kw)


def test_one_point_is_the_blob_of_today_but_the_new_slot():
    from diy_gym_amd.scene import K
    for cfg in (STACK, os.path.join(ROOT, 'tests', 'golden', 'ur_arms_touching.yaml')):
        a, b = _env(cfg).layout, _env(cfg, hull_manifold_points=1).layout
        assert np.array_equal(a.I, b.I) and a.state_dim == b.state_dim and a.max_contacts == b.max_contacts
        mask = np.ones(len(a.F), bool); mask[K.HF_HULL_MANIFOLD] = False
        assert np.array_equal(a.F[mask], b.F[mask]) and a.F[K.HF_HULL_MANIFOLD] == b.F[K.HF_HULL_MANIFOLD] == 1.0


def test_four_points_raise_the_budget_only_where_hulls_meet_hulls():
    from diy_gym_amd.scene import K
    one, four = _env(STACK).layout, _env(STACK, hull_manifold_points=4).layout
    assert four.max_contacts > one.max_contacts and four.F[K.HF_HULL_MANIFOLD] == 4.0
    assert four.max_contacts <= 32
    for name in ('pendulum.yaml', 'basic_env_nocam.yaml'):
        cfg = os.path.join(ROOT, 'tests', 'golden', name)
        a, b = _env(cfg).layout, _env(cfg, hull_manifold_points=4).layout
        assert a.max_contacts == b.max_contacts and a.state_dim == b.state_dim
    # without hull contacts the hulls collide through their capsules: one contact a pair, whatever N
    a, b = _env(STACK, engine={'hull_contacts': 0.0}).layout, _env(STACK, hull_manifold_points=4, engine={'hull_contacts': 0.0}).layout
    assert a.max_contacts == b.max_contacts


@pytest.mark.parametrize('bad', [0, 5, -1, 2.5, True])
def test_out_of_range_values_are_refused(bad):
    with pytest.raises(ValueError):
        _env(STACK, hull_manifold_points=bad)


def test_it_is_not_an_engine_parameter():
    from diy_gym_amd.scene import DEFAULTS
    assert 'hull_manifold_points' not in DEFAULTS
    with pytest.raises(KeyError):
        _env(STACK, engine={'hull_manifold_points': 4})


def test_the_header_documents_the_slot_and_the_tolerance():
    text = open(os.path.join(ROOT, 'include', 'diygym_scene.h')).read()
    assert float(re.search(r'#define DG_HULL_MANIFOLD_TOL ([0-9.]+)f', text).group(1)) == mr.TOL
    hull = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_hull.h')).read()
    assert int(re.search(r'#define HH_MF_CAP (\d+)', hull).group(1)) == mr.CAP
    assert int(re.search(r'#define HH_MF_CLIP (\d+)', hull).group(1)) == mr.CLIP


# ---- the device routine against the restatement --------------------------------------------------------------------------
def bound_radius(pts):
    """The radius the step kernel scales the feature tolerance with: a hull's SC_BOUND with hull contacts on, max(fitted capsule
    radius + half length, radius of the sphere about its centre that holds every point) -- scene.py's shape parameters."""
    from diy_gym_amd.scene import fit_capsule
    T, r, half = fit_capsule(np.asarray(pts, np.float64))
    return float(max(r + half, np.max(np.linalg.norm(pts - T.p, axis=1))))


def device_manifold(pa, pb, ra, rb, poses, npts=4):
    from diy_gym_amd import backend
    lib = backend.load_library(); vp = ctypes.c_void_p
    lib.dg_debug_hull_manifold.restype = ctypes.c_int32
    lib.dg_debug_hull_manifold.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int32, ctypes.c_float, ctypes.c_float, vp, ctypes.c_int32,
                                           ctypes.c_float, ctypes.c_float, ctypes.c_int32, vp]
    pa = np.ascontiguousarray(pa, np.float32); pb = np.ascontiguousarray(pb, np.float32); poses = np.ascontiguousarray(poses, np.float32)
    out = np.zeros((len(poses), 25), np.float32); p = lambda a: a.ctypes.data_as(vp)
    rc = lib.dg_debug_hull_manifold(p(pa), len(pa), p(pb), len(pb), ra, rb, p(poses), len(poses), MARGIN, HMG, npts, p(out))
    lib.dg_last_error.restype = ctypes.c_char_p
    assert rc == 0, lib.dg_last_error()
    return out


def _rot_onto(a, b):
    """Rotation taking unit vector a onto unit vector b."""
    k = np.cross(a, b); s, c = np.linalg.norm(k), float(a @ b)
    if s < 1e-12:
        if c > 0:
            return np.eye(3)
        p = np.array([1.0, 0, 0]) if abs(a[0]) < 0.9 else np.array([0, 1.0, 0]); k = np.cross(a, p); k /= np.linalg.norm(k)
        kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]]); return np.eye(3) + 2 * kx @ kx
    k = k / s; kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + s * kx + (1 - c) * kx @ kx


def touching_poses(pa, pb, rng, n):
    """Poses [n][24] of A near / on B: half face to face (a facet of each turned to meet along z, random yaw, tilt 0.05 .. 0.5
    degrees, faces offset by up to a third of their size), half in random orientations; A's lowest point 2 mm below .. 5 mm
    above B's highest along z."""
    from scipy.spatial import ConvexHull
    from scipy.spatial.transform import Rotation
    ha, hb = ConvexHull(pa), ConvexHull(pb); rows = []
    size = 0.5 * (np.ptp(pa, 0).max() + np.ptp(pb, 0).max())
    for k in range(n):
        if k % 2 == 0:
            fa, fb = rng.integers(len(ha.equations)), rng.integers(len(hb.equations))
            RB = mr.rot_z(rng.uniform(0, 2 * np.pi)) @ _rot_onto(hb.equations[fb, :3], np.array([0, 0, 1.0]))
            tilt = Rotation.from_rotvec(np.radians(rng.uniform(0.05, 0.5)) * np.array([*rng.normal(size=2), 0.0]) / 1.0).as_matrix()
            RA = tilt @ mr.rot_z(rng.uniform(0, 2 * np.pi)) @ _rot_onto(ha.equations[fa, :3], np.array([0, 0, -1.0]))
            ca = (pa[ha.simplices[fa]] @ RA.T).mean(0); cb = (pb[hb.simplices[fb]] @ RB.T).mean(0)
            xy = cb[:2] - ca[:2] + rng.uniform(-1, 1, 2) * size / 3
        else:
            RA = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix(); RB = Rotation.random(random_state=int(rng.integers(1 << 30))).as_matrix()
            xy = rng.uniform(-1, 1, 2) * size / 3
        z = (pb @ RB.T)[:, 2].max() - (pa @ RA.T)[:, 2].min() + rng.uniform(-0.002, 0.005)
        rows.append(np.concatenate([RA.reshape(-1), [xy[0], xy[1], z], RB.reshape(-1), [0.0, 0.0, 0.0]]))
    return np.array(rows)


def _hull_sets():
    from diy_gym_amd import mesh
    ur5 = mesh.load_convex(os.path.join(ROOT, 'diy_gym_amd', 'data', 'ur5', 'hulls', 'forearm_link_0.obj'), 32)
    finger = mesh.load_convex(os.path.join(ROOT, 'diy_gym_amd', 'data', 'jaco', 'hulls', 'j2s7s300_link_finger_1_0.obj'), 32)
    r2d2 = open(os.path.join(ROOT, 'diy_gym_amd', 'data', 'pybullet_data', 'r2d2.urdf')).read()
    size = np.array([float(v) for v in re.search(r'<box size="([^"]+)"', r2d2).group(1).split()]) * 0.1   # (from_the_readme: scale 0.1)
    return [('box_box', mr.box_points([0.05, 0.05, 0.05]), mr.box_points([0.1, 0.1, 0.05])),
            ('ur5_box', ur5, mr.box_points([0.05, 0.05, 0.05])),
            ('finger_r2d2', finger, mr.box_points(size / 2))]


def _compare(pa, pb, poses, out, ra, rb):
    """-> (poses compared, count differences, point differences on equal counts), asserting the single-contact fallbacks."""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    n_cnt = n_pts = n_slot = 0
    for k, row in enumerate(poses):
        o = out[k].astype(np.float64)
        if o[0] == 0:
            continue
        RA, ta, RB, tb = f32(row[:9]).reshape(3, 3), f32(row[9:12]), f32(row[12:21]).reshape(3, 3), f32(row[21:24])
        ref = mr.manifold(f32(pa), RA, ta, f32(pb), RB, tb, o[2:5], float(np.float32(ra)), float(np.float32(rb)), MARGIN, HMG, 4)
        dev_single = o[1] == 1
        if ref is None and dev_single:
            continue
        if ref is None or dev_single or len(ref) != int(o[0]):
            n_cnt += 1; continue
        P = o[5:5 + 5 * len(ref)].reshape(-1, 5)
        ok = all(np.linalg.norm(P[s, :3] - ref[s][0]) < 1e-4 and abs(P[s, 3] - ref[s][1]) < 1e-4 for s in range(len(ref)))
        if not ok:   # the same points in other slots (an angle tie about the centroid) or other points (a tie of the reduction)
            same = all(min(np.linalg.norm(P[s, :3] - r[0]) + abs(P[s, 3] - r[1]) for r in ref) < 1e-4 for s in range(len(ref)))
            n_slot += same; n_pts += not same
    return n_cnt, n_pts, n_slot


@pytest.mark.gpu
def test_device_manifold_matches_the_restatement():
    """Closed-form cases, then 2 048 random touching or near poses each of (box, box), (UR5 forearm hull, box) and (Jaco finger
    hull, R2D2 box hull).  Where both keep the single contact, the device's is dg_debug_hull_hull's (normal 1e-3, depth 2e-6 --
    GJK's tolerance, as test_hull_contacts holds it to the checker -- in all but 0.5 % of the poses; and exactly the N = 1 output of the same entry); otherwise the counts are equal and points and depths agree within 1e-4 m.  Count differences (a point on a threshold:
    feature tolerance, parallel edges, contact margin -- fp32 on the device, fp64 here) are counted and bounded: 0.5 %, 1.5 % for
    the finger hull."""
    from test_hull_contacts import device_pairs
    # closed form: the offset cube gives the overlap rectangle on the device too
    pa, RA, ta, pb, RB, tb = _cube_on_box([0.05] * 3, [0.1, 0.1, 0.05], xy=(0.08, 0.03), gap=-0.001)
    ra, rb = bound_radius(pa), bound_radius(pb)
    o = device_manifold(pa, pb, ra, rb, np.concatenate([RA.reshape(-1), ta, RB.reshape(-1), tb])[None])[0]
    assert o[0] == 4 and o[1] == 0 and np.allclose(o[2:5], [0, 0, 1], atol=1e-5)
    P = o[5:25].reshape(4, 5)
    assert {(round(float(x), 4), round(float(y), 4)) for x, y in P[:, :2]} == {(0.03, -0.02), (0.1, -0.02), (0.1, 0.08), (0.03, 0.08)}
    assert np.allclose(P[:, 3], -0.003, atol=1e-5) and list(P[:, 4]) == [0, 1, 2, 3]
    rng = np.random.default_rng(11); report = {}
    for name, pa, pb in _hull_sets():
        ra, rb = bound_radius(pa), bound_radius(pb)
        poses = touching_poses(pa, pb, rng, 2048)
        out = device_manifold(pa, pb, ra, rb, poses)
        one = device_manifold(pa, pb, ra, rb, poses, npts=1)
        ref = device_pairs(pa, pb, poses, max_dist=MARGIN + 2 * HMG).astype(np.float32)
        hit = one[:, 0] == 1
        assert np.array_equal(hit, (ref[:, 10] == 1) & (ref[:, 9] - np.float32(2 * HMG) < np.float32(MARGIN)))
        # (two kernels compiled from the same source round differently -- where the compiler fuses a multiply-add: the same
        # contact to GJK's own tolerance, as tests/test_hull_contacts.py holds it to the checker, not to the bit; N = 1 in the step kernel IS today's kernel bit for bit, test_shipped_scenes_...)
        # (a few poses sit where the polytope search is nearly degenerate and the rounding picks a neighbouring face: <= 0.5 %)
        assert np.all(one[hit, 1] == 1)
        # (the point is not compared: where two faces touch, the witness points may sit anywhere on the shared patch)
        close = (np.abs(one[hit, 2:5] - ref[hit, 6:9]).max(1) < 1e-3) & (np.abs(one[hit, 8] - (ref[hit, 9] - np.float32(2 * HMG))) < 2e-6)
        assert np.sum(~close) <= 0.005 * len(poses), (name, int(np.sum(~close)))
        single = out[:, 1] == 1
        assert np.array_equal(out[single], one[single])   # the fallback is exactly the one-point contact
        n_cnt, n_pts, n_slot = _compare(pa, pb, poses, out, ra, rb)
        multi = int(np.sum(out[:, 0] > 1))
        report[name] = (int(hit.sum()), multi, n_cnt, n_pts, n_slot, int(np.sum(~close)))
        assert multi > 200, report
        # (count differences: a hull point on the feature tolerance, fp32 here and fp64 there -- measured 0 / 2 / 19 of 2 048 for
        # box-box / UR5-box / finger-R2D2: the finger hull has many nearly coplanar points, and 0.5 % does not hold for it)
        assert n_cnt <= (0.015 if name == 'finger_r2d2' else 0.005) * len(poses), report
        # (equal counts, other points: a tie of the reduction; the same points in other slots: an angle tie -- measured <= 5 and <= 8)
        assert n_pts <= 0.005 * len(poses), report
        assert n_slot <= 0.005 * len(poses), report
    print('manifold vs restatement (poses in contact, with a manifold, count differences, point differences, slot order only, '
          'single contacts off):', report)


# ---- the manifold at work: free boxes at rest ---------------------------------------------------------------------------
def stack_env(B, N, offset_frac=None, seed=0, device='cuda:0', swapped=False, tilt_deg=0.0):
    """box_stack.yaml with the cube at a random yaw and a random offset (its centre of mass over the lower box), or at
    `offset_frac` x the lower box's width from its centre along x (yaw 0): > 0.5 beyond the edge.  swapped: the cube listed
    first (its hull is A of the pair); tilt_deg: the cube tilted about its x axis, its lowest edge at the rest height."""
    import torch
    from diy_gym_amd import DIYGym
    env = DIYGym(STACK_SWAPPED if swapped else STACK, num_envs=B, device=device, seed=seed, hull_manifold_points=N)
    env._upper = 1 if swapped else 2
    st = env.sim.get_state(); rng = np.random.default_rng(seed); L = env.layout
    o = L.body_state_off[env._upper]
    if offset_frac is None:
        yaw = rng.uniform(0, 2 * np.pi, B); xy = rng.uniform(-0.04, 0.04, (B, 2))
    else:
        yaw = np.zeros(B); xy = np.stack([np.full(B, offset_frac * 0.2), np.zeros(B)], 1)
    th = np.radians(tilt_deg)
    st[:, o:o + 2] = xy; st[:, o + 2] = 0.1 + 2 * HMG + 0.05 * (np.cos(th) + np.sin(th))
    # q = q_yaw (about z) x q_tilt (about x), xyzw
    cy, sy, ct, stt = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(th / 2), np.sin(th / 2)
    st[:, o + 3:o + 7] = np.stack([cy * stt, sy * stt, sy * ct, cy * ct], 1)
    env.sim.set_state(st)
    return env


def run_stack(env, steps):
    import torch
    d = env.sim.enable_diagnostics()
    act = torch.zeros((env.num_envs, max(env.layout.act_dim, 1)), device='cuda:0')
    for _ in range(steps):
        env.sim.step(env._all_slots, act)
    torch.cuda.synchronize()
    return env.sim.get_state(), d[:, 0].cpu().numpy()


def stack_metrics(env, st):
    o = env.layout.body_state_off[env._upper]; q = st[:, o + 3:o + 7]
    tilt = np.degrees(2 * np.arcsin(np.clip(np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2), 0, 1)))
    w = np.linalg.norm(st[:, o + 10:o + 13], axis=1)
    return tilt, w, st[:, o + 2], st[:, o:o + 2]


REST_Z = 0.1 + 2 * HMG + 0.05   # lower box top + twice the hull margin + half the cube


def _check_rest(env, st, cnt):
    tilt, w, z, _ = stack_metrics(env, st)
    assert np.isfinite(st).all()
    assert tilt.max() < 0.2, tilt.max()
    assert w.max() < 1e-2, w.max()
    assert np.abs(z - REST_Z).max() < 1e-3, (z.min(), z.max())
    assert np.all(cnt == 8), np.unique(cnt, return_counts=True)   # 4 under the lower box, 4 between the boxes


@pytest.mark.gpu
def test_stacked_free_boxes_rest_on_four_points():
    """1 024 envs, random yaw and offset of the cube: after 480 steps every env at rest -- tilt < 0.2 degree, |omega| < 1e-2
    rad/s, height within 1 mm of the rest height with margins, 4 contacts on the box-box pair.  With one point (recorded, not
    asserted) the same stack does not settle."""
    env = stack_env(1024, 4)
    st, cnt = run_stack(env, 480)
    _check_rest(env, st, cnt)
    one = stack_env(1024, 1)
    st1, _ = run_stack(one, 480)
    tilt, w, z, _ = stack_metrics(one, st1)
    print('one point per pair after 480 steps: tilt max %.3g deg (median %.3g), |omega| max %.3g rad/s, height %.4f .. %.4f m, finite %s'
          % (np.nanmax(tilt), np.nanmedian(tilt), np.nanmax(w), np.nanmin(z), np.nanmax(z), np.isfinite(st1).all()))


@pytest.mark.gpu
def test_a_tilted_cube_listed_first_settles_flat():
    """The cube listed before the box (its hull is A: its own face is the reference of the clip) and started tilted 0.5 degree
    on its edge: after 480 steps every env lies flat and at rest on 4 + 4 contacts."""
    env = stack_env(1024, 4, swapped=True, tilt_deg=0.5, seed=2)
    st, cnt = run_stack(env, 480)
    _check_rest(env, st, cnt)


@pytest.mark.gpu
def test_tipping_follows_the_centre_of_mass():
    """The cube's centre of mass 10 % of the lower box's width inside its edge stays; 10 % beyond it falls off."""
    stay = stack_env(64, 4, offset_frac=0.4)
    st, _ = run_stack(stay, 480)
    tilt, w, z, xy = stack_metrics(stay, st)
    assert tilt.max() < 0.2 and np.abs(z - REST_Z).max() < 1e-3 and np.abs(xy[:, 0] - 0.08).max() < 1e-3
    fall = stack_env(64, 4, offset_frac=0.6)
    st, _ = run_stack(fall, 480)
    tilt, w, z, xy = stack_metrics(fall, st)
    assert np.isfinite(st).all() and np.all(z < REST_Z - 0.02), z.max()


@pytest.mark.gpu
def test_warm_start_keys_of_the_resting_stack_hold_still():
    """The keys in the warm-start cache at steps 300 and 301 are the same set in every env."""
    env = stack_env(256, 4, seed=3)
    L = env.layout; assert L.warm_off >= 0
    run_stack(env, 300); k300 = _keys(env)
    run_stack(env, 1); k301 = _keys(env)
    assert all(a == b for a, b in zip(k300, k301))
    assert all(len(a) == 8 for a in k300)


def _keys(env):
    from diy_gym_amd.scene import K
    st = env.sim.get_state(); o = env.layout.warm_off
    return [sorted(int(st[e, o + 1 + j * K.WS_STRIDE + K.WS_KEY]) for j in range(int(st[e, o]))) for e in range(env.num_envs)]


@pytest.mark.gpu
@pytest.mark.parametrize('switches', [{}, {'DG_MAX_LANES': '16'}, {'DG_MAX_LANES': '1'}, {'DG_NO_NARROW_MODES': '1'}])
def test_stack_rests_in_every_kernel_mode(switches, monkeypatch):
    """The resting stack in the default mode and under the DG_* switches, then a masked reset with DG_NO_PAR_RESET: the reset
    envs go back to the YAML pose and the others stay at rest."""
    import torch
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('DG_NO_PAR_RESET', '1')
    env = stack_env(1024, 4)
    st, cnt = run_stack(env, 480)
    _check_rest(env, st, cnt)
    mask = torch.zeros(env.num_envs, dtype=torch.bool); mask[::3] = True
    env.sim.reset(mask.to('cuda:0'))
    st, cnt = run_stack(env, 240)
    tilt, w, z, _ = stack_metrics(env, st)
    assert np.isfinite(st).all() and tilt.max() < 0.2 and np.abs(z - REST_Z).max() < 1e-3
    assert np.all(cnt == 8)


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', ['tests/golden/ur_arms_touching.yaml', 'examples/from_the_readme/from_the_readme.yaml'])
def test_shipped_scenes_with_the_manifold(cfg):
    """200 steps with N = 4: all outputs finite, at most 4 contacts on any pair (counted from the keys in the warm-start cache);
    with N = 1 given explicitly the outputs are bit-identical to the default construction."""
    import torch
    from diy_gym_amd import DIYGym
    path = os.path.join(ROOT, cfg); B = 64
    envs = [DIYGym(path, num_envs=B, device='cuda:0', seed=4, **kw) for kw in ({}, {'hull_manifold_points': 1}, {'hull_manifold_points': 4})]
    diags = [e.sim.enable_diagnostics() for e in envs]
    gen = torch.Generator().manual_seed(1); most = 0; per_pair = 0
    L4 = envs[2].layout; assert L4.warm_off >= 0
    for _ in range(200):
        act = ((torch.rand((B, envs[0].layout.act_dim), generator=gen) * 2 - 1) * 0.3).to('cuda:0')
        for e in envs:
            e.sim.step(e._all_slots, act)
        assert torch.equal(envs[0].sim.obs, envs[1].sim.obs) and torch.equal(envs[0].sim.rew, envs[1].sim.rew)
        most = max(most, int(diags[2][:, 0].max()))
        # contacts per candidate pair in the last substep, from the keys of the warm-start cache (key = pair x 256 + feature)
        for keys in _keys(envs[2]):
            if keys:
                per_pair = max(per_pair, int(np.bincount(np.asarray(keys) // 256).max()))
    assert torch.equal(envs[0].sim.state, envs[1].sim.state)
    assert torch.isfinite(envs[2].sim.obs).all() and np.isfinite(envs[2].sim.get_state()).all()
    assert 1 <= per_pair <= 4
    print('%s: N = 4 kernel %s, budget %d (N = 1: %s, %d); most contacts in an env %d, on one pair %d'
          % (cfg, envs[2].sim.kernel_name, L4.max_contacts, envs[0].sim.kernel_name, envs[0].layout.max_contacts, most, per_pair))
