"""Ray casting on the CPU: known answers through the fp64 numpy reference (tests/raycast_ref.py) and the ``lidar`` addon on
``RaycastOracleBackend``, the reference pinned to the oracle's renderer, and the edge-ray cap of the ray sets the GPU tests use."""
import os

import numpy as np
import pytest
import torch

import raycast_ref as R
from diy_gym_amd import DIYGym
from diy_gym_amd.config import Configuration
from raycast_ref import RaycastOracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(extra=None, B=1):
    tree = {'plane': {'model': 'grass/plane.urdf'},
            'ball': {'model': 'sphere2.urdf', 'xyz': [0, 0, 0.5], 'scale': 0.2, 'use_fixed_base': True},   # radius 0.1, held at z = 0.5
            'crate': {'model': 'wall/wall.urdf', 'use_fixed_base': True, 'scale': 0.01, 'xyz': [3.0, 0.0, 0.0],
                      'rpy': [1.5707963267948966, 0, 1.5707963267948966]}}   # a wall of the maze: 0.1 x 1 x 1 m, standing, its face at x = 2.95
    tree.update(extra or {})
    import diy_gym_amd.examples  # noqa: F401
    return DIYGym(Configuration.from_dict('rays', tree), num_envs=B, seed=1, backend_factory=RaycastOracleBackend)


def _cast(env, a, b, **kw):
    hits = env.sim.ray_test_batch(torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32), **kw)
    return hits, env.sim.last_ray64


def test_known_answers_ground_sphere_box_inside_and_zero_length():
    env = _scene()
    uid = {k: m.uid for k, m in env.models.items()}
    z = 0.5
    a = [[1.0, 1.0, 2.0], [0.0, 0.0, 2.0], [0.0, 0.0, z], [1.0, 1.0, 2.0], [1.0, 1.0, 0.5]]
    b = [[1.0, 1.0, -2.0], [0.0, 0.0, -2.0], [0.0, 0.0, 3.0], [1.0, 1.0, 2.0], [1.0, 1.0, 2.0]]
    hits, r = _cast(env, a, b)
    frac, ids = r['frac'][0], r['id'][0]
    # straight down onto the ground plane (top face z = 0): 2 m of a 4 m ray; normal +z; position on the plane
    assert abs(frac[0] * 4.0 - 2.0) < 1e-9 and ids[0] == uid['plane'] and np.allclose(r['normal'][0, 0], [0, 0, 1]) and np.allclose(r['pos'][0, 0], [1, 1, 0], atol=1e-9)
    # onto the top of sphere2.urdf scaled 0.2 (radius 0.1) at z = 0.5, from 2 m: 2.0 - 0.6
    assert abs(frac[1] * 4.0 - (2.0 - 0.6)) < 1e-9 and ids[1] == uid['ball'] and np.allclose(r['normal'][0, 1], [0, 0, 1], atol=1e-9)
    assert np.isinf(r['margin'][0, 1])
    # a ray that starts inside the sphere does not hit it (and nothing else lies above)
    assert frac[2] == 1.0 and ids[2] == -1 and np.allclose(r['pos'][0, 2], [0, 0, 3.0]) and np.allclose(r['normal'][0, 2], 0.0)
    # a zero-length ray hits nothing; a ray that stops short of everything neither
    assert frac[3] == 1.0 and ids[3] == -1 and frac[4] == 1.0 and ids[4] == -1
    # what the backend hands out: float32 / int32 tensors of the same values
    assert hits.frac.dtype == torch.float32 and hits.id.dtype == torch.int32 and hits.frac.shape == (1, 5) and hits.pos.shape == (1, 5, 3)
    assert np.allclose(hits.frac.numpy(), r['frac'], atol=1e-6) and np.array_equal(hits.id.numpy(), r['id'])


def test_a_ray_that_starts_inside_a_capsule_does_not_hit_it():
    """R2D2's cylinders are capsules here.  From inside one, along its axis (the cylinder term has no root: only the end sphere is
    left, entered from within at a point inside the solid) and obliquely: no hit on that shape.  From outside, the same lines do
    hit it, on its surface."""
    tree = {'r2d2': {'model': 'r2d2.urdf', 'xyz': [0, 0, 2.0], 'use_fixed_base': True}}
    env = DIYGym(Configuration.from_dict('caps', tree), num_envs=1, seed=1, backend_factory=RaycastOracleBackend)
    ref = R.RaycastRef(env.layout)
    caps = [k for k in range(ref.nsh) if ref.SI[k, R.K.SI_TYPE] == R.K.SHAPE_CAPSULE and ref.SF[k, R.K.SF_PARAMS + 1] > 0.05]
    assert caps
    checked = 0
    for k in caps:
        Rm, p = (x[0] for x in ref.shape_poses(env.sim)[k][:2])
        r_, half = ref.SF[k, R.K.SF_PARAMS], ref.SF[k, R.K.SF_PARAMS + 1]
        ax, side = Rm[:, 2], Rm[:, 0]
        far = 2.0 * (half + r_)
        inside = [p, p + ax * 0.5 * half, p - ax * 0.9 * half + side * 0.5 * r_, p + ax * (half + 0.5 * r_)]   # centre, on the axis, off it, in an end cap
        dirs = [ax, -ax, ax + side * 0.3, -ax + side * 0.7, side, ax * 0.2 - side]
        a = np.array([q for q in inside for _ in dirs]); b = np.array([q + v / np.linalg.norm(v) * far for q in inside for v in dirs])
        _, res = _cast(env, a, b)
        assert not (res['shape'][0] == k).any(), (k, res['shape'][0])
        # the same lines from outside: they enter the capsule, at distance r from its axis segment
        _, out = _cast(env, b, a, )
        hit = out['shape'][0] == k
        assert hit.sum() >= len(a) // 2
        x = out['pos'][0][hit]; s_ = np.clip((x - (p - ax * half)) @ ax / (2 * half), 0, 1)
        assert np.allclose(np.linalg.norm(x - ((p - ax * half) + np.outer(s_, ax) * 2 * half), axis=1), r_, atol=1e-9)
        checked += 1
    assert checked


def test_box_face_hit_has_an_axis_normal_and_a_margin():
    env = _scene()
    ref = env.sim._ray_ref if hasattr(env.sim, '_ray_ref') else R.RaycastRef(env.layout)
    crate = env.models['crate'].uid
    boxes = [k for k in range(ref.nsh) if ref.SI[k, R.K.SI_BODY] == crate]
    assert boxes and all(ref.SI[k, R.K.SI_TYPE] in (R.K.SHAPE_BOX, R.K.SHAPE_POINTS) for k in boxes)
    # towards the wall's centre from 2 m in front of its bounding volume, along -x ... and from the side, along +y
    c = np.mean([ref.shape_poses(env.sim)[k][1][0] for k in boxes], axis=0)
    for start, axis in (([c[0] + 2.5, c[1] + 0.2, c[2] + 0.1], 0), ([c[0] + 0.2, c[1] - 2.5, c[2] + 0.1], 1)):   # (a little oblique: every slab has a crossing)
        _, r = _cast(env, [start], [list(c)])
        assert r['id'][0, 0] == crate and 0.0 < r['frac'][0, 0] < 1.0
        n = r['normal'][0, 0]
        assert abs(abs(n[axis]) - 1.0) < 1e-9 and abs(np.linalg.norm(n) - 1.0) < 1e-9, n   # +-axis
        assert np.dot(n, np.asarray(c) - np.asarray(start)) < 0          # facing the ray
        assert np.isfinite(r['margin'][0, 0]) and r['margin'][0, 0] > R.EDGE   # the middle of a face: far from its edges


def test_skip_body_removes_exactly_that_bodys_hits():
    env = _scene()
    rng = np.random.default_rng(3)
    a = np.c_[rng.uniform(-1, 4, 200), rng.uniform(-1.5, 1.5, 200), np.full(200, 2.0)]
    b = np.c_[a[:, 0] + rng.uniform(-1, 1, 200), a[:, 1] + rng.uniform(-1, 1, 200), np.full(200, -1.0)]
    a[:40, :2] = rng.uniform(-0.08, 0.08, (40, 2)); b[:40, :2] = a[:40, :2]   # forty of them onto the ball
    _, full = _cast(env, a, b)
    ball = env.models['ball'].uid
    _, skip = _cast(env, a, b, skip_body=ball)
    on_ball = full['id'][0] == ball
    assert on_ball.sum() >= 30 and (~on_ball).sum() >= 100
    assert not (skip['id'][0] == ball).any()
    assert np.array_equal(skip['id'][0][~on_ball], full['id'][0][~on_ball]) and np.array_equal(skip['frac'][0][~on_ball], full['frac'][0][~on_ball])
    assert (skip['frac'][0][on_ball] > full['frac'][0][on_ball]).all()   # what lay behind the ball (the ground)
    assert (skip['id'][0][on_ball] == env.models['plane'].uid).all()


def test_lidar_addon_ranges_ids_and_the_fan():
    lidar = {'addon': 'lidar', 'xyz': [0.0, 0.0, 0.8], 'num_rays': 8, 'range': [0.1, 4.0], 'use_ids': True}
    down = {'addon': 'lidar', 'xyz': [1.0, 1.0, 2.0], 'rpy': [0.0, 1.5707963267948966, 0.0], 'num_rays': 1, 'horizontal_fov': [0, 0], 'range': [0.5, 5.0]}
    rings = {'addon': 'lidar', 'xyz': [0.0, 0.0, 1.0], 'num_rays': 5, 'num_rings': 3, 'horizontal_fov': [-90, 90], 'vertical_fov': [-30, 30]}
    env = _scene({'scan': lidar, 'down': down, 'rings': rings}, B=2)
    scan = env.addons['scan']
    assert env.observation_space['rays']['scan']['ranges'].shape == (1, 8) and env.observation_space['rays']['scan']['ids'].shape == (1, 8)
    assert float(env.observation_space['rays']['scan']['ranges'].high.max()) == 4.0 and env.observation_space['rays']['rings']['ranges'].shape == (3, 5)
    # a 360 degree fan of N rays: N distinct directions, 360 / N apart, the first along -x (azimuth -180), none doubled
    az = np.degrees(np.arctan2(scan.directions[:, 1], scan.directions[:, 0]))
    assert np.allclose(np.sort(az % 360.0), np.arange(8) * 45.0) and len({tuple(np.round(d, 9)) for d in scan.directions}) == 8
    # a partial fan keeps both ends; rings are elevations towards +z
    rd = env.addons['rings'].directions.reshape(3, 5, 3)
    assert np.allclose(rd[1, 0], [0, -1, 0], atol=1e-12) and np.allclose(rd[1, 4], [0, 1, 0], atol=1e-12) and np.allclose(rd[1, 2], [1, 0, 0], atol=1e-12)
    assert np.allclose(rd[0, :, 2], -0.5) and np.allclose(rd[2, :, 2], 0.5)
    obs = env.observe()['rays']
    rg, ids = obs['scan']['ranges'], obs['scan']['ids']
    assert rg.shape == (2, 1, 8) and rg.dtype == torch.float32 and ids.dtype == torch.int32
    # 0.8 m above the ground, horizontal rays: ray 4 (azimuth 0, +x) meets the wall's face at x = 2.95, the others miss and read max exactly
    crate = env.models['crate'].uid
    assert int(ids[0, 0, 4]) == crate and abs(float(rg[0, 0, 4]) - 2.95) < 1e-5
    miss = ids[0, 0] == -1
    assert int(miss.sum()) >= 5 and bool((rg[0, 0][miss] == 4.0).all())
    # the sensor looking straight down from z = 2 (pitch 90 degrees turns +x into -z): 2 m to the ground
    assert abs(float(obs['down']['ranges'][0, 0, 0]) - 2.0) < 1e-5
    # lazily once per tick: the same tensors until the state changes
    again = env.addons['scan'].observe()['ranges']
    assert again.data_ptr() == scan.observe()['ranges'].data_ptr()
    # attached to a model with ignore_parent (the default): the ball never sees itself
    env2 = _scene({'ball': {'model': 'sphere2.urdf', 'xyz': [0, 0, 0.5], 'scale': 0.2,
                            'eye': {'addon': 'lidar', 'num_rays': 4, 'num_rings': 2, 'vertical_fov': [-90, 0], 'range': [0.0, 3.0], 'use_ids': True}}})
    o2 = env2.observe()['ball']['eye']
    assert not bool((o2['ids'] == env2.models['ball'].uid).any())
    z = float(env2.sim.get_state()[0, env2.layout.body_state_off[env2.models['ball'].uid] + 2])
    assert abs(float(o2['ranges'][0, 0, 0]) - z) < 1e-5 and int(o2['ids'][0, 0, 0]) == env2.models['plane'].uid   # ring 0 looks straight down


def _camera_case(which):
    import yaml
    if which == 'basic_env':
        tree = yaml.safe_load(open(R.BASIC)); tree['camera']['resolution'] = [64, 64]; tree['camera']['use_segmentation_mask'] = True
        rec, name = 'basic_env', 'camera'
    else:
        tree = yaml.safe_load(open(R.SCENES['from_the_readme'][0])); tree['r2d2']['arm_camera']['resolution'] = [40, 40]; tree['r2d2']['arm_camera']['use_segmentation_mask'] = True
        rec, name = 'r2d2', 'arm_camera'
    import diy_gym_amd.examples  # noqa: F401
    env = DIYGym(Configuration.from_dict(which, tree), num_envs=2, seed=2, backend_factory=RaycastOracleBackend)
    R.advance(env, R.actions(env))
    return env, env.receptors[rec].addons[name]


@pytest.mark.parametrize('which', ['basic_env', 'from_the_readme'])
def test_reference_is_pinned_to_the_oracles_renderer(which):
    """Pixel-centre rays (the oracle's own convention, dgo_render) through the numpy reference against the oracle's depth and
    segmentation after 20 oracle steps, both sides fp64.  Largest depth deviation measured on the pixels whose ids agree:
    basic_env 64 x 64: 3.24e-14 m; from_the_readme arm_camera 40 x 40: 2.22e-16 m -- the assertion is ten times the larger
    one (and far below the 1e-4 m at which the reference would be wrong).  Every id agrees in both."""
    env, cam = _camera_case(which)
    cam.observe()
    _, d64, s32 = env.sim.last_render64
    body, frame, a, b, zn, zf = R.pixel_rays(env.layout, cam.camera_index)
    r = R.RaycastRef(env.layout).cast(env.sim, a, b, body, frame)
    depth = -(zn + r['frac'] * (zf - zn))
    d64, s32 = d64.reshape(depth.shape), s32.reshape(depth.shape)
    same = r['id'] == s32
    dev = float(np.abs(depth - d64)[same].max())
    print('%s: ids equal %.6f, max |depth - oracle| %.3g m' % (which, same.mean(), dev))
    assert same.all()
    assert (s32 >= 0).mean() > 0.01    # (something is in the picture)
    assert dev < 10 * 3.24e-14


@pytest.mark.parametrize('scene', sorted(R.SCENES))
def test_the_widened_bounding_sphere_reject_drops_no_hit(scene):
    """The kernel rejects a shape for a ray whose segment stays outside the shape's bounding sphere widened by 1 % + 0.1 mm.
    Restated in the reference (``cull=True``): 6 000 world rays and 6 000 mounted rays per scene give the same shape, fraction
    and normal with and without it -- in particular for the hulls, whose face planes may reach beyond the sphere around their
    (thinned) points."""
    env = R.make_env(scene, 3, backend_factory=R.case_backend())
    R.advance(env, R.actions(env))
    ref = R.RaycastRef(env.layout)
    mb, mf = env.layout.resolve_frame(*R.mount_of(env, scene))
    rng = np.random.default_rng(11)
    lo, hi = (np.asarray(v) for v in R.SCENES[scene][3])
    n = 2000
    a = lo + (hi - lo) * rng.random((n, 3)); b = lo + (hi - lo) * rng.random((n, 3)); b[:, 2] -= 0.6
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    am = (rng.random((n, 3)) - 0.5) * 0.6; bm = am + v * (0.2 + 4 * rng.random((n, 1)))
    for aa, bb, body, frame in ((a, b, -1, -1), (am, bm, mb, mf)):
        full, culled = ref.cast(env.sim, aa, bb, body, frame), ref.cast(env.sim, aa, bb, body, frame, cull=True)
        assert (full['shape'] >= 0).mean() > 0.2
        for key in ('shape', 'frac', 'normal'):
            assert np.array_equal(full[key], culled[key]), (scene, key)


@pytest.mark.parametrize('scene,B', R.CASES)
def test_edge_ray_cap_of_the_gpu_ray_sets(scene, B):
    """At most 2 % of the rays of every seeded ray set the GPU tests use are edge rays (box / hull hits within 1e-3 m, along the
    ray, of the neighbouring face): a condition on the ray sets, not a tolerance."""
    env = R.make_env(scene, B, backend_factory=RaycastOracleBackend)
    R.advance(env, R.actions(env))
    ref = R.RaycastRef(env.layout)
    uid, frame = R.mount_of(env, scene)
    mb, mf = env.layout.resolve_frame(uid, frame)
    hit_any = 0
    for n in R.RAY_COUNTS:
        for name, (a, b, mounted) in R.ray_sets(scene, B, n).items():
            r = ref.cast(env.sim, a, b, mb if mounted else -1, mf if mounted else -1)
            edge = r['margin'] < R.EDGE
            assert edge.mean() <= 0.02, (scene, B, n, name, float(edge.mean()))
            hit_any += int((r['id'] >= 0).sum())
    assert hit_any > 0
