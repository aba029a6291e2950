"""dg_world_raycast / env.sim.ray_test_batch / the lidar addon on the GPU against the fp64 numpy reference (tests/raycast_ref.py),
on states advanced by the same 20 random-action steps on both backends (the pattern of test_hip_render_matches_oracle).
Tolerances are those of tests/test_camera.py: ids equal on > 99.5 % of the rays; on the agreeing rays 1e-3 m in distance along
the ray and in hit position; normals within 1e-3 on agreeing rays that are not edge rays (raycast_ref.EDGE)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import raycast_ref as R
from diy_gym_amd import DIYGym
from diy_gym_amd.config import Configuration

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
_CASES = {}


def case(scene, B):
    """(gpu env, cpu env, reference) of a case, both envs advanced by the same actions; built once per session."""
    if (scene, B) not in _CASES:
        gpu = R.make_env(scene, B, device=DEV)
        cpu = R.make_env(scene, B, backend_factory=R.case_backend())
        acts = R.actions(cpu)
        R.advance(gpu, acts); R.advance(cpu, acts)
        _CASES[(scene, B)] = (gpu, cpu, R.RaycastRef(cpu.layout))
    return _CASES[(scene, B)]


def combos(B):
    """(ray count, form) pairs of a case: the whole cross product at the small batches.  At 70 envs every ray count in both
    per-env forms (their indexing is env x n_rays) and both shared forms at 65 rays (a chunk and its tail; the chunking of
    shared rays does not depend on the batch): the fp64 reference costs 0.3 - 0.5 s per cast of the 136-shape maze at 70 envs,
    the whole cross product 10 s of a test that is to take a few."""
    if B <= 3:
        return [(n, f) for n in R.RAY_COUNTS for f in R.FORMS]
    return [(n, f) for n in R.RAY_COUNTS for f in R.FORMS if f.endswith('per_env')] + [(65, f) for f in R.FORMS if f.endswith('shared')]


def gpu_cast(env, a, b, mount=None, **kw):
    a, b = torch.as_tensor(a, device=DEV), torch.as_tensor(b, device=DEV)
    if mount is not None:
        kw.update(body=mount[0], frame=mount[1])
    return env.sim.ray_test_batch(a, b, **kw)


def compare(hits, r, label):
    """The tolerances of this file between RayHits of the GPU and the reference's dict; returns (rays, id mismatches)."""
    frac, ids = hits.frac.cpu().numpy().astype(np.float64), hits.id.cpu().numpy()
    same = ids == r['id']
    d_frac = np.abs(frac - r['frac']) * r['length']
    d_pos = np.linalg.norm(hits.pos.cpu().numpy() - r['pos'], axis=-1)
    nrm = same & (r['id'] >= 0) & ~(r['margin'] < R.EDGE)
    d_n = np.abs(hits.normal.cpu().numpy() - r['normal']).max(-1)
    worst = (float(d_frac[same].max()) if same.any() else 0.0, float(d_pos[same].max()) if same.any() else 0.0, float(d_n[nrm].max()) if nrm.any() else 0.0)
    print('%s: rays %d, ids differ %d, hit %.2f, max dist %.3g m, pos %.3g m, normal %.3g' % ((label, same.size, int((~same).sum()), float((r['id'] >= 0).mean())) + worst))
    assert worst[0] < 1e-3 and worst[1] < 1e-3 and worst[2] < 1e-3, (label, worst)
    assert bool(((frac >= 0) & (frac <= 1)).all()) and bool((frac[ids < 0] == 1.0).all()) and bool((frac[ids >= 0] < 1.0).all()), label
    return same.size, int((~same).sum())


@pytest.mark.parametrize('scene,B', R.CASES)
def test_raycast_matches_the_reference(scene, B):
    gpu, cpu, ref = case(scene, B)
    uid, frame = R.mount_of(gpu, scene)
    mb, mf = cpu.layout.resolve_frame(uid, frame)
    total = differ = hit = 0
    for n, form in combos(B):
        a, b, mounted = R.ray_sets(scene, B, n)[form]
        hits = gpu_cast(gpu, a, b, (uid, frame) if mounted else None)
        r = ref.cast(cpu.sim, a, b, mb if mounted else -1, mf if mounted else -1)
        assert hits.frac.shape == (B, n) and hits.id.shape == (B, n) and hits.pos.shape == (B, n, 3) and hits.normal.shape == (B, n, 3)
        t, d = compare(hits, r, '%s x%d n=%d %s' % (scene, B, n, form))
        total += t; differ += d; hit += int((r['id'] >= 0).sum())
    print('%s x%d: %d rays, %d ids differ (%.4f), %d hits' % (scene, B, total, differ, differ / total, hit))
    assert 1.0 - differ / total > 0.995
    assert hit > 0.2 * total    # (the ray sets do meet the scene)


@pytest.mark.parametrize('scene,B', [('basic_env', 3), ('from_the_readme', 3), ('from_the_readme', 70), ('r2d2_maze', 3), ('r2d2_maze', 1), ('r2d2_maze', 70)])
def test_bitwise_properties(scene, B):
    """Shared rays and the same rays broadcast per env, two calls on one state, outputs left out, the kernel that reads the
    table through wave-uniform loads instead of LDS, and the kernel with its bounding-sphere rejects switched off: all the same bits."""
    gpu, _, _ = case(scene, B)
    mount = R.mount_of(gpu, scene)
    lib = gpu.sim.lib
    lib.dg_debug_raycast_lds_words.restype = ctypes.c_int32
    lib.dg_debug_raycast_lds_words.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    lib.dg_debug_raycast_no_cull.restype = ctypes.c_int32
    lib.dg_debug_raycast_no_cull.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    for n in (65, 130):
        for form in ('world_shared', 'mounted_shared'):
            a, b, mounted = R.ray_sets(scene, B, n)[form]
            m = mount if mounted else None
            first = [t.clone() for t in gpu_cast(gpu, a, b, m)]
            again = gpu_cast(gpu, a, b, m)
            for x, y in zip(first, again):
                assert torch.equal(x, y), (n, form, 'second call')
            per_env = gpu_cast(gpu, np.broadcast_to(a, (B, ) + a.shape).copy(), np.broadcast_to(b, (B, ) + b.shape).copy(), m)
            for x, y in zip(first, per_env):
                assert torch.equal(x, y), (n, form, 'per_env')
            only = gpu_cast(gpu, a, b, m, want=('frac', ))
            assert only.id is None and only.pos is None and only.normal is None and torch.equal(only.frac, first[0]), (n, form, 'frac only')
            try:
                assert lib.dg_debug_raycast_lds_words(gpu.sim.handle, 0) == 0
                table = gpu_cast(gpu, a, b, m)
                for x, y in zip(first, table):
                    assert torch.equal(x, y), (n, form, 'table-reading kernel')
            finally:
                assert lib.dg_debug_raycast_lds_words(gpu.sim.handle, 12288) == 0
            try:   # every ray against every shape: the bounding-sphere rejects (per wavefront and per lane) change no bit
                assert lib.dg_debug_raycast_no_cull(gpu.sim.handle, 1) == 0
                brute = gpu_cast(gpu, a, b, m)
                for x, y in zip(first, brute):
                    assert torch.equal(x, y), (n, form, 'no cull')
            finally:
                assert lib.dg_debug_raycast_no_cull(gpu.sim.handle, 0) == 0
            assert bool((first[1] >= 0).any())


def _camera_env():
    import yaml
    tree = yaml.safe_load(open(R.BASIC))
    tree['camera']['use_segmentation_mask'] = True
    tree['camera']['resolution'] = [64, 64]
    tree['green_marble']['eye'] = {'addon': 'camera', 'xyz': [0, -2.0, 0.5], 'rpy': [1.2, 0, 0], 'resolution': [40, 40], 'use_segmentation_mask': True}
    env = DIYGym(Configuration.from_dict('basic_env', tree), num_envs=3, device=DEV, seed=2)
    R.advance(env, R.actions(env))
    return env


def test_rays_against_the_camera_and_render_untouched():
    """Pixel-centre rays through ray_test_batch against the depth and segmentation dg_world_render gives for the same state (a
    fixed camera and one riding on a marble), 1e-3 m and 99.5 %; and a render after the ray casts is the render before them."""
    env = _camera_env()
    for rec, name in (('basic_env', 'camera'), ('green_marble', 'eye')):
        cam = env.receptors[rec].addons[name]
        before = {k: v.clone() for k, v in cam.observe().items()}
        body, frame, a, b, zn, zf = R.pixel_rays(env.layout, cam.camera_index)
        hits = env.sim.ray_test_batch(torch.as_tensor(a, dtype=torch.float32, device=DEV), torch.as_tensor(b, dtype=torch.float32, device=DEV), body=body, frame=frame)
        depth = -(zn + hits.frac * (zf - zn))
        want_d, want_s = before['depth'].reshape(depth.shape), before['segmentation_mask'].reshape(depth.shape)
        same = hits.id == want_s
        dev = float((depth - want_d).abs()[same].max())
        print('%s: ids equal %.5f, max |depth| difference %.3g m' % (name, float(same.float().mean()), dev))
        assert float(same.float().mean()) > 0.995 and dev < 1e-3 and float((want_s >= 0).float().mean()) > 0.05
        env._tick += 1
        after = cam.observe()
        for k in before:
            assert torch.equal(before[k], after[k]), (name, k)


def test_lidar_addon_on_the_maze():
    import copy
    import yaml
    import diy_gym_amd.examples  # noqa: F401
    from diy_gym_amd.utils import flatten
    tree = yaml.safe_load(open(os.path.join(ROOT, 'examples', 'r2d2_maze', 'r2d2_maze_lidar.yaml')))
    B = 5
    mk = lambda t, **kw: DIYGym(Configuration.from_dict('r2d2_maze_lidar', copy.deepcopy(t)), num_envs=B, seed=2, **kw)
    gpu, cpu = mk(tree, device=DEV), mk(tree, backend_factory=R.case_backend())
    flat_tree = dict(tree, flatten_observations=True)
    gflat = mk(flat_tree, device=DEV)
    space = gpu.observation_space['r2d2']['lidar']['ranges']
    assert space.shape == (1, 64) and float(space.high.max()) == 10.0 and 'ids' not in gpu.observation_space['r2d2']['lidar'].spaces
    lidar = cpu.models['r2d2'].addons['lidar']
    for act in R.actions(cpu, steps=10):
        for env in (gpu, cpu, gflat):
            env.sim.step(env._all_slots, act.to(env.device)); env._tick += 1
        g, c = gpu.observe(), cpu.observe()
        rg, rc = g['r2d2']['lidar']['ranges'].cpu(), c['r2d2']['lidar']['ranges']
        assert rg.shape == (B, 1, 64)
        ok = torch.from_numpy(~(cpu.sim.last_ray64['margin'] < R.EDGE)).reshape(rg.shape)
        assert float((rg - rc).abs()[ok].max()) < 1e-3
        assert float(rg.min()) >= lidar.range_min and float(rg.max()) <= lidar.range_max
        assert torch.equal(flatten(g, batch_dims=1), gflat.observe())   # dict and flat paths: the same numbers in the same order
    # R2D2 starts at the maze's entrance, OUTSIDE its outer wall (y = -5.5; the maze spans +-5): the half of the fan that faces the
    # maze meets walls, the half that faces away sees nothing within 10 m -- so both a hit and a miss are in every scan (checked on
    # the reference's scan: at least a quarter of the rays hit, at least a quarter miss)
    seen = float((rc < 10.0).float().mean())
    assert 0.25 < seen < 0.75, seen


def test_argument_errors_launch_nothing():
    gpu, _, _ = case('basic_env', 3)
    sim, lib, n = gpu.sim, gpu.sim.lib, 8
    a = torch.zeros((n, 3), device=DEV); b = torch.ones((n, 3), device=DEV)
    scratch = torch.empty((int(lib.dg_world_raycast_scratch_floats(sim.handle)), ), device=DEV)
    assert scratch.numel() >= 3 * 24
    frac = torch.full((3, n), 7.0, device=DEV); ids = torch.full((3, n), 7, dtype=torch.int32, device=DEV)
    pos = torch.full((3, n, 3), 7.0, device=DEV); nrm = torch.full((3, n, 3), 7.0, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def call(body=-1, frame=-1, n_rays=n, skip=-1, scr=scratch, fr=frac):
        return lib.dg_world_raycast(sim.handle, p(sim.state), body, frame, n_rays, p(a), p(b), 0, skip, p(scr), p(fr), p(ids), p(pos), p(nrm), sim._stream())

    nb = gpu.layout.n_bodies
    for kw in (dict(n_rays=0), dict(n_rays=-3), dict(fr=None), dict(scr=None), dict(body=nb), dict(body=-2), dict(body=1, frame=99), dict(frame=0),
               dict(body=1, frame=-2), dict(skip=nb), dict(skip=-2)):
        assert call(**kw) == -4, kw          # DG_ERR_ARG
        assert lib.dg_last_error()
    torch.cuda.synchronize()
    assert bool((frac == 7.0).all()) and bool((ids == 7).all()) and bool((pos == 7.0).all()) and bool((nrm == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((frac <= 1.0).all()) and not bool((ids == 7).all())
    with pytest.raises(ValueError):
        sim.ray_test_batch(a.cpu(), b.cpu())
    with pytest.raises(ValueError):
        sim.ray_test_batch(a[:, :2].contiguous(), b[:, :2].contiguous())
    with pytest.raises(ValueError):
        sim.ray_test_batch(a, b, want=('id', ))
