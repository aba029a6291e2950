"""Time of one batched ray cast next to the step time of the same scene:

    python tools/gpu_raycast_time.py <scene> <envs> <rays>

<scene> names a config under examples/ (r2d2_maze_lidar, from_the_readme, ...).  The rays are one 360 degree fan of <rays> rays
from 0.05 to 10 m: the rays of the scene's first `lidar` addon when it has one and <rays> is its ray count (else a fan
through its mounting transform over its range; the model itself skipped either way), else fixed in the world 1 m above the origin and tilted 20 degrees down.  Both figures are means over timed
calls on one stream between two events (200 ray casts, 100 steps) after a warm-up; want = frac + id, what a lidar reads."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import diy_gym_amd.examples  # noqa: F401
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.sensors import Lidar
from diy_gym_amd.scene import K
from diy_gym_amd.utils import flatten, get_bounds_for_space

name, B, N = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
paths = glob.glob(os.path.join(ROOT, 'examples', '*', name + '.yaml'))
if not paths:
    sys.exit('no examples/*/%s.yaml' % name)
env = DIYGym(paths[0], num_envs=B, device='cuda:0')
dev = env.device
lo = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, True)), dtype=torch.float32), neginf=-1.0).clamp(-10, 10)
hi = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, False)), dtype=torch.float32), posinf=1.0).clamp(-10, 10)
gen = torch.Generator().manual_seed(1)
ring = [(lo + (hi - lo) * torch.rand((B, lo.numel()), generator=gen)).to(dev) for _ in range(8)]

lidars = [a for r in env.receptors.values() for a in r.addons.values() if isinstance(a, Lidar)]
az = -np.pi + 2 * np.pi * np.arange(N) / N
if lidars:
    lid = lidars[0]
    if N == lid.num_rays * lid.num_rings:   # the addon's own rays
        a, b = lid.ray_from, lid.ray_to
    else:                                   # a fan of N rays through the addon's mounting transform
        T = lid.T_parent_sensor
        d = np.stack([np.cos(az), np.sin(az), np.zeros(N)], -1)
        a, b = T.p + (d * lid.range_min) @ T.R.T, T.p + (d * lid.range_max) @ T.R.T
    kw = dict(body=lid.uid, frame=lid.frame_id, skip_body=lid.uid if lid.ignore_parent else -1)
    where = 'frame %d of model uid %d' % (lid.frame_id, lid.uid)
else:
    el = np.radians(-20.0)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.full(N, np.sin(el))], -1)
    p = np.array([0.0, 0.0, 1.0])
    a, b, kw, where = p + d * 0.05, p + d * 10.0, {}, 'the world at (0, 0, 1), 20 degrees down'
a, b = torch.as_tensor(a, dtype=torch.float32, device=dev), torch.as_tensor(b, dtype=torch.float32, device=dev)


def timed(fn, warm, count):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(count):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / count


step_ms = timed(lambda i: env.sim.step(env._all_slots, ring[i % 8]), 30, 100)
ray_ms = timed(lambda i: env.sim.ray_test_batch(a, b, want=('frac', 'id'), **kw), 20, 200)
hits = env.sim.ray_test_batch(a, b, want=('frac', 'id'), **kw)
print('%s x %d envs: step %.4f ms (%s); ray cast of %d rays in %s: %.4f ms per call (pose pass + raycast_kernel), %.1f %% of the rays hit, %d shapes'
      % (name, B, step_ms, env.sim.kernel_name, N, where, ray_ms, 100.0 * float((hits.id >= 0).float().mean()), int(env.layout.I[K.H_N_SHAPES])))
