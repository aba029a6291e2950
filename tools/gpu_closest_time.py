"""Time of one batched closest-points query next to the step time of the same scene:

    python tools/gpu_closest_time.py <scene> <envs>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, from_the_readme, contacts_arms, ...).  The scene is stepped with
random actions, then ``env.sim.closest_points`` is timed for the scene's first model that moves against every other body: every
output at 0.1 m and at 1 m, and the nearest pair alone (``max_points=0``, what the ``proximity_sensor`` addon asks) at 0.5 m.  Every
figure is the mean over timed calls on one stream between two events (200 queries, 100 steps) after a warm-up."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import diy_gym_amd.examples  # noqa: F401
from diy_gym_amd import DIYGym
from diy_gym_amd.utils import flatten, get_bounds_for_space

name, B = sys.argv[1], int(sys.argv[2])
paths = glob.glob(os.path.join(ROOT, 'examples', '*', name + '.yaml')) + glob.glob(os.path.join(ROOT, 'tests', 'golden', name + '.yaml'))
if not paths:
    sys.exit('no examples/*/%s.yaml or tests/golden/%s.yaml' % (name, name))


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


env = DIYGym(paths[0], num_envs=B, device='cuda:0')
dev, sim, L = env.device, env.sim, env.layout
lo = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, True)), dtype=torch.float32), neginf=-1.0).clamp(-10, 10)
hi = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, False)), dtype=torch.float32), posinf=1.0).clamp(-10, 10)
gen = torch.Generator().manual_seed(1)
ring = [(lo + (hi - lo) * torch.rand((B, lo.numel()), generator=gen)).to(dev) for _ in range(8)]
step_ms = timed(lambda i: sim.step(env._all_slots, ring[i % 8]), 30, 100)
print('%s x %d envs: step %.4f ms (%s, %d envs per wavefront, %d substeps)' % (name, B, step_ms, sim.kernel_name, sim.envs_per_wave, L.substeps))
moving = [m for m in env.models.values() if m.uid < L.n_bodies and not (L.body_fixed[m.uid] and L.body_n_links[m.uid] == 0)]
if not moving:
    sys.exit('the scene has no model that moves')
uid = moving[0].uid
cases = [('within 0.1 m, every output', dict(distance=0.1)), ('within 1 m, every output', dict(distance=1.0)),
         ('nearest pair alone within 0.5 m', dict(distance=0.5, max_points=0, want=('nearest', )))]
print('  model %r against every other body' % moving[0].name)
for label, kw in cases:
    ms = timed(lambda i: sim.closest_points(uid, **kw), 20, 200)
    cp = sim.closest_points(uid, **kw)
    cnt = cp.count.float()
    print('  %-40s %.4f ms   pairs per env: mean %.2f, max %d%s' % (label, ms, float(cnt.mean()), int(cnt.max()),
                                                                  '' if cp.id_a is None else ' (K = %d)' % cp.id_a.shape[1]))
env.close()
