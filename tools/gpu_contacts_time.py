"""Time of one batched contact query next to the step time of the same scene:

    python tools/gpu_contacts_time.py <scene> <envs>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, from_the_readme, r2d2_maze, ...).  The scene is stepped with
random actions until its contacts exist, then ``env.sim.contact_points`` is timed unfiltered with every output, unfiltered with the
count alone, and filtered to the scene's first model that moves.  Every figure is the mean over timed calls on one stream between
two events (200 queries, 100 steps) after a warm-up."""
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
print('%s x %d envs: step %.4f ms (%s, %d envs per wavefront, %d substeps); max_contacts %d' % (name, B, step_ms, sim.kernel_name, sim.envs_per_wave, L.substeps, L.max_contacts))
every = ('id', 'pos', 'normal', 'distance', 'force') if L.warm_off >= 0 else ('id', 'pos', 'normal', 'distance')
moving = [m for m in env.models.values() if m.uid < L.n_bodies and not (L.body_fixed[m.uid] and L.body_n_links[m.uid] == 0)]
cases = [('every contact, every output', dict(want=every)), ('every contact, count only', dict(want=()))]
if moving:
    cases.append(('contacts of model %r' % moving[0].name, dict(body_a=moving[0].uid, want=every)))
for label, kw in cases:
    ms = timed(lambda i: sim.contact_points(**kw), 20, 200)
    cnt = sim.contact_points(**kw).count.float()
    print('  %-40s %.4f ms   contacts per env: mean %.2f, max %d' % (label, ms, float(cnt.mean()), int(cnt.max())))
env.close()
