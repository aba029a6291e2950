"""Time of the contact-force queries next to the contact query and the step of the same scene:

    python tools/gpu_contact_forces_time.py <scene> <envs>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, from_the_readme, r2d2_maze, ...).  The scene is stepped with
random actions until its contacts exist, then ``env.sim.contact_points`` (every output), ``env.sim.contact_forces`` (every output,
and the count alone) and ``env.sim.net_contact_forces`` of the scene's first model that moves (the whole body; the whole body and up
to 15 of its links) are timed.  Every figure is the mean over timed calls on one stream between
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
if L.warm_off < 0:
    sys.exit('the scene keeps no contact impulse cache: no forces to report')
moving = [m for m in env.models.values() if m.uid < L.n_bodies and not (L.body_fixed[m.uid] and L.body_n_links[m.uid] == 0)]
cases = [('contact_points, every output', lambda i: sim.contact_points()),
         ('contact_forces, every output', lambda i: sim.contact_forces()),
         ('contact_forces, count only', lambda i: sim.contact_forces(want=()))]
if moving:
    uid = moving[0].uid
    links = [None] + list(range(-1, min(sim._body_n_frames(uid), 14)))
    cases.append(('net_contact_forces of %r, whole body' % moving[0].name, lambda i: sim.net_contact_forces(uid)))
    cases.append(('net_contact_forces of %r, %d selectors' % (moving[0].name, len(links)), lambda i: sim.net_contact_forces(uid, links)))
for label, fn in cases:
    print('  %-50s %.4f ms' % (label, timed(fn, 20, 200)))
cnt = sim.contact_forces(want=()).count.float()
print('  contacts per env: mean %.2f, max %d' % (float(cnt.mean()), int(cnt.max())))
env.close()
