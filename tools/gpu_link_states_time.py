"""Time of the batched link-state query and the base reset next to what they replace and the step of the same scene:

    python tools/gpu_link_states_time.py <scene> <envs> <n>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, from_the_readme, cart_tree, ...).  The scene's first model that
moves is read at n selectors -- its base and its frames in turn, repeated when it has fewer than n -- by ONE
``env.sim.link_states`` call and by the n ``env.sim.frame_state`` calls that call replaces; ``env.sim.reset_base_state`` (pose and
both velocities, every env) is timed on the first model whose base the scene lets move.  A ``link_states`` of n times the base writes
the same rows with next to no arithmetic in front of the stores: what the env-major output layout costs by itself.  Every figure is the mean over timed calls on
one stream between two events (200 queries, 100 steps) after a warm-up; the state is put back before the steps are timed."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import diy_gym_amd.examples  # noqa: F401
from diy_gym_amd import DIYGym
from diy_gym_amd.utils import flatten, get_bounds_for_space

name, B, n = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
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
ring = [None] * 8   # (a scene without controllers takes no actions)
if L.act_dim:
    lo = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, True)), dtype=torch.float32), neginf=-1.0).clamp(-10, 10)
    hi = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, False)), dtype=torch.float32), posinf=1.0).clamp(-10, 10)
    gen = torch.Generator().manual_seed(1)
    ring = [(lo + (hi - lo) * torch.rand((B, lo.numel()), generator=gen)).to(dev) for _ in range(8)]
step = lambda i: sim.step(env._all_slots, ring[i % 8])
for i in range(10):
    step(i)
models = [m for m in env.models.values() if m.uid < L.n_bodies]
moving = [m for m in models if not (L.body_fixed[m.uid] and L.body_n_links[m.uid] == 0)]
if not moving:
    sys.exit('the scene has no body that moves')
model = moving[0]
nf = sim._body_n_frames(model.uid)
frames = ([-1] + list(range(nf))) * n
frames = frames[:n]
print('%s x %d envs (%s, %d envs per wavefront, %d substeps); %r: %d joints, %d frames' %
      (name, B, sim.kernel_name, sim.envs_per_wave, L.substeps, model.name, L.body_n_links[model.uid], nf))
for com in (False, True):
    one = timed(lambda i: sim.link_states(model.uid, frames, com=com), 20, 200)
    many = timed(lambda i: [sim.frame_state(model.uid, f, com=com) for f in frames], 20, 200)
    print('  com=%d  one link_states of %d frames %.4f ms   %d frame_state calls %.4f ms   ratio %.2f' % (com, n, one, n, many, many / one))
# the same 13 n stores per env with next to no arithmetic in front of them: n times the base, whose velocity needs no walk up a chain
base = timed(lambda i: sim.link_states(model.uid, [-1] * n), 20, 200)
print('  one link_states of %d x the base (the stores of the call above, no chain walked) %.4f ms' % (n, base))
movable = [m for m in models if sim.base_is_movable(m.uid)]
if movable:
    m = movable[0]
    saved = sim.state.clone()
    rep = sim.frame_state(m.uid, -1, com=True).clone()
    vel = {} if L.body_fixed[m.uid] else dict(lin_vel=rep[:, 7:10].contiguous(), ang_vel=rep[:, 10:13].contiguous())
    pos, orn = rep[:, 0:3].contiguous(), rep[:, 3:7].contiguous()
    t = timed(lambda i: sim.reset_base_state(m.uid, pos=pos, orn=orn, **vel), 20, 200)
    print('  reset_base_state of %r (pose%s, every env) %.4f ms' % (m.name, '' if L.body_fixed[m.uid] else ' and both velocities', t))
    sim.state.copy_(saved)
else:
    print('  reset_base_state: the scene pins every base to its load pose (no floating base, no respawn addon)')
print('  step %.4f ms' % timed(step, 30, 100))
env.close()
