"""Time of one inverse_dynamics_regressor call at P points per env -- Y alone, and tau + grad alone (what adaptive_controller asks
for) -- next to one calculate_inverse_dynamics call and the eager step of the same scene:

    python tools/gpu_regressor_time.py <scene> <envs> <P>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, ur5_gripper, ...).  The queries run on the scene's first
fixed-base body with joints, at points around every env's current joint state.  calculate_inverse_dynamics takes one row per env
(one point).  Every figure is the mean over 100 timed calls or steps on one stream between two events after a warm-up.  No threshold
is attached."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import diy_gym_amd.examples  # noqa: F401
from diy_gym_amd import DIYGym
from diy_gym_amd.utils import flatten, get_bounds_for_space

name, B, P = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
paths = glob.glob(os.path.join(ROOT, 'examples', '*', name + '.yaml')) + glob.glob(os.path.join(ROOT, 'tests', 'golden', name + '.yaml'))
if not paths:
    sys.exit('no examples/*/%s.yaml or tests/golden/%s.yaml' % (name, name))
env = DIYGym(paths[0], num_envs=B, device='cuda:0')
dev, sim, L = env.device, env.sim, env.layout
lo = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, True)), dtype=torch.float32), neginf=-1.0).clamp(-10, 10)
hi = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, False)), dtype=torch.float32), posinf=1.0).clamp(-10, 10)
gen = torch.Generator().manual_seed(1)
ring = [(lo + (hi - lo) * torch.rand((B, lo.numel()), generator=gen)).to(dev) for _ in range(8)]
models = [m for m in env.models.values() if m.uid < L.n_bodies and L.body_fixed[m.uid] and L.body_n_links[m.uid] >= 1]
if not models:
    sys.exit('%s has no fixed-base body with joints' % name)
model = models[0]
uid, nv = model.uid, L.body_n_links[model.uid]


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


step_ms = timed(lambda i: sim.step(env._all_slots, ring[i % 8]), 30, 100)
print('%s x %d envs: eager step %.4f ms (%s, %d envs per wavefront, %d LDS bytes per workgroup); model %r: %d joints; P = %d, %d workgroups'
      % (name, B, step_ms, sim.kernel_name, sim.envs_per_wave, sim.lds_bytes, model.name, nv, P, sim.rollout_grid(P)))
q0, qd0 = (t.clone() for t in sim.joint_states(uid))
rand = lambda: (torch.rand((B, P, nv), generator=gen) * 2 - 1).to(dev)
q, qd, qdd, qd_ref, s = (q0[:, None, :] + 0.2 * rand()).contiguous(), (qd0[:, None, :] + rand()).contiguous(), 3.0 * rand(), rand(), rand()
theta = sim.inertial_parameters(uid).clone()
y_ms = timed(lambda i: sim.inverse_dynamics_regressor(uid, q, qd, qdd, qd_ref=qd_ref, want=('Y', )), 10, 100)
tg_ms = timed(lambda i: sim.inverse_dynamics_regressor(uid, q, qd, qdd, qd_ref=qd_ref, theta=theta, s=s, want=('tau', 'grad')), 10, 100)
q1, qd1, qdd1 = (t[:, 0].contiguous() for t in (q, qd, qdd))
id_ms = timed(lambda i: sim.calculate_inverse_dynamics(uid, q1, qd1, qdd1), 10, 100)
y_bytes = B * P * 40 * nv * nv
print('  Y alone            %.4f ms  (%d items, %.1f MB of stores: %.1f GB/s)' % (y_ms, B * P, y_bytes / 1e6, y_bytes / y_ms / 1e6))
print('  tau + grad alone   %.4f ms' % tg_ms)
print('  calculate_inverse_dynamics (one point per env)  %.4f ms' % id_ms)
print('  eager step         %.4f ms' % step_ms)
