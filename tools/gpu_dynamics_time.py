"""Time of each batched dynamics query next to the step time of the same scene:

    python tools/gpu_dynamics_time.py <scene> <envs>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, ur5_gripper, ...).  The queries run on the scene's first
fixed-base body with joints, at every env's current joint state (q = None) and again at explicit per-env q / qd / qdd; the
Jacobian is taken at the body's last frame.  Every figure is the mean over timed calls on one stream between two events (200
calls of a query, 100 steps) after a warm-up."""
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
uid, nv, frame = model.uid, L.body_n_links[model.uid], len(model.robot.joints) - 1


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
q, qd = (t.clone() for t in sim.joint_states(uid))
qdd = torch.rand((B, nv), generator=gen).to(dev)
tau = torch.zeros((B, nv), device=dev)
rows = [('joint_states', lambda i: sim.joint_states(uid), None),
        ('calculate_jacobian', lambda i: sim.calculate_jacobian(uid, frame), lambda i: sim.calculate_jacobian(uid, frame, (0.0, 0.0, 0.0), q)),
        ('calculate_inverse_dynamics', lambda i: sim.calculate_inverse_dynamics(uid), lambda i: sim.calculate_inverse_dynamics(uid, q, qd, qdd)),
        ('calculate_mass_matrix', lambda i: sim.calculate_mass_matrix(uid), lambda i: sim.calculate_mass_matrix(uid, q)),
        ('apply_joint_torque', None, lambda i: sim.apply_joint_torque(uid, tau))]
print('%s x %d envs: step %.4f ms (%s, %d envs per wavefront); queries on model %r: %d joints, Jacobian at frame %d'
      % (name, B, step_ms, sim.kernel_name, sim.envs_per_wave, model.name, nv, frame))
for label, current, explicit in rows:
    a = '%.4f' % timed(current, 20, 200) if current else '     -'
    b = '%.4f' % timed(explicit, 20, 200) if explicit else '     -'
    print('  %-28s current state %s ms   explicit inputs %s ms' % (label, a, b))
