"""Time of the task-space dynamics query next to the step time of the same scene, next to the same quantities composed from the four
older queries plus torch.linalg, and of one osc_controller tick:

    python tools/gpu_task_space_time.py <scene> <envs>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, ur5_gripper, ...).  The query runs on the scene's first
fixed-base body with joints, at the body's last frame, with six task rows (three when the body has fewer than six joints, one when
fewer than three), at every env's current joint state.  Every figure is the mean over timed calls on one stream between two events
(200 calls of a query or tick, 100 steps) after a warm-up.  No threshold is attached."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import diy_gym_amd.examples  # noqa: F401
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.controllers import OperationalSpaceController
from diy_gym_amd.config import Configuration
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
axes = tuple(range(6 if nv >= 6 else 3 if nv >= 3 else 1))
m = len(axes)


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
acc = (torch.rand((B, m), generator=gen) * 2 - 1).to(dev)
eye = torch.eye(m, device=dev)
zeros = torch.zeros((B, nv), device=dev)


def composed(want_all):
    """The same quantities from joint_states, calculate_jacobian, calculate_inverse_dynamics (twice: h, and Jdot qd is not available
    from the older queries at all -- it is left out), calculate_mass_matrix and batched torch.linalg."""
    q, qd = sim.joint_states(uid)
    jt, jr = sim.calculate_jacobian(uid, frame)
    J = torch.cat([jt, jr], dim=1)[:, :m]
    h = sim.calculate_inverse_dynamics(uid, q, qd, zeros)
    M = sim.calculate_mass_matrix(uid)
    X = torch.cholesky_solve(J.transpose(1, 2), torch.linalg.cholesky(M))
    A = J @ X
    LA = torch.linalg.cholesky(A + 1e-6 * eye)
    f = torch.cholesky_solve(acc.unsqueeze(2), LA)
    tau = (J.transpose(1, 2) @ f).squeeze(2) + h
    return (tau, torch.cholesky_solve(eye.expand(B, m, m), LA)) if want_all else tau


print('%s x %d envs: step %.4f ms (%s, %d envs per wavefront); model %r: %d joints, frame %d, %d task rows'
      % (name, B, step_ms, sim.kernel_name, sim.envs_per_wave, model.name, nv, frame, m))
frame_args = (uid, frame, (0.0, 0.0, 0.0), axes)
print('  task_space_dynamics, every output            %.4f ms' % timed(lambda i: sim.task_space_dynamics(*frame_args, acc=acc), 20, 200))
print('  task_space_dynamics, tau only                %.4f ms' % timed(lambda i: sim.task_space_dynamics(*frame_args, acc=acc, want=('tau', )), 20, 200))
print('  task_space_dynamics, point only              %.4f ms' % timed(lambda i: sim.task_space_dynamics(*frame_args, want=('point', )), 20, 200))
print('  four older queries + torch.linalg, tau+lambda %.4f ms (without Jdot qd, which they cannot give)' % timed(lambda i: composed(True), 20, 200))
print('  four older queries + torch.linalg, tau only   %.4f ms' % timed(lambda i: composed(False), 20, 200))
if m >= 3:
    # a hook addon needs no compile(): one can be put on the built scene.  Its reset() switches the body's motors off and puts the
    # joints at rest, so it comes last
    cfg = Configuration.from_dict('osc', {'addon': 'osc_controller', 'end_effector': model.robot.joints[frame].name, 'use_orientation': m == 6})
    osc = OperationalSpaceController(model, cfg)
    env.reset_mask = None
    osc.reset()
    act = {'linear': torch.zeros((B, 3), device=dev), 'rotation': torch.zeros((B, 3), device=dev)}
    print('  one osc_controller tick (two queries, torch arithmetic, apply_joint_torque)  %.4f ms' % timed(lambda i: osc.update(act), 20, 200))
