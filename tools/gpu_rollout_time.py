"""Time of one forward-dynamics query and of one K-sample, T-step rollout next to the step time of the same scene, next to the same
work done with the older queries -- T rounds of calculate_mass_matrix + calculate_inverse_dynamics + torch.linalg.solve + torch
integration on B x K rows -- and of one mppi_controller tick:

    python tools/gpu_rollout_time.py <scene> <envs> <K> <T>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, ur5_gripper, ...).  The queries run on the scene's first
fixed-base body with joints, at the body's last frame, from every env's current joint state.  The older queries take one row per
env, so their version of the rollout is timed on a world of B x K envs of the same scene (built only for that, and only when B x K
<= 65 536).  Every figure is the mean over timed calls on one stream between two events (100 calls or steps, 20 of the composed
rollout) after a warm-up.  No threshold is attached."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import diy_gym_amd.examples  # noqa: F401
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.controllers import MppiController
from diy_gym_amd.config import Configuration
from diy_gym_amd.utils import flatten, get_bounds_for_space

name, B, K, T = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
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
print('%s x %d envs: step %.4f ms (%s, %d envs per wavefront, %d LDS bytes per workgroup); model %r: %d joints, frame %d; K = %d, T = %d, %d workgroups'
      % (name, B, step_ms, sim.kernel_name, sim.envs_per_wave, sim.lds_bytes, model.name, nv, frame, K, T, sim.rollout_grid(K)))
tau1 = (torch.rand((B, nv), generator=gen) * 2 - 1).to(dev)
tau = (torch.rand((B, K, T, nv), generator=gen) * 2 - 1).to(dev)
print('  calculate_forward_dynamics                         %.4f ms' % timed(lambda i: sim.calculate_forward_dynamics(uid, tau=tau1), 20, 100))
print('  rollout_joint_dynamics, q and qd                   %.4f ms' % timed(lambda i: sim.rollout_joint_dynamics(uid, tau), 20, 100))
print('  rollout_joint_dynamics, qd and pos                 %.4f ms' % timed(lambda i: sim.rollout_joint_dynamics(uid, tau, frame=frame, want=('qd', 'pos')), 20, 100))


def composed_fd(s, q, qd, t):
    M = s.calculate_mass_matrix(uid, q)
    h = s.calculate_inverse_dynamics(uid, q, qd)
    return torch.linalg.solve(M, (t - h).unsqueeze(2)).squeeze(2)


q0, qd0 = (t.clone() for t in sim.joint_states(uid))
print('  mass matrix + inverse dynamics + torch.linalg.solve %.4f ms (one forward dynamics the older way)' % timed(lambda i: composed_fd(sim, q0, qd0, tau1), 20, 100))
if B * K <= 65536:
    wide = DIYGym(paths[0], num_envs=B * K, device='cuda:0').sim   # the older queries take one row per env
    rows = tau.reshape(B * K, T, nv)
    q0w, qd0w = q0.repeat_interleave(K, dim=0), qd0.repeat_interleave(K, dim=0)

    def composed_rollout(i):
        q, qd = q0w.clone(), qd0w.clone()
        for t in range(T):
            qd = qd + L.dt * composed_fd(wide, q, qd, rows[:, t].contiguous())
            q = q + L.dt * qd
        return q

    print('  the rollout the older way, %d rows x %d rounds   %.4f ms' % (B * K, T, timed(composed_rollout, 3, 20)))
if nv >= 3:
    # a hook addon needs no compile(): one can be put on the built scene.  Its reset() switches the body's motors off, so it comes last
    cfg = Configuration.from_dict('mppi', {'addon': 'mppi_controller', 'end_effector': model.robot.joints[frame].name, 'samples': K, 'horizon': T})
    mppi = MppiController(model, cfg)
    env.reset_mask = None
    mppi.reset()
    act = {'linear': torch.zeros((B, 3), device=dev)}
    print('  one mppi_controller tick (inverse dynamics, noise, rollout, cost, softmax, apply_joint_torque)  %.4f ms' % timed(lambda i: mppi.update(act), 20, 100))
