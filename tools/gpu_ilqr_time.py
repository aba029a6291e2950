"""Times of the feedback rollout, the LQ backward pass and the controllers built on them, next to the step time of the same scene:

    python tools/gpu_ilqr_time.py <scene> <envs> <T>

  * one rollout_joint_feedback of 4 alphas over T steps (gains, references and a direction given) beside an open-loop
    rollout_joint_dynamics of 4 samples;
  * one lq_backward_pass of T steps along a trajectory (P = T);
  * the stationary pass of horizon 100 beside lqr_gain in torch (float64) on the same matrices;
  * one ilqr_controller tick (horizon T, one iteration);
  * one linearising lqr_controller tick with ``riccati: torch`` and with ``riccati: kernel``.

<scene> names a config under examples/ or tests/golden/ (ur_high_5, ur_admittance, ur5_gripper, ...).  The queries run on the scene's
first fixed-base body with joints, from every env's current joint state.  Every figure is the mean over timed calls on one stream
between two events after a warm-up.  No threshold is attached."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import diy_gym_amd.examples  # noqa: F401
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.controllers import IlqrController, LqrController, lqr_discretise, lqr_gain
from diy_gym_amd.config import Configuration
from diy_gym_amd.utils import flatten, get_bounds_for_space

name, B, T = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
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
print('%s x %d envs: step %.4f ms (%s, %d envs per wavefront, %d LDS bytes per workgroup); model %r: %d joints; T = %d'
      % (name, B, step_ms, sim.kernel_name, sim.envs_per_wave, sim.lds_bytes, model.name, nv, T))
dt = float(L.dt) * int(L.substeps)
q0, qd0 = (t.clone() for t in sim.joint_states(uid))
tau_g = sim.calculate_inverse_dynamics(uid, q=q0, qd=torch.zeros_like(q0)).clone()
U = tau_g[:, None, :].expand(B, T, nv).contiguous()
nom = sim.rollout_joint_feedback(uid, U, q0=q0, qd0=qd0, dt=dt, joint_damping=True)
qs, qds = torch.cat([q0[:, None], nom.q[:, 0, :-1]], dim=1).contiguous(), torch.cat([qd0[:, None], nom.qd[:, 0, :-1]], dim=1).contiguous()
d = sim.forward_dynamics_derivatives(uid, qs, qds, U, joint_damping=True)
A_q, A_v, Minv = (t.clone() for t in (d.dqdd_dq, d.dqdd_dqd, d.dqdd_dtau))
eye = lambda k, v: torch.diag(torch.tensor(v, dtype=torch.float32, device=dev)) if isinstance(v, list) else v * torch.eye(k, device=dev)
lxx, luu, lxx_T = eye(2 * nv, [10.0] * nv + [0.1] * nv), eye(nv, 1e-4), eye(2 * nv, [1000.0] * nv + [10.0] * nv)
lx = torch.cat([10.0 * (qs - q0[:, None]), 0.1 * qds], dim=2).contiguous()
back = sim.lq_backward_pass(uid, A_q, A_v, Minv, dt, lxx, luu, lxx_T, lx=lx)
gain, k = back.K.clone(), back.k.clone()
alphas = torch.tensor([1.0, 0.5, 0.25, 0.125], device=dev)
tau4 = U[:, None].expand(B, 4, T, nv).contiguous()
print('  rollout_joint_dynamics, 4 samples (open loop)            %.4f ms' % timed(lambda i: sim.rollout_joint_dynamics(uid, tau4, q0, qd0, dt=dt, joint_damping=True), 10, 50))
print('  rollout_joint_feedback, 4 alphas, gains and direction    %.4f ms'
      % timed(lambda i: sim.rollout_joint_feedback(uid, U, gain, qs, qds, k, alphas, q0, qd0, dt=dt, joint_damping=True), 10, 50))
print('  rollout_joint_feedback, 1 sample, torques alone          %.4f ms' % timed(lambda i: sim.rollout_joint_feedback(uid, U, q0=q0, qd0=qd0, dt=dt, joint_damping=True), 10, 50))
print('  lq_backward_pass, T = %-3d along the trajectory           %.4f ms (status max %d)'
      % (T, timed(lambda i: sim.lq_backward_pass(uid, A_q, A_v, Minv, dt, lxx, luu, lxx_T, lx=lx), 10, 50), int(back.status.max())))
Q, R = eye(2 * nv, [1000.0] * nv + [10.0] * nv), eye(nv, 1e-3)
A0, V0, M0 = (t[:, 0].contiguous() for t in (A_q, A_v, Minv))
kernel_ms = timed(lambda i: sim.lq_backward_pass(uid, A0, V0, M0, float(L.dt), Q, R, Q, horizon=100, substeps=int(L.substeps), want=('K', )), 10, 50)


def in_torch(i):
    A, Bm = lqr_discretise(A0.double(), V0.double(), M0.double(), float(L.dt), int(L.substeps))
    return lqr_gain(A, Bm, Q.double(), R.double(), 100).float()


torch_ms = timed(in_torch, 3, 20)
Kk = -sim.lq_backward_pass(uid, A0, V0, M0, float(L.dt), Q, R, Q, horizon=100, substeps=int(L.substeps), want=('K', )).K[:, 0]
Kt = in_torch(0)
print('  stationary pass of horizon 100: lq_backward_pass %.4f ms, lqr_gain in torch %.4f ms (%.1f x); gains differ by %.3g of the largest'
      % (kernel_ms, torch_ms, torch_ms / kernel_ms, float((Kk - Kt).abs().max() / Kt.abs().max())))
# hook addons need no compile(): they can be put on the built scene.  Their reset() switches the body's motors off, so they come last
act = {'target': torch.zeros((B, nv), device=dev)}
ilqr = IlqrController(model, Configuration.from_dict('ilqr', {'addon': 'ilqr_controller', 'horizon': T}))
env.reset_mask = None
ilqr.reset()
print('  one ilqr_controller tick (horizon %d, 1 iteration)        %.4f ms' % (T, timed(lambda i: ilqr.update(act), 5, 50)))
for riccati in ('torch', 'kernel'):
    lqr = LqrController(model, Configuration.from_dict('lqr', {'addon': 'lqr_controller', 'relinearize': 1, 'riccati': riccati}))
    env.reset_mask = None
    lqr.reset()
    print('  one lqr_controller tick, linearising, riccati: %-6s    %.4f ms' % (riccati, timed(lambda i: lqr.update(act), 5, 50)))
