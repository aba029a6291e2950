"""Time of one forward_dynamics_derivatives call at P points per env next to the step time of the same scene, next to one
calculate_forward_dynamics call, next to the older way to the same three matrices -- the 4 nv forward-dynamics launches of a central
difference in q and qd (2 nv each) plus the nv launches that give M^-1 column by column are not counted: only the 4 nv -- and of one
lqr_controller tick with and without its linearisation:

    python tools/gpu_dynderiv_time.py <scene> <envs> <P>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, ur5_gripper, ...).  The queries run on the scene's first
fixed-base body with joints, from every env's current joint state.  The older queries take one row per env, so the central
difference is timed on a world of B x P envs of the same scene (built only for that, and only when B x P <= 65 536).  Every figure is
the mean over timed calls on one stream between two events (100 calls or steps, 20 of the central difference) after a warm-up.  No
threshold is attached."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import diy_gym_amd.examples  # noqa: F401
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.controllers import LqrController
from diy_gym_amd.config import Configuration
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
print('%s x %d envs: step %.4f ms (%s, %d envs per wavefront, %d LDS bytes per workgroup); model %r: %d joints; P = %d, %d workgroups'
      % (name, B, step_ms, sim.kernel_name, sim.envs_per_wave, sim.lds_bytes, model.name, nv, P, sim.rollout_grid(P)))
q0, qd0 = (t.clone() for t in sim.joint_states(uid))
q = (q0[:, None, :] + 0.2 * (torch.rand((B, P, nv), generator=gen) * 2 - 1).to(dev)).contiguous()
qd = (torch.rand((B, P, nv), generator=gen) * 2 - 1).to(dev)
tau = (torch.rand((B, P, nv), generator=gen) * 2 - 1).to(dev)
print('  calculate_forward_dynamics (one point per env)      %.4f ms' % timed(lambda i: sim.calculate_forward_dynamics(uid, q0, qd0, tau[:, 0].contiguous()), 20, 100))
every = ('qdd', 'dqdd_dq', 'dqdd_dqd', 'dqdd_dtau', 'dtau_dq', 'dtau_dqd', 'singular')
for label, want in (('dqdd_dq, dqdd_dqd, dqdd_dtau', ('dqdd_dq', 'dqdd_dqd', 'dqdd_dtau')), ('every field', every), ('dqdd_dtau alone', ('dqdd_dtau', )),
                    ('dtau_dq, dtau_dqd', ('dtau_dq', 'dtau_dqd'))):
    print('  forward_dynamics_derivatives, %-28s %.4f ms' % (label, timed(lambda i: sim.forward_dynamics_derivatives(uid, q, qd, tau, joint_damping=True, want=want), 20, 100)))
f = sim.forward_dynamics_fn(uid, joint_damping=True)
leaves = [t.clone().requires_grad_(True) for t in (q, qd, tau)]


def autograd(i):
    for t in leaves:
        t.grad = None
    f(*leaves).sum().backward()


print('  forward_dynamics_fn forward + backward              %.4f ms' % timed(autograd, 20, 100))
if B * P <= 65536:
    wide = DIYGym(paths[0], num_envs=B * P, device='cuda:0').sim   # the older queries take one row per env
    qw, qdw, tw = (t.reshape(B * P, nv).contiguous() for t in (q, qd, tau))
    eye = torch.eye(nv, device=dev)

    def central(i):
        cols_q, cols_v = [], []
        for j in range(nv):
            e = eye[j]
            cols_q.append((wide.calculate_forward_dynamics(uid, qw + 1e-3 * e, qdw, tw, joint_damping=True).clone()
                           - wide.calculate_forward_dynamics(uid, qw - 1e-3 * e, qdw, tw, joint_damping=True)) / 2e-3)
            cols_v.append((wide.calculate_forward_dynamics(uid, qw, qdw + 1e-3 * e, tw, joint_damping=True).clone()
                           - wide.calculate_forward_dynamics(uid, qw, qdw - 1e-3 * e, tw, joint_damping=True)) / 2e-3)
        return torch.stack(cols_q, dim=2), torch.stack(cols_v, dim=2)

    print('  the older way: %d forward-dynamics launches of a central difference on %d rows  %.4f ms (dqdd_dq and dqdd_dqd only, and in fp32 too noisy to use)'
          % (4 * nv, B * P, timed(central, 3, 20)))
# a hook addon needs no compile(): one can be put on the built scene.  Its reset() switches the body's motors off, so it comes last
for relin, label in ((1, 'linearising every tick'), (10 ** 9, 'between linearisations')):
    lqr = LqrController(model, Configuration.from_dict('lqr', {'addon': 'lqr_controller', 'relinearize': relin}))
    env.reset_mask = None
    lqr.reset()
    act = {'target': torch.zeros((B, nv), device=dev)}
    print('  one lqr_controller tick, %-24s %.4f ms' % (label, timed(lambda i: lqr.update(act), 5, 50)))
