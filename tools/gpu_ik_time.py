"""Time of one batched inverse-kinematics query next to the step time of the same scene:

    python tools/gpu_ik_time.py <scene> <envs>

<scene> names a config under examples/ or tests/golden/ (ur_high_5, from_the_readme, ...).  The query runs on the scene's first
fixed-base body with joints, towards the current pose of the body's last frame (the end effector of the scene's ik_controller
where there is one) displaced by a centimetre, from every env's current joint state: position only and with the orientation, with
and without the four null-space lists.  The world's own engine parameters apply (20 iterations, early exit on the residual), so
the figure is what a Python controller pays per step; the line after it is the same query with the early exit switched off
(``ik_residual`` 0: every iteration runs).  Every figure is the mean over timed calls on one stream between two events (200
queries, 100 steps) after a warm-up."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
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


def measure(engine, with_step):
    env = DIYGym(paths[0], num_envs=B, device='cuda:0', engine=engine)
    dev, sim, L = env.device, env.sim, env.layout
    models = [m for m in env.models.values() if m.uid < L.n_bodies and L.body_fixed[m.uid] and L.body_n_links[m.uid] >= 1]
    if not models:
        sys.exit('%s has no fixed-base body with joints' % name)
    model = models[0]
    uid, nv, frame = model.uid, L.body_n_links[model.uid], len(model.robot.joints) - 1
    for addon in model.addons.values():
        frame = getattr(addon, 'end_effector_joint_id', frame)
    if with_step:
        lo = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, True)), dtype=torch.float32), neginf=-1.0).clamp(-10, 10)
        hi = torch.nan_to_num(torch.as_tensor(flatten(get_bounds_for_space(env.action_space, False)), dtype=torch.float32), posinf=1.0).clamp(-10, 10)
        gen = torch.Generator().manual_seed(1)
        ring = [(lo + (hi - lo) * torch.rand((B, lo.numel()), generator=gen)).to(dev) for _ in range(8)]
        step_ms = timed(lambda i: sim.step(env._all_slots, ring[i % 8]), 30, 100)
        print('%s x %d envs: step %.4f ms (%s, %d envs per wavefront); query on model %r: %d joints, frame %d, %d iterations at most'
              % (name, B, step_ms, sim.kernel_name, sim.envs_per_wave, model.name, nv, frame, env.builder.params['ik_iterations']))
    pose = sim.frame_state(uid, frame, com=True)
    pos, orn = (pose[:, 0:3] + 0.01).contiguous(), pose[:, 3:7].contiguous()
    lower = [j.lower if j.lower <= j.upper else -np.pi for j in model.robot.joints if j.q_index > -1]
    upper = [j.upper if j.lower <= j.upper else np.pi for j in model.robot.joints if j.q_index > -1]
    if len(lower) != nv:   # (a body with merged child models: no limits at hand for the children's joints)
        lower, upper = [-np.pi] * nv, [np.pi] * nv
    lists = dict(lower=lower, upper=upper, ranges=np.subtract(upper, lower).tolist(), rest=sim.joint_states(uid)[0][0].tolist())
    for label, o, kw in (('position', None, {}), ('position + orientation', orn, {}), ('position, lists', None, lists), ('position + orientation, lists', orn, lists)):
        ms = timed(lambda i: sim.calculate_inverse_kinematics(uid, frame, pos, o, **kw), 20, 200)
        iters = sim.calculate_inverse_kinematics(uid, frame, pos, o, return_iters=True, **kw)[1].float()
        print('  %-32s %.4f ms   iterations per env: mean %.1f, max %d' % (label, ms, float(iters.mean()), int(iters.max())))
    env.close()


measure(None, True)
print('with ik_residual = 0 (no early exit):')
measure({'ik_residual': 0.0}, False)
