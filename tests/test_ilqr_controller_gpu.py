"""The ilqr_controller addon -- a hook addon written on env.sim.rollout_joint_feedback, forward_dynamics_derivatives, lq_backward_pass,
calculate_inverse_dynamics, joint_states and apply_joint_torque -- on the GPU, through the real step: the UR5 of
tests/golden/ilqr/ur_ilqr.yaml, 3 envs, two substeps per step, the addon's defaults (horizon 32, one iteration per tick).

Reach: q* = [0.3, -1.0, 1.2, -0.5, 0.4, 0.1], env 0 started q* + [0.3, -0.2, 0.25, 0.2, -0.3, 0.2], env 1 at half and env 2 at minus a
quarter of that offset, at rest, 120 ticks: every env's largest joint error ends below 0.1 x its start.  The same loop in fp64 with
tests/fd_ref.py as plant (tools/ilqr_fp64_loop.py: two substeps of 1 / 480 with the torque held, clamp at the URDF's 150 / 28 N m) has
env 0 at 1.13 x its start at tick 30, 0.49 x at 60, 0.097 x at 90, 0.021 x at 110 and 0.038 x at 120; 0.1 x is the margin the lqr test
takes over its own fp64 figure.  The test can fail: with torque_weight 1e6 the arm must NOT arrive.  The same seed gives the same
torques in bits.

lqr_controller with ``riccati: kernel`` (tests/golden/derivs/ur_lqr.yaml): its gains agree with the ``torch`` gains of the same tick to
the backward pass's asserted tolerance (tests/test_ilqr_gpu.py), and the closed loop passes tests/test_lqr_controller_gpu.py's
criterion: 100 steps from q* + U(+-0.05), every env ends below 0.1 x its start."""
import os

import numpy as np
import pytest
import torch
import yaml

import test_ilqr_gpu as TI
import test_lqr_controller_gpu as TL
from diy_gym_amd import DIYGym
from diy_gym_amd.config import Configuration

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ilqr')
DEV = 'cuda:0'
B = 3
Q_STAR = [0.3, -1.0, 1.2, -0.5, 0.4, 0.1]
OFFSET = [0.3, -0.2, 0.25, 0.2, -0.3, 0.2]


def make(**edit):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_ilqr.yaml')))
    tree['arm']['ilqr'].update(edit)
    cfg = Configuration.from_dict('ur_ilqr', tree); cfg.source_dir = GOLDEN
    env = DIYGym(cfg, num_envs=B, device=DEV, seed=1)
    return env, env.models['arm'].addons['ilqr']


def start():
    q_star = torch.tensor(Q_STAR, device=DEV)
    return q_star, q_star + torch.tensor([1.0, 0.5, -0.25], device=DEV)[:, None] * torch.tensor(OFFSET, device=DEV)


def zero():
    return {'arm': {'ilqr': {'target': torch.zeros((B, 6), device=DEV)}}}


def run(env, a, q0, ticks=120, marks=()):
    """Largest joint error against Q_STAR per env after ``ticks`` (and at ``marks``), every tensor on the way finite; and the torques
    applied, per tick."""
    sim, uid = env.sim, a.uid
    sim.reset_joint_state(uid, q0.contiguous(), torch.zeros_like(q0))
    q_star = torch.tensor(Q_STAR, device=DEV)
    seen, torques = {}, []
    for tick in range(1, ticks + 1):
        env.step(zero())
        torques.append(a.torque.clone())
        q, qd = sim.joint_states(uid)
        assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(qd).all()) and bool(torch.isfinite(a.U).all())
        if tick in marks:
            seen[tick] = (q - q_star).abs().amax(dim=1)
    assert bool(torch.isfinite(env.sim.obs).all()) and bool(torch.isfinite(env.sim.state).all())
    return (sim.joint_states(uid)[0] - q_star).abs().amax(dim=1), seen, torch.stack(torques)


def test_it_reaches_the_target_and_a_vanishing_gain_does_not():
    q_star, q0 = start()
    e0 = (q0 - q_star).abs().amax(dim=1)
    env, a = make()
    assert env.layout.substeps == 2 and a.horizon == 32 and a.iterations == 1
    end, seen, _ = run(env, a, q0, marks=(30, 60, 90, 110))
    assert torch.equal(a.q_star, q_star.expand(B, 6))   # zero actions leave the target where it was
    print('ilqr reach: largest joint error / its start: %s, end %s; mu %s' % ({k: [round(x, 4) for x in (v / e0).tolist()] for k, v in seen.items()}, (end / e0).tolist(),
                                                                              a.mu.tolist()))
    assert bool((end < 0.1 * e0).all()), (end / e0).tolist()
    # torque_weight 1e6: torque costs more than any error is worth, the plan stays at gravity compensation and the arm does not arrive
    weak, w = make(torque_weight=1e6)
    end_weak, _, _ = run(weak, w, q0)
    print('torque_weight 1e6: %s x' % (end_weak / e0).tolist())
    assert not bool((end_weak < 0.1 * e0).any())


def test_the_same_seed_gives_the_same_torques_in_bits():
    _, q0 = start()
    runs = []
    for _ in range(2):
        env, a = make()
        _, _, torques = run(env, a, q0, ticks=12)
        runs.append((torques, a.U.clone(), env.sim.joint_states(a.uid)[0].clone()))
    assert float(runs[0][0].abs().max()) > 1.0 and all(torch.equal(x, y) for x, y in zip(*runs))


def test_lqr_controller_with_the_kernels_gains():
    q_star, q0 = TL.start()
    e0 = (q0 - q_star).abs().amax(dim=1)
    env, a = TL.make(riccati='kernel')
    ref, r = TL.make()
    assert a.riccati == 'kernel' and r.riccati == 'torch'
    env.step(TL.zero()); ref.step(TL.zero())   # the linearising tick of both, at the same target
    scale = float(r.gain.abs().amax())
    fig = float((a.gain.double() - r.gain.double()).abs().amax(dim=(1, 2)).max()) / scale
    print('lqr gains, kernel against torch: %.3g of the largest gain %.4g' % (fig, scale))
    assert scale > 10 and fig < TI.BOUND_LQ['K']
    end = TL.run(env, a.uid, q0, TL.zero)
    print('lqr hold with riccati: kernel: %s x' % (end / e0).tolist())
    assert bool((end < 0.1 * e0).all())
