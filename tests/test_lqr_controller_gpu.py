"""The lqr_controller addon -- a hook addon written on env.sim.forward_dynamics_derivatives, calculate_inverse_dynamics, joint_states
and apply_joint_torque -- on the GPU, through the real step: the UR5 of tests/golden/derivs/ur_lqr.yaml, 3 envs, two substeps per
step, the addon's defaults.

Hold: q* = [0.3, -1.0, 1.2, -0.5, 0.4, 0.1], start q* + U(+-0.05) (seed 3; env 0 starts where tests/test_ddq_ref.py's fp64 loop does)
at rest, 100 steps: every env's largest joint error ends below 0.1 x its start (the fp64 reference of tests/lqr_ref.py ends at
0.018 x).  The test can fail: with torque_weight 1e6 the gain vanishes and the arm does not meet the condition, and the same arm with
no controller and its motors off (tests/golden/derivs/ur_free.yaml) leaves the target."""
import os

import numpy as np
import pytest
import torch
import yaml

from diy_gym_amd import DIYGym
from diy_gym_amd.config import Configuration

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'derivs')
DEV = 'cuda:0'
B = 3
Q_STAR = [0.3, -1.0, 1.2, -0.5, 0.4, 0.1]


def make(drop=(), **edit):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_lqr.yaml')))
    tree['arm']['lqr'].update(edit)
    for key in drop:
        del tree['arm']['lqr'][key]
    cfg = Configuration.from_dict('ur_lqr', tree); cfg.source_dir = GOLDEN
    env = DIYGym(cfg, num_envs=B, device=DEV, seed=1)
    return env, env.models['arm'].addons['lqr']


def start():
    q_star = torch.tensor(Q_STAR, device=DEV)
    q0 = q_star + torch.as_tensor(np.random.default_rng(3).uniform(-0.05, 0.05, (B, 6)).astype(np.float32), device=DEV)
    return q_star, q0


def zero():
    return {'arm': {'lqr': {'target': torch.zeros((B, 6), device=DEV)}}}


def run(env, uid, q0, action, steps=100):
    """Largest joint error against Q_STAR after ``steps`` steps from q0 at rest, per env; every tensor on the way finite."""
    sim = env.sim
    sim.reset_joint_state(uid, q0.contiguous(), torch.zeros_like(q0))
    q_star = torch.tensor(Q_STAR, device=DEV)
    for _ in range(steps):
        env.step(action())
        q, qd = sim.joint_states(uid)
        assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(qd).all())
    assert bool(torch.isfinite(env.sim.obs).all()) and bool(torch.isfinite(env.sim.state).all())   # every observation, the whole state
    return (sim.joint_states(uid)[0] - q_star).abs().amax(dim=1)


def test_it_holds_the_target_and_a_vanishing_gain_does_not():
    q_star, q0 = start()
    e0 = (q0 - q_star).abs().amax(dim=1)
    env, a = make()
    assert env.layout.substeps == 2
    end = run(env, a.uid, q0, zero)
    assert torch.equal(a.q_star, q_star.expand(B, 6))   # zero actions leave the target where it was
    assert bool(torch.isfinite(a.gain).all()) and float(a.gain.abs().max()) > 1.0
    print('lqr hold: largest joint error ends at %s x its start' % (end / e0).tolist())
    assert bool((end < 0.1 * e0).all())
    # torque_weight 1e6: torque costs more than any error is worth, the gain vanishes, gravity compensation alone does not hold
    weak, w = make(torque_weight=1e6)
    end_weak = run(weak, w.uid, q0, zero)
    print('torque_weight 1e6: %s x' % (end_weak / e0).tolist())
    assert float(w.gain.abs().max()) < 1.0
    assert not bool((end_weak < 0.1 * e0).any())
    # ... and with no controller and the motors off the arm falls away
    free = DIYGym(os.path.join(GOLDEN, 'ur_free.yaml'), num_envs=B, device=DEV, seed=1)
    cfg = free.sim.motor_cfg(); cfg[:, 2] = 0.0; free.sim.set_motor_cfg(cfg)
    end_free = run(free, free.models['arm'].uid, q0, dict, steps=50)
    assert bool((end_free > e0).all())


def test_set_target_on_a_mask_moves_only_those_envs():
    env, a = make()
    q_star, q0 = start()
    env.step(zero())
    moved = q_star + 0.2
    a.set_target(moved, mask=[False, True, False])
    assert torch.equal(a.q_star[0], q_star) and torch.equal(a.q_star[2], q_star) and torch.equal(a.q_star[1], moved)
    for _ in range(100):
        env.step(zero())
    q = env.sim.joint_states(a.uid)[0]
    # the others never left their target (the hold condition's 0.1 x 0.05 rad); the masked env went to its own: it ends nearer the new
    # target than the old one (0.2 rad away on every joint, the torques clipped on the way: no rate is asserted)
    assert float((q[0] - q_star).abs().max()) < 0.005 and float((q[2] - q_star).abs().max()) < 0.005
    assert float((q[1] - moved).abs().max()) < float((q[1] - q_star).abs().max())
    # the action is ADDED to the target
    step = torch.full((B, 6), 0.01, device=DEV)
    env.step({'arm': {'lqr': {'target': step}}})
    assert torch.allclose(a.q_star[0], q_star + 0.01, atol=1e-6) and torch.allclose(a.q_star[1], moved + 0.01, atol=1e-6)


def test_without_a_target_it_takes_the_pose_the_reset_leaves():
    """No `target` key: q* is the pose the reset LEAVES -- the joint_controller's rest_position -- read on the first tick after the
    reset (a hook's reset() runs before the scene's reset ops), after construction and after a masked reset, for the envs that reset
    only."""
    env, a = make(drop=('target', ))
    rest = torch.tensor(Q_STAR, device=DEV)
    assert a.target is None
    env.step(zero())
    assert torch.allclose(a.q_star, rest.expand(B, 6), atol=1e-6)   # not the world's initial pose
    assert float(rest.abs().max()) > 0.1
    for _ in range(20):
        env.step(zero())
    assert float((env.sim.joint_states(a.uid)[0] - rest).abs().max()) < 0.005   # ... and it holds it
    # move every target away, let the arms follow, then reset env 1 only: its target goes back to the rest pose, the others keep theirs
    away = rest + 0.1
    a.set_target(away)
    for _ in range(30):
        env.step(zero())
    assert float((env.sim.joint_states(a.uid)[0] - rest).abs().max()) > 0.02   # the pose before the reset is not the rest pose
    env.reset(torch.tensor([False, True, False], device=DEV))
    env.step(zero())
    assert torch.allclose(a.q_star[1], rest, atol=1e-6) and torch.equal(a.q_star[0], away) and torch.equal(a.q_star[2], away)
