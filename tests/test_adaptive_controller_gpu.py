"""The adaptive_controller addon -- a hook addon written on env.sim.inverse_dynamics_regressor, inertial_parameters, joint_states and
apply_joint_torque -- on the GPU, through the real step: the UR5 of tests/golden/regressor/ur_adaptive.yaml, 8 envs whose link
masses a dynamics_randomizer scaled by about 0.5 to 3, two substeps per step.

From the reset pose at rest the target is set 0.3 x [0.3, -0.4, 0.5, 0.3, -0.3, 0.2] away and the scene runs 480 steps, once with the
estimate frozen (adapt_gain 0: a computed-torque law on the nominal masses) and once adapting (0.3).  Per env the adapting run's final
max |q - q*| must be below HALF the frozen run's, and the frozen run's must be within 25 % of what the fp64 model of the loop
(tests/adaptive_ref.py, recorded by tools/adaptive_fp64_loop.py --record in tests/golden/regressor/adaptive_fp64.json for these very
scales) predicts -- which shows that the comparison is not hiding a broken frozen run.  The model's own errors are 0.025 to 0.049 rad
frozen and 0.008 to 0.018 adapting (still falling at step 480), ratios 0.21 to 0.40; the real step adds link damping and effort
clipping, which the model leaves out.  Measured on an MI355X: the frozen run within 0.1 % of the model in every env, the adapting
run's error 0.21 to 0.40 x the frozen run's -- the model's figures to three digits."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import dynamics_ref as D
from diy_gym_amd import DIYGym
from diy_gym_amd.config import Configuration

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'regressor')
DEV = 'cuda:0'
B, STEPS = 8, 480
REST = [0.3, -1.0, 1.2, -0.5, 0.4, 0.1]
OFFSET = [0.3 * v for v in (0.3, -0.4, 0.5, 0.3, -0.3, 0.2)]


def run(adapt_gain):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_adaptive.yaml')))
    tree['arm']['adaptive'].update(adapt_gain=adapt_gain)
    cfg = Configuration.from_dict('ur_adaptive', tree); cfg.source_dir = GOLDEN
    env = DIYGym(cfg, num_envs=B, device=DEV, seed=1)
    a = env.models['arm'].addons['adaptive']
    scales = D.mass_scales(env, a.uid)
    target = torch.tensor(REST, device=DEV) + torch.tensor(OFFSET, device=DEV)
    zero = {'arm': {'adaptive': {'target': torch.zeros((B, 6), device=DEV)}}}
    q0 = env.sim.joint_states(a.uid)[0].clone()
    assert float((q0 - torch.tensor(REST, device=DEV)).abs().max()) < 1e-6   # the reset pose, at rest
    a.set_target(target)
    for _ in range(STEPS):
        env.step(zero)
    q, qd = env.sim.joint_states(a.uid)
    assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(qd).all()) and bool(torch.isfinite(env.sim.state).all())
    assert torch.equal(a.q_star, target.expand(B, 6))
    return scales, (q - target).abs().amax(dim=1).cpu().numpy().astype(np.float64), a.scale_estimate.cpu().numpy()


def test_adaptation_halves_the_error_of_the_frozen_model_and_the_frozen_run_is_the_models():
    record = json.load(open(os.path.join(GOLDEN, 'adaptive_fp64.json')))
    assert record['steps'] == STEPS
    scales, frozen, s_frozen = run(0.0)
    scales_b, adapting, s_hat = run(0.3)
    assert np.array_equal(scales, scales_b)
    assert scales.min() >= 0.4 and scales.max() <= 3.5 and np.abs(scales - 1.0).max() > 0.5, scales
    assert np.abs(scales - np.array(record['scales'])).max() <= 1e-5 * scales.max()   # the plants the model was run for
    assert (s_frozen == 1.0).all() and np.abs(s_hat - 1.0).max() > 0.1
    predicted = np.array(record['frozen'])
    for e in range(B):
        print('env %d: frozen %.4f (model %.4f, x%.3f), adapting %.4f (model %.4f): ratio %.3f; estimate %s, true %s'
              % (e, frozen[e], predicted[e], frozen[e] / predicted[e], adapting[e], record['adapting'][e], adapting[e] / frozen[e],
                 np.round(s_hat[e].astype(np.float64), 2).tolist(), np.round(scales[e], 2).tolist()))
    assert (np.abs(frozen - predicted) <= 0.25 * predicted).all(), (frozen, predicted)
    assert (adapting < 0.5 * frozen).all(), (adapting, frozen)
