"""The reference's admittance controller written as a Python hook addon on env.sim's dynamics queries (tests/user_controllers.py)
against the compiled DG_OP_ADMITTANCE: tests/golden/ur_admittance.yaml built twice, driven by the same seeded wrench actions.

The two are not the same bits: the compiled op sums J^T F, the gravity term (link by link over each joint's subtree) and the PD
term in another order than Newton-Euler + three torch kernels.  Error measure as tests/test_dynamics_queries_gpu.py: per env,
max |hook - compiled| over the joints divided by that env's largest |compiled| entry.  Bounds: 8 x the largest figure measured
on an MI355X over both batch sizes (DESIGN.md "Dynamics queries"); neither may exceed 1e-4.
"""
import os

import numpy as np
import pytest
import torch
import yaml

from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.config import Configuration
from diy_gym_amd.scene import K
from user_controllers import PyAdmittanceController

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, 'tests', 'golden', 'ur_admittance.yaml')
DEV = 'cuda:0'
# measured maxima (MI355X, 3 and 70 envs): torque after the first update 7.94e-8, joint positions after 20 steps 9.91e-8
BOUND_TORQUE, BOUND_Q = 8 * 7.94e-8, 8 * 9.91e-8
assert max(BOUND_TORQUE, BOUND_Q) < 1e-4


def pair(B):
    """(compiled, hooked): the scene with the compiled admittance_controller and with the Python class under that name."""
    def make(cls):
        registry = AddonFactory.get().addons
        saved = registry['admittance_controller']
        if cls is not None:
            AddonFactory.register_addon('admittance_controller', cls)
        try:
            return DIYGym(Configuration.from_dict('ur_admittance', yaml.safe_load(open(SCENE))), num_envs=B, device=DEV, seed=2)
        finally:
            registry['admittance_controller'] = saved
    compiled, hooked = make(None), make(PyAdmittanceController)
    assert not compiled._hook_addons and len(hooked._hook_addons) == 1 and compiled.layout.state_dim == hooked.layout.state_dim
    assert (compiled.sim.motor_cfg() == hooked.sim.motor_cfg()).all()   # the velocity motors: switched off on both sides
    return compiled, hooked


def actions(B, steps):
    gen = torch.Generator().manual_seed(9)
    return [{'arm': {'wrench': {'force': ((torch.rand((B, 3), generator=gen) * 2 - 1) * 5).to(DEV), 'torque': (torch.rand((B, 3), generator=gen) * 2 - 1).to(DEV)}}}
            for _ in range(steps)]


def figure(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float((np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max())


def columns(env, field):
    L = env.layout
    return [L.link_state_off[L.body_first_link[0] + i] + field for i in range(L.body_n_links[0])]


@pytest.mark.parametrize('B', [3, 70])
def test_python_admittance_controller_applies_the_compiled_ops_torques(B, monkeypatch):
    monkeypatch.setenv('DG_DEBUG_KEEP_EXT', '1')   # the step leaves DG_LS_TORQUE as the update left it
    compiled, hooked = pair(B)
    assert (compiled.sim.get_state() == hooked.sim.get_state()).all()   # the same reset: joints at rest, one hot-start step
    act = actions(B, 1)[0]
    compiled.step(act); hooked.step(act)
    tc, th = (e.sim.get_state()[:, columns(e, K.LS_TORQUE)] for e in (compiled, hooked))
    assert np.abs(tc).max() > 1.0   # (gravity compensation of a UR5: tens of N m)
    err = figure(th, tc)
    print('x%d: torque after the first update, hook against compiled: %.3g' % (B, err))
    assert err < BOUND_TORQUE


@pytest.mark.parametrize('B', [3, 70])
def test_python_admittance_controller_follows_the_compiled_op_for_20_steps(B):
    compiled, hooked = pair(B)
    for act in actions(B, 20):
        compiled.step(act); hooked.step(act)
    qc, qh = (e.sim.get_state()[:, columns(e, K.LS_Q)] for e in (compiled, hooked))
    rest = np.array([0.3, -1.0, 1.2, -0.5, 0.4, 0.1])
    assert np.abs(qc - rest).max() > 1e-3   # (the arm did move under the wrenches)
    err = figure(qh, qc)
    print('x%d: joint positions after 20 steps, hook against compiled: %.3g' % (B, err))
    assert err < BOUND_Q
    assert not (compiled.sim.get_state()[:, columns(compiled, K.LS_TORQUE)] != 0).any() and not (hooked.sim.get_state()[:, columns(hooked, K.LS_TORQUE)] != 0).any()
