"""The reference's inverse-kinematics controller written as a Python hook addon on env.sim's position-level calls
(tests/user_ik_controller.py) against the compiled DG_OP_IK_CONTROL: tests/golden/jaco_ik.yaml and ur_ik.yaml, each built twice and
driven by the same seeded actions inside the action space.

jaco_ik (position only, ten joints, no lists): the compiled op takes the general solve, run_ik; the query runs its twin -- a copy
(diy_gym_amd/csrc/dg_ikq.h), not one shared function, so the targets are held to a measured bound; the measured difference is
zero, which makes that bound bit equality.
ur_ik (orientation, six joints, the four lists; ``ik_residual`` 0 on both sides so that both run every iteration): the compiled
op is the packed register-resident solve, another order of every sum.

Error measure as tests/test_user_controllers_gpu.py: per env, max |hook - compiled| over the joints divided by that env's largest
|compiled| entry.  Bounds: 8 x the largest figure measured on an MI355X over both batch sizes (DESIGN.md "Inverse-kinematics
query"); none may exceed 1e-4.
Measured maxima (MI355X, 3 and 70 envs): jaco_ik target positions after the first step 0 -- the copy compiles to the same bits as
its twin, so that bound is bit equality; ur_ik target positions 2.06e-7 (x3) / 3.06e-7 (x70), joint positions after 20 steps
9.92e-8 / 3.98e-7.
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
from user_ik_controller import PyIKController

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DEV = 'cuda:0'
# measured maxima: target positions after the first step (jaco_ik, ur_ik), joint positions after 20 steps (ur_ik)
MEASURED = {'jaco_target': 0.0, 'ur_target': 3.06e-7, 'ur_q': 3.98e-7}
BOUND = {k: 8 * v for k, v in MEASURED.items()}
assert max(BOUND.values()) <= 1e-4
SCENES = {'jaco_ik': ('robot', {}), 'ur_ik': ('arm', {'ik_residual': 0.0})}
REST = {'jaco_ik': [0.0, 2.9, 0.0, 1.3, 4.2, 1.4, 0.0], 'ur_ik': [0.3, -1.0, 1.2, -0.5, 0.4, 0.1]}   # of the controlled joints


def pair(scene, B):
    """(compiled, hooked): the scene with the compiled ik_controller and with the Python class under that name."""
    def make(cls):
        registry = AddonFactory.get().addons
        saved = registry['ik_controller']
        if cls is not None:
            AddonFactory.register_addon('ik_controller', cls)
        try:
            return DIYGym(Configuration.from_dict(scene, yaml.safe_load(open(os.path.join(GOLDEN, scene + '.yaml')))), num_envs=B, device=DEV, seed=2,
                          engine=SCENES[scene][1])
        finally:
            registry['ik_controller'] = saved
    compiled, hooked = make(None), make(PyIKController)
    assert not compiled._hook_addons and len(hooked._hook_addons) == 1 and compiled.layout.state_dim == hooked.layout.state_dim
    return compiled, hooked


def actions(scene, B, steps):
    gen = torch.Generator().manual_seed(9)
    draw = lambda: ((torch.rand((B, 3), generator=gen) * 2 - 1) * 0.01).to(DEV)
    model = SCENES[scene][0]
    if scene == 'ur_ik':
        return [{model: {'controller': {'linear': draw(), 'rotation': draw()}}} for _ in range(steps)]
    return [{model: {'controller': {'linear': draw()}}} for _ in range(steps)]


def figure(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float((np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)).max())


def columns(env, field, joints=None):
    L = env.layout
    return [L.link_state_off[L.body_first_link[0] + i] + field for i in (range(L.body_n_links[0]) if joints is None else joints)]


@pytest.mark.parametrize('scene', ['jaco_ik', 'ur_ik'])
@pytest.mark.parametrize('B', [3, 70])
def test_python_ik_controller_sets_the_compiled_ops_targets(scene, B):
    compiled, hooked = pair(scene, B)
    assert (compiled.sim.get_state().view(np.uint32) == hooked.sim.get_state().view(np.uint32)).all()   # the same reset: joints at rest, one hot-start step
    ctl = hooked.models[SCENES[scene][0]].addons['controller']
    q0 = compiled.sim.get_state()[:, columns(compiled, K.LS_Q, ctl.dofs)]
    assert np.abs(q0 - np.asarray(REST[scene])).max() < 0.05   # (at rest, give or take the hot-start step)
    act = actions(scene, B, 1)[0]
    compiled.step(act); hooked.step(act)
    assert (compiled.sim.motor_cfg() == hooked.sim.motor_cfg()).all()   # gains and force limits: set by the first update on both sides
    sc, sh = compiled.sim.get_state(), hooked.sim.get_state()
    tc, th = sc[:, columns(compiled, K.LS_TARGET_POS, ctl.dofs)], sh[:, columns(hooked, K.LS_TARGET_POS, ctl.dofs)]
    assert np.abs(tc - q0).max() > 1e-4   # (the command moved the targets off the joint positions)
    rest = [i for i in range(compiled.layout.body_n_links[0]) if i not in ctl.dofs]
    assert (sh[:, columns(hooked, K.LS_TARGET_POS, rest)] == sc[:, columns(compiled, K.LS_TARGET_POS, rest)]).all()   # (the Jaco's fingers: not commanded)
    assert (sh[:, columns(hooked, K.LS_TARGET_VEL)] == 0).all() and (sc[:, columns(compiled, K.LS_TARGET_VEL)] == 0).all()
    err = figure(th, tc)
    key = 'jaco_target' if scene == 'jaco_ik' else 'ur_target'
    print('%s x%d: target positions after the first step, hook against compiled: %.3g (bit-identical: %s)' % (scene, B, err, bool((th.view(np.uint32) == tc.view(np.uint32)).all())))
    assert err <= BOUND[key]


@pytest.mark.parametrize('B', [3, 70])
def test_python_ik_controller_follows_the_compiled_op_for_20_steps(B):
    compiled, hooked = pair('ur_ik', B)
    for act in actions('ur_ik', B, 20):
        compiled.step(act); hooked.step(act)
    qc, qh = (e.sim.get_state()[:, columns(e, K.LS_Q)] for e in (compiled, hooked))
    assert np.abs(qc - np.asarray(REST['ur_ik'])).max() > 1e-3   # (the arm did move)
    err = figure(qh, qc)
    print('ur_ik x%d: joint positions after 20 steps, hook against compiled: %.3g' % (B, err))
    assert err <= BOUND['ur_q']


@pytest.mark.parametrize('scene', ['jaco_ik', 'ur_ik'])
def test_masked_reset_leaves_the_other_envs_joints_alone(scene):
    B = 70
    compiled, hooked = pair(scene, B)
    for act in actions(scene, B, 3):
        hooked.step(act)
    before = hooked.sim.get_state()
    mask = torch.zeros(B, dtype=torch.bool, device=DEV)
    mask[::2] = True
    hooked.reset(mask)
    after = hooked.sim.get_state()
    keep = ~mask.cpu().numpy()
    cols = columns(hooked, K.LS_Q) + columns(hooked, K.LS_QD)
    assert (after[keep][:, cols].view(np.uint32) == before[keep][:, cols].view(np.uint32)).all()
    ctl = hooked.models[SCENES[scene][0]].addons['controller']
    moved = np.abs(after[~keep][:, columns(hooked, K.LS_Q, ctl.dofs)] - before[~keep][:, columns(hooked, K.LS_Q, ctl.dofs)]).max(axis=1)
    assert (moved > 0).all()   # (the reset envs went back to rest)
    assert np.abs(after[~keep][:, columns(hooked, K.LS_Q, ctl.dofs)] - np.asarray(REST[scene])).max() < 0.05
