"""The joint_wrench_sensor addon on the host: registry, spaces, the launches it makes per tick, its columns, configuration errors.
No GPU: the scenes are built on the CPU checker, whose backend has no joint reaction query, so a stand-in below answers it with
numbered entries and records the call."""
import os

import pytest
import torch
import yaml

import oracle_backend
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.addons.sensors import JointWrenchSensor
from diy_gym_amd.config import Configuration
from diy_gym_amd.scene import K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'joint_wrench')


class _Backend(oracle_backend.OracleBackend):
    """The checker plus the two calls in the shapes HipBackend gives them: entry [e, k, c] of the wrench is 100 e + 10 k + c."""
    def joint_reaction_forces(self, body, joints=None):
        self.calls = getattr(self, 'calls', []) + [('wrench', body, None if joints is None else tuple(joints))]
        n = len(joints)
        return (100.0 * torch.arange(self.num_envs)[:, None, None] + 10.0 * torch.arange(n)[None, :, None] + torch.arange(6)[None, None, :]).float()

    def joint_motor_torques(self, body):
        self.calls = getattr(self, 'calls', []) + [('effort', body)]
        return torch.full((self.num_envs, int(self.layout.body_n_links[body])), 7.0)


def _env(name, tree_edit=None):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, name + '.yaml')))
    if tree_edit:
        tree_edit(tree)
    cfg = Configuration.from_dict(name, tree); cfg.source_dir = GOLDEN
    return DIYGym(cfg, num_envs=2, backend_factory=_Backend)


def test_registry_resolves_joint_wrench_sensor():
    assert AddonFactory.get().addons['joint_wrench_sensor'] is JointWrenchSensor
    assert 'joint_wrench_sensor' in open(os.path.join(ROOT, 'README.md')).read()


def test_spaces_launches_per_tick_and_columns():
    env = _env('pendulum_prop_sensor')
    pend = env.models['pend']; a, load = pend.addons['reactions'], pend.addons['load']
    ids = [pend.get_frame_id('mount'), pend.get_frame_id('hinge')]
    assert isinstance(a, JointWrenchSensor) and a.own_buffers and not env._flat_obs_fast
    assert a.frame_ids == ids and a.use_motor_torque and load.frame_ids == [pend.get_frame_id('hinge')] and not load.use_motor_torque
    sp = env.observation_space.spaces['pend'].spaces
    assert [(k, tuple(v.shape)) for k, v in sp['reactions'].spaces.items()] == [('force', (6, )), ('torque', (6, )), ('motor_torque', (1, ))]
    assert [(k, tuple(v.shape)) for k, v in sp['load'].spaces.items()] == [('force', (3, )), ('torque', (3, ))]
    env.sim.calls = []
    obs = env.step({})[0]
    assert sorted(env.sim.calls, key=str) == sorted([('wrench', pend.uid, tuple(ids)), ('effort', pend.uid), ('wrench', pend.uid, (ids[1], ))], key=str)
    env.observe()
    assert len(env.sim.calls) == 3   # (same tick: not evaluated again)
    o = obs['pend']['reactions']
    assert all(v.dtype == torch.float32 for v in o.values())
    assert o['force'].tolist() == [[0., 1., 2., 10., 11., 12.], [100., 101., 102., 110., 111., 112.]]
    assert o['torque'].tolist() == [[3., 4., 5., 13., 14., 15.], [103., 104., 105., 113., 114., 115.]]
    assert o['motor_torque'].tolist() == [[7.], [7.]]
    # compile() reserved nothing new: the compiled sensors of the model own the saved velocities, and the sensor shares them
    I = env.layout.I
    assert I[int(I[K.H_OFF_BODY_I]) + pend.uid * K.BI_STRIDE + K.BI_PREV_OFF] >= env.layout.addon_off


def test_the_sensor_alone_makes_the_scene_keep_the_velocities():
    def edit(tree):
        del tree['pend']['wrist'], tree['pend']['shoulder']
    env = _env('pendulum_prop_sensor', edit)
    I = env.layout.I; pend = env.models['pend'].uid
    po = int(I[int(I[K.H_OFF_BODY_I]) + pend * K.BI_STRIDE + K.BI_PREV_OFF])
    assert po >= env.layout.addon_off and int(I[K.H_N_ADDON_STATE]) == 1   # one joint, fixed base
    arm = _env('arm_swing')
    assert arm.models['arm'].addons['reactions'].frame_ids == [j.index for j in arm.models['arm'].robot.joints if j.q_index > -1]
    assert int(arm.layout.I[K.H_N_ADDON_STATE]) == 6


def test_configuration_errors():
    def frame(tree):
        tree['pend']['reactions']['frames'] = ['mount', 'no_such_joint']
    with pytest.raises(ValueError, match='no_such_joint'):
        _env('pendulum_prop_sensor', frame)

    def too_many(tree):
        tree['pend']['reactions']['frames'] = ['mount'] * 17
    with pytest.raises(ValueError, match='1 .. 16'):
        _env('pendulum_prop_sensor', too_many)

    def none(tree):
        tree['pend']['reactions']['frames'] = []
    with pytest.raises(ValueError, match='1 .. 16'):
        _env('pendulum_prop_sensor', none)

    def on_env(tree):
        tree['loads'] = {'addon': 'joint_wrench_sensor'}
    with pytest.raises(ValueError, match='goes on a model'):
        _env('pendulum_prop_sensor', on_env)


def test_backend_without_the_query_says_so():
    with pytest.raises(NotImplementedError, match='OracleBackend'):
        DIYGym(os.path.join(GOLDEN, 'pendulum_prop_sensor.yaml'), num_envs=2, backend_factory=oracle_backend.OracleBackend)
