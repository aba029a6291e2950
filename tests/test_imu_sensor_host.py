"""The imu_sensor addon on the host: registry, spaces, the launch it makes per tick, its columns, what its compile() does to the
scene, configuration errors.  No GPU: the scenes are built on the CPU checker, whose backend has no link acceleration query, so a
stand-in below answers it with numbered entries and records the call."""
import os

import numpy as np
import pytest
import torch
import yaml

import oracle_backend
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.addons.sensors import ImuSensor
from diy_gym_amd.backend import LinkAccelerations
from diy_gym_amd.config import Configuration
from diy_gym_amd.mathx import quat_from_euler
from diy_gym_amd.scene import K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'imu_sensor')


class _Backend(oracle_backend.OracleBackend):
    """The checker plus the call in the shape HipBackend gives it: entry [e, k, c] of the [B, n, 15] buffer is 100 e + 20 k + c."""
    def link_accelerations(self, body, frames=None, local_pos=None, local_orn=None, com=False):
        self.calls = getattr(self, 'calls', []) + [(body, tuple(frames), tuple(local_pos), tuple(local_orn), com)]
        n = len(frames)
        out = (100.0 * torch.arange(self.num_envs)[:, None, None] + 20.0 * torch.arange(n)[None, :, None] + torch.arange(15)[None, None, :]).float()
        return LinkAccelerations(*(out[:, :, k:k + 3] for k in range(0, 15, 3)))


def _env(name, tree_edit=None, backend=_Backend):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, name + '.yaml')))
    if tree_edit:
        tree_edit(tree)
    cfg = Configuration.from_dict(name, tree); cfg.source_dir = GOLDEN
    return DIYGym(cfg, num_envs=2, backend_factory=backend)


def test_registry_resolves_imu_sensor():
    assert AddonFactory.get().addons['imu_sensor'] is ImuSensor
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'imu_sensor' in readme and 'link_accelerations' in readme


def test_spaces_one_call_per_tick_and_columns():
    env = _env('marble_imu')
    marble = env.models['marble']; a, t = marble.addons['imu'], marble.addons['tilted']
    assert isinstance(a, ImuSensor) and a.own_buffers and not env._flat_obs_fast
    assert a.frame_id == -1 and a.local_pos == [0., 0., 0.] and a.local_orn == [0., 0., 0., 1.] and not a.use_gravity
    assert t.local_pos == [0.1, 0., 0.] and np.allclose(t.local_orn, quat_from_euler([0.3, -0.2, 0.5])) and t.use_gravity
    sp = env.observation_space.spaces['marble'].spaces
    assert [(k, tuple(v.shape)) for k, v in sp['imu'].spaces.items()] == [('linear_acceleration', (3, )), ('angular_velocity', (3, ))]
    assert [(k, tuple(v.shape)) for k, v in sp['tilted'].spaces.items()] == [('linear_acceleration', (3, )), ('angular_velocity', (3, )), ('gravity', (3, ))]
    env.sim.calls = []
    obs = env.step({})[0]
    assert sorted(env.sim.calls, key=str) == sorted([(marble.uid, (-1, ), tuple(a.local_pos), tuple(a.local_orn), False),
                                                     (marble.uid, (-1, ), tuple(t.local_pos), tuple(t.local_orn), False)], key=str)
    env.observe()
    assert len(env.sim.calls) == 2   # (same tick: not evaluated again)
    o = obs['marble']['tilted']
    assert all(v.dtype == torch.float32 for v in o.values())
    assert o['linear_acceleration'].tolist() == [[6., 7., 8.], [106., 107., 108.]]   # the specific force
    assert o['angular_velocity'].tolist() == [[9., 10., 11.], [109., 110., 111.]]
    assert o['gravity'].tolist() == [[12., 13., 14.], [112., 113., 114.]]
    assert list(obs['marble']['imu']) == ['linear_acceleration', 'angular_velocity']
    env.step({})
    assert len(env.sim.calls) == 4


def test_a_frame_behind_a_joint():
    env = _env('pendulum_imu')
    pend = env.models['pend']; a = pend.addons['imu']
    assert a.frame_id == pend.get_frame_id('hinge') >= 0
    env.sim.calls = []
    env.step({})
    assert env.sim.calls == [(pend.uid, (a.frame_id, ), (0., 0.05, -0.2), tuple(a.local_orn), False)]


def test_compile_alone_makes_the_scene_keep_the_velocities():
    env = _env('marble_imu')
    I = env.layout.I; marble = env.models['marble'].uid
    po = int(I[int(I[K.H_OFF_BODY_I]) + marble * K.BI_STRIDE + K.BI_PREV_OFF])
    assert po >= env.layout.addon_off and int(I[K.H_N_ADDON_STATE]) == 6   # a jointless floating body: six base slots, once for both sensors

    def without(tree):
        del tree['marble']['imu'], tree['marble']['tilted']
    bare = _env('marble_imu', without)
    assert bare.layout.state_dim == env.layout.state_dim - 6
    assert int(bare.layout.I[int(bare.layout.I[K.H_OFF_BODY_I]) + marble * K.BI_STRIDE + K.BI_PREV_OFF]) < 0
    pend = _env('pendulum_imu')
    assert int(pend.layout.I[K.H_N_ADDON_STATE]) == 1   # one joint, fixed base


def test_configuration_errors():
    def frame(tree):
        tree['marble']['imu']['frame'] = 'no_such_joint'
    with pytest.raises(ValueError, match='no_such_joint'):
        _env('marble_imu', frame)

    def on_env(tree):
        tree['imu'] = {'addon': 'imu_sensor'}
    with pytest.raises(ValueError, match='goes on a model'):
        _env('marble_imu', on_env)

    def on_fixed(tree):
        tree['marble']['use_fixed_base'] = True
    with pytest.raises(ValueError, match='fixed base and no joints'):
        _env('marble_imu', on_fixed)

    def on_plane(tree):
        tree['plane']['imu'] = {'addon': 'imu_sensor'}
    with pytest.raises(ValueError, match='fixed base and no joints'):
        _env('marble_imu', on_plane)


def test_backend_without_the_query_says_so():
    with pytest.raises(NotImplementedError, match='OracleBackend'):
        _env('marble_imu', backend=oracle_backend.OracleBackend)
