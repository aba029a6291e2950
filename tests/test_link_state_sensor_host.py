"""The link_state_sensor addon on the host: registry, spaces, the one query it makes per tick, its values, configuration errors.  No
GPU: the scenes are built on the CPU checker, whose backend has no batched link-state query, so a stand-in below answers it by
stacking the checker's own frame_state and records the call."""
import os

import pytest
import torch
import yaml

import oracle_backend
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.addons.sensors import LinkStateSensor
from diy_gym_amd.config import Configuration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'link_state_sensor')   # (a folder of its own: the scenes need a backend with the query)


class _Backend(oracle_backend.OracleBackend):
    """The checker plus link_states in the shape HipBackend gives it: [B, n, 13], the rows of frame_state."""
    def link_states(self, body, frames=None, com=False):
        frames = [-1] if frames is None else list(frames)
        self.calls = getattr(self, 'calls', []) + [(body, tuple(frames), bool(com))]
        return torch.stack([self.frame_state(*self.layout.resolve_frame(body, f), com=com) for f in frames], dim=1)


def _env(name, tree_edit=None):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, name + '.yaml')))
    if tree_edit:
        tree_edit(tree)
    cfg = Configuration.from_dict(name, tree); cfg.source_dir = GOLDEN
    return DIYGym(cfg, num_envs=2, backend_factory=_Backend)


def test_registry_resolves_link_state_sensor():
    assert AddonFactory.get().addons['link_state_sensor'] is LinkStateSensor
    assert 'link_state_sensor' in open(os.path.join(ROOT, 'README.md')).read()


def test_spaces_one_query_per_tick_and_values():
    env = _env('arm_keypoints')
    arm = env.models['arm']
    key, root = arm.addons['keypoints'], arm.addons['root']
    assert isinstance(key, LinkStateSensor) and key.own_buffers and not env._flat_obs_fast
    ids = [arm.get_frame_id('elbow_joint'), -1, arm.get_frame_id('wrist_3_joint')]
    assert min(ids[0], ids[2]) >= 0 and key.frame_ids == ids and root.frame_ids == [-1] and not key.com
    sp = env.observation_space.spaces['arm'].spaces
    assert list(sp['keypoints'].spaces) == ['position', 'orientation', 'velocity', 'angular_velocity']
    assert [tuple(s.shape) for s in sp['keypoints'].spaces.values()] == [(9, ), (12, ), (9, ), (9, )]
    assert list(sp['root'].spaces) == ['position', 'orientation'] and [tuple(s.shape) for s in sp['root'].spaces.values()] == [(3, ), (4, )]
    env.sim.calls = []
    obs = env.step({'arm': {'controller': torch.full((2, 6), 0.2)}})[0]   # (a step, so that velocities are not zero)
    assert sorted(env.sim.calls) == sorted([(arm.uid, tuple(ids), False), (arm.uid, (-1, ), False)])   # one query per sensor
    env.observe()
    assert len(env.sim.calls) == 2   # (same tick: not evaluated again)
    want = torch.stack([env.sim.frame_state(arm.uid, f) for f in ids], dim=1)
    o = obs['arm']['keypoints']
    assert all(v.dtype == torch.float32 for v in o.values())
    assert torch.equal(o['position'], want[:, :, 0:3].reshape(2, 9)) and torch.equal(o['orientation'], want[:, :, 3:7].reshape(2, 12))
    assert torch.equal(o['velocity'], want[:, :, 7:10].reshape(2, 9)) and torch.equal(o['angular_velocity'], want[:, :, 10:13].reshape(2, 9))
    assert float(o['velocity'].abs().max()) > 0.0
    assert torch.equal(obs['arm']['root']['position'], env.sim.frame_state(arm.uid, -1)[:, 0:3])


def test_one_frame_inertial_with_and_without_velocity():
    env = _env('falling_marble')
    m = env.models['marble']
    assert m.addons['pose'].com and m.addons['pose'].frame_ids == [-1]
    sp = env.observation_space.spaces['marble'].spaces
    assert [tuple(s.shape) for s in sp['pose'].spaces.values()] == [(3, ), (4, )]
    assert [tuple(s.shape) for s in sp['motion'].spaces.values()] == [(3, ), (4, ), (3, ), (3, )]
    env.step({})
    obs = env.observe()
    want = env.sim.frame_state(m.uid, -1, com=True)
    assert torch.equal(obs['marble']['pose']['position'], want[:, 0:3]) and torch.equal(obs['marble']['pose']['orientation'], want[:, 3:7])
    assert torch.equal(obs['marble']['motion']['velocity'], want[:, 7:10]) and torch.equal(obs['marble']['motion']['angular_velocity'], want[:, 10:13])
    assert float(want[:, 9].abs().min()) > 0.0   # (it falls)
    assert (m.uid, (-1, ), True) in env.sim.calls


def test_unknown_frame_and_env_level_sensor_raise():
    def frame(tree):
        tree['arm']['keypoints']['frames'] = ['elbow_joint', 'no_such_joint']
    with pytest.raises(ValueError, match='no_such_joint'):
        _env('arm_keypoints', frame)

    def on_env(tree):
        tree['poses'] = {'addon': 'link_state_sensor'}
    with pytest.raises(ValueError, match='goes on a model'):
        _env('arm_keypoints', on_env)

    def too_many(tree):
        tree['arm']['keypoints']['frames'] = ['elbow_joint'] * 33
    with pytest.raises(ValueError, match='1 .. 32'):
        _env('arm_keypoints', too_many)


def test_backend_without_the_query_says_so():
    with pytest.raises(NotImplementedError, match='OracleBackend'):
        DIYGym(os.path.join(GOLDEN, 'falling_marble.yaml'), num_envs=2, backend_factory=oracle_backend.OracleBackend)
