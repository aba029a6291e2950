"""The contact_sensor addon on the host: registry, spaces, the query it makes, configuration errors.  No GPU: the scenes are built
on the CPU checker, whose backend has no contact query, so a stand-in below answers it with an empty list and records the call."""
import os

import pytest
import torch
import yaml

import oracle_backend
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.addons.sensors import ContactSensor
from diy_gym_amd.config import Configuration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'contact_sensor')   # (a folder of its own: the scenes need a backend with the query)


class _Backend(oracle_backend.OracleBackend):
    """The checker plus an empty answer to contact_points in the shape HipBackend gives it."""
    def contact_points(self, body_a=None, body_b=None, link_a=None, link_b=None, want=('id', 'pos', 'normal', 'distance', 'force')):
        from diy_gym_amd.backend import ContactPoints
        self.calls = getattr(self, 'calls', []) + [(body_a, body_b, link_a, link_b, tuple(want))]
        B, C = self.num_envs, self.layout.max_contacts
        return ContactPoints(torch.zeros(B, dtype=torch.int32), None, None, None, None, None, torch.zeros((B, C)), torch.zeros((B, C)))


def _env(tree_edit=None, name='marbles'):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, name + '.yaml')))
    if tree_edit:
        tree_edit(tree)
    cfg = Configuration.from_dict(name, tree); cfg.source_dir = GOLDEN
    return DIYGym(cfg, num_envs=2, backend_factory=_Backend)


def test_registry_resolves_contact_sensor():
    assert AddonFactory.get().addons['contact_sensor'] is ContactSensor
    assert 'contact_sensor' in open(os.path.join(ROOT, 'README.md')).read()


def test_spaces_and_filters():
    env = _env()
    green = env.models['green_marble']
    for name, target in (('on_ground', 'plane'), ('on_blue', 'blue_marble')):
        a = green.addons[name]
        assert isinstance(a, ContactSensor) and a.own_buffers and not a.terminal and not a.late_terminal
        assert (a.uid, a.target_uid, a.frame_id) == (green.uid, env.models[target].uid, None)
        sp = env.observation_space.spaces['green_marble'].spaces[name].spaces
        assert list(sp) == ['touching', 'force'] and tuple(sp['touching'].shape) == (1, ) and tuple(sp['force'].shape) == (1, )
    assert env._late_terminals == [] and not env._flat_obs_fast
    # one query per sensor and tick, with the sensor's filters; the observation has the stated shapes
    obs = env.observe()   # (the tick of the constructor's reset: already evaluated then)
    assert sorted(env.sim.calls) == sorted((green.uid, env.models[t].uid, None, None, ('distance', 'force')) for t in ('plane', 'blue_marble'))
    o = obs['green_marble']['on_ground']
    assert tuple(o['touching'].shape) == (2, 1) and tuple(o['force'].shape) == (2, 1) and o['touching'].dtype == torch.float32
    assert float(o['touching'].sum()) == 0.0 and float(o['force'].sum()) == 0.0
    env.observe()
    assert len(env.sim.calls) == 2   # (same tick: not evaluated again)


def test_terminal_scene_registers_a_late_terminal():
    env = _env(name='drop_terminal')
    a = env.models['marble'].addons['landed']
    assert a.terminal and a.force_threshold == 0.0 and env._late_terminals == [a] and env.auto_reset


def test_unknown_target_raises():
    def edit(tree):
        tree['green_marble']['on_blue']['target'] = 'purple_marble'
    with pytest.raises(ValueError, match='purple_marble'):
        _env(edit)


def test_unknown_frame_and_env_level_sensor_raise():
    def frame(tree):
        tree['green_marble']['on_ground']['frame'] = 'no_such_joint'
    with pytest.raises(ValueError, match='no_such_joint'):
        _env(frame)

    def on_env(tree):
        tree['touch'] = {'addon': 'contact_sensor'}
    with pytest.raises(ValueError, match='goes on a model'):
        _env(on_env)


def test_backend_without_the_query_says_so():
    """The CPU checker's backend has no contact query: a scene with a contact_sensor on it fails with a message that names it."""
    from diy_gym_amd import DIYGym
    with pytest.raises(NotImplementedError, match='OracleBackend'):
        DIYGym(os.path.join(GOLDEN, 'marbles.yaml'), num_envs=2, backend_factory=oracle_backend.OracleBackend)
