"""The contact_force_sensor addon on the host: registry, spaces, the query it makes, configuration errors.  No GPU: the scenes are
built on the CPU checker, whose backend has no net contact wrench, so a stand-in below answers it with zeros and records the call."""
import os

import pytest
import torch
import yaml

import oracle_backend
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.addons.sensors import ContactForceSensor
from diy_gym_amd.config import Configuration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'contact_force_sensor')   # (a folder of its own: the scenes need a backend with the query)


class _Backend(oracle_backend.OracleBackend):
    """The checker plus a zero answer to net_contact_forces in the shape HipBackend gives it."""
    def net_contact_forces(self, body, links=None, body_b=None, link_b=None, want=('force', 'torque', 'count')):
        self.calls = getattr(self, 'calls', []) + [(body, None if links is None else tuple(links), body_b, link_b, tuple(want))]
        B, n = self.num_envs, 1 if links is None else len(links)
        return (torch.zeros((B, n, 3)) if 'force' in want else None, torch.ones((B, n, 3)) if 'torque' in want else None,
                torch.zeros((B, n), dtype=torch.int32) if 'count' in want else None)


def _env(tree_edit=None, name='marbles'):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, name + '.yaml')))
    if tree_edit:
        tree_edit(tree)
    cfg = Configuration.from_dict(name, tree); cfg.source_dir = GOLDEN
    return DIYGym(cfg, num_envs=2, backend_factory=_Backend)


def test_registry_resolves_contact_force_sensor():
    assert AddonFactory.get().addons['contact_force_sensor'] is ContactForceSensor
    assert 'contact_force_sensor' in open(os.path.join(ROOT, 'README.md')).read()


def test_whole_body_sensor_spaces_and_the_one_query_per_tick():
    env = _env()
    green = env.models['green_marble']
    for name, target in (('ground_reaction', env.models['plane'].uid), ('all_contacts', None)):
        a = green.addons[name]
        assert isinstance(a, ContactForceSensor) and a.own_buffers and not a.use_torque
        assert (a.uid, a.target_uid, a.frame_ids) == (green.uid, target, None)
        sp = env.observation_space.spaces['green_marble'].spaces[name].spaces
        assert list(sp) == ['force'] and tuple(sp['force'].shape) == (3, )
    obs = env.observe()   # (the tick of the constructor's reset: already evaluated then)
    assert sorted(env.sim.calls, key=str) == sorted(((green.uid, None, t, None, ('force', )) for t in (env.models['plane'].uid, None)), key=str)
    o = obs['green_marble']['ground_reaction']
    assert list(o) == ['force'] and tuple(o['force'].shape) == (2, 3) and o['force'].dtype == torch.float32 and float(o['force'].abs().sum()) == 0.0
    env.observe()
    assert len(env.sim.calls) == 2   # (same tick: not evaluated again)
    env.step({})
    assert len(env.sim.calls) == 4   # one launch per sensor and step


def test_per_link_sensor_with_torque():
    env = _env(name='arm_feet')
    arm = env.models['arm']; a = arm.addons['feet']
    ids = [arm.get_frame_id('wrist_3_joint'), arm.get_frame_id('elbow_joint')]
    assert min(ids) >= 0 and a.frame_ids == ids and a.use_torque and a.target_uid == env.models['plane'].uid
    sp = env.observation_space.spaces['arm'].spaces['feet'].spaces
    assert list(sp) == ['force', 'torque'] and tuple(sp['force'].shape) == (6, ) and tuple(sp['torque'].shape) == (6, )
    o = env.observe()['arm']['feet']
    assert env.sim.calls == [(arm.uid, tuple(ids), env.models['plane'].uid, None, ('force', 'torque'))]
    assert tuple(o['force'].shape) == (2, 6) and tuple(o['torque'].shape) == (2, 6) and float(o['torque'].sum()) == 12.0


def test_configuration_errors():
    def torque_without_frames(tree):
        tree['green_marble']['all_contacts']['use_torque'] = True
    with pytest.raises(ValueError, match='use_torque needs frames'):
        _env(torque_without_frames)

    def target(tree):
        tree['green_marble']['ground_reaction']['target'] = 'purple_marble'
    with pytest.raises(ValueError, match='purple_marble'):
        _env(target)

    def frame(tree):
        tree['arm']['feet']['frames'] = ['wrist_3_joint', 'no_such_joint']
    with pytest.raises(ValueError, match='no_such_joint'):
        _env(frame, name='arm_feet')

    def too_many(tree):
        tree['arm']['feet']['frames'] = ['elbow_joint'] * 17
    with pytest.raises(ValueError, match='1 .. 16'):
        _env(too_many, name='arm_feet')

    def on_env(tree):
        tree['push'] = {'addon': 'contact_force_sensor'}
    with pytest.raises(ValueError, match='goes on a model'):
        _env(on_env)


def test_backend_without_the_query_says_so():
    """The CPU checker's backend has no net contact wrench: a scene with a contact_force_sensor on it fails with a message that names it."""
    with pytest.raises(NotImplementedError, match='OracleBackend'):
        DIYGym(os.path.join(GOLDEN, 'marbles.yaml'), num_envs=2, backend_factory=oracle_backend.OracleBackend)
