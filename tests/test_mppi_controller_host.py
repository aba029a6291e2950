"""The mppi_controller addon on the host: registry, spaces, the env.sim calls it makes per tick and their shapes, the shift of the
nominal sequence, the softmax update against numpy on fixed numbers, how its target accumulates, what reset() does with
env.reset_mask, the motors switched off once, configuration errors, the same seed giving the same noise.  No GPU: the scene is built
on the CPU checker, whose backend has none of the queries, so a stand-in below answers them with fixed numbers -- a rollout whose
outputs are a known function of the torques it was given -- and records the calls."""
import os

import numpy as np
import pytest
import torch
import yaml

import oracle_backend
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.addons.controllers import MppiController
from diy_gym_amd.backend import JointRollout, TaskSpaceDynamics
from diy_gym_amd.config import Configuration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'rollout')
POSE = [0.4, 0.1, 0.6]   # what the stand-in reports as the point: this (+ 0.01 e in x for env e)
GRAV = [0.0, -40.0, -12.0, -1.5, 0.1, 0.0]   # ... and as the gravity compensation (+ e)
MIX = np.array([[0.002, -0.001, 0.0005], [0.001, 0.003, -0.002], [-0.0015, 0.0005, 0.001], [0.0, 0.002, 0.001], [0.001, 0.0, 0.0], [0.0, 0.0, 0.003]])


def standin_rollout(tau):
    """pos [B, K, T, 3] and qd [B, K, T, nv] as the stand-in derives them from tau [B, K, T, nv] (float64 numpy)."""
    run = np.cumsum(tau, axis=2)
    return np.array(POSE) + run @ MIX * 0.01, 0.001 * run


class _Backend(oracle_backend.OracleBackend):
    """The checker plus the calls mppi_controller makes, in the shapes HipBackend gives them."""
    def _log(self, *call):
        self.calls = getattr(self, 'calls', []) + [call]

    def task_space_dynamics(self, body, frame, local_pos=(0.0, 0.0, 0.0), axes=(0, 1, 2, 3, 4, 5), q=None, qd=None, acc=None, tau_null=None, damping=0.0,
                            want=('jac', 'bias_acc', 'bias_torque', 'lambda', 'tau', 'point', 'singular')):
        self._log('task_space_dynamics', body, frame, tuple(local_pos), tuple(axes), q, qd, acc, tau_null, damping, tuple(want))
        point = torch.tensor(POSE + [0.0, 0.0, 0.0, 1.0] + [0.0] * 6, dtype=torch.float32).repeat(self.num_envs, 1)
        point[:, 0] += 0.01 * torch.arange(self.num_envs) + getattr(self, 'moved', 0.0)
        return TaskSpaceDynamics(None, None, None, None, None, point, None)

    def calculate_inverse_dynamics(self, body, q=None, qd=None, qdd=None):
        self._log('calculate_inverse_dynamics', body, q, None if qd is None else qd.clone(), qdd)
        return torch.tensor(GRAV, dtype=torch.float32).repeat(self.num_envs, 1) + torch.arange(self.num_envs, dtype=torch.float32)[:, None]

    def rollout_joint_dynamics(self, body, tau, q0=None, qd0=None, dt=None, frame=None, local_pos=(0.0, 0.0, 0.0), joint_damping=False, want=('q', 'qd')):
        self._log('rollout_joint_dynamics', body, tau.clone(), q0, qd0, dt, frame, tuple(local_pos), joint_damping, tuple(want))
        pos, qd = standin_rollout(tau.double().numpy())
        return JointRollout(None, torch.from_numpy(qd).float() if 'qd' in want else None, torch.from_numpy(pos).float() if 'pos' in want else None, None)

    def apply_joint_torque(self, body, torque):
        self._log('apply_joint_torque', body, torque.clone())

    def set_motor_cfg(self, cfg):
        self._log('set_motor_cfg', np.array(cfg, copy=True))
        super().set_motor_cfg(cfg)


def _env(edit=None, B=2, seed=0):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_mppi.yaml')))
    tree['arm']['mppi'].update(samples=8, horizon=4)
    if edit:
        edit(tree['arm']['mppi'])
    cfg = Configuration.from_dict('ur_mppi', tree); cfg.source_dir = GOLDEN
    return DIYGym(cfg, num_envs=B, seed=seed, backend_factory=_Backend)


def _named(env, name):
    return [c for c in env.sim.calls if c[0] == name]


def _tick(env, linear=None):
    env.sim.calls = []
    env.step({'arm': {'mppi': {'linear': torch.zeros((env.num_envs, 3)) if linear is None else linear}}})
    return [c for c in env.sim.calls if c[0] != 'set_motor_cfg']


def test_registry_resolves_mppi_controller():
    assert AddonFactory.get().addons['mppi_controller'] is MppiController
    assert not hasattr(MppiController, 'compile')   # a hook addon: written on env.sim calls only
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'mppi_controller' in readme and 'rollout_joint_dynamics' in readme and 'calculate_forward_dynamics' in readme
    assert 'NOT shard-invariant' in MppiController.__doc__ and 'shard-invariant' in readme


def test_spaces_and_configuration():
    env = _env()
    a = env.models['arm'].addons['mppi']
    assert isinstance(a, MppiController) and a in env._hook_addons
    sp = env.action_space.spaces['arm'].spaces['mppi'].spaces
    assert [(k, tuple(v.shape), float(v.low.min()), float(v.high.max())) for k, v in sp.items()] == [('linear', (3, ), float(np.float32(-0.01)), float(np.float32(0.01)))]
    assert a.end_frame == env.models['arm'].get_frame_id('ee_fixed_joint') and a.offset == [0.0, 0.0, 0.05]
    assert (a.samples, a.horizon, a.noise, a.temperature) == (8, 4, 0.1, 1.0)
    assert (a.w_position, a.w_velocity, a.w_torque) == (1.0, 0.01, 0.0) and a.joint_damping and a.clip_torque
    assert a.dt == pytest.approx(4 * env.layout.dt)   # the default: four substeps per model step
    bare = {'addon': 'mppi_controller', 'end_effector': 'ee_fixed_joint'}   # every default
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_mppi.yaml')))
    tree['arm']['mppi'] = bare
    cfg = Configuration.from_dict('ur_mppi', tree); cfg.source_dir = GOLDEN
    d = DIYGym(cfg, num_envs=1, backend_factory=_Backend).models['arm'].addons['mppi']
    assert (d.samples, d.horizon, d.noise, d.temperature, d.offset) == (64, 16, 0.1, 1.0, [0.0, 0.0, 0.0])


def test_reset_switches_the_motors_off_once_and_honours_the_mask():
    env = _env(B=3)
    arm = env.models['arm']; a = arm.addons['mppi']
    off = _named(env, 'set_motor_cfg')
    assert len(off) == 1 and (off[0][1][:6, 2] == 0).all() and (env.sim.motor_cfg()[:6, 2] == 0).all()
    assert a._effort.tolist() == [j.effort for j in arm.robot.joints if j.q_index > -1] and min(a._effort.tolist()) > 0
    assert torch.allclose(a._sigma, 0.1 * a._effort)
    assert not _named(env, 'task_space_dynamics')   # the target is read on the first tick, from the pose the reset left
    calls = _tick(env)
    assert [c[0] for c in calls] == ['task_space_dynamics', 'calculate_inverse_dynamics', 'rollout_joint_dynamics', 'apply_joint_torque']
    assert calls[0][1:5] == (arm.uid, a.end_frame, (0.0, 0.0, 0.05), (0, 1, 2)) and calls[0][10] == ('point', )
    assert np.abs(a.target_pos.numpy() - np.array([[0.4, 0.1, 0.6], [0.41, 0.1, 0.6], [0.42, 0.1, 0.6]])).max() < 1e-6
    assert [c[0] for c in _tick(env)] == ['calculate_inverse_dynamics', 'rollout_joint_dynamics', 'apply_joint_torque']   # ... and on no other
    assert float(a.nominal.abs().max()) > 0
    # a masked reset: the nominal sequence of the masked envs is cleared and their target re-read; the motors stay
    a.set_target([1.0, 2.0, 3.0])
    before = a.nominal.clone()
    env.sim.calls = []
    env.reset(torch.tensor([False, True, False]))
    assert not _named(env, 'set_motor_cfg')
    assert float(a.nominal[1].abs().max()) == 0 and torch.equal(a.nominal[0], before[0]) and torch.equal(a.nominal[2], before[2])
    env.sim.moved = 0.5
    assert [c[0] for c in _tick(env)][0] == 'task_space_dynamics'
    assert np.abs(a.target_pos.numpy() - np.array([[1.0, 2.0, 3.0], [0.91, 0.1, 0.6], [1.0, 2.0, 3.0]])).max() < 1e-6
    # set_target with a mask, per-env rows
    a.set_target(torch.zeros((3, 3)), mask=[True, False, False])
    assert a.target_pos[0].tolist() == [0.0, 0.0, 0.0] and a.target_pos[2].tolist() == [1.0, 2.0, 3.0]


def test_the_calls_of_a_tick_their_shapes_and_the_accumulating_target():
    env = _env()
    arm = env.models['arm']; a = arm.addons['mppi']
    _tick(env)
    p0 = a.target_pos.clone()
    lin = torch.tensor([[0.01, 0.0, -0.005], [0.0, 0.002, 0.0]])
    grav, roll, apply = _tick(env, lin)
    assert grav[1] == arm.uid and grav[2] is None and grav[4] is None and tuple(grav[3].shape) == (2, 6) and float(grav[3].abs().max()) == 0   # qd = 0, qdd = 0
    _, body, tau, q0, qd0, dt, frame, lp, damping, want = roll
    assert body == arm.uid and tuple(tau.shape) == (2, 8, 4, 6) and tau.dtype == torch.float32 and tau.is_contiguous()
    assert q0 is None and qd0 is None and dt == pytest.approx(4 * env.layout.dt) and frame == a.end_frame and lp == (0.0, 0.0, 0.05) and damping is True
    assert want == ('qd', 'pos')
    assert apply[1] == arm.uid and tuple(apply[2].shape) == (2, 6)
    assert torch.allclose(a.target_pos, p0 + lin, atol=1e-7)
    _tick(env, lin)
    assert torch.allclose(a.target_pos, p0 + 2 * lin, atol=1e-7)
    env.sim.calls = []
    env.step({})   # an addon that is not named in the action is not updated
    assert not env.sim.calls


@pytest.mark.parametrize('temperature,weights', [(1.0, None), (0.2, {'position': 2.0, 'terminal_velocity': 0.5, 'torque': 1e-4})])
def test_the_shift_and_the_softmax_update_against_numpy(temperature, weights):
    def edit(c):
        c.update(temperature=temperature, clip_torque=False)
        if weights:
            c['weights'] = weights
    env = _env(edit)
    a = env.models['arm'].addons['mppi']
    w_p, w_v, w_u = (1.0, 0.01, 0.0) if weights is None else (2.0, 0.5, 1e-4)
    g = np.array(GRAV)[None, :] + np.arange(2)[:, None]
    U = np.zeros((2, 4, 6))
    for tick in range(3):
        calls = _tick(env)
        tau = _named(env, 'rollout_joint_dynamics')[0][2].double().numpy()
        U = np.concatenate([U[:, 1:], np.zeros((2, 1, 6))], axis=1)   # shifted by one, a zero enters
        eps = tau - (g[:, None, :] + U)[:, None]
        assert np.abs(eps[:, 0]).max() < 16 * 2.0 ** -23 * np.abs(tau).max()   # sample 0 is the nominal sequence itself (to the fp32 rounding of a few sums)
        sigma = 0.1 * np.array(a._effort.tolist())
        assert np.all(np.abs(eps[:, 1:].std(axis=(0, 1, 2)) / sigma - 1.0) < 0.35)   # 56 draws per joint
        pos, qd = standin_rollout(tau)
        target = a.target_pos.double().numpy()
        cost = w_p * ((pos - target[:, None, None, :]) ** 2).sum(axis=(2, 3)) + w_v * (qd[:, :, -1] ** 2).sum(axis=2) + w_u * (eps ** 2).sum(axis=(2, 3))
        rel = cost - cost.min(axis=1, keepdims=True)
        rel = rel / rel.mean(axis=1, keepdims=True)
        w = np.exp(-rel / temperature); w /= w.sum(axis=1, keepdims=True)
        U = U + (w[:, :, None, None] * eps).sum(axis=1)
        assert np.abs(a.nominal.double().numpy() - U).max() < 2e-4 * max(1.0, np.abs(U).max()), tick
        assert np.abs(calls[-1][2].double().numpy() - (g + U[:, 0])).max() < 2e-4 * np.abs(g).max()
    assert np.abs(U[:, -1]).max() > 0 and np.abs(U).max() > 0.1


def test_clip_torque_clamps_the_samples_and_the_applied_torque():
    def edit(c):
        c.update(noise=2.0)   # noise of twice the effort limit: most samples leave the limits
    env = _env(edit)
    a = env.models['arm'].addons['mppi']
    calls = _tick(env)
    eff = np.array(a._effort.tolist())
    tau = _named(env, 'rollout_joint_dynamics')[0][2].numpy()
    assert (np.abs(tau) <= eff + 1e-4).all() and (np.abs(np.abs(tau) - eff) < 1e-4).mean() > 0.3
    assert (np.abs(calls[-1][2].numpy()) <= eff + 1e-4).all()


def test_the_same_seed_gives_the_same_noise():
    taus = []
    for seed in (3, 3, 4):
        env = _env(seed=seed)
        _tick(env)
        _tick(env)
        taus.append(_named(env, 'rollout_joint_dynamics')[0][2])
    assert torch.equal(taus[0], taus[1]) and not torch.equal(taus[0], taus[2])


def test_configuration_errors():
    def missing(c):
        del c['end_effector']
    with pytest.raises(ValueError, match='end_effector is required'):
        _env(missing)

    def unknown(c):
        c['end_effector'] = 'no_such_joint'
    with pytest.raises(ValueError, match='no_such_joint'):
        _env(unknown)
    for key, value, text in (('offset', [0.0, 0.0], 'offset'), ('samples', 0, 'samples and horizon'), ('horizon', 0, 'samples and horizon'), ('dt', 0.0, 'dt must be > 0'),
                             ('noise', 0.0, 'noise and temperature'), ('temperature', -1.0, 'noise and temperature'), ('weights', {'position': -1.0}, 'weights must be >= 0'),
                             ('weights', {'velocity': 1.0}, 'weights takes')):
        def edit(c, key=key, value=value):
            c[key] = value
        with pytest.raises(ValueError, match=text):
            _env(edit)
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_mppi.yaml')))
    tree['mppi'] = {'addon': 'mppi_controller', 'end_effector': 'ee_fixed_joint'}
    cfg = Configuration.from_dict('ur_mppi', tree); cfg.source_dir = GOLDEN
    with pytest.raises(ValueError, match='goes on a model'):
        DIYGym(cfg, num_envs=2, backend_factory=_Backend)


def test_backend_without_the_queries_says_so():
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_mppi.yaml')))
    cfg = Configuration.from_dict('ur_mppi', tree); cfg.source_dir = GOLDEN
    env = DIYGym(cfg, num_envs=2, backend_factory=oracle_backend.OracleBackend)
    with pytest.raises((NotImplementedError, AttributeError), match='task_space_dynamics|rollout_joint_dynamics|OracleBackend'):
        env.step({'arm': {'mppi': {'linear': torch.zeros((2, 3))}}})


def test_the_example_scene_builds_and_steps():
    env = DIYGym(os.path.join(ROOT, 'examples', 'ur_high_5', 'mppi', 'ur_high_5_mppi.yaml'), num_envs=2, backend_factory=_Backend)
    both = [env.models[k].addons['controller'] for k in ('ur5_l', 'ur5_r')]
    assert all(isinstance(a, MppiController) and a.samples == 64 and a.horizon == 16 for a in both)
    assert (env.sim.motor_cfg()[:12, 2] == 0).all()   # both arms' motors off
    env.sim.calls = []
    zero = {'linear': torch.zeros((2, 3))}
    env.step({'ur5_l': {'controller': zero}, 'ur5_r': {'controller': zero}})
    assert [c[0] for c in env.sim.calls] == ['task_space_dynamics', 'calculate_inverse_dynamics', 'rollout_joint_dynamics', 'apply_joint_torque'] * 2
    assert {c[1] for c in env.sim.calls} == {a.uid for a in both}
    assert all(tuple(c[2].shape) == (2, 64, 16, 6) for c in _named(env, 'rollout_joint_dynamics'))
