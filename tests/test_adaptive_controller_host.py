"""The adaptive_controller addon on the host: registry, spaces, the env.sim calls it makes per tick with their arguments and shapes,
the control law and the update law on fixed numbers, the clamp of the estimate, what reset() does with env.reset_mask, set_target,
the motors switched off once, configuration errors.  No GPU: the scene is built on the CPU checker, whose backend has none of the
queries, so a stand-in below answers them with fixed numbers and records the calls."""
import os

import numpy as np
import pytest
import torch
import yaml

import oracle_backend
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.addons.controllers import AdaptiveController
from diy_gym_amd.backend import DynamicsRegressor
from diy_gym_amd.config import Configuration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'regressor')
REST = [0.3, -1.0, 1.2, -0.5, 0.4, 0.1]
DAMPING = [100.0, 100.0, 50.0, 10.0, 10.0, 5.0]
_RNG = np.random.default_rng(0)
THETA0 = _RNG.uniform(0.1, 2.0, (6, 10)).astype(np.float32)   # what the stand-in reports as the nominal parameters (every env's)
TAU = np.array([1.0, -40.0, -12.0, -1.5, 0.1, 0.0], dtype=np.float32)   # ... as r.tau (+ e for env e)
GRAD = _RNG.uniform(-1.0, 1.0, 60).astype(np.float32)   # ... as r.grad (x (1 + e))
Q_NOW = np.array(REST) + np.array([0.02, -0.01, 0.03, 0.0, -0.02, 0.01])   # ... and as the joint state (+ 0.001 e)
QD_NOW = np.array([0.1, 0.0, -0.2, 0.05, 0.0, 0.3])


class _Backend(oracle_backend.OracleBackend):
    """The checker plus the calls adaptive_controller makes, in the shapes HipBackend gives them."""
    def _log(self, *call):
        self.calls = getattr(self, 'calls', []) + [call]

    def inertial_parameters(self, body, nominal=False):
        self._log('inertial_parameters', body, nominal)
        return torch.tensor(THETA0).repeat(self.num_envs, 1, 1)

    def inverse_dynamics_regressor(self, body, q=None, qd=None, qdd=None, qd_ref=None, theta=None, s=None, want=('Y', )):
        self._log('inverse_dynamics_regressor', body, q.clone(), qd.clone(), qdd.clone(), qd_ref.clone(), theta.clone(), s.clone(), tuple(want))
        e = torch.arange(self.num_envs, dtype=torch.float32)[:, None]
        return DynamicsRegressor(None, torch.tensor(TAU).repeat(self.num_envs, 1) + e, torch.tensor(GRAD).repeat(self.num_envs, 1) * (1.0 + e) * getattr(self, 'push', 1.0))

    def joint_states(self, body):
        self._log('joint_states', body)
        e = torch.arange(self.num_envs, dtype=torch.float32)[:, None]
        return (torch.tensor(Q_NOW, dtype=torch.float32).repeat(self.num_envs, 1) + 0.001 * e + getattr(self, 'moved', 0.0),
                torch.tensor(QD_NOW, dtype=torch.float32).repeat(self.num_envs, 1))

    def apply_joint_torque(self, body, torque):
        self._log('apply_joint_torque', body, torque.clone())

    def set_motor_cfg(self, cfg):
        self._log('set_motor_cfg', np.array(cfg, copy=True))
        super().set_motor_cfg(cfg)


def _env(edit=None, B=2, seed=0):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_adaptive.yaml')))
    if edit:
        edit(tree['arm']['adaptive'])
    cfg = Configuration.from_dict('ur_adaptive', tree); cfg.source_dir = GOLDEN
    return DIYGym(cfg, num_envs=B, seed=seed, backend_factory=_Backend)


def _named(env, name):
    return [c for c in env.sim.calls if c[0] == name]


def _tick(env, target=None):
    env.sim.calls = []
    env.step({'arm': {'adaptive': {'target': torch.zeros((env.num_envs, 6)) if target is None else target}}})
    return [c for c in env.sim.calls if c[0] != 'set_motor_cfg']


def test_registry_resolves_adaptive_controller():
    assert AddonFactory.get().addons['adaptive_controller'] is AdaptiveController
    assert not hasattr(AdaptiveController, 'compile')   # a hook addon: written on env.sim calls only
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'adaptive_controller' in readme and 'inverse_dynamics_regressor' in readme and 'inertial_parameters' in readme
    doc = AdaptiveController.__doc__
    assert 'persistent excitation' in doc and 'unmodelled dissipation' in doc


def test_spaces_and_configuration():
    env = _env()
    a = env.models['arm'].addons['adaptive']
    assert isinstance(a, AdaptiveController) and a in env._hook_addons
    sp = env.action_space.spaces['arm'].spaces['adaptive'].spaces
    assert [(k, tuple(v.shape), float(v.low.min()), float(v.high.max())) for k, v in sp.items()] == [('target', (6, ), float(np.float32(-0.05)), float(np.float32(0.05)))]
    assert a.target is None and a.lam.tolist() == [10.0] * 6 and a.damping.tolist() == DAMPING
    assert (a.adapt_gain, a.scale_limits, a.reset_estimate, a.clip_torque) == (0.3, [0.05, 20.0], True, True)

    def edit(c):
        del c['damping']
        c.update({'lambda': [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], 'adapt_gain': 0.0, 'scale_limits': [0.5, 2.0], 'reset_estimate': False, 'clip_torque': False, 'target': REST})
    b = _env(edit).models['arm'].addons['adaptive']
    assert b.lam.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0] and b.damping.tolist() == [20.0] * 6 and b.target == REST
    assert (b.adapt_gain, b.scale_limits, b.reset_estimate, b.clip_torque) == (0.0, [0.5, 2.0], False, False)


def test_the_calls_of_a_tick_their_arguments_and_the_two_laws_on_fixed_numbers():
    def edit(c):
        c.update(clip_torque=False, target=REST)
    env = _env(edit)
    arm = env.models['arm']; a = arm.addons['adaptive']
    L = env.layout
    calls = _tick(env)
    assert [c[0] for c in calls] == ['inertial_parameters', 'joint_states', 'inverse_dynamics_regressor', 'apply_joint_torque']
    assert calls[0][1:] == (arm.uid, True)   # the NOMINAL parameters, once
    _, body, q, qd, qdd, qd_ref, theta, s, want = calls[2]
    assert body == arm.uid and want == ('tau', 'grad')
    assert all(tuple(t.shape) == (2, 6) and t.dtype == torch.float32 and t.is_contiguous() for t in (q, qd, qdd, qd_ref, s))
    assert tuple(theta.shape) == (2, 6, 10) and theta.is_contiguous()
    dt = L.dt * L.substeps
    for e in range(2):
        # the joint state as the stand-in gave it (sums rounded in fp32: an ulp of 1.2 is 1.2e-7); the laws from those very numbers
        assert np.abs(q[e].numpy() - (Q_NOW + 0.001 * e)).max() < 3e-7 and np.abs(qd[e].numpy() - QD_NOW).max() < 3e-7
        qe, qde = q[e].double().numpy(), qd[e].double().numpy()
        err = qe - np.array(REST, dtype=np.float32)
        assert np.abs(qd_ref[e].numpy() - (-10.0 * err)).max() < 1e-5   # qd_r = -lambda e
        assert np.abs(qdd[e].numpy() - (-10.0 * qde)).max() < 1e-5      # qdd_r = -lambda qd
        sl = qde + 10.0 * err
        assert np.abs(s[e].numpy() - sl).max() < 1e-5                   # sl = qd - qd_r
        assert np.abs(theta[e].numpy() - THETA0).max() == 0             # s_hat = 1 at the start
        expect = TAU + e - np.array(DAMPING) * sl                       # tau = Y theta_hat - Kd sl
        assert np.abs(calls[3][2][e].double().numpy() - expect).max() < 1e-4 * np.abs(expect).max()
        step = (GRAD.astype(np.float64).reshape(6, 10) * (1.0 + e) * THETA0).sum(axis=1)
        assert np.abs(a.scale_estimate[e].double().numpy() - (1.0 - dt * 0.3 * step)).max() < 1e-6   # the update law
    # the second tick: three launches, and the regressor gets the new estimate
    s1 = a.scale_estimate.clone()
    calls = _tick(env)
    assert [c[0] for c in calls] == ['joint_states', 'inverse_dynamics_regressor', 'apply_joint_torque']
    assert torch.allclose(calls[1][6], s1[:, :, None] * torch.tensor(THETA0), rtol=1e-6)
    assert not torch.equal(a.scale_estimate, s1)
    env.sim.calls = []
    env.step({})   # an addon that is not named in the action is not updated
    assert not env.sim.calls


def test_adapt_gain_zero_freezes_the_estimate_and_the_clamp_holds():
    def frozen(c):
        c.update(adapt_gain=0.0)
    env = _env(frozen)
    a = env.models['arm'].addons['adaptive']
    for _ in range(3):
        _tick(env)
    assert torch.equal(a.scale_estimate, torch.ones((2, 6)))

    def tight(c):
        c.update(scale_limits=[0.9, 1.1])
    env = _env(tight)
    a = env.models['arm'].addons['adaptive']
    env.sim.push = 1e4   # a gradient that would throw the estimate far outside
    _tick(env)
    s = a.scale_estimate
    assert float(s.min()) == pytest.approx(0.9) and float(s.max()) == pytest.approx(1.1) and bool(((s == s.min()) | (s == s.max())).all())


def test_the_target_accumulates_and_set_target_sets_it():
    def edit(c):
        c.update(target=REST)
    env = _env(edit)
    a = env.models['arm'].addons['adaptive']
    q0 = a.q_star.clone()
    assert torch.equal(q0, torch.tensor(REST).expand(2, 6))
    step = torch.tensor([[0.01, 0.0, -0.005, 0.0, 0.0, 0.02], [0.0, 0.002, 0.0, 0.0, -0.01, 0.0]])
    for k in range(4):
        _tick(env, step)
        assert torch.allclose(a.q_star, q0 + (k + 1) * step, atol=1e-6)   # the action is ADDED to a target that persists
    a.set_target(REST)
    assert torch.equal(a.q_star, q0)
    a.set_target([0.1] * 6, mask=[True, False])
    assert a.q_star[0].tolist() == pytest.approx([0.1] * 6) and torch.equal(a.q_star[1], q0[1])


def test_reset_switches_the_motors_off_once_and_honours_the_mask():
    env = _env(B=3)
    arm = env.models['arm']; a = arm.addons['adaptive']
    off = _named(env, 'set_motor_cfg')
    assert len(off) == 1 and (off[0][1][:6, 2] == 0).all() and (env.sim.motor_cfg()[:6, 2] == 0).all()
    assert a._effort.tolist() == [j.effort for j in arm.robot.joints if j.q_index > -1] and min(a._effort.tolist()) > 0
    # without `target` the pose the reset LEAVES is the target, read on the first tick after the reset
    assert a.target is None and bool(a._stale.all())
    _tick(env)
    pose = Q_NOW[None, :] + 0.001 * np.arange(3)[:, None]
    assert np.abs(a.q_star.numpy() - pose).max() < 1e-6 and not bool(a._stale.any())
    _tick(env)
    s = a.scale_estimate.clone()
    assert float((s - 1.0).abs().min()) > 0
    a.set_target([0.2] * 6)
    env.sim.moved = 0.5
    env.sim.calls = []
    env.reset(torch.tensor([False, True, False]))
    assert not _named(env, 'set_motor_cfg')
    assert torch.equal(a.scale_estimate[1], torch.ones(6)) and torch.equal(a.scale_estimate[0], s[0]) and torch.equal(a.scale_estimate[2], s[2])   # only the masked env's
    assert a.q_star[1].tolist() == pytest.approx([0.2] * 6)   # until the tick after the reset
    _tick(env)
    assert np.abs(a.q_star[1].numpy() - (pose[1] + 0.5)).max() < 1e-6 and a.q_star[0].tolist() == pytest.approx([0.2] * 6)
    assert not _named(env, 'inertial_parameters')   # theta0 is read once

    def keep(c):
        c.update(reset_estimate=False)
    env = _env(keep, B=3)
    a = env.models['arm'].addons['adaptive']
    _tick(env)
    s = a.scale_estimate.clone()
    env.reset(torch.tensor([True, True, True]))
    assert torch.equal(a.scale_estimate, s)


def test_clip_torque_clamps_the_applied_torque():
    def edit(c):
        c.update(damping=1e6)
    env = _env(edit)
    a = env.models['arm'].addons['adaptive']
    calls = _tick(env)
    eff = np.array(a._effort.tolist())
    tau = calls[-1][2].numpy()
    assert (np.abs(tau) <= eff + 1e-4).all() and (np.abs(np.abs(tau) - eff) < 1e-4).any()


def test_configuration_errors():
    for key, value, text in (('target', [0.0, 0.0], 'target must have 6'), ('lambda', [1.0, 2.0], 'lambda must be a number or have 6'),
                             ('damping', [1.0, 2.0], 'damping must be a number or have 6'), ('lambda', 0.0, 'lambda must be > 0'),
                             ('damping', -1.0, 'damping >= 0'), ('adapt_gain', -0.1, 'adapt_gain must be >= 0'),
                             ('scale_limits', [2.0, 3.0], 'scale_limits must be'), ('scale_limits', [0.5], 'scale_limits must be')):
        def edit(c, key=key, value=value):
            c[key] = value
        with pytest.raises(ValueError, match=text):
            _env(edit)
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_adaptive.yaml')))
    tree['adaptive'] = {'addon': 'adaptive_controller'}
    cfg = Configuration.from_dict('ur_adaptive', tree); cfg.source_dir = GOLDEN
    with pytest.raises(ValueError, match='goes on a model'):
        DIYGym(cfg, num_envs=2, backend_factory=_Backend)


def test_the_example_scene_builds_and_steps():
    env = DIYGym(os.path.join(ROOT, 'examples', 'ur_high_5', 'adaptive', 'ur_high_5_adaptive.yaml'), num_envs=2, backend_factory=_Backend)
    both = [env.models[k].addons['controller'] for k in ('ur5_l', 'ur5_r')]
    assert all(isinstance(a, AdaptiveController) and a.adapt_gain == 0.3 and a.damping.tolist() == DAMPING for a in both)
    assert (env.sim.motor_cfg()[:12, 2] == 0).all()   # both arms' motors off
    env.sim.calls = []
    zero = {'target': torch.zeros((2, 6))}
    env.step({'ur5_l': {'controller': zero}, 'ur5_r': {'controller': zero}})
    assert [c[0] for c in env.sim.calls] == ['inertial_parameters', 'joint_states', 'inverse_dynamics_regressor', 'apply_joint_torque'] * 2
    assert {c[1] for c in env.sim.calls} == {a.uid for a in both}
