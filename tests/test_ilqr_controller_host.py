"""The ilqr_controller addon on the host: registry, spaces, configuration and its errors, the env.sim calls of a tick and every shape,
the line-search choice against numpy on fixed numbers, the mu schedule after a non-zero status, the shift of U, what reset() does with
env.reset_mask, the example scene; and lqr_controller's ``riccati: kernel``.  No GPU: the scene is built on the CPU checker, whose
backend has none of the queries, so a stand-in below answers them with fixed numbers and records the calls."""
import os

import numpy as np
import pytest
import torch
import yaml

import oracle_backend
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import AddonFactory
from diy_gym_amd.addons.controllers import IlqrController, LqrController, ilqr_line_search
from diy_gym_amd.backend import DynamicsDerivatives, FeedbackRollout, LqBackward
from diy_gym_amd.config import Configuration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ilqr')
TARGET = [0.3, -1.0, 1.2, -0.5, 0.4, 0.1]
GRAV = [0.0, -40.0, -12.0, -1.5, 0.1, 0.0]   # what the stand-in reports as the gravity compensation (+ e for env e)
Q_NOW = np.array(TARGET) + np.array([0.02, -0.01, 0.03, 0.0, -0.02, 0.01])   # ... and as the joint state (+ 0.001 e)
QD_NOW = np.array([0.1, 0.0, -0.2, 0.05, 0.0, 0.3])


class _Backend(oracle_backend.OracleBackend):
    """The checker plus the calls ilqr_controller and lqr_controller make, in the shapes HipBackend gives them.  A feedback rollout
    answers q = q0 + 0.01 (t + 1) (1 - better[k]), qd = 0 and tau = the torque it was given + alpha dtau: sample k costs less than the
    nominal (better[k] = 0 for it) exactly where ``self.better[e][k]`` says so."""
    status = None    # [B] what lq_backward_pass reports (None: zeros)
    better = None    # [B][K] 1 where the line search's sample k is to cost less than the nominal

    def _log(self, *call):
        self.calls = getattr(self, 'calls', []) + [call]

    def joint_states(self, body):
        self._log('joint_states', body)
        e = torch.arange(self.num_envs, dtype=torch.float32)[:, None]
        return (torch.tensor(Q_NOW, dtype=torch.float32).repeat(self.num_envs, 1) + 0.001 * e + getattr(self, 'moved', 0.0), torch.tensor(QD_NOW, dtype=torch.float32).repeat(self.num_envs, 1))

    def calculate_inverse_dynamics(self, body, q=None, qd=None, qdd=None):
        self._log('calculate_inverse_dynamics', body, None if q is None else q.clone(), None if qd is None else qd.clone(), qdd)
        return torch.tensor(GRAV, dtype=torch.float32).repeat(self.num_envs, 1) + torch.arange(self.num_envs, dtype=torch.float32)[:, None]

    def rollout_joint_feedback(self, body, tau, gain=None, q_ref=None, qd_ref=None, dtau=None, alphas=None, q0=None, qd0=None, dt=None, frame=None, local_pos=(0.0, 0.0, 0.0),
                               joint_damping=False, tau_limit=None, want=('q', 'qd', 'tau')):
        clone = lambda t: None if t is None else t.clone()
        self._log('rollout_joint_feedback', body, clone(tau), clone(gain), clone(q_ref), clone(qd_ref), clone(dtau), clone(alphas), clone(q0), clone(qd0), dt, joint_damping,
                  clone(tau_limit), tuple(want))
        B, T, nv = tau.shape
        K = 1 if alphas is None else len(alphas)
        a = torch.zeros(K) if dtau is None else alphas
        u = tau[:, None] + a[None, :, None, None] * (torch.zeros_like(tau) if dtau is None else dtau)[:, None]
        worse = torch.ones((B, K))
        if gain is not None and self.better is not None:
            worse = 1.0 - torch.tensor(self.better, dtype=torch.float32)
        if gain is not None and self.better is None:
            worse = torch.zeros((B, K))
        q = q0[:, None, None, :] + 0.01 * torch.arange(1, T + 1, dtype=torch.float32)[None, None, :, None] * worse[:, :, None, None]
        return FeedbackRollout(q.expand(B, K, T, nv).contiguous(), torch.zeros((B, K, T, nv)), u.contiguous(), None, None)

    def forward_dynamics_derivatives(self, body, q=None, qd=None, tau=None, joint_damping=False, want=('dqdd_dq', 'dqdd_dqd', 'dqdd_dtau')):
        self._log('forward_dynamics_derivatives', body, q.clone(), qd.clone(), tau.clone(), joint_damping, tuple(want))
        lead, nv = tuple(q.shape[:-1]), q.shape[-1]
        mats = [s * torch.eye(nv).expand(lead + (nv, nv)).contiguous() for s in (-3.0, -0.2, 2.0)]
        return DynamicsDerivatives(None, mats[0], mats[1], mats[2], None, None, None)

    def lq_backward_pass(self, body, A_q, A_v, Minv, dt, lxx, luu, lxx_T, lx=None, lu=None, lx_T=None, mu=None, horizon=None, substeps=1, want=('K', 'k', 'dV')):
        clone = lambda t: None if t is None else t.clone()
        self._log('lq_backward_pass', body, A_q.clone(), A_v.clone(), Minv.clone(), dt, lxx.clone(), luu.clone(), lxx_T.clone(), clone(lx), clone(lu), clone(lx_T), clone(mu),
                  horizon, substeps, tuple(want))
        B, nv = A_q.shape[0], A_q.shape[-1]
        T = horizon if horizon is not None else A_q.shape[1]
        K = torch.arange(B * T * nv * 2 * nv, dtype=torch.float32).reshape(B, T, nv, 2 * nv) * 1e-3
        status = torch.zeros(B, dtype=torch.int32) if self.status is None else torch.tensor(self.status, dtype=torch.int32)
        return LqBackward(K, 0.5 * torch.ones((B, T, nv)) if 'k' in want else None, -torch.ones((B, 2)) if 'dV' in want else None, status)

    def apply_joint_torque(self, body, torque):
        self._log('apply_joint_torque', body, torque.clone())

    def set_motor_cfg(self, cfg):
        self._log('set_motor_cfg', np.array(cfg, copy=True))
        super().set_motor_cfg(cfg)


def _env(edit=None, B=2, seed=0, scene='ur_ilqr.yaml', golden=GOLDEN, key='ilqr'):
    tree = yaml.safe_load(open(os.path.join(golden, scene)))
    if edit:
        edit(tree['arm'][key])
    cfg = Configuration.from_dict(scene[:-5], tree); cfg.source_dir = golden
    return DIYGym(cfg, num_envs=B, seed=seed, backend_factory=_Backend)


def _named(env, name):
    return [c for c in env.sim.calls if c[0] == name]


def _tick(env, target=None, key='ilqr'):
    env.sim.calls = []
    env.step({'arm': {key: {'target': torch.zeros((env.num_envs, 6)) if target is None else target}}})
    return [c for c in env.sim.calls if c[0] != 'set_motor_cfg']


def test_registry_resolves_ilqr_controller_and_the_readme_names_the_calls():
    assert AddonFactory.get().addons['ilqr_controller'] is IlqrController
    assert not hasattr(IlqrController, 'compile')   # a hook addon: written on env.sim calls only
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert all(word in readme for word in ('ilqr_controller', 'rollout_joint_feedback', 'lq_backward_pass', 'gpu_ilqr_time.py'))


def test_spaces_and_configuration():
    env = _env()
    a = env.models['arm'].addons['ilqr']
    assert isinstance(a, IlqrController) and a in env._hook_addons
    sp = env.action_space.spaces['arm'].spaces['ilqr'].spaces
    assert [(k, tuple(v.shape), float(v.low.min()), float(v.high.max())) for k, v in sp.items()] == [('target', (6, ), float(np.float32(-0.05)), float(np.float32(0.05)))]
    assert a.target == TARGET and (a.horizon, a.iterations, a.clip_torque, a.regularization) == (32, 1, True, 0.0) and a.line_search == [1.0, 0.5, 0.25, 0.125]
    assert (a.q_weight, a.qd_weight, a.torque_weight, a.terminal_q_weight, a.terminal_qd_weight) == (10.0, 0.1, 1e-4, 1000.0, 10.0)
    assert a.dt == pytest.approx(env.layout.dt * env.layout.substeps)   # the env step: the warm start's shift by one row is exact

    def edit(c):
        c.update(q_weight=1.0, qd_weight=0.5, torque_weight=0.1, terminal_q_weight=7.0, terminal_qd_weight=3.0, horizon=5, iterations=2, dt=0.01, line_search=[1.0, 0.3],
                 regularization=1e-3, clip_torque=False)
    b = _env(edit).models['arm'].addons['ilqr']
    assert (b.horizon, b.iterations, b.dt, b.line_search, b.regularization, b.clip_torque) == (5, 2, 0.01, [1.0, 0.3], 1e-3, False)
    assert torch.equal(torch.diagonal(b._lxx), torch.tensor([1.0] * 6 + [0.5] * 6)) and torch.equal(torch.diagonal(b._lxx_T), torch.tensor([7.0] * 6 + [3.0] * 6))
    assert torch.equal(b._luu, 0.1 * torch.eye(6)) and b.mu.tolist() == pytest.approx([1e-3, 1e-3])


def test_the_calls_of_a_tick_their_shapes_and_the_shift():
    def edit(c):
        c.update(horizon=5)
    env = _env(edit)
    arm = env.models['arm']; a = arm.addons['ilqr']
    uid, T = arm.uid, 5
    calls = _tick(env)
    assert [c[0] for c in calls] == ['joint_states', 'calculate_inverse_dynamics', 'rollout_joint_feedback', 'forward_dynamics_derivatives', 'lq_backward_pass',
                                     'rollout_joint_feedback', 'apply_joint_torque']
    js, grav, nom, lin, back, line, apply = calls
    q_now = torch.tensor(Q_NOW, dtype=torch.float32).repeat(2, 1) + 0.001 * torch.arange(2.0)[:, None]
    qd_now = torch.tensor(QD_NOW, dtype=torch.float32).repeat(2, 1)
    g = torch.tensor(GRAV).repeat(2, 1) + torch.arange(2.0)[:, None]
    assert all(c[1] == uid for c in calls)
    assert torch.equal(grav[2], q_now) and float(grav[3].abs().max()) == 0 and grav[4] is None   # calculate_inverse_dynamics(q, 0, 0)
    # the nominal rollout: U (after a reset the gravity compensation in every row), one sample, clamped, damping on, the env step
    _, _, tau, gain, q_ref, qd_ref, dtau, alphas, q0, qd0, dt, damping, limit, want = nom
    assert torch.equal(tau, g[:, None, :].expand(2, T, 6)) and gain is None and q_ref is None and dtau is None and alphas is None
    assert torch.equal(q0, q_now) and torch.equal(qd0, qd_now) and dt == a.dt and damping is True and torch.equal(limit, a._effort) and set(want) == {'q', 'qd', 'tau'}
    # the derivatives at the T states BEFORE each step and the torques applied
    _, _, q, qd, u, damping, want = lin
    assert q.shape == qd.shape == u.shape == (2, T, 6) and torch.equal(q[:, 0], q_now) and torch.equal(qd[:, 0], qd_now) and damping is True
    assert torch.allclose(q[:, 1:], q_now[:, None, :] + 0.01 * torch.arange(1, T)[None, :, None]) and torch.equal(u, tau)
    assert want == ('dqdd_dq', 'dqdd_dqd', 'dqdd_dtau')
    # the backward pass: the continuous derivatives as they came, the cost along the nominal
    _, _, A_q, A_v, Minv, dt, lxx, luu, lxx_T, lx, lu, lx_T, mu, horizon, substeps, want = back
    assert A_q.shape == A_v.shape == Minv.shape == (2, T, 6, 6) and float(A_q[0, 0, 0, 0]) == -3.0 and float(Minv[1, 2, 3, 3]) == 2.0
    assert dt == a.dt and substeps == 1 and horizon is None and set(want) == {'K', 'k', 'dV'}
    assert lxx.shape == lxx_T.shape == (12, 12) and luu.shape == (6, 6) and lx.shape == (2, T, 12) and lu.shape == (2, T, 6) and lx_T.shape == (2, 12) and mu.shape == (2, )
    q_star = torch.tensor(TARGET).expand(2, 6)
    assert torch.allclose(lx[:, :, :6], 10.0 * (q - q_star[:, None, :])) and torch.allclose(lx[:, :, 6:], 0.1 * qd) and float(lu.abs().max()) == 0   # (u = tau_g)
    q_T = q_now + 0.01 * T
    assert torch.allclose(lx_T[:, :6], 1000.0 * (q_T - q_star)) and float(lx_T[:, 6:].abs().max()) == 0 and float(mu.abs().max()) == 0
    # the line search: ONE call over all alphas, about the nominal, with the backward pass's K and k
    _, _, tau2, gain, q_ref, qd_ref, dtau, alphas, q0, qd0, dt, damping, limit, want = line
    assert torch.equal(tau2, u) and gain.shape == (2, T, 6, 12) and float(gain[0, 0, 0, 1]) == pytest.approx(1e-3) and torch.equal(q_ref, q) and torch.equal(qd_ref, qd)
    assert torch.equal(dtau, 0.5 * torch.ones((2, T, 6))) and alphas.tolist() == [1.0, 0.5, 0.25, 0.125] and torch.equal(q0, q_now) and torch.equal(limit, a._effort)
    # every sample stays at q0 (cheaper than the nominal, which drifts): alpha = 1 is taken, U = tau + k; its first row is applied, then U shifts
    new_U = g[:, None, :] + 0.5
    assert torch.allclose(apply[2], torch.minimum(new_U[:, 0], a._effort)) and apply[2].shape == (2, 6) and apply[2].dtype == torch.float32
    assert a.U.shape == (2, T, 6) and torch.allclose(a.U, new_U.expand(2, T, 6))
    assert a.last[1].tolist() == [True, True] and a.last[2].tolist() == [0, 0]
    # the shift: rows 1 .. T-1 move up, the last row is repeated
    a.U = torch.arange(2 * T * 6, dtype=torch.float32).reshape(2, T, 6).clone()
    before = a.U.clone()
    env.sim.better = [[0, 0, 0, 0], [0, 0, 0, 0]]   # no alpha improves: U stays the nominal
    calls = _tick(env)
    assert torch.equal(calls[2][2], before)   # the nominal rollout of U as it stood
    assert torch.equal(a.U[:, :-1], before[:, 1:]) and torch.equal(a.U[:, -1], before[:, -1]) and a.last[1].tolist() == [False, False]
    assert torch.equal(calls[-1][2], torch.minimum(torch.maximum(before[:, 0], -a._effort), a._effort))
    env.sim.calls = []
    env.step({})   # an addon that is not named in the action is not updated
    assert not env.sim.calls


def test_iterations_repeat_the_four_launches():
    def edit(c):
        c.update(horizon=3, iterations=3, clip_torque=False)
    env = _env(edit)
    calls = _tick(env)
    assert [c[0] for c in calls] == ['joint_states', 'calculate_inverse_dynamics'] + ['rollout_joint_feedback', 'forward_dynamics_derivatives', 'lq_backward_pass',
                                                                                     'rollout_joint_feedback'] * 3 + ['apply_joint_torque']
    assert calls[2][12] is None and calls[5][12] is None   # clip_torque off: no tau_limit
    assert torch.allclose(calls[6][2], calls[2][2] + 0.5)   # the second iteration starts from the first one's U


def test_the_line_search_takes_the_first_alpha_that_improves():
    cost0 = torch.tensor([10.0, 10.0, 10.0, 10.0, 10.0])
    costs = torch.tensor([[9.0, 8.0, 7.0, 6.0], [11.0, 10.0, 9.5, 9.0], [12.0, 11.0, 10.5, 10.0], [float('nan'), float('inf'), 9.9, 1.0], [1.0, 1.0, 1.0, 1.0]])
    status = torch.tensor([0, 0, 0, 0, 3], dtype=torch.int32)
    taken, index = ilqr_line_search(cost0, costs, status)
    c0, c, st = cost0.numpy(), costs.numpy(), status.numpy()
    want_taken = [bool(st[e] == 0 and (c[e] < c0[e]).any()) for e in range(5)]
    want_index = [int(np.argmax(c[e] < c0[e])) for e in range(5)]
    assert taken.tolist() == want_taken == [True, True, False, True, False]
    assert [i for i, t in zip(index.tolist(), want_taken) if t] == [i for i, t in zip(want_index, want_taken) if t] == [0, 2, 2]
    # ... and the controller takes that sample's torques per env
    def edit(c):
        c.update(horizon=4, clip_torque=False)
    env = _env(edit, B=3)
    a = env.models['arm'].addons['ilqr']
    env.sim.better = [[1, 1, 1, 1], [0, 0, 1, 1], [0, 0, 0, 0]]
    _tick(env)
    g = torch.tensor(GRAV).repeat(3, 1) + torch.arange(3.0)[:, None]
    assert a.last[1].tolist() == [True, True, False] and a.last[2].tolist()[:2] == [0, 2]
    assert torch.allclose(a.U[0], (g[0] + 0.5).expand(4, 6)) and torch.allclose(a.U[1], (g[1] + 0.25 * 0.5).expand(4, 6)) and torch.allclose(a.U[2], g[2].expand(4, 6))


def test_the_mu_schedule_after_a_failed_backward_pass():
    def edit(c):
        c.update(horizon=3, clip_torque=False)
    env = _env(edit, B=3)
    a = env.models['arm'].addons['ilqr']
    g = torch.tensor(GRAV).repeat(3, 1) + torch.arange(3.0)[:, None]
    env.sim.status = [0, 2, 0]
    _tick(env)
    assert a.mu.tolist() == pytest.approx([0.0, 1e-6, 0.0])   # max(10 mu, 1e-6) for the env that failed
    assert a.last[1].tolist() == [True, False, True] and torch.allclose(a.U[1], g[1].expand(3, 6))   # ... which keeps its U whatever the samples cost
    calls = _tick(env)
    assert _named(env, 'lq_backward_pass')[0][12].tolist() == pytest.approx([0.0, 1e-6, 0.0])   # the next tick's pass gets it
    assert a.mu.tolist() == pytest.approx([0.0, 1e-5, 0.0])
    env.sim.status = None
    _tick(env)
    assert a.mu.tolist() == pytest.approx([0.0, 1e-6, 0.0])   # ... and it decays by 10 after a success
    assert [c[0] for c in calls][-1] == 'apply_joint_torque'


def test_reset_switches_the_motors_off_once_and_honours_the_mask():
    def edit(c):
        c.update(horizon=3, regularization=1e-4)
    env = _env(edit, B=3)
    arm = env.models['arm']; a = arm.addons['ilqr']
    off = _named(env, 'set_motor_cfg')
    assert len(off) == 1 and (off[0][1][:6, 2] == 0).all() and (env.sim.motor_cfg()[:6, 2] == 0).all()
    assert a._effort.tolist() == [j.effort for j in arm.robot.joints if j.q_index > -1] and min(a._effort.tolist()) > 0
    _tick(env)
    _tick(env)
    a.set_target(torch.tensor([[0.0] * 6, [0.5] * 6, [1.0] * 6]))
    env.sim.status = [1, 1, 1]
    _tick(env)
    env.sim.status = None
    U, mu = a.U.clone(), a.mu.clone()
    g = torch.tensor(GRAV).repeat(3, 1) + torch.arange(3.0)[:, None]
    assert not torch.allclose(U[1], g[1].expand(3, 6)) and float(mu[1]) == pytest.approx(1e-5)   # 1e-4, two successes, one failure
    env.sim.calls = []
    env.reset(torch.tensor([False, True, False]))
    assert not _named(env, 'set_motor_cfg')
    assert a.q_star[0].tolist() == [0.0] * 6 and a.q_star[2].tolist() == [1.0] * 6 and torch.equal(a.q_star[1], torch.tensor(TARGET))   # only the masked env's
    assert float(a.mu[1]) == pytest.approx(1e-4) and torch.equal(a.mu[[0, 2]], mu[[0, 2]])
    calls = _tick(env)
    nominal = calls[2][2]   # the next tick's nominal rollout: the reset env's U is the gravity compensation again, the others' as they were
    assert torch.equal(nominal[1], g[1].expand(3, 6)) and torch.equal(nominal[0], U[0]) and torch.equal(nominal[2], U[2])
    a.set_target([0.1] * 6, mask=[True, False, False])
    assert a.q_star[0].tolist() == pytest.approx([0.1] * 6) and a.q_star[2].tolist() == [1.0] * 6

    # without `target` the pose the reset LEAVES is the target, read on the first tick after the reset, for the envs that reset only
    def free_edit(c):
        del c['target']
        c.update(horizon=3)
    free = _env(free_edit, B=3)
    f = free.models['arm'].addons['ilqr']
    assert f.target is None and not _named(free, 'joint_states') and bool(f._stale.all())
    _tick(free)
    pose = Q_NOW[None, :] + 0.001 * np.arange(3)[:, None]
    assert np.abs(f.q_star.numpy() - pose).max() < 1e-6 and not bool(f._stale.any())
    f.set_target([0.2] * 6)
    free.sim.moved = 0.5
    free.reset(torch.tensor([False, True, False]))
    assert f.q_star[1].tolist() == pytest.approx([0.2] * 6)   # until the tick after the reset
    _tick(free)
    assert np.abs(f.q_star[1].numpy() - (pose[1] + 0.5)).max() < 1e-6 and f.q_star[0].tolist() == pytest.approx([0.2] * 6)
    step = torch.tensor([[0.01, 0.0, -0.005, 0.0, 0.0, 0.02]] * 3)
    before = f.q_star.clone()
    _tick(free, step)
    assert torch.allclose(f.q_star, before + step, atol=1e-6)   # the action is ADDED to a target that persists


def test_configuration_errors():
    for key, value, text in (('target', [0.0, 0.0], 'target must have 6'), ('q_weight', -1.0, 'state weights must be >= 0'), ('terminal_qd_weight', -1.0, 'state weights must be >= 0'),
                             ('torque_weight', 0.0, 'torque_weight must be > 0'), ('horizon', 0, 'horizon and iterations'), ('iterations', 0, 'horizon and iterations'),
                             ('dt', 0.0, 'dt must be > 0'), ('line_search', [], 'line_search must be'), ('line_search', [1.0, 0.0], 'line_search must be'),
                             ('line_search', [2.0], 'line_search must be'), ('regularization', -1.0, 'regularization must be >= 0')):
        def edit(c, key=key, value=value):
            c[key] = value
        with pytest.raises(ValueError, match=text):
            _env(edit)
    tree = yaml.safe_load(open(os.path.join(GOLDEN, 'ur_ilqr.yaml')))
    tree['ilqr'] = {'addon': 'ilqr_controller'}
    cfg = Configuration.from_dict('ur_ilqr', tree); cfg.source_dir = GOLDEN
    with pytest.raises(ValueError, match='goes on a model'):
        DIYGym(cfg, num_envs=2, backend_factory=_Backend)
    env = DIYGym(os.path.join(GOLDEN, 'ur_ilqr.yaml'), num_envs=2, backend_factory=oracle_backend.OracleBackend)
    with pytest.raises((NotImplementedError, AttributeError), match='joint_states|OracleBackend'):
        env.step({'arm': {'ilqr': {'target': torch.zeros((2, 6))}}})


def test_the_example_scene_builds_and_steps():
    env = DIYGym(os.path.join(ROOT, 'examples', 'ur_high_5', 'ilqr', 'ur_high_5_ilqr.yaml'), num_envs=2, backend_factory=_Backend)
    both = [env.models[k].addons['controller'] for k in ('ur5_l', 'ur5_r')]
    assert all(isinstance(a, IlqrController) and a.horizon == 32 and a.iterations == 1 for a in both)
    assert (env.sim.motor_cfg()[:12, 2] == 0).all()   # both arms' motors off
    env.sim.calls = []
    zero = {'target': torch.zeros((2, 6))}
    env.step({'ur5_l': {'controller': zero}, 'ur5_r': {'controller': zero}})
    assert [c[0] for c in env.sim.calls] == ['joint_states', 'calculate_inverse_dynamics', 'rollout_joint_feedback', 'forward_dynamics_derivatives', 'lq_backward_pass',
                                             'rollout_joint_feedback', 'apply_joint_torque'] * 2
    assert {c[1] for c in env.sim.calls} == {a.uid for a in both}


def test_lqr_controller_takes_its_gains_from_the_kernel_when_asked():
    derivs = os.path.join(ROOT, 'tests', 'golden', 'derivs')

    def edit(c):
        c.update(riccati='kernel', horizon=7, clip_torque=False)
    env = _env(edit, scene='ur_lqr.yaml', golden=derivs, key='lqr')
    a = env.models['arm'].addons['lqr']
    assert isinstance(a, LqrController) and a.riccati == 'kernel'
    calls = _tick(env, key='lqr')
    assert [c[0] for c in calls] == ['calculate_inverse_dynamics', 'forward_dynamics_derivatives', 'lq_backward_pass', 'joint_states', 'apply_joint_torque']
    _, body, A_q, A_v, Minv, dt, lxx, luu, lxx_T, lx, lu, lx_T, mu, horizon, substeps, want = calls[2]
    L = env.layout
    assert body == env.models['arm'].uid and A_q.shape == (2, 6, 6) and float(A_q[0, 0, 0]) == -3.0 and float(A_v[0, 0, 0]) == pytest.approx(-0.2) and float(Minv[0, 0, 0]) == 2.0
    assert dt == float(L.dt) and substeps == int(L.substeps) == 2 and horizon == 7 and want == ('K', ) and lx is None and lu is None and lx_T is None and mu is None
    assert lxx.dtype == torch.float32 and torch.equal(lxx, torch.diag(torch.tensor([1000.0] * 6 + [10.0] * 6))) and torch.equal(lxx_T, lxx)
    assert torch.allclose(luu, 0.001 * torch.eye(6))
    K0 = (torch.arange(2 * 7 * 6 * 12, dtype=torch.float32).reshape(2, 7, 6, 12) * 1e-3)[:, 0]
    assert torch.equal(a.gain, -K0)   # -K[:, 0]
    x = torch.cat([torch.tensor(Q_NOW, dtype=torch.float32).repeat(2, 1) + 0.001 * torch.arange(2.0)[:, None] - torch.tensor(TARGET), torch.tensor(QD_NOW, dtype=torch.float32).repeat(2, 1)], dim=1)
    g = torch.tensor(GRAV).repeat(2, 1) + torch.arange(2.0)[:, None]
    assert torch.allclose(calls[-1][2], g + (K0 @ x[:, :, None])[:, :, 0], atol=1e-5)
    assert [c[0] for c in _tick(env, key='lqr')] == ['calculate_inverse_dynamics', 'joint_states', 'apply_joint_torque']
    # the default makes no such call
    plain = _env(scene='ur_lqr.yaml', golden=derivs, key='lqr')
    assert plain.models['arm'].addons['lqr'].riccati == 'torch'
    assert [c[0] for c in _tick(plain, key='lqr')] == ['calculate_inverse_dynamics', 'forward_dynamics_derivatives', 'joint_states', 'apply_joint_torque']
    with pytest.raises(ValueError, match='riccati must be torch or kernel'):
        _env(lambda c: c.update(riccati='numpy'), scene='ur_lqr.yaml', golden=derivs, key='lqr')
