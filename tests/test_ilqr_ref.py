"""Pins tests/ilqr_ref.py -- the fp64 reference of the feedback rollout, the LQ backward pass and one iLQR iteration -- so that it is
not the only witness of what the kernels must compute.  Runs on any host.

(a) With zero gains and no ``dtau`` ``feedback_rollout`` equals ``fd_ref.rollout`` exactly (the same arithmetic on the same torques).
(b) Stationary and with ``lx = lu = 0`` the backward pass is the Riccati iteration of tests/lqr_ref.py: ``-K[0] == lqr_ref.gain`` to
    1e-9 relative on the matrices of tests/test_lqr_controller_host.py, and its ``Vxx`` is that iteration's ``P``.
(c) An indefinite ``Quu`` (``luu = 0``, ``lxx_T = 0``: at t = T - 1 ``Quu`` is the zero matrix) reports ``status == T`` and zeros; a
    positive ``mu`` clears it.
(d) The prediction of one iLQR iteration is honest on the fp64 UR5: ur_admittance's arm, q* = [0.3, -1.0, 1.2, -0.5, 0.4, 0.1], started
    q* + [0.3, -0.2, 0.25, 0.2, -0.3, 0.2] at rest, T = 16, dt = 1 / 120, ilqr_controller's default weights, U0 the gravity
    compensation at the start, damping on, no clamp, mu = 0.  The cost goes 210.250000 -> 95.392749 -> 95.238497 -> 95.238366 with
    alpha = 1 each time; predicted / actual decrease 115.1 / 114.9, 0.1547 / 0.1543, 1.336e-4 / 1.313e-4.  Asserted: the costs to
    1e-5 relative and each actual / predicted ratio within [0.95, 1.02].
"""
import os

import numpy as np

import dynamics_ref as D
import fd_ref as FD
import ilqr_ref as IL
import lqr_ref as LQ
from diy_gym_amd import DIYGym
from oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
G = (0.0, 0.0, -9.81)
TARGET = np.array([0.3, -1.0, 1.2, -0.5, 0.4, 0.1])
OFFSET = np.array([0.3, -0.2, 0.25, 0.2, -0.3, 0.2])
COSTS = (210.250000, 95.392749, 95.238497, 95.238366)
# the matrices of tests/test_lqr_controller_host.py
_RNG = np.random.default_rng(0)
A_Q = -3.0 * np.eye(6) + _RNG.uniform(-0.5, 0.5, (6, 6))
A_V = -0.2 * np.eye(6) + _RNG.uniform(-0.05, 0.05, (6, 6))
_S = _RNG.uniform(-0.3, 0.3, (6, 6))
MINV = np.diag([0.3, 0.3, 0.8, 5.0, 6.0, 20.0]) + 0.1 * (_S + _S.T)


def arm():
    env = DIYGym(os.path.join(GOLDEN, 'ur_admittance.yaml'), num_envs=1, seed=5, backend_factory=OracleBackend)
    model = env.models['arm']
    return model.robot, D.base_transforms(env, model.uid)[0]


def test_zero_gains_and_no_direction_are_the_open_loop_rollout():
    robot, Tb = arm()
    rng = np.random.default_rng(1)
    q0, qd0, tau = rng.uniform(-1.0, 1.0, 6), rng.uniform(-1.0, 1.0, 6), rng.uniform(-3.0, 3.0, (5, 6))
    frame = [j.name for j in robot.joints].index('ee_fixed_joint')
    q, qd, pos = FD.rollout(robot, q0, qd0, tau, 1.0 / 240.0, True, frame, (0.03, -0.02, 0.05), G, Tb)
    ref = np.zeros((5, 6))
    for args in (dict(), dict(gain=np.zeros((5, 6, 12)), q_ref=ref, qd_ref=ref)):
        q1, qd1, u1, pos1 = IL.feedback_rollout(robot, q0, qd0, tau, 1.0 / 240.0, damping=True, frame=frame, local_pos=(0.03, -0.02, 0.05), g=G, T_base=Tb, **args)
        assert np.array_equal(q, q1) and np.array_equal(qd, qd1) and np.array_equal(pos, pos1) and np.array_equal(u1, tau)
    # ... and the terms do what they say, on one step by hand
    gain, lim = rng.uniform(-2.0, 2.0, (1, 6, 12)), np.array([1.0, 0.0, 1.0, 0.0, 50.0, 50.0])
    qr, vr, dtau = rng.uniform(-1.0, 1.0, (1, 6)), rng.uniform(-1.0, 1.0, (1, 6)), rng.uniform(-1.0, 1.0, (1, 6))
    _, _, u, _ = IL.feedback_rollout(robot, q0, qd0, tau[:1], 1.0 / 240.0, gain, qr, vr, dtau, 0.5, lim, True, g=G, T_base=Tb)
    raw = tau[0] + 0.5 * dtau[0] + gain[0] @ np.concatenate([q0 - qr[0], qd0 - vr[0]])
    assert np.abs(u[0] - np.where(lim > 0, np.clip(raw, -lim, lim), raw)).max() < 1e-14 and (np.abs(raw[[0, 2]]) > 1.0).any() and np.array_equal(u[0, [1, 3]], raw[[1, 3]])


def test_the_stationary_pass_without_gradients_is_the_riccati_iteration():
    h, s = 1.0 / 240.0, 2
    A, B = LQ.discretise(A_Q, A_V, MINV, h, s)
    Q, R = LQ.weights(6)
    for T in (1, 7, 100):
        K_ref = LQ.gain(A, B, Q, R, T)
        P = Q.copy()
        for _ in range(T):
            Kt = np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)
            P = Q + A.T @ P @ (A - B @ Kt)
        b = IL.lq_backward(A_Q, A_V, MINV, h, Q, R, Q, T=T, substeps=s)
        assert b.status == 0 and b.K.shape == (T, 6, 12) and b.k.shape == (T, 6)
        assert np.abs(-b.K[0] - K_ref).max() < 1e-9 * np.abs(K_ref).max()
        assert np.abs(b.Vxx - P).max() < 1e-9 * np.abs(P).max()
        assert np.abs(b.k).max() == 0 and np.abs(b.dV).max() == 0 and np.abs(b.Vx).max() == 0
        # one matrix per step, T copies: the same numbers
        c = IL.lq_backward(np.stack([A_Q] * T), np.stack([A_V] * T), np.stack([MINV] * T), h, np.stack([Q] * T), np.stack([R] * T), Q, substeps=s)
        assert np.array_equal(b.K, c.K) and np.array_equal(b.Vxx, c.Vxx)


def test_an_indefinite_quu_is_reported_and_mu_clears_it():
    h, T = 1.0 / 240.0, 5
    Q, _ = LQ.weights(6)
    zero_R, zero_T = np.zeros((6, 6)), np.zeros((12, 12))
    b = IL.lq_backward(A_Q, A_V, MINV, h, Q, zero_R, zero_T, T=T)
    assert b.status == T and not b.K.any() and not b.k.any() and not b.dV.any()
    c = IL.lq_backward(A_Q, A_V, MINV, h, Q, zero_R, zero_T, lx=np.ones(12), mu=1e-3, T=T)
    assert c.status == 0 and np.isfinite(c.K).all() and np.abs(c.K).max() > 0 and np.abs(c.k).max() > 0


def test_the_predicted_decrease_of_an_iteration_is_the_actual_one():
    robot, Tb = arm()
    q0, qd0 = TARGET + OFFSET, np.zeros(6)
    tau_g = D.inverse_dynamics(robot, q0, np.zeros(6), np.zeros(6), G, Tb)
    U = np.tile(tau_g, (16, 1))
    costs, ratios = [], []
    for _ in range(3):
        it = IL.ilqr_iteration(robot, q0, qd0, U, TARGET, tau_g, 1.0 / 120.0, T_base=Tb)
        assert it.alpha == 1.0 and it.back.status == 0
        costs += [it.cost_before] if not costs else []
        costs.append(it.cost)
        ratios.append((it.cost_before - it.cost) / it.predicted)
        U = it.U
    print('costs', ['%.6f' % c for c in costs], 'actual / predicted', ['%.4f' % r for r in ratios])
    assert np.abs(np.array(costs) / np.array(COSTS) - 1.0).max() < 1e-5, costs
    assert all(0.95 <= r <= 1.02 for r in ratios), ratios


def test_the_references_default_weights_are_the_addons():
    """WEIGHTS stands for ilqr_controller's defaults in (d) and in the GPU tests: read them off the addon."""
    from diy_gym_amd.addons.controllers import IlqrController
    env = DIYGym(os.path.join(GOLDEN, 'ilqr', 'ur_ilqr.yaml'), num_envs=1, backend_factory=OracleBackend)
    a = env.models['arm'].addons['ilqr']
    assert isinstance(a, IlqrController) and {k: getattr(a, k) for k in IL.WEIGHTS} == IL.WEIGHTS
