"""A discrete joint-space LQR in fp64 numpy: what the ``lqr_controller`` addon computes, on the reference model of tests/ddq_ref.py.
The library under test is never called.

Linearised at ``(q*, 0, tau_g(q*))`` with joint damping on: ``A_q = dqdd_dq``, ``A_v = dqdd_dqd``, ``Minv = dqdd_dtau``.  Per substep
h, the step's semi-implicit order (qd += h qdd; q += h qd), state x = [q - q*; qd]:
    A_h = [[I + h^2 A_q, h (I + h A_v)], [h A_q, I + h A_v]]      B_h = [[h^2 Minv], [h Minv]]
Over an env step of s substeps with the torque held: A = A_h^s, B = sum_{k < s} A_h^k B_h.  ``horizon`` backward Riccati iterations
from P = Q = diag(q_weight, qd_weight), R = torque_weight I:  K = (R + B^T P B)^-1 B^T P A;  P = Q + A^T P (A - B K).
"""
import numpy as np

import ddq_ref as DD
import dynamics_ref as D
import fd_ref as FD


def discretise(A_q, A_v, Minv, h, substeps):
    n = A_q.shape[0]
    I = np.eye(n)
    Ah = np.block([[I + h * h * A_q, h * (I + h * A_v)], [h * A_q, I + h * A_v]])
    Bh = np.vstack([h * h * Minv, h * Minv])
    A, B, Ak = np.eye(2 * n), np.zeros((2 * n, n)), np.eye(2 * n)
    for _ in range(substeps):
        B = B + Ak @ Bh
        Ak = Ak @ Ah
    return Ak, B


def gain(A, B, Q, R, horizon):
    P = Q.copy()
    K = np.zeros((B.shape[1], A.shape[0]))
    for _ in range(horizon):
        K = np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)
        P = Q + A.T @ P @ (A - B @ K)
    return K


def weights(n, q_weight=1000.0, qd_weight=10.0, torque_weight=0.001):
    Q = np.diag(np.concatenate([np.broadcast_to(np.asarray(q_weight, dtype=np.float64), (n, )), np.broadcast_to(np.asarray(qd_weight, dtype=np.float64), (n, ))]))
    return Q, np.diag(np.broadcast_to(np.asarray(torque_weight, dtype=np.float64), (n, )).copy())


def design(robot, q_star, h, substeps, horizon=100, g=(0.0, 0.0, -9.81), T_base=None, **w):
    """(K [n, 2n], tau_g [n], A, B) about q_star."""
    n = robot.num_dofs
    q_star = np.asarray(q_star, dtype=np.float64)
    tau_g = D.inverse_dynamics(robot, q_star, np.zeros(n), np.zeros(n), g, T_base)
    d = DD.derivatives(robot, q_star, np.zeros(n), tau_g, True, g, T_base)
    A, B = discretise(d.dqdd_dq, d.dqdd_dqd, d.dqdd_dtau, h, substeps)
    Q, R = weights(n, **w)
    return gain(A, B, Q, R, horizon), tau_g, A, B


def effort_limits(robot):
    out = np.full(robot.num_dofs, np.inf)
    for j in robot.joints:
        if j.movable and getattr(j, 'effort', 0.0) and j.effort > 0:
            out[j.q_index] = j.effort
    return out


def closed_loop(robot, q_star, q0, h, substeps, steps, K, tau_g, g=(0.0, 0.0, -9.81), T_base=None, clip=None):
    """The fp64 model under tau = tau_g - K [q - q*; qd], held over each env step; returns (q [steps + 1, n], largest |tau|)."""
    q, qd = np.array(q0, dtype=np.float64), np.zeros(robot.num_dofs)
    qs, tmax = [q.copy()], 0.0
    for _ in range(steps):
        tau = tau_g - K @ np.concatenate([q - q_star, qd])
        if clip is not None:
            tau = np.clip(tau, -clip, clip)
        tmax = max(tmax, float(np.abs(tau).max()))
        for _ in range(substeps):
            qd = qd + h * FD.fd(robot, q, qd, tau, True, g, T_base)
            q = q + h * qd
        qs.append(q.copy())
    return np.stack(qs), tmax
