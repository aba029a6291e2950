"""fp64 numpy reference of env.sim.rollout_joint_feedback and env.sim.lq_backward_pass (dg_world_rollout_feedback,
dg_world_lq_backward) and of one iLQR iteration of the ilqr_controller addon, built on tests/fd_ref.py, tests/ddq_ref.py,
tests/dynamics_ref.py and tests/lqr_ref.py; the library under test is never called.  tests/test_ilqr_ref.py pins it.

  * ``feedback_rollout``: ONE sample.  At the state q_t, qd_t BEFORE step t: ``tau = tau_ff[t] + alpha dtau[t] + gain[t] @ [q_t -
    q_ref[t]; qd_t - qd_ref[t]]``, clamped to ``+-tau_limit`` where that is > 0; then ``fd_ref.rollout``'s step.  A term that is
    None is absent.  Row t of q, qd, pos is the state AFTER step t + 1; row t of tau the torque applied in step t.
  * ``lq_backward``: from Vx = lx_T, Vxx = lxx_T for t = T-1 .. 0, with A, B = ``lqr_ref.discretise`` of the point of step t:
        Qx = lx + A^T Vx;  Qu = lu + B^T Vx;  Qxx = lxx + A^T Vxx A;  Qux = B^T Vxx A;  Quu = luu + B^T Vxx B
        k = -(Quu + mu I)^-1 Qu;  K = -(Quu + mu I)^-1 Qux        (numpy.linalg.cholesky; not positive definite -> status = t + 1)
        dV += (k . Qu, 0.5 k^T Quu k)
        Vx = Qx + K^T Quu k + K^T Qu + Qux^T k;  Vxx = sym(Qxx + K^T Quu K + K^T Qux + Qux^T K)
  * ``ilqr_iteration``: the nominal rollout of U, the derivatives at its T points (central differences, joint damping on), the
    backward pass, a line search over ``alphas`` that takes the FIRST alpha whose cost is below the nominal's.
    Cost: sum_t 0.5 (wq |q_t - q*|^2 + wv |qd_t|^2 + wu |u_t - tau_g|^2) + 0.5 (wqT |q_T - q*|^2 + wvT |qd_T|^2), the states of the sum
    those BEFORE step t.
"""
import collections

import numpy as np

import ddq_ref as DD
import fd_ref as FD
import lqr_ref as LQ

WEIGHTS = dict(q_weight=10.0, qd_weight=0.1, torque_weight=1e-4, terminal_q_weight=1000.0, terminal_qd_weight=10.0)   # ilqr_controller's defaults
LqBackward = collections.namedtuple('LqBackward', ['K', 'k', 'dV', 'status', 'Vx', 'Vxx'])


def feedback_rollout(robot, q0, qd0, tau_ff, dt, gain=None, q_ref=None, qd_ref=None, dtau=None, alpha=0.0, tau_limit=None, damping=False, frame=None,
                     local_pos=(0.0, 0.0, 0.0), g=(0.0, 0.0, -9.81), T_base=None, scale=None):
    """``(q [T, n], qd [T, n], tau [T, n], pos [T, 3] or None)`` of ONE sample."""
    q, qd = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    tau_ff = np.asarray(tau_ff, dtype=np.float64)
    T, n = tau_ff.shape
    qs, qds, taus = np.zeros((T, n)), np.zeros((T, n)), np.zeros((T, n))
    pos = None if frame is None else np.zeros((T, 3))
    for t in range(T):
        tau = tau_ff[t].copy()
        if dtau is not None:
            tau = tau + float(alpha) * np.asarray(dtau[t], dtype=np.float64)
        if gain is not None:
            tau = tau + np.asarray(gain[t], dtype=np.float64) @ np.concatenate([q - q_ref[t], qd - qd_ref[t]])
        if tau_limit is not None:
            lim = np.asarray(tau_limit, dtype=np.float64)
            tau = np.where(lim > 0, np.clip(tau, -lim, lim), tau)
        qd = qd + dt * FD.fd(robot, q, qd, tau, damping, g, T_base, scale)
        q = q + dt * qd
        qs[t], qds[t], taus[t] = q, qd, tau
        if pos is not None:
            pos[t] = FD.point(robot, q, frame, local_pos, T_base)
    return qs, qds, taus, pos


def _at(a, t, tail):
    """Row t of an array that is per step (``[T] + tail``) or one for every step (``tail``); None stays None."""
    if a is None:
        return None
    a = np.asarray(a, dtype=np.float64)
    return a if a.ndim == tail else (a[0] if a.shape[0] == 1 else a[t])


def lq_backward(A_q, A_v, Minv, dt, lxx, luu, lxx_T, lx=None, lu=None, lx_T=None, mu=0.0, T=None, substeps=1):
    """One env.  ``A_q, A_v, Minv`` ``[T, n, n]``, or ``[n, n]`` / ``[1, n, n]`` with ``T`` given; the running cost per step or one for
    every step likewise.  Returns ``LqBackward`` with K ``[T, n, m]``, k ``[T, n]``, dV ``[2]``, status, and the value function at
    t = 0.  After a failure K, k and dV are zeros."""
    A_q = np.asarray(A_q, dtype=np.float64)
    n = A_q.shape[-1]
    m = 2 * n
    if T is None:
        T = A_q.shape[0] if A_q.ndim == 3 else 1
    Vxx = np.array(lxx_T, dtype=np.float64)
    Vx = np.zeros(m) if lx_T is None else np.array(lx_T, dtype=np.float64)
    K, k, dV = np.zeros((T, n, m)), np.zeros((T, n)), np.zeros(2)
    stationary = A_q.ndim == 2 or A_q.shape[0] == 1
    if stationary:
        A, B = LQ.discretise(_at(A_q, 0, 2), _at(A_v, 0, 2), _at(Minv, 0, 2), dt, substeps)
    for t in range(T - 1, -1, -1):
        if not stationary:
            A, B = LQ.discretise(_at(A_q, t, 2), _at(A_v, t, 2), _at(Minv, t, 2), dt, substeps)
        l_x, l_u = _at(lx, t, 1), _at(lu, t, 1)
        Qx = A.T @ Vx + (0.0 if l_x is None else l_x)
        Qu = B.T @ Vx + (0.0 if l_u is None else l_u)
        Qxx = _at(lxx, t, 2) + A.T @ Vxx @ A
        Qux = B.T @ Vxx @ A
        Quu = _at(luu, t, 2) + B.T @ Vxx @ B
        reg = Quu + float(mu) * np.eye(n)
        try:
            if not np.isfinite(reg).all():
                raise np.linalg.LinAlgError('not finite')
            np.linalg.cholesky(reg)
        except np.linalg.LinAlgError:
            return LqBackward(np.zeros((T, n, m)), np.zeros((T, n)), np.zeros(2), t + 1, Vx, Vxx)
        k[t], K[t] = -np.linalg.solve(reg, Qu), -np.linalg.solve(reg, Qux)
        dV += (k[t] @ Qu, 0.5 * k[t] @ Quu @ k[t])
        Vx = Qx + K[t].T @ Quu @ k[t] + K[t].T @ Qu + Qux.T @ k[t]
        Vxx = Qxx + K[t].T @ Quu @ K[t] + K[t].T @ Qux + Qux.T @ K[t]
        Vxx = 0.5 * (Vxx + Vxx.T)
    return LqBackward(K, k, dV, 0, Vx, Vxx)


def cost(q0, qd0, q, qd, u, q_star, tau_g, w=WEIGHTS):
    """The cost of a rollout: ``q, qd`` ``[T, n]`` the states AFTER each step, ``u`` ``[T, n]`` the torques applied."""
    qs, qds = np.vstack([np.asarray(q0)[None], q]), np.vstack([np.asarray(qd0)[None], qd])
    run = 0.5 * (w['q_weight'] * ((qs[:-1] - q_star) ** 2).sum() + w['qd_weight'] * (qds[:-1] ** 2).sum() + w['torque_weight'] * ((u - tau_g) ** 2).sum())
    return run + 0.5 * (w['terminal_q_weight'] * ((qs[-1] - q_star) ** 2).sum() + w['terminal_qd_weight'] * (qds[-1] ** 2).sum())


def cost_terms(q0, qd0, q, qd, u, q_star, tau_g, w=WEIGHTS):
    """``(lxx [m, m], luu [n, n], lx [T, m], lu [T, n], lxx_T [m, m], lx_T [m])`` of ``cost`` along a rollout."""
    n = len(q0)
    qs, qds = np.vstack([np.asarray(q0)[None], q]), np.vstack([np.asarray(qd0)[None], qd])
    lxx = np.diag([w['q_weight']] * n + [w['qd_weight']] * n)
    lxx_T = np.diag([w['terminal_q_weight']] * n + [w['terminal_qd_weight']] * n)
    lx = np.hstack([w['q_weight'] * (qs[:-1] - q_star), w['qd_weight'] * qds[:-1]])
    lx_T = np.concatenate([w['terminal_q_weight'] * (qs[-1] - q_star), w['terminal_qd_weight'] * qds[-1]])
    return lxx, w['torque_weight'] * np.eye(n), lx, w['torque_weight'] * (u - tau_g), lxx_T, lx_T


IlqrIteration = collections.namedtuple('IlqrIteration', ['U', 'cost', 'cost_before', 'alpha', 'predicted', 'back', 'q', 'qd'])


def ilqr_iteration(robot, q0, qd0, U, q_star, tau_g, dt, alphas=(1.0, 0.5, 0.25, 0.125), w=WEIGHTS, mu=0.0, tau_limit=None, g=(0.0, 0.0, -9.81), T_base=None):
    """One iteration about the torque sequence ``U [T, n]``.  ``alpha`` is None (and U, cost unchanged) when no alpha lowers the cost
    or the backward pass failed; ``predicted`` is ``-(alpha dV[0] + alpha^2 dV[1])`` of the alpha taken."""
    q0, qd0, U = np.asarray(q0, dtype=np.float64), np.asarray(qd0, dtype=np.float64), np.asarray(U, dtype=np.float64)
    q, qd, u, _ = feedback_rollout(robot, q0, qd0, U, dt, tau_limit=tau_limit, damping=True, g=g, T_base=T_base)
    c0 = cost(q0, qd0, q, qd, u, q_star, tau_g, w)
    qs, qds = np.vstack([q0[None], q[:-1]]), np.vstack([qd0[None], qd[:-1]])   # the states BEFORE each step
    ds = [DD.derivatives(robot, qs[t], qds[t], u[t], True, g, T_base) for t in range(len(U))]
    lxx, luu, lx, lu, lxx_T, lx_T = cost_terms(q0, qd0, q, qd, u, q_star, tau_g, w)
    back = lq_backward(np.stack([d.dqdd_dq for d in ds]), np.stack([d.dqdd_dqd for d in ds]), np.stack([d.dqdd_dtau for d in ds]), dt, lxx, luu, lxx_T, lx, lu, lx_T, mu)
    if back.status == 0:
        for alpha in alphas:
            q1, qd1, u1, _ = feedback_rollout(robot, q0, qd0, u, dt, back.K, qs, qds, back.k, alpha, tau_limit, True, g=g, T_base=T_base)
            c1 = cost(q0, qd0, q1, qd1, u1, q_star, tau_g, w)
            if c1 < c0:
                return IlqrIteration(u1, c1, c0, alpha, -(alpha * back.dV[0] + alpha * alpha * back.dV[1]), back, q1, qd1)
    return IlqrIteration(u, c0, c0, None, 0.0, back, q, qd)
