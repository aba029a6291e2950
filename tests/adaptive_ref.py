"""fp64 numpy model of the adaptive_controller's closed loop, never calling the library: the addon's tick on tests/regressor_ref.py
(control law's model term ``Y theta_hat`` and adaptation gradient ``Y^T s``) with tests/fd_ref.py as plant -- ``substeps`` substeps of
``h`` with the torque held, the step's semi-implicit order, joint damping on.  A model: no link damping, no effort clipping, no joint
limits or motors.  tools/adaptive_fp64_loop.py prints its error curves and records the predictions the GPU test compares with."""
import numpy as np

import fd_ref as FD
import regressor_ref as RR

G = (0.0, 0.0, -9.81)


def loop(robot, scale, q0, q_star, steps, h, substeps, lam=10.0, damping=20.0, adapt_gain=0.3, scale_limits=(0.05, 20.0), T_base=None, every=0):
    """``(errors, s_hat)``: max |q - q*| after each of ``steps`` env steps (``every`` > 0: only every that many and the last) from
    ``q0`` at rest, for a plant whose links weigh ``scale`` x the URDF's, and the final estimate."""
    n = robot.num_dofs
    q, qd = np.array(q0, dtype=np.float64), np.zeros(n)
    q_star, lam, kd = np.asarray(q_star, dtype=np.float64), np.broadcast_to(lam, (n, )), np.broadcast_to(damping, (n, ))
    theta0, s_hat = RR.theta(robot), np.ones(n)
    dt, errors = h * substeps, []
    for step in range(1, steps + 1):
        qd_r, qdd_r = -lam * (q - q_star), -lam * qd
        sl = qd - qd_r
        Y = RR.regressor(robot, q, qd, qdd_r, qd_r, G, T_base)
        tau = Y @ (s_hat[:, None] * theta0).reshape(-1) - kd * sl
        grad = (Y.T @ sl).reshape(n, 10)
        if adapt_gain > 0:
            s_hat = np.clip(s_hat - dt * adapt_gain * (grad * theta0).sum(axis=1), scale_limits[0], scale_limits[1])
        for _ in range(substeps):
            qd = qd + h * FD.fd(robot, q, qd, tau, True, G, T_base, scale)
            q = q + h * qd
        if not every or step % every == 0 or step == steps:
            errors.append(float(np.abs(q - q_star).max()))
    return np.array(errors), s_hat
