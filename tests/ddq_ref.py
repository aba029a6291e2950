"""fp64 numpy reference of env.sim.forward_dynamics_derivatives (dg_world_dynamics_derivatives), built on tests/fd_ref.py and
tests/dynamics_ref.py; the library under test is never called.  The kernel's derivatives are analytic; these are central differences
of the fp64 model, a different way to the same numbers:

  * ``dqdd_dq``: central differences of ``fd_ref.fd`` with step 1e-5;
  * ``dqdd_dqd``: the same with step 1e-3 (qdd is quadratic in qd: the central difference is exact up to rounding);
  * ``dqdd_dtau``: ``inv(dynamics_ref.mass_matrix)``;
  * ``dtau_dq``, ``dtau_dqd``: the same differences of ``dynamics_ref.inverse_dynamics`` at FIXED qdd = fd(q, qd, tau), the second
    plus the damping diagonal.
tests/test_ddq_ref.py pins it.
"""
import collections

import numpy as np

import dynamics_ref as D
import fd_ref as FD

H_Q, H_QD = 1e-5, 1e-3
Derivs = collections.namedtuple('Derivs', ['qdd', 'dqdd_dq', 'dqdd_dqd', 'dqdd_dtau', 'dtau_dq', 'dtau_dqd'])


def central(f, x, h):
    """[len(f(x)), len(x)]: column j is (f(x + h e_j) - f(x - h e_j)) / 2 h."""
    x = np.asarray(x, dtype=np.float64)
    cols = []
    for j in range(x.size):
        e = np.zeros_like(x); e[j] = h
        cols.append((f(x + e) - f(x - e)) / (2.0 * h))
    return np.stack(cols, axis=1)


def derivatives(robot, q, qd, tau=None, damping=False, g=(0.0, 0.0, -9.81), T_base=None, scale=None, h_q=H_Q, h_qd=H_QD):
    """``Derivs`` of one point, every field fp64."""
    q, qd = np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64)
    tau = np.zeros_like(q) if tau is None else np.asarray(tau, dtype=np.float64)
    d = FD.joint_damping(robot) if damping else np.zeros(q.size)
    qdd = FD.fd(robot, q, qd, tau, damping, g, T_base, scale)
    return Derivs(qdd,
                  central(lambda x: FD.fd(robot, x, qd, tau, damping, g, T_base, scale), q, h_q),
                  central(lambda x: FD.fd(robot, q, x, tau, damping, g, T_base, scale), qd, h_qd),
                  np.linalg.inv(D.mass_matrix(robot, q, T_base, scale)),
                  central(lambda x: D.inverse_dynamics(robot, x, qd, qdd, g, T_base, scale), q, h_q),
                  central(lambda x: D.inverse_dynamics(robot, q, x, qdd, g, T_base, scale), qd, h_qd) + np.diag(d))
