"""fp64 numpy reference of env.sim.calculate_forward_dynamics and env.sim.rollout_joint_dynamics (dg_world_forward_dynamics,
dg_world_rollout), built on tests/dynamics_ref.py; the library under test is never called.

  * ``fd``: ``qdd = solve(M(q), tau - d * qd - ID(q, qd, 0))`` with ``numpy.linalg.solve`` (LU with pivoting -- not the kernel's
    Cholesky), ``M = dynamics_ref.mass_matrix`` and ``ID = dynamics_ref.inverse_dynamics``; ``d`` the joints' URDF damping when
    ``joint_damping`` is on, else zero;
  * ``rollout``: for t = 0 .. T-1, ``qdd = fd(q, qd, tau[t]); qd += dt qdd; q += dt qd`` -- semi-implicit Euler, the step's order;
    row t of every output is the state AFTER step t + 1; ``pos`` is the world position of the point ``local_pos`` of the inertial
    frame of ``frame``'s child link at the NEW q (the point ``dynamics_ref.jacobian`` differentiates).
A model: no joint limits, motors, link damping or contacts.  tests/test_fd_ref.py pins it.
"""
import numpy as np

import dynamics_ref as D
from nphelpers import link_frames


def joint_damping(robot):
    """[n] URDF damping of the movable joints in q_index order."""
    out = np.zeros(robot.num_dofs)
    for j in robot.joints:
        if j.movable:
            out[j.q_index] = j.damping
    return out


def fd(robot, q, qd, tau=None, damping=False, g=(0.0, 0.0, -9.81), T_base=None, scale=None):
    """qdd [n]."""
    q, qd = np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64)
    tau = np.zeros_like(q) if tau is None else np.asarray(tau, dtype=np.float64)
    M = D.mass_matrix(robot, q, T_base, scale)
    h = D.inverse_dynamics(robot, q, qd, np.zeros_like(q), g, T_base, scale)
    d = joint_damping(robot) if damping else 0.0
    return np.linalg.solve(M, tau - d * qd - h)


def point(robot, q, frame, local_pos=(0.0, 0.0, 0.0), T_base=None):
    """World position of ``local_pos`` of the inertial frame of the child link of joint ``frame``."""
    link = robot.joints[frame].child
    T, _ = link_frames(robot, np.asarray(q, dtype=np.float64), T_base)
    return (T[link] * robot.links[link].inertial_origin).apply(local_pos)


def rollout(robot, q0, qd0, tau, dt, damping=False, frame=None, local_pos=(0.0, 0.0, 0.0), g=(0.0, 0.0, -9.81), T_base=None, scale=None):
    """``tau`` [T, n] -> ``(q [T, n], qd [T, n], pos [T, 3] or None)`` of ONE sample."""
    q, qd = np.array(q0, dtype=np.float64), np.array(qd0, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    T = tau.shape[0]
    qs, qds = np.zeros((T, q.size)), np.zeros((T, q.size))
    pos = None if frame is None else np.zeros((T, 3))
    for t in range(T):
        qd = qd + dt * fd(robot, q, qd, tau[t], damping, g, T_base, scale)
        q = q + dt * qd
        qs[t], qds[t] = q, qd
        if pos is not None:
            pos[t] = point(robot, q, frame, local_pos, T_base)
    return qs, qds, pos
