"""fp64 numpy reference of env.sim.task_space_dynamics (dg_world_task_space), built on tests/dynamics_ref.py and the URDF-tree
helpers of tests/nphelpers.py; the library under test is never called.

For the point ``local_pos`` of the inertial frame of the child link of joint ``frame`` and the rows ``axes`` of ``[v; w]``:
  * ``jac``: the selected rows of ``dynamics_ref.jacobian``;
  * ``bias_acc`` (``Jdot qd``): one root-to-tip pass over the URDF joints (fixed ones included) at ``qdd = 0`` with the base at
    REST -- no fictitious gravity to take off again, unlike the kernel -- then ``a + al x r + w x (w x r)`` at the point, and ``al``;
  * ``bias_torque``: ``dynamics_ref.inverse_dynamics(q, qd, 0)``;
  * ``lambda``: ``A^-1`` of ``A = J M^-1 J^T + damping I`` with ``M = dynamics_ref.mass_matrix``, through the SAME factorisation
    rule as the kernel (``cholesky_floor``: a pivot <= 1e-5 x the largest diagonal entry becomes that floor and raises ``singular``;
    M is held to it in its Jacobi-scaled form, whose diagonal is all ones),
    because that rule is part of the contract; where no pivot comes near the floor this is the plain inverse
    (tests/test_task_space_ref.py checks ``lambda A = I``);
  * ``tau``: ``J^T lambda (acc - Jdot qd) + h + tau0 - J^T lambda J M^-1 tau0``, term by term as written;
  * ``point``: position, quaternion (xyzw) of the link's inertial frame, ``J qd``.
tests/test_task_space_ref.py pins these against independent forms.
"""
import numpy as np

import dynamics_ref as D
from nphelpers import link_frames

PIVOT_FLOOR = 1e-5


def cholesky_floor(A, own=False):
    """(L, hit): the lower factor of the symmetric matrix ``A`` with every pivot <= PIVOT_FLOOR x max diag(A) replaced by that
    floor; ``hit`` says whether one was.  ``own``: ``A`` is taken in its Jacobi-scaled form ``D^-1/2 A D^-1/2``, ``D = diag A``,
    whose diagonal is all ones -- pivot j is held against PIVOT_FLOOR x A[j, j]; the factor returned is A's own.  The mass matrix
    is factored that way (see ``tq_cholesky`` in dg_taskq.h for why)."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    hit = False
    for j in range(n):
        floor = PIVOT_FLOOR * (A[j, j] if own else np.max(np.diag(A)))
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > floor:
            d, hit = floor, True
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L, hit


def solve_factored(L, b):
    """``(L L^T)^-1 b`` by the two triangular solves."""
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def bias_acceleration(robot, q, qd, frame, local_pos, T_base=None):
    """``Jdot qd`` [6]: linear acceleration of the point and angular acceleration of its link at ``qdd = 0``, world axes."""
    q, qd = np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64)
    T, _ = link_frames(robot, q, T_base)
    kin = {robot.root: (np.zeros(3), np.zeros(3), np.zeros(3))}
    for j in robot.joints:
        w, al, a = kin[j.parent]
        r = T[j.child].p - T[j.parent].p
        a = a + np.cross(al, r) + np.cross(w, np.cross(w, r))
        if j.movable:
            ax = T[j.child].R @ j.axis
            if j.type == 'prismatic':
                a = a + 2.0 * np.cross(w, ax) * qd[j.q_index]
            else:
                al = al + np.cross(w, ax) * qd[j.q_index]
                w = w + ax * qd[j.q_index]
        kin[j.child] = (w, al, a)
    link = robot.joints[frame].child
    w, al, a = kin[link]
    r = (T[link] * robot.links[link].inertial_origin).apply(local_pos) - T[link].p
    return np.concatenate([a + np.cross(al, r) + np.cross(w, np.cross(w, r)), al])


def task_space(robot, q, qd, frame, local_pos=(0.0, 0.0, 0.0), axes=(0, 1, 2, 3, 4, 5), acc=None, tau_null=None, damping=0.0,
               g=(0.0, 0.0, -9.81), T_base=None, scale=None):
    """Every output of the query for one env, as a dict; ``tau`` only with ``acc``.  Also ``A``, ``M`` and ``cond_A`` (2-norm
    condition number of ``A``), which the tests scale their error measures with."""
    q, qd = np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64)
    axes = sorted(int(a) for a in axes)
    jt, jr = D.jacobian(robot, q, frame, local_pos, T_base)
    J6 = np.vstack([jt, jr])
    J = J6[axes]
    M = D.mass_matrix(robot, q, T_base, scale)
    h = D.inverse_dynamics(robot, q, qd, np.zeros_like(q), g, T_base, scale)
    ba = bias_acceleration(robot, q, qd, frame, local_pos, T_base)[axes]
    LM, hit_m = cholesky_floor(M, own=True)
    X = solve_factored(LM, J.T)
    A = J @ X + damping * np.eye(len(axes))
    LA, hit_a = cholesky_floor(A)
    lam = solve_factored(LA, np.eye(len(axes)))
    link = robot.joints[frame].child
    T, _ = link_frames(robot, q, T_base)
    Tc = T[link] * robot.links[link].inertial_origin
    out = {'jac': J, 'bias_acc': ba, 'bias_torque': h, 'lambda': lam, 'singular': int(hit_m or hit_a),
           'point': np.concatenate([Tc.apply(local_pos), Tc.quat, J6 @ qd]), 'A': A, 'M': M, 'cond_A': float(np.linalg.cond(A))}
    if acc is not None:
        tau = J.T @ (lam @ (np.asarray(acc, dtype=np.float64) - ba)) + h
        if tau_null is not None:
            t0 = np.asarray(tau_null, dtype=np.float64)
            tau = tau + t0 - J.T @ (lam @ (J @ solve_factored(LM, t0)))
        out['tau'] = tau
    return out
