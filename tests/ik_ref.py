"""fp64 numpy reference of env.sim.calculate_inverse_kinematics: the recursion of the compiled ik_controller op (damped least squares
in task space, the optional null-space projection, the per-iteration clamp, the early exit on the position residual), built on
``nphelpers.link_frames`` and ``dynamics_ref.jacobian``; the library under test is never called.

Formulation (chosen to differ from the kernel's, which factors the 6 x 6 normal matrix once and back-substitutes twice):
  * the task Jacobian J is [3 or 6, n] -- without an orientation target only the three position rows exist;
  * dq = J^T (J J^T + lambda^2 I)^-1 e by ``numpy.linalg.solve``;
  * with the four lists, dq += (I - J^T (J J^T + lambda^2 I)^-1 J) v0, the projector written out as a matrix;
  * the orientation error is the rotation vector of target x current^-1, from rotation matrices (the kernel works on quaternions).
tests/test_ik_ref.py pins the Jacobian, the damped solve and the convergence independently.

``params``: the engine parameters ``ik_*`` (``diy_gym_amd.scene.DEFAULTS`` unless overridden).  Without lists the damping is
``ik_joint_damping`` (pybullet's joint-space form (J^T J + d I) dq = J^T e, equal by the push-through identity), with lists
``ik_lambda_sq``.
"""
import numpy as np

import dynamics_ref as D
from diy_gym_amd.mathx import mat_from_quat
from diy_gym_amd.scene import DEFAULTS
from nphelpers import link_frames

PARAMS = ('ik_iterations', 'ik_lambda_sq', 'ik_joint_damping', 'ik_residual', 'ik_max_angle', 'ik_null_rest_gain', 'ik_null_limit_gain')


def params(**over):
    p = {k: DEFAULTS[k] for k in PARAMS}
    p.update(over)
    return p


def forward(robot, q, frame, T_base=None):
    """(position [3], rotation [3, 3]) of the INERTIAL frame of the child link of joint ``frame`` -- what
    ``frame_state(uid, frame, com=True)`` reports."""
    link = robot.joints[frame].child
    T = link_frames(robot, q, T_base)[0][link] * robot.links[link].inertial_origin
    return T.p, T.R


def rotation_vector(R):
    """axis x angle of the rotation R, angle in [0, pi]."""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(w), 0.5 * (np.trace(R) - 1.0)
    ang = np.arctan2(s, c)
    if s > 1e-9:
        return w * (ang / (2.0 * s))
    if c > 0:
        return 0.5 * w
    # a half turn: the axis is the eigenvector of eigenvalue 1
    A = 0.5 * (R + np.eye(3))
    k = int(np.argmax(np.diag(A)))
    ax = A[:, k] / np.sqrt(A[k, k])
    return ax * ang


def task_jacobian(robot, q, frame, use_orn, T_base=None):
    jt, jr = D.jacobian(robot, q, frame, (0.0, 0.0, 0.0), T_base)
    return np.vstack([jt, jr]) if use_orn else jt


def pose_error(robot, q, frame, target_pos, target_R, T_base=None):
    p, R = forward(robot, q, frame, T_base)
    ep = np.asarray(target_pos, dtype=np.float64) - p
    return ep if target_R is None else np.concatenate([ep, rotation_vector(target_R @ R.T)])


def null_velocity(q, lists, p):
    rest, lower, upper, rng = lists
    v0 = p['ik_null_rest_gain'] * (rest - q)
    v0 = v0 + np.where(q > upper, p['ik_null_limit_gain'] * (upper - q) / rng, 0.0)
    return v0 + np.where(q < lower, p['ik_null_limit_gain'] * (lower - q) / rng, 0.0)


def step(J, e, lam2, v0=None):
    """One damped-least-squares step in task space; with v0 the null-space term through the damped projector."""
    n = J.shape[1]
    U = J @ J.T + lam2 * np.eye(J.shape[0])
    dq = J.T @ np.linalg.solve(U, e)
    if v0 is not None:
        dq = dq + (np.eye(n) - J.T @ np.linalg.solve(U, J)) @ v0
    return dq


def solve(robot, frame, target_pos, target_orn=None, q0=None, lists=None, T_base=None, p=None, history=None):
    """(q [n], iterations).  ``target_orn``: unit quaternion xyzw or None; ``lists``: (rest, lower, upper, range) or None;
    ``history``: a list that receives the pose error vector at the start of every iteration."""
    p = p or params()
    q = np.array(q0, dtype=np.float64)
    target_R = None if target_orn is None else mat_from_quat(np.asarray(target_orn, dtype=np.float64))
    lists = None if lists is None else [np.asarray(v, dtype=np.float64) for v in lists]
    lam2 = p['ik_lambda_sq'] if lists is not None else p['ik_joint_damping']
    iters = 0
    for it in range(int(p['ik_iterations'])):
        e = pose_error(robot, q, frame, target_pos, target_R, T_base)
        if history is not None:
            history.append(e.copy())
        if it > 0 and np.linalg.norm(e[:3]) < p['ik_residual']:
            break
        iters += 1
        J = task_jacobian(robot, q, frame, target_R is not None, T_base)
        dq = step(J, e, lam2, None if lists is None else null_velocity(q, lists, p))
        mx = np.abs(dq).max()
        q = q + (p['ik_max_angle'] / mx if mx > p['ik_max_angle'] else 1.0) * dq
    return q, iters
