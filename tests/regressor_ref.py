"""fp64 numpy reference of env.sim.inertial_parameters and env.sim.inverse_dynamics_regressor (dg_world_inertial_parameters,
dg_world_id_regressor), built on the URDF-tree helpers of tests/nphelpers.py; the library under test is never called.

Inverse dynamics is linear in the inertial parameters: ``tau = Y(q, qd, qdd) theta``.  A device link is a movable joint's child link
with every URDF link fixed to it merged; link ``l`` (its joint's q_index) has ten parameters in its own frame,

    theta_l = [m, m cx, m cy, m cz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz]

with ``c`` the centre of mass and ``I`` the inertia about the link frame's ORIGIN in link axes.  ``theta`` sums the URDF links a joint
carries, each moved into the carrier link's frame (the relative transforms go through fixed joints only, so they are constants).

``regressor`` is the Slotine-Li form: with a reference velocity ``qd_ref`` it is ``Y`` with ``Y theta = M qdd + C(q, qd) qd_ref - G`` for
the Christoffel ``C``, which is symmetric in ``(qd, qd_ref)``; ``qd_ref = qd`` (the default) gives the plain regressor.  Formulation
(chosen to differ from the kernel's two sweeps): one root-to-tip pass over the movable joints for ``w, w_r, al, a`` of each link in
world axes -- the base accelerating at -g -- the 6 x 10 matrix ``A_j`` of each link in link axes, then the PROJECTED form
``Y[:, 10 j : 10 j + 10] = [Jv_j^T R_j, Jw_j^T R_j] A_j`` with the Jacobians of link j's origin.  No tip-to-root pass.
tests/test_regressor_ref.py pins it.
"""
import numpy as np

import dynamics_ref as D
from nphelpers import ancestors, link_frames

SYM3 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))   # the order of Sym3: xx xy xz yy yz zz


def carrier_links(robot):
    """q_index -> name of the movable joint's child link (the device link's frame)."""
    return {j.q_index: j.child for j in robot.joints if j.movable}


def theta(robot, scale=None):
    """[n, 10] inertial parameters of the device links, ``scale`` [n] applied to all ten of a link's."""
    n = robot.num_dofs
    T, _ = link_frames(robot, np.zeros(n))   # (relative transforms through fixed joints do not depend on q)
    car, frame = D.carrier(robot), carrier_links(robot)
    out = np.zeros((n, 10))
    for name, link in robot.links.items():
        l = car[name]
        if l < 0 or link.mass <= 0:
            continue
        Tc = T[frame[l]].inverse() * T[name] * link.inertial_origin   # the link's inertial frame in the carrier's frame
        m, c = link.mass, Tc.p
        I = Tc.R @ link.inertia @ Tc.R.T + m * (c @ c * np.eye(3) - np.outer(c, c))
        out[l] += np.concatenate([[m], m * c, [I[a, b] for a, b in SYM3]])
    if scale is not None:
        out *= np.asarray(scale, dtype=np.float64).reshape(n, 1)
    return out


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def L(v):
    """3 x 6 with ``L(v) vec(I) = I v``, vec in Sym3's order."""
    out = np.zeros((3, 6))
    for k, (a, b) in enumerate(SYM3):
        out[a, k] += v[b]
        if a != b:
            out[b, k] += v[a]
    return out


def link_matrix(w, wr, al, a):
    """A [6, 10]: theta_j -> (force, moment about the link origin), all four vectors and the result in link axes."""
    A = np.zeros((6, 10))
    A[:3, 0] = a
    A[:3, 1:4] = skew(al) + 0.5 * (skew(w) @ skew(wr) + skew(wr) @ skew(w))
    A[3:, 1:4] = -skew(a)
    A[3:, 4:] = L(al) + 0.5 * (skew(w) @ L(wr) + skew(wr) @ L(w))
    return A


def regressor(robot, q, qd, qdd, qd_ref=None, g=(0.0, 0.0, -9.81), T_base=None):
    """Y [n, 10 n]."""
    n = robot.num_dofs
    q, qd, qdd = (np.asarray(v, dtype=np.float64) for v in (q, qd, qdd))
    qr = qd if qd_ref is None else np.asarray(qd_ref, dtype=np.float64)
    T, joints = link_frames(robot, q, T_base)
    zero = np.zeros(3)
    kin = {robot.root: (zero, zero, zero, -np.asarray(g, dtype=np.float64))}
    for j in robot.joints:
        w, wr, al, a = kin[j.parent]
        r = T[j.child].p - T[j.parent].p
        a = a + np.cross(al, r) + 0.5 * (np.cross(w, np.cross(wr, r)) + np.cross(wr, np.cross(w, r)))
        if j.movable:
            ax, i = T[j.child].R @ j.axis, j.q_index
            cv = 0.5 * (np.cross(w, ax) * qr[i] + np.cross(wr, ax) * qd[i])
            if j.type == 'prismatic':
                a = a + ax * qdd[i] + 2.0 * cv
            else:
                al = al + ax * qdd[i] + cv
                w, wr = w + ax * qd[i], wr + ax * qr[i]
        kin[j.child] = (w, wr, al, a)
    Y = np.zeros((n, 10 * n))
    for l, name in carrier_links(robot).items():
        R, p = T[name].R, T[name].p
        A = link_matrix(*(R.T @ v for v in kin[name]))
        anc = ancestors(robot, name)
        Jv, Jw = np.zeros((3, n)), np.zeros((3, n))
        for j, o, ax in joints:
            if j.q_index in anc:
                if j.type == 'prismatic':
                    Jv[:, j.q_index] = ax
                else:
                    Jv[:, j.q_index] = np.cross(ax, p - o)
                    Jw[:, j.q_index] = ax
        Y[:, 10 * l:10 * l + 10] = np.hstack([Jv.T @ R, Jw.T @ R]) @ A
    return Y
