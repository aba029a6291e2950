"""fp64 numpy reference of the dynamics queries (env.sim.calculate_jacobian / calculate_inverse_dynamics / calculate_mass_matrix),
built on the URDF-tree helpers of tests/nphelpers.py; the library under test is never called.

Formulations (chosen to differ from the kernels', which sweep the flattened 1-DoF links tip to root):
  * the geometric Jacobian of a point given in a link's INERTIAL frame, column by column from ``link_frames`` and ``ancestors``;
  * M as the sum over URDF links of ``m Jv^T Jv + Jw^T I Jw`` (``mass_matrix_and_gravity``'s form, with a mass scale);
  * inverse dynamics in the projected Newton-Euler form: one root-to-tip pass over the URDF joints (fixed ones included) for
    each link's angular velocity, angular acceleration and origin acceleration in world axes -- the base accelerating at -g --
    then ``tau = sum over links of Jv^T (m a_com) + Jw^T (I alpha + omega x I omega)`` with the Jacobians at the link's centre of
    mass.  There is no tip-to-root pass.
tests/test_dynamics_ref.py pins all three against independent formulations.

``scale`` is the per-env mass scale of the dynamics_randomizer: one factor per DoF, applied to mass and inertia of every URDF
link that moves with that joint (the links a fixed joint hangs on it included) -- what ``Lane::link_inertia`` does to the
flattened link.
"""
import numpy as np

from diy_gym_amd.mathx import Transform
from diy_gym_amd.scene import K
from nphelpers import ancestors, link_frames


def carrier(robot):
    """URDF link name -> q_index of the movable joint the link moves with (-1: rigidly on the base)."""
    out = {robot.root: -1}
    for j in robot.joints:   # depth-first: the parent is there
        out[j.child] = j.q_index if j.movable else out[j.parent]
    return out


def _link_scale(robot, scale):
    car = carrier(robot)
    return {name: (1.0 if scale is None or car[name] < 0 else float(scale[car[name]])) for name in robot.links}


def _com_jacobians(robot, joints, anc, point):
    n = robot.num_dofs
    Jv, Jw = np.zeros((3, n)), np.zeros((3, n))
    for j, o, a in joints:
        if j.q_index in anc:
            if j.type == 'prismatic':
                Jv[:, j.q_index] = a
            else:
                Jv[:, j.q_index] = np.cross(a, point - o)
                Jw[:, j.q_index] = a
    return Jv, Jw


def jacobian(robot, q, frame, local_pos=(0.0, 0.0, 0.0), T_base=None):
    """(jac_t, jac_r) [3, n] in world axes of the point ``local_pos`` of the inertial frame of the child link of joint ``frame``
    (the pybullet link index)."""
    link = robot.joints[frame].child
    T, joints = link_frames(robot, q, T_base)
    point = (T[link] * robot.links[link].inertial_origin).apply(local_pos)
    return _com_jacobians(robot, joints, ancestors(robot, link), point)


def mass_matrix(robot, q, T_base=None, scale=None):
    n = robot.num_dofs
    T, joints = link_frames(robot, q, T_base)
    s = _link_scale(robot, scale)
    M = np.zeros((n, n))
    for name, link in robot.links.items():
        if link.mass <= 0 or name == robot.root:
            continue
        Tc = T[name] * link.inertial_origin
        Jv, Jw = _com_jacobians(robot, joints, ancestors(robot, name), Tc.p)
        M += s[name] * (link.mass * Jv.T @ Jv + Jw.T @ (Tc.R @ link.inertia @ Tc.R.T) @ Jw)
    return M


def inverse_dynamics(robot, q, qd, qdd, g=(0.0, 0.0, -9.81), T_base=None, scale=None):
    """tau [n] = M(q) qdd + C(q, qd) qd - G(q), G = sum of Jv^T m g (``mass_matrix_and_gravity``'s G)."""
    n = robot.num_dofs
    q, qd, qdd = (np.asarray(v, dtype=np.float64) for v in (q, qd, qdd))
    T, joints = link_frames(robot, q, T_base)
    s = _link_scale(robot, scale)
    # angular velocity, angular acceleration, acceleration of the link frame's origin
    kin = {robot.root: (np.zeros(3), np.zeros(3), -np.asarray(g, dtype=np.float64))}
    for j in robot.joints:
        w, al, a = kin[j.parent]
        r = T[j.child].p - T[j.parent].p
        a = a + np.cross(al, r) + np.cross(w, np.cross(w, r))
        if j.movable:
            ax = T[j.child].R @ j.axis
            if j.type == 'prismatic':
                a = a + ax * qdd[j.q_index] + 2.0 * np.cross(w, ax) * qd[j.q_index]
            else:
                al = al + ax * qdd[j.q_index] + np.cross(w, ax) * qd[j.q_index]
                w = w + ax * qd[j.q_index]
        kin[j.child] = (w, al, a)
    tau = np.zeros(n)
    for name, link in robot.links.items():
        if link.mass <= 0 or name == robot.root:
            continue
        w, al, a = kin[name]
        Tc = T[name] * link.inertial_origin
        c = Tc.p - T[name].p
        Iw = s[name] * (Tc.R @ link.inertia @ Tc.R.T)
        F = s[name] * link.mass * (a + np.cross(al, c) + np.cross(w, np.cross(w, c)))
        N = Iw @ al + np.cross(w, Iw @ w)
        Jv, Jw = _com_jacobians(robot, joints, ancestors(robot, name), Tc.p)
        tau += Jv.T @ F + Jw.T @ N
    return tau


# ---- reading a world's state (GPU tests) -----------------------------------------------------------------------------------
def base_transforms(env, body):
    """The base LINK frame of ``body`` in every env, from the state."""
    so = env.layout.body_state_off[body]
    st = env.sim.get_state().astype(np.float64)
    return [Transform.from_xyz_quat(row[so:so + 3], row[so + 3:so + 7]) for row in st]


def mass_scales(env, body):
    """[B, nv] mass scales of ``body``'s links in every env, from the state (1 where no dynamics_randomizer owns the link)."""
    I = env.layout.I
    first, n = env.layout.body_first_link[body], env.layout.body_n_links[body]
    LI = I[I[K.H_OFF_LINK_I]:I[K.H_OFF_LINK_I] + env.layout.n_links * K.LI_STRIDE].reshape(-1, K.LI_STRIDE)
    st = env.sim.get_state().astype(np.float64)
    out = np.ones((st.shape[0], n))
    for i in range(n):
        off = int(LI[first + i, K.LI_MASS_SCALE])
        if off >= 0:
            out[:, i] = st[:, off]
    return out


def joint_limits(robot):
    """[n, 2] lower / upper of the movable joints in q_index order (an unlimited joint: -pi .. pi)."""
    out = np.zeros((robot.num_dofs, 2))
    for j in robot.joints:
        if j.movable:
            out[j.q_index] = (j.lower, j.upper) if j.lower <= j.upper else (-np.pi, np.pi)
    return out
