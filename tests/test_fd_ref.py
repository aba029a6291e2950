"""Pins tests/fd_ref.py -- the fp64 reference of the forward-dynamics and rollout queries -- so that it is not the only witness of
what the kernels must compute.  Runs on any host.

(a) ``ID(q, qd, fd(q, qd, tau)) == tau``: an fp64 round trip through two different code paths (a linear solve with M one way, the
    projected Newton-Euler sum the other).  Bound 1e-10 relative to the largest |tau|.
(b) A frictionless pendulum with tau = 0 conserves energy over 200 steps of dt = 1e-4 up to the drift of symplectic Euler.  The
    pendulum's M is constant, so H = p^2 / (2 M) + V(q) is separable, and ``qd += dt qdd(q); q += dt qd`` conserves the modified
    energy H~ = H - (dt / 2) qd V'(q) + O(dt^2) exactly (backward error analysis of the symplectic Euler method).  Hence
    |E_n - E_0| <= (dt / 2) (|qd V'|_n + |qd V'|_0) + O(dt^2) <= dt max|qd| max|V'|.  max|V'| is the largest gravity torque over
    the circle; max|qd| follows from the energy: sqrt(2 (E_0 - min V) / M).  The bound asserted is 1.5 x that (the O(dt^2) term:
    dt = 1e-4 leaves it four orders below the first).  An explicit-Euler rollout would gain energy monotonically at O(dt) PER UNIT
    TIME and still pass a bound of this form over so short a run, so the test also asserts the modified energy itself: H~ constant
    to dt^2 x the same scale.
(c) The SEMANTICS equal the step's: the CPU checker steps the scene with link damping 0 and motor force 0 from a state inside the
    limits and clear of contacts; the reference rollout runs with K = 1, dt = the substep, T = substeps x N, joint damping on.
    Both sides are fp64.  Measured here (N = 10): see MEASURED_C, the largest figure of the cases; the bound is 100 x that and never above 1e-6 relative.  The
    checker's state array takes a joint torque (the LS_TORQUE column, cleared by every step), so a constant-torque case is there
    too: the torque is written before each step and repeated per substep in the rollout.
"""
import os

import numpy as np
import pytest

import dynamics_ref as D
import fd_ref as FD
from diy_gym_amd import DIYGym
from diy_gym_amd.scene import K
from nphelpers import link_frames
from oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SCENES = {'pendulum': ('pendulum.yaml', 'pend'), 'double_pendulum': ('double_pendulum.yaml', 'dp'), 'cart_tree_fixed': ('cart_tree_fixed.yaml', 'cart'),
          'ur_admittance': ('ur_admittance.yaml', 'arm')}
G = (0.0, 0.0, -9.81)
# (c): the largest |checker - rollout| / largest |rollout| over q and qd, measured on this file's cases; bound 100 x, at most 1e-6
MEASURED_C = 5.69e-16   # (cart_tree_fixed with a torque; ur_admittance 3.97e-16, the pendulums 0 to 2.1e-16)
CASES_C = [(name, torque) for name in ('pendulum', 'double_pendulum', 'cart_tree_fixed', 'ur_admittance') for torque in (False, True)]


def scene(name, B=1, **kw):
    env = DIYGym(os.path.join(GOLDEN, SCENES[name][0]), num_envs=B, seed=5, backend_factory=OracleBackend, **kw)
    return env, env.models[SCENES[name][1]]


@pytest.mark.parametrize('name', sorted(SCENES))
def test_inverse_dynamics_of_forward_dynamics_is_the_torque(name):
    env, model = scene(name)
    robot, Tb = model.robot, D.base_transforms(env, model.uid)[0]
    rng = np.random.default_rng(sorted(SCENES).index(name) + 3)
    lim = D.joint_limits(robot)
    n = robot.num_dofs
    for k in range(12):
        q, qd, tau = rng.uniform(lim[:, 0], lim[:, 1]), rng.uniform(-2.0, 2.0, n), rng.uniform(-5.0, 5.0, n)
        scale = rng.uniform(0.5, 2.0, n) if k % 2 else None
        for damping in (False, True):
            qdd = FD.fd(robot, q, qd, tau, damping, G, Tb, scale)
            back = D.inverse_dynamics(robot, q, qd, qdd, G, Tb, scale) + (FD.joint_damping(robot) * qd if damping else 0.0)
            assert np.abs(back - tau).max() <= 1e-10 * np.abs(tau).max(), (name, k, damping)
    # tau = None is zero torque
    assert np.array_equal(FD.fd(robot, q, qd, None, False, G, Tb), FD.fd(robot, q, qd, np.zeros(n), False, G, Tb))


def test_a_frictionless_pendulum_conserves_energy_to_the_drift_of_symplectic_euler():
    env, model = scene('pendulum')
    robot, Tb = model.robot, D.base_transforms(env, model.uid)[0]
    assert robot.num_dofs == 1
    dt, T = 1e-4, 200

    def potential(q):
        frames, _ = link_frames(robot, np.array([q]), Tb)
        return -sum(link.mass * np.dot(G, (frames[name] * link.inertial_origin).p) for name, link in robot.links.items() if link.mass > 0 and name != robot.root)

    grid = np.linspace(-np.pi, np.pi, 721)
    M = float(D.mass_matrix(robot, np.zeros(1), Tb)[0, 0])
    assert all(abs(float(D.mass_matrix(robot, np.array([a]), Tb)[0, 0]) - M) < 1e-12 * M for a in grid[::60])   # constant: H is separable
    dV = lambda q: float(D.inverse_dynamics(robot, np.array([q]), np.zeros(1), np.zeros(1), G, Tb)[0])   # h(q, 0) = -G = V'(q)
    v_max, v_min = max(abs(dV(a)) for a in grid), min(potential(a) for a in grid)
    assert abs(dV(0.7) - (potential(0.7 + 1e-6) - potential(0.7 - 1e-6)) / 2e-6) < 1e-6 * v_max
    q0, qd0 = np.array([1.0]), np.array([0.5])
    qs, qds, _ = FD.rollout(robot, q0, qd0, np.zeros((T, 1)), dt, damping=False, g=G, T_base=Tb)
    energy = lambda q, qd: 0.5 * M * qd * qd + potential(q)
    E0 = energy(q0[0], qd0[0])
    qd_max = np.sqrt(2.0 * (E0 - v_min) / M) * 1.01   # (1 %: the numerical energy is E0 only to the drift bounded here)
    drift = max(abs(energy(qs[t, 0], qds[t, 0]) - E0) for t in range(T))
    bound = 1.5 * dt * qd_max * v_max
    print('pendulum: energy drift %.3g over %d steps of %g, bound %.3g' % (drift, T, dt, bound))
    assert 0 < drift <= bound
    # the modified energy is conserved one order better
    mod = lambda q, qd: energy(q, qd) - 0.5 * dt * qd * dV(q)
    drift2 = max(abs(mod(qs[t, 0], qds[t, 0]) - mod(q0[0], qd0[0])) for t in range(T))
    assert drift2 <= 0.05 * drift and drift2 <= dt * bound * 100
    # rows are the state AFTER each step, and a point rides along
    frame = [j.name for j in robot.joints].index('hinge')
    q1, qd1, p1 = FD.rollout(robot, q0, qd0, np.zeros((1, 1)), dt, frame=frame, local_pos=(0.0, 0.0, 0.1), g=G, T_base=Tb)
    qdd = FD.fd(robot, q0, qd0, None, False, G, Tb)
    assert np.allclose(qd1[0], qd0 + dt * qdd, rtol=0, atol=1e-15) and np.allclose(q1[0], q0 + dt * (qd0 + dt * qdd), rtol=0, atol=1e-15)
    assert np.array_equal(p1[0], FD.point(robot, q1[0], frame, (0.0, 0.0, 0.1), Tb))


@pytest.mark.parametrize('name,torque', CASES_C)
def test_the_rollout_is_the_checkers_step_without_limits_motors_and_contacts(name, torque):
    N = 10
    env, model = scene(name, B=1, engine={'linear_damping': 0.0, 'angular_damping': 0.0})
    robot, uid, L, sim = model.robot, model.uid, env.layout, env.sim
    n = robot.num_dofs
    cfg = sim.motor_cfg(); cfg[:, 2] = 0.0; sim.set_motor_cfg(cfg)   # motor force 0
    first = L.body_first_link[L.resolve_frame(uid, -1)[0]]
    off = [L.link_state_off[first + i] for i in range(n)]
    rng = np.random.default_rng(17)
    lim = D.joint_limits(robot)
    mid, half = 0.5 * (lim[:, 0] + lim[:, 1]), 0.5 * (lim[:, 1] - lim[:, 0])
    q0 = mid + 0.2 * half * rng.uniform(-1.0, 1.0, n) if name != 'ur_admittance' else np.array([0.3, -1.0, 1.2, -0.5, 0.4, 0.1])
    qd0 = rng.uniform(-0.3, 0.3, n)
    tau = rng.uniform(-1.0, 1.0, n) if torque else np.zeros(n)
    st = sim.get_state()
    for i in range(n):
        st[0, off[i] + K.LS_Q], st[0, off[i] + K.LS_QD] = q0[i], qd0[i]
    sim.set_state(st)
    Tb = D.base_transforms(env, uid)[0]
    for _ in range(N):
        if torque:
            st = sim.get_state()
            for i in range(n):
                st[0, off[i] + K.LS_TORQUE] = tau[i]
            sim.set_state(st)
        sim.step(0)
        assert sim.contacts(0) == 0
    st = sim.get_state()
    q_step, qd_step = np.array([st[0, o + K.LS_Q] for o in off]), np.array([st[0, o + K.LS_QD] for o in off])
    assert (q_step > lim[:, 0]).all() and (q_step < lim[:, 1]).all()   # the limit rows never woke
    T = L.substeps * N
    qs, qds, _ = FD.rollout(robot, q0, qd0, np.tile(tau, (T, 1)), L.dt, damping=True, g=G, T_base=Tb)
    assert np.abs(qs[-1] - q0).max() > 1e-4   # it moved
    err = max(np.abs(q_step - qs[-1]).max() / np.abs(qs).max(), np.abs(qd_step - qds[-1]).max() / np.abs(qds).max())
    print('%s torque=%s: checker against the rollout after %d steps (T = %d): %.3g relative' % (name, torque, N, T, err))
    assert err <= min(100 * MEASURED_C, 1e-6)
