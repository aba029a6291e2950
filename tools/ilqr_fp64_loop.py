"""The closed loop of tests/test_ilqr_controller_gpu.py in fp64 numpy, never calling the library: ilqr_controller's tick (tests/ilqr_ref.py's
ilqr_iteration with the addon's defaults: horizon 32, dt one env step, one iteration, the line search [1, 0.5, 0.25, 0.125], the clamp at
the URDF's effort limits) on tests/fd_ref.py as plant -- two substeps of 1 / 480 with the torque held, joint damping on:

    python tools/ilqr_fp64_loop.py [ticks]

Prints the largest joint error over its start every ten ticks for the arm of tests/golden/ur_admittance.yaml started
q* + [0.3, -0.2, 0.25, 0.2, -0.3, 0.2] at rest.  About ten minutes of central differences for 120 ticks: a tool, not a test."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import dynamics_ref as D
import fd_ref as FD
import ilqr_ref as IL
import lqr_ref as LQ
from diy_gym_amd import DIYGym
from oracle_backend import OracleBackend

ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 120
env = DIYGym(os.path.join(ROOT, 'tests', 'golden', 'ur_admittance.yaml'), num_envs=1, seed=5, backend_factory=OracleBackend)
model = env.models['arm']
robot, Tb = model.robot, D.base_transforms(env, model.uid)[0]
G = (0.0, 0.0, -9.81)
q_star = np.array([0.3, -1.0, 1.2, -0.5, 0.4, 0.1])
q, qd = q_star + np.array([0.3, -0.2, 0.25, 0.2, -0.3, 0.2]), np.zeros(6)
h, substeps, T = 1.0 / 480.0, 2, 32
limit = np.where(np.isfinite(LQ.effort_limits(robot)), LQ.effort_limits(robot), 0.0)
e0 = np.abs(q - q_star).max()
U = None
for tick in range(1, ticks + 1):
    tau_g = D.inverse_dynamics(robot, q, np.zeros(6), np.zeros(6), G, Tb)
    if U is None:
        U = np.tile(tau_g, (T, 1))
    it = IL.ilqr_iteration(robot, q, qd, U, q_star, tau_g, h * substeps, tau_limit=limit, g=G, T_base=Tb)
    U = it.U
    tau = np.where(limit > 0, np.clip(U[0], -limit, limit), U[0])
    for _ in range(substeps):
        qd = qd + h * FD.fd(robot, q, qd, tau, True, G, Tb)
        q = q + h * qd
    U = np.vstack([U[1:], U[-1:]])
    if tick % 10 == 0 or tick == ticks:
        print('tick %3d: largest joint error %.4f x its start (alpha %s, cost %.4f)' % (tick, np.abs(q - q_star).max() / e0, it.alpha, it.cost), flush=True)
