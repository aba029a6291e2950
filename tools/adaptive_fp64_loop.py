"""The closed loop of tests/test_adaptive_controller_gpu.py in fp64 numpy, never calling the library: adaptive_controller's tick
(tests/adaptive_ref.py: tests/regressor_ref.py for the control law and the adaptation gradient) on tests/fd_ref.py as plant -- two
substeps of 1 / 480 with the torque held, joint damping on; no link damping and no effort clipping:

    python tools/adaptive_fp64_loop.py [steps] [envs] [--record]

The plants are the UR5s of tests/golden/regressor/ur_adaptive.yaml with the mass scales its dynamics_randomizer draws at seed 1 (read
from the CPU checker's state).  From the reset pose at rest towards the pose 0.3 x [0.3, -0.4, 0.5, 0.3, -0.3, 0.2] away it prints the
largest joint error every 60 steps with the estimate frozen (adapt_gain 0) and adapting (0.3), and the final estimate beside the
true scales.  --record writes scales and final errors to tests/golden/regressor/adaptive_fp64.json, which the GPU test reads.  A
few seconds per env and hundred steps: a tool, not a test."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import adaptive_ref as AR
import dynamics_ref as D
from diy_gym_amd import DIYGym
from oracle_backend import OracleBackend

args = [a for a in sys.argv[1:] if not a.startswith('--')]
steps, B = int(args[0]) if args else 480, int(args[1]) if len(args) > 1 else 8
REST = np.array([0.3, -1.0, 1.2, -0.5, 0.4, 0.1])
TARGET = REST + 0.3 * np.array([0.3, -0.4, 0.5, 0.3, -0.3, 0.2])
DAMPING = [100.0, 100.0, 50.0, 10.0, 10.0, 5.0]
env = DIYGym(os.path.join(ROOT, 'tests', 'golden', 'regressor', 'ur_adaptive.yaml'), num_envs=B, seed=1, backend_factory=OracleBackend)
model = env.models['arm']
robot, Tb, scales = model.robot, D.base_transforms(env, model.uid), D.mass_scales(env, model.uid)
h, substeps = float(env.layout.dt), int(env.layout.substeps)
record = {'steps': steps, 'scales': scales.tolist(), 'frozen': [], 'adapting': []}
for e in range(B):
    print('env %d: scales %s' % (e, np.round(scales[e], 3).tolist()), flush=True)
    for name, gain in (('frozen', 0.0), ('adapting', 0.3)):
        err, s_hat = AR.loop(robot, scales[e], REST, TARGET, steps, h, substeps, 10.0, DAMPING, gain, T_base=Tb[e], every=60)
        print('  %-8s max |q - q*| every 60 steps: %s%s' % (name, ' '.join('%.4f' % v for v in err),
                                                          '' if gain == 0 else '; estimate %s' % np.round(s_hat, 3).tolist()), flush=True)
        record[name].append(float(err[-1]))
if '--record' in sys.argv:
    with open(os.path.join(ROOT, 'tests', 'golden', 'regressor', 'adaptive_fp64.json'), 'w') as f:
        json.dump(record, f, indent=1)
