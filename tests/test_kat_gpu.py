"""The closed-form cases of tests/kat_cases.py on the HIP kernels, in every kernel form a scene can take.

Each run: 70 envs (one full 64-lane wavefront plus a tail of 6), every env with a parameter of its own, then 1 env; the world
is created under the form's DG_* switches and the run asserts that the form was taken.  Every error must stay below
``kat_cases.TOL`` -- fixed on the CPU from the closed forms and the two oracle builds (tests/test_kat_ref.py), never from what
the kernels give -- and the failure message names the worst env.  Env 0 of the 70 and the single env solve the same problem
and must agree within the same tolerance.
"""
import numpy as np
import pytest

import kat_cases as kc
from diy_gym_amd.backend import debug_plan

pytestmark = pytest.mark.gpu

LANES = [({}, None), ({'DG_MAX_LANES': '16'}, 16), ({'DG_MAX_LANES': '4'}, 4), ({'DG_MAX_LANES': '1'}, 1)]
GENERIC = ['free_fall', 'marbles_at_rest', 'pendulum_period', 'double_pendulum', 'velocity_motor_hold', 'rolling_marble', 'inelastic_collision',
           'fixed_constraint_pair', 'drone_thrust', 'force_torque_sensor', 'pendulum_whole_turns']
ARMS = ('arms_hold_against_gravity', 'arm_end_effector_pose')
NARROW = ('free_fall', 'marbles_at_rest', 'rolling_marble', 'inelastic_collision', 'drone_thrust', 'joint_limits')   # scenes with the 4 / 1 LDS modes
PAR = ['DG_NO_HELPER_WAVE', 'DG_NO_SPLIT_SWEEPS', 'DG_NO_EARLY_DYNAMICS']
RUNS = ([(c, sw, lanes) for c in GENERIC for sw, lanes in LANES] + [('joint_limits', sw, lanes) for sw, lanes in (LANES[0], LANES[3])] +
        [('arms_hold_against_gravity', sw, None) for sw in [{}] + [{v: '1'} for v in PAR]] +
        [('arm_end_effector_pose', sw, lanes) for sw, lanes in LANES[:2]])


def _id(run):
    case, sw, _ = run
    return case + '-' + ('_'.join('%s=%s' % kv for kv in sw.items()) or 'default')


def _check_form(case, sw, lanes, env, monkeypatch):
    sim = env.sim
    with monkeypatch.context() as m:
        for k, v in sw.items():
            m.setenv(k, v)
        plan = debug_plan(env.layout, sim.num_envs)   # what the planner decides under the same switches, field by field
    what = (case, sw, sim.num_envs, sim.lanes, sim.kernel_name)
    assert sim.lanes == plan['lanes'] and bool(plan['par']) == sim.par, what
    if case in ARMS and 'DG_MAX_LANES' not in sw:
        # the scene of the four-wavefront kernel; one wavefront per 64 envs without the helper wave
        assert sim.par == ('DG_NO_HELPER_WAVE' not in sw) and sim.lanes == 64, what
        assert sim.kernel_name.startswith('step_kernel_par' if sim.par else 'step_kernel<64>'), what
        assert (plan['split_pgs'] != 0) == (sim.par and 'DG_NO_SPLIT_SWEEPS' not in sw), what
        # (the planner starts the dynamics early only where update ops with IK precede them: under joint_controller early_dyn is
        # 0 with or without the switch, and that run repeats the default form)
        assert 'DG_NO_EARLY_DYNAMICS' not in sw or plan['early_dyn'] == 0, what
        return
    # generic step_kernel<LANES>: 64 envs per wavefront by default (32 for the three marbles), 16, and below that the lane-sliced
    # LDS modes 4 and 1 where the planner has them for the scene, the global workspace (lanes 0) where it has not
    want = {None: 32 if case == 'marbles_at_rest' else 64, 16: 16, 4: 4 if case in NARROW else 0, 1: 1 if case in NARROW else 0}[lanes]
    assert not sim.par and sim.lanes == want and sim.kernel_name == 'step_kernel<%d>' % want, what


@pytest.mark.parametrize('run', RUNS, ids=_id)
def test_closed_form_on_the_kernels(run, monkeypatch):
    case, sw, lanes = run
    base = kc.make_env_factory(device='cuda:0')
    made = []

    def make_env(cfg, B, **engine):
        with monkeypatch.context() as m:   # the switches are read while the world is created
            for k, v in sw.items():
                m.setenv(k, v)
            env = base(cfg, B, **engine)
        made.append(env)
        return env

    results = {}
    for B in (70, 1):
        del made[:]
        r = results[B] = kc.CASES[case](make_env, B)
        assert made, case
        for env in made:
            _check_form(case, sw, lanes, env, monkeypatch)
        print('%s %s x%d %s: %s' % (case, sw, B, made[0].sim.kernel_name, ' '.join('%s %.3g (env %d, tol %.3g)' % (k, v, r.env[k], kc.TOL[case][k]) for k, v in r.items())))
        assert set(r) == set(kc.TOL[case]), (set(r), set(kc.TOL[case]))
        bad = {k: 'error %.4g in env %d > %.4g' % (v, r.env[k], kc.TOL[case][k]) for k, v in r.items() if not v <= kc.TOL[case][k]}
        assert not bad, (case, sw, B, made[0].sim.kernel_name, bad)
    for k, v in results[70].same.items():   # the same problem at the head of a full wavefront and alone
        d = float(np.abs(np.asarray(v)[0] - np.asarray(results[1].same[k])[0]).max())
        assert d <= kc.TOL[case][k], (case, sw, k, d, kc.TOL[case][k])
