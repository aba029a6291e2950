"""The planner's side of the skipped narrow phase (sc.np_skip, dg_plan.hip; substep_np_skip, dg_solver.h): in which worlds
a substep k >= 1 may go without its narrow phase and the pose pass in front of it, and the plan-time constant rho that turns
joint increments into an upper bound of how far a point of an arm moves.  No GPU: the device-free planner (dg_debug_plan).

rho_i of joint i is, over the shapes s on link j >= i of the chain, the largest of
    sum_{k = i+1 .. j} |LF_POS_k| + |centre of s in its link frame| + extent of s.
The check below does not restate that: it moves the arm in numpy (the link-table kinematics of
tests/test_narrow_phase_bounds.py) and measures how far the points the narrow phase's bounds are taken from have moved."""
import os

import numpy as np
import pytest

import oracle_backend
from test_narrow_phase_bounds import POINTS, SPHERE, Blob
from test_world_plan import CU, LDS_MAX, switch_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {
    'ur_ik': 'examples/ur_high_5/ur_high_5.yaml', 'ur_joint': 'examples/ur_high_5/ur_high_5_joint.yaml',
    'gripper': 'tests/golden/ur5_gripper.yaml', 'marbles': 'tests/golden/basic_env_nocam.yaml',
    'touching_ik': 'tests/golden/ur_arms_touching_ik.yaml',
}
_LAYOUTS = {}


def layout_of(name, update_freq=None):
    """The scene blob of `name`; update_freq = 240 gives the scene one substep per step (diy_gym.py: 1 / update_freq / timestep)."""
    import yaml
    import diy_gym_amd.examples  # noqa: F401  registers the example addons
    from diy_gym_amd import DIYGym
    from diy_gym_amd.config import Configuration
    key = (name, update_freq)
    if key not in _LAYOUTS:
        cfg = os.path.join(ROOT, CONFIGS[name])
        if update_freq is not None:
            tree = yaml.safe_load(open(cfg)); tree['update_freq'] = update_freq
            for v in tree.values():   # (model paths relative to the file's folder)
                if isinstance(v, dict) and 'model' in v and not os.path.isabs(v['model']) and os.path.exists(os.path.join(os.path.dirname(cfg), v['model'])):
                    v['model'] = os.path.join(os.path.dirname(cfg), v['model'])
            cfg = Configuration.from_dict(os.path.splitext(os.path.basename(cfg))[0], tree)
        _LAYOUTS[key] = DIYGym(cfg, num_envs=1, backend_factory=oracle_backend.OracleBackend).layout
    return _LAYOUTS[key]


def plan_of(monkeypatch, layout, num_envs, switches=()):
    from diy_gym_amd import backend
    for var in switch_table() + ['DG_NO_NP_SKIP']:
        monkeypatch.delenv(var, raising=False)
    for var in switches:
        monkeypatch.setenv(var, '1')
    return backend.debug_plan(layout, num_envs, CU)


@pytest.mark.parametrize('name', ['ur_ik', 'ur_joint'])
@pytest.mark.parametrize('num_envs', [67, 16384])
def test_two_six_axis_arms_skip(monkeypatch, name, num_envs):
    p = plan_of(monkeypatch, layout_of(name), num_envs)
    assert p['np_skip'] == 1
    assert p['par'] == 1 and p['coll_wave'] == 1 and p['coll_split'] == 1 and p['split_pgs'] > 0
    assert p['lds_bytes'] <= LDS_MAX and p['lds_bytes'] == p['total_slots'] * 64 * 4
    # the four slots are spare slots of the padding behind the velocity-change blocks: the plan is as large as without the feature
    off = plan_of(monkeypatch, layout_of(name), num_envs, ['DG_NO_NP_SKIP'])
    assert off['np_skip'] == 0
    assert off['lds_bytes'] == p['lds_bytes'] and off['total_slots'] == p['total_slots']
    assert {k: v for k, v in off.items() if k not in ('np_skip', 'table')} == {k: v for k, v in p.items() if k not in ('np_skip', 'table')}
    assert np.array_equal(off['table'], p['table'])


def test_the_switch_stands_beside_the_table():
    """DG_NO_NP_SKIP is read like the switches of DG_PLAN_SWITCHES but is not one of its entries (tests/test_world_plan.py pins that
    table, and README's list with it, at twenty): a field of PlanSwitches of its own, and a sentence below README's table."""
    assert 'DG_NO_NP_SKIP' not in switch_table()
    assert 'Switch no_np_skip;' in open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_plan.h')).read()
    text = open(os.path.join(ROOT, 'README.md')).read()
    section = text[text.index('### Environment switches'):]
    section = section[:section.index('\n#', 1)] if '\n#' in section[1:] else section
    assert '`DG_NO_NP_SKIP`' in section


def test_worlds_that_do_not_skip(monkeypatch):
    one = layout_of('ur_ik', update_freq=240)
    from diy_gym_amd.scene import K
    assert int(one.I[K.H_SUBSTEPS]) == 1 and int(layout_of('ur_ik').I[K.H_SUBSTEPS]) == 2
    assert plan_of(monkeypatch, one, 16384)['np_skip'] == 0            # no second substep
    assert plan_of(monkeypatch, layout_of('gripper'), 67)['np_skip'] == 0   # a tree
    assert plan_of(monkeypatch, layout_of('marbles'), 67)['np_skip'] == 0   # free bodies, no arm
    for sw in ('DG_NO_COLLIDE_SPLIT', 'DG_NO_COLLIDE_WAVE', 'DG_NO_SPLIT_SWEEPS', 'DG_NO_HELPER_WAVE'):
        assert plan_of(monkeypatch, layout_of('ur_ik'), 16384, [sw])['np_skip'] == 0, sw
    assert plan_of(monkeypatch, layout_of('ur_ik'), 16384, ['DG_NO_EARLY_DYNAMICS'])['np_skip'] == 1   # (ur_joint's order)


def rho_of(plan, n_links):
    return plan['table'][plan['rh_off']:plan['rh_off'] + n_links].view(np.float32).astype(np.float64)


def measured_points(blob, s):
    """The points of shape s, in its link frame, that the narrow phase's bounds are measured from: the centre of its bounding
    sphere, and both ends of the capsule the exact or the containing-capsule test uses (a hull: the fitted and the containing one)."""
    c, ax, prm = blob.centre(s), blob.rot(s)[:, 2], blob.prm(s)
    pts = [c]
    if blob.kind(s) != SPHERE:
        pts += [c - ax * prm[1], c + ax * prm[1]]
    if blob.kind(s) == POINTS:
        hh = float(blob.SF[s, blob.K.SF_HULL_HALF])
        pts += [c - ax * hh, c + ax * hh]
    return np.array(pts)


@pytest.mark.parametrize('name', ['ur_ik', 'touching_ik'])
def test_rho_bounds_the_motion_of_every_measured_point(monkeypatch, name):
    """2 000 random configurations of a UR5 inside its joint limits and joint increments up to the velocity clamp times the
    substep (signs and sizes random, some with every joint at the clamp): the centre of every shape's bounding sphere and both
    ends of its capsules move by no more than sum_i |dq_i| rho_i.  Every shape of both arms, no case left out; fp64 throughout, the
    planner's fp32 rho is rounded up."""
    layout = layout_of(name); blob = Blob(layout); K = blob.K
    plan = plan_of(monkeypatch, layout, 67)
    assert plan['np_skip'] == 1
    rho = rho_of(plan, len(blob.LI))
    h, vmax = float(blob.HF[K.HF_DT]), float(blob.HF[K.HF_MAX_COORD_VEL])
    rng = np.random.default_rng(9)
    arms = [plan['reg_body0'], plan['helper_body']]
    worst = 0.0; cases = 0
    for b in arms:
        first, n = int(blob.BI[b, K.BI_FIRST_LINK]), int(blob.BI[b, K.BI_N_LINKS])
        assert n == 6 and np.all(rho[first:first + n] > 0.0)
        assert np.all(np.diff(rho[first:first + n]) <= 1e-9)   # an inner joint carries everything an outer one does
        shapes = [s for s in range(len(blob.SI)) if blob.body_of(s) == b and int(blob.SI[s, K.SI_LINK]) >= 0]
        assert len(shapes) >= 6
        lo, hi = blob.joint_limits(b)
        for k in range(1000):
            q = rng.uniform(lo, hi)
            dq = rng.choice([-1.0, 1.0], size=n) * h * vmax * (1.0 if k % 10 == 0 else rng.uniform(0.0, 1.0, size=n))
            fa, fb = blob.link_frames(b, q), blob.link_frames(b, q + dq)
            bound = float(np.abs(dq) @ rho[first:first + n])
            for s in shapes:
                (Ra, pa), (Rb, pb) = blob.shape_frame(s, fa), blob.shape_frame(s, fb)
                pts = measured_points(blob, s)
                moved = np.linalg.norm((pts @ Rb.T + pb) - (pts @ Ra.T + pa), axis=1).max()
                # the bound of the joints that move this shape alone is tighter still; the full sum is what the kernel uses
                assert moved <= bound + 1e-12, (b, s, k, moved, bound)
                worst = max(worst, moved / bound if bound > 0 else 0.0)
                cases += 1
    print('%s: %d (configuration, shape) cases, largest motion / bound %.3f; rho %s' % (name, cases, worst, np.round(rho, 4).tolist()))
    assert cases >= 2000 * 6
