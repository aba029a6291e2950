"""What dg_world_create decides about a world -- workspace mode, LDS plan, kernel form -- pinned without a GPU, through the
device-free planner (diy_gym_amd/csrc/dg_plan.h, dg_debug_plan).  The expected values are the project's own record: the
``sim.lanes`` assertions of tests/test_parity_gpu.py (same scenes, switches and batch sizes), DESIGN §3's mode table, the
modes and LDS sizes BENCH_r04.json recorded on an MI355X, and the switch effects README / DESIGN state.  Every case also
checks the invariants of the LDS plan.  ``cu_count`` is the MI355X's 256 throughout (what the GPU tests ran with)."""
import copy
import functools
import json
import os
import re

import pytest
import yaml

import oracle_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU = 256
LDS_MAX = 160 * 1024
# sizes of the LDS plan's blocks in slots (dg_kernels.h: pose = two columns of R + position, MR_STRIDE, CL_STRIDE, the 21 words
# of a packed articulated inertia)
R0_SLOTS, POSE_SLOTS, MROW_SLOTS, CL_STRIDE, IAACC_SLOTS = 6, 9, 6, 14, 21

CONFIGS = {
    'marbles': 'tests/golden/basic_env_nocam.yaml', 'drone': 'examples/drone_pilot/drone_pilot.yaml',
    'ur_ik': 'examples/ur_high_5/ur_high_5.yaml', 'ur_joint': 'examples/ur_high_5/ur_high_5_joint.yaml',
    'cart_tree': 'tests/golden/cart_tree.yaml', 'maze': 'examples/r2d2_maze/r2d2_maze.yaml',
    'readme': 'examples/from_the_readme/from_the_readme.yaml', 'child': 'tests/golden/ur5_child_gripper.yaml',
    'constrained': 'tests/golden/ur5_constrained_gripper.yaml', 'touching': 'tests/golden/ur_arms_touching.yaml',
    'touching_ik': 'tests/golden/ur_arms_touching_ik.yaml', 'stack': 'tests/golden/box_stack.yaml',
}
SMOOTH_CONTACTS = ('touching', )   # as tests/test_parity_gpu.py: these scenes keep the capsule narrow phase (hull_contacts = 0)
REF = dict(motor_guess=0.0, warmstart=0.85)
COLD = dict(motor_guess=0.0)
WARM = dict(warmstart=0.85, warmstart_friction=0.5)
CONVERGED = dict(residual_threshold=1e-13)


def switch_table():
    """Names of the PlanSwitches table (the X-macro of dg_plan.h)."""
    text = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_plan.h')).read()
    return re.findall(r'^\s*X\((DG_[A-Z0-9_]+),\s*\w+,\s*"', text, flags=re.M)


@functools.lru_cache(maxsize=None)
def _layout(name, engine_items, max_contacts, manifold):
    import diy_gym_amd.examples  # noqa: F401  registers propellor / fell_over
    from diy_gym_amd import DIYGym
    from diy_gym_amd.config import Configuration
    engine = dict(engine_items)
    if name in SMOOTH_CONTACTS:
        engine.setdefault('hull_contacts', 0.0)
    kw = {} if manifold is None else {'hull_manifold_points': manifold}
    cfg = os.path.join(ROOT, CONFIGS[name])
    if max_contacts is not None:
        tree = yaml.safe_load(open(cfg)); tree['max_contacts'] = max_contacts
        cfg = Configuration.from_dict(os.path.splitext(os.path.basename(cfg))[0], copy.deepcopy(tree))
    return DIYGym(cfg, num_envs=1, backend_factory=oracle_backend.OracleBackend, engine=engine, **kw).layout


def plan_of(monkeypatch, name, num_envs, switches=None, engine=None, max_contacts=None, manifold=None):
    from diy_gym_amd import backend
    from diy_gym_amd.scene import K
    switches = switches or {}
    for var in switch_table():
        monkeypatch.delenv(var, raising=False)
    for var, value in switches.items():
        monkeypatch.setenv(var, value)
    layout = _layout(name, tuple(sorted((engine or {}).items())), max_contacts, manifold)
    plan = backend.debug_plan(layout, num_envs, CU)
    check_invariants(plan, layout, K, num_envs, switches)
    return plan


def check_invariants(p, layout, K, num_envs, switches):
    I = layout.I
    nb, nl, maxc, ncons = (int(I[k]) for k in (K.H_N_BODIES, K.H_N_LINKS, K.H_MAX_CONTACTS, K.H_N_CONSTRAINTS))
    assert p['lds_bytes'] <= LDS_MAX
    if p['lanes'] > 0:
        assert p['lds_bytes'] == p['total_slots'] * p['lanes'] * 4   # ws[slot][lane] of floats
    PLB = p['table'][:nb * p['plb_stride']].reshape(nb, p['plb_stride'])
    PLL = p['table'][nb * p['plb_stride']:nb * p['plb_stride'] + nl * p['pll_stride']].reshape(nl, p['pll_stride'])
    regions = []
    for b in range(nb):
        r0, minv, dv, nv = (int(v) for v in PLB[b, :4])
        if r0 >= 0:
            regions.append((r0, R0_SLOTS, 'R0 of body %d' % b))
        regions += [(minv, nv * nv, 'MINV of body %d' % b), (dv, nv, 'DV of body %d' % b)]
    for l in range(nl):
        regions += [(int(PLL[l, 0]), POSE_SLOTS, 'POSE of link %d' % l), (int(PLL[l, 1]), MROW_SLOTS, 'MROW of link %d' % l)]
    regions.append((p['cont_off'], 1 + (maxc + 2 * ncons) * CL_STRIDE, 'contact list'))
    regions.append((p['tr_off'], p['tr_slots'], 'transient region'))
    if p['coll_split']:
        regions.append((p['cont2_off'], 1 + maxc * CL_STRIDE, 'second contact list'))
    regions = sorted(r for r in regions if r[1] > 0)
    for (a, na, what_a), (b, _, what_b) in zip(regions, regions[1:]):
        assert a >= 0 and a + na <= b, (what_a, a, na, what_b, b)
    assert regions[-1][0] + regions[-1][1] <= p['total_slots'], regions[-1]
    # inertia accumulators: inside the transient region, and those of one body apart from each other
    BI = I[I[K.H_OFF_BODY_I]:].reshape(-1)[:nb * K.BI_STRIDE].reshape(nb, K.BI_STRIDE)
    for b in range(nb):
        first, n = int(BI[b, K.BI_FIRST_LINK]), int(BI[b, K.BI_N_LINKS])
        acc = sorted(int(PLL[l, 2]) for l in range(first, first + n) if PLL[l, 2] >= 0)
        for a in acc:
            assert p['tr_off'] <= a and a + IAACC_SLOTS <= p['tr_off'] + p['tr_slots'], (b, a)
        for a, c in zip(acc, acc[1:]):
            assert a + IAACC_SLOTS <= c, (b, a, c)
    assert p['par'] or p['split_pgs'] <= 0
    assert not p['coll_split'] or p['coll_wave']
    assert not p['coll_wave'] or p['par']
    assert not p['early_dyn'] or p['coll_wave']
    if p['lanes'] == 1:
        assert num_envs <= 4 * CU or switches.get('DG_MAX_LANES') == '1'


def ML(v, **more):
    return dict({'DG_MAX_LANES': str(v)}, **{k: '1' for k in more})


WE, NN, NSG = 'DG_NO_WAVE_ENV', 'DG_NO_NARROW_MODES', 'DG_NO_SLICED_GLOBAL'

# (scene, switches, lanes, num_envs, engine, max_contacts): every triple the GPU tests assert on sim.lanes, with their batch
GPU_ASSERTED = (
    # test_limit_guess_in_the_dense_sweep_forms
    [('cart_tree', sw, lanes, 9, CONVERGED, None) for sw, lanes in
     [({}, 64), (ML(32), 32), (ML(16), 16), (ML(8), 8), (ML(8, DG_NO_REG_ROWS=1), 8), (ML(4), 4), (ML(1), 1)]] +
    # test_contact_budget_cuts_the_list_in_pair_order
    [('readme', sw, lanes, 5, {}, 7) for sw, lanes in [(ML(1), 1), (ML(16), 16), (ML(4), 4)]] +
    # test_alternative_workspace_modes
    [(name, sw, lanes, 9, {}, None) for name, sw, lanes in [
        ('cart_tree', ML(16), 16), ('cart_tree', ML(32), 32), ('cart_tree', ML(8), 8), ('cart_tree', ML(4), 4), ('marbles', ML(16), 16),
        ('marbles', ML(8), 8), ('maze', ML(8), 8), ('drone', ML(32), 32), ('drone', ML(16), 16), ('child', ML(16), 16), ('maze', ML(4), 4),
        ('constrained', ML(32), 32), ('constrained', ML(16), 16), ('maze', ML(4, DG_NO_MINV_SLICES=1), 4), ('maze', ML(1), 1),
        ('readme', ML(1), 1), ('readme', {WE: '1'}, 4), ('cart_tree', ML(1), 1), ('marbles', ML(1), 1), ('readme', {NN: '1'}, -16),
        ('readme', {NN: '1', NSG: '1'}, 0), ('ur_ik', {'DG_NO_HELPER_WAVE': '1'}, 64), ('ur_ik', {'DG_NO_EARLY_DYNAMICS': '1'}, 64),
        ('ur_ik', {'DG_NO_COLLIDE_WAVE': '1'}, 64), ('ur_ik', {'DG_NO_SPLIT_SWEEPS': '1'}, 64), ('ur_ik', {'DG_NO_FULL_IK': '1'}, 64),
        ('touching', {'DG_NO_COLLIDE_SPLIT': '1'}, 64), ('touching', {'DG_NO_CHAIN_ROWS': '1'}, 64), ('touching_ik', {'DG_NO_CHAIN_ROWS': '1'}, 64),
        ('touching', {'DG_NO_EARLY_DYNAMICS': '1'}, 64)]] +
    # test_envs_of_a_wavefront_with_different_contact_counts
    [(name, sw, lanes, 12, {}, None) for name, sw, lanes in [
        ('readme', {WE: '1'}, 4), ('maze', ML(8), 8), ('marbles', ML(32), 32), ('maze', ML(8, DG_NO_REG_ROWS=1), 8), ('readme', {NN: '1'}, -16)]] +
    # test_zero_started_motor_rows_in_every_sweep_form
    [(name, sw, lanes, 9, engine, None) for name, sw, lanes, engine in [
        ('ur_ik', {}, 64, COLD), ('ur_ik', {}, 64, REF), ('ur_joint', {}, 64, COLD), ('ur_ik', {'DG_NO_SPLIT_SWEEPS': '1'}, 64, COLD),
        ('ur_ik', {'DG_NO_HELPER_WAVE': '1'}, 64, REF), ('touching', {}, 64, COLD), ('touching', {}, 64, REF),
        ('touching', {'DG_NO_SPLIT_SWEEPS': '1'}, 64, REF), ('touching', {'DG_NO_HELPER_WAVE': '1'}, 64, COLD), ('touching_ik', {}, 64, REF),
        ('readme', {}, 1, REF), ('readme', {WE: '1'}, 4, REF), ('readme', {NN: '1'}, -16, REF), ('readme', {NN: '1', NSG: '1'}, 0, COLD),
        ('maze', ML(8), 8, REF), ('maze', ML(8, DG_NO_REG_ROWS=1), 8, COLD), ('maze', ML(16), 16, COLD), ('maze', ML(1), 1, REF),
        ('cart_tree', {}, 64, REF)]] +
    # test_warm_start_factor_of_bullet_in_every_sweep_form
    [(name, sw, lanes, 9, WARM, None) for name, sw, lanes in [
        ('readme', {}, 1), ('readme', {WE: '1'}, 4), ('readme', {NN: '1'}, -16), ('readme', {NN: '1', NSG: '1'}, 0), ('marbles', ML(16), 16),
        ('marbles', ML(8, DG_NO_REG_ROWS=1), 8), ('touching', {}, 64), ('touching', {'DG_NO_SPLIT_SWEEPS': '1'}, 64),
        ('touching', {'DG_NO_HELPER_WAVE': '1'}, 64), ('cart_tree', {}, 64)]]
)


@pytest.mark.parametrize('name,switches,lanes,num_envs,engine,max_contacts', GPU_ASSERTED)
def test_modes_the_gpu_tests_assert(monkeypatch, name, switches, lanes, num_envs, engine, max_contacts):
    assert plan_of(monkeypatch, name, num_envs, switches, engine, max_contacts)['lanes'] == lanes


# DESIGN §3's mode table, the batch-dependent rows; lds: BENCH_r04.json's lds_bytes_per_workgroup of that leg where it has one
@pytest.mark.parametrize('name,num_envs,switches,lanes,lds', [
    ('ur_ik', 16384, {}, 64, 160512), ('readme', 1024, {}, 1, 23908), ('readme', 1025, {}, 4, None), ('readme', 16384, {}, 4, None),
    ('maze', 4096, {}, 8, 52832), ('drone', 16384, {}, 16, 20032), ('child', 16384, {}, 16, None),
    ('readme', 1024, {NN: '1'}, -16, None), ('readme', 1024, {NN: '1', NSG: '1'}, 0, None)])
def test_modes_of_the_design_table(monkeypatch, name, num_envs, switches, lanes, lds):
    p = plan_of(monkeypatch, name, num_envs, switches)
    assert p['lanes'] == lanes
    if name == 'ur_ik':
        assert p['par'] == 1   # the four-wavefront kernel
    if lds is not None:
        assert p['lds_bytes'] == lds
    assert (p['gws_floats'] > 0) == (lanes <= 0)


def test_bench_record_is_what_the_table_above_quotes():
    """The LDS sizes above are BENCH_r04.json's, not the planner's."""
    text = json.dumps(json.load(open(os.path.join(ROOT, 'BENCH_r04.json'))))
    for lanes, lds in ((64, 160512), (8, 52832), (16, 20032), (1, 23908)):
        assert re.search(r'envs_per_wavefront\W+%d\W+lds_bytes_per_workgroup\W+%d\b' % (lanes, lds), text), (lanes, lds)


def test_switch_effects(monkeypatch):
    assert plan_of(monkeypatch, 'ur_ik', 16384, {'DG_NO_HELPER_WAVE': '1'})['par'] == 0
    assert plan_of(monkeypatch, 'ur_ik', 16384, {'DG_NO_SPLIT_CONTACTS': '1'})['split_pgs'] == 1
    for name in ('ur_ik', 'touching', 'touching_ik'):
        assert plan_of(monkeypatch, name, 16384, {'DG_NO_COLLIDE_SPLIT': '1'})['coll_split'] == 0
    # the environment is read afresh by every call
    assert plan_of(monkeypatch, 'ur_ik', 16384)['par'] == 1


@pytest.mark.parametrize('name', ['touching_ik', 'stack'])
def test_the_manifold_has_no_helper_wave_form(monkeypatch, name):
    p = plan_of(monkeypatch, name, 64, manifold=2)
    assert p['mf'] == 1 and p['par'] == 0 and p['hull_ws_floats'] > 0
    assert plan_of(monkeypatch, name, 64)['mf'] == 0


def test_a_bad_blob_is_refused_with_the_message_of_dg_world_create(monkeypatch):
    from diy_gym_amd import backend
    from diy_gym_amd.scene import K
    layout = copy.copy(_layout('marbles', (), None, None))
    layout.I = layout.I.copy(); layout.I[K.H_MAGIC] ^= 1
    with pytest.raises(RuntimeError, match='bad scene magic/version'):
        backend.debug_plan(layout, 4, CU)


def test_readme_lists_the_switches_of_the_table():
    table = switch_table()
    assert len(table) == len(set(table)) == 20
    text = open(os.path.join(ROOT, 'README.md')).read()
    section = text[text.index('### Environment switches'):]
    section = section[:section.index('\n#', 1)] if '\n#' in section[1:] else section
    assert sorted(re.findall(r'^\| `(DG_[A-Z0-9_]+)` \|', section, flags=re.M)) == sorted(table)   # the rows of the section's table
