"""The C ABI of the task-space dynamics query (include/diygym_hip.h): declared, exported, refusing a NULL world without touching a
device; and every fixed-base jointed body of the repository's scenes fits the workspace its world has.  Runs without a GPU."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
NAME = 'dg_world_task_space'
DG_ERR_ARG = -4
vp, i32 = ctypes.c_void_p, ctypes.c_int32
ARGTYPES = [vp, vp, i32, i32, ctypes.POINTER(ctypes.c_float), i32, vp, vp, vp, vp, ctypes.c_float, vp, vp, vp, vp, vp, vp, vp, vp]


def test_header_declares_the_entry_and_the_binding_types_it():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'diygym_hip.h')).read(), flags=re.S)
    decl = re.search(r'\bint32_t\s+%s\s*\(([^)]*)\)\s*;' % NAME, text)
    assert decl, NAME
    params = [' '.join(p.split()) for p in decl.group(1).split(',')]
    assert params == ['dg_world* w', 'const float* state', 'int32_t body', 'int32_t frame', 'const float* local_pos', 'int32_t axes_mask', 'const float* q',
                      'const float* qd', 'const float* acc', 'const float* tau_null', 'float damping', 'float* jac', 'float* bias_acc', 'float* bias_torque',
                      'float* lambda', 'float* tau', 'float* point', 'int32_t* singular', 'void* stream']
    from diy_gym_amd import backend
    res, argtypes = backend.SYMBOLS[NAME]
    assert res is i32 and argtypes == ARGTYPES
    assert backend.TaskSpaceDynamics._fields == ('jac', 'bias_acc', 'bias_torque', 'lambda_', 'tau', 'point', 'singular')   # the outputs, in the entry's order


def test_library_exports_it_and_it_refuses_a_null_world():
    lib = ctypes.CDLL(LIB)
    lib.dg_last_error.restype = ctypes.c_char_p
    fn = getattr(lib, NAME)   # AttributeError: not exported
    fn.restype, fn.argtypes = i32, ARGTYPES
    lp = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    assert fn(None, None, 0, 0, lp, 63, None, None, None, None, 0.0, None, None, None, None, None, None, None, None) == DG_ERR_ARG
    assert lib.dg_last_error() == b'dg_world_task_space: null argument'


def taskq_slots():
    """``taskq_slots(n, m)`` as diy_gym_amd/csrc/dg_taskq.h defines it, evaluated here: the slots kept throughout plus the larger of
    the Newton-Euler and the task-inertia phase."""
    text = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_taskq.h')).read()
    dynq = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_dynq.h')).read()
    consts = {name: int(re.search(r'\b%s = (\d+)\b' % name, dynq).group(1)) for name in ('DQ_ID_STRIDE', 'DQ_CR_STRIDE')}
    parts = {}
    for name in ('taskq_keep', 'taskq_newton', 'taskq_inertia'):
        body = re.search(r'constexpr int %s\(int n, int m\) \{ return ([^;?]*); \}' % name, text).group(1)
        assert re.fullmatch(r'[\w\s+*/()]+', body), body
        parts[name] = body.replace('/', '//')
    assert ('constexpr int taskq_slots(int n, int m) { return taskq_keep(n, m) + (taskq_newton(n, m) > taskq_inertia(n, m) ? taskq_newton(n, m) : '
            'taskq_inertia(n, m)); }') in text
    part = lambda name, n, m: eval(parts[name], {'__builtins__': {}}, dict(consts, n=n, m=m))
    return lambda n, m: part('taskq_keep', n, m) + max(part('taskq_newton', n, m), part('taskq_inertia', n, m))


def test_the_layout_fits_what_the_planner_guarantees():
    """12 + 32 n for every 1 <= m <= min(6, n), n <= 12; and the figures of DESIGN's slot table."""
    slots = taskq_slots()
    for n in range(1, 13):
        for m in range(1, min(6, n) + 1):
            assert slots(n, m) <= 12 + 32 * n, (n, m, slots(n, m))
    assert [slots(n, min(6, n)) for n in (1, 2, 3, 6, 10, 12)] == [20, 42, 69, 174, 288, 351]


@pytest.mark.parametrize('max_lanes', [None, '4', '1'])
def test_every_fixed_base_body_of_the_repository_fits_its_worlds_transient_region(max_lanes, monkeypatch):
    """The pass borrows the transient region and never enlarges it.  Every scene under tests/golden and examples, planned at 1, 70
    and 16 384 envs in the default workspace mode and in the narrow modes the GPU tests pin, at the widest task the body takes (the
    C entry refuses a body that does not fit: no scene may come to that)."""
    from diy_gym_amd import DIYGym
    from diy_gym_amd.backend import debug_plan
    from raycast_ref import RaycastOracleBackend   # (the oracle plus the ray caster the lidar scene's addon asks its backend for)
    import diy_gym_amd.examples  # noqa: F401
    slots = taskq_slots()
    if max_lanes:
        monkeypatch.setenv('DG_MAX_LANES', max_lanes)
    seen = 0
    for cfg in sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', '*.yaml')) + glob.glob(os.path.join(ROOT, 'examples', '*', '*.yaml'))):
        L = DIYGym(cfg, num_envs=2, backend_factory=RaycastOracleBackend).layout
        for B in (1, 70, 16384):
            plan = debug_plan(L, B)
            for b in range(L.n_bodies):
                n = L.body_n_links[b]
                if L.body_fixed[b] and n >= 1:
                    seen += 1
                    assert slots(n, min(6, n)) <= plan['tr_slots'], (cfg, B, plan['lanes'], b, n, slots(n, min(6, n)), plan['tr_slots'])
    assert seen >= 3 * 20
