"""The C ABI of the forward-dynamics and rollout queries (include/diygym_hip.h): declared, typed by the binding, exported, refusing a
NULL world without touching a device; and every fixed-base jointed body of the repository's scenes fits the workspace its world
has.  Runs without a GPU."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
DG_ERR_ARG = -4
vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
ENTRIES = {
    'dg_world_forward_dynamics': (['dg_world* w', 'const float* state', 'int32_t body', 'const float* q', 'const float* qd', 'const float* tau', 'int32_t joint_damping',
                                   'float* qdd', 'int32_t* singular', 'void* stream'],
                                  [vp, vp, i32, vp, vp, vp, i32, vp, vp, vp]),
    'dg_world_rollout': (['dg_world* w', 'const float* state', 'int32_t body', 'int32_t frame', 'const float* local_pos', 'int32_t K', 'int32_t T', 'float dt',
                          'int32_t joint_damping', 'const float* q0', 'const float* qd0', 'const float* tau', 'float* q_out', 'float* qd_out', 'float* pos_out',
                          'int32_t* singular', 'void* stream'],
                         [vp, vp, i32, i32, ctypes.POINTER(f32), i32, i32, f32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
}


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_header_declares_the_entry_and_the_binding_types_it(name):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'diygym_hip.h')).read(), flags=re.S)
    decl = re.search(r'\bint32_t\s+%s\s*\(([^)]*)\)\s*;' % name, text)
    assert decl, name
    assert [' '.join(p.split()) for p in decl.group(1).split(',')] == ENTRIES[name][0]
    from diy_gym_amd import backend
    res, argtypes = backend.SYMBOLS[name]
    assert res is i32 and argtypes == ENTRIES[name][1]
    assert backend.JointRollout._fields == ('q', 'qd', 'pos', 'singular')   # the rollout's outputs, in the entry's order


def test_library_exports_them_and_they_refuse_a_null_world():
    lib = ctypes.CDLL(LIB)
    lib.dg_last_error.restype = ctypes.c_char_p
    for name, (_, argtypes) in ENTRIES.items():
        fn = getattr(lib, name)   # AttributeError: not exported
        fn.restype, fn.argtypes = i32, argtypes
    assert lib.dg_world_forward_dynamics(None, None, 0, None, None, None, 0, None, None, None) == DG_ERR_ARG
    assert lib.dg_last_error() == b'dg_world_forward_dynamics: null argument'
    lp = (f32 * 3)(0.0, 0.0, 0.0)
    assert lib.dg_world_rollout(None, None, 0, 0, lp, 1, 1, 0.01, 0, None, None, None, None, None, None, None, None) == DG_ERR_ARG
    assert lib.dg_last_error() == b'dg_world_rollout: null argument'


def fdq_slots():
    """``fdq_slots(n)`` as diy_gym_amd/csrc/dg_fdq.h defines it, evaluated here: the slots kept throughout plus the larger of the
    Newton-Euler and the joint-inertia phase."""
    text = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_fdq.h')).read()
    dynq = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_dynq.h')).read()
    consts = {name: int(re.search(r'\b%s = (\d+)\b' % name, dynq).group(1)) for name in ('DQ_ID_STRIDE', 'DQ_CR_STRIDE')}
    parts = {}
    for name in ('fdq_keep', 'fdq_newton', 'fdq_inertia'):
        body = re.search(r'constexpr int %s\(int n\) \{ return ([^;?]*); \}' % name, text).group(1)
        assert re.fullmatch(r'[\w\s+*/()]+', body), body
        parts[name] = body.replace('/', '//')
    assert 'constexpr int fdq_slots(int n) { return fdq_keep(n) + (fdq_newton(n) > fdq_inertia(n) ? fdq_newton(n) : fdq_inertia(n)); }' in text
    part = lambda name, n: eval(parts[name], {'__builtins__': {}}, dict(consts, n=n))
    return lambda n: part('fdq_keep', n) + max(part('fdq_newton', n), part('fdq_inertia', n))


def test_the_layout_fits_what_the_planner_guarantees():
    """12 + 32 n for every n <= 12; and the figures of DESIGN's slot table."""
    slots = fdq_slots()
    for n in range(1, 13):
        assert slots(n) <= 12 + 32 * n, (n, slots(n))
    assert [slots(n) for n in (1, 2, 3, 6, 10, 12)] == [18, 36, 54, 108, 185, 234]


@pytest.mark.parametrize('max_lanes', [None, '4', '1'])
def test_every_fixed_base_body_of_the_repository_fits_its_worlds_transient_region(max_lanes, monkeypatch):
    """The passes borrow the transient region and never enlarge it.  Every scene under tests/golden and examples (the sibling queries' list), planned at 1, 70 and 16 384 envs in the default workspace mode and in the narrow modes
    the GPU tests pin (the C entries refuse a body that does not fit: no scene may come to that)."""
    from diy_gym_amd import DIYGym
    from diy_gym_amd.backend import debug_plan
    from raycast_ref import RaycastOracleBackend   # (the oracle plus the ray caster the lidar scene's addon asks its backend for)
    import diy_gym_amd.examples  # noqa: F401
    slots = fdq_slots()
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
                    assert slots(n) <= plan['tr_slots'], (cfg, B, plan['lanes'], b, n, slots(n), plan['tr_slots'])
    assert seen >= 3 * 20
