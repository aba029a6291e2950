"""The C ABI of the inertial parameters and the inverse-dynamics regressor (include/diygym_hip.h): declared, typed by the binding,
exported, refusing a NULL world without touching a device; and every scene the GPU tests run the kernel on fits the workspace its
world has -- the layout borrows the transient region and the planner is not touched.  Runs without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DG_ERR_ARG = -4
vp, i32 = ctypes.c_void_p, ctypes.c_int32
ENTRIES = {
    'dg_world_inertial_parameters': (['dg_world* w', 'const float* state', 'int32_t body', 'int32_t nominal', 'float* theta', 'void* stream'],
                                     [vp, vp, i32, i32, vp, vp]),
    'dg_world_id_regressor': (['dg_world* w', 'const float* state', 'int32_t body', 'int32_t P', 'const float* q', 'const float* qd', 'const float* qdd',
                               'const float* qd_ref', 'const float* theta_hat', 'const float* s', 'float* Y', 'float* tau', 'float* grad', 'void* stream'],
                              [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
}
SCENES = ['pendulum.yaml', 'double_pendulum.yaml', 'cart_tree_fixed.yaml', 'ur_admittance.yaml', 'ur_randomized.yaml', 'ur5_gripper.yaml',
          os.path.join('regressor', 'ur_adaptive.yaml')]
EXAMPLES = [os.path.join('ur_high_5', 'ur_high_5.yaml'), os.path.join('ur_high_5', 'adaptive', 'ur_high_5_adaptive.yaml')]


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_header_declares_the_entry_and_the_binding_types_it(name):
    params, argtypes = ENTRIES[name]
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'diygym_hip.h')).read(), flags=re.S)
    decl = re.search(r'\bint32_t\s+%s\s*\(([^)]*)\)\s*;' % name, text)
    assert decl, name
    assert [' '.join(p.split()) for p in decl.group(1).split(',')] == params
    from diy_gym_amd import backend
    res, got = backend.SYMBOLS[name]
    assert res is i32 and got == argtypes
    assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_the_binding_has_the_two_calls_and_the_result_type():
    from diy_gym_amd import backend
    assert backend.DynamicsRegressor._fields == ('Y', 'tau', 'grad')   # the outputs, in the entry's order
    assert callable(backend.HipBackend.inertial_parameters) and callable(backend.HipBackend.inverse_dynamics_regressor)


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_library_exports_it_and_it_refuses_a_null_world(name):
    lib = ctypes.CDLL(LIB)
    lib.dg_last_error.restype = ctypes.c_char_p
    fn = getattr(lib, name)   # AttributeError: not exported
    fn.restype, fn.argtypes = i32, ENTRIES[name][1]
    args = [None if t is vp else 1 for t in ENTRIES[name][1]]
    args[2] = 0
    assert fn(*args) == DG_ERR_ARG
    assert lib.dg_last_error() == b'%s: null argument' % name.encode()


def regq_slots():
    """``regq_slots(n)`` as diy_gym_amd/csrc/dg_regq.h defines it, evaluated here: five joint vectors and RQ_STRIDE slots per link."""
    text = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_regq.h')).read()
    stride = int(re.search(r'\bRQ_STRIDE = (\d+)\b', text).group(1))
    body = re.search(r'constexpr int regq_slots\(int n\) \{ return ([^;?]*); \}', text).group(1)
    assert re.fullmatch(r'[\w\s+*()]+', body), body
    return lambda n: eval(body, {'__builtins__': {}}, {'RQ_STRIDE': stride, 'n': n})


def test_the_layout_fits_what_the_planner_guarantees():
    """[q qd qd_ref qdd s: 5 n] + (12 for the kinematic pass + 6 for force and moment or the virtual twist) n = 23 n, at or below the
    planner's 12 + 32 n for every n <= 12 (and beyond)."""
    slots = regq_slots()
    assert [slots(n) for n in (1, 2, 3, 6, 12)] == [23, 46, 69, 138, 276]
    for n in range(1, 65):
        assert slots(n) <= 12 + 32 * n, (n, slots(n))


@pytest.mark.parametrize('max_lanes', [None, '4', '1'])
def test_every_scene_of_the_gpu_tests_fits_its_worlds_transient_region(max_lanes, monkeypatch):
    """pendulum, double_pendulum, cart_tree_fixed, ur_admittance, ur_randomized, ur5_gripper, the adaptive controller's fixture and
    ur_high_5 with its adaptive example, planned at 1, 70 and 16 384 envs in the default workspace mode and in the narrow modes the GPU
    tests pin (the C entry refuses a body that does not fit: none of these may come to that)."""
    from diy_gym_amd import DIYGym
    from diy_gym_amd.backend import debug_plan
    from oracle_backend import OracleBackend
    import diy_gym_amd.examples  # noqa: F401
    slots = regq_slots()
    if max_lanes:
        monkeypatch.setenv('DG_MAX_LANES', max_lanes)
    seen, joints = 0, set()
    for cfg in [os.path.join(GOLDEN, s) for s in SCENES] + [os.path.join(ROOT, 'examples', s) for s in EXAMPLES]:
        L = DIYGym(cfg, num_envs=2, backend_factory=OracleBackend).layout
        for B in (1, 70, 16384):
            plan = debug_plan(L, B)
            for b in range(L.n_bodies):
                n = L.body_n_links[b]
                if L.body_fixed[b] and n >= 1:
                    seen += 1
                    joints.add(int(n))
                    assert slots(n) <= plan['tr_slots'], (cfg, B, plan['lanes'], b, n, slots(n), plan['tr_slots'])
    assert seen >= 3 * len(SCENES) and {1, 2, 6, 12} <= joints
