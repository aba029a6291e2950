"""The C ABI of the dynamics queries (include/diygym_hip.h): declared, exported, refusing a NULL world without touching a device;
and every fixed-base jointed body of the repository's scenes fits the workspace its world has.  Runs without a GPU."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
ENTRIES = ['dg_world_joint_state', 'dg_world_jacobian', 'dg_world_inverse_dynamics', 'dg_world_mass_matrix', 'dg_world_apply_joint_torque']
DG_ERR_ARG = -4
vp, i32 = ctypes.c_void_p, ctypes.c_int32


def test_header_declares_the_five_entries():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'diygym_hip.h')).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r'\bint32_t\s+%s\s*\(\s*dg_world\s*\*\s*w\s*,' % name, text), name
    from diy_gym_amd import backend
    assert set(ENTRIES) <= set(backend.SYMBOLS)


def test_library_exports_them_and_each_refuses_a_null_world():
    lib = ctypes.CDLL(LIB)
    lib.dg_last_error.restype = ctypes.c_char_p
    lp = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    args = {'dg_world_joint_state': ([vp, vp, i32, vp, vp, vp], (None, None, 0, None, None, None)),
            'dg_world_jacobian': ([vp, vp, i32, i32, ctypes.POINTER(ctypes.c_float), vp, vp, vp, vp], (None, None, 0, 0, lp, None, None, None, None)),
            'dg_world_inverse_dynamics': ([vp, vp, i32, vp, vp, vp, vp, vp], (None, None, 0, None, None, None, None, None)),
            'dg_world_mass_matrix': ([vp, vp, i32, vp, vp, vp], (None, None, 0, None, None, None)),
            'dg_world_apply_joint_torque': ([vp, vp, i32, vp, vp], (None, None, 0, None, None))}
    for name in ENTRIES:
        fn = getattr(lib, name)   # AttributeError: not exported
        fn.restype, fn.argtypes = i32, args[name][0]
        assert fn(*args[name][1]) == DG_ERR_ARG, name
        assert name.encode() in lib.dg_last_error()


def slots_per_joint():
    """{pass: workspace slots per joint} as diy_gym_amd/csrc/dg_dynq.h defines them (``dynq_slots``): the joint vectors a pass stages
    plus its per-link block."""
    text = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_dynq.h')).read()
    val = lambda name: int(re.search(r'\b%s = (\d+)\b' % name, text).group(1))
    assert re.search(r'DQ_ID_SLOTS = 3 \+ DQ_ID_STRIDE\b', text) and re.search(r'DQ_CR_SLOTS = 1 \+ DQ_CR_STRIDE\b', text)
    assert 'kind == DQ_KIND_ID ? DQ_ID_SLOTS : kind == DQ_KIND_MASS ? DQ_CR_SLOTS : 1' in text
    return {'inverse_dynamics': 3 + val('DQ_ID_STRIDE'), 'mass_matrix': 1 + val('DQ_CR_STRIDE'), 'jacobian': 1}


@pytest.mark.parametrize('max_lanes', [None, '4', '1'])
def test_every_fixed_base_body_of_the_repository_fits_its_worlds_transient_region(max_lanes, monkeypatch):
    """The passes borrow the transient region and never enlarge it; the planner gives every body at least 12 + 32 slots per joint.
    Every scene under tests/golden and examples, planned at 1, 70 and 16 384 envs in the default workspace mode and in the narrow
    modes the GPU tests pin (the C entries refuse a body that does not fit: no scene may come to that)."""
    from diy_gym_amd import DIYGym
    from diy_gym_amd.backend import debug_plan
    from raycast_ref import RaycastOracleBackend   # (the oracle plus the ray caster the lidar scene's addon asks its backend for)
    import diy_gym_amd.examples  # noqa: F401
    need = max(slots_per_joint().values())
    assert need == slots_per_joint()['inverse_dynamics']
    if max_lanes:
        monkeypatch.setenv('DG_MAX_LANES', max_lanes)
    seen = 0
    for cfg in sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', '*.yaml')) + glob.glob(os.path.join(ROOT, 'examples', '*', '*.yaml'))):
        L = DIYGym(cfg, num_envs=2, backend_factory=RaycastOracleBackend).layout
        for B in (1, 70, 16384):
            plan = debug_plan(L, B)
            for b in range(L.n_bodies):
                if L.body_fixed[b] and L.body_n_links[b] >= 1:
                    seen += 1
                    assert need * L.body_n_links[b] <= plan['tr_slots'], (cfg, B, plan['lanes'], b, L.body_n_links[b], plan['tr_slots'])
    assert seen >= 3 * 20
