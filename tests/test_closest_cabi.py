"""dg_world_closest at the C-ABI: declared in the header, exported by the library, bound by backend.py with matching argument
types, and the Python-side argument errors of HipBackend.closest_points -- none of which needs a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'diygym_hip.h')
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')

C_TYPES = {'dg_world*': ctypes.c_void_p, 'const dg_world*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'int32_t*': ctypes.c_void_p,
           'void*': ctypes.c_void_p, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float}


def _declaration(name):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'(\w+)\s+%s\s*\((.*?)\)\s*;' % name, text, flags=re.S)
    assert m, 'include/diygym_hip.h does not declare %s' % name
    args = [' '.join(a.split()) for a in m.group(2).split(',')]
    return m.group(1), [a.rsplit(' ', 1) for a in args]


def test_header_declares_the_entries():
    ret, args = _declaration('dg_world_closest')
    assert ret == 'int32_t'
    assert [n for _, n in args] == ['w', 'state', 'body_a', 'link_a', 'body_b', 'link_b', 'distance', 'max_points', 'scratch', 'count', 'ids', 'geom',
                                    'nearest_ids', 'nearest_geom', 'stream']
    ret, args = _declaration('dg_world_closest_scratch_floats')
    assert ret == 'int64_t' and [n for _, n in args] == ['w']
    assert 'dg_world_closest' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_binding_has_the_declared_argument_types():
    from diy_gym_amd import backend
    for name in ('dg_world_closest', 'dg_world_closest_scratch_floats'):
        ret, args = _declaration(name)
        res, argtypes = backend.SYMBOLS[name]
        assert res is C_TYPES[ret]
        assert argtypes == [C_TYPES[t] for t, _ in args]
    assert backend.ClosestPoints._fields == ('count', 'id_a', 'id_b', 'pos_a', 'pos_b', 'normal', 'distance', 'nearest_id_a', 'nearest_id_b',
                                             'nearest_pos_a', 'nearest_pos_b', 'nearest_normal', 'nearest_distance')


@pytest.mark.skipif(not os.path.isfile(LIB), reason='run __graft_entry__.build() first')
def test_library_exports_the_symbols_and_the_version_moved():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, 'dg_world_closest') and hasattr(lib, 'dg_world_closest_scratch_floats')
    lib.dg_version.restype = ctypes.c_int32
    assert lib.dg_version() >= 9   # the minor that added dg_world_closest


@pytest.mark.skipif(not os.path.isfile(LIB), reason='run __graft_entry__.build() first')
def test_null_world_is_an_argument_error_without_a_device():
    from diy_gym_amd import backend
    lib = backend.load_library()
    assert lib.dg_world_closest(None, None, 0, -2, -2, -2, 0.1, 0, None, None, None, None, None, None, None) == -4   # DG_ERR_ARG
    assert b'dg_world_closest' in lib.dg_last_error()
    assert lib.dg_world_closest_scratch_floats(None) == 0


class _Layout:
    aliases = {10000: (1, 6, 7, 7)}
    n_bodies = 3
    max_contacts = 4


def test_arguments_are_checked_in_python():
    """What closest_points refuses before it reaches the library, against a layout that has no blob: no body_a, a link without its
    body, a uid the scene does not have, a distance that is negative or not finite, a negative K, rows with nowhere to go, an unknown
    output group."""
    from diy_gym_amd.backend import HipBackend
    sim = HipBackend.__new__(HipBackend); sim.layout = _Layout(); sim.handle = None
    sim.num_envs = 2; sim._closest_out = {}; sim._closest_k = {}; sim._closest_scratch = None
    for kw in (dict(body_a=None), dict(body_a=None, body_b=1), dict(body_a=1, link_b=0), dict(body_a=3), dict(body_a=-1), dict(body_a=10001),
               dict(body_a=1, link_a=-2), dict(body_a=1, distance=-1e-3), dict(body_a=1, distance=float('inf')), dict(body_a=1, distance=float('nan')),
               dict(body_a=1, max_points=-1), dict(body_a=1, max_points=2, want=('nearest', )), dict(body_a=1, want=('id', 'force'))):
        with pytest.raises(ValueError):
            sim.closest_points(**kw)
