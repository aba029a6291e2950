"""dg_world_contacts at the C-ABI: declared in the header, exported by the library, bound by backend.py with matching argument
types, and the Python-side argument errors of HipBackend.contact_points -- none of which needs a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'diygym_hip.h')
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')

C_TYPES = {'dg_world*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'int32_t*': ctypes.c_void_p, 'void*': ctypes.c_void_p,
           'int32_t': ctypes.c_int32}


def _declaration():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'(\w+)\s+dg_world_contacts\s*\((.*?)\)\s*;', text, flags=re.S)
    assert m, 'include/diygym_hip.h does not declare dg_world_contacts'
    args = [' '.join(a.split()) for a in m.group(2).split(',')]
    return m.group(1), [a.rsplit(' ', 1) for a in args]


def test_header_declares_the_entry_and_the_wildcard():
    ret, args = _declaration()
    assert ret == 'int32_t'
    assert [n for _, n in args] == ['w', 'state', 'body_a', 'link_a', 'body_b', 'link_b', 'count', 'ids', 'geom', 'force', 'stream']
    assert re.search(r'#define\s+DG_CONTACT_ANY\s+\(-2\)', open(HEADER).read())
    assert 'dg_world_contacts' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_binding_has_the_declared_argument_types():
    from diy_gym_amd import backend
    ret, args = _declaration()
    res, argtypes = backend.SYMBOLS['dg_world_contacts']
    assert res is C_TYPES[ret]
    assert argtypes == [C_TYPES[t] for t, _ in args]
    assert backend.CONTACT_ANY == -2
    assert backend.ContactPoints._fields == ('count', 'id_a', 'id_b', 'pos_a', 'pos_b', 'normal', 'distance', 'normal_force')


@pytest.mark.skipif(not os.path.isfile(LIB), reason='run __graft_entry__.build() first')
def test_library_exports_the_symbol_and_the_version_moved():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, 'dg_world_contacts')
    lib.dg_version.restype = ctypes.c_int32
    assert lib.dg_version() >= 8   # the minor that added dg_world_contacts


@pytest.mark.skipif(not os.path.isfile(LIB), reason='run __graft_entry__.build() first')
def test_null_world_is_an_argument_error_without_a_device():
    from diy_gym_amd import backend
    lib = backend.load_library()
    assert lib.dg_world_contacts(None, None, -2, -2, -2, -2, None, None, None, None, None) == -4   # DG_ERR_ARG
    assert b'dg_world_contacts' in lib.dg_last_error()


class _Layout:
    aliases = {10000: (1, 6, 7, 7)}
    n_bodies = 3
    max_contacts = 4


def test_filter_arguments_are_checked_in_python():
    """The filters of contact_points, resolved without a world: None is DG_CONTACT_ANY, an alias uid becomes its parent's body, a link
    without its body and a uid the scene does not have raise ValueError."""
    from diy_gym_amd.backend import HipBackend, CONTACT_ANY
    sim = HipBackend.__new__(HipBackend); sim.layout = _Layout(); sim.handle = None
    assert sim._contact_filter('a', None, None) == (CONTACT_ANY, CONTACT_ANY)
    assert sim._contact_filter('a', 2, None) == (2, CONTACT_ANY)
    assert sim._contact_filter('b', 2, -1) == (2, -1)
    assert sim._contact_filter('a', 10000, 3) == (1, 3)
    for body, link in ((None, 0), (3, None), (-1, None), (10001, None), (1, -2)):
        with pytest.raises(ValueError):
            sim._contact_filter('a', body, link)
    with pytest.raises(ValueError):
        sim.contact_points(want=('id', 'speed'))
