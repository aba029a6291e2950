"""The C ABI of the link-state query and the base reset (include/diygym_hip.h): declared, typed in the Python binding, documented,
exported, and refusing a NULL world without touching a device.  Runs without a GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
ENTRIES = ['dg_world_link_states', 'dg_world_reset_base_state']
DG_ERR_ARG = -4
vp, i32 = ctypes.c_void_p, ctypes.c_int32


def header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'diygym_hip.h')).read(), flags=re.S)


def test_header_binding_and_integration_notes_name_both_entries():
    text = header()
    for name in ENTRIES:
        assert re.search(r'\bint32_t\s+%s\s*\(\s*dg_world\s*\*\s*w\s*,' % name, text), name
    from diy_gym_amd import backend
    assert set(ENTRIES) <= set(backend.SYMBOLS)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in ENTRIES)


def test_the_selector_cap_is_32():
    m = re.search(r'#define\s+DG_LINK_STATES_MAX\s+(\d+)', header())
    assert m and int(m.group(1)) == 32
    from diy_gym_amd import backend
    assert backend.LINK_STATES_MAX == 32


def test_library_exports_them_and_each_refuses_a_null_world():
    lib = ctypes.CDLL(LIB)
    lib.dg_last_error.restype = ctypes.c_char_p
    args = {'dg_world_link_states': ([vp, vp, vp, vp, i32, i32, vp, vp], (None, None, None, None, 1, 0, None, None)),
            'dg_world_reset_base_state': ([vp, vp, i32, vp, vp, vp, vp, vp, vp], (None, None, 0, None, None, None, None, None, None))}
    for name in ENTRIES:
        fn = getattr(lib, name)   # AttributeError: not exported
        fn.restype, fn.argtypes = i32, args[name][0]
        assert fn(*args[name][1]) == DG_ERR_ARG, name
        assert name.encode() in lib.dg_last_error()
