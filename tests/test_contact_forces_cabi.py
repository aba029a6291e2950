"""dg_world_contact_forces and dg_world_net_contact_wrench at the C-ABI: declared in the header, exported by the library, bound by
backend.py with matching argument types, and the Python-side argument errors of HipBackend.contact_forces / net_contact_forces --
none of which needs a GPU."""
import ctypes
import os
import re

import pytest

import oracle_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'diygym_hip.h')
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')

C_TYPES = {'dg_world*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'int32_t*': ctypes.c_void_p, 'void*': ctypes.c_void_p,
           'int32_t': ctypes.c_int32, 'const int32_t*': ctypes.POINTER(ctypes.c_int32)}
ENTRIES = {
    'dg_world_contact_forces': ['w', 'state', 'body_a', 'link_a', 'body_b', 'link_b', 'count', 'ids', 'forces', 'stream'],
    'dg_world_net_contact_wrench': ['w', 'state', 'body', 'links', 'n', 'body_b', 'link_b', 'wrench', 'ncontacts', 'stream'],
}


def _declaration(name):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'(\w+)\s+%s\s*\((.*?)\)\s*;' % name, text, flags=re.S)
    assert m, 'include/diygym_hip.h does not declare %s' % name
    args = [' '.join(a.split()) for a in m.group(2).split(',')]
    return m.group(1), [a.rsplit(' ', 1) for a in args]


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_header_declares_the_entry(name):
    ret, args = _declaration(name)
    assert ret == 'int32_t' and [n for _, n in args] == ENTRIES[name]
    text = open(HEADER).read()
    assert re.search(r'#define\s+DG_CONTACT_MAX_LINKS\s+16', text) and re.search(r'DG_CFO_FORCE_A = 12,\s*DG_CFO_STRIDE = 15', text)
    assert 'Lateral friction is\n * not reported' not in text and 'dg_world_contact_forces' in text.split('int32_t dg_world_contacts(')[0]
    assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_binding_has_the_declared_argument_types(name):
    from diy_gym_amd import backend
    ret, args = _declaration(name)
    res, argtypes = backend.SYMBOLS[name]
    assert res is C_TYPES[ret] and argtypes == [C_TYPES[t] for t, _ in args]
    assert backend.CONTACT_MAX_LINKS == 16
    assert backend.ContactForces._fields == ('count', 'id_a', 'id_b', 'normal', 'normal_force', 'lateral_friction1', 'lateral_dir1', 'lateral_friction2',
                                             'lateral_dir2', 'force_on_a')
    assert backend.ContactPoints._fields == ('count', 'id_a', 'id_b', 'pos_a', 'pos_b', 'normal', 'distance', 'normal_force')   # unchanged


@pytest.mark.skipif(not os.path.isfile(LIB), reason='run __graft_entry__.build() first')
def test_library_exports_the_symbols_and_the_version_moved():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, 'dg_world_contact_forces') and hasattr(lib, 'dg_world_net_contact_wrench')
    lib.dg_version.restype = ctypes.c_int32
    assert lib.dg_version() >= 10   # the minor that added the two entries


@pytest.mark.skipif(not os.path.isfile(LIB), reason='run __graft_entry__.build() first')
def test_null_world_is_an_argument_error_without_a_device():
    from diy_gym_amd import backend
    lib = backend.load_library()
    assert lib.dg_world_contact_forces(None, None, -2, -2, -2, -2, None, None, None, None) == -4   # DG_ERR_ARG
    assert b'dg_world_contact_forces' in lib.dg_last_error()
    assert lib.dg_world_net_contact_wrench(None, None, 0, None, 1, -2, -2, None, None, None) == -4
    assert b'dg_world_net_contact_wrench' in lib.dg_last_error()


def test_arguments_are_checked_in_python_before_any_launch():
    """With the layout of the merged-gripper scene and no world at all (handle None: a launch would crash): the selectors of
    net_contact_forces are resolved or refused in Python -- more than 16 or no links, a body the scene does not have, a link that is
    not a frame of the body, a link filter without its body, an unknown `want`."""
    from diy_gym_amd import DIYGym
    from diy_gym_amd.backend import HipBackend, CONTACT_ANY
    env = DIYGym(os.path.join(ROOT, 'tests', 'golden', 'contacts_child_gripper.yaml'), num_envs=1, backend_factory=oracle_backend.OracleBackend)
    arm = env.models['arm']; alias = arm.models['gripper'].uid
    sim = HipBackend.__new__(HipBackend); sim.layout = env.layout; sim.handle = None
    nfr = sim._body_n_frames(arm.uid)
    assert nfr >= 18 and sim._body_n_frames(env.models['plane'].uid) == 0   # (the arm's frames and the merged gripper's)
    assert sim._net_contact_links(arm.uid, None) == (arm.uid, [CONTACT_ANY])
    assert sim._net_contact_links(alias, [None, -1, 3, nfr - 1]) == (arm.uid, [CONTACT_ANY, -1, 3, nfr - 1])
    for body, links in ((arm.uid, []), (arm.uid, [0] * 17), (arm.uid, [nfr]), (arm.uid, [-2]), (env.models['plane'].uid, [0]), (17, None), (None, None)):
        with pytest.raises(ValueError):
            sim._net_contact_links(body, links)
    for call in (lambda: sim.net_contact_forces(arm.uid, [nfr]), lambda: sim.net_contact_forces(arm.uid, [0] * 17),
                 lambda: sim.net_contact_forces(arm.uid, None, None, 0), lambda: sim.net_contact_forces(arm.uid, want=('force', 'moment')),
                 lambda: sim.net_contact_forces(99), lambda: sim.contact_forces(None, None, 0), lambda: sim.contact_forces(want=('id', 'torque')),
                 lambda: sim.contact_forces(99)):
        with pytest.raises(ValueError):
            call()
