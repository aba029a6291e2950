"""dg_world_link_accelerations at the C-ABI: declared in the header, exported by the library, bound by backend.py with matching
argument types; the selector struct, the column constants, and the argument errors HipBackend.link_accelerations raises from the
layout alone -- none of which needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import yaml

import oracle_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'diygym_hip.h')
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
NAME = 'dg_world_link_accelerations'


def _header():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_and_the_binding_matches():
    from diy_gym_amd import backend
    m = re.search(r'(\w+)\s+%s\s*\((.*?)\)\s*;' % NAME, _header(), flags=re.S)
    assert m, 'include/diygym_hip.h does not declare %s' % NAME
    args = [' '.join(a.split()).rsplit(' ', 1) for a in m.group(2).split(',')]
    assert m.group(1) == 'int32_t' and [n for _, n in args] == ['w', 'state', 'body', 'selectors', 'n', 'out', 'stream']
    T = {'dg_world*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int32_t': ctypes.c_int32,
         'const dg_accel_selector*': ctypes.POINTER(backend.AccelSelector)}
    res, argtypes = backend.SYMBOLS[NAME]
    assert res is ctypes.c_int32 and argtypes == [T[t] for t, _ in args]
    assert NAME in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_selector_struct_and_columns_are_the_headers():
    """dg_accel_selector: int32 frame, int32 com, float pos[3], float quat[4] -- 36 bytes, no padding; DG_LINK_ACCEL_MAX and the
    DG_LA_* columns against the Python constants."""
    from diy_gym_amd import backend
    text = _header()
    body = re.search(r'typedef struct dg_accel_selector \{(.*?)\} dg_accel_selector;', text, flags=re.S).group(1)
    fields = [' '.join(f.split()) for f in body.split(';') if f.strip()]
    assert fields == ['int32_t frame', 'int32_t com', 'float pos[3]', 'float quat[4]']
    A = backend.AccelSelector
    assert [f[0] for f in A._fields_] == ['frame', 'com', 'pos', 'quat']
    assert ctypes.sizeof(A) == 36 and (A.frame.offset, A.com.offset, A.pos.offset, A.quat.offset) == (0, 4, 8, 20)
    assert re.search(r'#define\s+DG_LINK_ACCEL_MAX\s+16', text) and backend.LINK_ACCEL_MAX == 16
    cols = dict((k, int(v)) for k, v in re.findall(r'\b(DG_LA_[A-Z_]+)\s*=\s*(\d+)', text))
    assert cols == dict(DG_LA_LIN_ACC=backend.LA_LIN_ACC, DG_LA_ANG_ACC=backend.LA_ANG_ACC, DG_LA_SPECIFIC_FORCE=backend.LA_SPECIFIC_FORCE,
                        DG_LA_ANG_VEL=backend.LA_ANG_VEL, DG_LA_GRAVITY=backend.LA_GRAVITY, DG_LA_STRIDE=backend.LA_STRIDE)
    assert (backend.LA_LIN_ACC, backend.LA_ANG_ACC, backend.LA_SPECIFIC_FORCE, backend.LA_ANG_VEL, backend.LA_GRAVITY, backend.LA_STRIDE) == (0, 3, 6, 9, 12, 15)
    assert backend.LinkAccelerations._fields == ('lin_acc', 'ang_acc', 'specific_force', 'ang_vel', 'gravity')
    import link_accel_ref as ref
    assert (ref.LIN_ACC, ref.ANG_ACC, ref.SPECIFIC_FORCE, ref.ANG_VEL, ref.GRAVITY, ref.STRIDE) == (0, 3, 6, 9, 12, 15)


@pytest.mark.skipif(not os.path.isfile(LIB), reason='run __graft_entry__.build() first')
def test_library_exports_the_symbol_and_null_world_is_an_argument_error():
    from diy_gym_amd import backend
    lib = backend.load_library()
    assert lib.dg_version() >= 12   # the minor that added the entry
    assert lib.dg_world_link_accelerations(None, None, 0, None, 1, None, None) == -4   # DG_ERR_ARG
    assert NAME.encode() in lib.dg_last_error()


def _env(cfg, edit=None):
    from diy_gym_amd import DIYGym
    from diy_gym_amd.config import Configuration
    tree = yaml.safe_load(open(os.path.join(GOLDEN, cfg)))
    if edit:
        edit(tree)
    conf = Configuration.from_dict(os.path.splitext(os.path.basename(cfg))[0], tree)
    conf.source_dir = os.path.dirname(os.path.join(GOLDEN, cfg))
    return DIYGym(conf, num_envs=1, backend_factory=oracle_backend.OracleBackend)


def test_selectors_from_the_layout():
    from diy_gym_amd.backend import link_accel_selectors
    env = _env('ur_arms_touching_ft.yaml'); arm = env.models['ur5_l']
    body, arr = link_accel_selectors(env.layout, arm.uid)   # None: the base alone, identity mount
    assert body == arm.uid and len(arr) == 1 and (arr[0].frame, arr[0].com, list(arr[0].pos), list(arr[0].quat)) == (-1, 0, [0, 0, 0], [0, 0, 0, 1])
    frames = [arm.get_frame_id('ee_fixed_joint'), -1, arm.get_frame_id('elbow_joint')]
    _, arr = link_accel_selectors(env.layout, arm.uid, frames, [0.1, 0.2, 0.3], [0, 0, 2.0, 0], com=True)   # one vector: every selector
    assert [a.frame for a in arr] == frames and all(a.com == 1 for a in arr)
    assert all(np.allclose(list(a.pos), [0.1, 0.2, 0.3]) and list(a.quat) == [0, 0, 1, 0] for a in arr)   # normalised
    _, arr = link_accel_selectors(env.layout, arm.uid, frames[:2], [[1, 2, 3], [4, 5, 6]], [[0, 0, 0, 1], [1, 0, 0, 0]])
    assert list(arr[1].pos) == [4, 5, 6] and list(arr[1].quat) == [1, 0, 0, 0] and list(arr[0].pos) == [1, 2, 3]


def test_arguments_are_checked_in_python_before_any_launch():
    """With layouts alone and no world at all (handle None: a launch would crash): a body without saved velocities (the message
    names the remedy), a frozen body, an attached child model, a frame the body does not have, no frames or more than 16, a zero
    quaternion, mounts of the wrong shape."""
    from diy_gym_amd.backend import HipBackend
    env = _env('ur_arms_touching_ft.yaml')
    sim = HipBackend.__new__(HipBackend); sim.layout = env.layout; sim.handle = None; sim._link_accel_out = {}; sim._link_accel_sel = {}
    arm = env.models['ur5_l'].uid; nfr = len(env.models['ur5_l'].flat.frames)
    for call in (lambda: sim.link_accelerations(arm, [nfr]), lambda: sim.link_accelerations(arm, [-2]), lambda: sim.link_accelerations(arm, []),
                 lambda: sim.link_accelerations(arm, [0] * 17), lambda: sim.link_accelerations(99), lambda: sim.link_accelerations(arm, [0], local_orn=[0, 0, 0, 0]),
                 lambda: sim.link_accelerations(arm, [0, 1], local_pos=[[0, 0, 0]] * 3), lambda: sim.link_accelerations(arm, [0], local_orn=[0, 0, 1])):
        with pytest.raises(ValueError):
            call()
    bare = _env('contacts_arms.yaml')
    sim.layout = bare.layout
    with pytest.raises(ValueError, match='enable_joint_force_torque'):
        sim.link_accelerations(bare.models['ur5_l'].uid)
    child = _env('contacts_child_gripper.yaml')
    sim.layout = child.layout
    with pytest.raises(ValueError, match='frozen'):
        sim.link_accelerations(child.models['plane'].uid)
    with pytest.raises(ValueError, match='attached'):
        sim.link_accelerations(child.models['arm'].models['gripper'].uid)
