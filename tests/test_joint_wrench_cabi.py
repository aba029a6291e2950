"""dg_world_joint_wrench and dg_world_joint_efforts at the C-ABI: declared in the header, exported by the library, bound by backend.py
with matching argument types; the selectors HipBackend.joint_reaction_forces builds on the host and its argument errors -- none of
which needs a GPU."""
import ctypes
import os
import re

import pytest

import oracle_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'diygym_hip.h')
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

ENTRIES = {
    'dg_world_joint_wrench': ['w', 'state', 'body', 'selectors', 'n', 'wrench', 'stream'],
    'dg_world_joint_efforts': ['w', 'state', 'body', 'out', 'stream'],
}


def _c_types():
    from diy_gym_amd import backend
    return {'dg_world*': ctypes.c_void_p, 'const float*': ctypes.c_void_p, 'float*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int32_t': ctypes.c_int32,
            'const dg_joint_selector*': ctypes.POINTER(backend.JointSelector)}


def _declaration(name):
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'(\w+)\s+%s\s*\((.*?)\)\s*;' % name, text, flags=re.S)
    assert m, 'include/diygym_hip.h does not declare %s' % name
    args = [' '.join(a.split()) for a in m.group(2).split(',')]
    return m.group(1), [a.rsplit(' ', 1) for a in args]


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_header_declares_the_entry_and_the_binding_matches(name):
    from diy_gym_amd import backend
    ret, args = _declaration(name)
    assert ret == 'int32_t' and [n for _, n in args] == ENTRIES[name]
    res, argtypes = backend.SYMBOLS[name]
    T = _c_types()
    assert res is ctypes.c_int32 and argtypes == [T[t] for t, _ in args]
    text = open(HEADER).read()
    assert re.search(r'#define\s+DG_JOINT_WRENCH_MAX\s+16', text) and backend.JOINT_WRENCH_MAX == 16
    assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_selector_struct_is_the_headers():
    """dg_joint_selector: int32 frame, int32 flags, uint64 link_mask, uint64 frame_mask, float rigid[10] -- 64 bytes, no padding."""
    from diy_gym_amd.backend import JointSelector
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct dg_joint_selector \{(.*?)\} dg_joint_selector;', text, flags=re.S).group(1)
    fields = [' '.join(f.split()) for f in body.split(';') if f.strip()]
    assert fields == ['int32_t frame', 'int32_t flags', 'uint64_t link_mask', 'uint64_t frame_mask', 'float rigid[10]']
    assert [f[0] for f in JointSelector._fields_] == ['frame', 'flags', 'link_mask', 'frame_mask', 'rigid']
    assert ctypes.sizeof(JointSelector) == 64 and JointSelector.link_mask.offset == 8 and JointSelector.rigid.offset == 24


@pytest.mark.skipif(not os.path.isfile(LIB), reason='run __graft_entry__.build() first')
def test_library_exports_the_symbols_and_null_world_is_an_argument_error():
    from diy_gym_amd import backend
    lib = backend.load_library()
    assert lib.dg_version() >= 11   # the minor that added the two entries
    assert lib.dg_world_joint_wrench(None, None, 0, None, 1, None, None) == -4   # DG_ERR_ARG
    assert b'dg_world_joint_wrench' in lib.dg_last_error()
    assert lib.dg_world_joint_efforts(None, None, 0, None, None) == -4
    assert b'dg_world_joint_efforts' in lib.dg_last_error()


def _env(cfg):
    from diy_gym_amd import DIYGym
    return DIYGym(os.path.join(GOLDEN, cfg), num_envs=1, backend_factory=oracle_backend.OracleBackend)


def test_selectors_are_the_compiled_sensors_child_side():
    """For every joint of a UR5, fixed or movable: the selector's rigid numbers, flags and moving links are ft_cluster's, and the
    shapes its two masks select are exactly the shapes the compiled sensor lists (SceneBuilder.shapes_of)."""
    import numpy as np
    from diy_gym_amd.backend import joint_wrench_selectors
    from diy_gym_amd.scene import K
    env = _env('ur_arms_touching_ft.yaml'); layout = env.layout; I = layout.I
    ns = int(I[K.H_N_SHAPES]); SI = I[int(I[K.H_OFF_SHAPE_I]):][:ns * K.SI_STRIDE].reshape(ns, K.SI_STRIDE)
    for name in ('ur5_l', 'ur5_r'):
        m = env.models[name]; flat = m.flat; first = layout.body_first_link[m.uid]
        for j0 in range(0, len(flat.frames), 16):
            joints = list(range(j0, min(j0 + 16, len(flat.frames))))
            body, js, arr = joint_wrench_selectors(layout, m.uid, joints)
            assert body == m.uid and js == joints and len(arr) == len(joints)
            for k, j in enumerate(joints):
                cl = flat.ft_cluster(j)
                assert arr[k].frame == j and bool(arr[k].flags & K.FT_WHOLE_LINK) == bool(flat.robot.joints[j].movable)
                assert [i for i in range(64) if (arr[k].link_mask >> i) & 1] == cl['moving']
                assert [i for i in range(64) if (arr[k].frame_mask >> i) & 1] == cl['urdf_links']
                assert np.allclose(list(arr[k].rigid)[:4], [cl['rigid'][0], *cl['rigid'][1]], rtol=1e-6, atol=1e-9)
                ul, ll = ((SI[:, K.SI_FLAGS] >> 8) & 0xFFFF) - 1, SI[:, K.SI_LINK] - first
                on = (SI[:, K.SI_BODY] == m.uid) & ((((arr[k].frame_mask >> np.clip(ul, 0, 63).astype(np.uint64)) & np.uint64(1)) == 1) & (ul >= 0)
                                                   | (((arr[k].link_mask >> np.clip(ll, 0, 63).astype(np.uint64)) & np.uint64(1)) == 1) & (SI[:, K.SI_LINK] >= 0))
                assert sorted(np.nonzero(on)[0].tolist()) == sorted(env.builder.shapes_of(m.uid, cl['urdf_links'], cl['moving']))
        body, js, arr = joint_wrench_selectors(layout, m.uid, None)   # None: every movable joint
        assert js == list(flat.dof_to_joint) and len(arr) == 6


def test_arguments_are_checked_in_python_before_any_launch():
    """With layouts alone and no world at all (handle None: a launch would crash): a body without saved velocities (the message
    names the remedy), a frozen body, an attached child model, a joint the body does not have, no joints or more than 16."""
    from diy_gym_amd.backend import HipBackend
    env = _env('ur_arms_touching_ft.yaml')
    sim = HipBackend.__new__(HipBackend); sim.layout = env.layout; sim.handle = None; sim._joint_wrench_out = {}
    arm = env.models['ur5_l'].uid; nfr = len(env.models['ur5_l'].flat.frames)
    for call in (lambda: sim.joint_reaction_forces(arm, [nfr]), lambda: sim.joint_reaction_forces(arm, [-1]), lambda: sim.joint_reaction_forces(arm, []),
                 lambda: sim.joint_reaction_forces(arm, [0] * 17), lambda: sim.joint_reaction_forces(99), lambda: sim.joint_motor_torques(99)):
        with pytest.raises(ValueError):
            call()
    bare = _env('contacts_arms.yaml')
    sim.layout = bare.layout
    with pytest.raises(ValueError, match='enable_joint_force_torque'):
        sim.joint_reaction_forces(bare.models['ur5_l'].uid)
    child = _env('contacts_child_gripper.yaml')
    sim.layout = child.layout
    with pytest.raises(ValueError, match='frozen'):
        sim.joint_reaction_forces(child.models['plane'].uid, [0])
    with pytest.raises(ValueError, match='attached'):
        sim.joint_reaction_forces(child.models['arm'].models['gripper'].uid, [0])
    with pytest.raises(ValueError, match='no joints'):
        sim.joint_motor_torques(child.models['plane'].uid)
