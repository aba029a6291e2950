"""The C ABI of the inverse-kinematics query, the motor targets and the joint reset (include/diygym_hip.h): declared, exported,
refusing a NULL world without touching a device; every fixed-base jointed body of the repository's scenes fits the workspace its
world has; and a hook addon learns the mask of the reset in progress.  Runs without a GPU."""
import ctypes
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
ENTRIES = ['dg_world_inverse_kinematics', 'dg_world_set_joint_targets', 'dg_world_reset_joint_state']
DG_ERR_ARG = -4
vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64


def test_header_declares_the_three_entries():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'diygym_hip.h')).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r'\bint32_t\s+%s\s*\(\s*dg_world\s*\*\s*w\s*,' % name, text), name
    from diy_gym_amd import backend
    assert set(ENTRIES) <= set(backend.SYMBOLS)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in doc for name in ENTRIES)


def test_library_exports_them_and_each_refuses_a_null_world():
    lib = ctypes.CDLL(LIB)
    lib.dg_last_error.restype = ctypes.c_char_p
    args = {'dg_world_inverse_kinematics': ([vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp], (None, None, 0, 0, None, None, None, None, None, None, None)),
            'dg_world_set_joint_targets': ([vp, vp, i32, u64, vp, vp, vp], (None, None, 0, 1, None, None, None)),
            'dg_world_reset_joint_state': ([vp, vp, i32, u64, vp, vp, vp, vp], (None, None, 0, 1, None, None, None, None))}
    for name in ENTRIES:
        fn = getattr(lib, name)   # AttributeError: not exported
        fn.restype, fn.argtypes = i32, args[name][0]
        assert fn(*args[name][1]) == DG_ERR_ARG, name
        assert name.encode() in lib.dg_last_error()


def slots_per_joint():
    """Workspace slots per joint of the query's pass as diy_gym_amd/csrc/dg_ikq.h defines them (``ikq_slots``): [q n][J 6n][v0 n][dth n]."""
    text = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_ikq.h')).read()
    m = re.search(r'constexpr int ikq_slots\(int n\) \{ return (\d+) \* n; \}', text)
    assert m and 'const int qo = sc.tr_off, jo = qo + n, vo = jo + 6 * n, dto = vo + n;' in text   # (the layout the figure counts)
    api = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_api.hip')).read()
    assert 'ikq_slots(n) > w->sc.tr_slots' in api   # the C entry checks that figure
    return int(m.group(1))


@pytest.mark.parametrize('max_lanes', [None, '4', '1'])
def test_nine_slots_per_joint_fit_every_fixed_base_body_of_the_repository(max_lanes, monkeypatch):
    """The query borrows the transient region and never enlarges it.  Every scene under tests/golden and examples, planned at 1, 70
    and 16 384 envs in the default workspace mode and in the narrow modes the GPU tests pin (the C entry refuses a body that does
    not fit: no scene may come to that)."""
    from diy_gym_amd import DIYGym
    from diy_gym_amd.backend import debug_plan
    from raycast_ref import RaycastOracleBackend   # (the oracle plus the ray caster the lidar scene's addon asks its backend for)
    import diy_gym_amd.examples  # noqa: F401
    need = slots_per_joint()
    assert need == 9
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
    assert seen >= 3 * 22   # (the scenes of test_dynamics_cabi.py and the two fixtures of the query)


def test_a_hook_addon_sees_the_mask_of_the_reset_in_progress():
    import yaml
    from diy_gym_amd import DIYGym
    from diy_gym_amd.addons.addon import Addon, AddonFactory
    from diy_gym_amd.config import Configuration
    from oracle_backend import OracleBackend
    seen = []

    class Watcher(Addon):
        def reset(self):
            seen.append(self.env.reset_mask)

    registry = AddonFactory.get().addons
    assert 'reset_watcher' not in registry
    AddonFactory.register_addon('reset_watcher', Watcher)
    try:
        cfg = yaml.safe_load(open(os.path.join(ROOT, 'tests', 'golden', 'ur_admittance.yaml')))
        cfg['watcher'] = {'addon': 'reset_watcher'}
        env = DIYGym(Configuration.from_dict('ur_admittance', cfg), num_envs=4, backend_factory=OracleBackend)
    finally:
        del registry['reset_watcher']
    assert len(env._hook_addons) == 1
    assert seen == [None]   # the constructor's full reset
    mask = torch.tensor([True, False, True, False])
    env.reset(mask)
    assert len(seen) == 2 and seen[1] is mask and env.reset_mask is mask
    env.reset()
    assert len(seen) == 3 and seen[2] is None and env.reset_mask is None
