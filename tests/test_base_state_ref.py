"""tests/base_state_ref.py pinned two ways, without a GPU: its two directions are inverses of each other, and the CPU checker -- handed
the stored values the helper computes -- reports the pose and velocity the helper was given.  Scenes: the cart of cart_tree.yaml (a
floating base whose inertial frame sits off the link frame) and a marble of contacts_marbles.yaml."""
import os

import numpy as np
import pytest

import base_state_ref as R
from diy_gym_amd import DIYGym
from oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = [('cart_tree.yaml', 'cart'), ('contacts_marbles.yaml', 'green_marble')]
B = 5
_ENVS = {}


def make(cfg):
    if cfg not in _ENVS:
        _ENVS[cfg] = DIYGym(os.path.join(GOLDEN, cfg), num_envs=B, seed=4, backend_factory=OracleBackend)
    return _ENVS[cfg]


def draws(seed):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1.0, 1.0, (B, 3)) + np.array([0.0, 0.0, 2.0])
    orn = rng.normal(size=(B, 4))
    orn /= np.linalg.norm(orn, axis=1, keepdims=True)
    return pos, orn, rng.uniform(-2.0, 2.0, (B, 3)), rng.uniform(-3.0, 3.0, (B, 3))


def same_rotation(a, b):
    """max |a -/+ b| over rows of unit quaternions (q and -q are one rotation)."""
    return np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1)).max()


def test_the_cart_has_a_report_offset_worth_testing():
    layout = make('cart_tree.yaml').layout
    p_r, q_r = R.report_offset(layout, make('cart_tree.yaml').models['cart'].uid)
    assert np.linalg.norm(p_r) > 1e-3 and abs(np.linalg.norm(q_r) - 1.0) < 1e-12


@pytest.mark.parametrize('cfg,model', CASES)
def test_round_trip_is_the_identity(cfg, model):
    env = make(cfg)
    uid = env.models[model].uid
    pos, orn, lin, ang = draws(11)
    back = R.report_from_stored(env.layout, uid, *R.stored_from_report(env.layout, uid, pos, 2.0 * orn, lin, ang))   # (any norm goes in)
    assert np.abs(back[0] - pos).max() < 1e-12 and same_rotation(back[1], orn) < 1e-12
    assert np.abs(back[2] - lin).max() < 1e-12 and np.abs(back[3] - ang).max() < 1e-12
    # without velocities both are zero
    p_l, q_l, v_l, w = R.stored_from_report(env.layout, uid, pos, orn)
    assert not v_l.any() and not w.any()


@pytest.mark.parametrize('cfg,model', CASES)
def test_the_checker_reports_what_the_helper_was_given(cfg, model):
    env = make(cfg)
    sim, uid = env.sim, env.models[model].uid
    assert not env.layout.body_fixed[uid]
    pos, orn, lin, ang = draws(12)
    p_l, q_l, v_l, w = R.stored_from_report(env.layout, uid, pos, orn, lin, ang)
    saved = sim.get_state()
    st = saved.copy()
    cols = R.base_columns(env.layout, uid)
    assert cols.stop - cols.start == 13
    st[:, cols] = np.concatenate([p_l, q_l, v_l, w], axis=1)
    sim.set_state(st)
    try:
        rep = sim.frame_state64(uid, -1, com=True)
    finally:
        sim.set_state(saved)
    assert np.abs(rep[:, 0:3] - pos).max() < 1e-9 and same_rotation(rep[:, 3:7], orn) < 1e-9
    assert np.abs(rep[:, 7:10] - lin).max() < 1e-9 and np.abs(rep[:, 10:13] - ang).max() < 1e-9
