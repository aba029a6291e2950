"""The fp64 restatement of the joint reaction query (tests/joint_wrench_ref.py) pinned to the checker's COMPILED force_torque_sensor,
and the scene side of the feature: ``builder.enable_joint_force_torque``.  No GPU.

The checker computes the compiled sensor in fp64 and publishes its observations as fp32, so the restatement -- fed the checker's own
state, its ``frame_state64`` poses and the contact list of its last substep -- must meet every published 3-vector within
``4 * 2^-24 * (1 + |vector|)``."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import contact_force_ref as cref
import joint_wrench_ref as ref
from oracle_backend import OracleBackend
from diy_gym_amd import DIYGym
from diy_gym_amd.addons.addon import Addon, AddonFactory
from diy_gym_amd.config import Configuration
from diy_gym_amd.scene import K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)   # make_vectors: the pressed-together inputs of the arms
EPS = 4.0 * 2.0 ** -24


def make(cfg, B=1, edit=None, registry=None):
    tree = yaml.safe_load(open(os.path.join(GOLDEN, cfg)))
    if edit:
        edit(tree)
    conf = Configuration.from_dict(os.path.splitext(os.path.basename(cfg))[0], tree)
    conf.source_dir = os.path.dirname(os.path.join(GOLDEN, cfg))
    names = AddonFactory.get().addons
    for name, cls in (registry or {}).items():
        AddonFactory.register_addon(name, cls)
    try:
        return DIYGym(conf, num_envs=B, backend_factory=OracleBackend)
    finally:
        for name in (registry or {}):
            del names[name]


def check_against_compiled(env, sensors, with_contacts=True):
    """Every compiled sensor ``(model, addon)`` of ``env`` after a checker step against the restatement; the largest error over bound."""
    sim, layout = env.sim, env.layout
    S = sim.get_state(); obs = sim.obs.numpy().astype(np.float64)
    contacts = cref.oracle_contact_forces(env) if (with_contacts and layout.warm_off >= 0) else [None] * env.num_envs
    worst = 0.0
    for model, addon in sensors:
        m = env.models[model]; a = m.addons[addon]
        poses = ref.link_poses(sim, layout, m.uid)
        for e in range(env.num_envs):
            want, _ = ref.joint_wrench(layout, m.uid, [a.frame_id], S[e], poses[e], contacts[e])
            got = obs[e, a.op.io_off:a.op.io_off + 6]
            for k in (0, 3):
                err = np.abs(want[0, k:k + 3] - got[k:k + 3]).max(); bound = EPS * (1.0 + np.linalg.norm(got[k:k + 3]))
                worst = max(worst, err / bound)
                assert err <= bound, (model, addon, e, k, want[0], got)
    return worst


def pendulum(q0, steps, edit=None):
    env = make(os.path.join('joint_wrench', 'pendulum_prop.yaml'), edit=edit)
    pend = env.models['pend'].uid
    qo = env.layout.link_state_off[env.layout.body_first_link[pend]]
    st = env.sim.get_state(); st[0, qo] = q0; env.sim.set_state(st)
    env.sim.set_motor_cfg(np.array([[0.0, 1.0, 0.0]]))   # motor off
    for _ in range(steps):
        env.sim.step(0)
    return env, qo


def test_pendulum_swinging_free():
    env, qo = pendulum(-1.0, 25)
    s = env.sim.get_state()[0]
    assert env.sim.contacts(0) == 0 and abs(s[qo + 1]) > 0.5
    check_against_compiled(env, [('pend', 'wrist'), ('pend', 'shoulder')])


def test_pendulum_at_rest_on_the_block():
    env, qo = pendulum(0.95, 400)
    s = env.sim.get_state()[0]
    assert env.sim.contacts(0) == 1 and abs(s[qo + 1]) < 2e-3
    check_against_compiled(env, [('pend', 'wrist'), ('pend', 'shoulder')])
    # the support shows: without the contact term the restatement misses the compiled wrist force by the support force
    pend = env.models['pend']; a = pend.addons['wrist']
    free, _ = ref.joint_wrench(env.layout, pend.uid, [a.frame_id], s, ref.link_poses(env.sim, env.layout, pend.uid)[0], None)
    got = env.sim.obs.numpy()[0, a.op.io_off:a.op.io_off + 3]
    assert np.linalg.norm(free[0, :3] - got) > 1.0


def test_pressed_arms_with_contacts():
    import make_vectors
    env = make('ur_arms_touching_ft.yaml', B=3)
    acts = make_vectors.press_actions(env, 25)
    for s in range(25):
        env.sim.step(env._all_slots, acts[s])
    assert min(env.sim.contacts(e) for e in range(3)) >= 1
    check_against_compiled(env, [('ur5_l', 'flange'), ('ur5_l', 'elbow'), ('ur5_r', 'shoulder')])


def test_floating_cart():
    env = make(os.path.join('joint_wrench', 'cart_tree_ft.yaml'), B=2)
    act = torch.tensor([[0.05, 0.2, -0.1], [0.2, -0.6, 0.8]])
    touched = False
    for s in range(70):
        env.sim.step(env._all_slots, act)
        touched = touched or env.sim.contacts(0) > 0
        if s in (5, 40, 69):   # falling, about to land or landed, lying on the plane
            check_against_compiled(env, [('cart', 'elbow')])
    assert touched and not env.layout.body_fixed[env.models['cart'].uid]


def test_after_reset_the_reading_is_the_gravity_load():
    """No acceleration across a reset and an empty cache: the plain-observe columns are the restatement without a contact term."""
    env, _ = pendulum(0.95, 400, edit=lambda tree: tree.update(hot_start=0))   # (the state after the reset is what the reset wrote)
    env.sim.reset()
    S = env.sim.get_state()[0]; pend = env.models['pend']
    qo = env.layout.link_state_off[env.layout.body_first_link[pend.uid]]
    po = int(env.layout.I[int(env.layout.I[K.H_OFF_BODY_I]) + pend.uid * K.BI_STRIDE + K.BI_PREV_OFF])
    assert S[po] == S[qo + 1] and S[env.layout.warm_off] == 0.0
    check_against_compiled(env, [('pend', 'wrist'), ('pend', 'shoulder')], with_contacts=False)


# --------------------------------------------------------------------------------------------------------------------- the scene
class _Enable(Addon):
    """What a user addon does in its compile(): ask the scene to keep the model's velocities at the start of the last substep."""
    def compile(self, builder):
        builder.enable_joint_force_torque(self.parent.uid)


def _body_row(layout, body):
    I = layout.I
    return I[int(I[K.H_OFF_BODY_I]) + body * K.BI_STRIDE:][:K.BI_STRIDE]


@pytest.mark.parametrize('cfg,model,extra', [(os.path.join('joint_wrench', 'cart_tree_ft.yaml'), 'cart', 3 + 6), ('ur_arms_touching_ft.yaml', 'ur5_r', 6)])
def test_enable_reserves_the_slots_once_and_shares_them_with_a_compiled_sensor(cfg, model, extra):
    sensors = {'cart': ['elbow'], 'ur5_r': ['shoulder']}[model]

    def without(tree):
        for s in sensors:
            del tree[model][s]
    bare = make(cfg, edit=without)
    assert _body_row(bare.layout, bare.models[model].uid)[K.BI_PREV_OFF] < 0

    def only_enable(tree):
        without(tree); tree[model]['a_enable'] = {'addon': 'enable_ft'}
    on = make(cfg, edit=only_enable, registry={'enable_ft': _Enable})
    row = _body_row(on.layout, on.models[model].uid)
    assert on.layout.state_dim == bare.layout.state_dim + extra
    assert on.layout.addon_off <= row[K.BI_PREV_OFF] and row[K.BI_PREV_OFF] + extra <= (on.layout.warm_off if on.layout.warm_off >= 0 else on.layout.state_dim)
    compiled = make(cfg)
    assert compiled.layout.state_dim == bare.layout.state_dim + extra
    for name in ('a_enable', 'z_enable'):   # compiled before / after the model's force_torque_sensor; twice is once
        def both(tree):
            tree[model][name] = {'addon': 'enable_ft'}; tree[model][name + '2'] = {'addon': 'enable_ft'}
        env = make(cfg, edit=both, registry={'enable_ft': _Enable})
        assert env.layout.state_dim == compiled.layout.state_dim
        assert _body_row(env.layout, env.models[model].uid)[K.BI_PREV_OFF] == _body_row(compiled.layout, compiled.models[model].uid)[K.BI_PREV_OFF]
        assert np.array_equal(env.layout.F, compiled.layout.F) and env.layout.warm_off == compiled.layout.warm_off


def test_the_slots_hold_the_velocities_at_the_start_of_the_last_substep():
    def edit(tree):
        del tree['cart']['elbow']; tree['cart']['keep'] = {'addon': 'enable_ft'}; tree['update_freq'] = 200
    env = make(os.path.join('joint_wrench', 'cart_tree_ft.yaml'), edit=edit, registry={'enable_ft': _Enable})
    layout = env.layout; cart = env.models['cart'].uid
    assert layout.substeps == 1
    row = _body_row(layout, cart); po, n, so = int(row[K.BI_PREV_OFF]), int(row[K.BI_N_LINKS]), int(row[K.BI_STATE_OFF])
    act = torch.tensor([[0.2, -0.6, 0.8]])
    for _ in range(3):
        before = env.sim.get_state()[0]
        env.sim.step(env._all_slots, act)
        after = env.sim.get_state()[0]
        first = layout.body_first_link[cart]
        qd = [before[layout.link_state_off[first + i] + K.LS_QD] for i in range(n)]
        assert np.array_equal(after[po:po + n], qd) and np.array_equal(after[po + n:po + n + 6], before[so + K.BS_LINVEL:so + K.BS_LINVEL + 6])
    assert np.abs(after[po:po + n + 6]).min() > 0.0


def test_attached_child_model_is_refused():
    env = make('contacts_child_gripper.yaml')
    alias = env.models['arm'].models['gripper'].uid
    with pytest.raises(NotImplementedError, match='attached child'):
        env.builder.enable_joint_force_torque(alias)
