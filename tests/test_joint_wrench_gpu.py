"""Joint reaction wrenches and motor torques on the GPU: ``dg_world_joint_wrench`` / ``env.sim.joint_reaction_forces``,
``dg_world_joint_efforts`` / ``env.sim.joint_motor_torques``, the ``joint_wrench_sensor`` addon and the two user addons of
tests/user_force_torque.py.

1. The readout against the fp64 restatement (tests/joint_wrench_ref.py) of the GPU's own numbers: the state from ``get_state``, link
   poses from the checker fed that state, contacts from ``contact_points`` + ``restate_from_query``.
2. Against the compiled force_torque_sensor on the same world: where nothing touches, and at rest.
3. Independent of the checker: the joint-axis component of the reading, moment moved to the joint origin, is inverse dynamics.
4. Every workspace mode gives the same bits.
5. Refusals, the state untouched, the addon, the user addons.

Every bound of 1 - 3 is 8 x the largest error measured on an MI355X over exactly these scenes and batches (MEASURED; DESIGN.md
"Joint reactions"), the project's margin for a readout against its restatement; 8 x measured must stay under the cap given beside it."""
import os
import sys

import numpy as np
import pytest
import yaml

import contact_force_ref as cref
import joint_wrench_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)   # make_vectors: the pressed-together inputs of the arms
pytestmark = pytest.mark.gpu

# largest error per quantity (MI355X): `readout` / `dynamics` per 3-vector relative to 1 + the sum of the norms of the terms the
# reference adds; `compiled_free` / `compiled_rest` per 3-vector relative to 1 + the norm of the compiled reading (_ft_error of
# tests/test_parity_gpu.py).  A kind without a figure (None) makes its test print what it measured and fail.
MEASURED = dict(readout=3.047e-06, dynamics=9.325e-07, compiled_free=9.996e-07, compiled_rest=1.558e-07)
CAP = dict(readout=1e-4, dynamics=1e-4, compiled_free=1e-4, compiled_rest=5e-3)


def within(kind, value):
    m = MEASURED[kind]
    assert m is not None, 'no MI355X measurement recorded for %r yet; this run measured %.3e' % (kind, value)
    assert 8.0 * m <= CAP[kind], (kind, m)   # a larger figure is a defect to be found, not a bound to be raised
    assert value <= 8.0 * m, (kind, value, 8.0 * m)


def make(cfg, B, edit=None, registry=None, cpu=False, **kw):
    from diy_gym_amd import DIYGym
    from diy_gym_amd.addons.addon import AddonFactory
    from diy_gym_amd.config import Configuration
    from oracle_backend import OracleBackend
    tree = yaml.safe_load(open(os.path.join(GOLDEN, cfg)))
    if edit:
        edit(tree)
    conf = Configuration.from_dict(os.path.splitext(os.path.basename(cfg))[0], tree)
    conf.source_dir = os.path.dirname(os.path.join(GOLDEN, cfg))
    names = AddonFactory.get().addons
    for name, cls in (registry or {}).items():
        AddonFactory.register_addon(name, cls)
    try:
        if cpu:
            return DIYGym(conf, num_envs=B, backend_factory=OracleBackend, **kw)
        return DIYGym(conf, num_envs=B, seed=5, device='cuda:0', **kw)
    finally:
        for name in (registry or {}):
            del names[name]


def host(t):
    return type(t)(*[None if x is None else x.cpu().numpy().copy() for x in t])


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def body_row(layout, body):
    from diy_gym_amd.scene import K
    I = layout.I
    return I[int(I[K.H_OFF_BODY_I]) + body * K.BI_STRIDE:][:K.BI_STRIDE]


PEND, ARMS, CART, SWING = (os.path.join('joint_wrench', 'pendulum_prop.yaml'), 'ur_arms_touching_ft.yaml', os.path.join('joint_wrench', 'cart_tree_ft.yaml'),
                           os.path.join('joint_wrench', 'arm_swing.yaml'))
ARM_JOINTS = ('ee_fixed_joint', 'elbow_joint', 'shoulder_lift_joint')


def drop_pendulum(env, B, lo=0.93, hi=0.97):
    """Motor off, the tool a few centimetres above the block: it lands and comes to rest."""
    qo = env.layout.link_state_off[env.layout.body_first_link[env.models['pend'].uid]]
    st = env.sim.get_state(); st[:, qo] = np.linspace(lo, hi, B); env.sim.set_state(st)
    env.sim.set_motor_cfg(np.array([[0.0, 1.0, 0.0]]))


def press(env, steps, apart=0.0):
    import make_vectors
    acts = make_vectors.press_actions(env, steps)
    if apart:   # every other env keeps its arms apart: nothing touches there
        acts[:, 1::2, 0] -= apart; acts[:, 1::2, 6] -= apart
    for s in range(steps):
        env.sim.step(env._all_slots, acts[s].to(env.device))


# ------------------------------------------------------------------------------------------ 1. the readout against its restatement
def readout_error(env, cpu, selectors):
    """Largest error of joint_reaction_forces over ``selectors`` ({model: joint names}) and every env; also the state's bits stay."""
    sim, layout = env.sim, env.layout
    S = sim.get_state()
    cpu.sim.set_state(S.astype(np.float64))
    if layout.warm_off >= 0:
        contacts, _ = cref.restate_from_query(host(sim.contact_points()), S, layout)
    else:
        contacts = [None] * env.num_envs
    worst, touched = 0.0, 0
    for model, names in selectors.items():
        m = env.models[model]; joints = [m.get_frame_id(n) for n in names]
        got = sim.joint_reaction_forces(m.uid, joints).cpu().numpy()
        assert got.shape == (env.num_envs, len(joints), 6) and np.isfinite(got).all()
        poses = ref.link_poses(cpu.sim, layout, m.uid)
        for e in range(env.num_envs):
            want, mags = ref.joint_wrench(layout, m.uid, joints, S[e], poses[e], contacts[e])
            free, _ = ref.joint_wrench(layout, m.uid, joints, S[e], poses[e], None)
            touched += int(np.abs(want - free).max() > 1e-3)
            worst = max(worst, float(ref.errors(got[e], want, mags).max()))
    assert np.array_equal(bits(S), bits(sim.get_state()))   # the state is never written
    return worst, touched


def efforts_are_the_sensors(env, model, addon='joints'):
    m = env.models[model]; a = m.addons[addon]; n = a._n
    k = a.op.io_off + n * (1 + bool(a.include_velocity))
    got = env.sim.joint_motor_torques(m.uid).cpu().numpy()
    assert got.shape == (env.num_envs, n) and np.array_equal(bits(got), bits(env.sim.obs[:, k:k + n].cpu().numpy()))
    return float(np.abs(got).max())


def test_readout_pendulum_on_the_prop():
    B = 3
    env, cpu = make(PEND, B), make(PEND, B, cpu=True)
    drop_pendulum(env, B)
    worst, touched = 0.0, 0
    for step in range(300):
        env.sim.step(0)
        if step in (5, 60, 299):   # swinging free, bouncing on the block, at rest on it
            w, t = readout_error(env, cpu, {'pend': ['mount', 'hinge']}); worst = max(worst, w); touched += t
    assert touched >= B   # the support shows in the readings
    efforts_are_the_sensors(env, 'pend')
    print('MEASURE readout pendulum B=%d %.3e' % (B, worst))
    within('readout', worst)


def test_readout_pressed_arms():
    B = 70
    def effort(tree):   # (the scene's joint_state_sensors report no effort: ask for it, in both worlds)
        tree['ur5_l']['joint_state']['include_effort'] = tree['ur5_r']['joint_state']['include_effort'] = True
    env, cpu = make(ARMS, B, edit=effort), make(ARMS, B, edit=effort, cpu=True)
    press(env, 45)
    worst, touched = readout_error(env, cpu, {'ur5_l': ARM_JOINTS, 'ur5_r': ARM_JOINTS})
    assert touched >= B
    assert efforts_are_the_sensors(env, 'ur5_l', 'joint_state') > 0.0 and efforts_are_the_sensors(env, 'ur5_r', 'joint_state') > 0.0
    print('MEASURE readout arms B=%d %.3e' % (B, worst))
    within('readout', worst)


def test_readout_floating_cart_dropped_on_the_plane():
    import torch
    B = 3
    env, cpu = make(CART, B), make(CART, B, cpu=True)
    act = torch.tensor([[0.05, 0.2, -0.1], [0.2, -0.6, 0.8], [-0.05, 0.9, -0.7]], device=env.device)
    worst = 0.0
    for step in range(70):
        env.sim.step(env._all_slots, act)
        if step in (5, 40, 69):
            w, _ = readout_error(env, cpu, {'cart': ['slide', 'hinge_a', 'hinge_b', 'tip_joint']}); worst = max(worst, w)
    assert int(env.sim.contact_points(want=('id', )).count.min()) >= 1   # it lies on the plane
    assert efforts_are_the_sensors(env, 'cart') > 0.0   # (a floating base: joint_states would refuse it)
    print('MEASURE readout cart B=%d %.3e' % (B, worst))
    within('readout', worst)


# ------------------------------------------------------------------------------- 2. against the compiled sensor on the same world
def compiled_columns(env, model, addon):
    a = env.models[model].addons[addon]
    return env.sim.obs[:, a.op.io_off:a.op.io_off + 6].cpu().numpy().astype(np.float64), a.frame_id


def ft_error(got, want):
    """_ft_error of tests/test_parity_gpu.py: per 3-vector, relative to 1 + the norm of the compiled reading; per env."""
    return np.max([np.abs(got[:, k:k + 3] - want[:, k:k + 3]).max(1) / (1.0 + np.linalg.norm(want[:, k:k + 3], axis=1)) for k in (0, 3)], axis=0)


def test_compiled_sensor_where_nothing_touches():
    from diy_gym_amd.scene import K
    B = 37
    env = make(ARMS, B)
    press(env, 25, apart=0.3)
    S = env.sim.get_state(); count = env.sim.contact_points(want=('id', )).count.cpu().numpy()
    free = np.nonzero((count == 0) & (S[:, env.layout.warm_off] == 0))[0]
    assert len(free) >= 10 and (count > 0).sum() >= 10
    worst = 0.0
    for model, addon in (('ur5_l', 'flange'), ('ur5_l', 'elbow'), ('ur5_r', 'shoulder')):
        want, frame = compiled_columns(env, model, addon)
        got = env.sim.joint_reaction_forces(env.models[model].uid, [frame])[:, 0].cpu().numpy().astype(np.float64)
        worst = max(worst, float(ft_error(got[free], want[free]).max()))
        assert np.abs(want[free]).max() > 1.0
    print('MEASURE compiled_free arms B=%d %.3e over %d envs' % (B, worst, len(free)))
    within('compiled_free', worst)


def test_compiled_sensor_at_rest_on_the_prop():
    B = 3
    env = make(PEND, B, engine=dict(residual_threshold=1e-13))
    drop_pendulum(env, B)
    for _ in range(300):
        env.sim.step(0)
    assert env.sim.contact_points(want=('id', )).count.cpu().numpy().tolist() == [1] * B
    worst = 0.0
    for addon in ('wrist', 'shoulder'):
        want, frame = compiled_columns(env, 'pend', addon)
        got = env.sim.joint_reaction_forces(env.models['pend'].uid, [frame])[:, 0].cpu().numpy().astype(np.float64)
        worst = max(worst, float(ft_error(got, want).max()))
    print('MEASURE compiled_rest pendulum B=%d %.3e' % (B, worst))
    within('compiled_rest', worst)


# ------------------------------------------------------------------------------------------------ 3. independent of the checker
def test_joint_axis_component_is_inverse_dynamics():
    """A UR5 alone (no contact pair in the scene, no impulse cache), driven between poses: for every movable joint the reading's
    moment, moved from the child link's inertial origin to the joint origin and projected on the joint axis, is
    calculate_inverse_dynamics(q, qd, (qd - prev) / h)."""
    import torch
    from diy_gym_amd.scene import K
    B = 3
    env = make(SWING, B); sim, layout = env.sim, env.layout
    assert layout.warm_off < 0 and layout.max_contacts == 0
    arm = env.models['arm']; uid = arm.uid
    gen = torch.Generator().manual_seed(2)
    worst = 0.0
    for step in range(12):
        sim.step(env._all_slots, (torch.rand((B, 6), generator=gen) * 2.0 - 1.0).to(env.device))
        if step not in (3, 11):
            continue
        S = sim.get_state(); row = body_row(layout, uid); po, n, first = int(row[K.BI_PREV_OFF]), int(row[K.BI_N_LINKS]), int(row[K.BI_FIRST_LINK])
        q, qd = (t.clone() for t in sim.joint_states(uid))
        prev = torch.as_tensor(S[:, po:po + n], device=env.device)
        qdd = (qd - prev) * float(np.float32(1.0) / np.float32(layout.dt))
        tau = sim.calculate_inverse_dynamics(uid, q, qd, qdd).cpu().numpy().astype(np.float64)
        joints = list(arm.flat.dof_to_joint)
        W = sim.joint_reaction_forces(uid).cpu().numpy().astype(np.float64)
        com = sim.link_states(uid, joints, com=True).cpu().numpy().astype(np.float64)
        link = sim.link_states(uid, joints, com=False).cpu().numpy().astype(np.float64)
        LF = ref.table(layout, K.H_OFF_LINK_F, int(layout.I[K.H_N_LINKS]), K.LF_STRIDE, True)
        assert np.abs(qdd.cpu().numpy()).max() > 1.0   # it moves
        for e in range(B):
            for i in range(n):
                Rs, Rj = ref.quat_mat(com[e, i, 3:7]), ref.quat_mat(link[e, i, 3:7])
                F, M = Rs @ W[e, i, 0:3], Rs @ W[e, i, 3:6]
                arm_term = np.cross(com[e, i, 0:3] - link[e, i, 0:3], F)
                axis = Rj @ LF[first + i, K.LF_AXIS:K.LF_AXIS + 3]
                got = float(axis @ (M + arm_term))
                worst = max(worst, abs(got - tau[e, i]) / (1.0 + np.linalg.norm(M) + np.linalg.norm(arm_term)))
    print('MEASURE dynamics arm B=%d %.3e' % (B, worst))
    within('dynamics', worst)


# ------------------------------------------------------------------------------------------------------- 4. every workspace mode
LDS_SWITCHES = [({}, 64), ({'DG_MAX_LANES': '32'}, 32), ({'DG_MAX_LANES': '16'}, 16), ({'DG_MAX_LANES': '8'}, 8), ({'DG_MAX_LANES': '4'}, 4), ({'DG_MAX_LANES': '1'}, 1)]
MODES = {
    (ARMS, 70, 45): [({}, 64), ({'DG_MAX_LANES': '16'}, 16), ({'DG_MAX_LANES': '8'}, 0), ({'DG_NO_SLICED_GLOBAL': '1'}, 64)],
    # (the planner keeps the narrow LDS modes from a scene of one joint: below 16 envs per wavefront the pendulum gets the global workspace)
    (PEND, 3, 60): [(sw, lanes if lanes >= 16 else 0) for sw, lanes in LDS_SWITCHES],
    (CART, 3, 60): LDS_SWITCHES,
}


def both_calls(env):
    out = []
    for m in env.models.values():
        if env.layout.body_n_links[m.uid] < 1:
            continue
        out.append(env.sim.joint_reaction_forces(m.uid, list(range(min(len(m.flat.frames), 16)))).cpu().numpy().copy())
        out.append(env.sim.joint_motor_torques(m.uid).cpu().numpy().copy())
    return out


def mode_worlds(monkeypatch, name, B, steps, modes):
    """The answers of a first world run `steps` steps, then per entry of `modes` (switches, lanes, answers) of a world of that mode
    given the first world's state."""
    import torch
    switches = ['DG_MAX_LANES', 'DG_NO_SLICED_GLOBAL']
    for v in switches:
        monkeypatch.delenv(v, raising=False)
    first = make(name, B)
    if name == PEND:
        drop_pendulum(first, B)
        for _ in range(steps):
            first.sim.step(0)
    elif name == CART:
        for _ in range(steps):
            first.sim.step(first._all_slots, torch.tensor([[0.05, 0.2, -0.1], [0.2, -0.6, 0.8], [-0.05, 0.9, -0.7]], device=first.device))
    else:
        press(first, steps)
    S = first.sim.get_state(); want = both_calls(first)
    assert int(first.sim.contact_points(want=('id', )).count.min()) >= 1 and np.abs(want[0]).max() > 1.0
    yield None, None, want
    for sw, lanes in modes:
        for v in switches:
            monkeypatch.delenv(v, raising=False)
        for k, v in sw.items():
            monkeypatch.setenv(k, v)
        env = make(name, B)
        assert env.sim.lanes == lanes, (sw, env.sim.lanes)
        env.sim.set_state(S)
        yield sw, lanes, both_calls(env)
        env.close()


@pytest.mark.parametrize('name,B,steps', sorted(MODES))
def test_every_workspace_mode_gives_the_same_bits(monkeypatch, name, B, steps):
    """One state, set into worlds of every mode the scene can run in, gives bit-identical answers: the pressed arms at 70 envs in
    the default world, 16 envs per wavefront, the mode DG_MAX_LANES=8 leaves and without the sliced global mode; the pendulum on the
    prop at 3 envs under DG_MAX_LANES = 32 / 16 / 8 / 4 / 1 (64, 32, 16 envs per wavefront, then the global workspace); the floating cart
    lying on the plane at 3 envs under the same switches, which reach every LDS mode (64, 32, 16, 8, 4 envs per wavefront and one).  The
    cart at one env per wavefront is the case that needed the kernel's own kinematics pass: on the shared, contracted kinematics it
    differed from the other modes by up to 5 ulp in single components."""
    want = None
    for sw, lanes, got in mode_worlds(monkeypatch, name, B, steps, MODES[(name, B, steps)]):
        if want is None:
            want = got
            continue
        for i, (a, c) in enumerate(zip(want, got)):
            assert np.array_equal(bits(a), bits(c)), (sw, lanes, i)


# ------------------------------------------------------------------------------------ 5. refusals, state untouched, the addons
def test_refusals():
    env = make(ARMS, 3); sim = env.sim
    arm = env.models['ur5_l']; nfr = len(arm.flat.frames)
    for bad in ([nfr], [-1], [], [0] * 17):
        with pytest.raises(ValueError):
            sim.joint_reaction_forces(arm.uid, bad)
    with pytest.raises(ValueError):
        sim.joint_reaction_forces(99)
    with pytest.raises(ValueError):
        sim.joint_motor_torques(99)
    # the C entry itself: n, frame, masks
    from diy_gym_amd.backend import JointSelector, _ptr, joint_wrench_selectors
    import torch
    _, _, arr = joint_wrench_selectors(env.layout, arm.uid, [0, 1])
    out = torch.zeros((3, 2, 6), device=env.device)
    call = lambda a, n: sim.lib.dg_world_joint_wrench(sim.handle, _ptr(sim.state), arm.uid, a, n, _ptr(out), sim._stream())
    assert call(arr, 0) == -4 and call(arr, 17) == -4 and call(arr, 2) == 0
    bad = (JointSelector * 2)(); bad[0].frame = nfr
    assert call(bad, 1) == -4 and b'no frame' in sim.lib.dg_last_error()
    bad[0].frame = 0; bad[0].link_mask = 1 << 6
    assert call(bad, 1) == -4
    assert sim.lib.dg_world_joint_wrench(sim.handle, _ptr(sim.state), 7, arr, 2, _ptr(out), sim._stream()) == -4
    # a body without saved velocities: the message names the remedy; joint_motor_torques needs none
    bare = make('contacts_arms.yaml', 3)
    with pytest.raises(ValueError, match='enable_joint_force_torque'):
        bare.sim.joint_reaction_forces(bare.models['ur5_l'].uid)
    rc = bare.sim.lib.dg_world_joint_wrench(bare.sim.handle, _ptr(bare.sim.state), bare.models['ur5_l'].uid, arr, 2, _ptr(out), bare.sim._stream())
    assert rc == -4 and b'enable_joint_force_torque' in bare.sim.lib.dg_last_error()
    assert tuple(bare.sim.joint_motor_torques(bare.models['ur5_l'].uid).shape) == (3, 6)
    # a frozen body
    child = make('contacts_child_gripper.yaml', 3)
    with pytest.raises(ValueError, match='frozen'):
        child.sim.joint_reaction_forces(child.models['plane'].uid, [0])
    plane_sel = (JointSelector * 1)()
    rc = child.sim.lib.dg_world_joint_wrench(child.sim.handle, _ptr(child.sim.state), child.models['plane'].uid, plane_sel, 1, _ptr(out), child.sim._stream())
    assert rc == -4 and b'frozen' in child.sim.lib.dg_last_error()
    with pytest.raises(ValueError, match='no joints'):
        child.sim.joint_motor_torques(child.models['plane'].uid)
    # an alias uid gives the parent's nv
    alias = child.models['arm'].models['gripper'].uid
    assert tuple(child.sim.joint_motor_torques(alias).shape) == (3, int(child.layout.body_n_links[child.models['arm'].uid]))
    with pytest.raises(ValueError, match='attached'):
        child.sim.joint_reaction_forces(alias, [0])


def test_world_with_pairs_and_without_impulse_cache_is_refused():
    env = make(ARMS, 3, engine={'warmstart': 0, 'warmstart_friction': 0})
    assert env.layout.warm_off < 0 and env.layout.max_contacts > 0
    with pytest.raises(RuntimeError, match='impulse cache'):
        env.sim.joint_reaction_forces(env.models['ur5_l'].uid)
    with pytest.raises(RuntimeError, match='impulse cache'):
        env.sim.contact_forces()
    assert tuple(env.sim.joint_motor_torques(env.models['ur5_l'].uid).shape) == (3, 6)


def test_teleport_shows_as_a_jump_and_the_old_state_reads_as_before():
    import torch
    B = 3
    env = make(SWING, B); sim = env.sim; uid = env.models['arm'].uid
    act = torch.tensor([[0.3, -0.55, 1.22, -1.51, 0.84, 0.1]] * B, device=env.device)
    for _ in range(5):
        sim.step(env._all_slots, act)
    S = sim.get_state(); before = sim.joint_reaction_forces(uid).cpu().numpy().copy()
    q, qd = (t.clone() for t in sim.joint_states(uid))
    sim.reset_joint_state(uid, q, qd + 0.5)
    jumped = sim.joint_reaction_forces(uid).cpu().numpy().copy()
    assert np.abs(jumped - before).max() > 10.0   # 0.5 rad/s over one substep
    sim.set_state(S)
    assert np.array_equal(bits(sim.joint_reaction_forces(uid).cpu().numpy()), bits(before))
    env.reset()   # after a reset: no acceleration, the plain gravity load -- what a second reading gives too
    a = sim.joint_reaction_forces(uid).cpu().numpy().copy()
    assert np.array_equal(bits(a), bits(sim.joint_reaction_forces(uid).cpu().numpy())) and np.abs(a).max() > 1.0


def test_joint_wrench_sensor_reports_the_calls_and_leaves_the_state_alone():
    import torch
    cfg = os.path.join('joint_wrench', 'pendulum_prop_sensor.yaml'); B = 3
    env, plain = make(cfg, B), make(cfg, B)   # (the second one is stepped without ever evaluating its sensors)
    for e in (env, plain):
        drop_pendulum(e, B)
    for _ in range(120):
        obs = env.step({})[0]
        plain.sim.step(plain._all_slots)
    pend = env.models['pend']; ids = [pend.get_frame_id('mount'), pend.get_frame_id('hinge')]
    o = obs['pend']['reactions']; w = env.sim.joint_reaction_forces(pend.uid, ids)
    assert torch.equal(o['force'], w[:, :, 0:3].reshape(B, 6)) and torch.equal(o['torque'], w[:, :, 3:6].reshape(B, 6))
    assert torch.equal(o['motor_torque'], env.sim.joint_motor_torques(pend.uid))
    w1 = env.sim.joint_reaction_forces(pend.uid, [ids[1]])
    assert torch.equal(obs['pend']['load']['force'], w1[:, 0, 0:3]) and torch.equal(obs['pend']['load']['torque'], w1[:, 0, 3:6])
    assert float(o['force'].abs().max()) > 1.0
    assert np.array_equal(bits(env.sim.get_state()), bits(plain.sim.get_state()))


def test_user_addons_written_on_the_two_calls():
    """PyForceTorqueSensor reserves the saved velocities in its own compile() and reports the query's rows; PyElectricityCost is the
    compiled reward column within 4 nv 2^-24 sum |tau qd|."""
    import torch
    from user_force_torque import PyElectricityCost, PyForceTorqueSensor
    B = 3

    def edit(tree):
        del tree['arm']['reactions']
        tree['arm']['wrist'] = {'addon': 'py_force_torque', 'frame': 'ee_fixed_joint'}
        tree['arm']['py_power'] = {'addon': 'py_electricity', 'multiplier': 0.5}
    env = make(SWING, B, edit=edit, registry={'py_force_torque': PyForceTorqueSensor, 'py_electricity': PyElectricityCost})
    arm = env.models['arm']
    from diy_gym_amd.scene import K
    assert body_row(env.layout, arm.uid)[K.BI_PREV_OFF] >= env.layout.addon_off and len(env._hook_addons) == 1   # (the sensor has a compile(): only the reward is a hook)
    gen = torch.Generator().manual_seed(4)
    for _ in range(8):
        action = {'arm': {'controller': (torch.rand((B, 6), generator=gen) * 2.0 - 1.0).to(env.device)}}
        obs, rew, _, _ = env.step(action)
    w = env.sim.joint_reaction_forces(arm.uid, [arm.get_frame_id('ee_fixed_joint')])[:, 0]
    assert torch.equal(obs['arm']['wrist']['force'], w[:, 0:3]) and torch.equal(obs['arm']['wrist']['torque'], w[:, 3:6])
    assert float(w.abs().max()) > 0.1
    tau, qd = env.sim.joint_motor_torques(arm.uid).double(), env.sim.joint_states(arm.uid)[1].double()
    scale = (tau * qd).abs().sum(1)
    got, want = arm.addons['py_power'].reward().double(), arm.addons['power'].reward().double()
    assert float(scale.min()) > 0.0 and bool(((got - want).abs() <= 4.0 * 6 * 2.0 ** -24 * scale).all())
