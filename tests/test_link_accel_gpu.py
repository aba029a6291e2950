"""Link accelerations and IMU readings on the GPU: ``dg_world_link_accelerations`` / ``env.sim.link_accelerations`` and the
``imu_sensor`` addon.

1. The readout against the fp64 restatement (tests/link_accel_ref.py) of the GPU's own numbers: the state from ``get_state``, link
   poses from the checker fed that state.  All five vectors, ``com`` both ways, non-trivial mounts.
2. Known answers: the marble at rest, a rotated mount, after ``reset()``, the spinning marble.
3. Against ``joint_reaction_forces``: mass x (lin_acc - g) at the centre of mass of a free pendulum is the hinge's force.
4. Every workspace mode gives the same bits.
5. A teleport shows as a jump, the next step clears it, the old state reads the old bits.
6. Refusals, at the C entry and from ``env.sim``; a world without the contact impulse cache is taken.
7. The addon reports the call's columns and leaves the state alone.

Every bound of 1 - 3 is 8 x the largest error measured on an MI355X over exactly these scenes and batches (MEASURED; DESIGN.md
"Link accelerations"), the project's margin for a readout against its restatement -- fp32 velocity differences over h = 1/480 s;
8 x measured must stay under the cap 1e-4, the cap of the joint-reaction readout."""
import os

import numpy as np
import pytest
import yaml

import joint_wrench_ref as jref
import link_accel_ref as ref
from test_joint_wrench_gpu import ARMS, CART, MODES, PEND, SWING, bits, body_row, drop_pendulum, make, press

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DRONE = os.path.join(ROOT, 'examples', 'drone_pilot', 'imu', 'drone_pilot_imu.yaml')
MARBLE, PEND_IMU = os.path.join('imu_sensor', 'marble_imu.yaml'), os.path.join('imu_sensor', 'pendulum_imu.yaml')
pytestmark = pytest.mark.gpu
G = 9.81

# largest error per scene kind (MI355X): per 3-vector relative to 1 + the sum of the norms of the terms the reference adds.  A kind
# without a figure (None) makes its test print what it measured and fail.
MEASURED = dict(readout_pendulum=1.259e-07, readout_cart=1.623e-07, readout_drone=6.285e-08, readout_arms=3.824e-07, known_rest=6.196e-08, known_spin=1.282e-08, reaction=1.738e-07)
CAP = 1e-4

MOUNT_POS = [[0.03, -0.02, 0.05], [-0.1, 0.04, 0.02], [0., 0., 0.], [0.2, 0.1, -0.3], [0.01, 0.02, 0.03]]
MOUNT_ORN = [[0.1, -0.2, 0.3, 0.9], [0., 0., 0., 1.], [0.5, 0.5, -0.5, 0.5], [-0.3, 0.1, 0.2, 0.8], [0., 1., 0., 0.]]   # (not normalised: the call does)


def within(kind, value):
    m = MEASURED[kind]
    assert m is not None, 'no MI355X measurement recorded for %r yet; this run measured %.3e' % (kind, value)
    assert 8.0 * m <= CAP, (kind, m)   # a larger figure is a defect to be found, not a bound to be raised
    assert value <= 8.0 * m, (kind, value, 8.0 * m)


def make_imu(cfg, B, edit=None, cpu=False, **kw):
    """A scene that carries imu_sensor addons: on the GPU, or on the checker behind a stand-in that answers the addon's call with
    zeros (the checker is asked for poses only)."""
    import torch
    import diy_gym_amd.examples  # noqa: F401  (propellor, fell_over)
    from diy_gym_amd import DIYGym
    from diy_gym_amd.backend import LinkAccelerations
    from diy_gym_amd.config import Configuration
    from oracle_backend import OracleBackend

    class Stub(OracleBackend):
        def link_accelerations(self, body, frames=None, local_pos=None, local_orn=None, com=False):
            return LinkAccelerations(*([torch.zeros((self.num_envs, 1 if frames is None else len(frames), 3))] * 5))
    path = cfg if os.path.isabs(cfg) else os.path.join(GOLDEN, cfg)
    tree = yaml.safe_load(open(path))
    if edit:
        edit(tree)
    conf = Configuration.from_dict(os.path.splitext(os.path.basename(path))[0], tree)
    conf.source_dir = os.path.dirname(path)
    if cpu:
        return DIYGym(conf, num_envs=B, backend_factory=Stub, **kw)
    return DIYGym(conf, num_envs=B, seed=5, device='cuda:0', **kw)


def call(sim, uid, frames, pos, orn, com):
    r = sim.link_accelerations(uid, frames, pos, orn, com=com)
    base = r.lin_acc._base if r.lin_acc._base is not None else r.lin_acc
    out = base.cpu().numpy().copy()
    assert out.shape == (sim.num_envs, len(frames), 15) and np.isfinite(out).all()
    for i, v in enumerate(r):
        assert np.array_equal(bits(v.cpu().numpy()), bits(out[:, :, 3 * i:3 * i + 3]))
    return out


# ------------------------------------------------------------------------------------------ 1. the readout against its restatement
def readout_error(env, cpu, selectors):
    """Largest error of link_accelerations over ``selectors`` ({model: frames}), both ``com``, the mounts above and every env; the
    state's bits stay.  One call per model and ``com``."""
    sim, layout = env.sim, env.layout
    S = sim.get_state()
    cpu.sim.set_state(S.astype(np.float64))
    worst = np.zeros(5)
    for model, frames in selectors.items():
        m = env.models[model]; frames = list(frames); n = len(frames)
        poses = jref.link_poses(cpu.sim, layout, m.uid)
        for com in (False, True):
            got = call(sim, m.uid, frames, MOUNT_POS[:n], MOUNT_ORN[:n], com)
            sel = [(frames[k], int(com), MOUNT_POS[k], MOUNT_ORN[k]) for k in range(n)]
            for e in range(env.num_envs):
                want, mags = ref.link_accel(layout, m.uid, sel, S[e], poses[e])
                worst = np.maximum(worst, ref.errors(got[e], want, mags).max(0))
    assert np.array_equal(bits(S), bits(sim.get_state()))   # the state is never written
    return worst


def report(kind, scene, B, worst):
    print('MEASURE %s %s B=%d %s -> %.3e' % (kind, scene, B, ' '.join('%s=%.3e' % kv for kv in zip(ref.NAMES, worst)), worst.max()))
    within(kind, float(worst.max()))


def test_readout_pendulum_on_the_prop():
    B = 3
    env, cpu = make(PEND, B), make(PEND, B, cpu=True)
    drop_pendulum(env, B)
    pend = env.models['pend']
    worst = np.zeros(5)
    for step in range(300):
        env.sim.step(0)
        if step in (5, 60, 299):   # swinging free, bouncing on the block, at rest on it
            worst = np.maximum(worst, readout_error(env, cpu, {'pend': [pend.get_frame_id('mount'), pend.get_frame_id('hinge')]}))
    report('readout_pendulum', 'pendulum', B, worst)


def test_readout_floating_cart_dropped_on_the_plane():
    import torch
    B = 3
    env, cpu = make(CART, B), make(CART, B, cpu=True)
    cart = env.models['cart']
    frames = [-1] + [cart.get_frame_id(n) for n in ('slide', 'hinge_a', 'hinge_b', 'tip_joint')]
    act = torch.tensor([[0.05, 0.2, -0.1], [0.2, -0.6, 0.8], [-0.05, 0.9, -0.7]], device=env.device)
    worst = np.zeros(5)
    for step in range(70):
        env.sim.step(env._all_slots, act)
        if step in (5, 40, 69):   # falling, landing, lying on the plane
            worst = np.maximum(worst, readout_error(env, cpu, {'cart': frames}))
    assert int(env.sim.contact_points(want=('id', )).count.min()) >= 1
    report('readout_cart', 'cart', B, worst)


def test_readout_drone_a_jointless_floating_body():
    import torch
    B = 3
    env, cpu = make_imu(DRONE, B), make_imu(DRONE, B, cpu=True)
    assert env.layout.body_n_links[env.models['drone'].uid] == 0
    act = torch.tensor([[0.9, 0.9, 0.9, 0.9], [0.9, 0.5, 0.9, 0.5], [0.2, 0.9, 0.6, 1.0]], device=env.device)
    worst = np.zeros(5)
    for step in range(25):
        env.sim.step(env._all_slots, act)
        if step in (3, 24):
            worst = np.maximum(worst, readout_error(env, cpu, {'drone': [-1]}))
    assert float(np.abs(call(env.sim, env.models['drone'].uid, [-1], None, None, False)[:, 0, :6]).max()) > 1.0   # it accelerates and turns
    report('readout_drone', 'drone', B, worst)


def test_readout_pressed_arms():
    B = 70
    env, cpu = make(ARMS, B), make(ARMS, B, cpu=True)
    assert env.sim.par   # a helper-wave world
    press(env, 45)
    sel = {name: [env.models[name].get_frame_id('ee_fixed_joint'), env.models[name].get_frame_id('elbow_joint')] for name in ('ur5_l', 'ur5_r')}
    worst = readout_error(env, cpu, sel)
    assert int(env.sim.contact_points(want=('id', )).count.min()) >= 1
    report('readout_arms', 'arms', B, worst)


# ------------------------------------------------------------------------------------------------------------- 2. known answers
def test_marble_at_rest_a_rotated_mount_and_after_reset():
    from diy_gym_amd.mathx import quat_from_euler
    B = 3
    env = make_imu(MARBLE, B); sim = env.sim; uid = env.models['marble'].uid
    tilted = env.models['marble'].addons['tilted']
    Rm = jref.quat_mat(quat_from_euler([0.3, -0.2, 0.5]))
    want = np.zeros((2, 15))
    want[0, 6:9], want[0, 12:15] = [0, 0, G], [0, 0, -1]
    want[1, 6:9], want[1, 12:15] = Rm.T @ [0, 0, G], Rm.T @ [0, 0, -1]
    mags = np.array([[0., 0., G, 0., 1.]] * 2)
    worst = np.zeros(5)

    def check():
        got = call(sim, uid, [-1, -1], [[0., 0., 0.], tilted.local_pos], [[0., 0., 0., 1.], tilted.local_orn], False)
        return np.max([ref.errors(got[e], want, mags).max(0) for e in range(B)], axis=0)
    for step in range(300):
        obs = env.step({})[0]
        if step in (0, 1, 2, 5, 20, 100, 299):
            worst = np.maximum(worst, check())
    assert float((obs['marble']['imu']['linear_acceleration'] - obs['marble']['imu']['linear_acceleration'].new_tensor([0, 0, G])).abs().max()) < 1e-3
    env.reset()   # the hot-start step of a marble at rest: no acceleration, specific_force = -R_s^T g
    worst = np.maximum(worst, check())
    report('known_rest', 'marble', B, worst)


def test_spinning_marble():
    """reset_base_state(ang_vel = omega z) in the air, one step: lin_acc at r = (0.1, 0, 0) minus lin_acc at the origin, the angular
    acceleration's (the damping's) alpha x r taken off, is -omega^2 r."""
    import torch
    B = 3

    def lift(tree):
        tree['marble']['xyz'] = [0, 0, 3.0]
    env = make_imu(MARBLE, B, edit=lift); sim = env.sim; uid = env.models['marble'].uid
    omega = torch.tensor([[0., 0., 4.0], [0., 0., -7.0], [0., 0., 1.5]], device=env.device)
    sim.reset_base_state(uid, ang_vel=omega)
    sim.step(0)
    r = np.array([0.1, 0., 0.])
    got = call(sim, uid, [-1, -1], [[0., 0., 0.], list(r)], None, False).astype(np.float64)
    ls = sim.link_states(uid, [-1], com=False).cpu().numpy().astype(np.float64)[:, 0]
    worst = 0.0
    for e in range(B):
        w = ls[e, 10:13]; rw = jref.quat_mat(ls[e, 3:7]) @ r
        assert abs(w[2] - float(omega[e, 2])) < 0.05 * abs(float(omega[e, 2])) and np.abs(w[:2]).max() < 1e-6
        al = got[e, 0, 3:6]; t = np.cross(al, rw)
        want = got[e, 0, 0:3] + t - (w @ w) * rw
        scale = 1.0 + np.linalg.norm(got[e, 0, 0:3]) + np.linalg.norm(t) + (w @ w) * 0.1
        worst = max(worst, float(np.abs(got[e, 1, 0:3] - want).max() / scale))
        assert np.linalg.norm(got[e, 1, 0:3] - got[e, 0, 0:3]) == pytest.approx(float(omega[e, 2]) ** 2 * 0.1, rel=0.05)
        worst = max(worst, float(np.abs(got[e, 1, 9:12] - w).max() / (1.0 + np.linalg.norm(w))))   # (spinning about z: the gyro reads w)
    print('MEASURE known_spin marble B=%d %.3e' % (B, worst))
    within('known_spin', worst)


# ------------------------------------------------------------------------------------------- 3. against joint_reaction_forces
def test_mass_times_specific_force_is_the_hinge_reaction_of_a_free_pendulum():
    from diy_gym_amd.scene import K
    B = 3
    env = make_imu(PEND_IMU, B); sim, layout = env.sim, env.layout
    assert layout.max_contacts == 0
    pend = env.models['pend']; uid = pend.uid; hinge = pend.get_frame_id('hinge')
    first = int(layout.body_first_link[uid]); qo = layout.link_state_off[first]
    st = sim.get_state(); st[:, qo] = [-1.0, 0.4, 2.0]; sim.set_state(st)
    sim.set_motor_cfg(np.array([[0.0, 1.0, 0.0]]))   # motor off
    LF = jref.table(layout, K.H_OFF_LINK_F, int(layout.I[K.H_N_LINKS]), K.LF_STRIDE, True)[first]
    mass, com = float(LF[K.LF_MASS]), [float(x) for x in LF[K.LF_COM:K.LF_COM + 3]]
    assert mass == pytest.approx(1.3)
    worst = 0.0
    for step in range(25):
        sim.step(0)
        if step not in (4, 24):
            continue
        acc = call(sim, uid, [hinge], com, None, False).astype(np.float64)[:, 0]
        W = sim.joint_reaction_forces(uid, [hinge]).cpu().numpy().astype(np.float64)[:, 0]
        q = sim.link_states(uid, [hinge], com=True).cpu().numpy().astype(np.float64)[:, 0, 3:7]
        for e in range(B):
            want = jref.quat_mat(q[e]) @ W[e, 0:3]
            got = mass * (acc[e, 0:3] - [0, 0, -G])
            worst = max(worst, float(np.abs(got - want).max() / (1.0 + np.linalg.norm(want))))
            assert np.linalg.norm(acc[e, 0:3]) > 0.5   # it swings
    print('MEASURE reaction pendulum B=%d %.3e' % (B, worst))
    within('reaction', worst)


# ------------------------------------------------------------------------------------------------------- 4. every workspace mode
def every_call(env):
    from diy_gym_amd.scene import K
    out = []
    for m in env.models.values():
        if body_row(env.layout, m.uid)[K.BI_PREV_OFF] < 0:
            continue
        frames = ([-1] + list(range(len(m.flat.frames))))[:5]
        for com in (False, True):
            out.append(call(env.sim, m.uid, frames, MOUNT_POS[:len(frames)], MOUNT_ORN[:len(frames)], com))
    return out


@pytest.mark.parametrize('name,B,steps', sorted(MODES))
def test_every_workspace_mode_gives_the_same_bits(monkeypatch, name, B, steps):
    """One state, set into worlds of every mode the scene can run in (the table of tests/test_joint_wrench_gpu.py: the pressed arms
    at 70 envs; the pendulum at 3 envs with 64 / 32 / 16 envs per wavefront and the global workspace; the floating cart at 3 envs in
    every LDS mode down to one env per wavefront), gives bit-identical readings."""
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
    S = first.sim.get_state(); want = every_call(first)
    assert len(want) >= 2 and np.abs(want[0][:, :, 6:9]).max() > 1.0
    for sw, lanes in MODES[(name, B, steps)]:
        for v in switches:
            monkeypatch.delenv(v, raising=False)
        for k, v in sw.items():
            monkeypatch.setenv(k, v)
        env = make(name, B)
        assert env.sim.lanes == lanes, (sw, env.sim.lanes)
        env.sim.set_state(S)
        got = every_call(env)
        for i, (a, c) in enumerate(zip(want, got)):
            assert np.array_equal(bits(a), bits(c)), (sw, lanes, i)
        env.close()


# ------------------------------------------------------------------------------------------------------------------ 5. teleport
def test_teleport_shows_as_a_jump_and_the_old_state_reads_as_before():
    import torch
    B = 3
    env = make(SWING, B); sim = env.sim; arm = env.models['arm']; uid = arm.uid
    frames = [arm.get_frame_id('ee_fixed_joint'), arm.get_frame_id('elbow_joint'), -1]
    read = lambda: call(sim, uid, frames, MOUNT_POS[:3], MOUNT_ORN[:3], False)
    act = torch.tensor([[0.3, -0.55, 1.22, -1.51, 0.84, 0.1]] * B, device=env.device)
    for _ in range(5):
        sim.step(env._all_slots, act)
    S = sim.get_state(); before = read()
    assert np.array_equal(before[:, 2, :6], np.zeros((B, 6)))   # the fixed base never accelerates
    q, qd = (t.clone() for t in sim.joint_states(uid))
    sim.reset_joint_state(uid, q, qd + 0.5)
    jumped = read()
    assert np.abs(jumped[:, 1, 3:6] - before[:, 1, 3:6]).max() > 100.0   # 0.5 rad/s over one substep: 240 rad/s^2 per joint
    sim.step(env._all_slots, act)
    assert np.abs(read()[:, :, 3:6]).max() < 100.0   # the next step clears it
    sim.set_state(S)
    assert np.array_equal(bits(read()), bits(before))   # the old state reads the old bits


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_at_the_entry_and_from_env_sim():
    import torch
    from diy_gym_amd.backend import AccelSelector, _ptr
    env = make(ARMS, 3); sim = env.sim
    arm = env.models['ur5_l']; nfr = len(arm.flat.frames)
    for bad in (dict(frames=[nfr]), dict(frames=[-2]), dict(frames=[]), dict(frames=[0] * 17), dict(frames=[0], local_orn=[0., 0., 0., 0.])):
        with pytest.raises(ValueError):
            sim.link_accelerations(arm.uid, **bad)
    with pytest.raises(ValueError):
        sim.link_accelerations(99)
    out = torch.full((3, 17, 15), 7.0, device=env.device)

    def entry(s, body, arr, n):
        return s.lib.dg_world_link_accelerations(s.handle, _ptr(s.state), body, arr, n, _ptr(out), s._stream())
    arr = (AccelSelector * 17)()
    for a in arr:
        a.frame, a.quat[3] = 0, 1.0
    assert entry(sim, arm.uid, arr, 0) == -4 and entry(sim, arm.uid, arr, 17) == -4
    assert b'dg_world_link_accelerations' in sim.lib.dg_last_error()
    arr[0].frame = nfr
    assert entry(sim, arm.uid, arr, 1) == -4 and b'no frame' in sim.lib.dg_last_error()
    arr[0].frame = -2
    assert entry(sim, arm.uid, arr, 1) == -4
    arr[0].frame = 0; arr[0].quat[3] = 0.0
    assert entry(sim, arm.uid, arr, 1) == -4 and b'zero norm' in sim.lib.dg_last_error()
    arr[0].quat[3] = 1.0
    assert entry(sim, 7, arr, 1) == -4
    assert sim.lib.dg_world_link_accelerations(sim.handle, _ptr(sim.state), arm.uid, None, 1, _ptr(out), sim._stream()) == -4
    assert sim.lib.dg_world_link_accelerations(sim.handle, _ptr(sim.state), arm.uid, arr, 1, None, sim._stream()) == -4
    # a body without saved velocities: the message names the remedy
    bare = make('contacts_arms.yaml', 3)
    with pytest.raises(ValueError, match='enable_joint_force_torque'):
        bare.sim.link_accelerations(bare.models['ur5_l'].uid)
    assert entry(bare.sim, bare.models['ur5_l'].uid, arr, 1) == -4
    msg = bare.sim.lib.dg_last_error()
    assert b'enable_joint_force_torque' in msg and b'force_torque_sensor' in msg
    # a frozen body, an attached child's alias
    child = make('contacts_child_gripper.yaml', 3)
    with pytest.raises(ValueError, match='frozen'):
        child.sim.link_accelerations(child.models['plane'].uid)
    arr[0].frame = -1
    assert entry(child.sim, child.models['plane'].uid, arr, 1) == -4 and b'frozen' in child.sim.lib.dg_last_error()
    with pytest.raises(ValueError, match='attached'):
        child.sim.link_accelerations(child.models['arm'].models['gripper'].uid)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())   # outputs untouched by every refused call
    arr[0].frame = 0
    assert entry(sim, arm.uid, arr, 1) == 0   # ... and the same selectors are taken once they are right
    torch.cuda.synchronize()
    assert bool((out.flatten()[:3 * 15] != 7.0).any()) and bool((out.flatten()[3 * 15:] == 7.0).all())


def test_world_with_pairs_and_without_impulse_cache_is_taken():
    env, cached = make(ARMS, 3, engine={'warmstart': 0, 'warmstart_friction': 0}), make(ARMS, 3)
    assert env.layout.warm_off < 0 and env.layout.max_contacts > 0
    arm = env.models['ur5_l']
    got = call(env.sim, arm.uid, [arm.get_frame_id('ee_fixed_joint')], None, None, False)
    assert np.abs(got[:, 0, 6:9]).max() > 1.0
    press(cached, 10)
    S = cached.sim.get_state()   # there is no contact term: the same physical state reads the same bits with and without the cache
    T = env.sim.get_state(); T[:, :env.layout.physical_dim] = S[:, :cached.layout.physical_dim]; env.sim.set_state(T)
    a = call(env.sim, arm.uid, [arm.get_frame_id('ee_fixed_joint')], None, None, False)
    b = call(cached.sim, arm.uid, [arm.get_frame_id('ee_fixed_joint')], None, None, False)
    assert env.layout.physical_dim == cached.layout.physical_dim and np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------------------------------------------- 7. the addon
def test_imu_sensor_reports_the_call_and_leaves_the_state_alone():
    import torch
    B = 3
    env, plain = make_imu(DRONE, B), make_imu(DRONE, B)   # (the second one is stepped without ever evaluating its sensors)
    act = torch.tensor([[0.9, 0.9, 0.9, 0.9], [0.9, 0.5, 0.9, 0.5], [0.2, 0.9, 0.6, 1.0]], device=env.device)
    action = {'drone': {'motor%d' % (i + 1): act[:, i:i + 1] for i in range(4)}}
    for _ in range(12):
        obs = env.step(action)[0]
        plain.sim.step(plain._all_slots, act)
    drone = env.models['drone']
    before = env.sim.get_state()
    o = env.observe()['drone']['imu']
    assert np.array_equal(bits(before), bits(env.sim.get_state()))
    r = env.sim.link_accelerations(drone.uid, [-1])
    assert torch.equal(o['linear_acceleration'], r.specific_force[:, 0]) and torch.equal(o['angular_velocity'], r.ang_vel[:, 0])
    assert torch.equal(o['gravity'], r.gravity[:, 0]) and torch.equal(obs['drone']['imu']['linear_acceleration'], o['linear_acceleration'])
    assert float(o['linear_acceleration'].abs().max()) > 1.0 and float(o['angular_velocity'].abs().max()) > 1e-3
    assert np.array_equal(bits(env.sim.get_state()), bits(plain.sim.get_state()))
