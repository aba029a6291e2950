"""Pins tests/input_ops_ref.py -- the fp64 restatement of the update ops, the reset ops and the external wrench entry -- and fixes the
tolerance table the kernels are held to in tests/test_input_ops_gpu.py.  No GPU.

  * joint torques of a wrench against J^T [F; T] with J from central finite differences of the ``nphelpers`` kinematics; the base
    wrench against finite differences of the base pose (virtual work); gravity compensation against ``dynamics_ref``'s inverse
    dynamics at zero rate, with mass scales;
  * the counter RNG against arbitrary-precision integers, its first two moments over 10^6 draws, its range, and the independence
    of the streams across env, episode, op and component;
  * respawn poses inside their ranges; both limits of the mass scale reached within three episodes; every texture kind drawn;
  * everything against the two CPU builds of the oracle (``dgo_update`` after ``set_state``; the wrench entry with the calls of
    the GPU test -- the update ops of these scenes never put a wrench on a LINK 50 m from the origin, the entry does; three
    successive resets with hot_start 0): the fp64 build must agree to 1e-12, ``TOL = 4 x max(fp64 build, fp32 build)`` per class: both must stay below
    TOL / 4 and the table must be 4 x the maximum measured here, rounded up to three digits;
  * the episode counter beyond 2^24;
  * the comparison itself rejects a doubled torque, a dropped wrench, a jitter without its ``- 1/2`` and a target off by one ulp.
"""
import numpy as np
import pytest

import dynamics_ref as D
import input_ops_cases as C
import input_ops_ref as R
import oracle_backend as ob
import output_ops_ref as O
import base_state_ref as bs
from diy_gym_amd.mathx import Transform
from diy_gym_amd.scene import K

B = 70
SEED = 5
_CACHE, _MEASURED = {}, {}


def world(scene, build='f64', hot_start=0):
    """(env on the oracle build, reference, edge states, actions), built once per session."""
    key = scene, build, hot_start
    if key not in _CACHE:
        backend = ob.OracleBackend if build == 'f64' else ob.flavour(build)
        if backend is None:
            pytest.skip('oracle/%s is not built (make -C oracle builds every flavour)' % ob.FLAVOURS[build])
        env = C.make_env(scene, B, hot_start=hot_start, backend_factory=backend, seed=SEED)
        ref = R.InputRef(env)
        _CACHE[key] = env, ref, C.edge_states(scene, env, ref, B, seed=0), C.actions(env, B)
    return _CACHE[key]


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
def _point_and_rotation(b, row, link, local):
    b.at(row)
    return b.T[link].R @ local + b.T[link].p, b.T[link].R.copy()


@pytest.mark.parametrize('scene,name', [('generic', 'cart'), ('arms', 'ur5_l')])
def test_joint_torques_of_a_wrench_are_jacobian_transpose(scene, name):
    env, ref, states, _ = world(scene)
    rng = np.random.default_rng(3)
    b = ref.bodies[name]
    h, worst, seen = 1e-6, 0.0, set()
    for row in states[::9].astype(np.float64):
        for fr, j in enumerate(b.robot.joints):
            b.at(row)
            F, T, P = rng.normal(size=3), rng.normal(size=3), b.T[j.child].p + rng.normal(size=3) * 0.3
            got = ref.jt_wrench(b, fr, P, F, T)
            local = b.T[j.child].R.T @ (P - b.T[j.child].p)
            want = {}
            for q in range(b.robot.num_dofs):
                plus, minus = row.copy(), row.copy()
                plus[b.q_off[q] + K.LS_Q] += h
                minus[b.q_off[q] + K.LS_Q] -= h
                (pp, Rp), (pm, Rm) = _point_and_rotation(b, plus, j.child, local), _point_and_rotation(b, minus, j.child, local)
                W = (Rp @ Rm.T - Rm @ Rp.T) / (4 * h)
                tau = ((pp - pm) / (2 * h)) @ F + np.array([W[2, 1], W[0, 2], W[1, 0]]) @ T
                if abs(tau) > 1e-9 or q in got:
                    want[q] = tau
            assert set(got) == {q for q in want if q in got} and all(abs(v) < 1e-7 for q, v in want.items() if q not in got), (fr, got, want)
            worst = max([worst] + [abs(got[q] - want[q]) for q in got])
            seen |= {b.by_q[q].type for q in got}
    print('%s: J^T wrench against finite differences %.3g, joint types %s' % (scene, worst, sorted(seen)))
    assert worst < 1e-7   # measured 2e-9 (h^2 truncation)
    assert seen == ({'prismatic', 'revolute'} if scene == 'generic' else {'revolute'})


def test_base_wrench_is_force_and_moment_about_the_base_origin():
    """Virtual work: moving the base link frame by dp and turning it by dtheta about its own origin moves a point of the body by
    ``dP``; ``ext . [dp, dtheta] = F . dP + T . dtheta``.  In WORLD and in LINK frame, on the base, a bolted frame and a link."""
    env, ref, states, _ = world('generic')
    rng = np.random.default_rng(4)
    b, so = ref.bodies['cart'], env.layout.body_state_off[env.models['cart'].uid]
    from scipy.spatial.transform import Rotation
    h, worst = 1e-6, 0.0
    for row in states[[3, 20, 41, 43, 66]].astype(np.float64):
        for fr in (-1, env.models['cart'].get_frame_id('mast'), env.models['cart'].get_frame_id('tip_joint')):
            for link_frame in (False, True):
                f, t, pos = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3) * 0.2
                b.at(row)
                if not link_frame:
                    pos = pos + b.p_l
                ext, _ = ref._wrench(b, fr, link_frame, f, pos, t)
                fs = b.frame(fr, True)
                F, T, P = (fs.R @ f, fs.R @ t, fs.p + fs.R @ pos) if link_frame else (f, t, pos)
                base = Transform(O.quat_matrix(b.q_l), b.p_l)
                local = base.R.T @ (P - base.p)
                for k in range(6):
                    d = []
                    for s in (h, -h):
                        p2, R2 = base.p.copy(), base.R
                        if k < 3:
                            p2[k] += s
                        else:
                            R2 = Rotation.from_rotvec(np.eye(3)[k - 3] * s).as_matrix() @ base.R
                        d.append(R2 @ local + p2)
                    work = F @ ((d[0] - d[1]) / (2 * h)) + (T[k - 3] if k >= 3 else 0.0)
                    worst = max(worst, abs(work - ext[k]) / max(1.0, abs(ext[k])))
    print('base wrench against virtual work %.3g' % worst)
    assert worst < 1e-7   # measured 1e-9


def test_gravity_compensation_is_inverse_dynamics_at_zero_rate():
    env, ref, states, _ = world('arms')
    b, a = ref.bodies['ur5_l'], env.models['ur5_l'].addons['controller']
    worst, scales = 0.0, []
    for row in states.astype(np.float64):
        b.at(row)
        s = ref.scales('ur5_l', row)
        scales.append(s)
        want = D.inverse_dynamics(b.robot, b.q, np.zeros(6), np.zeros(6), g=ref.g, T_base=Transform(O.quat_matrix(b.q_l), b.p_l), scale=s)
        got = ref.gravity_compensation(b, s)
        worst = max(worst, np.abs(got - want).max())
        zero = ref.admittance(b, row, a, np.zeros(6))   # no wrench: gravity compensation and the joint PD
        pd = a.kp * (np.asarray(a.target_pose) - b.q) - a.kd * b.qd
        worst = max(worst, np.abs(zero - want - pd).max())
    print('gravity compensation against inverse dynamics %.3g; mass scales %.3g .. %.3g' % (worst, np.min(scales), np.max(scales)))
    assert worst < 1e-11 and np.min(scales) == pytest.approx(0.4) and np.max(scales) == pytest.approx(2.5)


_M64 = (1 << 64) - 1


def _mix_int(z):
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & _M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & _M64
    return z ^ (z >> 31)


def _rng_int(seed, env, episode, op, comp):
    z = _mix_int((seed + 0x9E3779B97F4A7C15 * (env + 1)) & _M64)
    z = _mix_int(z ^ ((episode * 0xD1342543DE82EF95 + op * 0x2545F4914F6CDD1D + comp + 1) & _M64))
    return (z >> 40) / 16777216.0


def test_rng_uniform():
    rng = np.random.default_rng(0)
    for _ in range(2000):   # the uint64 arithmetic against Python's integers, large arguments included
        args = [int(rng.integers(0, 2 ** 62)), int(rng.integers(0, 2 ** 31)), int(rng.integers(0, 2 ** 25)), int(rng.integers(0, 64)), int(rng.integers(0, 16))]
        assert R.rng_uniform(*args) == _rng_int(*args), args
    n = 10 ** 6
    u = R.rng_uniform(SEED, np.arange(n), 1, 3, 0)
    print('10^6 draws: mean %.6f variance %.6f max %.8f' % (u.mean(), u.var(), u.max()))
    assert abs(u.mean() - 0.5) < 4 * np.sqrt(1 / 12 / n) and abs(u.var() - 1 / 12) < 4 * np.sqrt((1 / 80 - 1 / 144) / n)   # four standard errors
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24)) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    m = 10 ** 5
    base = R.rng_uniform(SEED, np.arange(m), 1, 3, 0)
    for name, other in (('seed', R.rng_uniform(SEED + 1, np.arange(m), 1, 3, 0)), ('env', R.rng_uniform(SEED, np.arange(m) + 1, 1, 3, 0)), ('episode', R.rng_uniform(SEED, np.arange(m), 2, 3, 0)),
                        ('op', R.rng_uniform(SEED, np.arange(m), 1, 4, 0)), ('component', R.rng_uniform(SEED, np.arange(m), 1, 3, 1))):
        corr = np.corrcoef(base, other)[0, 1]
        assert abs(corr) < 5 / np.sqrt(m) and (base == other).mean() < 1e-3, (name, corr)


def _three_resets(scene):
    """The reference alone over three successive resets of the edge states: [(cells, state rows after)]."""
    env, ref, states, _ = world(scene)
    rows, out = states.astype(np.float64), []
    for _ in range(3):
        cells = ref.reset(rows, np.arange(B), SEED)
        draws = list(ref.draws)
        rows = rows.copy()
        for c, (cls, val, ex) in cells.col.items():
            rows[:, c] = val.astype(np.float32)
        for c, q in cells.quats.items():
            rows[:, c:c + 4] = q.astype(np.float32)
        out.append((cells, rows, draws))
    return env, ref, out


def test_respawn_poses_stay_inside_their_ranges():
    env, ref, eps = _three_resets('generic')
    for name in ('cart', 'marble'):
        a, m = env.models[name].addons['respawn'], env.models[name]
        so = env.layout.body_state_off[m.uid]
        seen = []
        for cells, rows, _ in eps:
            p, q, _, _ = bs.report_from_stored(env.layout, m.uid, rows[:, so:so + 3], rows[:, so + 3:so + 7])
            d = p - np.asarray(a.initial_pose[0])
            assert (np.abs(d) <= np.asarray(a.position_range) / 2 + 1e-6).all(), name
            rel = bs.qmul(bs.qconj(a.initial_pose[1]), q)
            ang = np.array([O.euler_plain(r) for r in rel])
            assert (np.abs(ang) <= np.asarray(a.rotation_range) / 2 + 1e-6).all(), name
            seen.append(np.concatenate([d / np.asarray(a.position_range), ang / np.asarray(a.rotation_range)], axis=1))
        seen = np.stack(seen)
        print(name, 'jitter / range: min %.3f max %.3f mean %.3f' % (seen.min(), seen.max(), seen.mean()))
        assert seen.min() < -0.45 and seen.max() > 0.45 and abs(seen.mean()) < 0.05   # centred: u - 1/2, not u
        if a.once:   # one draw for all episodes
            assert np.array_equal(seen[0], seen[1]) and np.array_equal(seen[1], seen[2])
        else:        # (the envs whose counter stands at 2^24 repeat theirs: test_the_episode_counter_stops_at_2_24)
            moving = np.asarray(C.EPISODES)[np.arange(B) % len(C.EPISODES)] < 2 ** 24 - 1
            assert (np.abs(seen[0] - seen[1])[moving].max(axis=1) > 0).all()


def test_randomizer_draws_reach_their_edges():
    for scene in ('generic', 'generic_vel'):
        env, ref, eps = _three_resets(scene)
        a = env.models['cart'].addons['dynamics']
        so, n = env.layout.addon_off + a.op.state_off, len(a.joint_ids)
        scales = np.stack([rows[:, so:so + n] for _, rows, _ in eps])
        damp = np.stack([rows[:, so + n] for _, rows, _ in eps])
        lo, hi = a.mass_scale_limits
        logs = np.log([a.mass_range[0] + (a.mass_range[1] - a.mass_range[0]) * u for kind, comp, u in eps[0][2] if kind == 'DynamicsRandomizer' and comp % 2 == 0])
        print(scene, 'scales at the lower limit %d, at the upper %d, between %d; log U < 0: %d of %d; damping zero %d, positive %d' % (
            (scales == np.float32(lo)).sum(), (scales == np.float32(hi)).sum(), ((scales > lo) & (scales < hi)).sum(), (logs < 0).sum(), logs.size, (damp == 0).sum(), (damp > 0).sum()))
        assert (scales == np.float32(lo)).sum() >= 10 and (scales == np.float32(hi)).sum() >= 10 and ((scales > lo) & (scales < hi)).sum() >= 10
        assert (logs < 0).sum() >= 10 and (scene == 'generic' or (logs > 0).sum() >= 10)
        assert (damp == 0).sum() >= 10 and (damp > 0).sum() >= 10   # log U < 0 below 1: clamped at zero
        # the damping that stays is the LAST joint's draw of the last round: with another joint's URDF damping it would differ
        last = np.array([u for kind, comp, u in eps[2][2] if kind == 'DynamicsRandomizer' and comp == 2 * (n - 1) + 1])
        want = np.maximum(np.log(a.damping_range[0] + (a.damping_range[1] - a.damping_range[0]) * last) * env.models['cart'].robot.joints[a.joint_ids[-1]].damping, 0.0)
        assert np.allclose(damp[2], want, rtol=1e-6, atol=0)
    tex = env.models['cart'].addons['look']
    so = env.layout.addon_off + tex.op.state_off
    kinds = np.concatenate([rows[:, so + K.TX_KIND] for _, rows, _ in eps])
    freq = np.concatenate([rows[:, so + K.TX_FREQ] for _, rows, _ in eps])
    assert set(kinds) == {1.0, 2.0, 3.0} and freq.min() >= 2.0 and freq.max() <= 16.0, (set(kinds), freq.min(), freq.max())


# ---- the two oracle builds: agreement in fp64, the tolerance table from fp32 ---------------------------------------------------------
def _merge(figs, rep, what, bad):
    for k, v in rep.figures.items():
        figs[k] = max(figs.get(k, 0.0), v)
    bad += [(what, b) for b in rep.bad if b.split()[0] not in R.TOL]


def measure(scene, build):
    """Raw errors of the build per class (update ops: all slots, a partial mask, no actions; three resets), what is not exact where
    it must be, and what exceeds a quarter of the table.  Once per session."""
    if (scene, build) not in _MEASURED:
        env, ref, states, act = world(scene, build)
        sim = env.sim
        unit = {k: 1.0 for k in R.TOL}
        quarter = {k: v / 4 for k, v in R.TOL.items()}
        figs, bad, over = {}, [], []
        half = sum(1 << a.op.slot for a in ref.update_addons[::2])
        for what, mask, actions in (('all', env._all_slots, act), ('half', half, act), ('none', env._all_slots, None)):
            sim.set_state(states.astype(sim.real))
            pre = np.asarray(sim.get_state(), dtype=np.float64)
            cells = ref.update(pre, None if actions is None else actions.numpy(), mask, real=np.float32 if sim.real is np.float32 else np.float64)
            sim.update(mask, actions)
            got = np.asarray(sim.get_state(), dtype=np.float64)
            _merge(figs, R.compare(cells, got, tol=unit), what, bad)
            over += R.compare(cells, got, tol=quarter).bad
            others = np.setdiff1d(np.arange(got.shape[1]), cells.columns())
            assert np.array_equal(got[:, others], pre[:, others]), (scene, build, what, 'an update op wrote a cell the reference does not name')
        if scene in ('generic', 'arms'):   # the wrench entry (dgo_apply_wrench) with the calls of the GPU test, accumulating
            sim.set_state(states.astype(sim.real))
            rng = np.random.default_rng(11)
            for name, frame_name in C.wrench_targets(scene):
                m = env.models[name]
                fr = -1 if frame_name is None else m.get_frame_id(frame_name)
                for flags in (sim.WORLD_FRAME, sim.LINK_FRAME):
                    link = flags == sim.LINK_FRAME
                    pre = np.asarray(sim.get_state(), dtype=np.float64)
                    f, p, t, one = C.wrench_rows(ref, pre, name, rng, not link)
                    for call, kw in ((lambda: sim.apply_external_force(m.uid, fr, f, p, flags), dict(f=f, pos=p)), (lambda: sim.apply_external_wrench(m.uid, fr, one, p[0], -one, flags), dict(f=one, pos=p[0], t=-one)),
                                     (lambda: sim.apply_external_torque(m.uid, fr, t, flags), dict(t=t))):
                        cells = ref.wrench(pre, name, fr, link, **kw)
                        call()
                        got = np.asarray(sim.get_state(), dtype=np.float64)
                        _merge(figs, R.compare(cells, got, tol=unit), 'wrench %s %s' % (name, frame_name), bad)
                        over += R.compare(cells, got, tol=quarter).bad
                        others = np.setdiff1d(np.arange(got.shape[1]), cells.columns())
                        assert np.array_equal(got[:, others], pre[:, others]), (scene, build, name, frame_name, 'a wrench call wrote a cell the reference does not name')
                        pre = got
        sim.set_state(states.astype(sim.real))
        for ep in range(3):
            pre = np.asarray(sim.get_state(), dtype=np.float64)
            cells = ref.reset(pre, np.arange(B), SEED)
            sim.reset()
            got = np.asarray(sim.get_state(), dtype=np.float64)
            _merge(figs, R.compare(cells, got, tol=unit), 'reset %d' % ep, bad)
            over += R.compare(cells, got, tol=quarter).bad
            others = np.setdiff1d(np.arange(got.shape[1]), cells.columns())
            assert np.array_equal(got[:, others], pre[:, others]), (scene, build, ep, 'a reset op wrote a cell the reference does not name')
        _MEASURED[scene, build] = figs, bad, over
    return _MEASURED[scene, build]


@pytest.mark.parametrize('build', ['f64', 'f32'])
@pytest.mark.parametrize('scene', list(C.SCENES))
def test_against_the_oracle_builds(scene, build):
    figs, bad, over = measure(scene, build)
    print('%s %s: %s' % (scene, build, ' '.join('%s %.4g' % (k, figs.get(k, 0.0)) for k in sorted(R.TOL))))
    assert not bad, (scene, build, bad)      # targets, torque-mode torques, reset joints, texture, counters, rotor speeds: exact
    assert not over, (scene, build, over)    # below a quarter of the table
    if build == 'f64':
        assert max(figs.get(k, 0.0) for k in R.TOL) < 1e-12, (scene, figs)


def test_the_table_is_four_times_the_measured_maximum():
    """Every entry of ``input_ops_ref.MEASURED`` is the largest figure of its class over the scenes and the two builds as this
    checkout measures them, rounded UP to three significant digits (measured <= entry < 1.011 x measured); ``TOL`` is 4 x that."""
    worst = {k: (0.0, None) for k in R.TOL}
    for scene in C.SCENES:
        for build in ('f64', 'f32'):
            figs = measure(scene, build)[0]
            for k in R.TOL:
                if figs.get(k, 0.0) > worst[k][0]:
                    worst[k] = (figs[k], (scene, build))
    print('measured maxima: %s' % ' '.join('%s %.6g %s' % (k, v, w) for k, (v, w) in worst.items()))
    assert R.TOL == {k: 4 * v for k, v in R.MEASURED.items()}
    off = {k: (v, R.MEASURED[k]) for k, (v, w) in worst.items() if not v <= R.MEASURED[k] < 1.011 * v}
    assert not off, off


def test_the_episode_counter_stops_at_2_24():
    """The counter is a float32 cell: 2^24 - 1 steps to 2^24, and 2^24 + 1 rounds back to 2^24, so from there every reset repeats
    the draws of episode 2^24 + 1.  Both builds of the oracle keep the cell in their own type; the fp32 build does what the kernels
    do, the fp64 build goes on counting -- the reference follows the float32 cell."""
    env, ref, states, _ = world('generic', 'f32')
    sim = env.sim
    sim.set_state(states.astype(sim.real))
    ladder = np.asarray(C.EPISODES)[np.arange(B) % len(C.EPISODES)]
    seen = []
    for _ in range(3):
        sim.reset()
        seen.append(np.asarray(sim.get_state(), dtype=np.float64))
    top, below = ladder == 2 ** 24, ladder == 2 ** 24 - 1
    assert (seen[0][top, K.ST_EPISODE] == 2 ** 24).all() and (seen[2][top, K.ST_EPISODE] == 2 ** 24).all()
    assert (seen[0][below, K.ST_EPISODE] == 2 ** 24).all() and (seen[2][below, K.ST_EPISODE] == 2 ** 24).all()
    so = env.layout.body_state_off[env.models['cart'].uid]
    assert np.array_equal(seen[0][top, so:so + 7], seen[1][top, so:so + 7]) and np.array_equal(seen[1][top, so:so + 7], seen[2][top, so:so + 7])   # the same jitter again
    assert np.array_equal(seen[1][below, so:so + 7], seen[2][below, so:so + 7]) and not np.array_equal(seen[0][below, so:so + 7], seen[1][below, so:so + 7])
    low = ladder < 1000
    assert (seen[2][low, K.ST_EPISODE] == ladder[low] + 3).all() and not np.array_equal(seen[1][low, so:so + 7], seen[2][low, so:so + 7])


# ---- the comparison can fail -----------------------------------------------------------------------------------------------------
def test_the_comparison_rejects_what_it_should():
    env, ref, states, act = world('arms')
    rows = states.astype(np.float64)
    cells = ref.update(rows, act.numpy())
    good = rows.copy()
    for c, (cls, val, ex) in cells.col.items():
        good[:, c] = val
    assert R.compare(cells, good).ok
    adm = ref.joint_col('ur5_l', 2, K.LS_TORQUE)
    doubled = good.copy()
    doubled[:, adm] += good[:, adm] - rows[:, adm]            # the admittance op run twice
    rep = R.compare(cells, doubled)
    assert any(b.startswith('torque') for b in rep.bad), rep.bad
    dropped = good.copy()
    eo = ref.ext_col('marble')
    dropped[:, eo:eo + 6] = rows[:, eo:eo + 6]                # the external force never applied
    rep = R.compare(cells, dropped)
    assert any(b.startswith('force') for b in rep.bad) and any(b.startswith('moment') for b in rep.bad), rep.bad
    ulp = good.copy()
    tq = ref.joint_col('ur5_r', 0, K.LS_TORQUE)
    ulp[:, tq] = np.nextafter(good[:, tq].astype(np.float32), np.float32(np.inf))   # a torque-mode torque off by one float32 ulp
    rep = R.compare(cells, ulp)
    assert any(b.startswith('exact') for b in rep.bad), rep.bad

    env, ref, states, _ = world('generic')
    rows = states.astype(np.float64)
    cells = ref.reset(rows, np.arange(B), SEED)
    a, so = env.models['cart'].addons['respawn'], env.layout.body_state_off[env.models['cart'].uid]
    shifted = rows.copy()
    for c, (cls, val, ex) in cells.col.items():
        shifted[:, c] = val
    for c, q in cells.quats.items():
        shifted[:, c:c + 4] = q
    assert R.compare(cells, shifted).ok
    shifted[:, so:so + 3] += 0.5 * np.asarray(a.position_range)   # u in place of u - 1/2
    rep = R.compare(cells, shifted)
    assert any(b.startswith('rpos') for b in rep.bad), rep.bad
    other = ref.reset(rows, np.arange(B) + 1, SEED)               # the neighbour's stream
    rep = R.compare(other, shifted)
    assert any(b.startswith('rrot') for b in rep.bad) and any(b.startswith('exact') for b in rep.bad), rep.bad
