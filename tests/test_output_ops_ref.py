"""Pins tests/output_ops_ref.py -- the fp64 restatement of the observe, reward and terminal ops -- and fixes the tolerance table
the kernels are held to in tests/test_output_ops_gpu.py.  No GPU.

  * the Euler formula and its inverse against scipy away from the gimbal branches, and the formula's own rebuilt-rotation error in
    them (what a gimbal env is allowed on top of the tolerance);
  * the quaternion of every link frame of the edge states against ``Rotation.from_matrix`` up to sign, every branch taken;
  * twists against central finite differences of the fp64 poses;
  * everything against the two CPU builds of the oracle on the edge states of tests/output_ops_cases.py and on the three seeded
    steps the GPU test takes from them: the fp64 build must agree far below fp32 spacing (bound 1e-12; measured 3.1e-15 on
    observations, 4.5e-16 on rewards), and ``TOL = 4 x max(fp64 build, fp32 build)`` per class: both must stay below TOL / 4 and the
    table must be 4 x the maximum measured here, rounded up to three digits;
  * the ladders: every branch count, zero envs within a margin of a threshold at the edge states, at most 5 % after each step;
  * the comparison itself rejects a pitch moved by 10 rotation tolerances, a flipped joint rate and a step counter off by one, and
    accepts q replaced by -q.
"""
import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import oracle_backend as ob
import output_ops_cases as C
import output_ops_ref as R
from diy_gym_amd.scene import K

B = 70
STEPPED = ('generic', 'generic_all', 'arms', 'arms_ik', 'one_arm', 'pair_ik')
_CACHE = {}


def world(scene, build='f64'):
    """(env on the oracle build, reference, edge states), built once per session."""
    if (scene, build) not in _CACHE:
        backend = ob.OracleBackend if build == 'f64' else ob.flavour(build)
        if backend is None:
            pytest.skip('oracle/%s is not built (make -C oracle builds every flavour)' % ob.FLAVOURS[build])
        env = C.make_env(scene, B, backend_factory=backend)
        ref = R.OutputRef(env)
        _CACHE[scene, build] = env, ref, C.edge_states(scene, env, ref, B, seed=0)
    return _CACHE[scene, build]


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
def test_euler_formula_against_scipy():
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(2000):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        if abs(R.sarg_of(q)) >= R.COMPONENTS:
            continue
        rot = Rotation.from_quat(q)
        worst = max(worst, np.abs(R.wrap(R.euler_pybullet(q) - rot.as_euler('xyz'))).max(), np.abs(R.euler_matrix(R.euler_pybullet(q)) - rot.as_matrix()).max(),
                    np.abs(R.quat_matrix(q) - rot.as_matrix()).max(), R.geodesic(R.euler_matrix(R.euler_pybullet(q)), rot.as_matrix()))
    print('Euler formula, matrices and the geodesic angle against scipy: %.3g' % worst)
    assert worst < 1e-12   # measured 1.8e-15


def test_gimbal_branches_are_approximate_by_what_the_reference_says():
    """Inside the branches the formula drops roll: rebuilt rotation off by up to 6.3e-3 rad at the threshold, exact at the pole."""
    rng = np.random.default_rng(1)
    at_threshold, at_pole = 0.0, 0.0
    for sign in (1.0, -1.0):
        for _ in range(200):
            for delta, which in ((np.sqrt(2e-5) * 0.999, 'threshold'), (0.0, 'pole')):
                q = C.quat_rpy(rng.uniform(-np.pi, np.pi), sign * (np.pi / 2 - delta), rng.uniform(-np.pi, np.pi)) * rng.choice([-1.0, 1.0])
                assert abs(R.sarg_of(q)) >= R.GIMBAL
                err = R.geodesic(R.euler_matrix(R.euler_pybullet(q)), R.quat_matrix(q))
                at_threshold, at_pole = (max(at_threshold, err), at_pole) if which == 'threshold' else (at_threshold, max(at_pole, err))
    print('gimbal formula, rebuilt rotation error: %.3g at the threshold, %.3g at the pole' % (at_threshold, at_pole))
    assert 4e-3 < at_threshold < 6.4e-3 and at_pole < 1e-12   # measured 6.32e-3 and 7.4e-16


@pytest.mark.parametrize('scene', ['generic', 'arms', 'joints'])
def test_link_quaternions_against_scipy(scene):
    env, ref, states = world(scene)
    worst, seen = 0.0, set()
    for row in states:
        for b in ref.bodies.values():
            b.at(row)
            for T in b.T.values():
                q, br = R.matrix_quat(T.R)
                s = Rotation.from_matrix(T.R).as_quat()
                worst = max(worst, min(np.abs(q - s).max(), np.abs(q + s).max()))
                seen.add(br)
    print('%s: link-frame quaternions against scipy up to sign %.3g, branches %s' % (scene, worst, sorted(seen)))
    assert worst < 1e-12 and seen == {0, 1, 2, 3}   # measured 1.2e-15


def _advance(ref, row, h):
    """The state ``h`` seconds along its own velocities (no dynamics): joints by qd, base origins by v, base rotations by w."""
    out = np.array(row, dtype=np.float64)
    for b in ref.bodies.values():
        for o in b.q_off:
            out[o + K.LS_Q] += h * row[o + K.LS_QD]
        if not b.fixed:
            so = ref.layout.body_state_off[b.body]
            out[so:so + 3] += h * row[so + K.BS_LINVEL:so + K.BS_LINVEL + 3]
            out[so + 3:so + 7] = (Rotation.from_rotvec(h * row[so + K.BS_ANGVEL:so + K.BS_ANGVEL + 3]) * Rotation.from_quat(row[so + 3:so + 7])).as_quat()
    return out


@pytest.mark.parametrize('scene', ['generic', 'arms'])
def test_twists_against_finite_differences(scene):
    env, ref, states = world(scene)
    h, worst = 1e-5, 0.0
    for row in states[::7].astype(np.float64):
        plus, minus = _advance(ref, row, h), _advance(ref, row, -h)
        for b in ref.bodies.values():
            for fr in range(-1, len(b.robot.joints)):
                for com in (False, True):
                    f0, fp, fm = b.at(row).frame(fr, com), b.at(plus).frame(fr, com), b.at(minus).frame(fr, com)
                    v = (fp.p - fm.p) / (2 * h)
                    W = (fp.R @ fm.R.T - fm.R @ fp.R.T) / (4 * h)   # skew(w) to second order
                    w = np.array([W[2, 1], W[0, 2], W[1, 0]])
                    worst = max(worst, np.abs(v - f0.v).max(), np.abs(w - f0.w).max())
    print('%s: frame twists against central differences of the poses %.3g' % (scene, worst))
    assert worst < 1e-7   # measured 3e-9 (h^2 truncation at rates of a few rad/s)


# ---- the two oracle builds: agreement in fp64, the tolerance table from fp32 ---------------------------------------------------------
def _tilt_figure(env, ref, res, build):
    """Error of the tilt angle computed in the build's own precision from the build's reported base quaternion, per margin."""
    worst = 0.0
    real = env.sim.real
    for k, cls in enumerate(res.term_class):
        if cls != 'tilt':
            continue
        a = [a for r, a in ref.addons if getattr(getattr(a, 'term_op', None), 'io_off', None) == k and type(a).__name__ == 'FellOver'][0]
        q = env.sim.frame_state64(a.uid, -1, True)[:, 3:7].astype(real)
        tilt = real(2.0) * np.arctan2(np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]).astype(real), np.abs(q[:, 3])).astype(real)
        worst = max(worst, float(np.abs(tilt.astype(np.float64) - res.term_value[:, k]).max()))
    return worst


_MEASURED = {}


def measure(scene, build):
    """Per step (the edge states, then three seeded steps where the scene has actions): the build's errors against the reference in
    the classes' own units, what exceeds a quarter of the table, and the envs within a margin of a threshold.  Once per session."""
    if (scene, build) not in _MEASURED:
        env, ref, states = world(scene, build)
        sim = env.sim
        sim.set_state(states.astype(sim.real))
        sim.observe()
        unit = {k: 1.0 for k in R.TOL}   # figures come out in the classes' own units
        quarter = {k: v / 4 for k, v in R.TOL.items()}
        gen = torch.Generator().manual_seed(7)
        out = []
        for step in range(4 if scene in STEPPED else 1):
            if step:
                sim.step(env._all_slots, C.seeded_actions(env, gen))
            res = ref.evaluate(np.asarray(sim.get_state(), dtype=np.float64))
            got = R.outputs_of(sim)
            raw = R.compare(res, got, tol=unit)
            raw.figures['tilt'] = _tilt_figure(env, ref, res, build)
            # (which envs may take either Euler branch is decided by the rotation tolerance itself: that class in its real window)
            raw.figures['rot'] = R.compare(res, got).figures.get('rot', 0.0) * R.TOL['rot']
            out.append(dict(figures=raw.figures, bad=R.compare(res, got, tol=quarter).bad, near=np.nonzero(R.compare(res, got).near)[0]))
        _MEASURED[scene, build] = out
    return _MEASURED[scene, build]


@pytest.mark.parametrize('build', ['f64', 'f32'])
@pytest.mark.parametrize('scene', list(C.SCENES))
def test_against_the_oracle_builds(scene, build):
    steps = measure(scene, build)
    for step, m in enumerate(steps):
        assert not m['bad'], (scene, build, step, m['bad'])
        assert m['figures']['tilt'] <= R.TOL['tilt'] / 4, (scene, build, step, m['figures']['tilt'])
        if build == 'f64':
            assert max(v for k, v in m['figures'].items() if k not in ('rew_sum', 'elec')) < 1e-12, (scene, step, m['figures'])
            # the ladders: nothing within a margin of a threshold at the edge states, at most 5 % of the envs after a step
            assert len(m['near']) <= (0 if step == 0 else 0.05 * B), (scene, step, m['near'])
    print('%s %s: %s' % (scene, build, ' '.join('%s %.4g' % (k, max(m['figures'].get(k, 0.0) for m in steps)) for k in sorted(R.TOL))))


def test_the_table_is_four_times_the_measured_maximum():
    """Every entry of ``output_ops_ref.MEASURED`` is the largest figure of its class over the scenes, steps and the two builds as
    this checkout measures them, rounded UP to three significant digits (so: measured <= entry < 1.011 x measured), and
    ``TOL`` is 4 x that.  A scene or ladder edit that moves a figure makes this test name the new one."""
    worst = {k: (0.0, None) for k in R.TOL}
    for scene in C.SCENES:
        for build in ('f64', 'f32'):
            for m in measure(scene, build):
                for k in R.TOL:
                    if m['figures'].get(k, 0.0) > worst[k][0]:
                        worst[k] = (m['figures'][k], (scene, build))
    print('measured maxima: %s' % ' '.join('%s %.4g %s' % (k, v, w) for k, (v, w) in worst.items()))
    assert R.TOL == {k: 4 * v for k, v in R.MEASURED.items()}
    off = {k: (v, R.MEASURED[k]) for k, (v, w) in worst.items() if not v <= R.MEASURED[k] < 1.011 * v}
    assert not off, off


# ---- the ladders -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scene,frame', [('generic', ('cart', 'hinge_b')), ('arms', ('ur5_l', 'wrist_2_joint')), ('arms_ik', ('ur5_l', 'wrist_2_joint'))])
def test_every_branch_of_the_matrix_conversion_has_its_envs(scene, frame):
    env, ref, states = world(scene)
    res = ref.evaluate(states)
    count = np.bincount(res.branches[frame[0], env.models[frame[0]].get_frame_id(frame[1])], minlength=4)
    print(scene, frame, dict(zip(R.BRANCHES, count.tolist())))
    assert (count >= 8).all(), count


@pytest.mark.parametrize('scene', list(C.SCENES))
def test_ladders_stand_ten_margins_from_their_thresholds(scene):
    env, ref, states = world(scene)
    res = ref.evaluate(states)
    for k, cls in enumerate(res.term_class):
        if cls == 'timer':
            assert set(res.term_value[:, k]) == {env._max_episode_steps - 1, env._max_episode_steps, env._max_episode_steps + 1}
            continue
        assert R.TOL[cls] <= C.LADDER_MARGIN[cls] <= 1.5 * R.TOL[cls], (cls, R.TOL[cls], C.LADDER_MARGIN[cls])
        margins = res.term_margin[:, k] / R.margin_unit(res, k)   # in tolerances: what decides whether a byte is compared
        built = res.term_margin[:, k] / C.LADDER_MARGIN[cls]       # in the margins the ladder was built with
        rungs = sorted(set(np.round(built[built < 150]).astype(int)))
        print(scene, 'terminal column', k, cls, 'rungs (margins)', rungs, 'fired', int(res.term[:, k].sum()))
        assert margins.min() > 9.0 and {10, 100} <= set(rungs), (k, cls, margins.min(), rungs)   # (10 less the rounding of the state to fp32)
        assert 0 < res.term[:, k].sum() < B
    gimbal = [int((np.abs(rot['sarg']) >= R.GIMBAL).sum()) for rot in res.rots]
    if scene not in ('joints', 'pair_ik'):
        assert max(gimbal) >= 10, gimbal   # five rungs of the ladder, both signs
        both = [rot for rot in res.rots if (np.abs(rot['sarg']) >= R.GIMBAL).sum() >= 10][0]
        assert (both['sarg'] >= R.GIMBAL).any() and (both['sarg'] <= -R.GIMBAL).any()
    if scene == 'generic':   # the base ladder (cart pose), the link ladder (tip) and the marble
        assert sum(g >= 10 for g in gimbal) >= 3, gimbal


def test_all_but_one_group_fires():
    """terminal_if_all with three groups (cart, marble, the environment): envs where exactly one group holds the flag back, for
    each of the three, and envs where all fire."""
    env, ref, states = world('generic_all')
    res = ref.evaluate(states)
    groups = sorted(set(res.term_group), key=res.term_group.index)
    assert len(groups) == 3
    fired = np.stack([res.term[:, [k for k, g in enumerate(res.term_group) if g == grp]].any(axis=1) for grp in groups], axis=1)
    for g in range(3):
        alone = ~fired[:, g] & fired[:, [k for k in range(3) if k != g]].all(axis=1)
        assert alone.sum() >= 2 and not res.term_flag[alone].any(), (g, alone.sum())
    assert fired.all(axis=1).sum() >= 2 and (res.term_flag == fired.all(axis=1)).all()
    assert (ref.evaluate(states).term_flag != world('generic')[1].evaluate(states).term_flag).any()


# ---- the comparison can fail -----------------------------------------------------------------------------------------------------
def test_the_comparison_rejects_what_it_should():
    env, ref, states = world('generic')
    e = 66   # a random pose away from every ladder
    row = states[e:e + 1].astype(np.float64)
    row[0, K.ST_STEP] = env._max_episode_steps - 1
    res = ref.evaluate(row)
    assert R.compare(res, ref.evaluate(row)).ok
    so = env.layout.body_state_off[env.models['cart'].uid]
    cart = ref.bodies['cart']

    pitched = row.copy()
    q = row[0, so + 3:so + 7]
    pitched[0, so + 3:so + 7] = (Rotation.from_euler('y', 10 * R.TOL['rot']) * Rotation.from_quat(q)).as_quat()
    rep = R.compare(res, ref.evaluate(pitched))
    assert not rep.ok and any(b.startswith('rot') for b in rep.bad), rep.bad

    flipped = row.copy()
    flipped[0, cart.q_off[1] + K.LS_QD] *= -1.0
    rep = R.compare(res, ref.evaluate(flipped))
    assert not rep.ok and any(b.startswith('exact') for b in rep.bad) and any(b.startswith('lin') for b in rep.bad), rep.bad

    later = row.copy()
    later[0, K.ST_STEP] += 1.0
    rep = R.compare(res, ref.evaluate(later))
    assert rep.bad and all(b.startswith('term') for b in rep.bad), rep.bad   # the timer's byte (and the flag where nothing else fired), nothing else

    negated = row.copy()
    negated[0, so + 3:so + 7] *= -1.0
    rep = R.compare(res, ref.evaluate(negated))
    assert rep.ok and max(rep.figures.values()) < 1e-6, (rep.bad, rep.figures)
