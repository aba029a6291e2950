"""Every cull of the narrow phase is a lower bound: no stage that discards a candidate pair before an exact routine runs may
discard a pair that routine would report.

The stages (collide<LANES, TBL, SLC> in diy_gym_amd/csrc/dg_solver.h, DESIGN.md 3 "Broad phase"):
  1. build-time pruning of pairs between bolted-down bodies (scene.py, statically_apart);
  2. the group broad phase -- for a frozen partner the GD descriptors of dg_plan.hip, else BF_BOUND and the shape parameters;
  3. the per-pair bounding spheres (SC_BOUND);
  4. for hull pairs the capsules that contain the hulls (DG_SF_HULL_HALF);
  5. the early exit of GJK (covered by tests/test_hull_contacts.py).

The CPU tests restate each device bound in numpy FROM THE TABLES THE DEVICE READS (the scene blob, and the plan table of
backend.debug_plan for GD) and compare it with exact geometry.  The GPU tests put whole wavefronts into the thin band where a
cull decides -- the device culls are __any() over the wavefront, so one lane outside the band keeps a pair alive for all 64 and
hides a bound that is no bound -- and compare the device's contact list with the fp64 checker's.

Before the fixes that came with this file the following failed (CPU: run on the parent commit with these restatements of its
expressions; GPU: see each test's docstring):
  (a) test_the_sphere_of_a_hull_holds_its_points[0.0]: SC_BOUND = r + half of the fitted capsule when hull_contacts = 0 --
      np_cube 31.8 mm short, np_slab 20.2 mm, the UR5 shoulder 14 mm;
  (b) test_group_reach_covers_partner_and_report_distance[np_gem_wedge*]: the extent of a static hull in the group reach was
      the same r + half (np_wedge: 28 mm short), frozen (GD[3]) and not frozen;
  (c) the same test on every scene with a hull-hull pair (2 x hull_margin missing from the reach), and
      test_pruned_pairs_never_come_within_reporting_distance[np_two_arms] (threshold contact_margin + 1 mm)."""
import copy
import functools
import glob
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import oracle_backend
from test_hull_contacts import hull_lib, oracle_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DATA = os.path.join(ROOT, 'diy_gym_amd', 'data')
SPHERE, BOX, CAPSULE, POINTS = 0, 1, 2, 3
EPS = 1e-9   # scene.py's own epsilon on DG_SF_HULL_HALF; the tables are fp64, the bounds are compared in fp64
F32 = 2.0 ** -22   # relative slack where the device's fp32 copy of a table value is compared with fp64 geometry

SCENES = {
    'ur_high_5': 'examples/ur_high_5/ur_high_5.yaml', 'ur_arms_touching': 'tests/golden/ur_arms_touching.yaml',
    'from_the_readme': 'examples/from_the_readme/from_the_readme.yaml', 'r2d2_maze': 'examples/r2d2_maze/r2d2_maze.yaml',
    'basic_env': 'tests/golden/basic_env_nocam.yaml', 'box_stack': 'tests/golden/box_stack.yaml',
    'ur5_child_gripper': 'tests/golden/ur5_child_gripper.yaml', 'cart_tree': 'tests/golden/cart_tree.yaml',
    'np_cube_ground': 'tests/golden/np_cube_ground.yaml', 'np_slab_ground': 'tests/golden/np_slab_ground.yaml',
    'np_gem_wedge': 'tests/golden/np_gem_wedge.yaml', 'np_gem_wedge_respawned': 'tests/golden/np_gem_wedge_respawned.yaml',
    'np_gems': 'tests/golden/np_gems.yaml', 'np_two_arms': 'tests/golden/np_two_arms.yaml',
}


def make(cfg, num_envs=1, device=None, flavour=None, **engine):
    import diy_gym_amd.examples  # noqa: F401  registers the example addons
    from diy_gym_amd import DIYGym
    cfg = os.path.join(ROOT, SCENES.get(cfg, cfg)) if isinstance(cfg, str) and not os.path.isabs(cfg) else cfg
    kw = dict(device=device) if device else dict(backend_factory=oracle_backend.flavour(flavour) if flavour else oracle_backend.OracleBackend)
    return DIYGym(cfg, num_envs=num_envs, seed=3, engine=engine, **kw)


class Blob:
    """The tables of a scene blob as numpy views (include/diygym_scene.h)."""

    def __init__(self, layout):
        from diy_gym_amd.scene import K
        I, F = layout.I, layout.F
        self.K, self.layout = K, layout
        n = lambda k: int(I[getattr(K, k)])
        ti = lambda off, rows, stride: I[n(off):n(off) + rows * stride].reshape(rows, stride)
        tf = lambda off, rows, stride: F[n(off):n(off) + rows * stride].reshape(rows, stride)
        self.BI, self.BF = ti('H_OFF_BODY_I', n('H_N_BODIES'), K.BI_STRIDE), tf('H_OFF_BODY_F', n('H_N_BODIES'), K.BF_STRIDE)
        self.LI, self.LF = ti('H_OFF_LINK_I', n('H_N_LINKS'), K.LI_STRIDE), tf('H_OFF_LINK_F', n('H_N_LINKS'), K.LF_STRIDE)
        self.SI, self.SF = ti('H_OFF_SHAPE_I', n('H_N_SHAPES'), K.SI_STRIDE), tf('H_OFF_SHAPE_F', n('H_N_SHAPES'), K.SF_STRIDE)
        self.PF = tf('H_OFF_POINT_F', n('H_N_POINTS'), 3)
        self.PI, self.GI = ti('H_OFF_PAIR_I', n('H_N_PAIRS'), K.PI_STRIDE), ti('H_OFF_GROUP_I', n('H_N_GROUPS'), K.GI_STRIDE)
        self.HF = F[:K.HF_FLOAT_COUNT]
        self.margin, self.hmg, self.hull_mode = float(self.HF[K.HF_CONTACT_MARGIN]), float(self.HF[K.HF_HULL_MARGIN]), self.HF[K.HF_HULL_CONTACTS] > 0

    # -- shapes -----------------------------------------------------------------------------------------------------------
    def kind(self, s):
        return int(self.SI[s, self.K.SI_TYPE])

    def body_of(self, s):
        return int(self.SI[s, self.K.SI_BODY])

    def frozen_shape(self, s):
        return bool(self.SI[s, self.K.SI_FLAGS] & self.K.SHAPE_WORLD)

    def prm(self, s):
        return self.SF[s, self.K.SF_PARAMS:self.K.SF_PARAMS + 3]

    def centre(self, s):
        """Shape frame origin (a hull: the centre of its fitted capsule) in the frame the shape is stored in."""
        return self.SF[s, self.K.SF_POS:self.K.SF_POS + 3]

    def rot(self, s):
        return self.SF[s, self.K.SF_ROT:self.K.SF_ROT + 9].reshape(3, 3)

    def points(self, s):
        o, n = int(self.SI[s, self.K.SI_POINT_OFF]), int(self.SI[s, self.K.SI_N_POINTS])
        return self.PF[o:o + n]

    def extent_points(self, s):
        """Points (in the shape's storage frame) and a radius around them that together hold the shape exactly: the shape is
        within `radius` of the convex hull of the points."""
        k, c, R, p = self.kind(s), self.centre(s), self.rot(s), self.prm(s)
        if k == SPHERE:
            return c[None, :], float(p[0])
        if k == CAPSULE:
            return np.stack([c - R[:, 2] * p[1], c + R[:, 2] * p[1]]), float(p[0])
        if k == BOX:
            sg = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
            return c + (sg * p) @ R.T, 0.0
        return self.points(s), 0.0

    def capsule_of_hull(self, s):
        """The capsule fitted to a hull -- what a sphere, a capsule or (hull_contacts = 0) another hull collides with."""
        c, R, p = self.centre(s), self.rot(s), self.prm(s)
        return np.stack([c - R[:, 2] * p[1], c + R[:, 2] * p[1]]), float(p[0])

    # -- kinematics (numpy restatement of the link table; checked against the checker's dgo_frame_state below) -------------------
    def joint_limits(self, b):
        first, n = int(self.BI[b, self.K.BI_FIRST_LINK]), int(self.BI[b, self.K.BI_N_LINKS])
        lo, hi = self.LF[first:first + n, self.K.LF_LOWER].copy(), self.LF[first:first + n, self.K.LF_UPPER].copy()
        free = lo > hi   # a continuous joint
        lo[free], hi[free] = -np.pi, np.pi
        return lo, hi

    def link_frames(self, b, q, base=None):
        """[(R, p)] of the base link frame (index 0) and of every link of body b (index 1 + local link) in the world."""
        K = self.K
        if base is None:
            base = (Rotation.from_quat(self.BF[b, K.BF_INIT_QUAT:K.BF_INIT_QUAT + 4]).as_matrix(), self.BF[b, K.BF_INIT_POS:K.BF_INIT_POS + 3])
        first, n = int(self.BI[b, K.BI_FIRST_LINK]), int(self.BI[b, K.BI_N_LINKS])
        out = [base]
        for i in range(n):
            lf, li = self.LF[first + i], self.LI[first + i]
            Rp, pp = out[0] if li[K.LI_PARENT] < 0 else out[1 + int(li[K.LI_PARENT]) - first]
            RT, pT, ax = lf[K.LF_ROT:K.LF_ROT + 9].reshape(3, 3), lf[K.LF_POS:K.LF_POS + 3], lf[K.LF_AXIS:K.LF_AXIS + 3]
            if li[K.LI_TYPE] == 0:
                Rpc, r = RT @ Rotation.from_rotvec(ax / np.linalg.norm(ax) * q[i]).as_matrix(), pT
            else:
                Rpc, r = RT, pT + RT @ (ax * q[i])
            out.append((Rp @ Rpc, pp + Rp @ r))
        return out

    def shape_frame(self, s, frames_of_body):
        """(R, p) of the frame the shape's centre / points are stored in, in the world."""
        if self.frozen_shape(s):
            return np.eye(3), np.zeros(3)
        gl = int(self.SI[s, self.K.SI_LINK]); b = self.body_of(s)
        return frames_of_body[0] if gl < 0 else frames_of_body[1 + gl - int(self.BI[b, self.K.BI_FIRST_LINK])]


@functools.lru_cache(maxsize=None)
def blob_of(name, engine_items=()):
    env = make(name, **dict(engine_items))
    return Blob(env.layout), env


def sample_configurations(lo, hi, n, rng):
    """Joint configurations inside the limits: all joints at zero (clipped into the limits) first, then the limits' corners (all of
    them up to 6 joints, a random 512 of them beyond), then uniform samples -- at least n in all."""
    k = len(lo)
    out = [np.clip(np.zeros(k), lo, hi)]
    if k:
        bits = np.array([[(c >> j) & 1 for j in range(k)] for c in range(1 << k)]) if k <= 6 else rng.integers(0, 2, size=(512, k))
        out += list(np.where(bits == 1, hi, lo))
    while len(out) < n:
        out.append(rng.uniform(lo, hi))
    return out


# ------------------------------------------------------------------------------------------------------------- shape bounds
def _write_hull_zoo(tmp_path):
    """One free body carrying every shipped hull and the authored point sets as collision shapes of its base link."""
    authored = {
        'cube': [[sx * 0.1, sy * 0.1, sz * 0.1] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)],
        'slab': [[sx * 0.05, sy * 0.1, sz * 0.3] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)],
        'tetrahedron': [[0, 0, 0], [0.2, 0, 0], [0, 0.15, 0], [0.02, 0.03, 0.25]],
        'needle': [[0, 0, -0.4], [0, 0, 0.4], [0.002, 0, 0], [-0.001, 0.002, 0.1], [0, -0.002, -0.2]],
        'plate': [[sx * 0.3, sy * 0.25, sz * 0.004] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)] + [[0.1, 0.05, 0.01]],
    }
    meshes = sorted(glob.glob(os.path.join(DATA, '*', 'hulls', '*')))
    for name, pts in authored.items():
        path = tmp_path / (name + '.obj')
        path.write_text(''.join('v %r %r %r\n' % tuple(float(v) for v in p) for p in pts))
        meshes.append(str(path))
    coll = ''.join('<collision><origin xyz="0 0 0" rpy="0 0 0"/><geometry><mesh filename="%s"/></geometry></collision>\n' % m for m in meshes)
    coll += '<collision><origin xyz="0.1 0.2 0.3" rpy="0.3 0.2 0.1"/><geometry><box size="0.1 0.2 0.6"/></geometry></collision>\n'   # a box on a moving body: its eight corners
    (tmp_path / 'zoo.urdf').write_text('<?xml version="1.0"?>\n<robot name="zoo"><link name="base"><inertial><origin xyz="0 0 0" rpy="0 0 0"/>'
                                       '<mass value="1.0"/><inertia ixx="0.01" ixy="0" ixz="0" iyy="0.01" iyz="0" izz="0.01"/></inertial>\n' + coll + '</link></robot>\n')
    (tmp_path / 'zoo.yaml').write_text('render: no\nzoo: {model: %s, xyz: [0, 0, 1]}\n' % (tmp_path / 'zoo.urdf'))
    return str(tmp_path / 'zoo.yaml'), len(meshes) + 1


def sc_bound(prm, kind, hull_mode):
    """SC_BOUND as collide() stores it (dg_solver.h; the source line is pinned by test_the_restated_expressions_are_the_sources)."""
    if kind == POINTS:
        return max(prm[0] + prm[1], prm[2])
    return prm[0] + (0.0 if kind == SPHERE else prm[1])


def static_extent(prm, kind):
    """Extent of a static partner in the group reach (dg_plan.hip for a frozen one, dg_solver.h for a fixed one that is not)."""
    if kind == SPHERE:
        return prm[0]
    if kind == BOX:
        return float(np.sqrt(prm @ prm))
    if kind == POINTS:
        return max(prm[0] + prm[1], prm[2])
    return prm[0] + prm[1]


def group_margin(blob):
    """Distance term of every group reach: the contact margin, plus the two hull margins when hulls collide as hulls."""
    return blob.margin + (2.0 * blob.hmg if blob.hull_mode else 0.0)


def test_the_restated_expressions_are_the_sources():
    """sc_bound / static_extent / group_margin above restate device code; this pins the lines they restate."""
    solver = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_solver.h')).read()
    plan = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_plan.hip')).read()
    assert 'ln.L(o + SC_BOUND) = type == DG_SHAPE_POINTS ? fmaxf(w.prm0 + w.prm1, w.prm2) : w.prm0 + (type == DG_SHAPE_SPHERE ? 0.f : w.prm1);' in solver
    assert len(re.findall(r'sphere_box\((?:cu\.)?ca, ln\.L\(oa \+ SC_BOUND\), b, margin\)', solver)) == 2   # both hull-against-box culls read it
    ext = 'st == DG_SHAPE_POINTS ? fmaxf(p0 + p1, p2) : p0 + p1'
    assert ext in plan and ext in solver
    gm = 'const float gmargin = margin + (hull_mode ? 2.f * hmg : 0.f);'
    assert gm in solver and 'float reach = sc.BF[ba * DG_BF_STRIDE + DG_BF_BOUND] + gmargin;' in solver
    assert '(float)F[DG_HF_CONTACT_MARGIN] + (F[DG_HF_HULL_CONTACTS] > 0 ? 2.f * (float)F[DG_HF_HULL_MARGIN] : 0.f) + ext' in plan


@pytest.mark.parametrize('hull_contacts', [0.0, 1.0])
def test_the_sphere_of_a_hull_holds_its_points(tmp_path, hull_contacts):
    """SC_BOUND of every hull -- every file under data/*/hulls, a cube, the 0.05 x 0.1 x 0.3 slab, a tetrahedron, a needle, a
    plate and a box on a moving body -- around the centre the device uses (the fitted capsule's) holds every hull point, in both
    hull_contacts modes; so do the scene's own fixtures.  The hull-against-box culls of both code paths test exactly this sphere."""
    cfg, n_hulls = _write_hull_zoo(tmp_path)
    blobs = [Blob(make(cfg, hull_contacts=hull_contacts).layout)] + [Blob(make(n, hull_contacts=hull_contacts).layout) for n in ('np_cube_ground', 'np_slab_ground', 'np_gem_wedge', 'ur_high_5')]
    assert sum(blobs[0].kind(s) == POINTS for s in range(len(blobs[0].SI))) == n_hulls
    checked = 0
    for blob in blobs:
        for s in range(len(blob.SI)):
            if blob.kind(s) != POINTS:
                continue
            need = float(np.max(np.linalg.norm(blob.points(s) - blob.centre(s), axis=1)))
            assert sc_bound(blob.prm(s), POINTS, blob.hull_mode) >= need - EPS, (s, need - sc_bound(blob.prm(s), POINTS, blob.hull_mode))
            checked += 1
    assert checked > n_hulls + 10


def test_the_capsule_of_the_second_cull_holds_its_hull(tmp_path):
    """The capsule of radius prm0 and half length DG_SF_HULL_HALF about the fitted axis holds every hull point (shortfall <= 1e-9,
    scene.py's epsilon): the distance of two such capsules is a lower bound of the hulls'."""
    cfg, n_hulls = _write_hull_zoo(tmp_path)
    worst = 0.0
    for blob in [Blob(make(cfg).layout), Blob(make('ur5_child_gripper').layout), Blob(make('np_gem_wedge').layout)]:
        for s in range(len(blob.SI)):
            if blob.kind(s) != POINTS:
                continue
            d, ax, hh = blob.points(s) - blob.centre(s), blob.rot(s)[:, 2], float(blob.SF[s, blob.K.SF_HULL_HALF])
            t = d @ ax
            on_seg = np.clip(t, -hh, hh)[:, None] * ax[None, :]
            short = float(np.max(np.linalg.norm(d - on_seg, axis=1))) - float(blob.prm(s)[0])
            worst = max(worst, short)
            assert short <= EPS, (s, short)
    assert worst > -1.0


# -------------------------------------------------------------------------------------------------------------- body bounds
def _jaco_yaml(tmp_path):
    (tmp_path / 'jaco.yaml').write_text('render: no\njaco: {model: jaco/j2s7s300_standalone.urdf, use_fixed_base: yes, xyz: [0.1, -0.2, 0.3], rpy: [0.0, 0.0, 0.4]}\n')
    return str(tmp_path / 'jaco.yaml')


def test_numpy_kinematics_of_the_link_table_agree_with_the_checker():
    """Blob.link_frames against dgo_frame_state (frame 7 of the UR5 is its ee_link, on the last link) at a random configuration."""
    blob, env = blob_of('ur_high_5')
    K, rng = blob.K, np.random.default_rng(0)
    q = rng.uniform(-2, 2, 6); st = env.sim.get_state()
    for i in range(6):
        st[0, env.layout.link_state_off[env.layout.body_first_link[1] + i]] = q[i]
    env.sim.set_state(st)
    got = env.sim.frame_state64(1, 6)[0]   # the wrist_3 link frame
    R, p = blob.link_frames(1, q)[6]
    assert np.allclose(got[:3], p, atol=1e-12)
    assert np.allclose(Rotation.from_quat(got[3:7]).as_matrix(), R, atol=1e-9)


@pytest.mark.parametrize('scene,body', [('ur_high_5', 0), ('jaco', 0), ('ur5_child_gripper', None), ('cart_tree', None), ('np_two_arms', 1)])
def test_body_bound_and_anchors_hold_every_shape_in_every_configuration(tmp_path, scene, body):
    """BF_BOUND (a sphere around the base origin) and the anchors of the static pruning hold every collision shape of the body --
    hull points, box corners, spheres, capsules, and the capsule fitted to each hull, which is what round shapes collide with -- at
    2 000+ joint configurations inside the limits, the limits' corners included."""
    env = make(_jaco_yaml(tmp_path) if scene == 'jaco' else scene)
    blob, rng = Blob(env.layout), np.random.default_rng(11)
    bodies = [body] if body is not None else [b for b in range(len(blob.BI)) if blob.BI[b, blob.K.BI_N_LINKS] > 0]
    assert bodies
    for b in bodies:
        shapes = [s for s in range(len(blob.SI)) if blob.body_of(s) == b]
        bound = float(blob.BF[b, blob.K.BF_BOUND])
        lo, hi = blob.joint_limits(b)
        worst = -np.inf
        for q in sample_configurations(lo, hi, 2000, rng):
            frames = blob.link_frames(b, q)
            base = frames[0][1]
            for s in shapes:
                R, p = blob.shape_frame(s, frames)
                sets = [blob.extent_points(s)] + ([blob.capsule_of_hull(s)] if blob.kind(s) == POINTS else [])
                for pts, rad in sets:
                    w = pts @ R.T + p
                    far = float(np.max(np.linalg.norm(w - base, axis=1))) + rad
                    worst = max(worst, far - bound)
                    assert far <= bound * (1 + F32) + EPS, (b, s, far, bound)
                    anchor = env.layout.shape_anchors[s]
                    if anchor is not None:
                        assert float(np.max(np.linalg.norm(w - anchor[0], axis=1))) + rad <= anchor[1] + EPS, (b, s)
        assert worst > -0.5 * bound   # (the bound is not vacuous either)


# -------------------------------------------------------------------------------------------------------------- group reach
def gd_table(layout):
    from diy_gym_amd import backend
    plan = backend.debug_plan(layout, 64, 256)
    ng = int(layout.I[Blob(layout).K.H_N_GROUPS])
    return plan['table'][plan['gd_off']:plan['gd_off'] + 4 * ng].view(np.float32).reshape(ng, 4).astype(np.float64)


def pair_report_distance(blob, a, c):
    return blob.margin + (2.0 * blob.hmg if blob.hull_mode and blob.kind(a) == POINTS and blob.kind(c) == POINTS else 0.0)


def true_extent(blob, s, partner, centre):
    """How far shape s reaches from `centre` (storage frame of s), as the exact routine of the pair (s, partner) sees it."""
    if blob.kind(s) == POINTS and not (blob.kind(partner) == BOX or (blob.kind(partner) == POINTS and blob.hull_mode)):
        pts, rad = blob.capsule_of_hull(s)    # against round shapes a hull is its fitted capsule
    else:
        pts, rad = blob.extent_points(s)
    return float(np.max(np.linalg.norm(pts - centre, axis=1))) + rad


@pytest.mark.parametrize('hull_margin', [0.001, 0.01])
@pytest.mark.parametrize('scene', ['ur_high_5', 'ur_arms_touching', 'from_the_readme', 'r2d2_maze', 'basic_env', 'box_stack',
                                   'np_cube_ground', 'np_slab_ground', 'np_gem_wedge', 'np_gem_wedge_respawned', 'np_gems', 'np_two_arms'])
def test_group_reach_covers_partner_and_report_distance(monkeypatch, scene, hull_margin):
    """reach of a group >= bound of the moving body + true extent of the partner about the centre the device uses + the distance
    at which the exact routine still reports a hit, for every pair of every group: GD[3] of the plan table for a frozen partner,
    the restated expressions of collide() for a fixed partner that is not frozen and for a moving one."""
    for var in ('DG_MAX_LANES', 'DG_NO_NARROW_MODES'):
        monkeypatch.delenv(var, raising=False)
    env = make(scene, hull_margin=hull_margin)
    blob = Blob(env.layout); K = blob.K; GD = gd_table(env.layout)
    kinds = set()
    for g, gi in enumerate(blob.GI):
        ba, bb, ss = int(gi[K.GI_BODY_A]), int(gi[K.GI_BODY_B]), int(gi[K.GI_STATIC_SHAPE])
        bound_a = float(blob.BF[ba, K.BF_BOUND])
        frozen = ss >= 0 and blob.frozen_shape(ss)
        assert (GD[g, 3] >= 0) == frozen
        if frozen:
            reach, centre = GD[g, 3] * (1 + F32), GD[g, :3]
            assert np.allclose(centre, blob.centre(ss), atol=1e-6 * max(1.0, float(np.abs(centre).max())))
        elif ss >= 0:
            reach, centre = bound_a + group_margin(blob) + static_extent(blob.prm(ss), blob.kind(ss)), blob.centre(ss)
        else:
            reach = bound_a + group_margin(blob) + float(blob.BF[bb, K.BF_BOUND])
        kinds.add('frozen' if frozen else 'static' if ss >= 0 else 'moving')
        for a, c in blob.PI[int(gi[K.GI_FIRST]):int(gi[K.GI_FIRST]) + int(gi[K.GI_COUNT])]:
            a, c = int(a), int(c)
            if ss >= 0:
                other = a if c == ss else c
                assert ss in (a, c) and blob.body_of(other) == ba
                need = bound_a + true_extent(blob, ss, other, blob.centre(ss)) + pair_report_distance(blob, a, c)
            else:
                assert {blob.body_of(a), blob.body_of(c)} == {ba, bb}
                need = bound_a + float(blob.BF[bb, K.BF_BOUND]) + pair_report_distance(blob, a, c)   # (the body bounds themselves: the test above)
            assert reach >= need - EPS, (scene, g, a, c, need - reach)
    assert kinds or len(blob.PI) == 0   # (np_two_arms at the default hull margin: its one pair is rightly pruned)


# ------------------------------------------------------------------------------------------------------------------ pruning
def _seg_seg(p1, q1, p2, q2):
    """Distance of two segments (Ericson 5.1.9), numpy."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f = d1 @ d1, d2 @ d2, d2 @ r
    if a <= 1e-18 and e <= 1e-18:
        return float(np.linalg.norm(r))
    if a <= 1e-18:
        s, t = 0.0, np.clip(f / e, 0, 1)
    else:
        c = d1 @ r
        if e <= 1e-18:
            t, s = 0.0, np.clip(-c / a, 0, 1)
        else:
            b = d1 @ d2; den = a * e - b * b
            s = np.clip((b * f - c * e) / den, 0, 1) if den > 1e-18 else 0.0
            t = (b * s + f) / e
            if t < 0:
                t, s = 0.0, np.clip(-c / a, 0, 1)
            elif t > 1:
                t, s = 1.0, np.clip((b - c) / a, 0, 1)
    return float(np.linalg.norm((p1 + d1 * s) - (p2 + d2 * t)))


def exact_within(blob, L64, a, c, Ta, Tc, reach):
    """Would the narrow phase's exact routine report pair (a, c), posed by the storage frames Ta / Tc = (R, p), within `reach`?
    Hull against hull: the fp64 checker's GJK (dgo_hull_hull); everything else: closed forms on the shapes' skeletons."""
    ka, kc = blob.kind(a), blob.kind(c)
    if ka == POINTS and kc == POINTS and blob.hull_mode:
        hit, out, _ = oracle_pair(L64, blob.points(a), Ta, blob.points(c), Tc, max_dist=reach)
        return bool(hit) and out[9] < reach
    if BOX in (ka, kc):
        s, bx, Ts, Tb = (a, c, Ta, Tc) if kc == BOX else (c, a, Tc, Ta)
        pts, rad = blob.extent_points(s)    # hull points / capsule ends + radius / sphere centre + radius: what the routines test against a box
        w = pts @ Ts[0].T + Ts[1]
        Rb = Tb[0] @ blob.rot(bx); pb = Tb[1] + Tb[0] @ blob.centre(bx)
        local = (w - pb) @ Rb
        d = np.linalg.norm(local - np.clip(local, -blob.prm(bx), blob.prm(bx)), axis=1)
        return float(d.min()) - rad < reach
    sa, ra = blob.capsule_of_hull(a) if ka != SPHERE else blob.extent_points(a)
    sc_, rc = blob.capsule_of_hull(c) if kc != SPHERE else blob.extent_points(c)
    wa, wc = sa @ Ta[0].T + Ta[1], sc_ @ Tc[0].T + Tc[1]
    return _seg_seg(wa[0], wa[-1], wc[0], wc[-1]) - ra - rc < reach


@pytest.mark.parametrize('scene,engine', [('ur_high_5', {}), ('ur_arms_touching', {}), ('np_two_arms', {'hull_margin': 0.01})])
def test_pruned_pairs_never_come_within_reporting_distance(scene, engine):
    """Every shape pair the static pruning removed (layout.pruned_pairs, scene.statically_apart): at 2 000+ configurations of the
    two bodies, limits' corners included, the exact routine of the pair would report nothing.

    np_two_arms with hull_margin = 0.01 is the case the old threshold (contact_margin + 1 mm, whatever the hull margin) got wrong:
    sample 0 -- both joints at zero, the tips 0.03 m apart -- is inside contact_margin + 2 x hull_margin = 0.04 m, and the pair was
    pruned (anchor gap 0.03 m > 0.021 m).  With the threshold at the reporting distance it is kept: the fixture then has one
    candidate pair and nothing pruned, which the test asserts as well."""
    env = make(scene, **engine)
    blob, L64, rng = Blob(env.layout), hull_lib('f64'), np.random.default_rng(5)
    pruned = [(int(a), int(c)) for a, c in env.layout.pruned_pairs]
    if scene == 'np_two_arms':
        assert pruned == [] and len(blob.PI) == 1
        # the sample that shows it: joints at zero, tips 0.03 m apart, one hull-hull contact within 0.04 m
        fa, fb = blob.link_frames(0, np.zeros(1)), blob.link_frames(1, np.zeros(1))
        a, c = (int(v) for v in blob.PI[0])
        assert exact_within(blob, L64, a, c, blob.shape_frame(a, fa), blob.shape_frame(c, fb), pair_report_distance(blob, a, c))
        hit, out, _ = oracle_pair(L64, blob.points(a), blob.shape_frame(a, fa), blob.points(c), blob.shape_frame(c, fb))
        assert abs(out[9] - 0.03) < 1e-9
        return
    assert pruned   # (the shoulders of the two arms, at least)
    by_bodies = {}
    for a, c in pruned:
        by_bodies.setdefault((blob.body_of(a), blob.body_of(c)), []).append((a, c))
    for (ba, bc), pairs in by_bodies.items():
        qa = sample_configurations(*blob.joint_limits(ba), 2000, rng); qc = sample_configurations(*blob.joint_limits(bc), 2000, rng)
        order = rng.permutation(len(qc))
        for k in range(min(len(qa), len(qc))):
            fa, fc = blob.link_frames(ba, qa[k]), blob.link_frames(bc, qc[k if k == 0 else order[k]])
            for a, c in pairs:
                assert not exact_within(blob, L64, a, c, blob.shape_frame(a, fa), blob.shape_frame(c, fc), pair_report_distance(blob, a, c)), (a, c, k)


# ======================================================================================================================
# GPU: the device's contact list against the checker where a cull decides
# ======================================================================================================================
B = 128   # two wavefronts of 64 envs (more wavefronts in the narrower workspace modes); the sweeps are sorted, so the envs of a wavefront are neighbours in the sweep
KERNEL_FORMS = {'default': {}, 'lanes16': {'DG_MAX_LANES': '16'}, 'lanes1': {'DG_MAX_LANES': '1'}, 'no_narrow_modes': {'DG_NO_NARROW_MODES': '1'},
                'no_helper_wave': {'DG_NO_HELPER_WAVE': '1'}}
SWITCHES = ('DG_MAX_LANES', 'DG_NO_NARROW_MODES', 'DG_NO_HELPER_WAVE')
CLEAR = 1e-4   # every swept distance stays this far from every threshold


def sweep(lo, hi, n, avoid=()):
    """n sorted values in [lo, hi], none within 2 x CLEAR of a threshold in `avoid` (moved to the nearer side)."""
    v = np.linspace(lo, hi, n)
    for t in avoid:
        near = np.abs(v - t) < 2 * CLEAR
        v[near] = np.where(v[near] < t, t - 2 * CLEAR, t + 2 * CLEAR)
    return np.sort(v)


def rot_to(src, dst):
    """A rotation that takes the unit vector src to dst."""
    src, dst = np.asarray(src, float) / np.linalg.norm(src), np.asarray(dst, float) / np.linalg.norm(dst)
    ax = np.cross(src, dst); s = np.linalg.norm(ax)
    if s < 1e-12:
        return np.eye(3) if src @ dst > 0 else Rotation.from_rotvec(np.pi * np.array([0.0, 0.0, 1.0] if abs(src[2]) < 0.9 else [1.0, 0.0, 0.0])).as_matrix()
    return Rotation.from_rotvec(ax / s * np.arctan2(s, src @ dst)).as_matrix()


def yaws(n):
    return np.linspace(0.0, 2.0 * np.pi, n, endpoint=False) * 0.37 + 0.05


def place(env, st, body, R, p):
    """Write the pose of the root inertial frame = base link frame (the fixtures' URDFs have them coincide) of a body into a state
    array, velocities zero."""
    from diy_gym_amd.scene import K
    off = env.layout.body_state_off[body]
    st[:, off:off + 3] = p
    st[:, off + 3:off + 7] = Rotation.from_matrix(R).as_quat()
    if not env.layout.body_fixed[body]:
        st[:, off + K.BS_LINVEL:off + K.BS_FLOAT_END] = 0.0


def corner_down_states(env, scene, heights):
    """The box of np_cube_ground / np_slab_ground standing on the corner (-hx, -hy, -hz), that corner at the given heights over the
    ground, each env turned by its own yaw about the vertical (the contact normal)."""
    half = np.array([0.1, 0.1, 0.1]) if scene == 'np_cube_ground' else np.array([0.05, 0.1, 0.3])
    R0 = rot_to(half, [0, 0, 1])   # the body diagonal upright: the corner -half is the lowest point
    st = np.asarray(env.sim.get_state(), dtype=np.float64).copy()
    R = np.stack([Rotation.from_euler('z', y).as_matrix() @ R0 for y in yaws(len(heights))])
    p = np.stack([np.array([0.01 * np.cos(k), 0.01 * np.sin(k), h + np.linalg.norm(half)]) for k, h in enumerate(heights)])
    place(env, st, 1, R, p)
    return st


def second_corner_rise(scene):
    """Height of the second-lowest corner over the lowest one for the box standing on a corner."""
    half = np.array([0.1, 0.1, 0.1]) if scene == 'np_cube_ground' else np.array([0.05, 0.1, 0.3])
    return 2.0 * float(np.min(half ** 2)) / float(np.linalg.norm(half))


WEDGE_CORNER = np.array([0.0, 0.1, 0.3])   # of np_wedge.obj, 28 mm outside r + half of its fitted capsule
GEM_TIP = 0.06                             # of np_gem.obj along its x axis = BF_BOUND of the free gem


def gem_at_wedge_states(env, blob, gaps):
    """np_gem_wedge*: the gem's +x tip pointing at the wedge's corner (0, 0.1, 0.3) along the line from the centre the group test
    uses (the fitted capsule's) through that corner, the tip `gap` away from it, each env turned about that line."""
    wedge_shape = [s for s in range(len(blob.SI)) if blob.body_of(s) == 0][0]
    Rw, pw = np.eye(3), np.array([0.0, 0.0, 1.0])   # pose of the wedge's body (the YAML's; written into the state where it has one)
    c_local = blob.centre(wedge_shape) - (pw if blob.frozen_shape(wedge_shape) else 0.0)   # (a frozen shape is stored in world coordinates)
    u = (WEDGE_CORNER - c_local) / np.linalg.norm(WEDGE_CORNER - c_local)
    st = np.asarray(env.sim.get_state(), dtype=np.float64).copy()
    R0 = rot_to([1, 0, 0], -u)
    R = np.stack([Rotation.from_rotvec(u * y).as_matrix() @ R0 for y in yaws(len(gaps))])
    p = np.stack([pw + WEDGE_CORNER + u * (g + GEM_TIP) for g in gaps])
    if env.layout.body_state_off[0] >= 0:
        place(env, st, 0, np.stack([Rw] * len(gaps)), np.stack([pw] * len(gaps)))
    place(env, st, 1, R, p)
    return st


def gems_states(env, gaps):
    """np_gems: the two gems tip to tip along x, `gap` between the tips, the right one turned about x by its env's yaw."""
    st = np.asarray(env.sim.get_state(), dtype=np.float64).copy()
    n = len(gaps)
    place(env, st, 0, np.stack([np.eye(3)] * n), np.stack([np.array([-GEM_TIP - 0.5 * g, 0.0, 1.0]) for g in gaps]))
    place(env, st, 1, np.stack([Rotation.from_euler('x', y).as_matrix() for y in yaws(n)]), np.stack([np.array([GEM_TIP + 0.5 * g, 0.0, 1.0]) for g in gaps]))
    return st


def checker_step(scene, st, engine, flavour=None):
    cpu = make(scene, num_envs=len(st), flavour=flavour, **engine)
    cpu.sim.set_state(np.asarray(st, dtype=cpu.sim.real))
    cpu.sim.step(cpu._all_slots, cpu.sim.act * 0)
    return cpu, [cpu.sim.contacts(e) for e in range(len(st))]


def run_case(monkeypatch, scene, st, engine, form, want_par=None):
    """One step from `st` on the device in kernel form `form` and in the fp64 checker: the same contact count in every env, and the
    observations as close as the teacher-forced single steps of tests/test_hull_contacts.py ask (median < 5e-4, 97 % of the envs
    < 5e-3).  First, on the CPU: the fp32 and fp64 builds of the checker agree on the count of every env -- the poses are at least
    1e-4 m from every threshold, so the count cannot turn on rounding; no (env, step) pair is left out.

    The share of envs allowed beyond 5e-3 is calibrated from the two checker builds on the same inputs: 3 % as in
    test_hull_contacts.py, or twice the share of envs in which the fp32 and the fp64 build of the checker are themselves more than
    5e-3 apart, whichever is larger.  That share is 0 in every case but the hull at the prism's corner: there 5 of the 128 envs
    (3.9 %; gaps -1.6 .. -0.1 mm, the margin-free hulls overlapping vertex into vertex, where the minimum-translation direction is
    discontinuous and the 0.2 kg hull spins up by 2 rad/s either way) differ by up to 2.05 between the builds, so 92.2 % of the
    envs must be within 5e-3; the device measured 95.3 .. 96.1 % over the kernel forms."""
    import torch
    cpu, counts = checker_step(scene, st, engine)
    cpu32, counts32 = checker_step(scene, st, engine, flavour='f32')
    assert counts == counts32
    builds_apart = float(np.mean((cpu32.sim.obs - cpu.sim.obs).abs().max(1).values.numpy() >= 5e-3))
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    for var, value in KERNEL_FORMS[form].items():
        monkeypatch.setenv(var, value)
    gpu = make(scene, num_envs=len(st), device='cuda:0', **engine)
    if want_par is not None:
        assert gpu.sim.par == want_par
    if 'DG_MAX_LANES' in KERNEL_FORMS[form]:
        assert gpu.sim.lanes <= int(KERNEL_FORMS[form]['DG_MAX_LANES'])   # (0 / -16: a global-workspace mode, where the scene does not fit)
    d = gpu.sim.enable_diagnostics()
    gpu.sim.set_state(np.asarray(st, dtype=np.float32))
    gpu.sim.step(gpu._all_slots, gpu.sim.act * 0)
    torch.cuda.synchronize()
    got = d[:, 0].tolist()
    errs = (gpu.sim.obs.cpu() - cpu.sim.obs).abs().max(1).values.numpy()
    print('%s %s %s: lanes %d, device counts %s checker %s, obs err median %.3g max %.3g within 5e-3 %.4f, checker builds apart in %.4f' %
          (scene, engine, form, gpu.sim.lanes, sorted(set(got)), sorted(set(counts)), np.median(errs), errs.max(), np.mean(errs < 5e-3), builds_apart))
    assert got == counts
    assert np.isfinite(errs).all() and np.median(errs) < 5e-4, (np.median(errs), errs.max())
    assert np.mean(errs < 5e-3) > 1.0 - max(0.03, 2.0 * builds_apart), (np.mean(errs < 5e-3), builds_apart, errs.max())
    return counts


FREE_FORMS = ['default', 'lanes16', 'lanes1', 'no_narrow_modes']


@pytest.mark.gpu
@pytest.mark.parametrize('form', FREE_FORMS)
@pytest.mark.parametrize('hull_contacts', [0.0, 1.0])
@pytest.mark.parametrize('scene', ['np_cube_ground', 'np_slab_ground'])
def test_a_box_landing_on_a_corner_gets_its_ground_contact(monkeypatch, scene, hull_contacts, form):
    """A free cube (half edge 0.1) / the 0.05 x 0.1 x 0.3 slab standing on a corner over the ground box, the corner swept from
    -5 mm to contact_margin - 0.1 mm over 128 envs: the checker reports the corner's contact in every env (the slab's second
    corner as well below 4.4 mm).  Before the fix hull_contacts = 0 failed in every form: SC_BOUND = r + half ended 31.8 mm (cube)
    / 20.2 mm (slab) short of the corner, so a wavefront whose corners were all above -11.8 mm / -0.2 mm got no contact."""
    margin = 0.02
    heights = sweep(-0.005, margin - CLEAR, B, avoid=[margin - second_corner_rise(scene)])
    env = make(scene, num_envs=B, hull_contacts=hull_contacts)
    counts = run_case(monkeypatch, scene, corner_down_states(env, scene, heights), dict(hull_contacts=hull_contacts), form)
    assert min(counts) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize('form', FREE_FORMS)
@pytest.mark.parametrize('scene', ['np_gem_wedge', 'np_gem_wedge_respawned'])
def test_a_hull_at_the_corner_of_a_static_hull(monkeypatch, scene, form):
    """A free hull with its tip at the far corner of a static prism, the gap swept from -5 mm to contact_margin + 2 x hull_margin
    - 0.1 mm: one hull-hull contact in every env.  The prism is frozen in the world (its group reach is GD[3] of the plan table) or
    respawned (fixed, not frozen: the reach is worked out in collide()).  Before the fix both failed: the prism's extent in the
    reach was r + half = 0.300 m of its fitted capsule, its corner is 0.328 m from that capsule's centre, and the group was culled
    for every gap above -8 mm."""
    env = make(scene, num_envs=B); blob = Blob(env.layout)
    gaps = sweep(-0.005, blob.margin + 2 * blob.hmg - CLEAR, B, avoid=[CLEAR])   # (the GJK / polytope switch, at a hull distance of 0.1 mm)
    counts = run_case(monkeypatch, scene, gem_at_wedge_states(env, blob, gaps), {}, form)
    assert counts == [1] * B


@pytest.mark.gpu
@pytest.mark.parametrize('form', FREE_FORMS)
@pytest.mark.parametrize('hull_margin', [0.001, 0.01])
def test_two_free_hulls_inside_their_margins(monkeypatch, hull_margin, form):
    """Two free hulls tip to tip, the gap swept over (contact_margin, contact_margin + 2 x hull_margin), 0.1 mm off both ends: one
    contact in every env.  Before the fix the group test of two moving bodies (BF_BOUND + BF_BOUND + contact_margin) culled all of
    them: the tips are the points farthest from the base origins."""
    margin = 0.02
    gaps = sweep(margin + CLEAR, margin + 2 * hull_margin - CLEAR, B)
    env = make('np_gems', num_envs=B, hull_margin=hull_margin)
    counts = run_case(monkeypatch, 'np_gems', gems_states(env, gaps), dict(hull_margin=hull_margin), form)
    assert counts == [1] * B


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['default', 'no_helper_wave', 'lanes16', 'lanes1', 'no_narrow_modes'])
def test_the_two_arm_fixture_keeps_its_pair(monkeypatch, form):
    """np_two_arms with hull_margin = 0.01, joints at the closest pass (zero) and up to +-0.01 rad about it: the tips are 0.030 ..
    0.031 m apart, inside contact_margin + 2 x hull_margin = 0.04 m.  The expected count comes from dgo_hull_hull on the posed
    hulls (one contact in every env), not from the stepped checker alone -- before the fix the pair was pruned from the table both
    backends read, and both reported nothing."""
    engine = dict(hull_margin=0.01)
    env = make('np_two_arms', num_envs=B, **engine); blob, L64 = Blob(env.layout), hull_lib('f64')
    st = np.asarray(env.sim.get_state(), dtype=np.float64).copy()
    qa, qb = np.linspace(-0.01, 0.01, B), 0.01 * np.sin(np.arange(B))
    st[:, env.layout.link_state_off[0]], st[:, env.layout.link_state_off[1]] = qa, qb
    assert len(blob.PI) == 1
    a, c = (int(v) for v in blob.PI[0])
    for e in range(B):
        fa, fb = blob.link_frames(0, qa[e:e + 1]), blob.link_frames(1, qb[e:e + 1])
        hit, out, _ = oracle_pair(L64, blob.points(a), blob.shape_frame(a, fa), blob.points(c), blob.shape_frame(c, fb))
        assert hit and blob.margin + CLEAR < out[9] < blob.margin + 2 * blob.hmg - CLEAR
    counts = run_case(monkeypatch, 'np_two_arms', st, engine, form, want_par={'default': True, 'no_helper_wave': False}.get(form))
    assert counts == [1] * B


@pytest.mark.gpu
def test_a_masked_reset_runs_its_hot_start_steps_with_the_contact(monkeypatch, tmp_path):
    """The reset kernel's narrow phase (TBL == 0: one scalar load per pair, under the per-env mask) on the cube over the ground:
    the cube is LOADED standing on a corner 4 mm inside the ground with hull_contacts = 0, the second wavefront is reset, and its
    hot-start steps must push the cube out as the checker's do.  Before the fix the cull dropped the contact (the corner would
    have had to be 11.8 mm inside) and the cube fell freely."""
    import torch
    import yaml
    from diy_gym_amd.config import Configuration
    for var in SWITCHES:
        monkeypatch.delenv(var, raising=False)
    half = np.array([0.1, 0.1, 0.1])
    tree = yaml.safe_load(open(os.path.join(ROOT, SCENES['np_cube_ground'])))
    tree['hot_start'] = 3
    tree['hull']['respawn'] = {'addon': 'respawn'}   # (a reset puts only respawned bodies back to their load pose)
    tree['hull']['xyz'] = [0.0, 0.0, float(np.linalg.norm(half)) - 0.004]
    tree['hull']['rpy'] = [float(v) for v in Rotation.from_matrix(rot_to(half, [0, 0, 1])).as_euler('xyz')]
    tree['plane']['model'] = os.path.join(DATA, 'pybullet_data', 'plane.urdf'); tree['hull']['model'] = os.path.join(GOLDEN, 'urdf', 'np_cube.urdf')
    cfg = lambda: Configuration.from_dict('np_cube_reset', copy.deepcopy(tree))
    engine = dict(hull_contacts=0.0)
    gpu, cpu = make(cfg(), num_envs=B, device='cuda:0', **engine), make(cfg(), num_envs=B, **engine)
    far = np.asarray(cpu.sim.get_state()).copy(); far[:, cpu.layout.body_state_off[1] + 2] += 1.0   # everyone a metre up ...
    gpu.sim.set_state(far.astype(np.float32)); cpu.sim.set_state(far)
    mask = torch.zeros(B, dtype=torch.bool); mask[64:] = True                                   # ... then the second wavefront back to the load pose
    gpu.sim.reset(mask.to('cuda:0')); cpu.sim.reset(mask)
    torch.cuda.synchronize()
    phys = cpu.layout.physical_dim
    g, c = np.asarray(gpu.sim.get_state(), dtype=np.float64)[:, :phys], np.asarray(cpu.sim.get_state(), dtype=np.float64)[:, :phys]
    off = cpu.layout.body_state_off[1]
    assert np.all(c[64:, off + 9] > 0.05)    # the checker pushes the reset cubes out: upward velocity (free fall would be -0.06 m/s)
    assert np.allclose(g[:64], c[:64], atol=1e-5)
    err = np.abs(g[64:] - c[64:]).max(axis=1)
    print('masked reset: state err median %.3g max %.3g, checker vz %.3g' % (np.median(err), err.max(), c[64, off + 9]))
    assert np.median(err) < 5e-4 and np.mean(err < 5e-3) > 0.97
