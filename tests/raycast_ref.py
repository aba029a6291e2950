"""fp64 numpy ray caster over the scene layout: the reference of the ray-casting tests.

Shape parameters and hull face planes are read from the layout's blob, link poses from ``OracleBackend.frame_state64``; the
library under test is never called.  ``RaycastOracleBackend`` puts it behind ``ray_test_batch`` so that host tests can run the
``lidar`` addon without a GPU.  Semantics as ``dg_world_raycast`` (include/diygym_hip.h): the nearest entry point with
0 <= frac < 1 wins, a ray that starts inside a convex shape does not hit it, a zero-length ray hits nothing, ties go to the
lower shape index.

For every hit the caster also returns an EDGE MARGIN: for a box or hull hit the gap, in metres along the ray, between the
entering face that won and the runner-up (a ray within a hair of an edge may enter through the neighbouring face in fp32: same
point, another normal); infinite for spheres and capsules.

A capsule is cast as its cylinder between the end planes plus each end sphere BEYOND its end plane -- the solid's surface and
nothing else -- where the kernel takes the earliest of cylinder and whole end spheres after rejecting rays that start inside:
two formulations of the same solid.
"""
import copy
import os

import numpy as np
import torch

from diy_gym_amd.backend import RayHits
from diy_gym_amd.scene import K
from oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 1e-30
EDGE = 1e-3   # metres: a hit whose margin is below this is an "edge ray"


def quat_mat(q):
    """Rotation matrices [..., 3, 3] of quaternions [..., 4] (x, y, z, w)."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - z * w); R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w); R[..., 2, 1] = 2 * (y * z + x * w); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


class RaycastRef:
    def __init__(self, layout):
        I, F = layout.I, np.asarray(layout.F, dtype=np.float64)
        self.layout = layout
        nfr, self.nsh = int(I[K.H_N_FRAMES]), int(I[K.H_N_SHAPES])
        self.FI = I[I[K.H_OFF_FRAME_I]:I[K.H_OFF_FRAME_I] + nfr * K.FI_STRIDE].reshape(-1, K.FI_STRIDE)
        self.SI = I[I[K.H_OFF_SHAPE_I]:I[K.H_OFF_SHAPE_I] + self.nsh * K.SI_STRIDE].reshape(-1, K.SI_STRIDE)
        self.SF = F[I[K.H_OFF_SHAPE_F]:I[K.H_OFF_SHAPE_F] + self.nsh * K.SF_STRIDE].reshape(-1, K.SF_STRIDE)
        self.FF = F[I[K.H_OFF_FRAME_F]:I[K.H_OFF_FRAME_F] + len(self.FI) * K.FF_STRIDE].reshape(-1, K.FF_STRIDE)
        self.PLN = F[I[K.H_OFF_PLANE_F]:I[K.H_OFF_PLANE_F] + 4 * int(I[K.H_N_PLANES])]
        self.seg = self.SI[:, K.SI_BODY] + (((self.SI[:, K.SI_FLAGS] >> 8) & 0xFFFF) << 24)

    # ---- poses -------------------------------------------------------------------------------------------------------
    def _local_frame(self, body, gframe):
        return int(np.nonzero(np.nonzero(self.FI[:, K.FI_BODY] == body)[0] == gframe)[0][0])

    def link_pose(self, sim, body, glink, cache):
        """World rotation [B, 3, 3] and origin [B, 3] of link ``glink`` (global index, -1: the base link) of ``body``."""
        key = (body, glink)
        if key not in cache:
            if glink < 0:
                st = sim.frame_state64(body, -1, com=False)
                cache[key] = (quat_mat(st[:, 3:7]), st[:, 0:3].astype(np.float64))
            else:
                gf = int(np.nonzero((self.FI[:, K.FI_BODY] == body) & (self.FI[:, K.FI_LINK] == glink))[0][0])
                st = sim.frame_state64(body, self._local_frame(body, gf), com=False)
                Rf, pf = quat_mat(st[:, 3:7]), st[:, 0:3].astype(np.float64)
                Ro, off = quat_mat(self.FF[gf, K.FF_QUAT:K.FF_QUAT + 4]), self.FF[gf, K.FF_POS:K.FF_POS + 3]
                Rl = Rf @ Ro.T   # frame = link * offset
                cache[key] = (Rl, pf - Rl @ off)
        return cache[key]

    def shape_poses(self, sim):
        """Per shape: (R [B,3,3], p [B,3]) of the shape frame and (Rl, pl) of the frame its hull planes live in."""
        B, cache, out = sim.num_envs, {}, []
        for k in range(self.nsh):
            si, sf = self.SI[k], self.SF[k]
            if si[K.SI_FLAGS] & K.SHAPE_WORLD:
                Rl, pl = np.broadcast_to(np.eye(3), (B, 3, 3)), np.zeros((B, 3))
            else:
                Rl, pl = self.link_pose(sim, int(si[K.SI_BODY]), int(si[K.SI_LINK]), cache)
            Rs = sf[K.SF_ROT:K.SF_ROT + 9].reshape(3, 3)
            out.append((Rl @ Rs, pl + Rl @ sf[K.SF_POS:K.SF_POS + 3], Rl, pl))
        return out

    # ---- the caster --------------------------------------------------------------------------------------------------
    def cast(self, sim, ray_from, ray_to, body=-1, frame=-1, skip_body=-1, cull=False):
        """``ray_from`` / ``ray_to``: [N, 3] or [B, N, 3]; ``body`` / ``frame``: a body index and its local frame (-1: base), as
        ``dg_world_raycast`` takes them.  Returns a dict of fp64 / int arrays: frac [B, N], id, shape, pos [B, N, 3], normal,
        margin [B, N] (metres), length [B, N] (|to - from|, world).  ``cull``: a shape is only tested by the rays whose segment comes
        within 1.01 x + 1e-4 m of its bounding sphere -- the kernel's reject restated, to check that it drops nothing."""
        B = sim.num_envs
        a = np.broadcast_to(np.asarray(ray_from, dtype=np.float64), (B, ) + tuple(np.shape(ray_from)[-2:])).copy()
        b = np.broadcast_to(np.asarray(ray_to, dtype=np.float64), a.shape).copy()
        if body >= 0:
            st = sim.frame_state64(body, frame, com=frame < 0)
            Rm, pm = quat_mat(st[:, 3:7]), st[:, 0:3].astype(np.float64)
            a = pm[:, None, :] + a @ Rm.transpose(0, 2, 1)
            b = pm[:, None, :] + b @ Rm.transpose(0, 2, 1)
        o, d = a, b - a
        N = o.shape[1]
        length = np.linalg.norm(d, axis=-1)
        live = length > 0
        best = np.ones((B, N)); shape = np.full((B, N), -1, dtype=np.int64); normal = np.zeros((B, N, 3)); margin = np.full((B, N), np.inf)

        reach = [live]

        def take(ok, t, n, mg, k):
            ok = ok & reach[0] & (t >= 0) & (t < best)
            best[ok] = t[ok]; shape[ok] = k; normal[ok] = n[ok]; margin[ok] = mg[ok]

        def sphere(c, r, k, accept=None):
            oc = o - c[:, None, :]
            A, Bq, C = (d * d).sum(-1), (oc * d).sum(-1), (oc * oc).sum(-1) - r * r
            disc = Bq * Bq - A * C
            with np.errstate(all='ignore'):
                t = (-Bq - np.sqrt(np.where(disc >= 0, disc, 0))) / A
                n = ((o + d * t[..., None]) - c[:, None, :]) / r
            take((disc >= 0) & (True if accept is None else accept(o + d * t[..., None])), t, n, np.full((B, N), np.inf), k)

        with np.errstate(all='ignore'):
            for k, (R, p, Rl, pl) in enumerate(self.shape_poses(sim)):
                si, prm = self.SI[k], self.SF[k, K.SF_PARAMS:K.SF_PARAMS + 3]
                if si[K.SI_BODY] == skip_body:
                    continue
                typ = int(si[K.SI_TYPE])
                reach[0] = live
                if cull:
                    bound = {K.SHAPE_SPHERE: prm[0], K.SHAPE_BOX: float(np.linalg.norm(prm)), K.SHAPE_CAPSULE: prm[0] + prm[1], K.SHAPE_POINTS: prm[2]}[typ]   # (hull: the sphere around the shape's origin that contains its points)
                    oc = p[:, None, :] - o
                    tc = np.clip((oc * d).sum(-1) / (d * d).sum(-1), 0.0, 1.0); q = oc - d * tc[..., None]
                    reach[0] = live & ((q * q).sum(-1) <= (bound * 1.01 + 1e-4) ** 2)
                if typ == K.SHAPE_SPHERE:
                    sphere(p, prm[0], k)
                elif typ == K.SHAPE_CAPSULE:
                    axis = R[:, :, 2] * prm[1]; e0, e1 = p - axis, p + axis; ax = e1 - e0; L2 = (ax * ax).sum(-1)[:, None]
                    oc = o - e0[:, None, :]; dax = (d * ax[:, None, :]).sum(-1); oax = (oc * ax[:, None, :]).sum(-1)
                    A = (d * d).sum(-1) - dax * dax / L2; Bq = (oc * d).sum(-1) - oax * dax / L2; C = (oc * oc).sum(-1) - oax * oax / L2 - prm[0] ** 2
                    disc = Bq * Bq - A * C
                    t = (-Bq - np.sqrt(np.where(disc >= 0, disc, 0))) / A; s = (oax + t * dax) / L2
                    n = ((o + d * t[..., None]) - (e0[:, None, :] + ax[:, None, :] * s[..., None])) / prm[0]
                    take((L2 > 1e-24) & (A > 1e-24) & (disc >= 0) & (s >= 0) & (s <= 1), t, n, np.full((B, N), np.inf), k)
                    # an end sphere counts where it is the capsule's surface: beyond its end of the axis segment (elsewhere its
                    # surface lies inside the solid: a ray that starts inside the cylinder would "enter" it there)
                    sax = lambda x: ((x - e0[:, None, :]) * ax[:, None, :]).sum(-1) / L2
                    degenerate = ~(L2 > 1e-24)
                    sphere(e0, prm[0], k, lambda x: degenerate | (sax(x) < 0)); sphere(e1, prm[0], k, lambda x: degenerate | (sax(x) > 1))
                else:
                    if typ == K.SHAPE_BOX:   # six face planes n . x + dd <= 0 in the shape frame
                        Rf, pf = R, p
                        planes = np.array([[s if a_ == ax_ else 0.0 for a_ in range(3)] + [-prm[ax_]] for ax_ in range(3) for s in (1.0, -1.0)])
                    else:
                        Rf, pf = Rl, pl
                        planes = self.PLN[4 * si[K.SI_PLANE_OFF]:4 * (si[K.SI_PLANE_OFF] + si[K.SI_N_PLANES])].reshape(-1, 4)
                    if len(planes) == 0:
                        continue
                    ol = (o - pf[:, None, :]) @ Rf; dl = d @ Rf   # (R^T v, batched)
                    den = dl @ planes[:, :3].T; dist = ol @ planes[:, :3].T + planes[:, 3]   # [B, N, np]
                    par = np.abs(den) < TINY
                    miss = (par & (dist > 0)).any(-1)
                    t = -dist / den
                    ent = np.where(~par & (den < 0), t, -np.inf); ext = np.where(~par & (den > 0), t, np.inf)
                    kn = ent.argmax(-1); tn = np.take_along_axis(ent, kn[..., None], -1)[..., 0]; tf = ext.min(-1)
                    ent2 = ent.copy(); np.put_along_axis(ent2, kn[..., None], -np.inf, -1)
                    mg = (tn - ent2.max(-1)) * length
                    n = planes[kn, :3] @ Rf.transpose(0, 2, 1)
                    take(~miss & ~(tn > tf), tn, n, mg, k)
        hit = shape >= 0
        frac = np.where(hit, best, 1.0)
        return dict(frac=frac, shape=shape, id=np.where(hit, self.seg[np.maximum(shape, 0)], -1).astype(np.int32),
                    pos=np.where(hit[..., None], o + d * frac[..., None], b), normal=normal, margin=np.where(hit, margin, np.inf), length=length)


class RaycastOracleBackend(OracleBackend):
    """The oracle plus a numpy ``ray_test_batch`` (CPU tensors): what the ``lidar`` addon needs to run in host tests."""
    def ray_test_batch(self, ray_from, ray_to, body=-1, frame=-1, skip_body=-1, want=('frac', 'id', 'pos', 'normal')):
        if body >= 0:
            body, frame = self.layout.resolve_frame(body, frame)
        if skip_body >= 0:
            skip_body = self.layout.resolve_frame(skip_body, -1)[0]
        if not hasattr(self, '_ray_ref'):
            self._ray_ref = RaycastRef(self.layout)
        r = self.last_ray64 = self._ray_ref.cast(self, ray_from.detach().cpu().numpy(), ray_to.detach().cpu().numpy(), int(body), int(frame), int(skip_body))
        return RayHits(torch.from_numpy(r['frac']).float(), torch.from_numpy(r['id']) if 'id' in want else None,
                       torch.from_numpy(r['pos']).float() if 'pos' in want else None, torch.from_numpy(r['normal']).float() if 'normal' in want else None)


# ---- the cases the GPU tests run (tests/test_raycast_gpu.py) and the CPU file checks the edge-ray cap of -------------------
BASIC = os.path.join(ROOT, 'tests', 'golden', 'basic_env.yaml')
SCENES = {
    # name: (config, model the mounted rays ride on, its frame, box the world rays live in: (lo, hi))
    'basic_env': (BASIC, 'green_marble', None, ([-2.5, -2.5, 0.05], [2.5, 2.5, 2.5])),
    'from_the_readme': (os.path.join(ROOT, 'examples', 'from_the_readme', 'from_the_readme.yaml'), 'r2d2', 'left_tip_joint', ([-1.5, -1.5, 0.05], [1.5, 1.5, 2.0])),
    'r2d2_maze': (os.path.join(ROOT, 'examples', 'r2d2_maze', 'r2d2_maze.yaml'), 'r2d2', 'head_swivel', ([-5.5, -5.5, 0.05], [5.5, 5.5, 1.5])),
}
CASES = [('basic_env', 3), ('basic_env', 70), ('from_the_readme', 3), ('from_the_readme', 70), ('r2d2_maze', 1), ('r2d2_maze', 3), ('r2d2_maze', 70)]
RAY_COUNTS = (1, 63, 64, 65, 130)
STEPS = 20
SEED = 0   # of the ray sets


def case_backend():
    """The oracle backend the cases are stepped on: the OpenMP build of the same fp64 source where it exists (envs are
    independent, so the states are the serial build's; from_the_readme x 70 envs x 20 steps: 13 s serial)."""
    from oracle_backend import FLAVOURS
    path = os.path.join(ROOT, 'oracle', FLAVOURS['f64_omp'])
    return type('RaycastOracleBackend_omp', (RaycastOracleBackend, ), {'lib_path': path}) if os.path.isfile(path) else RaycastOracleBackend


def make_env(scene, B, **kw):
    import yaml
    import diy_gym_amd.examples  # noqa: F401
    from diy_gym_amd import DIYGym
    from diy_gym_amd.config import Configuration
    tree = yaml.safe_load(open(SCENES[scene][0]))
    # (without the scene's cameras: they play no part in the physics, and the oracle renders them at every reset)
    tree = {k: ({a: b for a, b in v.items() if not (isinstance(b, dict) and b.get('addon') == 'camera')} if isinstance(v, dict) else v)
            for k, v in tree.items() if not (isinstance(v, dict) and v.get('addon') == 'camera')}
    return DIYGym(Configuration.from_dict(scene, copy.deepcopy(tree)), num_envs=B, seed=2, **kw)


def actions(env, steps=STEPS, seed=0):
    """The random actions every backend of a case is stepped with: uniform over the action space, [steps][B, act_dim]."""
    from diy_gym_amd.utils import flatten, get_bounds_for_space
    lo = torch.as_tensor(flatten(get_bounds_for_space(env.action_space, True)), dtype=torch.float32)
    hi = torch.as_tensor(flatten(get_bounds_for_space(env.action_space, False)), dtype=torch.float32)
    lo, hi = torch.nan_to_num(lo, neginf=-1.0).clamp(-10, 10), torch.nan_to_num(hi, posinf=1.0).clamp(-10, 10)
    gen = torch.Generator().manual_seed(seed)
    return [lo + (hi - lo) * torch.rand((env.num_envs, lo.numel()), generator=gen) for _ in range(steps)]


def advance(env, acts):
    for a in acts:
        env.sim.step(env._all_slots, a.to(env.device))
    env._tick += 1


FORMS = ('world_shared', 'world_per_env', 'mounted_shared', 'mounted_per_env')
# ray sets whose seed-0 draw exceeds the edge-ray cap of tests/test_raycast.py (the Jaco arm's hulls are round meshes of
# millimetre facets: most hits on them are edge rays) and the seed that replaces it
SEED_OVERRIDES = {
    ('from_the_readme', 3, 63, 'world_per_env'): 3,
    ('from_the_readme', 3, 64, 'mounted_shared'): 1,
    ('from_the_readme', 3, 65, 'world_shared'): 1,
    ('from_the_readme', 70, 1, 'world_per_env'): 1,
    ('from_the_readme', 70, 63, 'mounted_shared'): 1,
    ('from_the_readme', 70, 130, 'world_shared'): 1,
}


def ray_sets(scene, B, n):
    """The seeded ray sets of one (scene, batch, ray count): form -> (ray_from, ray_to, mounted), float32 arrays.  World rays
    start and end inside the scene's box; mounted rays leave a point within 0.3 m of the link frame's origin in a random
    direction, 0.5 - 4 m long."""
    lo, hi = (np.asarray(v) for v in SCENES[scene][3])
    out = {}
    for f, form in enumerate(FORMS):
        rng = np.random.default_rng([SEED_OVERRIDES.get((scene, B, n, form), SEED), sorted(SCENES).index(scene), B, n, f])
        lead = (B, n) if form.endswith('per_env') else (n, )
        if form.startswith('world'):
            a = lo + (hi - lo) * rng.random(lead + (3, ))
            b = lo + (hi - lo) * rng.random(lead + (3, )); b[..., 2] = -0.5 + 1.5 * rng.random(lead)   # most of them come down to the floor
        else:
            a = (rng.random(lead + (3, )) - 0.5) * 0.6
            v = rng.normal(size=lead + (3, )); v /= np.linalg.norm(v, axis=-1, keepdims=True)
            b = a + v * (0.5 + 3.5 * rng.random(lead + (1, )))
        out[form] = (a.astype(np.float32), b.astype(np.float32), form.startswith('mounted'))
    return out


def mount_of(env, scene):
    """(uid, frame id) the mounted rays of ``scene`` are given in."""
    model = env.models[SCENES[scene][1]]
    return model.uid, (model.get_frame_id(SCENES[scene][2]) if SCENES[scene][2] else -1)


def pixel_rays(layout, camera):
    """Pixel-centre rays of camera ``camera`` in its PARENT frame, by the oracle's convention (dgo_render): direction
    T_parent_cam (xn tan aspect, yn tan, -1) with xn = 2 (col + 1/2) / W - 1, yn = 1 - 2 (row + 1/2) / H, from the near to the
    far distance: eye-space depth = -(near + frac (far - near)).  Returns (body, local frame, from [H W, 3], to, near, far)."""
    I, F = layout.I, layout.F
    ci = I[I[K.H_OFF_CAMERA_I] + camera * K.CI_STRIDE:][:K.CI_STRIDE]; cf = F[I[K.H_OFF_CAMERA_F] + camera * K.CF_STRIDE:][:K.CF_STRIDE]
    W, H, zn, zf = int(ci[K.CI_WIDTH]), int(ci[K.CI_HEIGHT]), float(cf[K.CF_NEAR]), float(cf[K.CF_FAR])
    th = np.tan(0.5 * cf[K.CF_FOV] * np.pi / 180.0); aspect = W / H
    row, col = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    xn, yn = ((col + 0.5) / W) * 2.0 - 1.0, 1.0 - ((row + 0.5) / H) * 2.0
    d = np.stack([xn * th * aspect, yn * th, -np.ones_like(xn)], -1).reshape(-1, 3) @ quat_mat(cf[K.CF_QUAT:K.CF_QUAT + 4]).T
    pc = cf[K.CF_POS:K.CF_POS + 3]
    body, gf = int(ci[K.CI_BODY]), int(ci[K.CI_FRAME])
    frame = -1 if gf < 0 else RaycastRef(layout)._local_frame(body, gf)
    return body, frame, pc + d * zn, pc + d * zf, zn, zf
