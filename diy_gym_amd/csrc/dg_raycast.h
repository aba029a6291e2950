// dg_raycast.h -- batched ray casting against the collision geometry (pybullet's p.rayTest / p.rayTestBatch; the reference never
// calls either -- this is the world query behind the `lidar` addon and env.sim.ray_test_batch).
//
// Two launches per call:
//   pose_kernel     (dg_render.h) with one mount row: world frame + bounding sphere of every shape and the world pose of the frame
//                   the rays are given in -> the caller's scratch, per env [nsh][RS_STRIDE] + [RC_STRIDE];
//   raycast_kernel  one workgroup per (env, chunk of rays), one ray per lane.  The env's shape rows -- pose, bounding sphere,
//                   parameters, type, segmentation value: RY_STRIDE words each, the colours of the render table left out -- are
//                   staged into LDS once per workgroup and every lane then walks the shapes IN SHAPE ORDER (ties between
//                   coincident surfaces go to the lower shape index, as in render_band_slow): one ballot rejects a shape whose
//                   bounding sphere no ray of the wavefront reaches, the lanes whose own ray reaches it intersect it with the
//                   ray_* functions of dg_render.h (d = to - from, tmin = 0, h.t = 1: t is the hit fraction).  Hull face planes
//                   come through wave-uniform loads as in render_band_slow.
// A scene whose rows do not fit the LDS budget (DG_RAY_LDS_WORDS) runs the same loop with the rows read through wave-uniform
// loads from the table and the scene arrays: the same values into the same arithmetic, so the same bits out.
// What bounds it: a lidar's output is 4-32 B per ray, so unlike the camera this path is bound by instruction issue (the shape
// loop), not by HBM writes.
#pragma once
#include "dg_render.h"

namespace dg {

#define DG_RAY_LDS_WORDS 12288  /* 48 KiB of staged rows: 512 shapes */
// a staged row: every group of words a lane reads together starts on a 16-byte boundary (a wide LDS read off its alignment is replayed)
enum { RY_R = 0 /* 9 */, RY_C = 12 /* centre 3, bounding radius */, RY_P = 16 /* 3 */, RY_META = 19 /* type | 4 if no ray can hit it (skip_body) */, RY_PRM = 20 /* 3 */, RY_SEG = 23, RY_STRIDE = 24 };

static_assert(RS_BOUND == RS_C + 3, "the staged row copies centre and bounding radius as one group");

template <bool LDS>
__global__ __launch_bounds__(256) void raycast_kernel(DevScene sc, cfp PLN, cfp table, int n_rays, int nchunks, const float* ray_from, const float* ray_to,
                                                       int per_env, int mounted, int skip_body, int no_cull /* diagnostic: every ray against every shape */, float* frac, int32_t* id, float* pos, float* normal) {
  extern __shared__ __attribute__((aligned(16))) float s_ray[];
  const int env = blockIdx.x / nchunks, chunk = blockIdx.x - env * nchunks, tid = threadIdx.x, nth = blockDim.x;
  const int nsh = sc.nsh;
  cfp tb = table + (size_t)env * (nsh * RS_STRIDE + RC_STRIDE);
  auto meta_of = [&](int k) { cip si = sc.SI + k * DG_SI_STRIDE; return si[DG_SI_TYPE] | (si[DG_SI_BODY] == skip_body ? 4 : 0); };
  auto seg_of = [&](int k) { cip si = sc.SI + k * DG_SI_STRIDE; return si[DG_SI_BODY] + (((si[DG_SI_FLAGS] >> 8) & 0xFFFF) << 24); };
  if constexpr (LDS) {
    for (int w = tid; w < nsh * RY_STRIDE; w += nth) {
      const int k = w / RY_STRIDE, j = w - k * RY_STRIDE; float v;
      if (j < 9) v = tb[k * RS_STRIDE + RS_R + j];
      else if (j < RY_C) v = 0.f;
      else if (j < RY_P) {  // (RS_BOUND follows RS_C)
        // a hull's RS_BOUND is its FITTED capsule's reach, which lets points near the caps stick out (fine for the render, whose
        // near plane and cone tests stand behind it); the sphere that contains every point is DG_SF_PARAMS + 2
        const bool hull_bound = j == RY_C + 3 && sc.SI[k * DG_SI_STRIDE + DG_SI_TYPE] == DG_SHAPE_POINTS;
        v = hull_bound ? sc.SF[k * DG_SF_STRIDE + DG_SF_PARAMS + 2] : tb[k * RS_STRIDE + RS_C + (j - RY_C)];
      }
      else if (j < RY_META) v = tb[k * RS_STRIDE + RS_P + (j - RY_P)];
      else if (j == RY_META) v = __int_as_float(meta_of(k));
      else if (j < RY_SEG) v = sc.SF[k * DG_SF_STRIDE + DG_SF_PARAMS + (j - RY_PRM)];
      else v = __int_as_float(seg_of(k));
      s_ray[w] = v;
    }
    __syncthreads();
  }
  const int ray = chunk * nth + tid; const bool have = ray < n_rays;
  if (!__any(have)) return;  // (a wavefront of the last chunk's tail; nothing below synchronises the workgroup)
  const int r = have ? ray : n_rays - 1;
  const size_t ri = (per_env ? (size_t)env * n_rays : (size_t)0) + r;
  V3 a = v3(ray_from[3 * ri], ray_from[3 * ri + 1], ray_from[3 * ri + 2]), b = v3(ray_to[3 * ri], ray_to[3 * ri + 1], ray_to[3 * ri + 2]);
  if (mounted) {
    cfp m = tb + nsh * RS_STRIDE; M3 Rm; _Pragma("unroll") for (int q = 0; q < 9; q++) Rm.m[q] = m[q];
    const V3 pm = v3(m[9], m[10], m[11]); a = pm + mul(Rm, a); b = pm + mul(Rm, b);
  }
  const V3 o = a, d = b - a; const float dd = dot(d, d);
  const bool live = have && dd > 0.f;  // a zero-length ray hits nothing
  const float idd = live ? __frcp_rn(dd) : 0.f;
  RayHit h; h.t = 1.f; h.shape = -1; h.n = v3(0.f, 0.f, 0.f); h.tmin = 0.f;
  for (int k = 0; k < nsh; k++) {
    V3 c; float bound; int meta;
    if constexpr (LDS) { const float* e = s_ray + k * RY_STRIDE; c = v3(e[RY_C], e[RY_C + 1], e[RY_C + 2]); bound = e[RY_C + 3]; meta = __float_as_int(e[RY_META]); }
    else {
      cfp e = tb + k * RS_STRIDE; c = v3(e[RS_C], e[RS_C + 1], e[RS_C + 2]); meta = meta_of(k);
      bound = (meta & 3) == DG_SHAPE_POINTS ? sc.SF[k * DG_SF_STRIDE + DG_SF_PARAMS + 2] : e[RS_BOUND];
    }
    if (meta & 4) continue;
    // the segment's point nearest the shape's centre against its bounding sphere, a hair wider (1 % + 0.1 mm: a box's sphere touches
    // its corners and a thinned hull's face planes reach a hair beyond the sphere around its points)
    const V3 oc = c - o; const float tc = fminf(fmaxf(dot(oc, d) * idd, 0.f), 1.f); const V3 qv = oc - d * tc;
    const float bw = bound * 1.01f + 1e-4f; const bool reach = live && (no_cull || dot(qv, qv) <= bw * bw);
    if (!__any(reach)) continue;  // no ray of the wavefront reaches it
    M3 R; V3 p; float p0, p1, p2;
    if constexpr (LDS) {
      const float* e = s_ray + k * RY_STRIDE;
      _Pragma("unroll") for (int q = 0; q < 9; q++) R.m[q] = e[RY_R + q];
      p = v3(e[RY_P], e[RY_P + 1], e[RY_P + 2]); p0 = e[RY_PRM]; p1 = e[RY_PRM + 1]; p2 = e[RY_PRM + 2];
    } else {
      cfp e = tb + k * RS_STRIDE; cfp sf = sc.SF + k * DG_SF_STRIDE + DG_SF_PARAMS;
      _Pragma("unroll") for (int q = 0; q < 9; q++) R.m[q] = e[RS_R + q];
      p = v3(e[RS_P], e[RS_P + 1], e[RS_P + 2]); p0 = sf[0]; p1 = sf[1]; p2 = sf[2];
    }
    if (!reach) continue;  // this lane's ray passes it by
    const int type = meta & 3;
    if (type == DG_SHAPE_SPHERE) ray_sphere(o, d, p, p0, h, k);
    else if (type == DG_SHAPE_BOX) ray_box(o, d, R, p, p0, p1, p2, h, k);
    else if (type == DG_SHAPE_CAPSULE) {
      // ray_capsule takes the earliest of the cylinder's and the two end spheres' entries: the capsule's entry for a ray that starts
      // outside it.  One that starts INSIDE (nearer the axis segment than r) would be given the point where it enters an end
      // sphere from within the cylinder -- the render clips that away at its near plane, a world query has no such clip
      const V3 ax = v3(R.m[2], R.m[5], R.m[8]) * p1, e0 = p - ax, w0 = o - e0, a2 = ax * 2.f; const float L2 = dot(a2, a2);
      const float sp = L2 > 1e-24f ? fminf(fmaxf(fdiv(dot(w0, a2), L2), 0.f), 1.f) : 0.f; const V3 off = w0 - a2 * sp;
      if (!(dot(off, off) < p0 * p0)) ray_capsule(o, d, e0, p + ax, p0, h, k);
    }
    else { cip si = sc.SI + k * DG_SI_STRIDE; ray_hull(o, d, R, p, PLN + 4 * si[DG_SI_PLANE_OFF], si[DG_SI_N_PLANES], h, k); }
  }
  if (!have) return;
  const bool hit = h.shape >= 0; const size_t oi = (size_t)env * n_rays + ray;
  frac[oi] = hit ? h.t : 1.f;
  if (id) { int v = -1; if (hit) { if constexpr (LDS) v = __float_as_int(s_ray[h.shape * RY_STRIDE + RY_SEG]); else v = seg_of(h.shape); } id[oi] = v; }
  if (pos) { const V3 x = hit ? o + d * h.t : b; pos[3 * oi] = x.x; pos[3 * oi + 1] = x.y; pos[3 * oi + 2] = x.z; }
  if (normal) { const V3 n = hit ? h.n : v3(0.f, 0.f, 0.f); normal[3 * oi] = n.x; normal[3 * oi + 1] = n.y; normal[3 * oi + 2] = n.z; }
}

}  // namespace dg
