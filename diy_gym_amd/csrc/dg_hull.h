// dg_hull.h -- convex hull against convex hull (DG_HF_HULL_CONTACTS): what pybullet does with two URDF collision meshes
// (reference model.py:65 loadURDF -> Bullet's btConvexConvexAlgorithm on the meshes' convex hulls [R]).
//
//   C = A - B (Minkowski difference), support s_C(d) = s_A(d) - s_B(-d), the hull points read through wave-uniform addresses
//   (both hulls of a candidate pair are the same in every lane; the poses differ);
//   GJK: closest point v of C to the origin over a simplex of <= 4 support points (Voronoi-region tests of Ericson, Real-Time
//        Collision Detection 5.1.5 / 5.1.6): distance |v|, normal v / |v| (from B towards A), witness points from the
//        barycentric weights; a lane leaves as soon as v . w / |v| -- a lower bound of its distance -- exceeds what it asks for;
//   EPA: origin inside C or nearer than HH_SWITCH: an expanding polytope inside C with SIGNED plane distances of the origin, started
//        from a tetrahedron of four support points of its own; the face with the smallest distance is pushed out to its support point
//        until it is a face of C.  Its vertices, faces and horizon edges are arrays with per-lane sizes and indices in a device
//        buffer of the world: the rare, slow part -- only lanes whose hulls interpenetrate beyond their 2 x 1 mm of margin get here.
// Same steps, same constants, same tie-breaks (strict comparisons, lowest index first) as the CPU checker's hull_hull (the tests
// compare the two, and both with a brute-force Minkowski difference); coordinates are relative to A's frame origin.  The simplex of the GJK part lives in registers: every index into it
// is a compile-time constant, a run-time position is a chain of selects.
#pragma once
#include "dg_device.h"

namespace dg {

// The two routines are inlined into the narrow phase: as functions of their own (one copy per kernel instead of one per call site)
// they made every step kernel a kernel WITH CALLS -- stack pointer and scratch descriptor reserved, a different register
// allocation throughout -- and the contact-free headline scene, which never enters them, ran 25 % slower in every section.
#ifndef HH_FN
#define HH_FN DGD
#endif
#define HH_GJK_ITERS 32
#define HH_EPA_ITERS 24
#define HH_EPA_MAXV (4 + HH_EPA_ITERS)
#define HH_EPA_MAXF (2 * HH_EPA_MAXV)
#define HH_EPA_MAXE 96
#define HH_FACE_PTS 8
#define HH_SWITCH 1e-4f

// compile-time loop: every index into the simplex arrays below must be a constant or the arrays land in scratch memory (a
// `#pragma unroll` the optimizer declines leaves run-time indices behind -- it did, inside the GJK loop: 800 bytes of scratch per
// lane and, worse, a different spilling strategy for the whole kernel)
template <int I, int N, class F> DGD void hh_for(F&& f) { if constexpr (I < N) { f(std::integral_constant<int, I>{}); hh_for<I + 1, N>(f); } }
typedef const float __attribute__((address_space(4)))* hh_cfp;
// tabled: lane k of the wavefront holds hull point k of A in (tax, tay, taz) and of B in (tbx, tby, tbz) -- loaded once per pair with
// every lane active (hull_tables); the support loops then read a point with three v_readlane instead of a scalar load whose
// round trip to the scalar cache a lone wavefront cannot hide (32 + 32 dependent loads per support: 25 k cycles, measured as
// 11 x the step time of arms in contact).  Not tabled (the reset kernel steps under a per-env mask; hulls of more points than
// active lanes): the points come through wave-uniform scalar loads.
struct HullPairD { hh_cfp pa, pb; int na, nb; M3 RA, RB; V3 tBA; float tax, tay, taz, tbx, tby, tbz; bool tabled; float* ew /* this lane's column of its wavefront's polytope workspace (hull_ws_of) */; };
DGD void hull_tables(HullPairD& h, bool tabled) {
  const int lane = threadIdx.x & 63; h.tabled = tabled; h.tax = h.tay = h.taz = h.tbx = h.tby = h.tbz = 0.f;
  if (tabled) {
    const int ka = min(lane, h.na - 1), kb = min(lane, h.nb - 1);
    h.tax = h.pa[3 * ka]; h.tay = h.pa[3 * ka + 1]; h.taz = h.pa[3 * ka + 2]; h.tbx = h.pb[3 * kb]; h.tby = h.pb[3 * kb + 1]; h.tbz = h.pb[3 * kb + 2];
  }
}
struct HullHit { V3 pa, pb, n; float dist; bool hit; int iters /* GJK iterations this lane needed (diagnostics) */; };
struct HV { V3 w, a, b; int id; };
// component-wise selects: `c ? a : b` on two structs selects between their ADDRESSES, which keeps both (and every array one of them
// is an element of) in scratch memory -- the simplex arrays of the GJK loop were, 84 scratch round trips per iteration: 28 k cycles
// an iteration instead of 7 k
DGD V3 hh_sel(bool c, V3 a, V3 b) { return v3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }
DGD HV hh_sel(bool c, const HV& a, const HV& b) { HV r; r.w = hh_sel(c, a.w, b.w); r.a = hh_sel(c, a.a, b.a); r.b = hh_sel(c, a.b, b.b); r.id = c ? a.id : b.id; return r; }

// (four points per round, their loads in flight together)
DGD int hh_argmax(hh_cfp p, int n, V3 d, V3& pt) {
  int bi = 0; float best = -3.0e38f; V3 bp = v3(0.f, 0.f, 0.f);
  for (int k0 = 0; k0 < n; k0 += 4) {
    float q[4][3];
#pragma unroll
    for (int j = 0; j < 4; j++) { const int k = min(k0 + j, n - 1); q[j][0] = p[3 * k]; q[j][1] = p[3 * k + 1]; q[j][2] = p[3 * k + 2]; }
#pragma unroll
    for (int j = 0; j < 4; j++) {  // (a round's spare slots repeat the last point: never strictly better)
      const float sd = q[j][0] * d.x + q[j][1] * d.y + q[j][2] * d.z; const bool g = sd > best;
      best = g ? sd : best; bi = g ? min(k0 + j, n - 1) : bi; bp.x = g ? q[j][0] : bp.x; bp.y = g ? q[j][1] : bp.y; bp.z = g ? q[j][2] : bp.z;
    }
  }
  pt = bp; return bi;
}
DGD int hh_argmax_tab(float tx, float ty, float tz, int n, V3 d, V3& pt) {
  // (the loop carries the best index only; the point itself is fetched afterwards with three ds_bpermute from the lane tables --
  // every lane of the wavefront is active here, the GJK loop is wave-uniform)
  int bi = 0; float best = -3.0e38f;
  auto rl = [](float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); };
  for (int k = 0; k < n; k++) {
    const float x = rl(tx, k), y = rl(ty, k), z = rl(tz, k), sd = x * d.x + y * d.y + z * d.z; const bool g = sd > best;
    best = g ? sd : best; bi = g ? k : bi;
  }
  pt = v3(__shfl(tx, bi), __shfl(ty, bi), __shfl(tz, bi)); return bi;
}
template <bool TAB = true>
DGD HV hh_support(const HullPairD& h, V3 d) {
  HV o; V3 qa, qb; int ia, ib;
  if (TAB && h.tabled) { ia = hh_argmax_tab(h.tax, h.tay, h.taz, h.na, tmul(h.RA, d), qa); ib = hh_argmax_tab(h.tbx, h.tby, h.tbz, h.nb, tmul(h.RB, -d), qb); }
  else { ia = hh_argmax(h.pa, h.na, tmul(h.RA, d), qa); ib = hh_argmax(h.pb, h.nb, tmul(h.RB, -d), qb); }
  o.a = mul(h.RA, qa); o.b = mul(h.RB, qb) + h.tBA; o.w = o.a - o.b; o.id = (ia << 8) | ib; return o;
}
// barycentric weights of the point of triangle (a, b, c) closest to the origin (Ericson 5.1.5)
DGD void hh_closest_tri(V3 a, V3 b, V3 c, float (&l)[3]) {
  const V3 ab = b - a, ac = c - a;
  const float d1 = -dot(ab, a), d2 = -dot(ac, a);
  l[0] = l[1] = l[2] = 0.f;
  if (d1 <= 0.f && d2 <= 0.f) { l[0] = 1.f; return; }
  const float d3 = -dot(ab, b), d4 = -dot(ac, b);
  if (d3 >= 0.f && d4 <= d3) { l[1] = 1.f; return; }
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { const float t = fdiv(d1, d1 - d3); l[0] = 1.f - t; l[1] = t; return; }
  const float d5 = -dot(ab, c), d6 = -dot(ac, c);
  if (d6 >= 0.f && d5 <= d6) { l[2] = 1.f; return; }
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { const float t = fdiv(d2, d2 - d6); l[0] = 1.f - t; l[2] = t; return; }
  const float va = d3 * d6 - d5 * d4;
  if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) { const float t = fdiv(d4 - d3, (d4 - d3) + (d5 - d6)); l[1] = 1.f - t; l[2] = t; return; }
  const float den = frcp(va + vb + vc); l[1] = vb * den; l[2] = vc * den; l[0] = 1.f - l[1] - l[2];
}
// point of the simplex (n vertices, in slots 0 .. n - 1) closest to the origin: weights l; true: the origin is inside a tetrahedron
DGD bool hh_closest_simplex(const V3 (&w)[4], int n, float (&l)[4]) {
  l[0] = l[1] = l[2] = l[3] = 0.f;
  if (n == 1) { l[0] = 1.f; return false; }
  if (n == 2) {
    const V3 ab = w[1] - w[0]; const float den = dot(ab, ab); float t = den > 0.f ? fdiv(-dot(w[0], ab), den) : 0.f;
    t = fminf(fmaxf(t, 0.f), 1.f); l[0] = 1.f - t; l[1] = t; return false;
  }
  if (n == 3) { float lt[3]; hh_closest_tri(w[0], w[1], w[2], lt); l[0] = lt[0]; l[1] = lt[1]; l[2] = lt[2]; return false; }
  // tetrahedron (Ericson 5.1.6): the faces that have the origin on their outer side (a flat tetrahedron: every face)
  float best = 3.0e38f; bool inside = true;
  hh_for<0, 4>([&](auto FI) {
    constexpr int f = decltype(FI)::value;
    constexpr int F[4][4] = {{0, 1, 2, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {1, 3, 2, 0}};
    const V3 a = w[F[f][0]], b = w[F[f][1]], c = w[F[f][2]], d = w[F[f][3]];
    const V3 nn = cross(b - a, c - a);
    const float sp = -dot(a, nn), sd = dot(d - a, nn), scale = dot(nn, nn) * dot(d - a, d - a);
    const bool flat = sd * sd <= 1e-10f * scale, outside = flat || sp * sd < 0.f;
    if (outside) {
      inside = false;
      float lt[3]; hh_closest_tri(a, b, c, lt);
      const V3 q = a * lt[0] + b * lt[1] + c * lt[2]; const float qq = dot(q, q);
      if (qq < best) { best = qq; l[0] = l[1] = l[2] = l[3] = 0.f; l[F[f][0]] = lt[0]; l[F[f][1]] = lt[1]; l[F[f][2]] = lt[2]; }
    }
  });
  return inside;
}

// ---- the expanding polytope.  Its vertices, faces and horizon edges are arrays with per-lane sizes and indices: they live in a
// device buffer the world owns (DevScene::hull_ws), one block of HH_WS_SLOTS x 64 floats per wavefront of the step grid laid out
// [slot][lane] -- as private arrays they made every step kernel carry 3 KB of scratch per lane, and the launch of the contact-free
// headline scene 25 % slower for a routine none of its lanes ever entered.  Called under divergence (only the lanes that
// need it): the support points come through scalar-free loads here, not the lane tables (an inactive lane's table
// registers are not restored around the call).
enum { HW_VW = 0 /* vertex w: 3 x MAXV */, HW_VID = 3 * HH_EPA_MAXV, HW_FV = HW_VID + HH_EPA_MAXV /* face: vertex indices, 8 bits each, bit 24 = alive */,
       HW_FN = HW_FV + HH_EPA_MAXF /* normal: 3 x MAXF */, HW_FD = HW_FN + 3 * HH_EPA_MAXF, HW_ED = HW_FD + HH_EPA_MAXF, HW_PW = HW_ED + HH_EPA_MAXE /* coplanar points: 3 x FACE_PTS */,
       HW_PID = HW_PW + 3 * HH_FACE_PTS, HH_WS_SLOTS = HW_PID + HH_FACE_PTS };
// this lane's column of its wavefront's block
DGD float* hull_ws_of(float* ws) { return ws ? ws + ((size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (size_t)(HH_WS_SLOTS * 64) + (threadIdx.x & 63) : nullptr; }
struct HEpa {
  float* e;
  DGD float& F(int slot) const { return e[slot * 64]; }
  DGD int& I(int slot) const { return reinterpret_cast<int*>(e)[slot * 64]; }
  DGD V3 W(int k) const { return v3(F(HW_VW + 3 * k), F(HW_VW + 3 * k + 1), F(HW_VW + 3 * k + 2)); }
  DGD void put(int k, const HV& s) const { F(HW_VW + 3 * k) = s.w.x; F(HW_VW + 3 * k + 1) = s.w.y; F(HW_VW + 3 * k + 2) = s.w.z; I(HW_VID + k) = s.id; }
  DGD V3 N(int f) const { return v3(F(HW_FN + 3 * f), F(HW_FN + 3 * f + 1), F(HW_FN + 3 * f + 2)); }
  DGD void face(int f, int i, int j, int k, V3 g) const {
    const V3 a = W(i), b = W(j), c = W(k); V3 nn = cross(b - a, c - a); const float len = norm(nn);
    if (!(len > 1e-12f)) { I(HW_FV + f) = i | (j << 8) | (k << 16) | (1 << 24); F(HW_FN + 3 * f) = 0.f; F(HW_FN + 3 * f + 1) = 0.f; F(HW_FN + 3 * f + 2) = 1.f; F(HW_FD + f) = 3.0e38f; return; }  // a sliver: kept for the topology, never the closest
    nn = nn * frcp(len);
    const bool flip = dot(nn, a - g) < 0.f;  // outward: away from the interior point g
    if (flip) nn = -nn;
    I(HW_FV + f) = i | ((flip ? k : j) << 8) | ((flip ? j : k) << 16) | (1 << 24); F(HW_FN + 3 * f) = nn.x; F(HW_FN + 3 * f + 1) = nn.y; F(HW_FN + 3 * f + 2) = nn.z; F(HW_FD + f) = dot(nn, a);
  }
};
// signed distance of the origin from the boundary of C along its nearest face (> 0: inside, the penetration depth), that face's
// outward normal and the witness points of the origin's projection onto it
HH_FN float hh_epa(const HullPairD& h, V3 seed, bool have_start, const V3 (&sw)[4], const int (&sid)[4], V3& n_out, V3& pa, V3& pb) {
  const HEpa E = {h.ew}; int nv = 0, nf = 0;
  // start: the tetrahedron GJK ended with when it found the origin inside one (it already has a face near the origin); else a
  // tetrahedron of C built here: two opposite support points, the one farthest from their line, the one farthest from their plane
  if (have_start) { hh_for<0, 4>([&](auto K) { constexpr int k = decltype(K)::value; HV s; s.w = sw[k]; s.id = sid[k]; s.a = s.w; s.b = s.w; E.put(k, s); }); }
  else {
  const V3 d0 = dot(seed, seed) > 1e-12f ? seed * frsq(dot(seed, seed)) : v3(1.f, 0.f, 0.f);
  const HV s0 = hh_support<false>(h, d0), s1 = hh_support<false>(h, -d0); E.put(0, s0); E.put(1, s1);
  const V3 e = s1.w - s0.w;
  const V3 ax = (fabsf(e.x) <= fabsf(e.y) && fabsf(e.x) <= fabsf(e.z)) ? v3(1.f, 0.f, 0.f) : (fabsf(e.y) <= fabsf(e.z) ? v3(0.f, 1.f, 0.f) : v3(0.f, 0.f, 1.f));
  V3 d1 = cross(e, ax); d1 = d1 * frcp(norm(d1) + 1e-37f);
  { const HV c1 = hh_support<false>(h, d1), c2 = hh_support<false>(h, -d1); E.put(2, hh_sel(fabsf(dot(c1.w - s0.w, d1)) >= fabsf(dot(c2.w - s0.w, d1)), c1, c2)); }
  V3 nn = cross(e, E.W(2) - s0.w); nn = nn * frcp(norm(nn) + 1e-37f);
  { const HV c1 = hh_support<false>(h, nn), c2 = hh_support<false>(h, -nn); E.put(3, hh_sel(fabsf(dot(c1.w - s0.w, nn)) >= fabsf(dot(c2.w - s0.w, nn)), c1, c2)); }
  }
  nv = 4;
  const V3 g = ((E.W(0) + E.W(1)) + (E.W(2) + E.W(3))) * 0.25f;
  E.face(0, 0, 1, 2, g); E.face(1, 0, 1, 3, g); E.face(2, 0, 2, 3, g); E.face(3, 1, 2, 3, g); nf = 4;
  int best = 0;
  for (int it = 0; it < HH_EPA_ITERS; it++) {
    best = -1; float bd = 3.0e38f;
    for (int f0 = 0; f0 < nf; f0 += 4) {  // (four faces per round, their loads issued together: a load at a time is a memory round trip per face)
      float fd4[4]; int fv4[4];
#pragma unroll
      for (int j = 0; j < 4; j++) { const int f = min(f0 + j, nf - 1); fd4[j] = E.F(HW_FD + f); fv4[j] = E.I(HW_FV + f); }
#pragma unroll
      for (int j = 0; j < 4; j++) if (f0 + j < nf && (fv4[j] >> 24) && fd4[j] < bd) { bd = fd4[j]; best = f0 + j; }
    }
    if (best < 0) { best = 0; break; }
    const V3 bn = E.N(best);
    const HV w = hh_support<false>(h, bn);
    if (dot(w.w, bn) - bd <= 1e-6f || nv >= HH_EPA_MAXV) break;  // the face lies on the boundary of C
    bool dup = false; for (int k = 0; k < nv; k++) dup = dup || E.I(HW_VID + k) == w.id;
    if (dup) break;
    E.put(nv, w);
    // faces that see the new point go; the edges that belonged to exactly one of them are the horizon
    int ne = 0; bool full = false;
    for (int f = 0; f < nf; f++) {
      const int fv = E.I(HW_FV + f); const float fd = E.F(HW_FD + f);
      if (!(fv >> 24) || fd >= 3.0e38f) continue;
      if (!(dot(E.N(f), w.w) - fd > 1e-9f) && f != best) continue;
      E.I(HW_FV + f) = fv & 0xFFFFFF;
      for (int q = 0; q < 3; q++) {
        const int i = (fv >> (8 * q)) & 255, j = (fv >> (8 * ((q + 1) % 3))) & 255, key = i < j ? (i | (j << 8)) : (j | (i << 8));
        int found = -1;
        for (int t = 0; t < ne; t++) if (E.I(HW_ED + t) == key) { found = t; break; }
        if (found >= 0) { E.I(HW_ED + found) = E.I(HW_ED + ne - 1); ne--; } else if (ne < HH_EPA_MAXE) { E.I(HW_ED + ne) = key; ne++; } else full = true;
      }
    }
    for (int t = 0; t < ne; t++) {
      int slot = -1; for (int f = 0; f < nf; f++) if (!(E.I(HW_FV + f) >> 24)) { slot = f; break; }
      if (slot < 0) { if (nf >= HH_EPA_MAXF) break; slot = nf++; }
      const int key = E.I(HW_ED + t); E.face(slot, key & 255, key >> 8, nv, g);
    }
    nv++;
    if (full) break;
  }
  // Witness points: the origin's projection p onto the face's plane as a combination of support points lying IN that plane.  The
  // triangle found is only part of C's face there (a parallelogram when two edges cross, a polygon when a face of one hull rests on
  // the other) and p may lie in another part of it: while p is outside every triangle of the coplanar points found so far, the
  // support point of a direction tilted from the normal towards p (1e-3 rad) is the face's corner on that side.
  const V3 fn = E.N(best); const float fd = E.F(HW_FD + best); const V3 p = fn * fd; int np = 3;
  for (int q = 0; q < 3; q++) { const int k = (E.I(HW_FV + best) >> (8 * q)) & 255; const V3 wk = E.W(k); E.F(HW_PW + 3 * q) = wk.x; E.F(HW_PW + 3 * q + 1) = wk.y; E.F(HW_PW + 3 * q + 2) = wk.z; E.I(HW_PID + q) = E.I(HW_VID + k); }
  auto P = [&](int k) { return v3(E.F(HW_PW + 3 * k), E.F(HW_PW + 3 * k + 1), E.F(HW_PW + 3 * k + 2)) - p; };
  int bi = 0, bj = 1, bk = 2; float bl[3] = {1.f, 0.f, 0.f};
  for (int round = 0; ; round++) {
    float bq = 3.0e38f; V3 qbest = p;
    for (int i = 0; i < np; i++) for (int j = i + 1; j < np; j++) for (int k = j + 1; k < np; k++) {
      float l[3]; hh_closest_tri(P(i), P(j), P(k), l);
      const V3 q = P(i) * l[0] + P(j) * l[1] + P(k) * l[2]; const float qq = dot(q, q);
      if (qq < bq) { bq = qq; qbest = q; bi = i; bj = j; bk = k; bl[0] = l[0]; bl[1] = l[1]; bl[2] = l[2]; }
    }
    if (bq <= 1e-12f || np >= HH_FACE_PTS || round >= HH_FACE_PTS) break;
    const HV w = hh_support<false>(h, fn + qbest * (-1e-3f * frsq(bq)));  // (qbest = nearest point - p: towards p is -qbest)
    if (fd - dot(w.w, fn) > 1e-4f) break;  // not in the plane (0.1 mm): the face ends before p
    bool dup = false; for (int k = 0; k < np; k++) dup = dup || E.I(HW_PID + k) == w.id;
    if (dup) break;
    E.F(HW_PW + 3 * np) = w.w.x; E.F(HW_PW + 3 * np + 1) = w.w.y; E.F(HW_PW + 3 * np + 2) = w.w.z; E.I(HW_PID + np) = w.id; np++;
  }
  auto wit = [&](int k, V3& a, V3& b) {  // the two hull points behind support point k (per-lane index: a vector load from the point table)
    const int id = E.I(HW_PID + k), ia = id >> 8, ib = id & 255;
    a = mul(h.RA, v3(h.pa[3 * ia], h.pa[3 * ia + 1], h.pa[3 * ia + 2])); b = mul(h.RB, v3(h.pb[3 * ib], h.pb[3 * ib + 1], h.pb[3 * ib + 2])) + h.tBA;
  };
  V3 a0, b0, a1, b1, a2, b2; wit(bi, a0, b0); wit(bj, a1, b1); wit(bk, a2, b2);
  pa = a0 * bl[0] + a1 * bl[1] + a2 * bl[2]; pb = b0 * bl[0] + b1 * bl[1] + b2 * bl[2];
  n_out = fn; return fd;
}

// signed distance of hull A from hull B (< 0: they overlap by that much), unit normal from B towards A, witness points (relative
// to A's frame origin).  hit = false once the distance is known to exceed max_dist, or for a lane that did not ask (active false).
HH_FN void hull_hull(const HullPairD& h, V3 seed, float max_dist, bool active, HullHit& out) {
  V3 sw[4], sa[4], sb[4]; int sid[4]; float l[4] = {0.f, 0.f, 0.f, 0.f}; int ns = 0;
  hh_for<0, 4>([&](auto K) { constexpr int k = decltype(K)::value; sw[k] = v3(0.f, 0.f, 0.f); sa[k] = sw[k]; sb[k] = sw[k]; sid[k] = -1; });
  V3 v = dot(seed, seed) > 1e-12f ? seed : v3(1.f, 0.f, 0.f); float vv = 3.0e38f; bool inside = false, far = false, done = !active; int my_iters = 0;
  for (int it = 0; it < HH_GJK_ITERS; it++) {
    if (!__any(!done)) break;
    my_iters += done ? 0 : 1;
    const HV w = hh_support(h, -v);
    if (!done && ns > 0) {
      const float vw = dot(v, w.w), vn = fsqrt(vv);
      if (vw > max_dist * vn) { far = true; done = true; }  // a separating plane farther than anyone asks
      bool dup = false;
      hh_for<0, 4>([&](auto K) { constexpr int k = decltype(K)::value; dup = dup || (k < ns && sid[k] == w.id); });
      if (dup || vv - vw <= 1e-6f * vv + 1e-7f * vn) done = true;  // no support point nearer along v: v is the closest point
    }
    if (!done) {
      V3 tw[4], ta[4], tb[4]; int ti[4];
      hh_for<0, 4>([&](auto K) { constexpr int k = decltype(K)::value; const bool nw = k == ns; tw[k] = hh_sel(nw, w.w, sw[k]); ta[k] = hh_sel(nw, w.a, sa[k]); tb[k] = hh_sel(nw, w.b, sb[k]); ti[k] = nw ? w.id : sid[k]; });
      float ln[4]; const bool in = hh_closest_simplex(tw, ns + 1, ln);
      const V3 nv = tw[0] * ln[0] + tw[1] * ln[1] + tw[2] * ln[2] + tw[3] * ln[3]; const float nvv = dot(nv, nv);
      hh_for<0, 4>([&](auto K) { constexpr int k = decltype(K)::value; sw[k] = hh_sel(in, tw[k], sw[k]); sid[k] = in ? ti[k] : sid[k]; });  // (inside: the tetrahedron the polytope search starts from)
      if (in) { inside = true; done = true; }
      else if (ns > 0 && !(nvv < vv)) done = true;  // (rounding: no progress -- keep the previous simplex)
      else {
        // keep the vertices that carry weight, in their order (slot m takes the m-th of them)
        int m = 0;
        hh_for<0, 4>([&](auto K) {
          constexpr int k = decltype(K)::value; const bool keep = k <= ns && ln[k] > 0.f;
          hh_for<0, k + 1>([&](auto J) { constexpr int j = decltype(J)::value; const bool here = keep && m == j;
            sw[j] = hh_sel(here, tw[k], sw[j]); sa[j] = hh_sel(here, ta[k], sa[j]); sb[j] = hh_sel(here, tb[k], sb[j]); sid[j] = here ? ti[k] : sid[j]; l[j] = here ? ln[k] : l[j]; });
          m += keep ? 1 : 0;
        });
        hh_for<0, 4>([&](auto J) { constexpr int j = decltype(J)::value; l[j] = j < m ? l[j] : 0.f; });  // (slots beyond the simplex keep stale vertices: no weight)
        ns = m; v = nv; vv = nvv;
        if (vv <= HH_SWITCH * HH_SWITCH) done = true;
      }
    }
  }
  const bool deep = active && !far && (inside || vv <= HH_SWITCH * HH_SWITCH);
  out.hit = active && !far; out.iters = my_iters;
  if (__any(deep)) {
    if (deep && h.ew) { V3 nf, pa, pb; const float d = hh_epa(h, seed, inside, sw, sid, nf, pa, pb); out.n = -nf; out.dist = -d; out.pa = pa; out.pb = pb; }
  }
  if (!deep || !h.ew) {  // (no polytope workspace -- a world without hull pairs never gets here: the GJK answer, ~0 along the last direction)
    const float vn = fsqrt(vv), iv = vn > 0.f ? frcp(vn) : 0.f; out.n = v * iv; out.dist = vn;
    out.pa = sa[0] * l[0] + sa[1] * l[1] + sa[2] * l[2] + sa[3] * l[3]; out.pb = sb[0] * l[0] + sb[1] * l[1] + sb[2] * l[2] + sb[3] * l[3];
  }
}

// ---- one-shot contact manifold (DG_HF_HULL_MANIFOLD > 1): up to four points of a hull pair, rebuilt every substep from the pair's
// normal n (B towards A).  Restated in numpy by tests/manifold_ref.py -- same steps, constants and tie-breaks.
//   1. feature of A: its points within tol = DG_HULL_MANIFOLD_TOL x bounding radius of its extreme along -n; of B: along n.  At
//      most HH_MF_CAP points each: the extreme point, then the lowest point indices.  (On a curved hull the angle order can make
//      C non-convex; clipping against its edges then keeps a subset of C's convex hull -- never a point outside C.)  Each ordered by angle about its centroid in the plane normal
//      to n (basis u, v = n x u: u is A's link-frame x axis -- y when x is within 26 degrees of n -- projected on the plane):
//      counter-clockwise about n.
//   2. a single point on either side, or two crossed edges: no manifold (the caller keeps the pair's one contact).  Otherwise the
//      reference feature C is A if it has >= 3 points, else B if it has, else A's edge (parallel edges); the other, S, is clipped
//      against the half-planes of C's edges (a polygon: Sutherland-Hodgman, <= HH_MF_CLIP vertices; an edge: its parameter
//      interval).  A clipped point x of S is separated along n from C's feature plane (its own normal: a tilted face is
//      measured as tilted, whichever hull is A) by sep: depth = sep - 2 x hull margin, kept if below the contact margin; the
//      contact point is the midpoint between x and that plane along n.
//   3. reduction to N: the deepest point, the one farthest from it, the one that spans the largest triangle with those two, the one
//      that adds the most area outside that triangle (Bullet's sortCachedPoints idea); strict comparisons, lowest index first.
//   4. slots: the chosen points ordered by angle about their centroid, from u: slot s gets key DG_CONTACT_KEY(pair, s).
// Everything per lane lives in the lane's column of the polytope workspace (dead once hh_epa has returned), never in private
// arrays with run-time indices.  The point loops are wave-uniform (lane tables / scalar loads, as the support loop); the rest runs
// under divergence on memory only.
#define HH_MF_CAP 8
#define HH_MF_CLIP 16
enum { MF_A = 0 /* A's feature, ordered: 3 x CAP */, MF_B = 3 * HH_MF_CAP, MF_T = 6 * HH_MF_CAP /* unordered points 3 x CAP, angles CAP */,
       MF_P0 = 10 * HH_MF_CAP /* clip buffers: 3 x CLIP each */, MF_P1 = MF_P0 + 3 * HH_MF_CLIP, MF_D = MF_P1 + 3 * HH_MF_CLIP /* depths */,
       MF_R = MF_D + HH_MF_CLIP /* result: 4 x (midpoint 3, depth) in slot order */, MF_END = MF_R + 16 };
static_assert(MF_END <= HH_WS_SLOTS, "manifold buffers must fit the polytope workspace");
// angle about the origin as a monotone stand-in in [0, 4) (0 along +x, counter-clockwise)
DGD float hh_pseudo_angle(float x, float y) {
  const float s = fabsf(x) + fabsf(y); if (!(s > 0.f)) return 0.f;
  const float p = y / s; return x < 0.f ? 2.f - p : (y < 0.f ? 4.f + p : p);
}
template <int SIDE> DGD V3 hh_point(const HullPairD& h, int k) {  // point k of A (0) / B (1) in its link frame; k wave-uniform
  auto rl = [](float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); };
  if (h.tabled) return SIDE ? v3(rl(h.tbx, k), rl(h.tby, k), rl(h.tbz, k)) : v3(rl(h.tax, k), rl(h.tay, k), rl(h.taz, k));
  const hh_cfp p = SIDE ? h.pb : h.pa; return v3(p[3 * k], p[3 * k + 1], p[3 * k + 2]);
}
// feature of one side into `dst` (ordered), its point count; *href = its extreme along n (A: lowest, B: highest)
template <int SIDE>
HH_FN int hh_feature(const HullPairD& h, const HEpa& E, V3 n, V3 u, V3 v, float tol, bool active, int dst, float& href) {
  const M3& R = SIDE ? h.RB : h.RA; const int np = SIDE ? h.nb : h.na;
  const V3 dl = tmul(R, SIDE ? n : -n);
  float s = -3.0e38f; int ks = 0;
  for (int k = 0; k < np; k++) { const float d = dot(hh_point<SIDE>(h, k), dl); if (d > s) { s = d; ks = k; } }
  int m = 0; V3 c = v3(0.f, 0.f, 0.f);
  for (int k = 0; k < np; k++) {  // (the extreme point ks always; the others by index, a slot kept free for ks until it comes)
    const V3 p = hh_point<SIDE>(h, k);
    if (active && (k == ks || m < HH_MF_CAP - (k < ks ? 1 : 0)) && dot(p, dl) >= s - tol) {
      const V3 x = SIDE ? mul(R, p) + h.tBA : mul(R, p);
      E.F(MF_T + 3 * m) = x.x; E.F(MF_T + 3 * m + 1) = x.y; E.F(MF_T + 3 * m + 2) = x.z; c = c + x; m++;
    }
  }
  href = SIDE ? s + dot(h.tBA, n) : -s;
  if (!active || m == 0) return 0;
  c = c * (1.f / (float)m);
  for (int i = 0; i < m; i++) { const V3 d = v3(E.F(MF_T + 3 * i), E.F(MF_T + 3 * i + 1), E.F(MF_T + 3 * i + 2)) - c; E.F(MF_T + 3 * HH_MF_CAP + i) = hh_pseudo_angle(dot(d, u), dot(d, v)); }
  for (int i = 0; i < m; i++) {
    const float ai = E.F(MF_T + 3 * HH_MF_CAP + i); int r = 0;
    for (int j = 0; j < m; j++) { const float aj = E.F(MF_T + 3 * HH_MF_CAP + j); r += (aj < ai || (aj == ai && j < i)) ? 1 : 0; }
    E.F(dst + 3 * r) = E.F(MF_T + 3 * i); E.F(dst + 3 * r + 1) = E.F(MF_T + 3 * i + 1); E.F(dst + 3 * r + 2) = E.F(MF_T + 3 * i + 2);
  }
  return m;
}
// number of manifold points written to MF_R (slot order), 0: keep the pair's single contact.  Coordinates relative to A's origin.
HH_FN int hull_manifold(const HullPairD& h, V3 n, float rad_a, float rad_b, float margin, float hmg, int npts, bool active) {
  const HEpa E = {h.ew};
  V3 a = v3(h.RA.m[0], h.RA.m[3], h.RA.m[6]);
  if (fabsf(dot(a, n)) > 0.9f) a = v3(h.RA.m[1], h.RA.m[4], h.RA.m[7]);
  V3 u = a - n * dot(a, n); u = u * frsq(dot(u, u)); const V3 v = cross(n, u);
  float hA, hB;
  const int ma = hh_feature<0>(h, E, n, u, v, DG_HULL_MANIFOLD_TOL * rad_a, active, MF_A, hA);
  const int mb = hh_feature<1>(h, E, n, u, v, DG_HULL_MANIFOLD_TOL * rad_b, active, MF_B, hB);
  if (!active || ma < 2 || mb < 2) return 0;
  auto X = [&](int base, int i) { return v3(E.F(base + 3 * i), E.F(base + 3 * i + 1), E.F(base + 3 * i + 2)); };
  auto put = [&](int base, int i, V3 x) { E.F(base + 3 * i) = x.x; E.F(base + 3 * i + 1) = x.y; E.F(base + 3 * i + 2) = x.z; };
  if (ma == 2 && mb == 2) {  // two edges: crossed (no manifold) or parallel
    const V3 ea = X(MF_A, 1) - X(MF_A, 0), eb = X(MF_B, 1) - X(MF_B, 0), cx = cross(ea, eb);
    if (dot(cx, cx) > DG_HULL_MANIFOLD_TOL * DG_HULL_MANIFOLD_TOL * dot(ea, ea) * dot(eb, eb)) return 0;
  }
  const bool refA = ma >= 3 || mb < 3;  // the reference feature C: A, unless only B is a polygon
  const int cb = refA ? MF_A : MF_B, mc = refA ? ma : mb, sb = refA ? MF_B : MF_A, ms = refA ? mb : ma;
  const float href = refA ? hA : hB, sgn = refA ? -1.f : 1.f;
  const int npl = mc >= 3 ? mc : 2;
  auto plane = [&](int j, V3& q, V3& d) {  // half-plane j of C: dot(x - q, d) >= 0 inside
    if (mc >= 3) { q = X(cb, j); d = cross(n, X(cb, j + 1 < mc ? j + 1 : 0) - q); }
    else { q = X(cb, j); d = X(cb, 1 - j) - q; }
  };
  int src, cnt;
  if (ms == 2) {  // an edge: its parameter interval inside every half-plane
    const V3 p0 = X(sb, 0), dir = X(sb, 1) - p0; float t0 = 0.f, t1 = 1.f;
    for (int j = 0; j < npl; j++) {
      V3 q, d; plane(j, q, d); const float f0 = dot(p0 - q, d), fd = dot(dir, d);
      if (fd == 0.f) { if (f0 < 0.f) t1 = -1.f; }
      else if (fd > 0.f) t0 = fmaxf(t0, -f0 / fd);
      else t1 = fminf(t1, -f0 / fd);
    }
    cnt = 0; src = MF_P0;
    if (t0 <= t1) { put(MF_P0, 0, p0 + dir * t0); put(MF_P0, 1, p0 + dir * t1); cnt = 2; }
  } else {  // a polygon: Sutherland-Hodgman, ping-pong between the two clip buffers
    src = sb; cnt = ms; int dst = MF_P0;
    for (int j = 0; j < npl && cnt > 0; j++) {
      V3 q, d; plane(j, q, d); int oc = 0;
      V3 prev = X(src, cnt - 1); float fp = dot(prev - q, d);
      for (int i = 0; i < cnt; i++) {
        const V3 cur = X(src, i); const float fc = dot(cur - q, d);
        if ((fc >= 0.f) != (fp >= 0.f) && oc < HH_MF_CLIP) { put(dst, oc, prev + (cur - prev) * (fp / (fp - fc))); oc++; }
        if (fc >= 0.f && oc < HH_MF_CLIP) { put(dst, oc, cur); oc++; }
        prev = cur; fp = fc;
      }
      cnt = oc; src = dst; dst = dst == MF_P0 ? MF_P1 : MF_P0;
    }
  }
  // C's feature plane: through its centroid, normal = the polygon's area vector (Newell); an edge: the plane through it nearest to
  // normal to n.  A feature whose plane leans more than ~26 degrees from n (nearly collinear points) falls back to the plane
  // normal to n through C's extreme
  V3 c0 = v3(0.f, 0.f, 0.f), nc = v3(0.f, 0.f, 0.f);
  for (int j = 0; j < mc; j++) c0 = c0 + X(cb, j);
  c0 = c0 * (1.f / (float)mc);
  if (mc >= 3) { for (int j = 0; j < mc; j++) nc = nc + cross(X(cb, j) - c0, X(cb, j + 1 < mc ? j + 1 : 0) - c0); }
  else { const V3 e = X(cb, 1) - X(cb, 0); const float ee = dot(e, e); nc = ee > 1e-20f ? n - e * (dot(e, n) / ee) : n; }
  float dn = dot(n, nc);
  if (!(dn * dn >= 0.81f * dot(nc, nc)) || !(dn != 0.f)) { nc = n; c0 = n * href; dn = 1.f; }
  // depths: along n from a clipped point x of S to C's plane (x + t n on it); the points below the contact margin, as midpoints,
  // into the other clip buffer
  const int kb = src == MF_P0 ? MF_P1 : MF_P0; int nk = 0;
  for (int i = 0; i < cnt; i++) {
    const V3 x = X(src, i); const float t = -dot(x - c0, nc) / dn, sep = -sgn * t, depth = sep - 2.f * hmg;
    if (depth < margin) { put(kb, nk, x + n * (0.5f * t)); E.F(MF_D + nk) = depth; nk++; }
  }
  if (nk == 0) return 0;
  // reduction: deepest, farthest from it, largest triangle, most area added outside the triangle
  int i0 = 0; { float bd = E.F(MF_D); for (int i = 1; i < nk; i++) { const float di = E.F(MF_D + i); if (di < bd) { bd = di; i0 = i; } } }
  const V3 x0 = X(kb, i0); int i1 = -1, i2 = -1, i3 = -1;
  if (npts >= 2) { float bs = -3.0e38f; for (int i = 0; i < nk; i++) { const V3 e = X(kb, i) - x0; const float s = dot(e, e); if (i != i0 && s > bs) { bs = s; i1 = i; } } }
  const V3 x1 = X(kb, i1 < 0 ? i0 : i1);
  if (npts >= 3 && i1 >= 0) { float bs = -3.0e38f; for (int i = 0; i < nk; i++) { const V3 c = cross(x1 - x0, X(kb, i) - x0); const float s = dot(c, c); if (i != i0 && i != i1 && s > bs) { bs = s; i2 = i; } } }
  const V3 x2 = X(kb, i2 < 0 ? i0 : i2);
  if (npts >= 4 && i2 >= 0) {
    const float o = dot(cross(x1 - x0, x2 - x0), n) >= 0.f ? -1.f : 1.f;  // (outside of a counter-clockwise edge: negative)
    float bs = -3.0e38f;
    for (int i = 0; i < nk; i++) {
      const V3 x = X(kb, i);
      const float s = fmaxf(fmaxf(o * dot(cross(x1 - x0, x - x0), n), o * dot(cross(x2 - x1, x - x1), n)), o * dot(cross(x0 - x2, x - x2), n));
      if (i != i0 && i != i1 && i != i2 && s > bs) { bs = s; i3 = i; }
    }
  }
  const int m = 1 + (i1 >= 0) + (i2 >= 0) + (i3 >= 0);
  const V3 x3 = X(kb, i3 < 0 ? i0 : i3);
  const V3 cm = (((x0 + (i1 >= 0 ? x1 : v3(0.f, 0.f, 0.f))) + (i2 >= 0 ? x2 : v3(0.f, 0.f, 0.f))) + (i3 >= 0 ? x3 : v3(0.f, 0.f, 0.f))) * (1.f / (float)m);
  const float g0 = hh_pseudo_angle(dot(x0 - cm, u), dot(x0 - cm, v)), g1 = hh_pseudo_angle(dot(x1 - cm, u), dot(x1 - cm, v));
  const float g2 = hh_pseudo_angle(dot(x2 - cm, u), dot(x2 - cm, v)), g3 = hh_pseudo_angle(dot(x3 - cm, u), dot(x3 - cm, v));
  // slot of choice c: the chosen points before it by angle (ties: earlier choice first)
  const int r0 = (m > 1 && g1 < g0) + (m > 2 && g2 < g0) + (m > 3 && g3 < g0);
  const int r1 = (g0 <= g1) + (m > 2 && g2 < g1) + (m > 3 && g3 < g1);
  const int r2 = (g0 <= g2) + (g1 <= g2) + (m > 3 && g3 < g2);
  const int r3 = (g0 <= g3) + (g1 <= g3) + (g2 <= g3);
  auto res = [&](int slot, int i, V3 x) { E.F(MF_R + 4 * slot) = x.x; E.F(MF_R + 4 * slot + 1) = x.y; E.F(MF_R + 4 * slot + 2) = x.z; E.F(MF_R + 4 * slot + 3) = E.F(MF_D + i); };
  res(r0, i0, x0);
  if (m > 1) res(r1, i1, x1);
  if (m > 2) res(r2, i2, x2);
  if (m > 3) res(r3, i3, x3);
  return m;
}

}  // namespace dg
