// dg_contactf.h -- contact forces in full: the lateral friction the contact query (dg_contactq.h) leaves out, and the per-link net
// contact wrench.  One env per lane in the world's own workspace mode, one launch per call, nothing allocated; the state is read,
// never written, and nothing the step stores changed: store_warm_cache (dg_solver.h) already writes [key, normal, t1, t2] per contact.
//
//   contact_force_kernel       per contact, in pair order, with the filters and the side swapping of contact_query_kernel: ids,
//                              the normal, the normal force, the two friction forces along the solver's tangents, the tangents,
//                              and the total force on side A,  force_on_a = fn n + f1 t1 + f2 t2.
//   net_contact_wrench_kernel  for one body and up to DG_CONTACT_MAX_LINKS link selectors: per selector the sum over the
//                              contacts whose side on this body matches of the force on this body and of its moment about the
//                              origin of the link's inertial frame (what frame_state reports with com = 1; the base's for
//                              DG_CONTACT_ANY), the arm being the surface point on this body's side, p +/- n d / 2.
// GEOMETRY, tangents and arms are those of the state handed in; the IMPULSES are what the solver applied in the LAST SUBSTEP to
// the contact of the same key, 0 for a new one (include/diygym_hip.h has the rule in full).  The three impulses of a contact are
// loaded together, in one round trip, as warm_impulses does; the warm-start factors are NOT applied.
//
// Signs.  In the solver's rows (build_contact_rows) the accumulated impulse along `dir` acts on A along +dir and on B along -dir,
// whichever side is dynamic, and CL_N points from B to A: the force on the narrow phase's A is fn n + f1 t1 + f2 t2 with
// (t1, t2) = tangent_basis(n) of the narrow phase's OWN normal.  Where the filter swaps the sides, the normal and BOTH tangents are
// negated and the scalars kept -- tangent_basis(-n) is not -tangent_basis(n) (t1 flips, t2 does not), so a basis recomputed from
// the negated normal would report a force that is not the negative of the other side's.
//
// Workspace and grid: those of dg_contactq.h, for its two reasons -- launched with the grid and block of reset_kernel<LANES>
// (the polytope workspace is indexed by wavefront), lanes without an env stay in every call that votes with __any, clamped to the
// last env, and only their stores are masked.  net_contact_wrench_kernel keeps each contact's force vector in the three slots
// CL_DVA, CL_NVA, CL_DVB of the lane's own contact list, which only build_contact_rows writes and which the next step rebuilds:
// the cache is then searched once per contact, not once per contact and selector, and the selectors re-read the list.
#pragma once
#include "dg_contactq.h"
#include "dg_launch.h"  // CfSelectors, the link selectors of net_contact_wrench_kernel, which the host side shares

namespace dg {

// (the columns of a row: DG_CFO_* of include/diygym_hip.h)

// normal, t1 and t2 force of the contact at list offset `co`: the cached impulses of its key over the substep, 0 without an entry.
// Called under divergence like warm_find; `keep` false searches for no key.
template <int LANES>
DGD void cf_forces(const Lane<LANES>& ln, int co, bool keep, float (&f)[3]) {
  const DevScene& sc = ln.sc;
  const int found = warm_find(ln, keep ? ln.L(co + CL_KEY) : -1.f);
  const int e = sc.warm_off + 1 + max(found, 0) * DG_WS_STRIDE + DG_WS_NORMAL;
  const float v0 = ln.S(e), v1 = ln.S(e + 1), v2 = ln.S(e + 2), inv_h = 1.0f / sc.h;
  f[0] = found >= 0 ? v0 * inv_h : 0.f; f[1] = found >= 0 ? v1 * inv_h : 0.f; f[2] = found >= 0 ? v2 * inv_h : 0.f;
}

// count [num_envs]; ids [num_envs][C][2], out [num_envs][C][DG_CFO_STRIDE] (each may be null), C = sc.max_contacts.
// Every slot is written: -1 ids and zeros behind the env's count.  The host refuses a world without the impulse cache.
template <int LANES>
__global__ __launch_bounds__(64) void contact_force_kernel(DevScene sc, MotorTable mt, float* state, int body_a, int link_a, int body_b, int link_b,
                                                            int32_t* count, int32_t* ids, float* out, float* gws) {
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  const int env = blockIdx.x * ACTIVE + lane; const bool valid = env < sc.num_envs; const int e = valid ? env : sc.num_envs - 1;
  Lane<LANES> ln(sc, mt, workspace_of<LANES>(sc, smem, gws, lane), state + e, e, false);  // never stores state
  for (int b = 0; b < sc.nba; b++) ln.kinematics(b);
  const int ncont = collide<LANES, 0>(ln);
  const int C = sc.max_contacts; const size_t row = (size_t)e * (size_t)C;
  int k = 0;  // rows written so far: the contacts that pass the filter, in pair order
  for (int c = 0; c < C; c++) {
    const bool has = c < ncont;
    if (!__any(has)) break;
    const int co = sc.cont_off + 1 + c * CL_STRIDE;
    const int pair = has ? (int)ln.L(co + CL_PAIR) : 0;
    int ia = cq_shape_id(sc, sc.PI[pair * DG_PI_STRIDE + DG_PI_A]), ib = cq_shape_id(sc, sc.PI[pair * DG_PI_STRIDE + DG_PI_B]);
    const bool fwd = cq_match(ia, body_a, link_a) && cq_match(ib, body_b, link_b), rev = cq_match(ib, body_a, link_a) && cq_match(ia, body_b, link_b);
    const bool keep = has && (fwd || rev), swap = !fwd;
    float f[3] = {0.f, 0.f, 0.f};
    if (out && __any(keep)) cf_forces(ln, co, keep, f);  // (a slot no lane reports is not searched for)
    if (!keep) continue;
    if (valid) {
      if (out) {
        V3 n = ln.L3(co + CL_N), t1, t2; tangent_basis(n, t1, t2);  // the basis the rows were built with
        V3 fa = n * f[0] + t1 * f[1] + t2 * f[2];
        if (swap) { n = -n; t1 = -t1; t2 = -t2; fa = -fa; }
        float* o = out + (row + k) * DG_CFO_STRIDE;
        o[DG_CFO_NORMAL] = n.x; o[DG_CFO_NORMAL + 1] = n.y; o[DG_CFO_NORMAL + 2] = n.z; o[DG_CFO_NORMAL_FORCE] = f[0];
        o[DG_CFO_LATERAL1] = f[1]; o[DG_CFO_DIR1] = t1.x; o[DG_CFO_DIR1 + 1] = t1.y; o[DG_CFO_DIR1 + 2] = t1.z;
        o[DG_CFO_LATERAL2] = f[2]; o[DG_CFO_DIR2] = t2.x; o[DG_CFO_DIR2 + 1] = t2.y; o[DG_CFO_DIR2 + 2] = t2.z;
        o[DG_CFO_FORCE_A] = fa.x; o[DG_CFO_FORCE_A + 1] = fa.y; o[DG_CFO_FORCE_A + 2] = fa.z;
      }
      if (ids) { int32_t* o = ids + (row + k) * 2; o[0] = swap ? ib : ia; o[1] = swap ? ia : ib; }
    }
    k++;
  }
  if (!valid) return;
  count[e] = k;
  for (int j = k; j < C; j++) {
    if (ids) { int32_t* o = ids + (row + j) * 2; o[0] = -1; o[1] = -1; }
    if (out) { float* o = out + (row + j) * DG_CFO_STRIDE; for (int t = 0; t < DG_CFO_STRIDE; t++) o[t] = 0.f; }
  }
}

// wrench [num_envs][n][6] (force 3, moment 3), ncontacts [num_envs][n] (may be null).  Each slot is stored exactly once, from
// registers: selector by selector over the contact list in pair order, so the order of summation is the same in every mode.
template <int LANES>
__global__ __launch_bounds__(64) void net_contact_wrench_kernel(DevScene sc, MotorTable mt, float* state, int body, CfSelectors sel, int body_b, int link_b,
                                                                 float* wrench, int32_t* ncontacts, float* gws) {
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  const int env = blockIdx.x * ACTIVE + lane; const bool valid = env < sc.num_envs; const int e = valid ? env : sc.num_envs - 1;
  Lane<LANES> ln(sc, mt, workspace_of<LANES>(sc, smem, gws, lane), state + e, e, false);  // never stores state
  for (int b = 0; b < sc.nba; b++) ln.kinematics(b);
  const int ncont = collide<LANES, 0>(ln);
  const int C = sc.max_contacts;
  // 1. the force on the narrow phase's side A of every contact that has this body on a side, into the lane's own list
  for (int c = 0; c < C; c++) {
    const bool has = c < ncont;
    if (!__any(has)) break;
    const int co = sc.cont_off + 1 + c * CL_STRIDE;
    const int pair = has ? (int)ln.L(co + CL_PAIR) : 0;
    const int ia = cq_shape_id(sc, sc.PI[pair * DG_PI_STRIDE + DG_PI_A]), ib = cq_shape_id(sc, sc.PI[pair * DG_PI_STRIDE + DG_PI_B]);
    const bool keep = has && ((cq_match(ia, body, DG_CONTACT_ANY) && cq_match(ib, body_b, link_b)) || (cq_match(ib, body, DG_CONTACT_ANY) && cq_match(ia, body_b, link_b)));
    if (!__any(keep)) continue;
    float f[3]; cf_forces(ln, co, keep, f);
    if (!keep) continue;
    V3 n = ln.L3(co + CL_N), t1, t2; tangent_basis(n, t1, t2);
    const V3 fa = n * f[0] + t1 * f[1] + t2 * f[2];
    ln.L(co + CL_DVA) = fa.x; ln.L(co + CL_NVA) = fa.y; ln.L(co + CL_DVB) = fa.z;
  }
  // 2. the sums, selector by selector
  for (int s = 0; s < sel.n; s++) {
    const int link = sel.link[s];
    V3 org, v_, w_; Q4 q_; ln.frame_state(body, sel.frame[s], true, org, q_, v_, w_, false);
    V3 F = v3(0.f, 0.f, 0.f), T = v3(0.f, 0.f, 0.f); int cnt = 0;
    for (int c = 0; c < ncont; c++) {
      const int co = sc.cont_off + 1 + c * CL_STRIDE;
      const int pair = (int)ln.L(co + CL_PAIR);
      const int ia = cq_shape_id(sc, sc.PI[pair * DG_PI_STRIDE + DG_PI_A]), ib = cq_shape_id(sc, sc.PI[pair * DG_PI_STRIDE + DG_PI_B]);
      const bool fwd = cq_match(ia, body, link) && cq_match(ib, body_b, link_b), rev = cq_match(ib, body, link) && cq_match(ia, body_b, link_b);
      if (!fwd && !rev) continue;
      // (a contact between two links of this body that both match counts once, as side A: the sides of contact_force_kernel)
      const V3 p = ln.L3(co + CL_P), n = ln.L3(co + CL_N); const float d = ln.L(co + CL_DIST);
      const V3 hn = n * (0.5f * d), fa = v3(ln.L(co + CL_DVA), ln.L(co + CL_NVA), ln.L(co + CL_DVB));
      const V3 f = fwd ? fa : -fa, arm = (fwd ? p + hn : p - hn) - org;
      F = F + f; T = T + cross(arm, f); cnt++;
    }
    if (valid) {
      float* o = wrench + ((size_t)e * sel.n + s) * 6;
      o[0] = F.x; o[1] = F.y; o[2] = F.z; o[3] = T.x; o[4] = T.y; o[5] = T.z;
      if (ncontacts) ncontacts[(size_t)e * sel.n + s] = cnt;
    }
  }
}

}  // namespace dg
