// dg_contactq.h -- batched contact query (pybullet's p.getContactPoints(bodyA, bodyB, linkIndexA, linkIndexB); the reference never
// calls it -- no addon of its own reads contacts -- so there is no call site to name: this is the query a pybullet user expects, and
// what the `contact_sensor` addon is built on).  One env per lane in the world's own workspace mode, one launch per call, nothing
// allocated; the state is read, never written.
//
//   contact_query_kernel  world kinematics of every moving body, then collide<LANES, 0> (dg_solver.h) -- the narrow phase of the
//                         step, in the form the reset kernel runs one lane per env -- and the list it leaves at sc.cont_off read
//                         back: per contact both sides' ids (uid + ((link + 1) << 24), the expression of dg_raycast.h and
//                         dg_render.h), the two surface points p +/- n d / 2, the normal from B towards A, the signed distance
//                         and the normal force.
// GEOMETRY is that of the state handed in.  The FORCE is the normal impulse the solver applied in the LAST SUBSTEP to the contact
// of the same key (DG_CONTACT_KEY(pair, feature); the contact impulse cache DG_WS_* that store_warm_cache writes), divided by the
// substep: a contact that is new since then, or whose feature changed, reports 0 (include/diygym_hip.h has the rule in full).
//
// Workspace.  (a) collide's hull-against-hull branch indexes the polytope workspace by WAVEFRONT (hull_ws_of: blockIdx.x x waves
// per block + wave), which dg_plan.hip sizes as ceil(num_envs / envs per wavefront) blocks (x 4 in helper-wave worlds).  The query
// is launched with the grid and block of reset_kernel<LANES> -- ceil(num_envs / envs per wavefront) workgroups of ONE wavefront --
// so its wavefront index is blockIdx.x < that count in every world, and the same holds for the global scratch of the modes 0 and
// -16 (workspace_of).  (b) collide votes with __any and reads lane tables: the lanes of the last wavefront that have no env stay
// in the call, clamped to the last env as observe_kernel does (they recompute that env's contacts in their own workspace column);
// only the output stores are masked.  The transient region holds collide's per-shape cache as in every step; nothing else is used.
#pragma once
#include "dg_solver.h"

namespace dg {

enum { CQ_POS_A = 0, CQ_POS_B = 3, CQ_NORMAL = 6, CQ_DIST = 9, CQ_GEOM_STRIDE = 10 };

// id of a shape as the camera's segmentation mask and the ray cast report it
DGD int cq_shape_id(const DevScene& sc, int sh) { cip si = sc.SI + sh * DG_SI_STRIDE; return si[DG_SI_BODY] + (((si[DG_SI_FLAGS] >> 8) & 0xFFFF) << 24); }
// a side's id against a (body, link) filter: DG_CONTACT_ANY matches everything
DGD bool cq_match(int id, int body, int link) {
  return body == DG_CONTACT_ANY || ((id & 0xFFFFFF) == body && (link == DG_CONTACT_ANY || (id >> 24) - 1 == link));
}

// count [num_envs]; ids [num_envs][C][2], geom [num_envs][C][10], force [num_envs][C] (each may be null), C = sc.max_contacts.
// Every slot is written: -1 ids and zeros behind the env's count.
template <int LANES>
__global__ __launch_bounds__(64) void contact_query_kernel(DevScene sc, MotorTable mt, float* state, int body_a, int link_a, int body_b, int link_b,
                                                            int32_t* count, int32_t* ids, float* geom, float* force, float* gws) {
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  const int env = blockIdx.x * ACTIVE + lane; const bool valid = env < sc.num_envs; const int e = valid ? env : sc.num_envs - 1;
  Lane<LANES> ln(sc, mt, workspace_of<LANES>(sc, smem, gws, lane), state + e, e, false);  // never stores state
  for (int b = 0; b < sc.nba; b++) ln.kinematics(b);
  const int ncont = collide<LANES, 0>(ln);
  const int C = sc.max_contacts; const float inv_h = 1.0f / sc.h; const bool want_force = force != nullptr && sc.warm_off >= 0;
  const size_t row = (size_t)e * (size_t)C;
  int k = 0;  // rows written so far: the contacts that pass the filter, in pair order
  for (int c = 0; c < C; c++) {
    const bool has = c < ncont;
    if (!__any(has)) break;
    const int co = sc.cont_off + 1 + c * CL_STRIDE;
    const int pair = has ? (int)ln.L(co + CL_PAIR) : 0;  // (per lane: the slot behind the count holds whatever the last step left)
    int ia = cq_shape_id(sc, sc.PI[pair * DG_PI_STRIDE + DG_PI_A]), ib = cq_shape_id(sc, sc.PI[pair * DG_PI_STRIDE + DG_PI_B]);
    const bool fwd = cq_match(ia, body_a, link_a) && cq_match(ib, body_b, link_b), rev = cq_match(ib, body_a, link_a) && cq_match(ia, body_b, link_b);
    const bool keep = has && (fwd || rev), swap = !fwd;
    float f = 0.f;
    if (want_force && __any(keep)) {  // (warm_find: the search the step's row construction does, eight keys per round trip; a slot
                                      // no lane reports -- the usual case of a filtered query -- is not searched for)
      const int found = warm_find(ln, keep ? ln.L(co + CL_KEY) : -1.f);
      const float imp = ln.S(sc.warm_off + 1 + max(found, 0) * DG_WS_STRIDE + DG_WS_NORMAL);
      f = found >= 0 ? imp * inv_h : 0.f;
    }
    if (!keep) continue;
    const V3 p = ln.L3(co + CL_P); V3 n = ln.L3(co + CL_N); const float d = ln.L(co + CL_DIST);
    const V3 hn = n * (0.5f * d); V3 pa = p + hn, pb = p - hn;
    if (swap) { const int t = ia; ia = ib; ib = t; const V3 tp = pa; pa = pb; pb = tp; n = v3(-n.x, -n.y, -n.z); }
    if (valid) {
      if (ids) { int32_t* o = ids + (row + k) * 2; o[0] = ia; o[1] = ib; }
      if (geom) {
        float* o = geom + (row + k) * CQ_GEOM_STRIDE;
        o[CQ_POS_A] = pa.x; o[CQ_POS_A + 1] = pa.y; o[CQ_POS_A + 2] = pa.z; o[CQ_POS_B] = pb.x; o[CQ_POS_B + 1] = pb.y; o[CQ_POS_B + 2] = pb.z;
        o[CQ_NORMAL] = n.x; o[CQ_NORMAL + 1] = n.y; o[CQ_NORMAL + 2] = n.z; o[CQ_DIST] = d;
      }
      if (force) force[row + k] = f;
    }
    k++;
  }
  if (!valid) return;
  count[e] = k;
  for (int j = k; j < C; j++) {
    if (ids) { int32_t* o = ids + (row + j) * 2; o[0] = -1; o[1] = -1; }
    if (geom) { float* o = geom + (row + j) * CQ_GEOM_STRIDE; for (int t = 0; t < CQ_GEOM_STRIDE; t++) o[t] = 0.f; }
    if (force) force[row + j] = 0.f;
  }
}

}  // namespace dg
