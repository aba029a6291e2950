// dg_fdq.h -- batched forward dynamics of a fixed-base articulated body, and K-sample joint-space rollouts through that model:
//   forward_dynamics_kernel   qdd = M(q)^-1 (tau - h(q, qd)), h = C qd - G: the rigid-body terms of inverse_dynamics_kernel, so the
//                             two calls are inverses of each other.  One env per lane, in inverse_dynamics_kernel's frame.
//   rollout_kernel            one work item per (env e, sample k), B x K in all: the item stages q0, qd0 (the caller's rows or env
//                             e's own), then for t = 0 .. T-1 reads tau[e][k][t][:], computes qdd as above and integrates
//                             semi-implicitly, the step's order: qd += dt qdd; q += dt qd.  Row t of q, qd, pos is the state AFTER
//                             step t + 1; pos is the world position of the point `lx ly lz` of the INERTIAL frame of `frame`'s link
//                             (the point jacobian_kernel and task_space_kernel take) at the NEW q.
// With `damp` the joint damping of the step, DG_LF_DAMPING x qd (Lane::dynamics), comes off tau first.  A MODEL, not the step: no
// joint limits, no motors, no link (linear / angular) damping, no contacts.
//
// Form (fq_solve): a Newton-Euler pass at qdd = 0 for h (the right-hand side tau - damping qd - h is formed on the backward pass),
// composite rigid bodies for M packed lower, Cholesky in place, two triangular solves.  The passes are this header's own copies of
// those in dg_taskq.h (statement for statement, pivot floor rule included: a pivot <= FQ_PIVOT_FLOOR x its own diagonal entry of
// M is held at that floor and flagged), so dg_taskq.h, dg_dynq.h and their kernels are as they were.
//
// Workspace: the transient region, nothing enlarged; matrices live in workspace slots, not in per-lane arrays.
//   kept throughout   [q n][qd n][tau -> right-hand side -> qdd n]                          3 n
//   Newton-Euler      [DQ_ID_STRIDE per link]                                               + 15 n
//   joint inertia     [composite bodies DQ_CR_STRIDE per link][M packed lower n (n + 1) / 2]  + 10 n + n (n + 1) / 2
// fdq_slots() is 3 n + the larger of the two; the planner's 12 + 32 n holds it for every n <= 12.
//
// GRID AND WORKSPACE of rollout_kernel.  The global workspace is [workgroups of the STEP grid][slot][lane]: a workgroup past the
// step's grid would write behind it in the global-workspace modes (LANES <= 0).  So the kernel is a grid-stride loop over the
// items -- item = blockIdx.x ACTIVE + lane; item < B K; item += gridDim.x ACTIVE -- on the workspace column of ITS workgroup and
// lane, whatever env the item belongs to, and dg_world_rollout launches ceil(B K / ACTIVE) workgroups in the LDS modes and no
// more than the step's grid in the global-workspace modes.  The lanes of a wavefront leave the loop after different trip counts at
// the tail; that is safe only because these passes hold no cross-lane operation (no ballot, shuffle, DPP or barrier: no lane talks
// to another, as in dg_dynq.h) -- keep it so.  Link tables and parent lookups are wave-uniform (scalar loads).  Every output index
// is a size_t.
#pragma once
#include "dg_dynq.h"

namespace dg {

constexpr float FQ_PIVOT_FLOOR = 1e-5f;
constexpr int fdq_keep(int n) { return 3 * n; }
constexpr int fdq_newton(int n) { return DQ_ID_STRIDE * n; }
constexpr int fdq_inertia(int n) { return DQ_CR_STRIDE * n + n * (n + 1) / 2; }
constexpr int fdq_slots(int n) { return fdq_keep(n) + (fdq_newton(n) > fdq_inertia(n) ? fdq_newton(n) : fdq_inertia(n)); }

// The n values at xo: tau in, qdd = M^-1 (tau - damping qd - h) out, at the q staged at qo (ln.kinematics(body, qo) done) and the
// qd at vo; blk: fdq_newton / fdq_inertia slots of scratch.  True: a pivot of M's factorisation was held at the floor.
template <int LANES>
DGD bool fq_solve(const Lane<LANES>& ln, int body, int first, int n, int vo, int xo, int blk, bool damp) {
  const DevScene& sc = ln.sc;
  const V3 zero = v3(0.f, 0.f, 0.f);
  // ---- recursive Newton-Euler at qdd = 0 (inverse_dynamics_kernel's passes)
  {
    const V3 g = v3(sc.gx, sc.gy, sc.gz);
    for (int i = 0; i < n; i++) {  // root to tip
      const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_ID_STRIDE;
      const M3 R = ln.LR(po); const V3 p = ln.L3(po + 6), axw = dq_axis(ln, gl, R);
      const float qdi = ln.L(vo + i), qddi = 0.f;
      V3 wp = zero, alp = zero, ap = -g, r = zero;  // the fixed base: at rest, accelerating against gravity
      if (par >= 0) { const int op = blk + (par - first) * DQ_ID_STRIDE; wp = ln.L3(op + DQ_W); alp = ln.L3(op + DQ_AL); ap = ln.L3(op + DQ_A); r = p - ln.L3(ln.pll(par)[PLL_POSE] + 6); }
      V3 w = wp, al = alp, a = ap + cross(alp, r) + cross(wp, cross(wp, r));
      const V3 sv = axw * qdi, cv = cross(wp, sv);
      if (ln.li(gl)[DG_LI_TYPE] == 0) { w = wp + sv; al = alp + axw * qddi + cv; }
      else a = a + axw * qddi + cv * 2.f;
      float ms; V3 c; Sym3 Ic; ln.link_inertia(gl, ms, c, Ic);
      const V3 cw = mul(R, c), ac = a + cross(al, cw) + cross(w, cross(w, cw)), F = ac * ms;
      const V3 N = dq_rot_inertia(R, Ic, al) + cross(w, dq_rot_inertia(R, Ic, w)) + cross(cw, F);  // about the link origin
      ln.L3set(o + DQ_W, w); ln.L3set(o + DQ_AL, al); ln.L3set(o + DQ_A, a); ln.L3set(o + DQ_F, F); ln.L3set(o + DQ_N, N);
    }
    for (int i = n - 1; i >= 0; i--) {  // tip to root; the right-hand side on the way
      const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_ID_STRIDE;
      const V3 f = ln.L3(o + DQ_F), nn = ln.L3(o + DQ_N), axw = dq_axis(ln, gl, ln.LR(po));
      const float hi = ln.li(gl)[DG_LI_TYPE] == 0 ? dot(axw, nn) : dot(axw, f);
      float t = ln.L(xo + i); if (damp) t -= ln.lf(gl)[DG_LF_DAMPING] * ln.L(vo + i);
      ln.L(xo + i) = t - hi;
      if (par >= 0) {
        const int op = blk + (par - first) * DQ_ID_STRIDE; const V3 r = ln.L3(po + 6) - ln.L3(ln.pll(par)[PLL_POSE] + 6);
        ln.L3set(op + DQ_F, ln.L3(op + DQ_F) + f); ln.L3set(op + DQ_N, ln.L3(op + DQ_N) + nn + cross(r, f));
      }
    }
  }
  // ---- M by composite rigid bodies (mass_matrix_kernel's passes), packed lower, over the dead Newton-Euler blocks
  const int Mo = blk + DQ_CR_STRIDE * n;
  {
    const V3 O = ln.base_pos(body);  // moments are taken about the base origin
    for (int i = 0; i < n; i++) {  // each link's own rigid inertia
      const int gl = first + i, po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_CR_STRIDE;
      const M3 R = ln.LR(po); float ms; V3 c; Sym3 Ic; ln.link_inertia(gl, ms, c, Ic);
      const V3 cw = (ln.L3(po + 6) - O) + mul(R, c); const float cc = dot(cw, cw);
      const Sym3 Iw = symmetrize(mul(mul(R, full(Ic)), transpose(R)));
      ln.L(o + DQ_I) = Iw.xx + ms * (cc - cw.x * cw.x); ln.L(o + DQ_I + 1) = Iw.xy - ms * cw.x * cw.y; ln.L(o + DQ_I + 2) = Iw.xz - ms * cw.x * cw.z;
      ln.L(o + DQ_I + 3) = Iw.yy + ms * (cc - cw.y * cw.y); ln.L(o + DQ_I + 4) = Iw.yz - ms * cw.y * cw.z; ln.L(o + DQ_I + 5) = Iw.zz + ms * (cc - cw.z * cw.z);
      ln.L3set(o + DQ_H, cw * ms); ln.L(o + DQ_M) = ms;
    }
    for (int i = n - 1; i >= 0; i--) {  // tip to root: a link's block becomes its subtree's
      const int par = ln.li(first + i)[DG_LI_PARENT]; if (par < 0) continue;
      const int o = blk + i * DQ_CR_STRIDE, op = blk + (par - first) * DQ_CR_STRIDE;
      for (int k = 0; k < DQ_CR_STRIDE; k++) ln.L(op + k) += ln.L(o + k);
    }
    for (int i = 0; i < n; i++) {
      const int gl = first + i, po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_CR_STRIDE;
      const V3 axi = dq_axis(ln, gl, ln.LR(po)); const bool revi = ln.li(gl)[DG_LI_TYPE] == 0;
      const V3 wi = revi ? axi : zero, vi = revi ? cross(ln.L3(po + 6) - O, axi) : axi;
      const Sym3 Io = {ln.L(o + DQ_I), ln.L(o + DQ_I + 1), ln.L(o + DQ_I + 2), ln.L(o + DQ_I + 3), ln.L(o + DQ_I + 4), ln.L(o + DQ_I + 5)};
      const V3 h = ln.L3(o + DQ_H); const float ms = ln.L(o + DQ_M);
      const V3 lin = vi * ms + cross(wi, h), ang = mul(Io, wi) + cross(h, vi);
      int k = i;
      for (int j = i; j >= 0; j--) {
        float v = 0.f;
        if (j == k) {
          const int g = first + j, pj = ln.pll(g)[PLL_POSE]; const V3 axj = dq_axis(ln, g, ln.LR(pj));
          v = ln.li(g)[DG_LI_TYPE] == 0 ? dot(axj, ang) + dot(cross(ln.L3(pj + 6) - O, axj), lin) : dot(axj, lin);
          const int par = ln.li(g)[DG_LI_PARENT]; k = par < 0 ? -1 : par - first;
        }
        ln.L(Mo + i * (i + 1) / 2 + j) = v;
      }
    }
  }
  // ---- M = L L^T in place, each pivot held against FQ_PIVOT_FLOOR x its own diagonal entry (tq_cholesky<true>'s rule)
  bool hit = false;
  for (int j = 0; j < n; j++) {
    const int rj = Mo + j * (j + 1) / 2;
    float d = ln.L(rj + j); const float floor_ = FQ_PIVOT_FLOOR * d;
    for (int k = 0; k < j; k++) d -= ln.L(rj + k) * ln.L(rj + k);
    if (!(d > floor_)) { d = floor_; hit = true; }
    const float l = sqrtf(d), il = 1.f / l; ln.L(rj + j) = l;
    for (int i = j + 1; i < n; i++) {
      const int ri = Mo + i * (i + 1) / 2;
      float s = ln.L(ri + j); for (int k = 0; k < j; k++) s -= ln.L(ri + k) * ln.L(rj + k);
      ln.L(ri + j) = s * il;
    }
  }
  // ---- x <- (L L^T)^-1 x
  for (int i = 0; i < n; i++) {
    const int ri = Mo + i * (i + 1) / 2;
    float s = ln.L(xo + i); for (int k = 0; k < i; k++) s -= ln.L(ri + k) * ln.L(xo + k);
    ln.L(xo + i) = s / ln.L(ri + i);
  }
  for (int i = n - 1; i >= 0; i--) {
    float s = ln.L(xo + i); for (int k = i + 1; k < n; k++) s -= ln.L(Mo + k * (k + 1) / 2 + i) * ln.L(xo + k);
    ln.L(xo + i) = s / ln.L(Mo + i * (i + 1) / 2 + i);
  }
  return hit;
}

// qdd [num_envs][n], singular [num_envs] int32 (nullable); q, qd, tau [num_envs][n] or NULL = the env's own q, qd and zero torque
template <int LANES>
__global__ __launch_bounds__(64) void forward_dynamics_kernel(DevScene sc, MotorTable mt, float* state, int body, const float* q, const float* qd, const float* tau,
                                                               int damp, float* qdd, int32_t* singular, float* gws) {
  DG_DYNQ_LANE(false);
  const int qo = sc.tr_off, vo = qo + n, xo = vo + n, blk = xo + n;
  dq_stage(ln, first, n, q, DG_LS_Q, qo); dq_stage(ln, first, n, qd, DG_LS_QD, vo); dq_stage(ln, first, n, tau, -1, xo);
  ln.kinematics(body, qo);
  const bool sing = fq_solve(ln, body, first, n, vo, xo, blk, damp != 0);
  if (qdd) { float* out = qdd + (size_t)env * n; for (int i = 0; i < n; i++) out[i] = ln.L(xo + i); }
  if (singular) singular[env] = sing ? 1 : 0;
}

// tau [num_envs][K][T][n]; q0, qd0 [num_envs][n] or NULL = the env's own; q_out, qd_out [num_envs][K][T][n], pos_out
// [num_envs][K][T][3] (`frame`: the GLOBAL frame index, read only with pos_out), singular [num_envs][K] int32: each nullable
template <int LANES>
__global__ __launch_bounds__(64) void rollout_kernel(DevScene sc, MotorTable mt, float* state, int body, int frame, float lx, float ly, float lz, int K, int T, float dt,
                                                      int damp, const float* q0, const float* qd0, const float* tau, float* q_out, float* qd_out, float* pos_out,
                                                      int32_t* singular, float* gws) {
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  float* const ws = workspace_of<LANES>(sc, smem, gws, lane);  // this workgroup's and lane's column, for every item of the loop
  const size_t items = (size_t)sc.num_envs * (size_t)K;
  for (size_t item = (size_t)blockIdx.x * ACTIVE + lane; item < items; item += (size_t)gridDim.x * ACTIVE) {
    const int env = (int)(item / (size_t)K);
    Lane<LANES> ln(sc, mt, ws, state + env, env, false);  // env's state, read-only: its mass_scale applies
    const int first = ln.bi(body)[DG_BI_FIRST_LINK], n = ln.bi(body)[DG_BI_N_LINKS];
    const int qo = sc.tr_off, vo = qo + n, xo = vo + n, blk = xo + n;
    dq_stage(ln, first, n, q0, DG_LS_Q, qo); dq_stage(ln, first, n, qd0, DG_LS_QD, vo);
    ln.kinematics(body, qo);
    bool sing = false;
    for (int t = 0; t < T; t++) {
      const size_t row = item * (size_t)T + (size_t)t;
      const float* tr = tau + row * (size_t)n;
      for (int i = 0; i < n; i++) ln.L(xo + i) = tr[i];
      sing = fq_solve(ln, body, first, n, vo, xo, blk, damp != 0) || sing;
      float* qr = q_out ? q_out + row * (size_t)n : nullptr; float* vr = qd_out ? qd_out + row * (size_t)n : nullptr;
      for (int i = 0; i < n; i++) {  // semi-implicit, the step's order
        const float v = ln.L(vo + i) + dt * ln.L(xo + i), p = ln.L(qo + i) + dt * v;
        ln.L(vo + i) = v; ln.L(qo + i) = p;
        if (vr) vr[i] = v;
        if (qr) qr[i] = p;
      }
      if (t + 1 < T || pos_out) ln.kinematics(body, qo);  // the next step's pass; after the last step only for pos
      if (pos_out) {
        V3 fp, fv, fw; Q4 fq; ln.frame_state(body, frame, true, fp, fq, fv, fw, false);
        const V3 pw = fp + mul(qmat(fq), v3(lx, ly, lz));
        float* o = pos_out + row * 3; o[0] = pw.x; o[1] = pw.y; o[2] = pw.z;
      }
    }
    if (singular) singular[item] = sing ? 1 : 0;
  }
}

// rollout_kernel's frame (items, grid stride, workspace column, no cross-lane operation, size_t indices) with the torque of step t
// formed inside the loop from the state BEFORE the step:
//   tau = tau_ff[e][t] + alpha[k] dtau[e][t] + gain[e][t] . [q - q_ref[e][t]; qd - qd_ref[e][t]],  clamped to +-tau_limit[i] where that is > 0.
// tau_ff, dtau, q_ref, qd_ref [num_envs][T][n]; gain [num_envs][T][n][2 n] row-major, columns [q | qd]; alpha [K]; tau_limit [n].
// dtau (with alpha), gain (with q_ref, qd_ref) and tau_limit are nullable: the term is then absent, not zero, so the torque of a
// call without them is tau_ff to the bit.  The products are rounded one by one (no fused multiply-add across a term), so that
// tau_ff + alpha dtau is what the caller's own arithmetic gives.  The feedback sum reads q, qd from their kept slots and the gain
// row from global memory: fdq_slots(n) as for rollout_kernel.  Row t of tau_out is the torque applied in step t, after clamping;
// q_out, qd_out, pos_out, singular as rollout_kernel's.
template <int LANES>
__global__ __launch_bounds__(64) void rollout_feedback_kernel(DevScene sc, MotorTable mt, float* state, int body, int frame, float lx, float ly, float lz, int K, int T,
                                                               float dt, int damp, const float* q0, const float* qd0, const float* tau_ff, const float* dtau,
                                                               const float* alpha, const float* gain, const float* q_ref, const float* qd_ref, const float* tau_limit,
                                                               float* q_out, float* qd_out, float* tau_out, float* pos_out, int32_t* singular, float* gws) {
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  float* const ws = workspace_of<LANES>(sc, smem, gws, lane);  // this workgroup's and lane's column, for every item of the loop
  const size_t items = (size_t)sc.num_envs * (size_t)K;
  for (size_t item = (size_t)blockIdx.x * ACTIVE + lane; item < items; item += (size_t)gridDim.x * ACTIVE) {
    const int env = (int)(item / (size_t)K);
    Lane<LANES> ln(sc, mt, ws, state + env, env, false);  // env's state, read-only: its mass_scale applies
    const int first = ln.bi(body)[DG_BI_FIRST_LINK], n = ln.bi(body)[DG_BI_N_LINKS];
    const int qo = sc.tr_off, vo = qo + n, xo = vo + n, blk = xo + n;
    dq_stage(ln, first, n, q0, DG_LS_Q, qo); dq_stage(ln, first, n, qd0, DG_LS_QD, vo);
    ln.kinematics(body, qo);
    const float a = dtau ? alpha[item - (size_t)env * (size_t)K] : 0.f;
    bool sing = false;
    for (int t = 0; t < T; t++) {
      const size_t row = item * (size_t)T + (size_t)t, erow = ((size_t)env * (size_t)T + (size_t)t) * (size_t)n;
      float* ur = tau_out ? tau_out + row * (size_t)n : nullptr;
      for (int i = 0; i < n; i++) {  // q, qd stay in their slots; the torque goes to xo
        float u = tau_ff[erow + i];
        if (dtau) u = __fadd_rn(u, __fmul_rn(a, dtau[erow + i]));
        if (gain) {
          const float* g = gain + (erow + (size_t)i) * (size_t)(2 * n);
          float s = 0.f;
          for (int j = 0; j < n; j++) s = __fadd_rn(s, __fmul_rn(g[j], ln.L(qo + j) - q_ref[erow + j]));
          for (int j = 0; j < n; j++) s = __fadd_rn(s, __fmul_rn(g[n + j], ln.L(vo + j) - qd_ref[erow + j]));
          u = __fadd_rn(u, s);
        }
        if (tau_limit) { const float lim = tau_limit[i]; if (lim > 0.f) u = fminf(fmaxf(u, -lim), lim); }
        ln.L(xo + i) = u;
        if (ur) ur[i] = u;
      }
      sing = fq_solve(ln, body, first, n, vo, xo, blk, damp != 0) || sing;
      float* qr = q_out ? q_out + row * (size_t)n : nullptr; float* vr = qd_out ? qd_out + row * (size_t)n : nullptr;
      for (int i = 0; i < n; i++) {  // semi-implicit, the step's order
        const float v = ln.L(vo + i) + dt * ln.L(xo + i), p = ln.L(qo + i) + dt * v;
        ln.L(vo + i) = v; ln.L(qo + i) = p;
        if (vr) vr[i] = v;
        if (qr) qr[i] = p;
      }
      if (t + 1 < T || pos_out) ln.kinematics(body, qo);  // the next step's pass; after the last step only for pos
      if (pos_out) {
        V3 fp, fv, fw; Q4 fq; ln.frame_state(body, frame, true, fp, fq, fv, fw, false);
        const V3 pw = fp + mul(qmat(fq), v3(lx, ly, lz));
        float* o = pos_out + row * 3; o[0] = pw.x; o[1] = pw.y; o[2] = pw.z;
      }
    }
    if (singular) singular[item] = sing ? 1 : 0;
  }
}

}  // namespace dg
