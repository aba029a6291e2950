// dg_ddq.h -- batched derivatives of the forward dynamics of a fixed-base articulated body, at P points per env in one launch:
//   dynamics_derivatives_kernel   one work item per (env e, point p), B x P in all.  With d the joints' URDF damping when `damp`
//                                 is set, else zero, and ID the rigid-body inverse dynamics of inverse_dynamics_kernel:
//     qdd      = M^-1 (tau - d o qd - h(q, qd))            fq_solve's result, bit for bit, with its pivot-floor rule and flag
//     dtau_dq  [i][j] = d ID_i(q, qd, qdd) / d q_j         at FIXED qdd
//     dtau_dqd [i][j] = d ID_i / d qd_j + d_i delta_ij
//     dqdd_dq  = -M^-1 dtau_dq,   dqdd_dqd = -M^-1 dtau_dqd,   dqdd_dtau = M^-1
// The derivatives are ANALYTIC: a forward-mode tangent of the Newton-Euler passes of fq_solve, one sweep per column (dd_sweep).
// Tangent rules, in world coordinates.  For a revolute joint j with world axis s at p_j every link i of j's subtree (j included)
// turns about that axis: R_i' = [s]x R_i, p_i' = s x (p_i - p_j), hence axw_i' = s x axw_i, (R_i c)' = s x (R_i c) and
// (R Ic R^T x)' = R Ic R^T x' + s x (R Ic R^T x) - R Ic R^T (s x x).  For a prismatic joint j the subtree slides: R_i' = 0,
// p_i' = s.  Links outside the subtree do not move.  The qd_j tangent leaves the geometry alone and seeds sv_j' = axw_j.  Every
// statement of the two loops is differentiated, the axw_i' . n_i term of the projection included.
//
// Phases and workspace: the transient region, nothing enlarged.
//   (A) fq_solve for qdd                                            [q n][qd n][x n] + fdq_newton / fdq_inertia
//   (B0) the point the tangents are taken at.  fq_solve builds M by composite bodies about the BASE origin, which costs a small distal
//       link (a gripper finger of 1e-6 kg m^2 a metre out) digits by cancellation: the twelve-joint gripper tree's qdd is 2.7e-4 off
//       relative to its largest entry, and dtau_dq = d ID(q, qd, qdd) / dq, which there is d(M qdd)/dq almost alone, would carry that
//       error undivided.  So the nominal pass runs once at fq_solve's qdd, its projected torques give the residual
//       r = tau - d o qd - ID(q, qd, qdd) -- Newton-Euler about each link's own origin, no such cancellation -- and
//       qdd += (L L^T)^-1 r with the rebuilt factor: one step of iterative refinement.  The OUTPUT qdd stays fq_solve's, bit for bit.
//                                                                    [q n][qd n][qdd n][composite 10 n][M packed][.. residual n at the end]
//   (B) the nominal pass again at that qdd, blocks kept (F, N summed tip to root), then the 2 n tangent sweeps, each writing its raw
//       dtau column straight into the item's own rows of the output     [q n][qd n][qdd n][nominal 15 n][tangent 15 n]
//   (C) M and its Cholesky factor rebuilt over the dead blocks (dd_factor: fq_solve's statements); each raw column read back from the
//       item's own rows -- the lane's own stores, no fence needed -- solved in the n slots qdd left and stored negated; n unit
//       columns for M^-1                                            [q n][qd n][column n][composite 10 n][M packed n (n + 1) / 2]
// The raw columns go to dtau_* when that output is wanted, else to dqdd_*, which phase (C) then overwrites in place.
// ddq_slots() is 3 n + the largest phase = 33 n for every n <= 37; the planner's 12 + 32 n holds it for every n <= 12.
//
// GRID AND WORKSPACE: rollout_kernel's (dg_fdq.h).  A grid-stride loop over the items on the workspace column of the item's OWN
// workgroup and lane; the C entry caps the grid at the step's grid in the global-workspace modes.  No cross-lane operation anywhere
// (the lanes leave the loop after different trip counts); the subtree mask of a sweep is wave-uniform.  Every output index is a
// size_t.
#pragma once
#include "dg_fdq.h"

namespace dg {

constexpr int DDQ_MAX_JOINTS = 64;  // the subtree mask of a sweep is one 64-bit word
constexpr int ddq_keep(int n) { return 3 * n; }
constexpr int ddq_tangent(int n) { return 2 * DQ_ID_STRIDE * n; }
constexpr int ddq_refine(int n) { return fdq_inertia(n) + n; }  // the factor with the residual behind it
constexpr int ddq_slots(int n) { return ddq_keep(n) + (ddq_tangent(n) > ddq_refine(n) ? ddq_tangent(n) : ddq_refine(n)); }

// the nominal Newton-Euler pass at the q staged (kinematics done), the qd at vo and the qdd at ao; blocks of DQ_ID_STRIDE at blk,
// F and N summed tip to root: what the tangent sweeps read
template <int LANES>
DGD void dd_nominal(const Lane<LANES>& ln, int first, int n, int vo, int ao, int blk) {
  const DevScene& sc = ln.sc;
  const V3 zero = v3(0.f, 0.f, 0.f), g = v3(sc.gx, sc.gy, sc.gz);
  for (int i = 0; i < n; i++) {  // root to tip
    const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_ID_STRIDE;
    const M3 R = ln.LR(po); const V3 p = ln.L3(po + 6), axw = dq_axis(ln, gl, R);
    const float qdi = ln.L(vo + i), qddi = ln.L(ao + i);
    V3 wp = zero, alp = zero, ap = -g, r = zero;
    if (par >= 0) { const int op = blk + (par - first) * DQ_ID_STRIDE; wp = ln.L3(op + DQ_W); alp = ln.L3(op + DQ_AL); ap = ln.L3(op + DQ_A); r = p - ln.L3(ln.pll(par)[PLL_POSE] + 6); }
    V3 w = wp, al = alp, a = ap + cross(alp, r) + cross(wp, cross(wp, r));
    const V3 sv = axw * qdi, cv = cross(wp, sv);
    if (ln.li(gl)[DG_LI_TYPE] == 0) { w = wp + sv; al = alp + axw * qddi + cv; }
    else a = a + axw * qddi + cv * 2.f;
    float ms; V3 c; Sym3 Ic; ln.link_inertia(gl, ms, c, Ic);
    const V3 cw = mul(R, c), ac = a + cross(al, cw) + cross(w, cross(w, cw)), F = ac * ms;
    const V3 N = dq_rot_inertia(R, Ic, al) + cross(w, dq_rot_inertia(R, Ic, w)) + cross(cw, F);
    ln.L3set(o + DQ_W, w); ln.L3set(o + DQ_AL, al); ln.L3set(o + DQ_A, a); ln.L3set(o + DQ_F, F); ln.L3set(o + DQ_N, N);
  }
  for (int i = n - 1; i >= 0; i--) {  // tip to root
    const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT]; if (par < 0) continue;
    const int po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_ID_STRIDE, op = blk + (par - first) * DQ_ID_STRIDE;
    const V3 f = ln.L3(o + DQ_F), nn = ln.L3(o + DQ_N), r = ln.L3(po + 6) - ln.L3(ln.pll(par)[PLL_POSE] + 6);
    ln.L3set(op + DQ_F, ln.L3(op + DQ_F) + f); ln.L3set(op + DQ_N, ln.L3(op + DQ_N) + nn + cross(r, f));
  }
}

// One tangent sweep: column j of d ID / d q (wrt_qd false) or of d ID / d qd (wrt_qd true) at fixed qdd, written to col[i * n] for
// i = 0 .. n-1 (`col` points at element [0][j] of the item's row-major [n][n] matrix); `diag` is added to entry j (the damping).
// nom: dd_nominal's blocks; tan: DQ_ID_STRIDE x n slots of scratch.
template <int LANES>
DGD void dd_sweep(const Lane<LANES>& ln, int first, int n, int vo, int ao, int nom, int tan, int j, bool wrt_qd, float diag, float* col) {
  const V3 zero = v3(0.f, 0.f, 0.f);
  const int gj = first + j, pj = ln.pll(gj)[PLL_POSE];
  const bool revj = ln.li(gj)[DG_LI_TYPE] == 0;
  const V3 s = dq_axis(ln, gj, ln.LR(pj)), Pj = ln.L3(pj + 6);
  uint64_t sub = 0;  // links of j's subtree, j included: the links joint j moves (none for a qd tangent); wave-uniform
  for (int i = 0; i < n; i++) {  // root to tip
    const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = nom + i * DQ_ID_STRIDE, ot = tan + i * DQ_ID_STRIDE;
    const int ip = par < 0 ? -1 : par - first;
    const bool in = !wrt_qd && (i == j || (ip >= 0 && ((sub >> ip) & 1))), inp = ip >= 0 && ((sub >> ip) & 1);
    if (in) sub |= (uint64_t)1 << i;
    const bool turn = in && revj;  // the link turns about s
    const M3 R = ln.LR(po); const V3 p = ln.L3(po + 6), axw = dq_axis(ln, gl, R);
    const float qdi = ln.L(vo + i), qddi = ln.L(ao + i);
    const bool rev = ln.li(gl)[DG_LI_TYPE] == 0;
    const V3 w = ln.L3(o + DQ_W), al = ln.L3(o + DQ_AL), a = ln.L3(o + DQ_A);
    V3 wp = zero, alp = zero, r = zero, dwp = zero, dalp = zero, dap = zero, dr = zero;
    if (par >= 0) {
      const int op = nom + ip * DQ_ID_STRIDE, opt = tan + ip * DQ_ID_STRIDE; const V3 pp = ln.L3(ln.pll(par)[PLL_POSE] + 6);
      wp = ln.L3(op + DQ_W); alp = ln.L3(op + DQ_AL); r = p - pp;
      dwp = ln.L3(opt + DQ_W); dalp = ln.L3(opt + DQ_AL); dap = ln.L3(opt + DQ_A);
      const V3 dp = in ? (revj ? cross(s, p - Pj) : s) : zero, dpp = inp ? (revj ? cross(s, pp - Pj) : s) : zero;
      dr = dp - dpp;
    }
    const V3 daxw = turn ? cross(s, axw) : zero;
    V3 dw = dwp, dal = dalp;
    V3 da = dap + cross(dalp, r) + cross(alp, dr) + cross(dwp, cross(wp, r)) + cross(wp, cross(dwp, r) + cross(wp, dr));
    const V3 sv = axw * qdi, dsv = daxw * qdi + (wrt_qd && i == j ? axw : zero), dcv = cross(dwp, sv) + cross(wp, dsv);
    if (rev) { dw = dwp + dsv; dal = dalp + daxw * qddi + dcv; }
    else da = da + daxw * qddi + dcv * 2.f;
    float ms; V3 c; Sym3 Ic; ln.link_inertia(gl, ms, c, Ic);
    const V3 cw = mul(R, c), dcw = turn ? cross(s, cw) : zero;
    const V3 wcw = cross(w, cw), ac = a + cross(al, cw) + cross(w, wcw), F = ac * ms;
    const V3 dac = da + cross(dal, cw) + cross(al, dcw) + cross(dw, wcw) + cross(w, cross(dw, cw) + cross(w, dcw)), dF = dac * ms;
    const V3 Iw = dq_rot_inertia(R, Ic, w);
    V3 dIal = dq_rot_inertia(R, Ic, dal), dIw = dq_rot_inertia(R, Ic, dw);
    if (turn) {
      dIal = dIal + cross(s, dq_rot_inertia(R, Ic, al)) - dq_rot_inertia(R, Ic, cross(s, al));
      dIw = dIw + cross(s, Iw) - dq_rot_inertia(R, Ic, cross(s, w));
    }
    const V3 dN = dIal + cross(dw, Iw) + cross(w, dIw) + cross(dcw, F) + cross(cw, dF);
    ln.L3set(ot + DQ_W, dw); ln.L3set(ot + DQ_AL, dal); ln.L3set(ot + DQ_A, da); ln.L3set(ot + DQ_F, dF); ln.L3set(ot + DQ_N, dN);
  }
  for (int i = n - 1; i >= 0; i--) {  // tip to root; the nominal f, n are the subtree sums dd_nominal left
    const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = nom + i * DQ_ID_STRIDE, ot = tan + i * DQ_ID_STRIDE;
    const bool in = (sub >> i) & 1;
    const V3 f = ln.L3(o + DQ_F), nn = ln.L3(o + DQ_N), df = ln.L3(ot + DQ_F), dn = ln.L3(ot + DQ_N), axw = dq_axis(ln, gl, ln.LR(po));
    const V3 daxw = in && revj ? cross(s, axw) : zero;
    float t = ln.li(gl)[DG_LI_TYPE] == 0 ? dot(daxw, nn) + dot(axw, dn) : dot(daxw, f) + dot(axw, df);
    if (i == j) t += diag;
    col[(size_t)i * (size_t)n] = t;
    if (par >= 0) {
      const int ip = par - first, opt = tan + ip * DQ_ID_STRIDE; const bool inp = (sub >> ip) & 1;
      const V3 p = ln.L3(po + 6), pp = ln.L3(ln.pll(par)[PLL_POSE] + 6), r = p - pp;
      const V3 dp = in ? (revj ? cross(s, p - Pj) : s) : zero, dpp = inp ? (revj ? cross(s, pp - Pj) : s) : zero, dr = dp - dpp;
      ln.L3set(opt + DQ_F, ln.L3(opt + DQ_F) + df); ln.L3set(opt + DQ_N, ln.L3(opt + DQ_N) + dn + cross(dr, f) + cross(r, df));
    }
  }
}

// M by composite rigid bodies, packed lower at blk + DQ_CR_STRIDE n, and its Cholesky factor in place: fq_solve's statements, pivot
// floor rule included (so the factor is the one qdd was solved with)
template <int LANES>
DGD int dd_factor(const Lane<LANES>& ln, int body, int first, int n, int blk) {
  const V3 zero = v3(0.f, 0.f, 0.f);
  const int Mo = blk + DQ_CR_STRIDE * n;
  const V3 O = ln.base_pos(body);
  for (int i = 0; i < n; i++) {
    const int gl = first + i, po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_CR_STRIDE;
    const M3 R = ln.LR(po); float ms; V3 c; Sym3 Ic; ln.link_inertia(gl, ms, c, Ic);
    const V3 cw = (ln.L3(po + 6) - O) + mul(R, c); const float cc = dot(cw, cw);
    const Sym3 Iw = symmetrize(mul(mul(R, full(Ic)), transpose(R)));
    ln.L(o + DQ_I) = Iw.xx + ms * (cc - cw.x * cw.x); ln.L(o + DQ_I + 1) = Iw.xy - ms * cw.x * cw.y; ln.L(o + DQ_I + 2) = Iw.xz - ms * cw.x * cw.z;
    ln.L(o + DQ_I + 3) = Iw.yy + ms * (cc - cw.y * cw.y); ln.L(o + DQ_I + 4) = Iw.yz - ms * cw.y * cw.z; ln.L(o + DQ_I + 5) = Iw.zz + ms * (cc - cw.z * cw.z);
    ln.L3set(o + DQ_H, cw * ms); ln.L(o + DQ_M) = ms;
  }
  for (int i = n - 1; i >= 0; i--) {
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
  for (int j = 0; j < n; j++) {
    const int rj = Mo + j * (j + 1) / 2;
    float d = ln.L(rj + j); const float floor_ = FQ_PIVOT_FLOOR * d;
    for (int k = 0; k < j; k++) d -= ln.L(rj + k) * ln.L(rj + k);
    if (!(d > floor_)) d = floor_;
    const float l = sqrtf(d), il = 1.f / l; ln.L(rj + j) = l;
    for (int i = j + 1; i < n; i++) {
      const int ri = Mo + i * (i + 1) / 2;
      float s = ln.L(ri + j); for (int k = 0; k < j; k++) s -= ln.L(ri + k) * ln.L(rj + k);
      ln.L(ri + j) = s * il;
    }
  }
  return Mo;
}

// the n slots at xo <- (L L^T)^-1 of them (fq_solve's two triangular solves)
template <int LANES>
DGD void dd_solve(const Lane<LANES>& ln, int n, int Mo, int xo) {
  for (int i = 0; i < n; i++) {
    const int ri = Mo + i * (i + 1) / 2;
    float s = ln.L(xo + i); for (int k = 0; k < i; k++) s -= ln.L(ri + k) * ln.L(xo + k);
    ln.L(xo + i) = s / ln.L(ri + i);
  }
  for (int i = n - 1; i >= 0; i--) {
    float s = ln.L(xo + i); for (int k = i + 1; k < n; k++) s -= ln.L(Mo + k * (k + 1) / 2 + i) * ln.L(xo + k);
    ln.L(xo + i) = s / ln.L(Mo + i * (i + 1) / 2 + i);
  }
}

// n joint values of item `item` into the slots at `off`: the caller's row [item][n], else the env's state column `field`, else zero
template <int LANES>
DGD void dd_stage(const Lane<LANES>& ln, int first, int n, const float* src, size_t item, int field, int off) {
  const float* row = src ? src + item * (size_t)n : nullptr;
  for (int i = 0; i < n; i++) ln.L(off + i) = row ? row[i] : field >= 0 ? ln.S(ln.li(first + i)[DG_LI_STATE_OFF] + field) : 0.f;
}

// q, qd, tau [num_envs][P][n] or NULL = the env's own q, qd and zero torque at every point of that env; qdd [num_envs][P][n], the five
// matrices [num_envs][P][n][n] row-major, singular [num_envs][P] int32: each nullable
template <int LANES>
__global__ __launch_bounds__(64) void dynamics_derivatives_kernel(DevScene sc, MotorTable mt, float* state, int body, int P, const float* q, const float* qd, const float* tau,
                                                                   int damp, float* qdd, float* dqdd_dq, float* dqdd_dqd, float* dqdd_dtau, float* dtau_dq, float* dtau_dqd,
                                                                   int32_t* singular, float* gws) {
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  float* const ws = workspace_of<LANES>(sc, smem, gws, lane);  // this workgroup's and lane's column, for every item of the loop
  const size_t items = (size_t)sc.num_envs * (size_t)P;
  for (size_t item = (size_t)blockIdx.x * ACTIVE + lane; item < items; item += (size_t)gridDim.x * ACTIVE) {
    const int env = (int)(item / (size_t)P);
    Lane<LANES> ln(sc, mt, ws, state + env, env, false);  // env's state, read-only: its mass_scale applies
    const int first = ln.bi(body)[DG_BI_FIRST_LINK], n = ln.bi(body)[DG_BI_N_LINKS];
    const int qo = sc.tr_off, vo = qo + n, xo = vo + n, blk = xo + n, tan = blk + DQ_ID_STRIDE * n;
    const size_t nn = (size_t)n * (size_t)n;
    dd_stage(ln, first, n, q, item, DG_LS_Q, qo); dd_stage(ln, first, n, qd, item, DG_LS_QD, vo); dd_stage(ln, first, n, tau, item, -1, xo);
    ln.kinematics(body, qo);
    // (A)
    const bool sing = fq_solve(ln, body, first, n, vo, xo, blk, damp != 0);
    if (qdd) { float* out = qdd + item * (size_t)n; for (int i = 0; i < n; i++) out[i] = ln.L(xo + i); }
    if (singular) singular[item] = sing ? 1 : 0;
    // (B) raw columns into dtau_*, else into dqdd_*
    float* const raw_q = dtau_dq ? dtau_dq + item * nn : dqdd_dq ? dqdd_dq + item * nn : nullptr;
    float* const raw_v = dtau_dqd ? dtau_dqd + item * nn : dqdd_dqd ? dqdd_dqd + item * nn : nullptr;
    if (raw_q || raw_v) {
      // the point the tangents are taken at: qdd once refined against the Newton-Euler residual (see the header); the output qdd stays
      // fq_solve's
      dd_nominal(ln, first, n, vo, xo, blk);
      const int ro = blk + (ddq_tangent(n) > ddq_refine(n) ? ddq_tangent(n) : ddq_refine(n)) - n;
      for (int i = 0; i < n; i++) {
        const int gl = first + i, o = blk + i * DQ_ID_STRIDE; const V3 axw = dq_axis(ln, gl, ln.LR(ln.pll(gl)[PLL_POSE]));
        const float ti = ln.li(gl)[DG_LI_TYPE] == 0 ? dot(axw, ln.L3(o + DQ_N)) : dot(axw, ln.L3(o + DQ_F));
        float t = tau ? tau[item * (size_t)n + i] : 0.f; if (damp) t -= ln.lf(gl)[DG_LF_DAMPING] * ln.L(vo + i);
        ln.L(ro + i) = t - ti;
      }
      dd_solve(ln, n, dd_factor(ln, body, first, n, blk), ro);
      for (int i = 0; i < n; i++) ln.L(xo + i) += ln.L(ro + i);
      dd_nominal(ln, first, n, vo, xo, blk);
      for (int j = 0; j < n; j++) {
        if (raw_q) dd_sweep(ln, first, n, vo, xo, blk, tan, j, false, 0.f, raw_q + j);
        if (raw_v) dd_sweep(ln, first, n, vo, xo, blk, tan, j, true, damp ? ln.lf(first + j)[DG_LF_DAMPING] : 0.f, raw_v + j);
      }
    }
    // (C)
    if (dqdd_dq || dqdd_dqd || dqdd_dtau) {
      const int Mo = dd_factor(ln, body, first, n, blk);
      for (int m = 0; m < 2; m++) {
        const float* const raw = m == 0 ? raw_q : raw_v; float* const out = m == 0 ? dqdd_dq : dqdd_dqd;
        if (!out) continue;
        float* const o = out + item * nn;
        for (int j = 0; j < n; j++) {
          for (int i = 0; i < n; i++) ln.L(xo + i) = raw[(size_t)i * (size_t)n + j];
          dd_solve(ln, n, Mo, xo);
          for (int i = 0; i < n; i++) o[(size_t)i * (size_t)n + j] = -ln.L(xo + i);
        }
      }
      if (dqdd_dtau) {
        float* const o = dqdd_dtau + item * nn;
        for (int j = 0; j < n; j++) {
          for (int i = 0; i < n; i++) ln.L(xo + i) = i == j ? 1.f : 0.f;
          dd_solve(ln, n, Mo, xo);
          for (int i = 0; i < n; i++) o[(size_t)i * (size_t)n + j] = ln.L(xo + i);
        }
      }
    }
  }
}

}  // namespace dg
