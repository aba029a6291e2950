// dg_taskq.h -- batched task-space dynamics of one point of a fixed-base articulated body: what an operational-space (Cartesian
// impedance) controller needs per tick, in ONE launch.  For the task vector [v; w] of the point `lx ly lz` of the INERTIAL frame of
// `frame`'s link, in world axes, with the m rows the six bits of axes_mask select:
//   jac          J [m][n]                  the selected rows of the geometric Jacobian (jacobian_kernel's walk)
//   bias_acc     Jdot qd [m]               the point's acceleration at qdd = 0: the forward Newton-Euler pass, a_link + al x r +
//                                          w x (w x r) with the base's fictitious -g taken off again; the angular rows are al
//   bias_torque  h = C qd - G [n]          the backward pass: inverse_dynamics(q, qd, 0)
//   lambda       (J M^-1 J^T + damping I)^-1 [m][m]    Cholesky of M (composite rigid bodies), X = M^-1 J^T, A = J X + damping I,
//                                          Cholesky of A; each off-diagonal value is stored to both halves
//   tau          J^T Lambda (acc - Jdot qd) + h + (tau0 - J^T Lambda J M^-1 tau0) [n], evaluated as
//                J^T Lambda (acc - Jdot qd - J M^-1 tau0) + h + tau0: one solve with A
//   point        [p 3][quaternion of the link's inertial frame, xyzw 4][v 3][w 3]; the velocity rows are J qd
//   singular     1 when a pivot of either factorisation was <= TQ_PIVOT_FLOOR x the largest diagonal entry of the matrix factored
//                (M in its Jacobi-scaled form, see tq_cholesky); the pivot is then that floor, so every output stays finite
// The passes are this header's own copies of those in dg_dynq.h (statement for statement, qdd = 0), so dg_dynq.h and its kernels
// are as they were.  Conventions as there: one env per lane in the world's own workspace mode, wave-uniform (scalar) loads of the
// link tables, no lane talks to another, nothing allocated; q, qd NULL = the env's own, staged by dq_stage, so a NULL call and a
// call given the same numbers are the same bits.  Work is skipped by wave-uniform branches on the output pointers.
//
// Workspace: the transient region, nothing enlarged; matrices live in workspace slots, not in per-lane arrays.
//   kept throughout   [q n][qd n][J m n][h n][bias_acc m]                                   P = 3 n + m n + m
//   Newton-Euler      [DQ_ID_STRIDE per link]                                               P + 15 n
//   task inertia      [composite bodies DQ_CR_STRIDE per link, then X m n][M packed lower n (n + 1) / 2][A packed lower
//                     m (m + 1) / 2][right-hand side m][right-hand side n]                  P + 10 n + n (n + 1) / 2 + m (m + 1) / 2 + m + n
// taskq_slots() is the larger of the two; the planner's 12 + 32 n holds it for every 1 <= m <= min(6, n), n <= 12.
#pragma once
#include "dg_dynq.h"

namespace dg {

constexpr float TQ_PIVOT_FLOOR = 1e-5f;
constexpr int taskq_keep(int n, int m) { return 3 * n + m * n + m; }
constexpr int taskq_newton(int n, int m) { return DQ_ID_STRIDE * n; }
constexpr int taskq_inertia(int n, int m) { return DQ_CR_STRIDE * n + n * (n + 1) / 2 + m * (m + 1) / 2 + m + n; }
constexpr int taskq_slots(int n, int m) { return taskq_keep(n, m) + (taskq_newton(n, m) > taskq_inertia(n, m) ? taskq_newton(n, m) : taskq_inertia(n, m)); }

// component k of the task vector [t; r]
DGD float tq_comp(V3 t, V3 r, int k) { return k == 0 ? t.x : k == 1 ? t.y : k == 2 ? t.z : k == 3 ? r.x : k == 4 ? r.y : r.z; }

// In-place Cholesky factor (lower, packed row by row at `o`) of the symmetric positive matrix of order n stored there; a pivot
// <= TQ_PIVOT_FLOOR x the largest diagonal entry becomes that floor.  True: some pivot did.  OWN: the matrix is taken in its
// Jacobi-scaled form D^-1/2 M D^-1/2, D = diag M, whose diagonal is all ones -- pivot j is held against TQ_PIVOT_FLOOR x M[j][j]
// -- without the scaling ever being carried out: the factor stored is M's own.  That is how M is factored: the inertias its
// diagonal holds differ by more than the floor between an arm's shoulder and a gripper's finger (cond M = 1.4e6 on the twelve-joint
// UR5 + gripper), which says nothing about rank; the ratio pivot / M[j][j] -- the share of joint j's inertia that the joints before
// it do not account for -- does, whatever the units and sizes of the joints.
template <bool OWN, int LANES>
DGD bool tq_cholesky(const Lane<LANES>& ln, int o, int n) {
  float top = 0.f; for (int i = 0; i < n; i++) top = fmaxf(top, ln.L(o + i * (i + 1) / 2 + i));
  bool hit = false;
  for (int j = 0; j < n; j++) {
    const int rj = o + j * (j + 1) / 2;
    float d = ln.L(rj + j); const float floor_ = TQ_PIVOT_FLOOR * (OWN ? d : top);
    for (int k = 0; k < j; k++) d -= ln.L(rj + k) * ln.L(rj + k);
    if (!(d > floor_)) { d = floor_; hit = true; }
    const float l = sqrtf(d), il = 1.f / l; ln.L(rj + j) = l;
    for (int i = j + 1; i < n; i++) {
      const int ri = o + i * (i + 1) / 2;
      float s = ln.L(ri + j); for (int k = 0; k < j; k++) s -= ln.L(ri + k) * ln.L(rj + k);
      ln.L(ri + j) = s * il;
    }
  }
  return hit;
}
// x <- (L L^T)^-1 x for the n values at `x`, L the packed factor at `o`
template <int LANES>
DGD void tq_solve(const Lane<LANES>& ln, int o, int n, int x) {
  for (int i = 0; i < n; i++) {
    const int ri = o + i * (i + 1) / 2;
    float s = ln.L(x + i); for (int k = 0; k < i; k++) s -= ln.L(ri + k) * ln.L(x + k);
    ln.L(x + i) = s / ln.L(ri + i);
  }
  for (int i = n - 1; i >= 0; i--) {
    float s = ln.L(x + i); for (int k = i + 1; k < n; k++) s -= ln.L(o + k * (k + 1) / 2 + i) * ln.L(x + k);
    ln.L(x + i) = s / ln.L(o + i * (i + 1) / 2 + i);
  }
}

template <int LANES>
__global__ __launch_bounds__(64) void task_space_kernel(DevScene sc, MotorTable mt, float* state, int body, int frame, float lx, float ly, float lz, int axes_mask,
                                                         const float* q, const float* qd, const float* acc, const float* tau_null, float damping,
                                                         float* jac, float* bias_acc, float* bias_torque, float* lambda, float* tau, float* point,
                                                         int32_t* singular, float* gws) {
  DG_DYNQ_LANE(false);
  const int m = __popc((unsigned)axes_mask);
  const int qo = sc.tr_off, vo = qo + n, Jo = vo + n, ho = Jo + m * n, bo = ho + n, blk = bo + m;
  dq_stage(ln, first, n, q, DG_LS_Q, qo); dq_stage(ln, first, n, qd, DG_LS_QD, vo);
  ln.kinematics(body, qo);
  V3 fp, fv, fw; Q4 fq; ln.frame_state(body, frame, true, fp, fq, fv, fw, false);
  const V3 pw = fp + mul(qmat(fq), v3(lx, ly, lz));
  const int fl = sc.FI[frame * DG_FI_STRIDE + DG_FI_LINK];  // the frame's link (-1: rigidly on the base)
  const V3 zero = v3(0.f, 0.f, 0.f);
  // ---- the Jacobian's selected rows into the slots (and out), the point's velocity J qd on the way
  {
    float* jo = jac ? jac + (size_t)env * m * n : nullptr;
    V3 pv = zero, pwv = zero;
    int k = fl < 0 ? -1 : fl - first;  // the next ancestor (or the link itself) on the way down to the root
    for (int j = n - 1; j >= 0; j--) {
      V3 ct = zero, cr = ct;
      if (j == k) {
        const int g = first + j, po = ln.pll(g)[PLL_POSE]; const V3 axw = dq_axis(ln, g, ln.LR(po));
        if (ln.li(g)[DG_LI_TYPE] == 0) { ct = cross(axw, pw - ln.L3(po + 6)); cr = axw; } else ct = axw;
        const int par = ln.li(g)[DG_LI_PARENT]; k = par < 0 ? -1 : par - first;
        const float qdj = ln.L(vo + j); pv = pv + ct * qdj; pwv = pwv + cr * qdj;
      }
      for (int a = 0, r = 0; a < 6; a++) {
        if (!((axes_mask >> a) & 1)) continue;
        const float c = tq_comp(ct, cr, a); ln.L(Jo + r * n + j) = c; if (jo) jo[r * n + j] = c;
        r++;
      }
    }
    if (point) {
      float* o = point + (size_t)env * 13;
      o[0] = pw.x; o[1] = pw.y; o[2] = pw.z; o[3] = fq.x; o[4] = fq.y; o[5] = fq.z; o[6] = fq.w;
      o[7] = pv.x; o[8] = pv.y; o[9] = pv.z; o[10] = pwv.x; o[11] = pwv.y; o[12] = pwv.z;
    }
  }
  // ---- recursive Newton-Euler at qdd = 0 (inverse_dynamics_kernel's passes): Jdot qd from the forward one, h from the backward one
  if (bias_acc || bias_torque || tau) {
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
    {  // the point rides on link fl: its acceleration with the base's -g taken off, and the link's angular acceleration
      V3 at = zero, ar = zero;
      if (fl >= 0) {
        const int o = blk + (fl - first) * DQ_ID_STRIDE; const V3 w = ln.L3(o + DQ_W), r = pw - ln.L3(ln.pll(fl)[PLL_POSE] + 6);
        ar = ln.L3(o + DQ_AL); at = ln.L3(o + DQ_A) + cross(ar, r) + cross(w, cross(w, r)) + g;
      }
      float* out = bias_acc ? bias_acc + (size_t)env * m : nullptr;
      for (int a = 0, r = 0; a < 6; a++) {
        if (!((axes_mask >> a) & 1)) continue;
        const float c = tq_comp(at, ar, a); ln.L(bo + r) = c; if (out) out[r] = c;
        r++;
      }
    }
    float* out = bias_torque ? bias_torque + (size_t)env * n : nullptr;
    for (int i = n - 1; i >= 0; i--) {  // tip to root
      const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_ID_STRIDE;
      const V3 f = ln.L3(o + DQ_F), nn = ln.L3(o + DQ_N), axw = dq_axis(ln, gl, ln.LR(po));
      const float hi = ln.li(gl)[DG_LI_TYPE] == 0 ? dot(axw, nn) : dot(axw, f);
      ln.L(ho + i) = hi; if (out) out[i] = hi;
      if (par >= 0) {
        const int op = blk + (par - first) * DQ_ID_STRIDE; const V3 r = ln.L3(po + 6) - ln.L3(ln.pll(par)[PLL_POSE] + 6);
        ln.L3set(op + DQ_F, ln.L3(op + DQ_F) + f); ln.L3set(op + DQ_N, ln.L3(op + DQ_N) + nn + cross(r, f));
      }
    }
  }
  if (!lambda && !tau && !singular) return;
  // ---- M by composite rigid bodies (mass_matrix_kernel's passes), packed lower
  const int Xo = blk, Mo = blk + DQ_CR_STRIDE * n, Ao = Mo + n * (n + 1) / 2, yo = Ao + m * (m + 1) / 2, zo = yo + m;
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
  // ---- M = L L^T; X = M^-1 J^T row by row over the dead composite bodies; A = J X + damping I; A = L L^T
  bool sing = tq_cholesky<true>(ln, Mo, n);
  for (int r = 0; r < m; r++) {
    for (int j = 0; j < n; j++) ln.L(Xo + r * n + j) = ln.L(Jo + r * n + j);
    tq_solve(ln, Mo, n, Xo + r * n);
  }
  for (int r = 0; r < m; r++)
    for (int s = 0; s <= r; s++) {
      float v = r == s ? damping : 0.f; for (int j = 0; j < n; j++) v += ln.L(Jo + r * n + j) * ln.L(Xo + s * n + j);
      ln.L(Ao + r * (r + 1) / 2 + s) = v;
    }
  sing = tq_cholesky<false>(ln, Ao, m) || sing;
  if (singular) singular[env] = sing ? 1 : 0;
  if (lambda) {  // column by column; each value to both halves
    float* out = lambda + (size_t)env * m * m;
    for (int c = 0; c < m; c++) {
      for (int r = 0; r < m; r++) ln.L(yo + r) = r == c ? 1.f : 0.f;
      tq_solve(ln, Ao, m, yo);
      for (int r = c; r < m; r++) { const float v = ln.L(yo + r); out[r * m + c] = v; out[c * m + r] = v; }
    }
  }
  if (tau) {
    const float* ar = acc + (size_t)env * m; const float* t0 = tau_null ? tau_null + (size_t)env * n : nullptr;
    for (int r = 0; r < m; r++) ln.L(yo + r) = ar[r] - ln.L(bo + r);
    if (t0) {  // the null-space torque's own task acceleration J M^-1 tau0 comes off the demand
      for (int j = 0; j < n; j++) ln.L(zo + j) = t0[j];
      tq_solve(ln, Mo, n, zo);
      for (int r = 0; r < m; r++) { float u = 0.f; for (int j = 0; j < n; j++) u += ln.L(Jo + r * n + j) * ln.L(zo + j); ln.L(yo + r) -= u; }
    }
    tq_solve(ln, Ao, m, yo);
    float* out = tau + (size_t)env * n;
    for (int j = 0; j < n; j++) {
      float v = ln.L(ho + j) + (t0 ? t0[j] : 0.f); for (int r = 0; r < m; r++) v += ln.L(Jo + r * n + j) * ln.L(yo + r);
      out[j] = v;
    }
  }
}

}  // namespace dg
