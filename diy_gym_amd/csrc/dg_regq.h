// dg_regq.h -- the inertial parameters of a fixed-base articulated body and the regressor of its inverse dynamics:
//   inertial_params_kernel   one env per lane: theta [num_envs][n][10], per link (joint index l = 0 .. n-1) in the link's OWN frame
//                            (PLL_POSE)  theta_l = [m, m cx, m cy, m cz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz]  with c the centre of mass and I
//                            the inertia about the link-frame ORIGIN in link axes, I = Ic + m (c.c 1 - c c^T), Ic as link_inertia
//                            returns it (the env's mass scale on mass and Ic, hence on all ten); `nominal`: the unscaled table values;
//   id_regressor_kernel      one work item per (env e, point p), B x P in all.  Inverse dynamics is linear in theta:
//                              tau = Y(q, qd, qdd) theta,   Y [n][10 n]
//                            and with a reference velocity qd_ref (Slotine-Li)  Y theta = M qdd + C(q, qd) qd_ref - G  for the
//                            Christoffel C, whose product is symmetric in (qd, qd_ref); qd_ref = qd is the plain regressor.
// World coordinates like inverse_dynamics_kernel.  Root-to-tip pass, carrying w, w_r, al, a per link (the base at rest, a = -g):
//   a  = a_p + al_p x r + 1/2 (w_p x (w_rp x r) + w_rp x (w_p x r))
//   cv = 1/2 (w_p x axw qd_ref_i + w_rp x axw qd_i)
//   revolute:  al = al_p + axw qdd_i + cv,  w = w_p + axw qd_i,  w_r = w_rp + axw qd_ref_i;     prismatic:  a += axw qdd_i + 2 cv
// -- with qd_ref = qd inverse_dynamics_kernel's pass.  Per link j, with w, w_r, al, a rotated into link axes by R_j^T, the 6 x 10 matrix
// A_j maps theta_j to force and moment about the link origin in link axes ([x] the cross-product matrix, L(v) vec(I) = I v):
//   force  rows:  column 0  a;   columns 1..3  [al] + 1/2 ([w][w_r] + [w_r][w]);   columns 4..9  0
//   moment rows:  column 0  0;   columns 1..3  -[a];                              columns 4..9  L(al) + 1/2 ([w] L(w_r) + [w_r] L(w))
// A_j is never formed: u^T A_j for a 6-vector u = [uf; um] is ten cross and dot products (rq_row).
//   Y     for every ancestor joint i of j (j included; the cursor of jacobian_kernel and mass_matrix_kernel, wave-uniform)
//         Y[i][10 j .. 10 j + 9] = u^T A_j with u = [R_j^T (axw_i x (p_j - p_i)); R_j^T axw_i] for a revolute i, [R_j^T axw_i; 0] for a
//         prismatic one; every other block is written as zeros (the buffer is reused);
//   tau   = Y theta_hat (theta_hat [num_envs][10 n], per env) without Y: each link's force and moment A_j theta_hat_j, then the
//         tip-to-root sum and projection of inverse_dynamics_kernel: O(n);
//   grad  = Y^T s (s [item][n]) without Y: a second root-to-tip pass with joint rates s gives each link's virtual twist (v_s at p_j,
//         w_s), and grad_j = A_j^T [R_j^T v_s; R_j^T w_s]: O(n).
// Workspace: the transient region, [q n][qd n][qd_ref n][qdd n][s n] then RQ_STRIDE per link ([w 3][w_r 3][al 3][a 3] and six for force
// and moment, then for the virtual twist): regq_slots(n) = 23 n, below the planner's 12 + 32 n for every n.
// GRID AND WORKSPACE: dynamics_derivatives_kernel's (dg_ddq.h).  No cross-lane operation; every output index is a size_t.  A lane
// writes its own item's rows; a block of ten floats starts 8-byte aligned (an item is 40 n^2 bytes, a row 40 n, a block 40) and goes
// out as five 8-byte stores; the C entries refuse an output pointer that is not 8-byte aligned.  Y goes column block by column block
// (j outermost).  Row by row (i outermost, a lane's stores running through 40 n contiguous bytes, the carried links flagged parent
// first) was tried and measured SLOWER on an MI355X, 0.0307 against 0.0275 ms at 16 384 items of six joints and 0.2188 against 0.1929 ms
// at 131 072: DESIGN "Inverse-dynamics regressor".
#pragma once
#include "dg_ddq.h"

namespace dg {

enum { RQ_W = 0, RQ_WR = 3, RQ_AL = 6, RQ_A = 9, RQ_F = 12, RQ_N = 15, RQ_STRIDE = 18 };
constexpr int regq_slots(int n) { return 5 * n + RQ_STRIDE * n; }

// ten floats at an 8-byte aligned address
DGD void rq_store10(float* p, const float* v) {
  float2* o = reinterpret_cast<float2*>(p);
  _Pragma("unroll") for (int k = 0; k < 5; k++) o[k] = make_float2(v[2 * k], v[2 * k + 1]);
}
// x^T L(v): the coefficients of vec(I) (Sym3's order) in x . I v
DGD void rq_sym6(V3 x, V3 v, float s, float* o) {
  o[0] += s * x.x * v.x; o[1] += s * (x.x * v.y + x.y * v.x); o[2] += s * (x.x * v.z + x.z * v.x);
  o[3] += s * x.y * v.y; o[4] += s * (x.y * v.z + x.z * v.y); o[5] += s * x.z * v.z;
}
// out[10] = [uf; um]^T A(w, wr, al, a), every vector in link axes
DGD void rq_row(V3 uf, V3 um, V3 w, V3 wr, V3 al, V3 a, float* out) {
  out[0] = dot(uf, a);
  const V3 umw = cross(um, w), umr = cross(um, wr);
  const V3 h = cross(uf, al) + (cross(cross(uf, w), wr) + cross(cross(uf, wr), w)) * 0.5f - cross(um, a);
  out[1] = h.x; out[2] = h.y; out[3] = h.z;
  _Pragma("unroll") for (int k = 4; k < 10; k++) out[k] = 0.f;
  rq_sym6(um, al, 1.f, out + 4); rq_sym6(umw, wr, 0.5f, out + 4); rq_sym6(umr, w, 0.5f, out + 4);
}

template <int LANES>
__global__ __launch_bounds__(64) void inertial_params_kernel(DevScene sc, MotorTable mt, float* state, int body, int nominal, float* theta, float* gws) {
  DG_DYNQ_LANE(false);
  for (int i = 0; i < n; i++) {
    const int gl = first + i;
    float m; V3 c; Sym3 Ic;
    if (nominal) { cfp f = ln.lf(gl); m = f[DG_LF_MASS]; c = v3(f[DG_LF_COM], f[DG_LF_COM + 1], f[DG_LF_COM + 2]); Ic = ln.sym6(f + DG_LF_INERTIA); }
    else ln.link_inertia(gl, m, c, Ic);
    const float cc = dot(c, c);
    const float v[10] = {m, m * c.x, m * c.y, m * c.z, Ic.xx + m * (cc - c.x * c.x), Ic.xy - m * c.x * c.y, Ic.xz - m * c.x * c.z,
                         Ic.yy + m * (cc - c.y * c.y), Ic.yz - m * c.y * c.z, Ic.zz + m * (cc - c.z * c.z)};
    rq_store10(theta + ((size_t)env * (size_t)n + (size_t)i) * 10, v);
  }
}

// q, qd, qdd, qd_ref, s [num_envs][P][n]; NULL: the env's own q and qd, qdd = 0, qd_ref = qd.  theta_hat [num_envs][10 n].
// Y [num_envs][P][n][10 n], tau [num_envs][P][n] (needs theta_hat), grad [num_envs][P][10 n] (needs s): each nullable
template <int LANES>
__global__ __launch_bounds__(64) void id_regressor_kernel(DevScene sc, MotorTable mt, float* state, int body, int P, const float* q, const float* qd, const float* qdd,
                                                           const float* qd_ref, const float* theta_hat, const float* s, float* Y, float* tau, float* grad, float* gws) {
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  float* const ws = workspace_of<LANES>(sc, smem, gws, lane);  // this workgroup's and lane's column, for every item of the loop
  const size_t items = (size_t)sc.num_envs * (size_t)P;
  const V3 zero = v3(0.f, 0.f, 0.f), g = v3(sc.gx, sc.gy, sc.gz);
  for (size_t item = (size_t)blockIdx.x * ACTIVE + lane; item < items; item += (size_t)gridDim.x * ACTIVE) {
    const int env = (int)(item / (size_t)P);
    Lane<LANES> ln(sc, mt, ws, state + env, env, false);  // env's state, read-only
    const int first = ln.bi(body)[DG_BI_FIRST_LINK], n = ln.bi(body)[DG_BI_N_LINKS];
    const int qo = sc.tr_off, vo = qo + n, ro = vo + n, ao = ro + n, so = ao + n, blk = so + n;
    dd_stage(ln, first, n, q, item, DG_LS_Q, qo); dd_stage(ln, first, n, qd, item, DG_LS_QD, vo); dd_stage(ln, first, n, qdd, item, -1, ao);
    if (qd_ref) dd_stage(ln, first, n, qd_ref, item, -1, ro); else for (int i = 0; i < n; i++) ln.L(ro + i) = ln.L(vo + i);
    ln.kinematics(body, qo);
    for (int i = 0; i < n; i++) {  // root to tip
      const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = blk + i * RQ_STRIDE;
      const M3 R = ln.LR(po); const V3 p = ln.L3(po + 6), axw = dq_axis(ln, gl, R);
      const float qdi = ln.L(vo + i), qri = ln.L(ro + i), qddi = ln.L(ao + i);
      V3 wp = zero, wrp = zero, alp = zero, ap = -g, r = zero;  // the fixed base: at rest, accelerating against gravity
      if (par >= 0) {
        const int op = blk + (par - first) * RQ_STRIDE;
        wp = ln.L3(op + RQ_W); wrp = ln.L3(op + RQ_WR); alp = ln.L3(op + RQ_AL); ap = ln.L3(op + RQ_A); r = p - ln.L3(ln.pll(par)[PLL_POSE] + 6);
      }
      V3 w = wp, wr = wrp, al = alp, a = ap + cross(alp, r) + (cross(wp, cross(wrp, r)) + cross(wrp, cross(wp, r))) * 0.5f;
      const V3 cv = (cross(wp, axw) * qri + cross(wrp, axw) * qdi) * 0.5f;
      if (ln.li(gl)[DG_LI_TYPE] == 0) { w = wp + axw * qdi; wr = wrp + axw * qri; al = alp + axw * qddi + cv; }
      else a = a + axw * qddi + cv * 2.f;
      ln.L3set(o + RQ_W, w); ln.L3set(o + RQ_WR, wr); ln.L3set(o + RQ_AL, al); ln.L3set(o + RQ_A, a);
    }
    if (Y) {
      float* const out = Y + item * (size_t)n * (size_t)(10 * n);
      const float zeros[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < n; j++) {
        const int gj = first + j, pj = ln.pll(gj)[PLL_POSE], o = blk + j * RQ_STRIDE;
        const M3 Rj = ln.LR(pj); const V3 Pj = ln.L3(pj + 6);
        const V3 w = tmul(Rj, ln.L3(o + RQ_W)), wr = tmul(Rj, ln.L3(o + RQ_WR)), al = tmul(Rj, ln.L3(o + RQ_AL)), a = tmul(Rj, ln.L3(o + RQ_A));
        int k = j;  // the next ancestor (or the link itself) on the way down to the root
        for (int i = n - 1; i >= 0; i--) {
          float* const dst = out + ((size_t)i * (size_t)n + (size_t)j) * 10;
          if (i == k) {
            const int gi = first + i, pi = ln.pll(gi)[PLL_POSE]; const V3 axw = dq_axis(ln, gi, ln.LR(pi));
            const bool rev = ln.li(gi)[DG_LI_TYPE] == 0;
            const V3 uf = tmul(Rj, rev ? cross(axw, Pj - ln.L3(pi + 6)) : axw), um = rev ? tmul(Rj, axw) : zero;
            float row[10]; rq_row(uf, um, w, wr, al, a, row);
            rq_store10(dst, row);
            const int par = ln.li(gi)[DG_LI_PARENT]; k = par < 0 ? -1 : par - first;
          } else rq_store10(dst, zeros);
        }
      }
    }
    if (tau) {
      const float* th = theta_hat + (size_t)env * (size_t)(10 * n);
      for (int i = 0; i < n; i++) {  // each link's force and moment about its origin, A_i theta_hat_i, in world axes
        const int gl = first + i, o = blk + i * RQ_STRIDE; const M3 R = ln.LR(ln.pll(gl)[PLL_POSE]);
        const V3 w = tmul(R, ln.L3(o + RQ_W)), wr = tmul(R, ln.L3(o + RQ_WR)), al = tmul(R, ln.L3(o + RQ_AL)), a = tmul(R, ln.L3(o + RQ_A));
        const float* t = th + 10 * i;
        const float m = t[0]; const V3 h = v3(t[1], t[2], t[3]); const Sym3 I = {t[4], t[5], t[6], t[7], t[8], t[9]};
        const V3 F = a * m + cross(al, h) + (cross(w, cross(wr, h)) + cross(wr, cross(w, h))) * 0.5f;
        const V3 N = mul(I, al) + (cross(w, mul(I, wr)) + cross(wr, mul(I, w))) * 0.5f + cross(h, a);
        ln.L3set(o + RQ_F, mul(R, F)); ln.L3set(o + RQ_N, mul(R, N));
      }
      float* const out = tau + item * (size_t)n;
      for (int i = n - 1; i >= 0; i--) {  // tip to root
        const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = blk + i * RQ_STRIDE;
        const V3 f = ln.L3(o + RQ_F), nn = ln.L3(o + RQ_N), axw = dq_axis(ln, gl, ln.LR(po));
        out[i] = ln.li(gl)[DG_LI_TYPE] == 0 ? dot(axw, nn) : dot(axw, f);
        if (par >= 0) {
          const int op = blk + (par - first) * RQ_STRIDE; const V3 r = ln.L3(po + 6) - ln.L3(ln.pll(par)[PLL_POSE] + 6);
          ln.L3set(op + RQ_F, ln.L3(op + RQ_F) + f); ln.L3set(op + RQ_N, ln.L3(op + RQ_N) + nn + cross(r, f));
        }
      }
    }
    if (grad) {
      dd_stage(ln, first, n, s, item, -1, so);
      float* const out = grad + item * (size_t)(10 * n);
      for (int i = 0; i < n; i++) {  // root to tip: the virtual twist (velocity of the link origin, angular velocity) of joint rates s
        const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = blk + i * RQ_STRIDE;
        const M3 R = ln.LR(po); const V3 axw = dq_axis(ln, gl, R); const float si = ln.L(so + i);
        V3 vs = zero, wsv = zero;
        if (par >= 0) {
          const int op = blk + (par - first) * RQ_STRIDE; const V3 r = ln.L3(po + 6) - ln.L3(ln.pll(par)[PLL_POSE] + 6);
          wsv = ln.L3(op + RQ_N); vs = ln.L3(op + RQ_F) + cross(wsv, r);
        }
        if (ln.li(gl)[DG_LI_TYPE] == 0) wsv = wsv + axw * si; else vs = vs + axw * si;
        ln.L3set(o + RQ_F, vs); ln.L3set(o + RQ_N, wsv);
        const V3 w = tmul(R, ln.L3(o + RQ_W)), wr = tmul(R, ln.L3(o + RQ_WR)), al = tmul(R, ln.L3(o + RQ_AL)), a = tmul(R, ln.L3(o + RQ_A));
        float row[10]; rq_row(tmul(R, vs), tmul(R, wsv), w, wr, al, a, row);
        rq_store10(out + (size_t)i * 10, row);
      }
    }
  }
}

}  // namespace dg
