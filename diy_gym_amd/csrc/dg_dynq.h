// dg_dynq.h -- batched dynamics queries on a fixed-base articulated body (pybullet's p.getJointStates, p.calculateJacobian,
// p.calculateInverseDynamics, p.calculateMassMatrix and the TORQUE_CONTROL form of p.setJointMotorControlArray; reference call
// site: diy_gym/addons/controllers/admittance_controller.py:36-55).  The query half of the contract env.sim gives user addons
// written in Python, beside frame_kernel and wrench_kernel (dg_entry.h): one env per lane in the world's own workspace mode,
// one launch per call, nothing allocated.
//
// Every kernel first copies the joint positions it works at -- the caller's or the env's own -- into workspace slots and runs
// ln.kinematics(body, slots): the general path whatever the source, so a call with q = NULL and a call given the same numbers
// are the same bits.  All recursions then run in WORLD coordinates on the link poses of the POSE region:
//   jacobian_kernel          one tip-to-root walk from the frame's link; a cursor that follows the parent table while the
//                            column index counts down marks the ancestors, every other column is written as zero;
//   inverse_dynamics_kernel  recursive Newton-Euler: root-to-tip angular velocity / angular acceleration / acceleration of the
//                            link origin (the base accelerates at -g), tip-to-root force and moment about each link origin;
//   mass_matrix_kernel       composite rigid bodies: per link [inertia about the base origin 6][mass x centre 3][mass], summed
//                            tip to root into the parent's block; column i is the momentum of subtree i moving with joint i,
//                            projected on the joints of i's ancestors (the same cursor); M[i][j] and M[j][i] are one value
//                            stored twice.
// Workspace: the transient region (sc.tr_off, sc.tr_slots slots), dead outside a step -- the planner gives it at least
// AB_FIXED_STRIDE + AW_STRIDE x links slots, the passes below use at most DQ_ID_SLOTS x links; dynq_slots() is what the C-ABI checks.
// Link tables and parent lookups are wave-uniform (scalar loads); no lane talks to another.
#pragma once
#include "dg_kernels.h"

namespace dg {

// per-link blocks behind the joint vectors: inverse dynamics [q n][qd n][qdd n] then DQ_ID_STRIDE per link, mass matrix [q n]
// then DQ_CR_STRIDE per link, Jacobian [q n]
enum { DQ_W = 0, DQ_AL = 3, DQ_A = 6, DQ_F = 9, DQ_N = 12, DQ_ID_STRIDE = 15, DQ_ID_SLOTS = 3 + DQ_ID_STRIDE };
enum { DQ_I = 0, DQ_H = 6, DQ_M = 9, DQ_CR_STRIDE = 10, DQ_CR_SLOTS = 1 + DQ_CR_STRIDE };
enum { DQ_KIND_JACOBIAN = 0, DQ_KIND_ID, DQ_KIND_MASS };
constexpr int dynq_slots(int kind, int n) { return (kind == DQ_KIND_ID ? DQ_ID_SLOTS : kind == DQ_KIND_MASS ? DQ_CR_SLOTS : 1) * n; }

#define DG_DYNQ_LANE(STORES)                                                                                             \
  extern __shared__ float smem[];                                                                                        \
  constexpr int ACTIVE = envs_per_wave(LANES);                                                                           \
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;                                                              \
  const int env = blockIdx.x * ACTIVE + lane; if (env >= sc.num_envs) return;                                            \
  Lane<LANES> ln(sc, mt, workspace_of<LANES>(sc, smem, gws, lane), state + env, env, STORES);                            \
  const int first = ln.bi(body)[DG_BI_FIRST_LINK], n = ln.bi(body)[DG_BI_N_LINKS]; (void)first

// n joint values into the slots at `off`: the caller's row, else the state's column `field` (DG_LS_*), else zero
template <int LANES>
DGD void dq_stage(const Lane<LANES>& ln, int first, int n, const float* src, int field, int off) {
  const float* row = src ? src + (size_t)ln.env * n : nullptr;
  for (int i = 0; i < n; i++) ln.L(off + i) = row ? row[i] : field >= 0 ? ln.S(ln.li(first + i)[DG_LI_STATE_OFF] + field) : 0.f;
}
template <int LANES>
DGD V3 dq_axis(const Lane<LANES>& ln, int gl, const M3& R) { cfp f = ln.lf(gl); return mul(R, v3(f[DG_LF_AXIS], f[DG_LF_AXIS + 1], f[DG_LF_AXIS + 2])); }
// R Ic R^T x
DGD V3 dq_rot_inertia(const M3& R, const Sym3& Ic, V3 x) { return mul(R, mul(Ic, tmul(R, x))); }

template <int LANES>
__global__ __launch_bounds__(64) void joint_state_kernel(DevScene sc, MotorTable mt, float* state, int body, float* q_out, float* qd_out, float* gws) {
  DG_DYNQ_LANE(false);
  for (int i = 0; i < n; i++) {
    const int lo = ln.li(first + i)[DG_LI_STATE_OFF];
    if (q_out) q_out[(size_t)env * n + i] = ln.S(lo + DG_LS_Q);
    if (qd_out) qd_out[(size_t)env * n + i] = ln.S(lo + DG_LS_QD);
  }
}

// tau [num_envs][n] ADDED to the joints' DG_LS_TORQUE: consumed (and cleared) by the next step, like an external wrench
template <int LANES>
__global__ __launch_bounds__(64) void joint_torque_kernel(DevScene sc, MotorTable mt, float* state, int body, const float* tau, float* gws) {
  DG_DYNQ_LANE(true);
  for (int i = 0; i < n; i++) {
    const int lo = ln.li(first + i)[DG_LI_STATE_OFF];
    ln.Sset(lo + DG_LS_TORQUE, ln.S(lo + DG_LS_TORQUE) + tau[(size_t)env * n + i]);
  }
}

// jac_t, jac_r [num_envs][3][n] (either may be null) of the point `lx ly lz` of the INERTIAL frame of `frame`'s link, world axes
template <int LANES>
__global__ __launch_bounds__(64) void jacobian_kernel(DevScene sc, MotorTable mt, float* state, int body, int frame, float lx, float ly, float lz,
                                                       const float* q, float* jac_t, float* jac_r, float* gws) {
  DG_DYNQ_LANE(false);
  const int qo = sc.tr_off;
  dq_stage(ln, first, n, q, DG_LS_Q, qo);
  ln.kinematics(body, qo);
  V3 fp, fv, fw; Q4 fq; ln.frame_state(body, frame, true, fp, fq, fv, fw, false);
  const V3 pw = fp + mul(qmat(fq), v3(lx, ly, lz));  // (the point DG_OP_ADMITTANCE takes its Jacobian at)
  const int gl = sc.FI[frame * DG_FI_STRIDE + DG_FI_LINK];
  float* jt = jac_t ? jac_t + (size_t)env * 3 * n : nullptr; float* jr = jac_r ? jac_r + (size_t)env * 3 * n : nullptr;
  int k = gl < 0 ? -1 : gl - first;  // the next ancestor (or the link itself) on the way down to the root
  for (int j = n - 1; j >= 0; j--) {
    V3 ct = v3(0.f, 0.f, 0.f), cr = ct;
    if (j == k) {
      const int g = first + j, po = ln.pll(g)[PLL_POSE]; const V3 axw = dq_axis(ln, g, ln.LR(po));
      if (ln.li(g)[DG_LI_TYPE] == 0) { ct = cross(axw, pw - ln.L3(po + 6)); cr = axw; } else ct = axw;
      const int par = ln.li(g)[DG_LI_PARENT]; k = par < 0 ? -1 : par - first;
    }
    if (jt) { jt[j] = ct.x; jt[n + j] = ct.y; jt[2 * n + j] = ct.z; }
    if (jr) { jr[j] = cr.x; jr[n + j] = cr.y; jr[2 * n + j] = cr.z; }
  }
}

// tau [num_envs][n] = M(q) qdd + C(q, qd) qd - G(q): rigid-body terms only (no joint damping, motors or limits)
template <int LANES>
__global__ __launch_bounds__(64) void inverse_dynamics_kernel(DevScene sc, MotorTable mt, float* state, int body, const float* q, const float* qd,
                                                               const float* qdd, float* tau, float* gws) {
  DG_DYNQ_LANE(false);
  const int qo = sc.tr_off, vo = qo + n, ao = vo + n, blk = ao + n;
  dq_stage(ln, first, n, q, DG_LS_Q, qo); dq_stage(ln, first, n, qd, DG_LS_QD, vo); dq_stage(ln, first, n, qdd, -1, ao);
  ln.kinematics(body, qo);
  const V3 g = v3(sc.gx, sc.gy, sc.gz), zero = v3(0.f, 0.f, 0.f);
  for (int i = 0; i < n; i++) {  // root to tip
    const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_ID_STRIDE;
    const M3 R = ln.LR(po); const V3 p = ln.L3(po + 6), axw = dq_axis(ln, gl, R);
    const float qdi = ln.L(vo + i), qddi = ln.L(ao + i);
    V3 wp = zero, alp = zero, ap = -g, r = zero;  // the fixed base: at rest, accelerating against gravity
    if (par >= 0) { const int op = blk + (par - first) * DQ_ID_STRIDE; wp = ln.L3(op + DQ_W); alp = ln.L3(op + DQ_AL); ap = ln.L3(op + DQ_A); r = p - ln.L3(ln.pll(par)[PLL_POSE] + 6); }
    V3 w = wp, al = alp, a = ap + cross(alp, r) + cross(wp, cross(wp, r));
    const V3 sv = axw * qdi, cv = cross(wp, sv);
    if (ln.li(gl)[DG_LI_TYPE] == 0) { w = wp + sv; al = alp + axw * qddi + cv; }
    else a = a + axw * qddi + cv * 2.f;  // (the origin slides along an axis that turns with the parent)
    float m; V3 c; Sym3 Ic; ln.link_inertia(gl, m, c, Ic);
    const V3 cw = mul(R, c), ac = a + cross(al, cw) + cross(w, cross(w, cw)), F = ac * m;
    const V3 N = dq_rot_inertia(R, Ic, al) + cross(w, dq_rot_inertia(R, Ic, w)) + cross(cw, F);  // about the link origin
    ln.L3set(o + DQ_W, w); ln.L3set(o + DQ_AL, al); ln.L3set(o + DQ_A, a); ln.L3set(o + DQ_F, F); ln.L3set(o + DQ_N, N);
  }
  float* out = tau + (size_t)env * n;
  for (int i = n - 1; i >= 0; i--) {  // tip to root
    const int gl = first + i, par = ln.li(gl)[DG_LI_PARENT], po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_ID_STRIDE;
    const V3 f = ln.L3(o + DQ_F), nn = ln.L3(o + DQ_N), axw = dq_axis(ln, gl, ln.LR(po));
    out[i] = ln.li(gl)[DG_LI_TYPE] == 0 ? dot(axw, nn) : dot(axw, f);
    if (par >= 0) {
      const int op = blk + (par - first) * DQ_ID_STRIDE; const V3 r = ln.L3(po + 6) - ln.L3(ln.pll(par)[PLL_POSE] + 6);
      ln.L3set(op + DQ_F, ln.L3(op + DQ_F) + f); ln.L3set(op + DQ_N, ln.L3(op + DQ_N) + nn + cross(r, f));
    }
  }
}

// M [num_envs][n][n]
template <int LANES>
__global__ __launch_bounds__(64) void mass_matrix_kernel(DevScene sc, MotorTable mt, float* state, int body, const float* q, float* M, float* gws) {
  DG_DYNQ_LANE(false);
  const int qo = sc.tr_off, blk = qo + n;
  dq_stage(ln, first, n, q, DG_LS_Q, qo);
  ln.kinematics(body, qo);
  const V3 O = ln.base_pos(body);  // moments are taken about the base origin: lever arms stay within the body's reach
  for (int i = 0; i < n; i++) {  // each link's own rigid inertia
    const int gl = first + i, po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_CR_STRIDE;
    const M3 R = ln.LR(po); float m; V3 c; Sym3 Ic; ln.link_inertia(gl, m, c, Ic);
    const V3 cw = (ln.L3(po + 6) - O) + mul(R, c); const float cc = dot(cw, cw);
    const Sym3 Iw = symmetrize(mul(mul(R, full(Ic)), transpose(R)));
    ln.L(o + DQ_I) = Iw.xx + m * (cc - cw.x * cw.x); ln.L(o + DQ_I + 1) = Iw.xy - m * cw.x * cw.y; ln.L(o + DQ_I + 2) = Iw.xz - m * cw.x * cw.z;
    ln.L(o + DQ_I + 3) = Iw.yy + m * (cc - cw.y * cw.y); ln.L(o + DQ_I + 4) = Iw.yz - m * cw.y * cw.z; ln.L(o + DQ_I + 5) = Iw.zz + m * (cc - cw.z * cw.z);
    ln.L3set(o + DQ_H, cw * m); ln.L(o + DQ_M) = m;
  }
  for (int i = n - 1; i >= 0; i--) {  // tip to root: a link's block becomes its subtree's
    const int par = ln.li(first + i)[DG_LI_PARENT]; if (par < 0) continue;
    const int o = blk + i * DQ_CR_STRIDE, op = blk + (par - first) * DQ_CR_STRIDE;
    for (int k = 0; k < DQ_CR_STRIDE; k++) ln.L(op + k) += ln.L(o + k);
  }
  float* out = M + (size_t)env * n * n;
  for (int i = 0; i < n; i++) {
    const int gl = first + i, po = ln.pll(gl)[PLL_POSE], o = blk + i * DQ_CR_STRIDE;
    const V3 axi = dq_axis(ln, gl, ln.LR(po)); const bool revi = ln.li(gl)[DG_LI_TYPE] == 0;
    // joint i's unit motion of subtree i as (angular velocity, velocity of the subtree's point at O), and that motion's momentum
    const V3 wi = revi ? axi : v3(0.f, 0.f, 0.f), vi = revi ? cross(ln.L3(po + 6) - O, axi) : axi;
    const Sym3 Io = {ln.L(o + DQ_I), ln.L(o + DQ_I + 1), ln.L(o + DQ_I + 2), ln.L(o + DQ_I + 3), ln.L(o + DQ_I + 4), ln.L(o + DQ_I + 5)};
    const V3 h = ln.L3(o + DQ_H); const float m = ln.L(o + DQ_M);
    const V3 lin = vi * m + cross(wi, h), ang = mul(Io, wi) + cross(h, vi);
    int k = i;
    for (int j = i; j >= 0; j--) {
      float v = 0.f;
      if (j == k) {
        const int g = first + j, pj = ln.pll(g)[PLL_POSE]; const V3 axj = dq_axis(ln, g, ln.LR(pj));
        v = ln.li(g)[DG_LI_TYPE] == 0 ? dot(axj, ang) + dot(cross(ln.L3(pj + 6) - O, axj), lin) : dot(axj, lin);
        const int par = ln.li(g)[DG_LI_PARENT]; k = par < 0 ? -1 : par - first;
      }
      out[i * n + j] = v; out[j * n + i] = v;
    }
  }
}

}  // namespace dg
