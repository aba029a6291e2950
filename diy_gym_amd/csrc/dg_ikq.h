// dg_ikq.h -- batched inverse-kinematics query and the two joint-level push entries that go with it (pybullet's
// p.calculateInverseKinematics, the POSITION_CONTROL / VELOCITY_CONTROL forms of p.setJointMotorControlArray and
// p.resetJointState; reference call sites: diy_gym/addons/controllers/ik_controller.py:47-80, joint_controller.py:38-53).
// With the dynamics queries (dg_dynq.h) this is what a position-level controller written in Python needs of env.sim: one env
// per lane in the world's own workspace mode, one launch per call, nothing allocated.
//
//   ik_query_kernel       stages the start (the caller's q0 or the env's joint positions) into the slots [q n] and runs
//                         ikq_iterate, the iteration of run_ik (dg_solver.h) -- what the compiled DG_OP_IK_CONTROL runs after
//                         its target set-up.  The state is read, never written.
//   joint_targets_kernel  DG_LS_TARGET_POS / DG_LS_TARGET_VEL of the selected joints, as DG_OP_JOINT_CONTROL writes them.
//   joint_reset_kernel    DG_LS_Q / DG_LS_QD of the selected joints of the selected envs, and those envs' contact cache count.
// Workspace of the query: the transient region as run_ik lays it out, [q n][J 6n][v0 n][dth n]; ikq_slots() is what the C-ABI
// checks.  The lists and the link tables are wave-uniform loads; no lane talks to another (the iteration's vote on `live` apart).
#pragma once
#include "dg_solver.h"
#include "dg_dynq.h"

namespace dg {

constexpr int ikq_slots(int n) { return 9 * n; }

// joint i of a body selected by the mask: all ones selects every joint, whatever their number
DGD bool ikq_selected(uint64_t joint_mask, int i) { return joint_mask == ~0ull || (i < 64 && ((joint_mask >> i) & 1ull)); }

// The iteration of run_ik (dg_solver.h:2457), its TWIN: the loop below is that function's loop statement for statement, with the
// op's fields (body, frame, flags, lists) as arguments and the target handed in instead of being made of the current pose and an
// action.  It is a copy and not a shared function because splitting run_ik moved the register allocation of every step kernel
// that inlines it (DESIGN.md "Inverse-kinematics query"); a change to either loop belongs in both, and
// tests/test_user_ik_controller_gpu.py holds the two against each other.  The joint positions in the slots [q n] are moved
// towards the pose (tp, tq) of frame fr (global index) of body b; `rest` = [rest n][lower n][upper n][range n], read only with
// DG_IK_NULLSPACE in flags.  Returns the iterations in which the lane was still live.
template <int LANES>
DGD int ikq_iterate(const Lane<LANES>& ln, int b, int fr, V3 tp, Q4 tq, int flags, cfp rest, bool live_lane) {
  const DevScene& sc = ln.sc;
  const bool use_orn = flags & DG_IK_USE_ORIENTATION, nullsp = flags & DG_IK_NULLSPACE;
  const int first = ln.bi(b)[DG_BI_FIRST_LINK], n = ln.bi(b)[DG_BI_N_LINKS];
  const int qo = sc.tr_off, jo = qo + n, vo = jo + 6 * n, dto = vo + n;
  const int eel = sc.FI[fr * DG_FI_STRIDE + DG_FI_LINK];
  const float lam2 = nullsp ? sc.HF[DG_HF_IK_LAMBDA_SQ] : sc.HF[DG_HF_IK_JOINT_DAMPING], maxang = sc.HF[DG_HF_IK_MAX_ANGLE], g0 = sc.HF[DG_HF_IK_NULL_REST_GAIN], g1 = sc.HF[DG_HF_IK_NULL_LIMIT_GAIN];
  const float resid = sc.HF[DG_HF_IK_RESIDUAL];
  bool live = live_lane; int iters = 0;
  for (int it = 0; it < sc.ik_iters; it++) {
    ln.kinematics(b, qo);
    V3 fp, fv, fw; Q4 fq; ln.frame_state(b, fr, true, fp, fq, fv, fw, false);
    V3 ep = tp - fp;
    if (it > 0 && norm(ep) < resid) live = false;
    if (!__any(live)) break;
    iters += live ? 1 : 0;
    float dS[6] = {ep.x, ep.y, ep.z, 0.f, 0.f, 0.f};
    if (use_orn) {
      Q4 dq = qmul(tq, qconj(fq)); if (dq.w < 0.f) { dq.x = -dq.x; dq.y = -dq.y; dq.z = -dq.z; dq.w = -dq.w; }
      float sn = sqrtf(dq.x * dq.x + dq.y * dq.y + dq.z * dq.z), an = 2.0f * atan2f(sn, dq.w), k = sn > 1e-12f ? an / sn : 2.0f;
      dS[3] = dq.x * k; dS[4] = dq.y * k; dS[5] = dq.z * k;
    }
    // Jacobian columns (world frame) for the chain root -> end-effector link, zero elsewhere
    for (int i = 0; i < 6 * n; i++) ln.L(jo + i) = 0.f;
    for (int k = eel; k >= 0; k = ln.li(k)[DG_LI_PARENT]) {
      int po = ln.pll(k)[PLL_POSE]; M3 Rk = ln.LR(po); V3 pk = ln.L3(po + 6); cfp f = ln.lf(k);
      V3 axw = mul(Rk, v3(f[DG_LF_AXIS], f[DG_LF_AXIS + 1], f[DG_LF_AXIS + 2])); int i = k - first;
      V3 jl, ja; if (ln.li(k)[DG_LI_TYPE] == 0) { jl = cross(axw, fp - pk); ja = axw; } else { jl = axw; ja = v3(0, 0, 0); }
      ln.L(jo + i) = jl.x; ln.L(jo + n + i) = jl.y; ln.L(jo + 2 * n + i) = jl.z;
      if (use_orn) { ln.L(jo + 3 * n + i) = ja.x; ln.L(jo + 4 * n + i) = ja.y; ln.L(jo + 5 * n + i) = ja.z; }
    }
    // U = J J^T + lambda^2 I (rows 3..5 are zero without orientation: block diagonal, same solution)
    float U[21];
#pragma unroll
    for (int k = 0; k < 21; k++) U[k] = 0.f;
    for (int k = 0; k < n; k++) {
      float col[6];
#pragma unroll
      for (int r = 0; r < 6; r++) col[r] = ln.L(jo + r * n + k);
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c <= r; c++) U[r * (r + 1) / 2 + c] += col[r] * col[c];
    }
#pragma unroll
    for (int r = 0; r < 6; r++) U[r * (r + 1) / 2 + r] += lam2;
    chol6(U);
    float y[6]; chol6_solve(U, dS, y);
    float Jv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < n; k++) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < 6; r++) t += ln.L(jo + r * n + k) * y[r];
      float v0 = 0.f;
      if (nullsp) {
        float q = ln.L(qo + k), lo = rest[n + k], hi = rest[2 * n + k], rg = rest[3 * n + k];
        v0 = g0 * (rest[k] - q);
        if (q > hi) v0 += g1 * (hi - q) / rg;
        if (q < lo) v0 += g1 * (lo - q) / rg;
#pragma unroll
        for (int r = 0; r < 6; r++) Jv[r] += ln.L(jo + r * n + k) * v0;
      }
      ln.L(vo + k) = v0; ln.L(dto + k) = t;
    }
    float mx = 0.f;
    if (nullsp) {
      float z[6]; chol6_solve(U, Jv, z);
      for (int k = 0; k < n; k++) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 6; r++) t += ln.L(jo + r * n + k) * z[r];
        float d = ln.L(dto + k) + ln.L(vo + k) - t; ln.L(dto + k) = d; mx = fmaxf(mx, fabsf(d));
      }
    } else {
      for (int k = 0; k < n; k++) mx = fmaxf(mx, fabsf(ln.L(dto + k)));
    }
    const float scl = mx > maxang ? maxang / mx : 1.0f;
    for (int k = 0; k < n; k++) if (live) ln.L(qo + k) += scl * ln.L(dto + k);
  }
  return iters;
}

// q_out [num_envs][n]; iters_out [num_envs] (may be null): the iterations in which the env was still live
template <int LANES>
__global__ __launch_bounds__(64) void ik_query_kernel(DevScene sc, MotorTable mt, float* state, int body, int frame, const float* target_pos,
                                                       const float* target_orn, const float* lists, const float* q0, float* q_out, int32_t* iters_out,
                                                       float* gws) {
  DG_DYNQ_LANE(false);
  dq_stage(ln, first, n, q0, DG_LS_Q, sc.tr_off);
  const float* t = target_pos + (size_t)env * 3; const V3 tp = v3(t[0], t[1], t[2]);
  Q4 tq = {0.f, 0.f, 0.f, 1.f};
  if (target_orn) { const float* o = target_orn + (size_t)env * 4; Q4 g = {o[0], o[1], o[2], o[3]}; tq = g; }
  const int flags = (target_orn ? DG_IK_USE_ORIENTATION : 0) | (lists ? DG_IK_NULLSPACE : 0);
  // (the lists are immutable while the kernel runs: read like the scene tables, through the scalar cache)
  const int it = ikq_iterate(ln, body, frame, tp, tq, flags, (cfp)lists, true);
  for (int i = 0; i < n; i++) q_out[(size_t)env * n + i] = ln.L(sc.tr_off + i);
  if (iters_out) iters_out[env] = it;
}

// pos given: position target pos, velocity target vel or 0 (POSITION_CONTROL); only vel given: velocity target vel, position
// target 0 (VELOCITY_CONTROL) -- the two forms of DG_OP_JOINT_CONTROL
template <int LANES>
__global__ __launch_bounds__(64) void joint_targets_kernel(DevScene sc, MotorTable mt, float* state, int body, uint64_t joint_mask, const float* pos,
                                                            const float* vel, float* gws) {
  DG_DYNQ_LANE(true);
  for (int i = 0; i < n; i++) {
    if (!ikq_selected(joint_mask, i)) continue;
    const int lo = ln.li(first + i)[DG_LI_STATE_OFF]; const size_t k = (size_t)env * n + i;
    ln.Sset(lo + DG_LS_TARGET_POS, pos ? pos[k] : 0.f); ln.Sset(lo + DG_LS_TARGET_VEL, vel ? vel[k] : 0.f);
  }
}

// the targets stay; a teleported body's cached contact impulses mean nothing, so the env's cache is emptied as a reset does
template <int LANES>
__global__ __launch_bounds__(64) void joint_reset_kernel(DevScene sc, MotorTable mt, float* state, int body, uint64_t joint_mask, const float* q,
                                                          const float* qd, const uint8_t* env_mask, float* gws) {
  DG_DYNQ_LANE(true);
  if (env_mask && !env_mask[env]) return;
  for (int i = 0; i < n; i++) {
    if (!ikq_selected(joint_mask, i)) continue;
    const int lo = ln.li(first + i)[DG_LI_STATE_OFF]; const size_t k = (size_t)env * n + i;
    ln.Sset(lo + DG_LS_Q, q[k]); ln.Sset(lo + DG_LS_QD, qd ? qd[k] : 0.f);
  }
  if (sc.warm_off >= 0) ln.Sset(sc.warm_off, 0.f);
}

}  // namespace dg
