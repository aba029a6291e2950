// dg_accelq.h -- how links ACCELERATE, and what an IMU mounted on one reads: the accelerometer's specific force, the gyro's angular
// velocity and the projected gravity direction, for up to DG_LINK_ACCEL_MAX sensor frames of one body.  pybullet has no such call;
// what the `imu_sensor` addon and env.sim.link_accelerations are built on.  One env per lane in the world's own workspace mode, one
// launch per call, nothing allocated; the state is read, never written, and nothing the step stores changed: the body's velocities
// at the start of the last substep are where save_prev_velocities keeps them (DG_BI_PREV_OFF).
//
//   link_accel_kernel  the pose and motion pass of joint_wrench_kernel (dg_jointq.h, its step 2) for the queried body -- R, p, w, v,
//                      alpha, a of the base and of every link, root to tip, accelerations (v_now - v_prev) / h -- and then, per
//                      selector, the readout at the sensor frame S: the frame's offset on its moving link L (DG_FF_POS/QUAT, or
//                      DG_FF_COM_POS/QUAT with `com`; the base: identity or DG_BF_REPORT_*) composed with the mount pose.  With
//                      r = p_s - p_L and the scene's gravity g:
//                        lin_acc        a + alpha x r + w x (w x r)      world axes
//                        ang_acc        alpha                            world axes
//                        specific_force R_s^T (lin_acc - g)              what an accelerometer reads
//                        ang_vel        R_s^T w                          what a gyro reads
//                        gravity        R_s^T g / |g|  (0 when g = 0)    the projected gravity direction
//                      No contact term and no narrow phase: contact, motor and external forces show through the motion.  Neither
//                      Lane::kinematics nor collide is called, so a world without candidate pairs or without the contact impulse
//                      cache is served like any other.
//
// Staleness follows joint_wrench_kernel: nothing saves velocities on a teleport, so after a joint or base reset or a state written by
// the caller that changes a velocity the reading carries the jump (v_new - v_prev) / h until the next step; after dg_world_reset the
// accelerations are zero and specific_force = -R_s^T g.
//
// Workspace and grid: those of joint_wrench_kernel -- the grid and block of reset_kernel<LANES>, lanes without an env clamped to the
// last env, only their stores masked.  Borrowed: the head of the transient region (sc.tr_off), JW_STRIDE = 21 slots for the base and
// for every link of the body (jointq_slots(), which the C-ABI checks against sc.tr_slots); nothing else of the workspace is touched.
// Link tables and selectors are wave-uniform (scalar loads); no lane talks to another.
//
// The same bits in every mode: all arithmetic is on the jw_* helpers of dg_jointq.h, each under `#pragma clang fp contract(off)`, so
// every instantiation runs the source's own IEEE operations in the source's order.  r is formed as R_L off + R_f pos, not as the
// difference of two world points, so a sensor far from the world's origin loses nothing to cancellation.
#pragma once
#include "dg_jointq.h"
#include "dg_launch.h"  // LaSelectors

namespace dg {

// out [num_envs][sel.n][DG_LA_STRIDE].  Each slot is stored exactly once, from registers.
template <int LANES>
__global__ __launch_bounds__(64) void link_accel_kernel(DevScene sc, MotorTable mt, float* state, int body, LaSelectors sel, float* out, float* gws) {
  JW_NO_CONTRACT
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  const int env = blockIdx.x * ACTIVE + lane; const bool valid = env < sc.num_envs; const int e = valid ? env : sc.num_envs - 1;
  Lane<LANES> ln(sc, mt, workspace_of<LANES>(sc, smem, gws, lane), state + e, e, false);  // never stores state
  // 1. the pose and the motion of the base and of each link of this body, once, root to tip: joint_wrench_kernel's step 2
  cip B = ln.bi(body); const int po = B[DG_BI_PREV_OFF], first = B[DG_BI_FIRST_LINK], n = B[DG_BI_N_LINKS]; const float ih = 1.0f / sc.h;
  {
    LinkMotion o; o.w = o.v = o.al = o.a = v3(0.f, 0.f, 0.f);
    if (!ln.fixed(body)) {
      const int so = B[DG_BI_STATE_OFF];
      o.v = v3(ln.S(so + DG_BS_LINVEL), ln.S(so + DG_BS_LINVEL + 1), ln.S(so + DG_BS_LINVEL + 2)); o.w = v3(ln.S(so + DG_BS_ANGVEL), ln.S(so + DG_BS_ANGVEL + 1), ln.S(so + DG_BS_ANGVEL + 2));
      o.a = jw_scale(jw_sub(o.v, v3(ln.S(po + n), ln.S(po + n + 1), ln.S(po + n + 2))), ih);
      o.al = jw_scale(jw_sub(o.w, v3(ln.S(po + n + 3), ln.S(po + n + 4), ln.S(po + n + 5))), ih);
    }
    jw_store_pose(ln, first, -1, jw_qmat(ln.base_quat(body)), ln.base_pos(body)); jw_store_motion(ln, first, -1, o);
  }
  for (int k = first; k < first + n; k++) {
    LinkMotion o; jw_load(ln, first, ln.li(k)[DG_LI_PARENT], o);
    cfp f = ln.lf(k); const bool rev = ln.li(k)[DG_LI_TYPE] == 0; const int lo = ln.li(k)[DG_LI_STATE_OFF];
    const float q = ln.S(lo + DG_LS_Q), qd = ln.S(lo + DG_LS_QD), qdd = (qd - ln.S(po + (k - first))) * ih;
    M3 RT; _Pragma("unroll") for (int t = 0; t < 9; t++) RT.m[t] = f[DG_LF_ROT + t];
    const V3 pT = v3(f[DG_LF_POS], f[DG_LF_POS + 1], f[DG_LF_POS + 2]), axl = v3(f[DG_LF_AXIS], f[DG_LF_AXIS + 1], f[DG_LF_AXIS + 2]);
    const M3 Rpc = rev ? jw_mul(RT, jw_rot_axis(axl, q)) : RT; const V3 rl = rev ? pT : jw_add(pT, jw_mul(RT, jw_scale(axl, q)));
    jw_store_pose(ln, first, k, jw_mul(o.R, Rpc), jw_add(o.p, jw_mul(o.R, rl)));
    LinkMotion me; jw_load(ln, first, k, me);   // (the pose as every reader sees it: third column from the stored two)
    const V3 ax = jw_mul(me.R, axl), r = jw_sub(me.p, o.p);
    const V3 a1 = jw_add(jw_add(o.a, jw_cross(o.al, r)), jw_cross(o.w, jw_cross(o.w, r))), v1 = jw_add(o.v, jw_cross(o.w, r));
    const V3 axqd = jw_scale(ax, qd), axqdd = jw_scale(ax, qdd);
    if (rev) { o.al = jw_add(jw_add(o.al, axqdd), jw_cross(o.w, axqd)); o.a = a1; o.v = v1; o.w = jw_add(o.w, axqd); }
    else { o.a = jw_add(jw_add(a1, axqdd), jw_scale(jw_cross(o.w, axqd), 2.0f)); o.v = jw_add(v1, axqd); }
    jw_store_motion(ln, first, k, o);
  }
  // 2. the readout, selector by selector
  const V3 g = v3(sc.gx, sc.gy, sc.gz), gh = v3(sel.ghat[0], sel.ghat[1], sel.ghat[2]);
  for (int s = 0; s < sel.n; s++) {
    const dg_accel_selector& as = sel.s[s];
    const int fr = as.frame, gl = fr < 0 ? -1 : sc.FI[fr * DG_FI_STRIDE + DG_FI_LINK];
    V3 off = v3(0.f, 0.f, 0.f); Q4 qo = {0.f, 0.f, 0.f, 1.f};
    if (fr >= 0 || as.com) {  // (both tables: pos3 then quat4)
      cfp ff = fr >= 0 ? sc.FF + fr * DG_FF_STRIDE + (as.com ? DG_FF_COM_POS : DG_FF_POS) : ln.bf(body) + DG_BF_REPORT_POS;
      off = v3(ff[0], ff[1], ff[2]); const Q4 t = {ff[3], ff[4], ff[5], ff[6]}; qo = t;
    }
    LinkMotion m; jw_load(ln, first, gl, m);
    const Q4 qm = {as.quat[0], as.quat[1], as.quat[2], as.quat[3]};
    const M3 Rf = jw_mul(m.R, jw_qmat(qo)), Rs = jw_mul(Rf, jw_qmat(qm));
    const V3 r = jw_add(jw_mul(m.R, off), jw_mul(Rf, v3(as.pos[0], as.pos[1], as.pos[2])));  // p_s - p_L
    const V3 la = jw_add(jw_add(m.a, jw_cross(m.al, r)), jw_cross(m.w, jw_cross(m.w, r)));
    const V3 sf = jw_tmul(Rs, jw_sub(la, g)), wv = jw_tmul(Rs, m.w), gv = jw_tmul(Rs, gh);
    if (valid) {
      float* o = out + ((size_t)e * sel.n + s) * DG_LA_STRIDE;
      o[DG_LA_LIN_ACC] = la.x; o[DG_LA_LIN_ACC + 1] = la.y; o[DG_LA_LIN_ACC + 2] = la.z;
      o[DG_LA_ANG_ACC] = m.al.x; o[DG_LA_ANG_ACC + 1] = m.al.y; o[DG_LA_ANG_ACC + 2] = m.al.z;
      o[DG_LA_SPECIFIC_FORCE] = sf.x; o[DG_LA_SPECIFIC_FORCE + 1] = sf.y; o[DG_LA_SPECIFIC_FORCE + 2] = sf.z;
      o[DG_LA_ANG_VEL] = wv.x; o[DG_LA_ANG_VEL + 1] = wv.y; o[DG_LA_ANG_VEL + 2] = wv.z;
      o[DG_LA_GRAVITY] = gv.x; o[DG_LA_GRAVITY + 1] = gv.y; o[DG_LA_GRAVITY + 2] = gv.z;
    }
  }
}

}  // namespace dg
