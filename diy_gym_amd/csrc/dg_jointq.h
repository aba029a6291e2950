// dg_jointq.h -- the second half of p.getJointState(s) for many joints at once: jointReactionForces (after
// p.enableJointForceTorqueSensor) and appliedJointMotorTorque.  One env per lane in the world's own workspace mode, one launch per
// call, nothing allocated; the state is read, never written, and nothing the step stores changed: the body's velocities at the
// start of the last substep are where save_prev_velocities keeps them (DG_BI_PREV_OFF), the impulses where store_warm_cache does.
//
//   joint_wrench_kernel  for one body and up to DG_JOINT_WRENCH_MAX joint selectors: per selector what ft_wrench (dg_solver.h)
//                        computes for the compiled force_torque_sensor -- the force and torque the parent side exerts on the child
//                        side through the joint, in the inertial frame of the joint's child link, torque about its origin:
//                        Newton-Euler over the child side with the accelerations (v_now - v_prev) / h, gravity taken off, minus
//                        the contact forces on child-side shapes with the contact point CL_P as the arm.
//   joint_effort_kernel  DG_LS_APPLIED of every joint of a body.
//
// What differs from the compiled op is WHERE the numbers come from, not what is done with them.  The op walks from the root once
// per (sensor, child-side link) pair (link_motion); here the pose and the motion of the base and of every link of the body -- R, p,
// w, v, alpha, a -- are computed ONCE, root to tip, each link from its parent's stored values, with the transforms of
// Lane::kinematics and link_motion's formulas, and the selectors read them back.  The op reads the last substep's own contact list and rows; here the GEOMETRY is that
// of the state handed in (collide<LANES, 0>) and the IMPULSES are the cached ones of the contact with the same key over h, 0 for a
// new one -- the staleness rule of dg_contactf.h.  A contact counts for a selector when exactly one of its two shapes is on the
// child side; a shape is on the child side when it belongs to the body and either its URDF link is in the selector's frame mask
// (the rigid cluster) or its moving link is in the link mask (everything hanging off the cluster).
//
// Workspace and grid: those of dg_contactq.h / dg_contactf.h -- launched with the grid and block of reset_kernel<LANES>, lanes
// without an env stay in every call that votes with __any, clamped to the last env, and only their stores are masked.  Borrowed:
//   * CL_DVA, CL_NVA, CL_DVB of the lane's own contact list for each contact's force vector, as net_contact_wrench_kernel;
//   * the head of the transient region (sc.tr_off) for the pose and motion block, JW_STRIDE = 21 slots for the base and for every
//     link of the body.  collide keeps its shape cache (SC_STRIDE per shape) there, so the block is written only AFTER collide has returned:
//     the contact list lives at sc.cont_off, outside the region, and nothing reads the shape cache again.  jointq_slots() is what
//     the C-ABI checks against sc.tr_slots.
// Link tables, selectors and masks are wave-uniform (scalar loads); no lane talks to another.
//
// The same bits in every mode.  Everything this kernel computes after the narrow phase -- the poses of the queried body's links, the
// motion pass and the sums -- is written on the jw_* helpers below, each under `#pragma clang fp contract(off)`: every instantiation
// then runs the source's own IEEE operations in the source's order.  Measured on an MI355X while this was built: on the shared
// operators of dg_device.h and the shared poses of the POSE region (Lane::kinematics) the floating cart of cart_tree differed by up
// to 5 ulp in single components between one env per wavefront and every other LDS mode, and it still did with only the motion pass
// and the sums on the helpers -- which multiply the compiler fuses into which add of the shared kinematics is decided per
// instantiation.  Building the whole kernel with -ffp-contract=off cured it but re-rounds the narrow phase (the hull contacts of two
// pressed arms then left the ones dg_world_contacts reports: readout error 2.3e-5 instead of 1.1e-6).  So the narrow phase runs on
// the shared kinematics, as in every other query, and the queried body's poses are computed a second time here, without contraction;
// they can differ from dg_world_frame_state's in the last bits.
#pragma once
#include "dg_contactf.h"
#include "dg_dynq.h"
#include "dg_launch.h"  // JwSelectors

namespace dg {

enum { JW_R = 0, JW_P = 6, JW_W = 9, JW_V = 12, JW_AL = 15, JW_A = 18, JW_STRIDE = 21 };  // R: its first two columns, as the POSE region
constexpr int jointq_slots(int n_links) { return JW_STRIDE * (n_links + 1); }

#define JW_NO_CONTRACT _Pragma("clang fp contract(off)")
DGD V3 jw_add(V3 a, V3 b) { JW_NO_CONTRACT return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
DGD V3 jw_sub(V3 a, V3 b) { JW_NO_CONTRACT return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
DGD V3 jw_scale(V3 a, float k) { JW_NO_CONTRACT return v3(a.x * k, a.y * k, a.z * k); }
DGD V3 jw_cross(V3 a, V3 b) { JW_NO_CONTRACT return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
DGD V3 jw_mul(const M3& A, V3 b) {
  JW_NO_CONTRACT
  return v3(A.m[0] * b.x + A.m[1] * b.y + A.m[2] * b.z, A.m[3] * b.x + A.m[4] * b.y + A.m[5] * b.z, A.m[6] * b.x + A.m[7] * b.y + A.m[8] * b.z);
}
DGD V3 jw_tmul(const M3& A, V3 b) {  // A^T b
  JW_NO_CONTRACT
  return v3(A.m[0] * b.x + A.m[3] * b.y + A.m[6] * b.z, A.m[1] * b.x + A.m[4] * b.y + A.m[7] * b.z, A.m[2] * b.x + A.m[5] * b.y + A.m[8] * b.z);
}
DGD V3 jw_mul(const Sym3& S, V3 b) {
  JW_NO_CONTRACT
  return v3(S.xx * b.x + S.xy * b.y + S.xz * b.z, S.xy * b.x + S.yy * b.y + S.yz * b.z, S.xz * b.x + S.yz * b.y + S.zz * b.z);
}
DGD M3 jw_mul(const M3& A, const M3& B) {
  JW_NO_CONTRACT
  M3 C;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C.m[3 * i + j] = A.m[3 * i] * B.m[j] + A.m[3 * i + 1] * B.m[3 + j] + A.m[3 * i + 2] * B.m[6 + j];
  return C;
}
DGD M3 jw_rot_axis(V3 a, float th) {  // rot_axis (dg_device.h)
  JW_NO_CONTRACT
  const float s = __sinf(th), c = __cosf(th); const float t = 1.f - c;
  M3 R = {{t * a.x * a.x + c, t * a.x * a.y - s * a.z, t * a.x * a.z + s * a.y, t * a.x * a.y + s * a.z, t * a.y * a.y + c,
           t * a.y * a.z - s * a.x, t * a.x * a.z - s * a.y, t * a.y * a.z + s * a.x, t * a.z * a.z + c}};
  return R;
}
DGD M3 jw_qmat(Q4 q) {  // qmat (dg_device.h)
  JW_NO_CONTRACT
  const float n = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w, s = n > 0.f ? 2.0f * frcp(n) : 0.f;
  const float xs = q.x * s, ys = q.y * s, zs = q.z * s;
  const float wx = q.w * xs, wy = q.w * ys, wz = q.w * zs, xx = q.x * xs, xy = q.x * ys, xz = q.x * zs, yy = q.y * ys, yz = q.y * zs, zz = q.z * zs;
  M3 R = {{1.f - (yy + zz), xy - wz, xz + wy, xy + wz, 1.f - (xx + zz), yz - wx, xz - wy, yz + wx, 1.f - (xx + yy)}};
  return R;
}
DGD Sym3 jw_scale(const Sym3& S, float k) { JW_NO_CONTRACT Sym3 o = {S.xx * k, S.xy * k, S.xz * k, S.yy * k, S.yz * k, S.zz * k}; return o; }

// the stored pose and motion of link gl (-1: the base) of the body whose first link is `first`: the rotation is kept as its first
// two columns, the third is their cross product, as in the POSE region
template <int LANES>
DGD void jw_load(const Lane<LANES>& ln, int first, int gl, LinkMotion& m) {
  const int o = ln.sc.tr_off + (gl < 0 ? 0 : gl - first + 1) * JW_STRIDE;
  const V3 c0 = ln.L3(o + JW_R), c1 = ln.L3(o + JW_R + 3), c2 = jw_cross(c0, c1);
  const M3 R = {{c0.x, c1.x, c2.x, c0.y, c1.y, c2.y, c0.z, c1.z, c2.z}};
  m.R = R; m.p = ln.L3(o + JW_P); m.w = ln.L3(o + JW_W); m.v = ln.L3(o + JW_V); m.al = ln.L3(o + JW_AL); m.a = ln.L3(o + JW_A);
}
template <int LANES>
DGD void jw_store_pose(const Lane<LANES>& ln, int first, int gl, const M3& R, V3 p) {
  const int o = ln.sc.tr_off + (gl < 0 ? 0 : gl - first + 1) * JW_STRIDE;
  ln.L3set(o + JW_R, v3(R.m[0], R.m[3], R.m[6])); ln.L3set(o + JW_R + 3, v3(R.m[1], R.m[4], R.m[7])); ln.L3set(o + JW_P, p);
}
template <int LANES>
DGD void jw_store_motion(const Lane<LANES>& ln, int first, int gl, const LinkMotion& m) {
  const int o = ln.sc.tr_off + (gl < 0 ? 0 : gl - first + 1) * JW_STRIDE;
  ln.L3set(o + JW_W, m.w); ln.L3set(o + JW_V, m.v); ln.L3set(o + JW_AL, m.al); ln.L3set(o + JW_A, m.a);
}
// ft_add_part (dg_solver.h) on the helpers above: force and torque (about ps) a rigid part moving with a link needs, gravity taken off
DGD void jw_add_part(const DevScene& sc, const LinkMotion& m, float mass, V3 c, const Sym3& Ic, V3 ps, V3& F, V3& T) {
  const V3 rc = jw_mul(m.R, c), pc = jw_add(m.p, rc);
  const V3 ac = jw_add(jw_add(m.a, jw_cross(m.al, rc)), jw_cross(m.w, jw_cross(m.w, rc)));
  const V3 f = jw_scale(jw_sub(ac, v3(sc.gx, sc.gy, sc.gz)), mass);
  const V3 nt = jw_add(jw_mul(m.R, jw_mul(Ic, jw_tmul(m.R, m.al))), jw_cross(m.w, jw_mul(m.R, jw_mul(Ic, jw_tmul(m.R, m.w)))));
  F = jw_add(F, f); T = jw_add(jw_add(T, nt), jw_cross(jw_sub(pc, ps), f));
}
// mass, centre and inertia of link gl with the per-env mass scale applied (Lane::link_inertia)
template <int LANES>
DGD void jw_link_inertia(const Lane<LANES>& ln, int gl, float& m, V3& c, Sym3& Ic) {
  JW_NO_CONTRACT
  cfp f = ln.lf(gl); m = f[DG_LF_MASS]; c = v3(f[DG_LF_COM], f[DG_LF_COM + 1], f[DG_LF_COM + 2]); 
  { const Sym3 t = {f[DG_LF_INERTIA], f[DG_LF_INERTIA + 1], f[DG_LF_INERTIA + 2], f[DG_LF_INERTIA + 3], f[DG_LF_INERTIA + 4], f[DG_LF_INERTIA + 5]}; Ic = t; }
  if (ln.li(gl)[DG_LI_MASS_SCALE] >= 0) { const float s = ln.mass_scale(gl); m = m * s; Ic = jw_scale(Ic, s); }
}

// wrench [num_envs][n][6] (force 3, torque 3).  Each slot is stored exactly once, from registers; the order of summation -- the
// rigid part, the moving links in ascending order, the contacts in pair order -- is ft_wrench's and the same in every mode.
template <int LANES>
__global__ __launch_bounds__(64) void joint_wrench_kernel(DevScene sc, MotorTable mt, float* state, int body, JwSelectors sel, float* wrench, float* gws) {
  JW_NO_CONTRACT
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  const int env = blockIdx.x * ACTIVE + lane; const bool valid = env < sc.num_envs; const int e = valid ? env : sc.num_envs - 1;
  Lane<LANES> ln(sc, mt, workspace_of<LANES>(sc, smem, gws, lane), state + e, e, false);  // never stores state
  for (int b = 0; b < sc.nba; b++) ln.kinematics(b);
  const int ncont = sc.npairs > 0 ? collide<LANES, 0>(ln) : 0;
  const int C = sc.max_contacts;
  // 1. the force on the narrow phase's side A of every contact that has this body on a side, into the lane's own list
  for (int c = 0; c < C; c++) {
    const bool has = c < ncont;
    if (!__any(has)) break;
    const int co = sc.cont_off + 1 + c * CL_STRIDE;
    const int pair = has ? (int)ln.L(co + CL_PAIR) : 0;
    const int sa = sc.PI[pair * DG_PI_STRIDE + DG_PI_A], sb = sc.PI[pair * DG_PI_STRIDE + DG_PI_B];
    const bool keep = has && (sc.SI[sa * DG_SI_STRIDE + DG_SI_BODY] == body || sc.SI[sb * DG_SI_STRIDE + DG_SI_BODY] == body);
    if (!__any(keep)) continue;
    float f[3]; cf_forces(ln, co, keep, f);
    if (!keep) continue;
    V3 n = ln.L3(co + CL_N), t1, t2; tangent_basis(n, t1, t2);
    const V3 fa = jw_add(jw_add(jw_scale(n, f[0]), jw_scale(t1, f[1])), jw_scale(t2, f[2]));
    ln.L(co + CL_DVA) = fa.x; ln.L(co + CL_NVA) = fa.y; ln.L(co + CL_DVB) = fa.z;
  }
  // 2. the pose and the motion of the base and of each link of THIS body, once, root to tip (a parent has a smaller index): the
  //    kinematics of Lane::kinematics and the formulas of link_motion, on the helpers above
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
  // 3. the sums, selector by selector
  for (int s = 0; s < sel.n; s++) {
    const dg_joint_selector& js = sel.s[s];
    const int fr = js.frame; cfp ff = sc.FF + fr * DG_FF_STRIDE;
    const int ga = sc.FI[fr * DG_FI_STRIDE + DG_FI_LINK];
    LinkMotion ma; jw_load(ln, first, ga, ma);
    const Q4 qo = {ff[DG_FF_COM_QUAT], ff[DG_FF_COM_QUAT + 1], ff[DG_FF_COM_QUAT + 2], ff[DG_FF_COM_QUAT + 3]};
    const M3 Rs = jw_mul(ma.R, jw_qmat(qo)); const V3 ps = jw_add(ma.p, jw_mul(ma.R, v3(ff[DG_FF_COM_POS], ff[DG_FF_COM_POS + 1], ff[DG_FF_COM_POS + 2])));
    V3 F = v3(0.f, 0.f, 0.f), T = v3(0.f, 0.f, 0.f);
    if (js.flags & DG_FT_WHOLE_LINK) { float m; V3 c; Sym3 Ic; jw_link_inertia(ln, ga, m, c, Ic); jw_add_part(sc, ma, m, c, Ic, ps, F, T); }
    else if (js.rigid[0] > 0.f) {
      const float* fl = js.rigid;
      const float ms = ga >= 0 ? ln.mass_scale(ga) : 1.0f; const Sym3 Ic = {fl[4] * ms, fl[5] * ms, fl[6] * ms, fl[7] * ms, fl[8] * ms, fl[9] * ms};
      jw_add_part(sc, ma, fl[0] * ms, v3(fl[1], fl[2], fl[3]), Ic, ps, F, T);
    }
    for (int i = 0; i < n; i++) {
      if (!((js.link_mask >> i) & 1ull)) continue;
      const int gl = first + i; float m; V3 c; Sym3 Ic; jw_link_inertia(ln, gl, m, c, Ic);
      LinkMotion mk; jw_load(ln, first, gl, mk); jw_add_part(sc, mk, m, c, Ic, ps, F, T);
    }
    for (int c = 0; c < ncont; c++) {
      const int co = sc.cont_off + 1 + c * CL_STRIDE, pair = (int)ln.L(co + CL_PAIR);
      const int sa = sc.PI[pair * DG_PI_STRIDE + DG_PI_A], sb = sc.PI[pair * DG_PI_STRIDE + DG_PI_B];  // per-lane index: vector loads
      bool in[2];
#pragma unroll
      for (int k = 0; k < 2; k++) {
        cip si = sc.SI + (k == 0 ? sa : sb) * DG_SI_STRIDE;
        const int ul = ((si[DG_SI_FLAGS] >> 8) & 0xFFFF) - 1, ll = si[DG_SI_LINK] - first;  // URDF link (-1: the base link), moving link
        in[k] = si[DG_SI_BODY] == body && ((ul >= 0 && ul < 64 && ((js.frame_mask >> ul) & 1ull)) || (si[DG_SI_LINK] >= 0 && ll < 64 && ((js.link_mask >> ll) & 1ull)));
      }
      if (in[0] == in[1]) continue;
      const V3 p = ln.L3(co + CL_P), fa = v3(ln.L(co + CL_DVA), ln.L(co + CL_NVA), ln.L(co + CL_DVB));
      const V3 f = in[0] ? fa : v3(-fa.x, -fa.y, -fa.z);
      F = jw_sub(F, f); T = jw_sub(T, jw_cross(jw_sub(p, ps), f));
    }
    const V3 Fl = jw_tmul(Rs, F), Tl = jw_tmul(Rs, T);
    if (valid) {
      float* o = wrench + ((size_t)e * sel.n + s) * 6;
      o[0] = Fl.x; o[1] = Fl.y; o[2] = Fl.z; o[3] = Tl.x; o[4] = Tl.y; o[5] = Tl.z;
    }
  }
}

// out [num_envs][n]: the motor torque applied to each joint of the body during the last solver pass (DG_LS_APPLIED)
template <int LANES>
__global__ __launch_bounds__(64) void joint_effort_kernel(DevScene sc, MotorTable mt, float* state, int body, float* out, float* gws) {
  DG_DYNQ_LANE(false);
  for (int i = 0; i < n; i++) out[(size_t)env * n + i] = ln.S(ln.li(first + i)[DG_LI_STATE_OFF] + DG_LS_APPLIED);
}

}  // namespace dg
