// dg_inst.hip -- instantiates the kernels of one envs-per-wavefront mode.  Compiled several times:
//   -DDG_LANES={64,32,16,8,4,1,0}  -DDG_PART=0  step kernels (+ stamped build for 64, 16 and 8)
//                            -DDG_PART=1  reset / observe / frame / pose / dynamics-query / IK-query / contact-query / contact-force / link-state / joint-wrench / link-acceleration kernels and the mode's launch table
//                                         (+ the closest-points query kernel for 64, which serves every mode)
//   -DDG_LANES=64            -DDG_PART=2  helper-wave step kernels
//   -DDG_LANES=-16 -DDG_TAG=g16           the global-workspace mode with 16 envs per wavefront
//   -DDG_MANIFOLD (with any of the above but the helper-wave part): the same kernels with the hull-hull contact manifold compiled
//                 in (hull_manifold_points > 1), in namespace dg_mf so that they do not clash with the default ones
#include <hip/hip_runtime.h>
#ifdef DG_MANIFOLD
#define dg dg_mf
#endif
#include "dg_launch.h"
#include "dg_entry.h"
#include "dg_dynq.h"
#if DG_PART == 1
#include "dg_ikq.h"
#include "dg_contactq.h"
#include "dg_contactf.h"
#include "dg_stateq.h"
#include "dg_jointq.h"
#include "dg_accelq.h"
#if DG_LANES == 64 && !defined(DG_MANIFOLD)
#include "dg_closestq.h"
#endif
#endif

#define DG_CAT_(a, b) a##b
#define DG_CAT(a, b) DG_CAT_(a, b)
#ifndef DG_TAG
#define DG_TAG DG_LANES
#endif
#define DGL(name) DG_CAT(DG_CAT(name, _), DG_TAG)

namespace dg {

constexpr int L = DG_LANES;
constexpr bool HAS_PROF = (DG_LANES == 64 || DG_LANES == 32 || DG_LANES == 16 || DG_LANES == 8 || DG_LANES == 4 || DG_LANES == 1 || DG_LANES == -16);

void DGL(l_step)(dim3 grid, int lds, hipStream_t st, bool prof, DG_STEP_PARAMS, float* gws);
hipError_t DGL(l_prepare_step)(int lds);
#if DG_LANES == 64 && !defined(DG_MANIFOLD)
void l_step_par_64(dim3 grid, int lds, hipStream_t st, bool prof, DG_STEP_PARAMS, const uint8_t* reset_mask, int reset_mode);
hipError_t l_prepare_par_64(int lds);
#endif

#if DG_PART == 0
void DGL(l_step)(dim3 grid, int lds, hipStream_t st, bool prof, DG_STEP_PARAMS, float* gws) {
  if constexpr (HAS_PROF) { if (prof) { hipLaunchKernelGGL((step_kernel<L, true>), grid, dim3(64), lds, st, sc, mt, state, actions, mask, obs, rew, term, rew_sum, term_flag, diag, cycles, gws); return; } }
  hipLaunchKernelGGL((step_kernel<L, false>), grid, dim3(64), lds, st, sc, mt, state, actions, mask, obs, rew, term, rew_sum, term_flag, diag, (unsigned long long*)nullptr, gws);
}
hipError_t DGL(l_prepare_step)(int lds) {
  hipError_t e = hipFuncSetAttribute((const void*)step_kernel<L, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if constexpr (HAS_PROF) { if (e == hipSuccess) e = hipFuncSetAttribute((const void*)step_kernel<L, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); }
  return e;
}
#elif DG_PART == 2
void l_step_par_64(dim3 grid, int lds, hipStream_t st, bool prof, DG_STEP_PARAMS, const uint8_t* reset_mask, int reset_mode) {
  if (reset_mode) hipLaunchKernelGGL(reset_kernel_par<1>, grid, dim3(256), lds, st, sc, mt, state, reset_mask, obs);
  else if (prof) hipLaunchKernelGGL(step_kernel_par<true>, grid, dim3(256), lds, st, sc, mt, state, actions, mask, obs, rew, term, rew_sum, term_flag, diag, cycles);
  else hipLaunchKernelGGL(step_kernel_par<false>, grid, dim3(256), lds, st, sc, mt, state, actions, mask, obs, rew, term, rew_sum, term_flag, diag, (unsigned long long*)nullptr);
}
hipError_t l_prepare_par_64(int lds) {
  hipError_t e = hipFuncSetAttribute((const void*)step_kernel_par<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)step_kernel_par<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)reset_kernel_par<1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  return e;
}
#else  // DG_PART == 1
static void l_reset(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, const uint8_t* mask, float* obs, float* gws) {
  hipLaunchKernelGGL(reset_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, mask, obs, gws);
}
static void l_observe(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, float* obs, float* rew, uint8_t* term, float* rew_sum, uint8_t* term_flag, float* gws) {
  hipLaunchKernelGGL(observe_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, obs, rew, term, rew_sum, term_flag, gws);
}
static void l_frame(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, int frame, int com, float* out, float* gws) {
  hipLaunchKernelGGL(frame_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, frame, com, out, gws);
}
static void l_wrench(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, int frame, int link_frame, const float* force, const float* pos, const float* torque, float* gws) {
  hipLaunchKernelGGL(wrench_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, frame, link_frame, force, pos, torque, gws);
}
static void l_pose(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int ncam, cip CI, cfp CF, float* table, float* gws, int nmount, int mbody, int mframe) {
  hipLaunchKernelGGL(pose_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, ncam, CI, CF, table, gws, nmount, mbody, mframe);
}
static void l_joint_state(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, float* q_out, float* qd_out, float* gws) {
  hipLaunchKernelGGL(joint_state_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, q_out, qd_out, gws);
}
static void l_joint_torque(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, const float* tau, float* gws) {
  hipLaunchKernelGGL(joint_torque_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, tau, gws);
}
static void l_jacobian(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, int frame, float lx, float ly, float lz, const float* q, float* jac_t, float* jac_r, float* gws) {
  hipLaunchKernelGGL(jacobian_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, frame, lx, ly, lz, q, jac_t, jac_r, gws);
}
static void l_inverse_dynamics(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, const float* q, const float* qd, const float* qdd, float* tau, float* gws) {
  hipLaunchKernelGGL(inverse_dynamics_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, q, qd, qdd, tau, gws);
}
static void l_mass_matrix(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, const float* q, float* M, float* gws) {
  hipLaunchKernelGGL(mass_matrix_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, q, M, gws);
}
static void l_ik_query(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, int frame, const float* target_pos, const float* target_orn, const float* lists, const float* q0, float* q_out, int32_t* iters_out, float* gws) {
  hipLaunchKernelGGL(ik_query_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, frame, target_pos, target_orn, lists, q0, q_out, iters_out, gws);
}
static void l_joint_targets(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, uint64_t joint_mask, const float* pos, const float* vel, float* gws) {
  hipLaunchKernelGGL(joint_targets_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, joint_mask, pos, vel, gws);
}
static void l_joint_reset(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, uint64_t joint_mask, const float* q, const float* qd, const uint8_t* env_mask, float* gws) {
  hipLaunchKernelGGL(joint_reset_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, joint_mask, q, qd, env_mask, gws);
}
static void l_contacts(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body_a, int link_a, int body_b, int link_b, int32_t* count, int32_t* ids, float* geom, float* force, float* gws) {
  hipLaunchKernelGGL(contact_query_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body_a, link_a, body_b, link_b, count, ids, geom, force, gws);
}
static void l_contact_forces(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body_a, int link_a, int body_b, int link_b, int32_t* count, int32_t* ids, float* out, float* gws) {
  hipLaunchKernelGGL(contact_force_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body_a, link_a, body_b, link_b, count, ids, out, gws);
}
static void l_net_contact_wrench(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, const CfSelectors& sel, int body_b, int link_b, float* wrench, int32_t* ncontacts, float* gws) {
  hipLaunchKernelGGL(net_contact_wrench_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, sel, body_b, link_b, wrench, ncontacts, gws);
}
static void l_link_states(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, const LsSelectors& sel, int com, float* out, float* gws) {
  hipLaunchKernelGGL(link_states_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, sel, com, out, gws);
}
static void l_reset_base(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, const float* pos, const float* orn, const float* lin_vel, const float* ang_vel, const uint8_t* env_mask, float* gws) {
  hipLaunchKernelGGL(reset_base_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, pos, orn, lin_vel, ang_vel, env_mask, gws);
}
static void l_joint_wrench(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, const JwSelectors& sel, float* wrench, float* gws) {
  hipLaunchKernelGGL(joint_wrench_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, sel, wrench, gws);
}
static void l_joint_effort(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, float* out, float* gws) {
  hipLaunchKernelGGL(joint_effort_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, out, gws);
}
static void l_link_accel(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, int body, const LaSelectors& sel, float* out, float* gws) {
  hipLaunchKernelGGL(link_accel_kernel<L>, grid, dim3(64), lds, st, sc, mt, state, body, sel, out, gws);
}
#if DG_LANES == 64 && !defined(DG_MANIFOLD)
void l_closest(dim3 grid, hipStream_t st, DevScene sc, const float* table, int body_a, int link_a, int body_b, int link_b, float distance, int max_points, int no_cull,
               float* hull_ws, int32_t* count, int32_t* ids, float* geom, int32_t* nearest_ids, float* nearest_geom) {
  hipLaunchKernelGGL(closest_query_kernel, grid, dim3(64), 0, st, sc, table, body_a, link_a, body_b, link_b, distance, max_points, no_cull, hull_ws, count, ids, geom, nearest_ids, nearest_geom);
}
#endif
static hipError_t l_prepare(int lds) {
  if (L == 0) return hipSuccess;
  if (L < 0) {  // only the step kernel uses LDS (the sliced sweeps' accumulated impulses)
    return DGL(l_prepare_step)(lds);
  }
  hipError_t e = DGL(l_prepare_step)(lds);
#define DG_ATTR(K) if (e == hipSuccess) e = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, lds)
  DG_ATTR(reset_kernel<L>); DG_ATTR(observe_kernel<L>); DG_ATTR(frame_kernel<L>); DG_ATTR(wrench_kernel<L>); DG_ATTR(pose_kernel<L>);
  DG_ATTR(joint_state_kernel<L>); DG_ATTR(joint_torque_kernel<L>); DG_ATTR(jacobian_kernel<L>); DG_ATTR(inverse_dynamics_kernel<L>); DG_ATTR(mass_matrix_kernel<L>);
  DG_ATTR(ik_query_kernel<L>); DG_ATTR(joint_targets_kernel<L>); DG_ATTR(joint_reset_kernel<L>);
  DG_ATTR(contact_query_kernel<L>); DG_ATTR(contact_force_kernel<L>); DG_ATTR(net_contact_wrench_kernel<L>);
  DG_ATTR(link_states_kernel<L>); DG_ATTR(reset_base_kernel<L>);
  DG_ATTR(joint_wrench_kernel<L>); DG_ATTR(joint_effort_kernel<L>);
  DG_ATTR(link_accel_kernel<L>);
#undef DG_ATTR
#if DG_LANES == 64 && !defined(DG_MANIFOLD)
  if (e == hipSuccess) e = l_prepare_par_64(lds);
#endif
  return e;
}
#ifndef __HIP_DEVICE_COMPILE__  // a host-side table of host function pointers
extern const LaunchTable DGL(g_launch_table) = {
    HAS_PROF, l_prepare, DGL(l_step),
#if DG_LANES == 64 && !defined(DG_MANIFOLD)
    l_step_par_64,
#else
    nullptr,
#endif
    l_reset, l_observe, l_frame, l_wrench, l_pose,
    l_joint_state, l_joint_torque, l_jacobian, l_inverse_dynamics, l_mass_matrix,
    l_ik_query, l_joint_targets, l_joint_reset,
    l_contacts,
    l_contact_forces, l_net_contact_wrench,
    l_link_states, l_reset_base,
    l_joint_wrench, l_joint_effort,
    l_link_accel};
#endif
#endif

}  // namespace dg
