// dg_inst.hip -- instantiates the kernels of one envs-per-wavefront mode.  Compiled several times:
//   -DDG_LANES={64,32,16,8,4,1,0}  -DDG_PART=0  step kernels (+ stamped build for 64, 16 and 8)
//                            -DDG_PART=1  every kernel of DG_QUERY_KERNELS (dg_launch.h) and the mode's launch table, made from that list
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
#include "dg_taskq.h"
#include "dg_fdq.h"
#include "dg_ddq.h"
#include "dg_regq.h"
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
// the launcher of every kernel of DG_QUERY_KERNELS: A... is deduced from the table member's type
template <auto K, class... A> static void launch_q(dim3 grid, int lds, hipStream_t st, A... a) { hipLaunchKernelGGL(K, grid, dim3(64), lds, st, a...); }
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
#define DG_ATTR(name, ...) if (e == hipSuccess) e = hipFuncSetAttribute((const void*)name##_kernel<L>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  DG_QUERY_KERNELS(DG_ATTR)
#undef DG_ATTR
#if DG_LANES == 64 && !defined(DG_MANIFOLD)
  if (e == hipSuccess) e = l_prepare_par_64(lds);
#endif
  return e;
}
#ifndef __HIP_DEVICE_COMPILE__  // a host-side table of host function pointers
extern const LaunchTable DGL(g_launch_table) = {
    .has_prof = HAS_PROF, .prepare = l_prepare, .step = DGL(l_step),
#if DG_LANES == 64 && !defined(DG_MANIFOLD)
    .step_par = l_step_par_64,
#else
    .step_par = nullptr,
#endif
#define DG_SLOT(name, ...) .name = launch_q<name##_kernel<L>>,
    DG_QUERY_KERNELS(DG_SLOT)
#undef DG_SLOT
};
#endif
#endif

}  // namespace dg
