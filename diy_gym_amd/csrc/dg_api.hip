// dg_api.hip -- kernels' entry points and the C-ABI (include/diygym_hip.h).
// Build: make -C diy_gym_amd/csrc (this file, dg_plan.hip and the instantiations of dg_inst.hip link into libdiygym_hip.so)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/diygym_hip.h"
#include "dg_launch.h"
#include "dg_plan.h"
#define DG_DEFINE_RENDER_KERNEL
#include "dg_render.h"
#include "dg_raycast.h"
#include "dg_dynq.h"
#include "dg_ikq.h"
#include "dg_jointq.h"
#include "dg_accelq.h"
#include "dg_taskq.h"
#include "dg_fdq.h"
#include "dg_ddq.h"
#include "dg_regq.h"
#include "dg_lqr.h"

using namespace dg;

// Every mode's table (dg_inst.hip), X(lanes, tag): in dg, and in dg_mf the same kernels with the hull-hull contact manifold compiled in
// (-DDG_MANIFOLD: the headers in namespace dg_mf, the same types member for member -- both tables come from the one list of
// dg_launch.h); no helper-wave form there.  The global-workspace mode comes last: an unknown `lanes` falls to it.
#define DG_MODES(X) X(64, 64) X(32, 32) X(16, 16) X(8, 8) X(4, 4) X(1, 1) X(-16, g16) X(0, 0)
#define DG_DECLARE(lanes, tag) namespace dg { extern const LaunchTable g_launch_table_##tag; } namespace dg_mf { extern const dg::LaunchTable g_launch_table_##tag; }
DG_MODES(DG_DECLARE)
#undef DG_DECLARE
namespace dg {
const LaunchTable& launch_table(int lanes, bool mf) {
  static const struct { int lanes; const LaunchTable *plain, *manifold; } rows[] = {
#define DG_ROW(lanes, tag) {lanes, &g_launch_table_##tag, &dg_mf::g_launch_table_##tag},
      DG_MODES(DG_ROW)
#undef DG_ROW
  };
  constexpr int n = sizeof rows / sizeof *rows;
  int r = 0;
  while (r < n - 1 && rows[r].lanes != lanes) r++;
  return mf ? *rows[r].manifold : *rows[r].plain;
}
}  // namespace dg

static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_err = buf; return code;
}
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(DG_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)

// Every entry point runs with the world's device current and puts the caller's device back on the way out (a torch
// process may have another device current; launches and frees must not land there).
struct DeviceGuard {
  int prev = -1; bool switched = false; hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess; }
  }
  ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define DG_ON_DEVICE(dev) DeviceGuard guard_(dev); if (guard_.err != hipSuccess) return fail(DG_ERR_HIP, "hipSetDevice(%d): %s", (dev), hipGetErrorString(guard_.err))

__global__ void init_state_kernel(const float* init, float* state, int state_dim, int stride) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x; if (e >= stride) return;
  for (int k = 0; k < state_dim; k++) state[(size_t)k * stride + e] = init[k];
}

// ------------------------------------------------------------------ world
struct dg_world {
  DevScene sc; MotorTable mt;
  std::vector<int32_t> I; std::vector<double> F;
  int device = 0, lanes = 64, lds_bytes = 0, num_envs = 0, stride = 0;
  void* d_blob_i = nullptr; void* d_blob_f = nullptr; void* d_plan = nullptr; float* d_init = nullptr;
  int32_t* diag = nullptr;
  unsigned long long* profile_cycles = nullptr;
  bool par = false;  // step runs as two wavefronts per workgroup (helper wave)
  bool mf = false;   // hull_manifold_points > 1 in a world that collides two hulls: the kernels with the manifold (dg_mf)
  bool no_par_reset = false;  // DG_NO_PAR_RESET: masked resets through reset_kernel<64> (one wavefront, generic solver)
  float* d_gws = nullptr;  // global scratch when the scene does not fit LDS (lanes == 0)
  float* d_hull_ws = nullptr;  // polytope workspace of the hull-hull narrow phase (dg_hull.h), one block per wavefront of the step grid
  int cu_count = 1;     // multiProcessorCount of `device`, read once in dg_world_create
  int render_diag = 0;  // the plan's at creation (DG_RENDER_NO_CULL / DG_RENDER_DIAG, diagnostics), dg_world_set_render_diag later
  int render_wpe = 2;   // wavefronts per SIMD of the render kernel's build (DG_RENDER_WPE=3: the spilling build)
  int ray_no_cull = 0;  // dg_debug_raycast_no_cull, for tests: every ray against every shape
  int closest_no_cull = 0;  // dg_debug_closest_no_cull, for tests: every candidate pair through its primitive
  int ray_lds_words = DG_RAY_LDS_WORDS;  // LDS budget of raycast_kernel's staged rows (dg_debug_raycast_lds_words, for tests)
  int ncam = 0; float* d_render_table = nullptr; cip d_CI = nullptr; cfp d_CF = nullptr, d_PLN = nullptr;
  ~dg_world() {  // also the clean-up of a dg_world_create that failed half way
    DeviceGuard g(device);
    (void)hipFree(d_gws); (void)hipFree(d_hull_ws); (void)hipFree(d_render_table); (void)hipFree(d_blob_i); (void)hipFree(d_blob_f); (void)hipFree(d_plan); (void)hipFree(d_init);
  }
};

// `frame` as the C-ABI takes it -- the body-local pybullet joint index -- to the global frame index the kernels use; -1: the body
// has no such frame
static int global_frame(const dg_world* w, int32_t body, int32_t frame) {
  const int32_t* I = w->I.data(); const int32_t* FI = I + I[DG_H_OFF_FRAME_I]; int seen = 0;
  for (int f = 0; f < w->sc.nfr; f++) if (FI[f * DG_FI_STRIDE + DG_FI_BODY] == body) { if (seen == frame) return f; seen++; }
  return -1;
}

static dim3 grid_of(const dg_world* w) { const int per = envs_per_wave(w->lanes); return dim3((w->num_envs + per - 1) / per); }

// The tail of every entry that launches a kernel of DG_QUERY_KERNELS: the world's device, the mode's launcher of `member` with the
// world's scene and motor table, `state` and `args` -- the kernel's parameters after `state` -- and what the launch left behind.
template <class M, class... A>
static int launch_grid(const dg_world* w, dim3 grid, void* stream, M LaunchTable::*member, const float* state, const A&... args) {
  DG_ON_DEVICE(w->device);
  (launch_table(w->lanes, w->mf).*member)(grid, w->lds_bytes, (hipStream_t)stream, w->sc, w->mt, const_cast<float*>(state), args...);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}
// ... on the step's grid, one env per lane: every kernel but the grid-stride rollout_kernel (dg_world_rollout)
template <class M, class... A>
static int launch_args(const dg_world* w, void* stream, M LaunchTable::*member, const float* state, const A&... args) {
  return launch_grid(w, grid_of(w), stream, member, state, args...);
}
// ... for the kernels that end in the workspace pointer: every one but pose_kernel
template <class M, class... A>
static int launch(const dg_world* w, void* stream, M LaunchTable::*member, const float* state, const A&... args) {
  return launch_args(w, stream, member, state, args..., w->d_gws);
}
// pose_kernel into `table`: the shape rows, the rows of the world's `ncam` cameras and of `nmount` mounts (body, global frame)
static int launch_pose(const dg_world* w, void* stream, const float* state, int ncam, float* table, int nmount, int mbody, int mframe) {
  return launch_args(w, stream, &LaunchTable::pose, state, ncam, w->d_CI, w->d_CF, table, w->d_gws, nmount, mbody, mframe);
}

// ------------------------------------------------------------------ refusals that several entries share
// 0 or the error code, the message under the entry's name `what`; the entries older than the queries name none (nullptr)
#define DG_WHAT(what) (what) ? (what) : "", (what) ? ": " : ""
static const int32_t* body_row(const dg_world* w, int32_t body) { const int32_t* I = w->I.data(); return I + I[DG_H_OFF_BODY_I] + body * DG_BI_STRIDE; }
static int body_check(const dg_world* w, int32_t body, const char* what) {
  if (body < 0 || body >= w->sc.nb) return fail(DG_ERR_ARG, "%s%sbody %d out of range", DG_WHAT(what), body);
  return DG_OK;
}
// `frame` as the C-ABI takes it to the global frame index in *gf; a negative one is the base (-1).  False: the body has no such frame
static bool frame_lookup(const dg_world* w, int32_t body, int32_t frame, int* gf) {
  *gf = frame < 0 ? -1 : global_frame(w, body, frame);
  return frame < 0 || *gf >= 0;
}
static int frame_check(const dg_world* w, int32_t body, int32_t frame, int* gf, const char* what) {
  if (!frame_lookup(w, body, frame, gf)) return fail(DG_ERR_ARG, "%s%sbody %d has no frame %d", DG_WHAT(what), body, frame);
  return DG_OK;
}
// a pass over the body would borrow `need` slots of the transient region, more than sc.tr_slots
static int slots_refusal(const dg_world* w, int32_t body, int need, const char* what) {
  return fail(DG_ERR_ARG, "%s: body %d needs %d workspace slots, the world's transient region has %d", what, body, need, w->sc.tr_slots);
}
// the contact readouts that report the solver's impulses
static int impulse_cache_check(const dg_world* w, const char* what) {
  if (w->sc.warm_off < 0)
    return fail(DG_ERR_UNSUPPORTED, "%s: the world keeps no contact impulse cache (warmstart and warmstart_friction are 0, or the scene has no candidate pairs): "
                                    "no forces to report", what);
  return DG_OK;
}
#undef DG_WHAT

extern "C" {

int32_t dg_version(void) { return (0 << 16) | 12; }
const char* dg_last_error(void) { return g_err.c_str(); }

int32_t dg_world_create(const int32_t* I, int64_t n_i, const double* F, int64_t n_f, int32_t num_envs, int32_t env_stride,
                        int32_t device, uint64_t seed, int64_t env_index_base, dg_world** out) {
  if (!I || !F || !out || n_i < DG_H_INT_COUNT) return fail(DG_ERR_ARG, "null or short scene arrays");
  { int ndev = 0; HIP_TRY(hipGetDeviceCount(&ndev)); if (device < 0 || device >= ndev) return fail(DG_ERR_ARG, "device %d out of range (%d visible)", device, ndev); }
  DG_ON_DEVICE(device);
  std::unique_ptr<dg_world> holder(new dg_world());  // every early return below frees what was allocated so far
  dg_world* w = holder.get(); w->device = device;
  { hipDeviceProp_t prop; HIP_TRY(hipGetDeviceProperties(&prop, device)); w->cu_count = std::max(prop.multiProcessorCount, 1); }  // (the one query)
  // ---- every decision about the world (dg_plan.h); below only the allocations and copies it asks for
  WorldPlan p;
  if (const int rc = plan_world(I, n_i, F, n_f, num_envs, env_stride, w->cu_count, seed, env_index_base, plan_switches_from_env(), p)) return fail(rc, "%s", p.error.c_str());
  w->I.assign(I, I + n_i); w->F.assign(F, F + n_f); w->num_envs = num_envs; w->stride = env_stride;
  w->lanes = p.lanes; w->lds_bytes = p.lds_bytes; w->par = p.par; w->mf = p.mf; w->no_par_reset = p.no_par_reset;
  w->render_diag = p.render_diag; w->render_wpe = p.render_wpe; w->sc = p.sc; w->mt = p.mt;
  auto upload = [](void** dst, const void* src, size_t bytes) {
    const hipError_t e = hipMalloc(dst, std::max<size_t>(bytes, 1));
    return e != hipSuccess ? e : hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  };
  if (p.gws_floats) HIP_TRY(hipMalloc((void**)&w->d_gws, sizeof(float) * p.gws_floats));
  if (p.hull_ws_floats) HIP_TRY(hipMalloc((void**)&w->d_hull_ws, sizeof(float) * p.hull_ws_floats));
  HIP_TRY(upload(&w->d_blob_i, p.blob_i.data(), sizeof(int32_t) * p.blob_i.size()));
  HIP_TRY(upload(&w->d_blob_f, p.blob_f.data(), sizeof(float) * p.blob_f.size()));
  HIP_TRY(upload(&w->d_plan, p.table.data(), sizeof(int32_t) * p.table.size()));
  HIP_TRY(upload((void**)&w->d_init, p.init.data(), sizeof(float) * p.init.size()));
  // ---- the scene's pointers, from the three allocations
  // global -> constant address space: a no-op on the hardware, a promise of immutability to the compiler
  cip dI = (cip)w->d_blob_i; cfp dF = (cfp)w->d_blob_f;
  DevScene& sc = w->sc;
  sc.BI = dI + I[DG_H_OFF_BODY_I]; sc.LI = dI + I[DG_H_OFF_LINK_I]; sc.FI = dI + I[DG_H_OFF_FRAME_I]; sc.SI = dI + I[DG_H_OFF_SHAPE_I];
  sc.PI = dI + I[DG_H_OFF_PAIR_I]; sc.GI = dI + I[DG_H_OFF_GROUP_I]; sc.OI = dI + I[DG_H_OFF_OP_I]; sc.IL = dI + I[DG_H_OFF_ILIST];
  sc.BF = dF + I[DG_H_OFF_BODY_F]; sc.LF = dF + I[DG_H_OFF_LINK_F]; sc.FF = dF + I[DG_H_OFF_FRAME_F]; sc.SF = dF + I[DG_H_OFF_SHAPE_F];
  sc.PF = dF + I[DG_H_OFF_POINT_F]; sc.OF = dF + I[DG_H_OFF_OP_F]; sc.FL = dF + I[DG_H_OFF_FLIST]; sc.HF = dF;
  sc.KI = dI + I[DG_H_OFF_CONS_I]; sc.KF = dF + I[DG_H_OFF_CONS_F];
  sc.PLB = (cip)w->d_plan; sc.PLL = sc.PLB + (size_t)sc.nb * PLB_STRIDE; sc.PD = sc.PLB + p.pd_off; sc.GD = (cfp)(sc.PLB + p.gd_off); sc.SD = sc.PLB + p.sd_off; sc.AM = sc.PLB + p.am_off; sc.RH = (cfp)(sc.PLB + p.rh_off);
  sc.hull_ws = w->d_hull_ws;
  // cameras: per-env shape/camera pose table written by pose_kernel, read by render_kernel
  w->ncam = I[DG_H_N_CAMERAS]; w->d_CI = dI + I[DG_H_OFF_CAMERA_I]; w->d_CF = dF + I[DG_H_OFF_CAMERA_F]; w->d_PLN = dF + I[DG_H_OFF_PLANE_F];
  if (w->ncam > 0) HIP_TRY(hipMalloc((void**)&w->d_render_table, sizeof(float) * (size_t)num_envs * (size_t)(sc.nsh * RS_STRIDE + w->ncam * RC_STRIDE)));
  // allow > 64 KiB of dynamic LDS for this mode's kernels
  HIP_TRY(launch_table(w->lanes, w->mf).prepare(w->lds_bytes));
  *out = holder.release();
  return DG_OK;
}

// diagnostics: what dg_world_create would decide for `num_envs` copies of the scene on a GPU of `cu_count` CUs, with the
// environment's switches -- the planner alone, no device (include/diygym_hip.h: DG_PLAN_*)
int32_t dg_debug_plan(const int32_t* I, int64_t n_i, const double* F, int64_t n_f, int32_t num_envs, int32_t cu_count, int32_t* out,
                      int32_t* table, int64_t table_cap) {
  if (!out) return fail(DG_ERR_ARG, "null argument");
  WorldPlan p;
  if (const int rc = plan_world(I, n_i, F, n_f, num_envs, (num_envs + 63) / 64 * 64, cu_count, 0, 0, plan_switches_from_env(), p)) return fail(rc, "%s", p.error.c_str());
  const DevScene& sc = p.sc;
  auto clamp = [](size_t v) { return (int32_t)std::min<size_t>(v, INT32_MAX); };
  static_assert(DG_PLAN_PLB_STRIDE == PLB_STRIDE && DG_PLAN_PLL_STRIDE == PLL_STRIDE, "diygym_hip.h describes the plan table");
  out[DG_PLAN_LANES] = p.lanes; out[DG_PLAN_LDS_BYTES] = p.lds_bytes; out[DG_PLAN_PAR] = p.par; out[DG_PLAN_MF] = p.mf;
  out[DG_PLAN_TOTAL_SLOTS] = sc.total_slots; out[DG_PLAN_TR_OFF] = sc.tr_off; out[DG_PLAN_TR_SLOTS] = sc.tr_slots;
  out[DG_PLAN_CONT_OFF] = sc.cont_off; out[DG_PLAN_CONT2_OFF] = sc.cont2_off; out[DG_PLAN_NV_MAX] = sc.nv_max; out[DG_PLAN_NT] = sc.nt;
  out[DG_PLAN_DENSE] = sc.dense; out[DG_PLAN_CROW_TAIL] = sc.crow_tail; out[DG_PLAN_HELPER_BODY] = sc.helper_body;
  out[DG_PLAN_REG_BODY0] = sc.reg_body[0]; out[DG_PLAN_REG_BODY1] = sc.reg_body[1]; out[DG_PLAN_COLL_WAVE] = sc.coll_wave;
  out[DG_PLAN_COLL_SPLIT] = sc.coll_split; out[DG_PLAN_SPLIT_PGS] = sc.split_pgs; out[DG_PLAN_EARLY_DYN] = sc.early_dyn;
  out[DG_PLAN_GWS_FLOATS] = clamp(p.gws_floats); out[DG_PLAN_HULL_WS_FLOATS] = clamp(p.hull_ws_floats); out[DG_PLAN_NBA] = sc.nba; out[DG_PLAN_NSHA] = sc.nsha;
  out[DG_PLAN_AB_STRIDE] = sc.ab_stride; out[DG_PLAN_PD_OFF] = clamp(p.pd_off); out[DG_PLAN_GD_OFF] = clamp(p.gd_off); out[DG_PLAN_SD_OFF] = clamp(p.sd_off);
  out[DG_PLAN_AM_OFF] = clamp(p.am_off); out[DG_PLAN_TABLE_WORDS] = clamp(p.table.size());
  out[DG_PLAN_NP_SKIP] = sc.np_skip; out[DG_PLAN_RH_OFF] = clamp(p.rh_off);
  if (table) memcpy(table, p.table.data(), sizeof(int32_t) * std::min<size_t>(p.table.size(), (size_t)std::max<int64_t>(table_cap, 0)));
  return DG_OK;
}

void dg_world_destroy(dg_world* w) { delete w; }  // ~dg_world frees the device allocations on the world's device

const char* dg_world_kernel_name(const dg_world* w) {
  if (!w) return "";
  static thread_local char buf[96];
  if (w->par) snprintf(buf, sizeof buf, "step_kernel_par (4 wavefronts per 64 envs)");
  else snprintf(buf, sizeof buf, "step_kernel<%d>", w->lanes);
  return buf;
}

int32_t dg_world_dims(const dg_world* w, int32_t dims[8]) {
  if (!w || !dims) return fail(DG_ERR_ARG, "null argument");
  dims[0] = w->sc.state_dim; dims[1] = w->sc.act_dim; dims[2] = w->sc.obs_dim; dims[3] = w->sc.rew_dim; dims[4] = w->sc.term_dim;
  dims[5] = w->sc.nl; dims[6] = w->lds_bytes; dims[7] = w->lanes;
  return DG_OK;
}
int32_t dg_world_get_motor_cfg(const dg_world* w, double* cfg) {
  if (!w || !cfg) return fail(DG_ERR_ARG, "null argument");
  for (int k = 0; k < 3 * w->sc.nl; k++) cfg[k] = w->mt.v[k];
  return DG_OK;
}
int32_t dg_world_set_motor_cfg(dg_world* w, const double* cfg) {
  if (!w || !cfg) return fail(DG_ERR_ARG, "null argument");
  for (int k = 0; k < 3 * w->sc.nl; k++) w->mt.v[k] = (float)cfg[k];
  return DG_OK;
}
int32_t dg_world_set_diag_buffer(dg_world* w, int32_t* diag) { if (!w) return fail(DG_ERR_ARG, "null world"); w->diag = diag; return DG_OK; }
int32_t dg_world_set_skip_counter(dg_world* w, int32_t* skipped) { if (!w) return fail(DG_ERR_ARG, "null world"); w->sc.skip_count = skipped; return DG_OK; }

int32_t dg_world_init_state(dg_world* w, float* state, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "null argument");
  DG_ON_DEVICE(w->device);
  hipLaunchKernelGGL(init_state_kernel, dim3((w->stride + 255) / 256), dim3(256), 0, (hipStream_t)stream, w->d_init, state, w->sc.state_dim, w->stride);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}

int32_t dg_world_reset(dg_world* w, float* state, const uint8_t* mask, float* obs, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "null argument");
  // four-wavefront scenes with the usual single hot-start step: the reset ops and that step run in the step kernel itself
  // (reset mode), the envs the mask does not name computing in their scratch workspace with stores off
  if (!(w->par && w->sc.hot_start == 1 && !w->no_par_reset)) return launch(w, stream, &LaunchTable::reset, state, mask, obs);
  DG_ON_DEVICE(w->device);
  launch_table(w->lanes, w->mf).step_par(grid_of(w), w->lds_bytes, (hipStream_t)stream, false, w->sc, w->mt, state, nullptr, 0ull, obs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, mask, 1);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}

int32_t dg_world_step(dg_world* w, float* state, const float* actions, uint64_t update_mask, float* obs, float* rew, uint8_t* term,
                      float* rew_sum, uint8_t* term_flag, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "null argument");
  if (w->sc.act_dim > 0 && update_mask != 0 && !actions) return fail(DG_ERR_ARG, "update_mask selects controller addons but actions is NULL");
  DG_ON_DEVICE(w->device);
  if (actions) {
    // motor gains / force limits are uniform over envs: the controller ops selected by the mask set them here
    // (p.setJointMotorControlArray's positionGains / velocityGains / forces; joint_controller.py:53-58, ik_controller.py:71-80)
    const int32_t* I = w->I.data(); const double* F = w->F.data();
    const int32_t* OI = I + I[DG_H_OFF_OP_I]; const int32_t* IL = I + I[DG_H_OFF_ILIST]; const double* OF = F + I[DG_H_OFF_OP_F]; const double* LF = F + I[DG_H_OFF_LINK_F];
    for (int op = 0; op < w->sc.nops; op++) {
      const int32_t* oi = OI + op * DG_OI_STRIDE; const double* of = OF + op * DG_OF_STRIDE; const int code = oi[DG_OI_CODE];
      if (code != DG_OP_JOINT_CONTROL && code != DG_OP_IK_CONTROL) continue;
      if (!((update_mask >> oi[DG_OI_SLOT]) & 1ull)) continue;
      if (code == DG_OP_JOINT_CONTROL && oi[DG_OI_FLAGS] == DG_JC_TORQUE) continue;
      const bool vel = code == DG_OP_JOINT_CONTROL && oi[DG_OI_FLAGS] == DG_JC_VELOCITY;
      for (int k = 0; k < oi[DG_OI_N]; k++) {
        const int gl = IL[oi[DG_OI_ILIST] + k];
        w->mt.v[3 * gl] = vel ? 0.f : (float)of[0]; w->mt.v[3 * gl + 1] = (float)of[1]; w->mt.v[3 * gl + 2] = (float)LF[gl * DG_LF_STRIDE + DG_LF_MAX_FORCE];
      }
    }
  }
  {
    const LaunchTable& lt = launch_table(w->lanes, w->mf); const bool prof = w->profile_cycles != nullptr;
    if (prof && !lt.has_prof) return fail(DG_ERR_UNSUPPORTED, "in-kernel stamps are not built for this workspace mode");
    if (w->par) lt.step_par(grid_of(w), w->lds_bytes, (hipStream_t)stream, prof, w->sc, w->mt, state, actions, update_mask, obs, rew, term, rew_sum, term_flag, w->diag, w->profile_cycles, nullptr, 0);
    else lt.step(grid_of(w), w->lds_bytes, (hipStream_t)stream, prof, w->sc, w->mt, state, actions, update_mask, obs, rew, term, rew_sum, term_flag, w->diag, w->profile_cycles, w->d_gws);
    HIP_TRY(hipGetLastError());
  }
  return DG_OK;
}

int32_t dg_world_render(dg_world* w, const float* state, int32_t camera, float* rgb, float* depth, int32_t* seg, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "null argument");
  if (camera < 0 || camera >= w->ncam) return fail(DG_ERR_ARG, "camera %d out of range (scene has %d)", camera, w->ncam);
  DG_ON_DEVICE(w->device);
  if (const int rc = launch_pose(w, stream, state, w->ncam, w->d_render_table, 0, -1, -1)) return rc;
  const int32_t* I = w->I.data(); const int32_t* ci = I + I[DG_H_OFF_CAMERA_I] + camera * DG_CI_STRIDE;
  // Rows per workgroup: a multiple of 8 (the tile height of render_kernel's wavefronts; 200-wide images: whole cache lines).
  // Every workgroup first builds its list of shapes, faces and vertices (phase A, a few microseconds of dependent loads),
  // so a workgroup should render as many rows as the machine's occupancy allows: about four workgroups per CU over the
  // whole launch -- with >= 1024 envs one workgroup renders a whole image.
  const int W = ci[DG_CI_WIDTH], H = ci[DG_CI_HEIGHT];
  if (W > 16 * 512) return fail(DG_ERR_UNSUPPORTED, "render: pictures wider than %d pixels are not supported (%d)", 16 * 512, W);  // DG_RTILE_CAP tiles per strip
  int band_rows;
  { const int want_blocks = 4 * std::max(w->cu_count, 1), bands_per_env = std::max(1, (want_blocks + w->num_envs - 1) / w->num_envs);
    band_rows = std::max(8, ((H + bands_per_env - 1) / bands_per_env + 7) / 8 * 8); }
  if (w->render_diag & 512) band_rows = H;  // (diag 512: one band per picture whatever the batch -- what a batch >= 4 x CUs gets; for tests)
  band_rows = std::min(band_rows, H);
  const int nbands = (H + band_rows - 1) / band_rows;
  const long long blocks = (long long)nbands * w->num_envs;  // the env index is folded into grid.x (grid.y stops at 65535)
  if (blocks > 0x7fffffffLL) return fail(DG_ERR_UNSUPPORTED, "render: %lld workgroups exceed the grid limit", blocks);
  auto render = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w->sc, w->d_CI, w->d_CF, w->d_PLN, camera, w->ncam,
                       (cfp)w->d_render_table, rgb, depth, seg, band_rows, nbands, w->render_diag);
  };
  if (w->render_wpe == 1) render(render_kernel<1>);
  else if (w->render_wpe == 3) render(render_kernel<3>);
  else render(render_kernel<2>);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}

// floats per env of dg_world_raycast's scratch: the shape rows of pose_kernel and the mount row
static size_t raycast_row_floats(const dg_world* w) { return (size_t)w->sc.nsh * RS_STRIDE + RC_STRIDE; }

int64_t dg_world_raycast_scratch_floats(const dg_world* w) {
  if (!w) { (void)fail(DG_ERR_ARG, "null world"); return 0; }
  return (int64_t)((size_t)w->num_envs * raycast_row_floats(w));
}

int32_t dg_world_raycast(dg_world* w, const float* state, int32_t body, int32_t frame, int32_t n_rays, const float* ray_from, const float* ray_to,
                         int32_t per_env, int32_t skip_body, float* scratch, float* frac, int32_t* id, float* pos, float* normal, void* stream) {
  if (!w || !state || !ray_from || !ray_to) return fail(DG_ERR_ARG, "null argument");
  if (n_rays <= 0) return fail(DG_ERR_ARG, "n_rays must be positive, got %d", n_rays);
  if (!frac) return fail(DG_ERR_ARG, "frac is NULL (id, pos and normal may be)");
  if (!scratch) return fail(DG_ERR_ARG, "scratch is NULL (dg_world_raycast_scratch_floats floats of device memory)");
  if (body < -1 || body >= w->sc.nb) return fail(DG_ERR_ARG, "body %d out of range", body);
  if (skip_body < -1 || skip_body >= w->sc.nb) return fail(DG_ERR_ARG, "skip_body %d out of range", skip_body);
  if (body < 0 && frame != -1) return fail(DG_ERR_ARG, "frame %d given without a body", frame);
  if (frame < -1) return fail(DG_ERR_ARG, "frame %d out of range", frame);
  int gf;
  if (const int rc = frame_check(w, body, frame, &gf, nullptr)) return rc;
  // one workgroup per (env, chunk of rays): a wavefront per 64 rays, at most four of them
  const int threads = 64 * std::min(4, (n_rays + 63) / 64), nchunks = (n_rays + threads - 1) / threads;
  const long long blocks = (long long)nchunks * w->num_envs;  // the env index is folded into grid.x
  if (blocks > 0x7fffffffLL) return fail(DG_ERR_UNSUPPORTED, "raycast: %lld workgroups exceed the grid limit", blocks);
  DG_ON_DEVICE(w->device);
  if (const int rc = launch_pose(w, stream, state, 0, scratch, 1, body, gf)) return rc;
  const int words = w->sc.nsh * RY_STRIDE;
  if (words <= w->ray_lds_words)
    hipLaunchKernelGGL(raycast_kernel<true>, dim3((unsigned)blocks), dim3(threads), sizeof(float) * (size_t)words, (hipStream_t)stream, w->sc, w->d_PLN, (cfp)scratch, n_rays, nchunks,
                       ray_from, ray_to, per_env != 0, body >= 0, skip_body, w->ray_no_cull, frac, id, pos, normal);
  else
    hipLaunchKernelGGL(raycast_kernel<false>, dim3((unsigned)blocks), dim3(threads), 0, (hipStream_t)stream, w->sc, w->d_PLN, (cfp)scratch, n_rays, nchunks,
                       ray_from, ray_to, per_env != 0, body >= 0, skip_body, w->ray_no_cull, frac, id, pos, normal);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}

// diagnostics: the LDS budget (in 4-byte words, at most DG_RAY_LDS_WORDS) of dg_world_raycast's staged shape rows; 0 sends every
// scene through the table-reading form of the kernel -- tests compare the two; not part of the public header
int32_t dg_debug_raycast_lds_words(dg_world* w, int32_t words) {
  if (!w || words < 0 || words > DG_RAY_LDS_WORDS) return fail(DG_ERR_ARG, "dg_debug_raycast_lds_words: bad argument");
  w->ray_lds_words = words;
  return DG_OK;
}

// diagnostics: dg_world_raycast without its bounding-sphere rejects (what the culled call must equal bit for bit); not part of the
// public header
int32_t dg_debug_raycast_no_cull(dg_world* w, int32_t on) {
  if (!w) return fail(DG_ERR_ARG, "null world");
  w->ray_no_cull = on != 0;
  return DG_OK;
}

// diagnostics: candidate counters of the render kernel (DG_RENDER_DIAG & 16); not part of the public header
int32_t dg_debug_render_counters(uint64_t* out16, int32_t reset) {
  unsigned long long h[16];
  HIP_TRY(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_render_count), sizeof h));
  for (int k = 0; k < 16; k++) out16[k] = h[k];
  if (reset) { memset(h, 0, sizeof h); HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_render_count), h, sizeof h)); }
  return DG_OK;
}

// the device buffers of the two hull diagnostics below, freed on every way out: both hulls' points, the poses [n][24], the output
// [n][out_floats] and the polytope workspace of the `blocks` wavefronts
struct HullDebugBufs {
  float *pts = nullptr, *poses = nullptr, *out = nullptr, *ws = nullptr; size_t blocks = 0;
  ~HullDebugBufs() { (void)hipFree(pts); (void)hipFree(poses); (void)hipFree(out); (void)hipFree(ws); }
};
static int hull_debug_upload(HullDebugBufs& b, const float* pts_a, int na, const float* pts_b, int nb, const float* poses, int n, int out_floats) {
  b.blocks = (size_t)((n + 63) / 64);
  HIP_TRY(hipMalloc(&b.ws, sizeof(float) * b.blocks * (size_t)HH_WS_SLOTS * 64));
  HIP_TRY(hipMalloc(&b.pts, sizeof(float) * 3 * (size_t)(na + nb))); HIP_TRY(hipMalloc(&b.poses, sizeof(float) * 24 * (size_t)n)); HIP_TRY(hipMalloc(&b.out, sizeof(float) * out_floats * (size_t)n));
  HIP_TRY(hipMemcpy(b.pts, pts_a, sizeof(float) * 3 * (size_t)na, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(b.pts + 3 * na, pts_b, sizeof(float) * 3 * (size_t)nb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b.poses, poses, sizeof(float) * 24 * (size_t)n, hipMemcpyHostToDevice));
  return DG_OK;
}
// diagnostics: the hull-against-hull narrow phase (dg_hull.h) on its own, one pair of poses per lane -- tests/test_hull_contacts.py
// compares it with the CPU checker and a brute-force Minkowski difference; host pointers; not part of the public header.
// poses [n][24] = A: rotation (9, row-major), position (3); B: the same.  out [n][12] = witness on A, witness on B, normal from B
// towards A, signed distance, 1 if the pair is nearer than max_dist (else the rest is undefined), GJK iterations the lane needed.
__global__ __launch_bounds__(64) void hull_pair_kernel(cfp pts, int na, int nb, const float* poses, int n, float max_dist, float* out, float* ws) {
  const int i = blockIdx.x * 64 + threadIdx.x; const bool have = i < n; const float* p = poses + 24 * (size_t)(have ? i : n - 1);
  HullPairD h; h.pa = pts; h.na = na; h.pb = pts + 3 * na; h.nb = nb;
#pragma unroll
  for (int k = 0; k < 9; k++) { h.RA.m[k] = p[k]; h.RB.m[k] = p[12 + k]; }
  const V3 ta = v3(p[9], p[10], p[11]), tb = v3(p[21], p[22], p[23]); h.tBA = tb - ta;
  V3 ca = v3(0.f, 0.f, 0.f), cb = ca;  // seed: the difference of the centroids, as the checker's test entry
  for (int k = 0; k < na; k++) ca = ca + v3(h.pa[3 * k], h.pa[3 * k + 1], h.pa[3 * k + 2]);
  for (int k = 0; k < nb; k++) cb = cb + v3(h.pb[3 * k], h.pb[3 * k + 1], h.pb[3 * k + 2]);
  const V3 seed = mul(h.RA, ca * (1.0f / (float)na)) - (mul(h.RB, cb * (1.0f / (float)nb)) + h.tBA);
  h.ew = hull_ws_of(ws); hull_tables(h, na <= 64 && nb <= 64);  // (every lane of the wavefront is here)
  HullHit r; hull_hull(h, seed, max_dist, have, r);
  if (have) { float* o = out + 12 * (size_t)i; o[11] = (float)r.iters; const V3 pa = r.pa + ta, pb = r.pb + ta;
    o[0] = pa.x; o[1] = pa.y; o[2] = pa.z; o[3] = pb.x; o[4] = pb.y; o[5] = pb.z; o[6] = r.n.x; o[7] = r.n.y; o[8] = r.n.z; o[9] = r.dist; o[10] = r.hit ? 1.f : 0.f; }
}
int32_t dg_debug_hull_hull(const float* pts_a, int32_t na, const float* pts_b, int32_t nb, const float* poses, int32_t n, float max_dist, float* out11 /* [n][12] */) {
  if (!pts_a || !pts_b || !poses || !out11 || na < 1 || nb < 1 || na > 256 || nb > 256 || n < 1) return fail(DG_ERR_ARG, "dg_debug_hull_hull: bad argument");
  HullDebugBufs b;
  if (const int rc = hull_debug_upload(b, pts_a, na, pts_b, nb, poses, n, 12)) return rc;
  hipLaunchKernelGGL(hull_pair_kernel, dim3((unsigned)b.blocks), dim3(64), 0, (hipStream_t)0, (cfp)b.pts, na, nb, (const float*)b.poses, n, max_dist, b.out, b.ws);
  HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out11, b.out, sizeof(float) * 12 * (size_t)n, hipMemcpyDeviceToHost));
  return DG_OK;
}

// diagnostics: the contacts the narrow phase makes of one hull pair with DG_HF_HULL_MANIFOLD = npts (dg_hull.h hull_manifold after
// hull_hull, as dg_solver.h collide calls them), one pair of poses per lane -- tests/test_hull_manifold.py compares it with its numpy
// restatement; host pointers; not part of the public header.  poses [n][24] as dg_debug_hull_hull; rad_a, rad_b: the hulls' bounding
// radii (the feature tolerance scales with them).  out [n][25] = contacts (0..npts), 1 if that is the pair's single contact (no
// manifold), normal from B towards A (3), then per slot s < 4: point (3, world), depth (distance - 2 x hull_margin), key feature,
// unused slots zero.
__global__ __launch_bounds__(64) void hull_manifold_kernel(cfp pts, int na, int nb, float rad_a, float rad_b, const float* poses, int n, float margin,
                                                            float hmg, int npts, float* out, float* ws) {
  const int i = blockIdx.x * 64 + threadIdx.x; const bool have = i < n; const float* p = poses + 24 * (size_t)(have ? i : n - 1);
  HullPairD h; h.pa = pts; h.na = na; h.pb = pts + 3 * na; h.nb = nb;
#pragma unroll
  for (int k = 0; k < 9; k++) { h.RA.m[k] = p[k]; h.RB.m[k] = p[12 + k]; }
  const V3 ta = v3(p[9], p[10], p[11]), tb = v3(p[21], p[22], p[23]); h.tBA = tb - ta;
  V3 ca = v3(0.f, 0.f, 0.f), cb = ca;  // (seed as dg_debug_hull_hull)
  for (int k = 0; k < na; k++) ca = ca + v3(h.pa[3 * k], h.pa[3 * k + 1], h.pa[3 * k + 2]);
  for (int k = 0; k < nb; k++) cb = cb + v3(h.pb[3 * k], h.pb[3 * k + 1], h.pb[3 * k + 2]);
  const V3 seed = mul(h.RA, ca * (1.0f / (float)na)) - (mul(h.RB, cb * (1.0f / (float)nb)) + h.tBA);
  h.ew = hull_ws_of(ws); hull_tables(h, na <= 64 && nb <= 64);
  HullHit hh; hull_hull(h, seed, margin + 2.f * hmg, have, hh);
  const bool hit = hh.hit && hh.dist - 2.f * hmg < margin;
  const int m = npts > 1 ? hull_manifold(h, hh.n, rad_a, rad_b, margin, hmg, npts, hit) : 0;
  if (!have) return;
  float* o = out + 25 * (size_t)i;
  for (int k = 0; k < 25; k++) o[k] = 0.f;
  if (!hit) return;
  o[0] = (float)(m > 0 ? m : 1); o[1] = m > 0 ? 0.f : 1.f; o[2] = hh.n.x; o[3] = hh.n.y; o[4] = hh.n.z;
  if (m == 0) {
    const V3 pa = (hh.pa + ta) - hh.n * hmg, pb = (hh.pb + ta) + hh.n * hmg, c = (pa + pb) * 0.5f;
    o[5] = c.x; o[6] = c.y; o[7] = c.z; o[8] = hh.dist - 2.f * hmg; o[9] = 0.f;
  } else {
    const HEpa E = {h.ew};
    for (int s = 0; s < m; s++) {
      o[5 + 5 * s] = E.F(MF_R + 4 * s) + ta.x; o[6 + 5 * s] = E.F(MF_R + 4 * s + 1) + ta.y; o[7 + 5 * s] = E.F(MF_R + 4 * s + 2) + ta.z;
      o[8 + 5 * s] = E.F(MF_R + 4 * s + 3); o[9 + 5 * s] = (float)s;
    }
  }
}
int32_t dg_debug_hull_manifold(const float* pts_a, int32_t na, const float* pts_b, int32_t nb, float rad_a, float rad_b, const float* poses, int32_t n,
                               float margin, float hull_margin, int32_t npts, float* out25 /* [n][25] */) {
  if (!pts_a || !pts_b || !poses || !out25 || na < 1 || nb < 1 || na > 256 || nb > 256 || n < 1 || npts < 1 || npts > 4)
    return fail(DG_ERR_ARG, "dg_debug_hull_manifold: bad argument");
  HullDebugBufs b;
  if (const int rc = hull_debug_upload(b, pts_a, na, pts_b, nb, poses, n, 25)) return rc;
  hipLaunchKernelGGL(hull_manifold_kernel, dim3((unsigned)b.blocks), dim3(64), 0, (hipStream_t)0, (cfp)b.pts, na, nb, rad_a, rad_b, (const float*)b.poses, n,
                     margin, hull_margin, (int)npts, b.out, b.ws);
  HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out25, b.out, sizeof(float) * 25 * (size_t)n, hipMemcpyDeviceToHost));
  return DG_OK;
}

int32_t dg_world_set_profile_buffer(dg_world* w, uint64_t* cycles) { if (!w) return fail(DG_ERR_ARG, "null world"); w->profile_cycles = (unsigned long long*)cycles; return DG_OK; }

int32_t dg_world_observe(dg_world* w, const float* state, float* obs, float* rew, uint8_t* term, float* rew_sum, uint8_t* term_flag, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "null argument");
  return launch(w, stream, &LaunchTable::observe, state, obs, rew, term, rew_sum, term_flag);
}

int32_t dg_world_frame_state(dg_world* w, const float* state, int32_t body, int32_t frame, int32_t com, float* out, void* stream) {
  if (!w || !state || !out) return fail(DG_ERR_ARG, "null argument");
  int gf;
  if (const int rc = body_check(w, body, nullptr)) return rc;
  if (const int rc = frame_check(w, body, frame, &gf, nullptr)) return rc;
  return launch(w, stream, &LaunchTable::frame, state, body, gf, com, out);
}

int32_t dg_world_set_render_diag(dg_world* w, int32_t flags) {
  if (!w) return fail(DG_ERR_ARG, "null argument");
  w->render_diag = flags;
  return DG_OK;
}

int32_t dg_world_apply_wrench(dg_world* w, float* state, int32_t body, int32_t frame, int32_t flags, const float* force, const float* pos,
                              const float* torque, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "null argument");
  int gf;
  if (const int rc = body_check(w, body, nullptr)) return rc;
  if (body_row(w, body)[DG_BI_FLAGS] & DG_BODY_FROZEN) return fail(DG_ERR_ARG, "body %d is part of the frozen static world: it has no state to push on", body);
  if (flags != DG_WRENCH_WORLD_FRAME && flags != DG_WRENCH_LINK_FRAME) return fail(DG_ERR_ARG, "flags must be DG_WRENCH_LINK_FRAME (1) or DG_WRENCH_WORLD_FRAME (2)");
  if (const int rc = frame_check(w, body, frame, &gf, nullptr)) return rc;
  if (!force && !torque) return DG_OK;
  return launch(w, stream, &LaunchTable::wrench, state, body, gf, flags == DG_WRENCH_LINK_FRAME ? 1 : 0, force, pos, torque);
}

// ------------------------------------------------------------------ dynamics queries (dg_dynq.h)
// the checks the five entries share: a fixed-base body with joints whose passes fit the transient region; 0 or the error code
static int dynq_check(const dg_world* w, const void* state, int32_t body, int kind, const char* what) {
  if (!w || !state) return fail(DG_ERR_ARG, "%s: null argument", what);
  if (const int rc = body_check(w, body, what)) return rc;
  const int32_t* B = body_row(w, body);
  if (B[DG_BI_FLAGS] & DG_BODY_FROZEN) return fail(DG_ERR_ARG, "%s: body %d is part of the frozen static world: it has no joints", what, body);
  if (!(B[DG_BI_FLAGS] & DG_BODY_FIXED)) return fail(DG_ERR_ARG, "%s: body %d has a floating base; the dynamics queries take fixed-base bodies only", what, body);
  if (B[DG_BI_N_LINKS] < 1) return fail(DG_ERR_ARG, "%s: body %d has no joints", what, body);
  if (kind >= 0 && dynq_slots(kind, B[DG_BI_N_LINKS]) > w->sc.tr_slots) return slots_refusal(w, body, dynq_slots(kind, B[DG_BI_N_LINKS]), what);
  return DG_OK;
}

int32_t dg_world_joint_state(dg_world* w, const float* state, int32_t body, float* q_out, float* qd_out, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_joint_state")) return rc;
  if (!q_out && !qd_out) return DG_OK;
  return launch(w, stream, &LaunchTable::joint_state, state, body, q_out, qd_out);
}

int32_t dg_world_jacobian(dg_world* w, const float* state, int32_t body, int32_t frame, const float* local_pos, const float* q, float* jac_t, float* jac_r, void* stream) {
  if (const int rc = dynq_check(w, state, body, DQ_KIND_JACOBIAN, "dg_world_jacobian")) return rc;
  if (!local_pos) return fail(DG_ERR_ARG, "dg_world_jacobian: local_pos is NULL (three host floats)");
  if (frame < 0) return fail(DG_ERR_ARG, "dg_world_jacobian: frame %d out of range (the base of a fixed body does not move)", frame);
  int gf;
  if (const int rc = frame_check(w, body, frame, &gf, "dg_world_jacobian")) return rc;
  if (!jac_t && !jac_r) return DG_OK;
  return launch(w, stream, &LaunchTable::jacobian, state, body, gf, local_pos[0], local_pos[1], local_pos[2], q, jac_t, jac_r);
}

int32_t dg_world_inverse_dynamics(dg_world* w, const float* state, int32_t body, const float* q, const float* qd, const float* qdd, float* tau, void* stream) {
  if (const int rc = dynq_check(w, state, body, DQ_KIND_ID, "dg_world_inverse_dynamics")) return rc;
  if (!tau) return fail(DG_ERR_ARG, "dg_world_inverse_dynamics: tau is NULL");
  return launch(w, stream, &LaunchTable::inverse_dynamics, state, body, q, qd, qdd, tau);
}

int32_t dg_world_mass_matrix(dg_world* w, const float* state, int32_t body, const float* q, float* M, void* stream) {
  if (const int rc = dynq_check(w, state, body, DQ_KIND_MASS, "dg_world_mass_matrix")) return rc;
  if (!M) return fail(DG_ERR_ARG, "dg_world_mass_matrix: M is NULL");
  return launch(w, stream, &LaunchTable::mass_matrix, state, body, q, M);
}

int32_t dg_world_apply_joint_torque(dg_world* w, float* state, int32_t body, const float* tau, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_apply_joint_torque")) return rc;
  if (!tau) return fail(DG_ERR_ARG, "dg_world_apply_joint_torque: tau is NULL");
  return launch(w, stream, &LaunchTable::joint_torque, state, body, tau);
}

// ------------------------------------------------------------------ inverse-kinematics query, motor targets, joint reset (dg_ikq.h)
int32_t dg_world_inverse_kinematics(dg_world* w, const float* state, int32_t body, int32_t frame, const float* target_pos, const float* target_orn,
                                    const float* lists, const float* q0, float* q_out, int32_t* iters_out, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_inverse_kinematics")) return rc;
  const int n = body_row(w, body)[DG_BI_N_LINKS];
  if (ikq_slots(n) > w->sc.tr_slots) return slots_refusal(w, body, ikq_slots(n), "dg_world_inverse_kinematics");
  if (frame < 0) return fail(DG_ERR_ARG, "dg_world_inverse_kinematics: frame %d out of range (the base of a fixed body does not move)", frame);
  int gf;
  if (const int rc = frame_check(w, body, frame, &gf, "dg_world_inverse_kinematics")) return rc;
  if (!target_pos) return fail(DG_ERR_ARG, "dg_world_inverse_kinematics: target_pos is NULL");
  if (!q_out) return fail(DG_ERR_ARG, "dg_world_inverse_kinematics: q_out is NULL");
  return launch(w, stream, &LaunchTable::ik_query, state, body, gf, target_pos, target_orn, lists, q0, q_out, iters_out);
}

// a mask other than all ones cannot name the joints past the 64th
static int joint_mask_check(const dg_world* w, int32_t body, uint64_t joint_mask, const char* what) {
  const int n = body_row(w, body)[DG_BI_N_LINKS];
  if (n > 64 && joint_mask != ~0ull) return fail(DG_ERR_ARG, "%s: body %d has %d joints; a partial joint mask covers 64", what, body, n);
  return DG_OK;
}

int32_t dg_world_set_joint_targets(dg_world* w, float* state, int32_t body, uint64_t joint_mask, const float* pos, const float* vel, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_set_joint_targets")) return rc;
  if (const int rc = joint_mask_check(w, body, joint_mask, "dg_world_set_joint_targets")) return rc;
  if (!pos && !vel) return fail(DG_ERR_ARG, "dg_world_set_joint_targets: pos and vel are both NULL");
  return launch(w, stream, &LaunchTable::joint_targets, state, body, joint_mask, pos, vel);
}

int32_t dg_world_reset_joint_state(dg_world* w, float* state, int32_t body, uint64_t joint_mask, const float* q, const float* qd, const uint8_t* env_mask, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_reset_joint_state")) return rc;
  if (const int rc = joint_mask_check(w, body, joint_mask, "dg_world_reset_joint_state")) return rc;
  if (!q) return fail(DG_ERR_ARG, "dg_world_reset_joint_state: q is NULL");
  return launch(w, stream, &LaunchTable::joint_reset, state, body, joint_mask, q, qd, env_mask);
}

// ------------------------------------------------------------------ link states, base reset (dg_stateq.h)
int32_t dg_world_link_states(dg_world* w, const float* state, const int32_t* bodies, const int32_t* frames, int32_t n, int32_t com, float* out, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "dg_world_link_states: null argument");
  if (!bodies || !frames || !out) return fail(DG_ERR_ARG, "dg_world_link_states: bodies, frames or out is NULL");
  if (n < 1 || n > DG_LINK_STATES_MAX) return fail(DG_ERR_ARG, "dg_world_link_states: n must be 1 .. %d, got %d", (int)DG_LINK_STATES_MAX, n);
  LsSelectors sel; memset(&sel, 0, sizeof sel); sel.n = n;
  for (int k = 0; k < n; k++) {  // what dg_world_frame_state takes, selector by selector
    const int body = bodies[k], frame = frames[k]; int gf;
    if (body < 0 || body >= w->sc.nb) return fail(DG_ERR_ARG, "dg_world_link_states: bodies[%d] = %d out of range", k, body);
    if (!frame_lookup(w, body, frame, &gf)) return fail(DG_ERR_ARG, "dg_world_link_states: body %d has no frame %d (selector %d)", body, frame, k);
    sel.body[k] = body; sel.frame[k] = gf;
  }
  return launch(w, stream, &LaunchTable::link_states, state, sel, com, out);
}

// A base can be moved only where the planner did not assume it stays at its load pose (scene.py: `frozen`, `anchored` -- static
// pair pruning, anchored bounding spheres): a floating base, or a fixed base that carries a DG_OP_RESPAWN.  Decided here from the
// tables the world holds; no scene table has a column for it.
int32_t dg_world_reset_base_state(dg_world* w, float* state, int32_t body, const float* pos, const float* orn, const float* lin_vel, const float* ang_vel,
                                  const uint8_t* env_mask, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "dg_world_reset_base_state: null argument");
  if (const int rc = body_check(w, body, "dg_world_reset_base_state")) return rc;
  if ((pos == nullptr) != (orn == nullptr)) return fail(DG_ERR_ARG, "dg_world_reset_base_state: pos and orn go together (both or neither)");
  if (!pos && !lin_vel && !ang_vel) return fail(DG_ERR_ARG, "dg_world_reset_base_state: nothing to write (pos, orn, lin_vel and ang_vel are all NULL)");
  const int32_t* I = w->I.data(); const int flags = body_row(w, body)[DG_BI_FLAGS];
  if (flags & DG_BODY_FIXED) {
    bool respawned = false; const int32_t* OI = I + I[DG_H_OFF_OP_I];
    for (int op = 0; op < w->sc.nops; op++) respawned = respawned || (OI[op * DG_OI_STRIDE + DG_OI_CODE] == DG_OP_RESPAWN && OI[op * DG_OI_STRIDE + DG_OI_BODY] == body);
    if ((flags & DG_BODY_FROZEN) || !respawned)
      return fail(DG_ERR_ARG, "dg_world_reset_base_state: body %d has a fixed base that the scene pins to its load pose; add a respawn addon to the model "
                              "(zero ranges will do) to make its base movable", body);
    if (lin_vel || ang_vel) return fail(DG_ERR_ARG, "dg_world_reset_base_state: body %d has a fixed base: it takes a pose, no velocity", body);
  }
  return launch(w, stream, &LaunchTable::reset_base, state, body, pos, orn, lin_vel, ang_vel, env_mask);
}

// ------------------------------------------------------------------ contact query (dg_contactq.h)
// a (body, link) filter of dg_world_contacts / dg_world_closest (`what`): 0 or the error code
static int contact_filter_check(const dg_world* w, int32_t body, int32_t link, const char* side, const char* what = "dg_world_contacts") {
  if (body == DG_CONTACT_ANY) {
    if (link != DG_CONTACT_ANY) return fail(DG_ERR_ARG, "%s: link_%s %d given without body_%s", what, side, link, side);
    return DG_OK;
  }
  if (body < 0 || body >= w->sc.nb) return fail(DG_ERR_ARG, "%s: body_%s %d out of range", what, side, body);
  if (link == DG_CONTACT_ANY || link == -1) return DG_OK;
  // A link the body has: one that a shape of the body carries in its id (the value the filter is compared with -- for the shapes of
  // a rigidly merged child model that is the CHILD's own link index), or one of the body's frames (a link without collision shapes)
  if (link >= 0) {
    const int32_t* I = w->I.data(); const int32_t* SI = I + I[DG_H_OFF_SHAPE_I];
    for (int s = 0; s < w->sc.nsh; s++)
      if (SI[s * DG_SI_STRIDE + DG_SI_BODY] == body && ((SI[s * DG_SI_STRIDE + DG_SI_FLAGS] >> 8) & 0xFFFF) - 1 == link) return DG_OK;
    if (global_frame(w, body, link) >= 0) return DG_OK;
  }
  return fail(DG_ERR_ARG, "%s: body %d has no link %d", what, body, link);
}

int32_t dg_world_contacts(dg_world* w, const float* state, int32_t body_a, int32_t link_a, int32_t body_b, int32_t link_b, int32_t* count, int32_t* ids,
                          float* geom, float* force, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "dg_world_contacts: null argument");
  if (!count) return fail(DG_ERR_ARG, "dg_world_contacts: count is NULL (ids, geom and force may be)");
  if (const int rc = contact_filter_check(w, body_a, link_a, "a")) return rc;
  if (const int rc = contact_filter_check(w, body_b, link_b, "b")) return rc;
  if (force) if (const int rc = impulse_cache_check(w, "dg_world_contacts")) return rc;
  // the grid and block of reset_kernel: one wavefront per workgroup, as many workgroups as the step has (dg_contactq.h, Workspace)
  return launch(w, stream, &LaunchTable::contact_query, state, body_a, link_a, body_b, link_b, count, ids, geom, force);
}

// ------------------------------------------------------------------ contact forces (dg_contactf.h)
int32_t dg_world_contact_forces(dg_world* w, const float* state, int32_t body_a, int32_t link_a, int32_t body_b, int32_t link_b, int32_t* count, int32_t* ids,
                                float* forces, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "dg_world_contact_forces: null argument");
  if (!count) return fail(DG_ERR_ARG, "dg_world_contact_forces: count is NULL (ids and forces may be)");
  if (const int rc = contact_filter_check(w, body_a, link_a, "a", "dg_world_contact_forces")) return rc;
  if (const int rc = contact_filter_check(w, body_b, link_b, "b", "dg_world_contact_forces")) return rc;
  if (const int rc = impulse_cache_check(w, "dg_world_contact_forces")) return rc;
  // the grid and block of reset_kernel, as dg_world_contacts (dg_contactq.h, Workspace)
  return launch(w, stream, &LaunchTable::contact_force, state, body_a, link_a, body_b, link_b, count, ids, forces);
}

int32_t dg_world_net_contact_wrench(dg_world* w, const float* state, int32_t body, const int32_t* links, int32_t n, int32_t body_b, int32_t link_b,
                                    float* wrench, int32_t* ncontacts, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "dg_world_net_contact_wrench: null argument");
  if (!links || !wrench) return fail(DG_ERR_ARG, "dg_world_net_contact_wrench: links or wrench is NULL (ncontacts may be)");
  if (n < 1 || n > DG_CONTACT_MAX_LINKS) return fail(DG_ERR_ARG, "dg_world_net_contact_wrench: n must be 1 .. %d, got %d", (int)DG_CONTACT_MAX_LINKS, n);
  if (const int rc = body_check(w, body, "dg_world_net_contact_wrench")) return rc;
  CfSelectors sel; memset(&sel, 0, sizeof sel); sel.n = n;
  for (int s = 0; s < n; s++) {  // DG_CONTACT_ANY or a frame of the body: the moment needs the link's inertial frame
    const int link = links[s]; int gf = -1;
    if (link != DG_CONTACT_ANY && link != -1 && (link < 0 || (gf = global_frame(w, body, link)) < 0))
      return fail(DG_ERR_ARG, "dg_world_net_contact_wrench: links[%d] = %d is not a frame of body %d (DG_CONTACT_ANY: the whole body)", s, link, body);
    sel.link[s] = link; sel.frame[s] = gf;
  }
  if (const int rc = contact_filter_check(w, body_b, link_b, "b", "dg_world_net_contact_wrench")) return rc;
  if (const int rc = impulse_cache_check(w, "dg_world_net_contact_wrench")) return rc;
  return launch(w, stream, &LaunchTable::net_contact_wrench, state, body, sel, body_b, link_b, wrench, ncontacts);
}

// ------------------------------------------------------------------ joint reaction wrenches, applied motor torques (dg_jointq.h)
int32_t dg_world_joint_wrench(dg_world* w, const float* state, int32_t body, const dg_joint_selector* selectors, int32_t n, float* wrench, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "dg_world_joint_wrench: null argument");
  if (!selectors || !wrench) return fail(DG_ERR_ARG, "dg_world_joint_wrench: selectors or wrench is NULL");
  if (n < 1 || n > DG_JOINT_WRENCH_MAX) return fail(DG_ERR_ARG, "dg_world_joint_wrench: n must be 1 .. %d, got %d", (int)DG_JOINT_WRENCH_MAX, n);
  if (const int rc = body_check(w, body, "dg_world_joint_wrench")) return rc;
  const int32_t* I = w->I.data(); const int32_t* B = body_row(w, body);
  if (B[DG_BI_FLAGS] & DG_BODY_FROZEN) return fail(DG_ERR_ARG, "dg_world_joint_wrench: body %d is part of the frozen static world: it has no joints", body);
  if (B[DG_BI_PREV_OFF] < 0)
    return fail(DG_ERR_ARG, "dg_world_joint_wrench: body %d keeps no saved velocities; call builder.enable_joint_force_torque(body) while the scene is built "
                            "(joint_wrench_sensor does), or put a compiled force_torque_sensor on the body", body);
  const int nl = B[DG_BI_N_LINKS]; int nfr = 0;
  for (int f = 0; f < w->sc.nfr; f++) nfr += I[I[DG_H_OFF_FRAME_I] + f * DG_FI_STRIDE + DG_FI_BODY] == body;
  if (nl > 64 || nfr > 64) return fail(DG_ERR_ARG, "dg_world_joint_wrench: body %d has %d links and %d frames; the selectors' masks cover 64", body, nl, nfr);
  if (jointq_slots(nl) > w->sc.tr_slots) return slots_refusal(w, body, jointq_slots(nl), "dg_world_joint_wrench");
  JwSelectors sel; memset(&sel, 0, sizeof sel); sel.n = n;
  for (int s = 0; s < n; s++) {
    const dg_joint_selector& js = selectors[s]; int gf;
    if (js.frame < 0 || !frame_lookup(w, body, js.frame, &gf)) return fail(DG_ERR_ARG, "dg_world_joint_wrench: body %d has no frame %d (selector %d)", body, js.frame, s);
    if ((nl < 64 && (js.link_mask >> nl)) || (nfr < 64 && (js.frame_mask >> nfr)))
      return fail(DG_ERR_ARG, "dg_world_joint_wrench: selector %d names a link or frame past the body's %d links and %d frames", s, nl, nfr);
    if ((js.flags & DG_FT_WHOLE_LINK) && I[I[DG_H_OFF_FRAME_I] + gf * DG_FI_STRIDE + DG_FI_LINK] < 0)
      return fail(DG_ERR_ARG, "dg_world_joint_wrench: selector %d asks for the whole moving link of frame %d, which sits on the base", s, js.frame);
    sel.s[s] = js; sel.s[s].frame = gf;
  }
  if (w->sc.npairs > 0 && w->sc.warm_off < 0)
    return fail(DG_ERR_UNSUPPORTED, "dg_world_joint_wrench: the world keeps no contact impulse cache (warmstart and warmstart_friction are 0): no contact forces "
                                    "to take off the child side");
  // the grid and block of reset_kernel, as dg_world_contacts (dg_contactq.h, Workspace)
  return launch(w, stream, &LaunchTable::joint_wrench, state, body, sel, wrench);
}

int32_t dg_world_joint_efforts(dg_world* w, const float* state, int32_t body, float* out, void* stream) {
  if (!w || !state || !out) return fail(DG_ERR_ARG, "dg_world_joint_efforts: null argument");
  if (const int rc = body_check(w, body, "dg_world_joint_efforts")) return rc;
  const int32_t* B = body_row(w, body);
  if (B[DG_BI_FLAGS] & DG_BODY_FROZEN) return fail(DG_ERR_ARG, "dg_world_joint_efforts: body %d is part of the frozen static world: it has no joints", body);
  if (B[DG_BI_N_LINKS] < 1) return fail(DG_ERR_ARG, "dg_world_joint_efforts: body %d has no joints", body);
  return launch(w, stream, &LaunchTable::joint_effort, state, body, out);
}

// ------------------------------------------------------------------ link accelerations, IMU readings (dg_accelq.h)
int32_t dg_world_link_accelerations(dg_world* w, const float* state, int32_t body, const dg_accel_selector* selectors, int32_t n, float* out, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "dg_world_link_accelerations: null argument");
  if (!selectors || !out) return fail(DG_ERR_ARG, "dg_world_link_accelerations: selectors or out is NULL");
  if (n < 1 || n > DG_LINK_ACCEL_MAX) return fail(DG_ERR_ARG, "dg_world_link_accelerations: n must be 1 .. %d, got %d", (int)DG_LINK_ACCEL_MAX, n);
  if (const int rc = body_check(w, body, "dg_world_link_accelerations")) return rc;
  const int32_t* B = body_row(w, body);
  if (B[DG_BI_FLAGS] & DG_BODY_FROZEN) return fail(DG_ERR_ARG, "dg_world_link_accelerations: body %d is part of the frozen static world: it never moves", body);
  if (B[DG_BI_PREV_OFF] < 0)
    return fail(DG_ERR_ARG, "dg_world_link_accelerations: body %d keeps no saved velocities; call builder.enable_joint_force_torque(body) while the scene is built "
                            "(imu_sensor does), or put a compiled force_torque_sensor on the body; a fixed base without joints keeps none", body);
  const int nl = B[DG_BI_N_LINKS];
  if (jointq_slots(nl) > w->sc.tr_slots) return slots_refusal(w, body, jointq_slots(nl), "dg_world_link_accelerations");
  LaSelectors sel; memset(&sel, 0, sizeof sel); sel.n = n;
  for (int s = 0; s < n; s++) {
    const dg_accel_selector& as = selectors[s]; int gf;
    if (as.frame < -1 || !frame_lookup(w, body, as.frame, &gf))
      return fail(DG_ERR_ARG, "dg_world_link_accelerations: body %d has no frame %d (selector %d)", body, as.frame, s);
    const double qn = std::sqrt((double)as.quat[0] * as.quat[0] + (double)as.quat[1] * as.quat[1] + (double)as.quat[2] * as.quat[2] + (double)as.quat[3] * as.quat[3]);
    if (!(qn > 0.0) || !std::isfinite(qn)) return fail(DG_ERR_ARG, "dg_world_link_accelerations: the mount quaternion of selector %d has zero norm", s);
    sel.s[s] = as; sel.s[s].frame = gf; sel.s[s].com = as.com != 0;
    for (int k = 0; k < 4; k++) sel.s[s].quat[k] = (float)(as.quat[k] / qn);
  }
  const double gn = std::sqrt((double)w->sc.gx * w->sc.gx + (double)w->sc.gy * w->sc.gy + (double)w->sc.gz * w->sc.gz);
  if (gn > 0.0) { sel.ghat[0] = (float)(w->sc.gx / gn); sel.ghat[1] = (float)(w->sc.gy / gn); sel.ghat[2] = (float)(w->sc.gz / gn); }
  // the grid and block of reset_kernel, as dg_world_joint_wrench
  return launch(w, stream, &LaunchTable::link_accel, state, body, sel, out);
}

// ------------------------------------------------------------------ task-space dynamics (dg_taskq.h)
int32_t dg_world_task_space(dg_world* w, const float* state, int32_t body, int32_t frame, const float* local_pos, int32_t axes_mask, const float* q, const float* qd,
                            const float* acc, const float* tau_null, float damping, float* jac, float* bias_acc, float* bias_torque, float* lambda, float* tau,
                            float* point, int32_t* singular, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_task_space")) return rc;
  if (!local_pos) return fail(DG_ERR_ARG, "dg_world_task_space: local_pos is NULL (three host floats)");
  if (frame < 0) return fail(DG_ERR_ARG, "dg_world_task_space: frame %d out of range (the base of a fixed body does not move)", frame);
  int gf;
  if (const int rc = frame_check(w, body, frame, &gf, "dg_world_task_space")) return rc;
  if (axes_mask <= 0 || axes_mask > 63) return fail(DG_ERR_ARG, "dg_world_task_space: axes_mask %d selects no row or a row above 5 of [v; w]", axes_mask);
  const int n = body_row(w, body)[DG_BI_N_LINKS], m = __builtin_popcount((unsigned)axes_mask);
  if (m > n) return fail(DG_ERR_ARG, "dg_world_task_space: %d task rows for a body of %d joints", m, n);
  if (!(damping >= 0.f) || !std::isfinite(damping)) return fail(DG_ERR_ARG, "dg_world_task_space: damping must be finite and >= 0, got %g", (double)damping);
  if (!jac && !bias_acc && !bias_torque && !lambda && !tau && !point && !singular) return fail(DG_ERR_ARG, "dg_world_task_space: every output is NULL");
  if (tau && !acc) return fail(DG_ERR_ARG, "dg_world_task_space: tau needs acc");
  if (tau_null && !tau) return fail(DG_ERR_ARG, "dg_world_task_space: tau_null without tau");
  if (taskq_slots(n, m) > w->sc.tr_slots) return slots_refusal(w, body, taskq_slots(n, m), "dg_world_task_space");
  return launch(w, stream, &LaunchTable::task_space, state, body, gf, local_pos[0], local_pos[1], local_pos[2], (int)axes_mask, q, qd, acc, tau_null, damping,
                jac, bias_acc, bias_torque, lambda, tau, point, singular);
}

// ------------------------------------------------------------------ forward dynamics, joint-space rollouts (dg_fdq.h)
int32_t dg_world_forward_dynamics(dg_world* w, const float* state, int32_t body, const float* q, const float* qd, const float* tau, int32_t joint_damping,
                                  float* qdd, int32_t* singular, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_forward_dynamics")) return rc;
  if (!qdd && !singular) return fail(DG_ERR_ARG, "dg_world_forward_dynamics: qdd and singular are both NULL");
  const int n = body_row(w, body)[DG_BI_N_LINKS];
  if (fdq_slots(n) > w->sc.tr_slots) return slots_refusal(w, body, fdq_slots(n), "dg_world_forward_dynamics");
  return launch(w, stream, &LaunchTable::forward_dynamics, state, body, q, qd, tau, joint_damping != 0 ? 1 : 0, qdd, singular);
}

// workgroups of a dg_world_rollout of K samples per env: one item per lane; in the global-workspace modes no more than the step's
// grid, which is what d_gws is sized for (rollout_kernel strides over the rest)
static unsigned rollout_grid(const dg_world* w, int64_t K) {
  const int64_t per = envs_per_wave(w->lanes), want = ((int64_t)w->num_envs * K + per - 1) / per, cap = (int64_t)grid_of(w).x;
  if (w->lanes <= 0 && want > cap) return (unsigned)cap;
  return (unsigned)(want > (int64_t)1 << 30 ? (int64_t)1 << 30 : want);  // (a grid dimension stays below 2^31; the kernel strides)
}

int32_t dg_world_rollout(dg_world* w, const float* state, int32_t body, int32_t frame, const float* local_pos, int32_t K, int32_t T, float dt, int32_t joint_damping,
                         const float* q0, const float* qd0, const float* tau, float* q_out, float* qd_out, float* pos_out, int32_t* singular, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_rollout")) return rc;
  if (K < 1) return fail(DG_ERR_ARG, "dg_world_rollout: K must be >= 1, got %d", K);
  if (T < 1) return fail(DG_ERR_ARG, "dg_world_rollout: T must be >= 1, got %d", T);
  if (!std::isfinite(dt) || !(dt > 0.f)) return fail(DG_ERR_ARG, "dg_world_rollout: dt must be finite and > 0, got %g", (double)dt);
  if (!tau) return fail(DG_ERR_ARG, "dg_world_rollout: tau is NULL");
  if (!q_out && !qd_out && !pos_out && !singular) return fail(DG_ERR_ARG, "dg_world_rollout: every output is NULL");
  const int n = body_row(w, body)[DG_BI_N_LINKS];
  {  // B K T n floats stay addressable in bytes
    const int64_t lim = INT64_MAX / 4; int64_t v = w->num_envs;
    for (const int64_t f : {(int64_t)K, (int64_t)T, (int64_t)n}) { if (v > lim / f) return fail(DG_ERR_ARG, "dg_world_rollout: %d envs x K %d x T %d x %d joints is beyond INT64_MAX / 4 values", w->num_envs, K, T, n); v *= f; }
  }
  int gf = -1; float lp[3] = {0.f, 0.f, 0.f};
  if (pos_out) {
    if (!local_pos) return fail(DG_ERR_ARG, "dg_world_rollout: local_pos is NULL (three host floats)");
    if (frame < 0) return fail(DG_ERR_ARG, "dg_world_rollout: frame %d out of range (the base of a fixed body does not move)", frame);
    if (const int rc = frame_check(w, body, frame, &gf, "dg_world_rollout")) return rc;
    lp[0] = local_pos[0]; lp[1] = local_pos[1]; lp[2] = local_pos[2];
  }
  if (fdq_slots(n) > w->sc.tr_slots) return slots_refusal(w, body, fdq_slots(n), "dg_world_rollout");
  return launch_grid(w, dim3(rollout_grid(w, K)), stream, &LaunchTable::rollout, state, body, gf, lp[0], lp[1], lp[2], (int)K, (int)T, dt, joint_damping != 0 ? 1 : 0,
                     q0, qd0, tau, q_out, qd_out, pos_out, singular, w->d_gws);
}

// dg_world_rollout with the torque formed in the loop: feed-forward + alpha x direction + time-varying state feedback, clamped
int32_t dg_world_rollout_feedback(dg_world* w, const float* state, int32_t body, int32_t frame, const float* local_pos, int32_t K, int32_t T, float dt,
                                  int32_t joint_damping, const float* q0, const float* qd0, const float* tau_ff, const float* dtau, const float* alpha,
                                  const float* gain, const float* q_ref, const float* qd_ref, const float* tau_limit,
                                  float* q_out, float* qd_out, float* tau_out, float* pos_out, int32_t* singular, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_rollout_feedback")) return rc;
  if (K < 1) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: K must be >= 1, got %d", K);
  if (T < 1) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: T must be >= 1, got %d", T);
  if (!std::isfinite(dt) || !(dt > 0.f)) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: dt must be finite and > 0, got %g", (double)dt);
  if (!tau_ff) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: tau_ff is NULL");
  if (dtau && !alpha) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: dtau needs alpha");
  if (gain && (!q_ref || !qd_ref)) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: gain needs q_ref and qd_ref");
  if (!q_out && !qd_out && !tau_out && !pos_out && !singular) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: every output is NULL");
  const int n = body_row(w, body)[DG_BI_N_LINKS];
  {  // B K T n floats of an output and B T n 2n of the gain stay addressable in bytes
    const int64_t lim = INT64_MAX / 4; int64_t v = w->num_envs;
    for (const int64_t f : {(int64_t)K, (int64_t)T, (int64_t)n}) { if (v > lim / f) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: %d envs x K %d x T %d x %d joints is beyond INT64_MAX / 4 values", w->num_envs, K, T, n); v *= f; }
    v = w->num_envs;
    for (const int64_t f : {(int64_t)T, (int64_t)n, (int64_t)2 * n}) { if (v > lim / f) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: gain of %d envs x T %d x %d x %d is beyond INT64_MAX / 4 values", w->num_envs, T, n, 2 * n); v *= f; }
  }
  int gf = -1; float lp[3] = {0.f, 0.f, 0.f};
  if (pos_out) {
    if (!local_pos) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: local_pos is NULL (three host floats)");
    if (frame < 0) return fail(DG_ERR_ARG, "dg_world_rollout_feedback: frame %d out of range (the base of a fixed body does not move)", frame);
    if (const int rc = frame_check(w, body, frame, &gf, "dg_world_rollout_feedback")) return rc;
    lp[0] = local_pos[0]; lp[1] = local_pos[1]; lp[2] = local_pos[2];
  }
  if (fdq_slots(n) > w->sc.tr_slots) return slots_refusal(w, body, fdq_slots(n), "dg_world_rollout_feedback");
  return launch_grid(w, dim3(rollout_grid(w, K)), stream, &LaunchTable::rollout_feedback, state, body, gf, lp[0], lp[1], lp[2], (int)K, (int)T, dt,
                     joint_damping != 0 ? 1 : 0, q0, qd0, tau_ff, dtau, alpha, gain, q_ref, qd_ref, tau_limit, q_out, qd_out, tau_out, pos_out, singular, w->d_gws);
}

// diagnostics: the workgroups dg_world_rollout would launch for K samples per env (tests: the cap of the global-workspace modes);
// not part of the public header
int32_t dg_debug_rollout_grid(const dg_world* w, int32_t K) {
  if (!w || K < 1) return fail(DG_ERR_ARG, "dg_debug_rollout_grid: bad argument");
  return (int32_t)rollout_grid(w, K);
}

// ------------------------------------------------------------------ forward-dynamics derivatives (dg_ddq.h)
int32_t dg_world_dynamics_derivatives(dg_world* w, const float* state, int32_t body, int32_t P, const float* q, const float* qd, const float* tau, int32_t joint_damping,
                                      float* qdd, float* dqdd_dq, float* dqdd_dqd, float* dqdd_dtau, float* dtau_dq, float* dtau_dqd, int32_t* singular, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_dynamics_derivatives")) return rc;
  if (P < 1) return fail(DG_ERR_ARG, "dg_world_dynamics_derivatives: P must be >= 1, got %d", P);
  if (!qdd && !dqdd_dq && !dqdd_dqd && !dqdd_dtau && !dtau_dq && !dtau_dqd && !singular) return fail(DG_ERR_ARG, "dg_world_dynamics_derivatives: every output is NULL");
  const int n = body_row(w, body)[DG_BI_N_LINKS];
  {  // B P n n floats stay addressable in bytes
    const int64_t lim = INT64_MAX / 4; int64_t v = w->num_envs;
    for (const int64_t f : {(int64_t)P, (int64_t)n, (int64_t)n}) { if (v > lim / f) return fail(DG_ERR_ARG, "dg_world_dynamics_derivatives: %d envs x P %d x %d x %d joints is beyond INT64_MAX / 4 values", w->num_envs, P, n, n); v *= f; }
  }
  if (n > DDQ_MAX_JOINTS) return fail(DG_ERR_ARG, "dg_world_dynamics_derivatives: body %d has %d joints, the derivatives take at most %d", body, n, DDQ_MAX_JOINTS);
  if (ddq_slots(n) > w->sc.tr_slots) return slots_refusal(w, body, ddq_slots(n), "dg_world_dynamics_derivatives");
  return launch_grid(w, dim3(rollout_grid(w, P)), stream, &LaunchTable::dynamics_derivatives, state, body, (int)P, q, qd, tau, joint_damping != 0 ? 1 : 0,
                     qdd, dqdd_dq, dqdd_dqd, dqdd_dtau, dtau_dq, dtau_dqd, singular, w->d_gws);
}

// ------------------------------------------------------------------ inertial parameters, inverse-dynamics regressor (dg_regq.h)
int32_t dg_world_inertial_parameters(dg_world* w, const float* state, int32_t body, int32_t nominal, float* theta, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_inertial_parameters")) return rc;
  if (!theta) return fail(DG_ERR_ARG, "dg_world_inertial_parameters: theta is NULL");
  if ((uintptr_t)theta & 7) return fail(DG_ERR_ARG, "dg_world_inertial_parameters: theta must be 8-byte aligned");
  return launch(w, stream, &LaunchTable::inertial_params, state, body, nominal != 0 ? 1 : 0, theta);
}

int32_t dg_world_id_regressor(dg_world* w, const float* state, int32_t body, int32_t P, const float* q, const float* qd, const float* qdd,
                              const float* qd_ref, const float* theta_hat, const float* s, float* Y, float* tau, float* grad, void* stream) {
  if (const int rc = dynq_check(w, state, body, -1, "dg_world_id_regressor")) return rc;
  if (P < 1) return fail(DG_ERR_ARG, "dg_world_id_regressor: P must be >= 1, got %d", P);
  if (!Y && !tau && !grad) return fail(DG_ERR_ARG, "dg_world_id_regressor: every output is NULL");
  if (tau && !theta_hat) return fail(DG_ERR_ARG, "dg_world_id_regressor: tau needs theta_hat");
  if (grad && !s) return fail(DG_ERR_ARG, "dg_world_id_regressor: grad needs s");
  if (((uintptr_t)Y | (uintptr_t)grad) & 7) return fail(DG_ERR_ARG, "dg_world_id_regressor: Y and grad must be 8-byte aligned");
  const int n = body_row(w, body)[DG_BI_N_LINKS];
  {  // B P n 10 n floats stay addressable in bytes
    const int64_t lim = INT64_MAX / 4; int64_t v = w->num_envs;
    for (const int64_t f : {(int64_t)P, (int64_t)n, (int64_t)10 * n}) { if (v > lim / f) return fail(DG_ERR_ARG, "dg_world_id_regressor: %d envs x P %d x %d x %d is beyond INT64_MAX / 4 values", w->num_envs, P, n, 10 * n); v *= f; }
  }
  if (regq_slots(n) > w->sc.tr_slots) return slots_refusal(w, body, regq_slots(n), "dg_world_id_regressor");
  return launch_grid(w, dim3(rollout_grid(w, P)), stream, &LaunchTable::id_regressor, state, body, (int)P, q, qd, qdd, qd_ref, theta_hat, s, Y, tau, grad, w->d_gws);
}

// ------------------------------------------------------------------ Riccati / iLQR backward pass (dg_lqr.h)
int32_t dg_world_lq_backward(dg_world* w, int32_t body, int32_t T, int32_t P, int32_t PC, int32_t substeps, double dt,
                             const float* A_q, const float* A_v, const float* Minv, const float* lxx, const float* luu, const float* lx, const float* lu,
                             const float* lxx_T, const float* lx_T, const float* mu, float* K_out, float* k_out, float* dV, int32_t* status, void* stream) {
  if (!w) return fail(DG_ERR_ARG, "dg_world_lq_backward: null argument");
  if (const int rc = body_check(w, body, "dg_world_lq_backward")) return rc;
  const int n = body_row(w, body)[DG_BI_N_LINKS];
  if (n < 1) return fail(DG_ERR_ARG, "dg_world_lq_backward: body %d has no joints", body);
  if (n > LQ_MAX_JOINTS) return fail(DG_ERR_ARG, "dg_world_lq_backward: body %d has %d joints, the backward pass takes at most %d", body, n, LQ_MAX_JOINTS);
  if (T < 1) return fail(DG_ERR_ARG, "dg_world_lq_backward: T must be >= 1, got %d", T);
  if (P != 1 && P != T) return fail(DG_ERR_ARG, "dg_world_lq_backward: P must be 1 or T = %d, got %d", T, P);
  if (PC != 1 && PC != T) return fail(DG_ERR_ARG, "dg_world_lq_backward: the cost's P must be 1 or T = %d, got %d", T, PC);
  if (substeps < 1) return fail(DG_ERR_ARG, "dg_world_lq_backward: substeps must be >= 1, got %d", substeps);
  if (!std::isfinite(dt) || !(dt > 0.0)) return fail(DG_ERR_ARG, "dg_world_lq_backward: dt must be finite and > 0, got %g", dt);
  if (!A_q || !A_v || !Minv) return fail(DG_ERR_ARG, "dg_world_lq_backward: A_q, A_v and Minv are required");
  if (!lxx || !luu || !lxx_T) return fail(DG_ERR_ARG, "dg_world_lq_backward: lxx, luu and lxx_T are required");
  if (!status) return fail(DG_ERR_ARG, "dg_world_lq_backward: status is NULL");
  {  // B T m m floats stay addressable in bytes
    const int64_t lim = INT64_MAX / 4; int64_t v = w->num_envs;
    for (const int64_t f : {(int64_t)T, (int64_t)2 * n, (int64_t)2 * n}) { if (v > lim / f) return fail(DG_ERR_ARG, "dg_world_lq_backward: %d envs x T %d x %d x %d is beyond INT64_MAX / 4 values", w->num_envs, T, 2 * n, 2 * n); v *= f; }
  }
  DG_ON_DEVICE(w->device);
  const LqArgs a = {n, (int)T, (int)P, (int)PC, (int)substeps, dt, A_q, A_v, Minv, lxx, luu, lx, lu, lxx_T, lx_T, mu, K_out, k_out, dV, status};
  hipLaunchKernelGGL(lq_backward_kernel, dim3((unsigned)w->num_envs), dim3(64), sizeof(double) * (size_t)lq_lds_doubles(n), (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}

// ------------------------------------------------------------------ closest-points query (dg_closestq.h)
// floats of the pose table and of the polytope workspace behind it (one block per wavefront of the query's own grid)
static size_t closest_table_floats(const dg_world* w) { return (size_t)w->num_envs * (size_t)w->sc.nsh * RS_STRIDE; }
static size_t closest_hull_ws_floats(const dg_world* w) { return (size_t)((w->num_envs + 63) / 64) * (size_t)HH_WS_SLOTS * 64; }

int64_t dg_world_closest_scratch_floats(const dg_world* w) {
  if (!w) { (void)fail(DG_ERR_ARG, "null world"); return 0; }
  return (int64_t)(closest_table_floats(w) + closest_hull_ws_floats(w));
}

int32_t dg_world_closest(dg_world* w, const float* state, int32_t body_a, int32_t link_a, int32_t body_b, int32_t link_b, float distance, int32_t max_points,
                         float* scratch, int32_t* count, int32_t* ids, float* geom, int32_t* nearest_ids, float* nearest_geom, void* stream) {
  if (!w || !state) return fail(DG_ERR_ARG, "dg_world_closest: null argument");
  if (!count) return fail(DG_ERR_ARG, "dg_world_closest: count is NULL (ids, geom, nearest_ids and nearest_geom may be)");
  if (!scratch) return fail(DG_ERR_ARG, "dg_world_closest: scratch is NULL (dg_world_closest_scratch_floats floats of device memory)");
  if (body_a == DG_CONTACT_ANY) return fail(DG_ERR_ARG, "dg_world_closest: body_a is required (body_b, link_a and link_b may be DG_CONTACT_ANY)");
  if (const int rc = contact_filter_check(w, body_a, link_a, "a", "dg_world_closest")) return rc;
  if (const int rc = contact_filter_check(w, body_b, link_b, "b", "dg_world_closest")) return rc;
  if (!std::isfinite(distance) || distance < 0.f) return fail(DG_ERR_ARG, "dg_world_closest: distance must be finite and >= 0, got %g", (double)distance);
  if (max_points < 0) return fail(DG_ERR_ARG, "dg_world_closest: max_points must be >= 0, got %d", max_points);
  if (max_points > 0 && !ids && !geom) return fail(DG_ERR_ARG, "dg_world_closest: max_points %d with ids and geom both NULL", max_points);
  DG_ON_DEVICE(w->device);
  // the shape poses in the world's own workspace mode, then one wavefront per 64 envs: the grid the polytope workspace is sized for
  if (const int rc = launch_pose(w, stream, state, 0, scratch, 0, -1, -1)) return rc;
  l_closest(dim3((unsigned)((w->num_envs + 63) / 64)), (hipStream_t)stream, w->sc, scratch, body_a, link_a, body_b, link_b, distance, max_points, w->closest_no_cull,
            scratch + closest_table_floats(w), count, ids, geom, nearest_ids, nearest_geom);
  HIP_TRY(hipGetLastError());
  return DG_OK;
}

// diagnostics: dg_world_closest without its culls (what the culled call must equal bit for bit); not part of the public header
int32_t dg_debug_closest_no_cull(dg_world* w, int32_t on) {
  if (!w) return fail(DG_ERR_ARG, "null world");
  w->closest_no_cull = on != 0;
  return DG_OK;
}

}  // extern "C"
