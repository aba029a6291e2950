// dg_plan.h -- everything dg_world_create decides about a world before it touches the device: the LDS plan, the workspace
// mode, the kernel form and the device-only tables.  plan_world is a pure function of the scene blob, the batch, the GPU's CU
// count and the ablation switches (no HIP call, no environment, no global state), so tests/test_world_plan.py pins its
// decisions on a machine without a GPU (through dg_debug_plan).  Host only: included by dg_api.hip and dg_plan.hip, never by
// the kernels' translation units.
#pragma once
#include <string>
#include <vector>

#include "dg_kernels.h"

namespace dg {

// The one table of environment switches: X(environment variable, PlanSwitches field, meaning).  README.md "Environment
// switches" lists the same names (tests/test_world_plan.py compares the two).
#define DG_PLAN_SWITCHES(X) \
  X(DG_MAX_LANES, max_lanes, "32|16|8|4|1: envs per wavefront to start from; any value also switches the automatic narrowing off") \
  X(DG_NO_NARROW_MODES, no_narrow_modes, "never below 16 envs per wavefront") \
  X(DG_NO_WAVE_ENV, no_wave_env, "never one env per wavefront") \
  X(DG_NO_SLICED_GLOBAL, no_sliced_global, "global workspace with 64 envs per wavefront instead of 16") \
  X(DG_NO_HELPER_WAVE, no_helper_wave, "single-wavefront step kernel") \
  X(DG_NO_COLLIDE_WAVE, no_collide_wave, "the main wavefront runs the narrow phase itself") \
  X(DG_NO_COLLIDE_SPLIT, no_collide_split, "one narrow-phase wavefront instead of two") \
  X(DG_NO_EARLY_DYNAMICS, no_early_dynamics, "the first substep's dynamics wait for the update ops") \
  X(DG_NO_SPLIT_SWEEPS, no_split_sweeps, "the main wavefront sweeps both arms") \
  X(DG_NO_SPLIT_CONTACTS, no_split_contacts, "contact rows stay on the main wavefront when the sweeps are split") \
  X(DG_NO_REG_ROWS, no_reg_rows, "sliced sweeps keep their rows in LDS") \
  X(DG_NO_FULL_IK, no_full_ik, "the general register-resident IK instead of the packed six-axis solve") \
  X(DG_NO_MINV_SLICES, no_minv_slices, "M^-1 columns by one lane per env") \
  X(DG_NO_CHAIN_ROWS, no_chain_rows, "contact rows between two register-chain bodies pair by pair") \
  X(DG_NO_SLICED_RESET, no_sliced_reset, "masked resets through the one-lane-per-env reset kernel") \
  X(DG_NO_PAR_RESET, no_par_reset, "masked resets of four-wavefront scenes through the one-wavefront reset kernel") \
  X(DG_DEBUG_KEEP_EXT, debug_keep_ext, "external wrenches and joint torques are not cleared at the end of a step") \
  X(DG_RENDER_NO_CULL, render_no_cull, "render: every shape tested for every pixel group (render diag bit 0)") \
  X(DG_RENDER_DIAG, render_diag, "render: initial value of the dg_world_set_render_diag flags") \
  X(DG_RENDER_WPE, render_wpe, "render: 1|3 wavefronts per SIMD builds of the render kernel instead of 2")

struct Switch {
  bool set = false;  // the variable exists, whatever it holds
  int value = 0;     // atoi of what it holds
  explicit operator bool() const { return set; }
};
struct PlanSwitches {
#define X(name, field, doc) Switch field;
  DG_PLAN_SWITCHES(X)
#undef X
  // DG_NO_NP_SKIP: every substep runs its narrow phase and the pose pass in front of it.  Read like the switches above but kept
  // beside the table: tests/test_world_plan.py pins the table at its twenty entries, and README.md's list with it.
  Switch no_np_skip;
};
PlanSwitches plan_switches_from_env();  // read afresh on every call

struct WorldPlan {
  int lanes = 64, lds_bytes = 0;
  bool par = false;           // step runs as four wavefronts per workgroup (helper wave)
  bool mf = false;            // hull_manifold_points > 1 in a world that collides two hulls: the kernels with the manifold (dg_mf)
  bool no_par_reset = false;  // masked resets through reset_kernel<64> (one wavefront, generic solver)
  int render_diag = 0, render_wpe = 2;
  size_t gws_floats = 0;      // global workspace [workgroup][slot][lane] (lanes <= 0), 0: not allocated
  size_t hull_ws_floats = 0;  // polytope workspace of the hull-hull narrow phase, one block per wavefront of the step grid, 0: not allocated
  std::vector<int32_t> table;             // PLB | PLL | PD | GD | SD | AM | RH
  size_t pd_off = 0, gd_off = 0, sd_off = 0, am_off = 0, rh_off = 0;
  std::vector<int32_t> blob_i;            // device copy of the int blob, with the IK hints in the op flags
  std::vector<float> blob_f;              // the float blob converted once
  MotorTable mt;                          // default velocity motors on every joint
  std::vector<float> init;                // load-time state vector
  DevScene sc;                            // every non-pointer field; the pointers are the caller's, from its three allocations
  std::string error;                      // message of a non-zero return
};

// DG_OK, or the DG_ERR_* / message dg_world_create reports for a blob it cannot run.
int plan_world(const int32_t* I, int64_t n_i, const double* F, int64_t n_f, int num_envs, int env_stride, int cu_count, uint64_t seed,
               int64_t env_index_base, const PlanSwitches& sw, WorldPlan& out);

}  // namespace dg
