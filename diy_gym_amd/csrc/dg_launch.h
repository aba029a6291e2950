// dg_launch.h -- host-side launch table: one table of launchers per envs-per-wavefront mode, each defined in its own
// translation unit (dg_inst.hip compiled with -DDG_LANES=... -DDG_PART=...), so the library builds in parallel.
// DG_QUERY_KERNELS below is the one list of the one-wavefront kernels: table, launchers and LDS attributes are made from it.
#pragma once
#include "dg_kernels.h"

namespace dg {

// the link selectors of net_contact_wrench_kernel (dg_contactf.h), by value in the kernel arguments: the pybullet link index the
// ids are compared with (DG_CONTACT_ANY: the whole body) and the global frame whose inertial origin the moment is taken about
// (-1: the base)
struct CfSelectors { int32_t n; int32_t link[DG_CONTACT_MAX_LINKS]; int32_t frame[DG_CONTACT_MAX_LINKS]; };
// the (body, frame) selectors of link_states_kernel (dg_stateq.h), by value in the kernel arguments: the body index and the global
// frame index (-1: the base)
struct LsSelectors { int32_t n; int32_t body[DG_LINK_STATES_MAX]; int32_t frame[DG_LINK_STATES_MAX]; };
// the joint selectors of joint_wrench_kernel (dg_jointq.h), by value in the kernel arguments: dg_joint_selector of the public header
// with `frame` already the GLOBAL frame index
struct JwSelectors { int32_t n; int32_t pad_; dg_joint_selector s[DG_JOINT_WRENCH_MAX]; };
// the sensor-frame selectors of link_accel_kernel (dg_accelq.h), by value in the kernel arguments: dg_accel_selector of the public
// header with `frame` already the GLOBAL frame index (-1: the base) and `quat` normalised; ghat is the scene's gravity direction
// g / |g| (zeros when g = 0)
struct LaSelectors { int32_t n; float ghat[3]; dg_accel_selector s[DG_LINK_ACCEL_MAX]; };

#define DG_STEP_PARAMS DevScene sc, MotorTable mt, float* state, const float* actions, uint64_t mask, float* obs, float* rew, uint8_t* term, \
                       float* rew_sum, uint8_t* term_flag, int32_t* diag, unsigned long long* cycles
// The one-wavefront kernels, one line each: X(name, the parameters of name_kernel<LANES> after `DevScene sc, MotorTable mt, float* state`).
// The list makes the members of LaunchTable, their launchers, the LDS attribute of each kernel and the slots of each mode's table
// (dg_inst.hip); a *Selectors struct goes by reference into the launcher and by value into the kernel.
#define DG_QUERY_KERNELS(X) \
  X(reset, const uint8_t* mask, float* obs, float* gws) \
  X(observe, float* obs, float* rew, uint8_t* term, float* rew_sum, uint8_t* term_flag, float* gws) \
  X(frame, int body, int frame, int com, float* out, float* gws) \
  X(wrench, int body, int frame, int link_frame, const float* force, const float* pos, const float* torque, float* gws) \
  X(pose, int ncam, cip CI, cfp CF, float* table, float* gws, int nmount, int mbody, int mframe) \
  /* dynamics queries (dg_dynq.h) */ \
  X(joint_state, int body, float* q_out, float* qd_out, float* gws) \
  X(joint_torque, int body, const float* tau, float* gws) \
  X(jacobian, int body, int frame, float lx, float ly, float lz, const float* q, float* jac_t, float* jac_r, float* gws) \
  X(inverse_dynamics, int body, const float* q, const float* qd, const float* qdd, float* tau, float* gws) \
  X(mass_matrix, int body, const float* q, float* M, float* gws) \
  /* inverse-kinematics query, motor targets, joint reset (dg_ikq.h) */ \
  X(ik_query, int body, int frame, const float* target_pos, const float* target_orn, const float* lists, const float* q0, float* q_out, int32_t* iters_out, float* gws) \
  X(joint_targets, int body, uint64_t joint_mask, const float* pos, const float* vel, float* gws) \
  X(joint_reset, int body, uint64_t joint_mask, const float* q, const float* qd, const uint8_t* env_mask, float* gws) \
  /* contact query (dg_contactq.h), contact forces (dg_contactf.h) */ \
  X(contact_query, int body_a, int link_a, int body_b, int link_b, int32_t* count, int32_t* ids, float* geom, float* force, float* gws) \
  X(contact_force, int body_a, int link_a, int body_b, int link_b, int32_t* count, int32_t* ids, float* out, float* gws) \
  X(net_contact_wrench, int body, const CfSelectors& sel, int body_b, int link_b, float* wrench, int32_t* ncontacts, float* gws) \
  /* link states, base reset (dg_stateq.h) */ \
  X(link_states, const LsSelectors& sel, int com, float* out, float* gws) \
  X(reset_base, int body, const float* pos, const float* orn, const float* lin_vel, const float* ang_vel, const uint8_t* env_mask, float* gws) \
  /* joint reaction wrenches, applied motor torques (dg_jointq.h) */ \
  X(joint_wrench, int body, const JwSelectors& sel, float* wrench, float* gws) \
  X(joint_effort, int body, float* out, float* gws) \
  /* link accelerations, IMU readings (dg_accelq.h) */ \
  X(link_accel, int body, const LaSelectors& sel, float* out, float* gws) \
  /* task-space dynamics (dg_taskq.h) */ \
  X(task_space, int body, int frame, float lx, float ly, float lz, int axes_mask, const float* q, const float* qd, const float* acc, const float* tau_null, \
    float damping, float* jac, float* bias_acc, float* bias_torque, float* lambda, float* tau, float* point, int32_t* singular, float* gws) \
  /* forward dynamics, joint-space rollouts (dg_fdq.h) */ \
  X(forward_dynamics, int body, const float* q, const float* qd, const float* tau, int damp, float* qdd, int32_t* singular, float* gws) \
  X(rollout, int body, int frame, float lx, float ly, float lz, int K, int T, float dt, int damp, const float* q0, const float* qd0, const float* tau, \
    float* q_out, float* qd_out, float* pos_out, int32_t* singular, float* gws) \
  X(rollout_feedback, int body, int frame, float lx, float ly, float lz, int K, int T, float dt, int damp, const float* q0, const float* qd0, const float* tau_ff, \
    const float* dtau, const float* alpha, const float* gain, const float* q_ref, const float* qd_ref, const float* tau_limit, \
    float* q_out, float* qd_out, float* tau_out, float* pos_out, int32_t* singular, float* gws) \
  /* forward-dynamics derivatives (dg_ddq.h) */ \
  X(dynamics_derivatives, int body, int P, const float* q, const float* qd, const float* tau, int damp, float* qdd, float* dqdd_dq, float* dqdd_dqd, float* dqdd_dtau, \
    float* dtau_dq, float* dtau_dqd, int32_t* singular, float* gws) \
  /* inertial parameters, inverse-dynamics regressor (dg_regq.h) */ \
  X(inertial_params, int body, int nominal, float* theta, float* gws) \
  X(id_regressor, int body, int P, const float* q, const float* qd, const float* qdd, const float* qd_ref, const float* theta_hat, const float* s, \
    float* Y, float* tau, float* grad, float* gws)

struct LaunchTable {
  bool has_prof;
  hipError_t (*prepare)(int lds_bytes);
  void (*step)(dim3 grid, int lds, hipStream_t st, bool prof, DG_STEP_PARAMS, float* gws);
  void (*step_par)(dim3 grid, int lds, hipStream_t st, bool prof, DG_STEP_PARAMS, const uint8_t* reset_mask, int reset_mode);  // reset_mode 1: masked reset + one hot-start step (mask NULL = every env)
#define DG_MEMBER(name, ...) void (*name)(dim3 grid, int lds, hipStream_t st, DevScene sc, MotorTable mt, float* state, __VA_ARGS__);
  DG_QUERY_KERNELS(DG_MEMBER)
#undef DG_MEMBER
};
// closest-points query (dg_closestq.h): one kernel for every mode -- it uses no workspace -- defined in the 64-lane query unit
void l_closest(dim3 grid, hipStream_t st, DevScene sc, const float* table, int body_a, int link_a, int body_b, int link_b, float distance, int max_points, int no_cull,
               float* hull_ws, int32_t* count, int32_t* ids, float* geom, int32_t* nearest_ids, float* nearest_geom);
const LaunchTable& launch_table(int lanes, bool mf);  // lanes in {64, 32, 16, 8, 4, 1, 0, -16}; mf: the kernels with the hull-hull manifold

}  // namespace dg
