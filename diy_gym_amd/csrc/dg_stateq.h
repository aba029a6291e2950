// dg_stateq.h -- batched link states and base reset: the state reads and the state write that close the contract env.sim gives
// user addons written in Python (pybullet's p.getLinkStates / p.getLinkState(computeLinkVelocity=1) / p.getBasePositionAndOrientation
// / p.getBaseVelocity and p.resetBasePositionAndOrientation / p.resetBaseVelocity; reference call sites:
// diy_gym/addons/sensors/object_state_sensor.py:35-42, rewards/reach_target.py:22-28, sensors/camera.py:60-63, misc/respawn.py:35,
// model.py:68-74).  One env per lane in the world's own workspace mode, one launch per call, nothing allocated.
//
//   link_states_kernel  n <= DG_LINK_STATES_MAX (body, frame) selectors, by value in the kernel's arguments.  Row k of an env is what
//                       frame_kernel (dg_entry.h) writes for (body[k], frame[k], com): the same Lane::frame_state with want_vel after
//                       the same ln.kinematics, so the same bits -- but the kinematics of a body run once per DISTINCT body among
//                       the selectors (each body's poses have slots of their own in the POSE region: the step computes them all
//                       side by side), and there is one launch and one output buffer for the n rows.  The state is read, never
//                       written.  The selector tables are wave-uniform (scalar) loads; the duplicate scan is scalar too.
//   reset_base_kernel   pose and / or velocity of a body's base, in the envs the mask selects.  The pose is that of the base's
//                       INERTIAL (report) frame and goes through set_base_com_pose (dg_solver.h) -- the function the compiled
//                       DG_OP_RESPAWN calls, so an equal pose is stored as the same bits -- after the orientation has been
//                       normalised.  Velocities are those of the same report (columns 7:13 of frame_state with com = 1): the world
//                       velocity v_c of that frame's origin and the world angular velocity w.  The state stores the velocity of
//                       the base LINK's origin, v_l = v_c - w x r with r = R_base x report offset (frame_state adds that term back).
//                       With a pose a velocity that is not given is zero (set_base_com_pose, pybullet); without a pose the one that
//                       is not given keeps its REPORTED value -- a new w alone re-bases v_l so that v_c stays.  The env's contact
//                       impulse cache is emptied as joint_reset_kernel (dg_ikq.h) does.  Joint state, targets, external wrenches,
//                       addon state and the counters are not touched.  The host refuses a body whose base the planner pinned to
//                       its load pose, and a velocity for a fixed base.
// The out rows are env-major, 13 n floats apart per lane: each of the 13 n stores of a wavefront touches 64 different rows.  No LDS
// staging pass: tools/gpu_link_states_time.py has the figures (DESIGN.md "Link states and base reset").
#pragma once
#include "dg_solver.h"
#include "dg_launch.h"  // LsSelectors, which the host side shares

namespace dg {

// out [num_envs][sel.n][13]: pos3 quat4 linvel3 angvel3
template <int LANES>
__global__ __launch_bounds__(64) void link_states_kernel(DevScene sc, MotorTable mt, float* state, LsSelectors sel, int com, float* out, float* gws) {
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  const int env = blockIdx.x * ACTIVE + lane; if (env >= sc.num_envs) return;
  Lane<LANES> ln(sc, mt, workspace_of<LANES>(sc, smem, gws, lane), state + env, env, false);  // never stores state
  for (int k = 0; k < sel.n; k++) {  // the poses of every distinct body, once
    const int b = sel.body[k]; bool seen = false;
    for (int j = 0; j < k; j++) seen = seen || sel.body[j] == b;
    if (!seen) ln.kinematics(b);
  }
  float* row = out + (size_t)env * (size_t)sel.n * 13;
  for (int k = 0; k < sel.n; k++) {
    V3 p, v, w; Q4 q; ln.frame_state(sel.body[k], sel.frame[k], com != 0, p, q, v, w, true);
    float* o = row + k * 13;
    o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = q.x; o[4] = q.y; o[5] = q.z; o[6] = q.w; o[7] = v.x; o[8] = v.y; o[9] = v.z; o[10] = w.x; o[11] = w.y; o[12] = w.z;
  }
}

// pos [num_envs][3] and orn [num_envs][4] (xyzw; both or neither), lin_vel, ang_vel [num_envs][3] (each may be null), env_mask
// [num_envs] or null = every env
template <int LANES>
__global__ __launch_bounds__(64) void reset_base_kernel(DevScene sc, MotorTable mt, float* state, int body, const float* pos, const float* orn,
                                                         const float* lin_vel, const float* ang_vel, const uint8_t* env_mask, float* gws) {
  extern __shared__ float smem[];
  constexpr int ACTIVE = envs_per_wave(LANES);
  const int lane = threadIdx.x; if (lane >= ACTIVE) return;
  const int env = blockIdx.x * ACTIVE + lane; if (env >= sc.num_envs) return;
  if (env_mask && !env_mask[env]) return;
  Lane<LANES> ln(sc, mt, workspace_of<LANES>(sc, smem, gws, lane), state + env, env, true);
  auto row3 = [&](const float* p) { return v3(p[3 * (size_t)env], p[3 * (size_t)env + 1], p[3 * (size_t)env + 2]); };
  const int so = ln.bi(body)[DG_BI_STATE_OFF];
  V3 vl = v3(0.f, 0.f, 0.f), wl = vl;  // what the state holds once the pose is in: zero behind set_base_com_pose
  if (pos) {
    const float* o = orn + 4 * (size_t)env; const Q4 qc = {o[0], o[1], o[2], o[3]};
    set_base_com_pose(ln, body, row3(pos), qnormalize(qc));
  } else if (!ln.fixed(body)) {
    vl = v3(ln.S(so + DG_BS_LINVEL), ln.S(so + DG_BS_LINVEL + 1), ln.S(so + DG_BS_LINVEL + 2));
    wl = v3(ln.S(so + DG_BS_ANGVEL), ln.S(so + DG_BS_ANGVEL + 1), ln.S(so + DG_BS_ANGVEL + 2));
  }
  if ((lin_vel || ang_vel) && !ln.fixed(body)) {
    cfp f = ln.bf(body);
    const V3 r = mul(qmat(ln.base_quat(body)), v3(f[DG_BF_REPORT_POS], f[DG_BF_REPORT_POS + 1], f[DG_BF_REPORT_POS + 2]));  // (the pose just stored)
    const V3 vc = lin_vel ? row3(lin_vel) : vl + cross(wl, r), w = ang_vel ? row3(ang_vel) : wl;
    const V3 v = vc - cross(w, r);
    ln.Sset(so + DG_BS_LINVEL, v.x); ln.Sset(so + DG_BS_LINVEL + 1, v.y); ln.Sset(so + DG_BS_LINVEL + 2, v.z);
    ln.Sset(so + DG_BS_ANGVEL, w.x); ln.Sset(so + DG_BS_ANGVEL + 1, w.y); ln.Sset(so + DG_BS_ANGVEL + 2, w.z);
  }
  if (sc.warm_off >= 0) ln.Sset(sc.warm_off, 0.f);  // cached impulses of a teleported body mean nothing
}

}  // namespace dg
