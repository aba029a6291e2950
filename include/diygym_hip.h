/* diygym_hip.h -- C-ABI of the MI355X batched simulation backend.
 *
 * This is the boundary that replaces the `pybullet` module API on DIYGym's
 * step path.  The reference is Python and binds pybullet through its CPython
 * extension; the calls it makes are enumerated in SURVEY.md 8(b).  Each entry
 * point below names the reference call sites it replaces.  All buffer
 * arguments are DEVICE pointers owned by the caller (torch tensors'
 * data_ptr()); `stream` is a hipStream_t (NULL = default stream).  No entry
 * point allocates, frees or synchronises after dg_world_create, so every call
 * can be captured into a hipGraph.  Return value: 0 on success, a negative
 * DG_ERR_* otherwise, with dg_last_error() giving the message.  One world per
 * GPU, one host thread per world (same rule as a pybullet client).
 *
 * Batched buffers:
 *   state    float [state_dim][env_stride]  struct-of-arrays over envs (coalesced)
 *   actions  float [num_envs][act_dim]      row per env, columns in the order of
 *                                           flatten(action_space) (reference utils.py:46-60)
 *   obs      float [num_envs][obs_dim]      ... of flatten(observe())
 *   rew      float [num_envs][rew_dim]      one column per reward addon
 *   term     uint8 [num_envs][term_dim]     one column per terminal addon
 *   rew_sum  float [num_envs]               collapsed reward  (sum_rewards, diy_gym.py:94,168)
 *   term_flag uint8 [num_envs]              collapsed terminal (terminal_if_any/all, diy_gym.py:95-96,185)
 */
#ifndef DIYGYM_HIP_H
#define DIYGYM_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DG_OK 0
#define DG_ERR_BAD_SCENE (-1)
#define DG_ERR_HIP (-2)
#define DG_ERR_UNSUPPORTED (-3)
#define DG_ERR_ARG (-4)

typedef struct dg_world dg_world;

/* library identification: (major << 16) | minor */
int32_t dg_version(void);
const char* dg_last_error(void);

/* Replaces p.connect / p.resetSimulation / p.setPhysicsEngineParameter /
 * p.setGravity / p.loadURDF / p.changeDynamics (reference diy_gym.py:68-82,
 * model.py:65-83): builds the device-side constant tables for `num_envs`
 * copies of the scene blob (include/diygym_scene.h) on HIP device `device`.
 * `env_stride` (>= num_envs, multiple of 64) is the row pitch of `state`.
 * `seed` and `env_index_base` key the per-env respawn RNG streams. */
int32_t dg_world_create(const int32_t* idata, int64_t n_i, const double* fdata, int64_t n_f, int32_t num_envs,
                        int32_t env_stride, int32_t device, uint64_t seed, int64_t env_index_base, dg_world** out);

/* Replaces p.disconnect (reference diy_gym.py:225). */
void dg_world_destroy(dg_world* w);

/* dims[0..7] = state_dim, act_dim, obs_dim, rew_dim, term_dim, n_links,
 * lds_bytes_per_workgroup, workspace mode.  Mode: 64 / 32 / 16 / 8 / 4 = that many envs per wavefront with the per-env
 * scratch in LDS; 0 = 64 envs per wavefront, scratch in a device buffer the world owns; -16 = 16 envs per
 * wavefront, scratch in that buffer (chosen by dg_world_create from the scene's scratch footprint). */
int32_t dg_world_dims(const dg_world* w, int32_t dims[8]);

/* Name of the step kernel dg_world_step launches for this world (for benchmark / profile labels):
 * "step_kernel<lanes>" or "step_kernel_par (...)".  The pointer is valid until the calling thread's next call. */
const char* dg_world_kernel_name(const dg_world* w);

/* Host-side view of the motor table (p.setJointMotorControlArray gains/forces,
 * uniform over envs): cfg[n_links][3] = kp, kd, max_force (<0: raw impulse). */
int32_t dg_world_get_motor_cfg(const dg_world* w, double* cfg);
int32_t dg_world_set_motor_cfg(dg_world* w, const double* cfg);

/* Writes the load-time state (model poses from the config, joints at zero)
 * into `state` for every env.  Replaces the p.resetBasePositionAndOrientation
 * done while models are constructed (reference model.py:68). */
int32_t dg_world_init_state(dg_world* w, float* state, void* stream);

/* Replaces DIYGym.reset()'s addon.reset() + hot_start x p.stepSimulation +
 * observe (reference diy_gym.py:130-148; respawn.py:31-35,
 * joint_controller.py:36-38) for the envs whose `mask` byte is non-zero
 * (mask == NULL: all envs).  obs (nullable) is written for the envs that were reset -- with mask == NULL that is every
 * env; with a mask, the rows of the other envs are left as the last step / reset / observe wrote them (in units of
 * one wavefront: rows sharing a wavefront with a reset env are recomputed, to the same values). */
int32_t dg_world_reset(dg_world* w, float* state, const uint8_t* mask, float* obs, void* stream);

/* Replaces one DIYGym.step(): addon.update() for the controller addons whose
 * bit is set in `update_mask` (p.setJointMotorControlArray,
 * p.calculateInverseKinematics, p.applyExternalForce/Torque), step_counter += 1,
 * p.stepSimulation, then observe / reward / is_terminal (p.getJointStates,
 * p.getLinkState, p.getBasePositionAndOrientation, p.getBaseVelocity)
 * (reference diy_gym.py:187-209).  Any output pointer may be NULL. */
int32_t dg_world_step(dg_world* w, float* state, const float* actions, uint64_t update_mask, float* obs, float* rew,
                      uint8_t* term, float* rew_sum, uint8_t* term_flag, void* stream);

/* Outputs for the current state without stepping (reference diy_gym.py:150-185). */
int32_t dg_world_observe(dg_world* w, const float* state, float* obs, float* rew, uint8_t* term, float* rew_sum,
                         uint8_t* term_flag, void* stream);

/* Debug getter replacing p.getLinkState / p.getBasePositionAndOrientation /
 * p.getBaseVelocity: out[num_envs][13] = pos3 quat4 linvel3 angvel3 of `frame`
 * (pybullet joint index, -1 = base) of body `body`; com != 0 selects the
 * inertial frame (items 0,1,6,7), else the URDF link frame (items 4,5). */
int32_t dg_world_frame_state(dg_world* w, const float* state, int32_t body, int32_t frame, int32_t com, float* out,
                             void* stream);

/* Replaces p.applyExternalForce(uid, linkIndex, force, pos, flags) + p.applyExternalTorque(uid, linkIndex, torque, flags)
 * for addons that are NOT compiled into the step kernel -- a user's Python addon acting on the world from its update()
 * hook (reference examples/drone_pilot/drone_pilot.py:34-37, diy_gym/addons/addon.py:80-81 registry, :91-186 hooks;
 * diy_gym/addons/controllers/external_force.py:24) -- every env at once: force, pos, torque are device arrays
 * [num_envs][3] (any may be NULL = zero).  `frame` is the pybullet joint index of the link (-1 = base).  flags as in
 * pybullet: DG_WRENCH_LINK_FRAME -- force / torque along the axes of the link's INERTIAL frame (URDF <inertial> origin:
 * centre of mass and its rpy), pos relative to that origin -- the frame pybullet resolves LINK_FRAME against [R], NOT the
 * joint frame; for a link without an <inertial><origin> the two coincide;
 * DG_WRENCH_WORLD_FRAME -- all three in world coordinates.  The wrench acts during the NEXT dg_world_step only
 * (pybullet clears external forces after every stepSimulation) and adds to what compiled ops apply.  For a frame on a
 * movable link the joints between it and the base receive J^T of the wrench.  The compiled external_force / propellor
 * ops run the same device function, so a Python addon built on this entry reproduces them bit for bit. */
enum { DG_WRENCH_LINK_FRAME = 1, DG_WRENCH_WORLD_FRAME = 2 };
int32_t dg_world_apply_wrench(dg_world* w, float* state, int32_t body, int32_t frame, int32_t flags, const float* force,
                              const float* pos, const float* torque, void* stream);

/* Replaces Camera.observe -> p.computeProjectionMatrixFOV / p.getCameraImage (reference
 * diy_gym/addons/sensors/camera.py:44,58-92) for camera `camera` of the scene, all envs:
 *   rgb   float [num_envs][h*w*3]  flat shaded body colour (NOT a parity output: pybullet renders visual meshes)
 *   depth float [num_envs][h*w]    eye-space z exactly as camera.py:82-85 computes it (negative; -far = nothing hit)
 *   seg   int32 [num_envs][h*w]    uid + ((link + 1) << 24), -1 = background
 * flat pixel index = row * width + col, row 0 at the top; any pointer may be NULL. */
int32_t dg_world_render(dg_world* w, const float* state, int32_t camera, float* rgb, float* depth, int32_t* seg, void* stream);

/* Diagnostic switches of dg_world_render (bit 0: test every shape for every pixel group -- the brute-force picture the
 * culled one must equal bit for bit; 2: no intersections, background only; 4: hulls skipped; 128: no strip / tile level culling;
 * 512: one band per picture whatever the batch size; 16: stage counters of a -DDG_RENDER_COUNTERS build, tools/gpu_cam_bench.py).
 * The environment variables DG_RENDER_NO_CULL / DG_RENDER_DIAG give the initial value, read once at dg_world_create. */
int32_t dg_world_set_render_diag(dg_world* w, int32_t flags);

/* Replaces p.rayTest / p.rayTestBatch (pybullet's batched world query; the reference itself never calls either -- no
 * addon of its own casts rays -- so there is no call site to name: this is the query a pybullet user expects, and what
 * the `lidar` addon is built on).  `n_rays` segments from `ray_from` to `ray_to` against the collision geometry of every
 * env, one launch for all envs:
 *   - the nearest ENTRY point with 0 <= frac < 1 wins;
 *   - a ray that starts inside a convex shape does not hit that shape (only entries are reported);
 *   - a zero-length ray hits nothing;
 *   - ties between coincident surfaces go to the lower shape index (as in dg_world_render).
 * dg_world_raycast_scratch_floats: floats of caller-owned device scratch dg_world_raycast needs for this world (the
 * per-env shape pose table + the mounting frame's pose).  Like every entry after dg_world_create, neither allocates,
 * frees nor synchronises.  DG_ERR_ARG (nothing launched, outputs untouched) for n_rays <= 0, NULL frac, NULL scratch,
 * and body, frame or skip_body out of range. */
int64_t dg_world_raycast_scratch_floats(const dg_world* w);
int32_t dg_world_raycast(dg_world* w, const float* state,
                         int32_t body, int32_t frame,        /* body -1: rays given in world coordinates; else in the URDF link frame
                                                                `frame` (pybullet joint index, -1 = base: the pose pybullet reports
                                                                for the base, as for a camera) of `body`, per env */
                         int32_t n_rays, const float* ray_from, const float* ray_to,
                         int32_t per_env,                    /* 0: [n_rays][3] shared by all envs; 1: [num_envs][n_rays][3] */
                         int32_t skip_body,                  /* -1, or a body whose shapes no ray can hit (the sensor's own model) */
                         float* scratch,
                         float* frac,      /* [num_envs][n_rays]  hit fraction in [0,1): hit = from + frac (to - from); 1.0 = nothing hit */
                         int32_t* id,      /* [num_envs][n_rays]  uid + ((link + 1) << 24) exactly as dg_world_render's seg; -1 = nothing hit; may be NULL */
                         float* pos,       /* [num_envs][n_rays][3] world hit position (world `to` on a miss); may be NULL */
                         float* normal,    /* [num_envs][n_rays][3] world unit normal at the hit (0 on a miss); may be NULL */
                         void* stream);

/* Dynamics queries on a FIXED-BASE articulated body with at least one joint (DG_BODY_FIXED, not frozen): the calls an
 * operational-space, impedance or computed-torque controller written against pybullet makes (reference
 * diy_gym/addons/controllers/admittance_controller.py:36-55), every env at once.  `nv` is the body's number of joints;
 * columns and entries are in the order of the body's links (the URDF's movable joints, q_index order).  All arrays are device
 * float32.  Like every entry after dg_world_create, none allocates, frees or synchronises; each is one launch on `stream`.
 * DG_ERR_ARG (nothing launched, outputs untouched) for a NULL world or state, a body that is out of range, floating, frozen or
 * without joints, a frame the body does not have, and a body whose passes would need more workspace than the world has.
 *
 * dg_world_joint_state       p.getJointStates (position and velocity): q_out, qd_out [num_envs][nv], either may be NULL.
 * dg_world_jacobian          p.calculateJacobian: `frame` is the pybullet joint index of the link (>= 0; a frame on a fixed joint
 *                            stands for the link it is rigidly attached to), local_pos[3] (HOST floats) a point in that link's
 *                            INERTIAL frame (pybullet's localPosition; the frame DG_WRENCH_LINK_FRAME means).  q [num_envs][nv]
 *                            or NULL = the env's current joint positions.  jac_t, jac_r [num_envs][3][nv] in world coordinates,
 *                            either may be NULL; the columns of joints that are not ancestors of the link are zero.
 * dg_world_inverse_dynamics  p.calculateInverseDynamics: tau [num_envs][nv] = M(q) qdd + C(q, qd) qd - G(q) by one recursive
 *                            Newton-Euler pass.  q, qd [num_envs][nv] or NULL = the env's current values; qdd NULL = zero (with
 *                            qd = qdd = 0: the torques that hold the body against gravity).  Rigid-body terms only: no joint
 *                            damping, friction, motors or limits.
 * dg_world_mass_matrix       p.calculateMassMatrix: M [num_envs][nv][nv] by composite rigid bodies; M[i][j] and M[j][i] are the
 *                            same bits.
 * dg_world_apply_joint_torque  p.setJointMotorControlArray(..., TORQUE_CONTROL, forces=tau): tau [num_envs][nv] is ADDED to
 *                            the joints' torque slots (DG_LS_TORQUE).  It acts during the NEXT dg_world_step only and adds to
 *                            what compiled ops apply -- the contract of dg_world_apply_wrench.
 * Masses and inertias carry the env's mass scale (dynamics_randomizer), gravity is the scene's: these are queries on the
 * world's state, not on the URDF. */
int32_t dg_world_joint_state(dg_world* w, const float* state, int32_t body, float* q_out, float* qd_out, void* stream);
int32_t dg_world_jacobian(dg_world* w, const float* state, int32_t body, int32_t frame, const float* local_pos, const float* q,
                          float* jac_t, float* jac_r, void* stream);
int32_t dg_world_inverse_dynamics(dg_world* w, const float* state, int32_t body, const float* q, const float* qd, const float* qdd,
                                  float* tau, void* stream);
int32_t dg_world_mass_matrix(dg_world* w, const float* state, int32_t body, const float* q, float* M, void* stream);
int32_t dg_world_apply_joint_torque(dg_world* w, float* state, int32_t body, const float* tau, void* stream);

/* Inverse-kinematics query, motor targets and joint reset: with the queries above, what a position-level controller written
 * against pybullet calls (reference diy_gym/addons/controllers/ik_controller.py:47-80, joint_controller.py:38-53), every env at
 * once.  Same bodies and the same rules as the dynamics queries: device float32 arrays, one launch on `stream`, nothing
 * allocated, freed or synchronised; DG_ERR_ARG (nothing launched, outputs untouched) for a NULL world or state, a body that is
 * out of range, floating, frozen or without joints, a frame the body does not have, a NULL required output or input, and a
 * body whose pass would need more workspace than the world has (the query: 9 x nv slots of the transient region).
 *
 * dg_world_inverse_kinematics  p.calculateInverseKinematics: the recursion of the compiled DG_OP_IK_CONTROL's general solve,
 *                            statement for statement -- damped least squares in task space, the optional null-space projection, the
 *                            per-iteration clamp DG_HF_IK_MAX_ANGLE and the early exit on DG_HF_IK_RESIDUAL -- with the world's
 *                            own engine parameters, for at most the world's ik_iterations.  `frame` is the pybullet joint index
 *                            of the link (>= 0, as for dg_world_jacobian); the target is the pose of that link's INERTIAL frame
 *                            (what pybullet targets, what dg_world_frame_state reports with com = 1); target_orn is a unit
 *                            quaternion.  With `lists` the null-space term pulls towards `rest` and off the limits; without,
 *                            the solve is plain damped least squares with DG_HF_IK_JOINT_DAMPING.  The state is not written.
 * dg_world_set_joint_targets  p.setJointMotorControlArray with POSITION_CONTROL / VELOCITY_CONTROL targets: bit i of joint_mask
 *                            selects joint i of the body (all ones: every joint); for those joints DG_LS_TARGET_POS and
 *                            DG_LS_TARGET_VEL are written.  With pos: position target pos, velocity target vel or 0.  With vel
 *                            only: velocity target vel, position target 0 -- exactly what DG_OP_JOINT_CONTROL writes.  Both
 *                            NULL is DG_ERR_ARG.  Targets persist until overwritten (a compiled controller op on the same
 *                            joints, when the step's update mask selects it, runs inside the step and overwrites them).  Gains
 *                            and force limits stay in the motor table (dg_world_set_motor_cfg), uniform over envs.  A body with
 *                            more than 64 joints takes the all-ones mask only.
 * dg_world_reset_joint_state  p.resetJointState: DG_LS_Q and DG_LS_QD of the selected joints of the selected envs; the targets
 *                            are left alone, as in pybullet.  The env's contact impulse cache (DG_H_WARM_OFF), where the scene
 *                            has one, is emptied as dg_world_reset does: cached impulses of a teleported body mean nothing.
 *                            Observations are not refreshed; the next dg_world_observe or dg_world_step does that. */
int32_t dg_world_inverse_kinematics(dg_world* w, const float* state, int32_t body, int32_t frame,
    const float* target_pos,   /* [num_envs][3] world position of the link's INERTIAL frame (what pybullet targets) */
    const float* target_orn,   /* [num_envs][4] xyzw, or NULL = position only */
    const float* lists,        /* [4][nv] rest, lower, upper, range (the order of DG_OP_IK_CONTROL's flist), uniform
                                  over envs; NULL = no null-space term: plain damped least squares with DG_HF_IK_JOINT_DAMPING */
    const float* q0,           /* [num_envs][nv] start, or NULL = the env's current joint positions */
    float* q_out,              /* [num_envs][nv] */
    int32_t* iters_out,        /* [num_envs] iterations in which the env was still live, or NULL */
    void* stream);
int32_t dg_world_set_joint_targets(dg_world* w, float* state, int32_t body, uint64_t joint_mask,
    const float* pos, const float* vel /* [num_envs][nv] each, either may be NULL */, void* stream);
int32_t dg_world_reset_joint_state(dg_world* w, float* state, int32_t body, uint64_t joint_mask,
    const float* q, const float* qd /* [num_envs][nv]; qd NULL = zero */, const uint8_t* env_mask /* [num_envs] or NULL = all */, void* stream);

/* Replaces p.getContactPoints(bodyA, bodyB, linkIndexA, linkIndexB) (pybullet's contact readout; the reference itself never calls
 * it -- none of its addons reads contacts -- so there is no call site to name: this is the query a pybullet user expects, and what
 * the `contact_sensor` addon is built on).  Every env at once, one launch on `stream`, nothing allocated, freed or synchronised;
 * the state is not written.  The kernel runs the step's own narrow phase on `state` and reports its contact list, in the order
 * of the candidate pairs, at most C = the world's max_contacts (DG_H_MAX_CONTACTS of the scene blob) per env -- the step never
 * has more, so the query never truncates beyond what the solver itself saw.  A world built with hull_manifold_points > 1 reports
 * the up-to-N points per hull pair that its step sees.
 *   count [num_envs]          contacts that passed the filter
 *   ids   [num_envs][C][2]    side A, side B: uid + ((link + 1) << 24) exactly as dg_world_render's seg and dg_world_raycast's id
 *   geom  [num_envs][C][10]   position on A (3), position on B (3), unit normal on B pointing towards A (3), signed distance
 *                             (negative: penetration) -- pybullet's positionOnA, positionOnB, contactNormalOnB, contactDistance
 *   force [num_envs][C]       normal force in newtons (pybullet's normalForce)
 * ids, geom and force may each be NULL.  EVERY slot of the given arrays is written: behind an env's count the ids are -1 and the
 * rest 0, so a reused buffer needs no memset and a sum over the C slots is right without a mask.
 * Filters: body_* is a body index (a Model's uid), link_* a pybullet link index (-1: the base), DG_CONTACT_ANY: no filter; they are
 * compared with the uid part (id & 0xFFFFFF) and the link part ((id >> 24) - 1) of the ids.  With only body_a given, a contact
 * that has that body on its B side is reported with the sides swapped and the normal negated: the caller always sees its body as
 * A and the normal pointing towards it.  With both given either orientation matches and is reported as (a, b).
 * STALENESS, the rule in full: the geometry is recomputed from the state handed in; the force is the normal impulse the solver
 * applied IN THE LAST SUBSTEP to the contact with the same key (DG_CONTACT_KEY(pair, feature), the contact impulse cache
 * DG_WS_*), divided by the substep length.  (pybullet is stale the other way round: its points are those of the last
 * stepSimulation whatever has been reset since.)  A contact that is new since that substep reports 0 N, and so does one whose
 * feature changed (a hull resting on a box whose deepest corner is now another one).  After dg_world_reset_joint_state every
 * force of the env is 0 until the next step; after dg_world_reset the cache is that of the hot-start steps.  Lateral friction:
 * dg_world_contact_forces.
 * DG_ERR_ARG (nothing launched, outputs untouched): NULL world, state or count; a body out of range; a link the body does not
 * have (one that neither a shape of the body carries in its id -- the shapes of a rigidly merged child model carry the CHILD's own
 * link index -- nor is one of the body's frames); a link filter without its body filter.  DG_ERR_UNSUPPORTED: force given in a world without the impulse cache
 * (DG_H_WARM_OFF < 0: warmstart and warmstart_friction both 0, or no candidate pairs).  A world without candidate pairs answers
 * DG_OK with every count 0 when force is NULL. */
#define DG_CONTACT_ANY (-2)
int32_t dg_world_contacts(dg_world* w, const float* state,
    int32_t body_a, int32_t link_a, int32_t body_b, int32_t link_b,   /* uid / pybullet link index; DG_CONTACT_ANY (-2) = no filter, link -1 = base */
    int32_t* count /* [B] */, int32_t* ids /* [B][C][2], may be NULL */, float* geom /* [B][C][10]: posA3 posB3 normal3 dist, may be NULL */,
    float* force /* [B][C], may be NULL */, void* stream);

/* Contact forces in full: what dg_world_contacts leaves out.  pybullet's getContactPoints also reports lateralFriction1,
 * lateralFrictionDir1, lateralFriction2 and lateralFrictionDir2; dg_world_contact_forces reports them for every env at once, and
 * dg_world_net_contact_wrench sums the contact forces per link -- the net contact force tensor of a batched simulator.  Each is one
 * launch on `stream`; nothing is allocated, freed or synchronised; the state is not written.  Both run the step's own narrow phase
 * on `state` and look every contact up in the contact impulse cache (DG_WS_*: [key, normal, t1, t2] per contact, written at the end
 * of every substep), so a world without the cache (DG_H_WARM_OFF < 0: warmstart and warmstart_friction both 0, or no candidate
 * pairs) answers DG_ERR_UNSUPPORTED to both.
 *
 * dg_world_contact_forces: rows, count, ids, filters and side swapping are exactly those of dg_world_contacts (same state, same
 * filters: the same rows in the same order).  forces [num_envs][C][DG_CFO_STRIDE], columns DG_CFO_*:
 *   DG_CFO_NORMAL (3)        unit normal on B pointing towards A, as dg_world_contacts
 *   DG_CFO_NORMAL_FORCE      normal force in newtons, the bits dg_world_contacts reports
 *   DG_CFO_LATERAL1, _2      friction force along the first / second tangent in newtons, signed (pybullet's lateralFriction1, 2)
 *   DG_CFO_DIR1, _DIR2 (3)   the unit tangents (lateralFrictionDir1, 2): the basis the solver's friction rows were built with
 *   DG_CFO_FORCE_A (3)       the total force the contact applies to side A, world axes; side B receives its negative:
 *                           force_on_a = normal_force x normal + lateral1 x dir1 + lateral2 x dir2
 * ids and forces may be NULL, count is required; EVERY slot of the given arrays is written: -1 ids and zeros behind the count.
 * When the filter swaps the sides (dg_world_contacts: the body asked for is always side A), the normal and BOTH tangents are
 * negated and the three scalars kept, so that (X, Y) and (Y, X) report forces that are exact negatives of each other.  (The
 * tangents are NOT the basis of the negated normal: that would flip the first tangent only.)
 *
 * dg_world_net_contact_wrench: one body, n link selectors links[0 .. n-1] (a HOST array, copied into the kernel's arguments; 1 <= n
 * <= DG_CONTACT_MAX_LINKS).  A selector is DG_CONTACT_ANY -- the whole body -- or a pybullet link index (-1: the base) that is a
 * FRAME of the body; body_b / link_b optionally restrict the other side as in dg_world_contacts (DG_CONTACT_ANY: no filter).
 *   wrench    [num_envs][n][6]  per selector the sum, over the contacts whose side on this body matches the selector, in pair
 *                               order, of the force on this body (3) and of its moment (3) about the origin of that link's INERTIAL
 *                               frame -- the point dg_world_frame_state reports with com = 1; for DG_CONTACT_ANY and -1 the base's.
 *                               The moment arm is the surface point on this body's side (position on A of dg_world_contacts).
 *   ncontacts [num_envs][n]     contacts summed; may be NULL
 * Every slot is written exactly once.  The shapes of a rigidly merged child model carry the CHILD's own link indices in their ids:
 * such an index is not a frame of the body and is refused as a selector here (where it coincides with a frame index of the body,
 * both match, as in dg_world_contacts) -- those shapes stay reachable through DG_CONTACT_ANY and, link by link, through
 * dg_world_contact_forces.  A contact between two links of the one body that both match a selector counts once, as side A.
 *
 * STALENESS, the rule in full (both entries): the geometry -- points, normal, tangents, moment arms and reference points -- is
 * recomputed from the state handed in.  The three impulses are those the solver ended the LAST SUBSTEP with for the contact with
 * the same key (DG_CONTACT_KEY(pair, feature)), divided by the substep length, without the warm-start factors; a contact that is
 * new since that substep, or whose feature changed, reports 0 in all three.  The tangents are those of the CURRENT normal
 * (a fixed function of it); for a contact that persists with an unchanged normal that is the basis the impulses were solved in,
 * and when the normal has turned since, the cached scalars are reported along the turned basis.  After dg_world_reset_joint_state
 * every force of the env is 0 until the next step.
 * DG_ERR_ARG (nothing launched, outputs untouched): NULL world, state, count (contact_forces), links or wrench (net wrench); the
 * filter errors of dg_world_contacts; n < 1 or n > DG_CONTACT_MAX_LINKS; a body out of range; a selector that is not a frame of
 * the body. */
enum { DG_CFO_NORMAL = 0, DG_CFO_NORMAL_FORCE = 3, DG_CFO_LATERAL1 = 4, DG_CFO_DIR1 = 5, DG_CFO_LATERAL2 = 8, DG_CFO_DIR2 = 9, DG_CFO_FORCE_A = 12,
       DG_CFO_STRIDE = 15 };
#define DG_CONTACT_MAX_LINKS 16
int32_t dg_world_contact_forces(dg_world* w, const float* state,
    int32_t body_a, int32_t link_a, int32_t body_b, int32_t link_b,   /* as dg_world_contacts */
    int32_t* count /* [B] */, int32_t* ids /* [B][C][2], may be NULL */, float* forces /* [B][C][DG_CFO_STRIDE], may be NULL */, void* stream);
int32_t dg_world_net_contact_wrench(dg_world* w, const float* state, int32_t body,
    const int32_t* links /* host [n]: DG_CONTACT_ANY or a frame of the body */, int32_t n,
    int32_t body_b, int32_t link_b,   /* the other side; DG_CONTACT_ANY = no filter */
    float* wrench /* [B][n][6]: force3 moment3 */, int32_t* ncontacts /* [B][n], may be NULL */, void* stream);

/* Replaces p.getClosestPoints(bodyA, bodyB, distance, linkIndexA, linkIndexB) (the reference itself never calls it -- none of its
 * addons asks for a clearance -- so there is no call site to name: this is the query a pybullet user expects, and what the
 * `proximity_sensor` addon is built on).  dg_world_contacts stops at the world's contact margin and knows only the pairs the step
 * tests; this entry reports every pair of shapes nearer than `distance`, the pairs static pruning removed from the step included.
 * Every env at once, two launches on `stream` (the shape poses, then the query), nothing allocated, freed or synchronised; the
 * state is not written.  dg_world_closest_scratch_floats: floats of caller-owned device scratch (the per-env shape pose table and
 * the polytope workspace of the hull-against-hull routine).
 * Candidate pairs: side A is every shape of (body_a, link_a) in ascending shape index, side B every shape of (body_b, link_b) --
 * with DG_CONTACT_ANY every shape of ANOTHER body -- in ascending index under each A shape.  Never a pair: two shapes of one body
 * (a rigidly merged child is its parent's body), visual-only shapes, two shapes neither of which can move, BOX AGAINST BOX (the
 * step has no routine for it either).  Each pair is measured in the step's own model of it (a hull against a round shape through
 * the hull's fitted capsule, a hull against a box through the hull's points, two hulls as polytopes in a hull_contacts world with
 * the hull margin subtracted -- overlapping hulls report the polytope depth), so the distance meets dg_world_contacts' as the
 * pair closes.
 *   count        [num_envs]        pairs with distance < `distance` (penetrating pairs always), whether or not they fit in K
 *   ids          [num_envs][K][2]  side A, side B: uid + ((link + 1) << 24) as dg_world_contacts
 *   geom         [num_envs][K][10] position on A (3), position on B (3), unit normal on B pointing towards A (3), signed distance
 *   nearest_ids  [num_envs][2]     the pair of smallest distance over ALL pairs found, independent of K (a tie: the first in pair
 *   nearest_geom [num_envs][10]    order).  Nothing within `distance`: ids -1, positions and normal 0, the distance field =
 *                                  `distance` -- usable as an observation as it is.
 * Rows come in (shape a, shape b) order; rows beyond K = max_points are dropped and still counted: count > K means truncated.
 * EVERY slot of the given arrays is written: behind the rows the ids are -1 and the rest 0.  The body given as A is always side A.
 * There is no force: pybullet reports 0 there.  Filters, ids and the alias rule of a merged child are those of dg_world_contacts.
 * DG_ERR_ARG (nothing launched, outputs untouched): NULL world, state, count or scratch; body_a == DG_CONTACT_ANY; a body out of
 * range; a link its body does not have; a link filter without its body; distance not finite or < 0; max_points < 0; max_points > 0
 * with ids and geom both NULL. */
int64_t dg_world_closest_scratch_floats(const dg_world* w);
int32_t dg_world_closest(dg_world* w, const float* state,
    int32_t body_a, int32_t link_a, int32_t body_b, int32_t link_b,  /* body_a required; the others may be DG_CONTACT_ANY */
    float distance, int32_t max_points /* K >= 0 */, float* scratch,
    int32_t* count        /* [B]       pairs within `distance`, whether or not they fit in K */,
    int32_t* ids          /* [B][K][2] may be NULL */, float* geom /* [B][K][10] posA3 posB3 normal3 dist, may be NULL */,
    int32_t* nearest_ids  /* [B][2]    may be NULL */, float* nearest_geom /* [B][10] may be NULL */, void* stream);

/* Link states and base reset: the state reads and the state write the reference's addons make through p.getLinkStates /
 * p.getLinkState(computeLinkVelocity=1) / p.getBasePositionAndOrientation / p.getBaseVelocity (reference
 * diy_gym/addons/sensors/object_state_sensor.py:35-42, rewards/reach_target.py:22-28, sensors/camera.py:60-63) and
 * p.resetBasePositionAndOrientation / p.resetBaseVelocity (misc/respawn.py:35, model.py:68-74), every env at once.  The rules of
 * the query entries above: device float32 arrays, one launch on `stream`, nothing allocated, freed or synchronised; on DG_ERR_ARG
 * nothing is launched, outputs are untouched and dg_last_error names the entry.
 *
 * dg_world_link_states       n (body, frame) selectors, 1 <= n <= DG_LINK_STATES_MAX, as two HOST arrays copied into the kernel's
 *                            arguments.  out [num_envs][n][13]: row k of an env is exactly what dg_world_frame_state(body =
 *                            bodies[k], frame = frames[k], com) writes for that env -- position (3), quaternion xyzw (4), world
 *                            linear (3) and angular (3) velocity, of the URDF link frame or with com = 1 of the link's inertial
 *                            frame -- bit for bit: the same device function after the same kinematics, which run once per
 *                            DISTINCT body among the selectors.  Every (body, frame) dg_world_frame_state takes is taken, a frozen
 *                            body's base included.  The state is not written.  DG_ERR_ARG: NULL world, state, bodies, frames or
 *                            out; n out of range; a body out of range; a frame its body does not have.
 * dg_world_reset_base_state  the base of `body` in the envs env_mask selects (NULL: all).  pos / orn (both or neither) are the pose
 *                            of the base's INERTIAL frame -- what dg_world_frame_state(body, -1, com = 1) reports in columns 0:7
 *                            and what the compiled DG_OP_RESPAWN hands to the same device function, so an equal pose is stored as
 *                            the same bits; orn is normalised on the device.  lin_vel / ang_vel are columns 7:13 of the same
 *                            report: the world velocity of that frame's origin and the world angular velocity.  The state stores
 *                            the velocity of the base LINK's origin; the entry converts, so dg_world_frame_state returns what was
 *                            written.  With a pose, a velocity that is NULL is set to zero (as DG_OP_RESPAWN and pybullet do);
 *                            with pos and orn NULL only the given velocities change, as p.resetBaseVelocity -- the other keeps its
 *                            REPORTED value; all four NULL is DG_ERR_ARG.  In the selected envs the contact impulse cache
 *                            (DG_H_WARM_OFF), where the scene has one, is emptied as dg_world_reset_joint_state does.  Joint
 *                            state, motor targets, external wrenches, addon state and the step and episode counters are not
 *                            touched; observations are refreshed by the next dg_world_observe or dg_world_step.
 *                            WHICH BODIES: a base can be moved only if the planner did not assume it stays at its load pose
 *                            (static pair pruning, anchored bounding spheres): a floating base, or a fixed base that carries a
 *                            DG_OP_RESPAWN (a `respawn` addon with zero ranges is how a scene declares a bolted-down body
 *                            movable).  Any other body -- a frozen one included -- is DG_ERR_ARG with a message that says to add
 *                            a respawn addon; so is a velocity for a fixed base, pos without orn or the reverse, a body out of
 *                            range, a NULL world or state. */
#define DG_LINK_STATES_MAX 32
int32_t dg_world_link_states(dg_world* w, const float* state,
    const int32_t* bodies /* host [n] */, const int32_t* frames /* host [n]: pybullet joint index, -1 = base */, int32_t n,
    int32_t com, float* out /* [num_envs][n][13]: pos3 quat4 linvel3 angvel3 */, void* stream);
int32_t dg_world_reset_base_state(dg_world* w, float* state, int32_t body,
    const float* pos /* [B][3] */, const float* orn /* [B][4] xyzw */,      /* both or neither */
    const float* lin_vel, const float* ang_vel /* [B][3] each, may be NULL */,
    const uint8_t* env_mask /* [B] or NULL = all */, void* stream);

/* Joint reaction wrenches and applied motor torques: the second half of p.getJointState(s) -- jointReactionForces (after
 * p.enableJointForceTorqueSensor) and appliedJointMotorTorque (reference diy_gym/addons/sensors/force_torque_sensor.py:14-23,
 * rewards/electricity_cost.py:13-18), every env at once.  The rules of the query entries above: device float32 arrays, one launch
 * on `stream`, nothing allocated, freed or synchronised, the state is not written; on an error nothing is launched, outputs are
 * untouched and dg_last_error names the entry.
 *
 * dg_world_joint_wrench   n joint selectors of ONE body, 1 <= n <= DG_JOINT_WRENCH_MAX, as a HOST array copied into the kernel's
 *                         arguments.  wrench [num_envs][n][6] = [Fx Fy Fz Mx My Mz]: the force and the torque the PARENT side
 *                         exerts on the CHILD side through the joint `frame` (fixed or movable), expressed in the inertial frame
 *                         of the joint's child link (DG_FF_COM_* of the frame), the torque about that frame's origin -- exactly
 *                         what the compiled DG_OP_OBS_FT reports.  The child side is the rigid cluster of URDF links behind the
 *                         joint -- `rigid`: mass, centre (3) and inertia about it (xx xy xz yy yz zz) in the frame of the moving
 *                         link the cluster is part of; with DG_FT_WHOLE_LINK in `flags` (a movable joint) the whole moving link
 *                         from the link table instead -- plus the moving links of `link_mask` (bit i: link i of the body).
 *                         Newton-Euler over these with the accelerations (v_now - v_prev) / h and gravity taken off, v_prev being
 *                         the body's velocities at the start of the last substep (DG_BI_PREV_OFF), MINUS the contact forces on
 *                         child-side shapes: a shape of the body is on the child side when its URDF link is in `frame_mask` (bit
 *                         j: pybullet link j) or its moving link in `link_mask`, and a contact counts when exactly ONE of its two
 *                         shapes is.  The arm of a contact force is the contact POINT, the midpoint of dg_world_contacts' position
 *                         on A and position on B, as in the compiled op -- NOT the surface point dg_world_net_contact_wrench uses.
 *                         Motors, applied joint torques and external wrenches are no terms of their own: they show through the
 *                         motion.
 *                         STALENESS follows dg_world_contact_forces: the contact geometry is that of the narrow phase run on the
 *                         state handed in, the three impulses the cached ones of the contact with the same key over h, 0 for a
 *                         new contact.  The compiled op reads the last substep's own list: the two agree to rounding where
 *                         nothing touches and at rest, and differ by one substep of motion while contacts move.
 *                         Nothing saves velocities on a teleport: after dg_world_reset_joint_state, dg_world_reset_base_state or a
 *                         state written by the caller that changes a velocity, the reading carries the jump (v_new - v_prev) / h
 *                         until the next step; the state of the last step handed in unchanged reads as before.  After
 *                         dg_world_reset the accelerations are zero and the cache is empty: the plain gravity load, the compiled
 *                         op's plain-observe mode.
 *                         DG_ERR_ARG: NULL world, state, selectors or wrench; n out of range; a body out of range, frozen, with
 *                         more than 64 links or frames, or WITHOUT SAVED VELOCITIES (the message names the remedy:
 *                         builder.enable_joint_force_torque(body) at build time, or a compiled force_torque_sensor on the body);
 *                         a frame the body does not have; a mask bit past the body's links or frames; a body whose pose and motion
 *                         block (21 slots for the base and per link) does not fit the world's transient region.  DG_ERR_UNSUPPORTED, as
 *                         dg_world_contact_forces: a world with candidate pairs that keeps no contact impulse cache.  A world
 *                         without candidate pairs has no contact term and is taken.
 *                         NOT CHECKED: a body that carries a rigidly merged child model.  The shapes of the child carry the child's
 *                         own URDF link indices, which coincide with bits of the parent's in `frame_mask`, and the rigid numbers of a
 *                         cluster the child hangs on do not include it: HipBackend refuses such a body (FlatBody.ft_cluster), a
 *                         direct caller must not pass one.
 * dg_world_joint_efforts  out [num_envs][n_links]: the motor torque applied to each joint of `body` during the last solver pass
 *                         (DG_LS_APPLIED; what joint_state_sensor's effort columns and DG_OP_REW_ELECTRICITY read), joints in link
 *                         order.  Any body with joints, fixed or floating base.  DG_ERR_ARG: NULL world, state or out; a body out
 *                         of range, frozen or without joints. */
#define DG_JOINT_WRENCH_MAX 16
typedef struct dg_joint_selector {
  int32_t frame;        /* pybullet joint index of the body (the kernels see the global frame index) */
  int32_t flags;        /* DG_FT_WHOLE_LINK: the joint is movable, the rigid part is its whole moving link */
  uint64_t link_mask;   /* child-side moving links, bit i = link i of the body */
  uint64_t frame_mask;  /* URDF links of the rigid cluster, bit j = pybullet link j: shape membership */
  float rigid[10];      /* mass, com3, inertia xx xy xz yy yz zz of the rigid cluster in its moving link's frame */
} dg_joint_selector;
int32_t dg_world_joint_wrench(dg_world* w, const float* state, int32_t body,
    const dg_joint_selector* selectors /* host [n] */, int32_t n, float* wrench /* [num_envs][n][6]: force3 torque3 */, void* stream);
int32_t dg_world_joint_efforts(dg_world* w, const float* state, int32_t body, float* out /* [num_envs][n_links] */, void* stream);

/* Link accelerations and IMU readings: how links ACCELERATE, and what an accelerometer and a gyro mounted on one read, every env at
 * once.  pybullet has no such call and the reference no such addon; what env.sim.link_accelerations and the imu_sensor addon are
 * built on.  The rules of the query entries above: device float32 arrays, one launch on `stream`, nothing allocated, freed or
 * synchronised, the state is not written; on an error nothing is launched, outputs are untouched and dg_last_error names the entry.
 *
 * dg_world_link_accelerations  n sensor-frame selectors of ONE body, 1 <= n <= DG_LINK_ACCEL_MAX, as a HOST array copied into the
 *                         kernel's arguments.  A selector names a frame S: `frame` the pybullet joint index (-1: the base), `com`
 *                         0 the URDF link frame (what camera and lidar mount on) or 1 the link's inertial frame (as
 *                         dg_world_link_states), and a mount pose `pos`, `quat` (xyzw, normalised by the entry) relative to it.
 *                         Let L be the moving link S is rigidly attached to, (R_L, p_L, w, v, alpha, a) its pose and motion --
 *                         accelerations (v_now - v_prev) / h with h the substep and v_prev the body's velocities at the start of
 *                         the last substep (DG_BI_PREV_OFF), exactly as dg_world_joint_wrench forms them -- R_s, p_s the world
 *                         pose of S, r = p_s - p_L and g the scene's gravity.  out [num_envs][n][DG_LA_STRIDE], columns DG_LA_*:
 *                           DG_LA_LIN_ACC         a + alpha x r + w x (w x r), world axes
 *                           DG_LA_ANG_ACC         alpha, world axes
 *                           DG_LA_SPECIFIC_FORCE  R_s^T (lin_acc - g): what an accelerometer reads ((0, 0, +|g|) at rest and level)
 *                           DG_LA_ANG_VEL         R_s^T w: what a gyro reads
 *                           DG_LA_GRAVITY         R_s^T g / |g|, zeros when g = 0: the projected gravity direction
 *                         No contact term and no narrow phase: contact, motor and external forces show through the motion, so a
 *                         world without candidate pairs or without the contact impulse cache is taken.
 *                         STALENESS follows dg_world_joint_wrench.  Nothing saves velocities on a teleport: after
 *                         dg_world_reset_joint_state, dg_world_reset_base_state or a state written by the caller that changes a
 *                         velocity, the reading carries the jump (v_new - v_prev) / h until the next step; the state of the last
 *                         step handed in unchanged reads as before.  After dg_world_reset the accelerations are zero and
 *                         specific_force = -R_s^T g.
 *                         Bodies: a floating base with or without joints, a fixed base with joints.
 *                         DG_ERR_ARG: NULL world, state, selectors or out; n out of range; a body out of range, frozen or WITHOUT
 *                         SAVED VELOCITIES (the message names the remedy: builder.enable_joint_force_torque(body) at build time
 *                         -- imu_sensor does -- or a compiled force_torque_sensor on the body; a fixed base without joints keeps
 *                         none: its reading is the constant -g); a frame the body does not have; a mount quaternion of zero norm;
 *                         a body whose pose and motion block (21 slots for the base and per link) does not fit the world's
 *                         transient region. */
#define DG_LINK_ACCEL_MAX 16
enum { DG_LA_LIN_ACC = 0, DG_LA_ANG_ACC = 3, DG_LA_SPECIFIC_FORCE = 6, DG_LA_ANG_VEL = 9, DG_LA_GRAVITY = 12, DG_LA_STRIDE = 15 };
typedef struct dg_accel_selector {
  int32_t frame;   /* pybullet joint index of the body, -1: the base (the kernels see the global frame index) */
  int32_t com;     /* 0: the URDF link frame, 1: the link's inertial frame */
  float pos[3];    /* the mount: position in that frame */
  float quat[4];   /* ... and orientation, xyzw */
} dg_accel_selector;  /* 36 bytes */
int32_t dg_world_link_accelerations(dg_world* w, const float* state, int32_t body,
    const dg_accel_selector* selectors /* host [n] */, int32_t n, float* out /* [num_envs][n][15] */, void* stream);

/* Task-space dynamics of one point of a fixed-base articulated body, every env at once, in ONE launch: what an operational-space
 * (Cartesian impedance) controller needs per tick.  Same bodies and rules as the dynamics queries: device float32 arrays, nothing
 * allocated, freed or synchronised; `frame` and local_pos[3] (HOST floats) as dg_world_jacobian takes them.  The task vector is
 * [v; w] of that point in world axes; bit k of axes_mask (k = 0 .. 5) selects its row k, m is the number of set bits, nv the
 * body's number of joints.
 *   q, qd      [num_envs][nv] or NULL = the env's own values (a NULL call and a call given the same numbers are the same bits)
 *   acc        [num_envs][m] or NULL: the desired task acceleration (required by tau)
 *   tau_null   [num_envs][nv] or NULL: a joint torque to be applied through the dynamically consistent null-space projector
 *   damping    >= 0, added to the diagonal of J M^-1 J^T
 * Outputs; each may be NULL, at least one must not be:
 *   jac          [num_envs][m][nv]  the selected rows of [jac_t; jac_r]
 *   bias_acc     [num_envs][m]      the selected rows of Jdot qd: the task acceleration at qdd = 0
 *   bias_torque  [num_envs][nv]     h = C qd - G: dg_world_inverse_dynamics(q, qd, 0)
 *   lambda       [num_envs][m][m]   (J M^-1 J^T + damping I)^-1, symmetric in bits
 *   tau          [num_envs][nv]     J^T lambda (acc - Jdot qd) + h + (tau_null - J^T lambda J M^-1 tau_null)
 *   point        [num_envs][13]     the point's position, the quaternion (xyzw) of the link's inertial frame, the point's
 *                                   linear velocity and the link's angular velocity at the q, qd worked at
 *   singular     [num_envs] int32   1 when a pivot of the Cholesky factorisation of M or of J M^-1 J^T + damping I was <= 1e-5 x
 *                                   the largest diagonal entry of the matrix factored; the pivot is then that floor, so every
 *                                   output stays finite.  M is taken in its Jacobi-scaled form (unit diagonal: pivot j against
 *                                   1e-5 x M[j][j]), so that a tree of very unequal links -- an arm with a gripper -- is not
 *                                   flagged for its sizes
 * DG_ERR_ARG (nothing launched, outputs untouched) for what the dynamics queries refuse, an axes_mask with no bit or a bit above 5,
 * m > nv, a damping that is negative or not finite, every output NULL, tau without acc, tau_null without tau, and a body whose
 * pass would need more workspace than the world has. */
int32_t dg_world_task_space(dg_world* w, const float* state, int32_t body, int32_t frame, const float* local_pos, int32_t axes_mask,
                            const float* q, const float* qd, const float* acc, const float* tau_null, float damping,
                            float* jac, float* bias_acc, float* bias_torque, float* lambda, float* tau, float* point, int32_t* singular,
                            void* stream);

/* Forward dynamics of a fixed-base articulated body, every env at once, in ONE launch: qdd = M(q)^-1 (tau - h(q, qd)) with
 * h = C qd - G, the rigid-body terms of dg_world_inverse_dynamics -- the two calls are inverses of each other.  Same bodies and
 * rules as the dynamics queries: device float32 arrays, nothing allocated, freed or synchronised.
 *   q, qd, tau     [num_envs][nv] or NULL = the env's own q, qd; a NULL tau is zero (a NULL call and a call given the same numbers
 *                  are the same bits)
 *   joint_damping  != 0: tau is first reduced by the joints' URDF damping x qd, the term the step applies
 *   qdd            [num_envs][nv]
 *   singular       [num_envs] int32, nullable: 1 when a pivot of the Cholesky factorisation of M was <= 1e-5 x its own diagonal
 *                  entry of M (dg_world_task_space's rule); the pivot is then that floor, so qdd stays finite
 * DG_ERR_ARG (nothing launched, outputs untouched) for what the dynamics queries refuse, qdd and singular both NULL, and a body
 * whose pass would need more workspace than the world has. */
int32_t dg_world_forward_dynamics(dg_world* w, const float* state, int32_t body, const float* q, const float* qd, const float* tau,
                                  int32_t joint_damping, float* qdd, int32_t* singular, void* stream);

/* K candidate torque sequences per env rolled T steps through the body's own rigid-body model, in ONE launch: the inner loop of
 * sampling MPC and shooting methods.  Sample k of env e starts at q0[e], qd0[e] (NULL: the env's own) and for t = 0 .. T-1 takes
 * qdd = dg_world_forward_dynamics(q, qd, tau[e][k][t]) and integrates semi-implicitly, the step's order: qd += dt qdd; q += dt qd.
 * Row t of every output is the state AFTER step t + 1.  The env's own per-env masses apply; the state is read, never written.  A
 * MODEL of the arm, not the step: no joint limits, motors, link damping or contacts.
 *   frame, local_pos   the point whose world position pos_out reports: local_pos[3] (HOST floats) in the INERTIAL frame of the link
 *                      of `frame` (the body's pybullet joint index), as dg_world_jacobian takes it; read only when pos_out is set
 *   tau                [num_envs][K][T][nv], required
 *   q_out, qd_out      [num_envs][K][T][nv]
 *   pos_out            [num_envs][K][T][3], at the NEW q of each step
 *   singular           [num_envs][K] int32: 1 when any step of the sample held a pivot at the floor
 * Each output may be NULL, at least one must not be.  DG_ERR_ARG (nothing launched, outputs untouched) for what the dynamics queries
 * refuse, K < 1, T < 1, a dt that is not finite or <= 0, tau NULL, every output NULL, num_envs x K x T x nv beyond INT64_MAX / 4,
 * with pos_out a NULL local_pos or a frame the body does not have, and a body whose pass would need more workspace than the world
 * has. */
int32_t dg_world_rollout(dg_world* w, const float* state, int32_t body, int32_t frame, const float* local_pos, int32_t K, int32_t T,
                         float dt, int32_t joint_damping, const float* q0, const float* qd0, const float* tau,
                         float* q_out, float* qd_out, float* pos_out, int32_t* singular, void* stream);

/* The derivatives of dg_world_forward_dynamics at P points per env, in ONE launch of num_envs x P work items: what LQR, iLQR / DDP,
 * an EKF and backpropagation through the model linearise with.  With d the joints' URDF damping when joint_damping != 0, else
 * zero, and ID the rigid-body inverse dynamics of dg_world_inverse_dynamics, per point:
 *   qdd        [num_envs][P][nv]      M^-1 (tau - d o qd - h(q, qd)): dg_world_forward_dynamics' result, bit for bit
 *   dqdd_dq    [num_envs][P][nv][nv]  -M^-1 dtau_dq        row-major, [i][j] = d qdd_i / d q_j
 *   dqdd_dqd   [num_envs][P][nv][nv]  -M^-1 dtau_dqd
 *   dqdd_dtau  [num_envs][P][nv][nv]   M^-1
 *   dtau_dq    [num_envs][P][nv][nv]  d ID_i(q, qd, qdd) / d q_j at FIXED qdd
 *                                     (the point is qdd refined once against the inverse-dynamics residual, in the workspace: the
 *                                     qdd output keeps dg_world_forward_dynamics' bits, whose fp32 error grows with cond(M))
 *   dtau_dqd   [num_envs][P][nv][nv]  d ID_i / d qd_j + d_i delta_ij
 *   singular   [num_envs][P] int32    dg_world_forward_dynamics' flag
 * The derivatives are analytic (a forward-mode tangent of the Newton-Euler passes), never finite differences; first derivatives only.
 *   q, qd, tau [num_envs][P][nv] or NULL = the env's own q, qd, zero torque, at every point of that env
 * Each output may be NULL and then costs nothing; at least one must not be.  The state is read, never written; the env's own per-env
 * masses apply.  DG_ERR_ARG (nothing launched, outputs untouched) for what dg_world_forward_dynamics refuses, P < 1, every output
 * NULL, num_envs x P x nv x nv beyond INT64_MAX / 4, a body of more than 64 joints, and a body whose pass would need more workspace
 * than the world has (33 nv slots of the transient region). */
int32_t dg_world_dynamics_derivatives(dg_world* w, const float* state, int32_t body, int32_t P, const float* q, const float* qd, const float* tau,
                                      int32_t joint_damping, float* qdd, float* dqdd_dq, float* dqdd_dqd, float* dqdd_dtau,
                                      float* dtau_dq, float* dtau_dqd, int32_t* singular, void* stream);

/* The inertial parameters of `body`'s links in every env: theta [num_envs][nv][10], per link (joint index l = 0 .. nv-1; a link is a
 * movable joint's child link with everything fixed to it merged) in the link's OWN frame
 *   theta_l = [m, m cx, m cy, m cz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz]
 * with c the centre of mass and I the inertia about the link-frame ORIGIN in link axes.  The env's per-env mass scale (the
 * dynamics_randomizer's) multiplies all ten; nominal != 0 gives the unscaled values of the scene instead.  theta must be 8-byte
 * aligned (a link's ten floats leave as 8-byte stores).  DG_ERR_ARG (nothing launched) for what the dynamics queries refuse, a NULL
 * theta and a theta that is not 8-byte aligned. */
int32_t dg_world_inertial_parameters(dg_world* w, const float* state, int32_t body, int32_t nominal, float* theta, void* stream);

/* The regressor of the rigid-body inverse dynamics at P points per env, in ONE launch of num_envs x P work items: what parameter
 * identification, adaptive control and excitation-trajectory design start from.  Inverse dynamics is linear in the inertial
 * parameters of dg_world_inertial_parameters, theta as [10 nv]:
 *   dg_world_inverse_dynamics(q, qd, qdd) = Y(q, qd, qdd) theta
 * and with a reference velocity qd_ref (Slotine-Li)  Y theta = M qdd + C(q, qd) qd_ref - G  with the Christoffel C, so that
 * Mdot - 2 C is skew-symmetric; the product is symmetric in (qd, qd_ref), and qd_ref = qd is the plain regressor.
 *   q, qd, qdd, qd_ref [num_envs][P][nv] or NULL = the env's own q and qd, qdd = 0, qd_ref = qd, at every point of that env
 *   theta_hat          [num_envs][10 nv], per env, nullable
 *   s                  [num_envs][P][nv], nullable
 *   Y                  [num_envs][P][nv][10 nv] row-major; the blocks of links a joint does not carry are written as zeros
 *   tau                [num_envs][P][nv]     Y theta_hat, formed WITHOUT Y by a Newton-Euler pass: O(nv); needs theta_hat
 *   grad               [num_envs][P][10 nv]  Y^T s, formed WITHOUT Y from the links' virtual twists: O(nv); needs s
 * Each output may be NULL and then costs nothing; at least one must not be.  The state is read, never written; the env's own masses
 * do not enter (theta_hat is the caller's).  DG_ERR_ARG (nothing launched, outputs untouched) for what the dynamics queries refuse,
 * P < 1, every output NULL, tau without theta_hat, grad without s, a Y or grad that is not 8-byte aligned (blocks of ten floats leave
 * as 8-byte stores), num_envs x P x nv x 10 nv beyond INT64_MAX / 4, and a body whose
 * pass would need more workspace than the world has (23 nv slots of the transient region). */
int32_t dg_world_id_regressor(dg_world* w, const float* state, int32_t body, int32_t P, const float* q, const float* qd, const float* qdd,
                              const float* qd_ref, const float* theta_hat, const float* s, float* Y, float* tau, float* grad, void* stream);

/* dg_world_rollout with the torque of every step formed INSIDE the loop from the state BEFORE the step: the forward pass and line
 * search of iLQR / DDP, and the model evaluation of any time-varying feedback policy (TVLQR tracking, tube MPC), in ONE launch of
 * num_envs x K work items.  Sample k of env e, step t, at the state q_t, qd_t (t = 0: q0[e], qd0[e], NULL = the env's own):
 *   tau = tau_ff[e][t] + alpha[k] dtau[e][t] + gain[e][t] . [q_t - q_ref[e][t]; qd_t - qd_ref[e][t]]
 *   tau = clamp(tau, -tau_limit, +tau_limit)       joint by joint where tau_limit[i] > 0, and only when tau_limit is given
 *   qdd = dg_world_forward_dynamics(q_t, qd_t, tau);  qd += dt qdd;  q += dt qd
 *   tau_ff             [num_envs][T][nv], required
 *   dtau, alpha        [num_envs][T][nv] and [K] (device), nullable: without dtau the alpha term is absent and alpha is not read
 *   gain               [num_envs][T][nv][2 nv] row-major, columns [q | qd], nullable; with it q_ref, qd_ref [num_envs][T][nv] are required
 *   tau_limit          [nv] (device), nullable
 *   q_out, qd_out      [num_envs][K][T][nv], row t the state AFTER step t + 1, as dg_world_rollout's
 *   tau_out            [num_envs][K][T][nv], row t the torque applied in step t, after clamping
 *   pos_out, singular  [num_envs][K][T][3], [num_envs][K] int32; frame, local_pos, joint_damping: as dg_world_rollout's
 * An absent term is absent, not zero: a call without dtau, gain and tau_limit gives dg_world_rollout's bits for tau_ff repeated over
 * K.  Each product of the torque is rounded on its own (tau_ff + alpha dtau is what fp32 arithmetic outside gives).  Each output may
 * be NULL, at least one must not be.  DG_ERR_ARG (nothing launched, outputs untouched) for everything dg_world_rollout refuses (tau_ff
 * in tau's place), dtau without alpha, gain without both references, and num_envs x T x nv x 2 nv beyond INT64_MAX / 4. */
int32_t dg_world_rollout_feedback(dg_world* w, const float* state, int32_t body, int32_t frame, const float* local_pos, int32_t K, int32_t T,
                                  float dt, int32_t joint_damping, const float* q0, const float* qd0, const float* tau_ff, const float* dtau,
                                  const float* alpha, const float* gain, const float* q_ref, const float* qd_ref, const float* tau_limit,
                                  float* q_out, float* qd_out, float* tau_out, float* pos_out, int32_t* singular, void* stream);

/* The Riccati / iLQR backward pass of the joint-space model of `body` (nv <= 12 joints, m = 2 nv states [dq; qd]), every env in ONE
 * launch.  It reads nothing of the scene but nv and takes the CONTINUOUS derivatives as dg_world_dynamics_derivatives returns them;
 * A_t, B_t are formed inside, in float64, over `substeps` substeps of dt with the torque held, the step's semi-implicit order:
 *   A_h = [[I + dt^2 A_q, dt (I + dt A_v)], [dt A_q, I + dt A_v]], B_h = [[dt^2 Minv], [dt Minv]], A = A_h^s, B = sum_{k<s} A_h^k B_h.
 * From Vx = lx_T, Vxx = lxx_T, for t = T-1 .. 0:
 *   Qx = lx + A^T Vx;  Qu = lu + B^T Vx;  Qxx = lxx + A^T Vxx A;  Qux = B^T Vxx A;  Quu = luu + B^T Vxx B
 *   k = -(Quu + mu I)^-1 Qu;  K = -(Quu + mu I)^-1 Qux     (Cholesky; a pivot <= 0 or not finite is a failure)
 *   dV += (k . Qu, 0.5 k^T Quu k)
 *   Vx = Qx + K^T Quu k + K^T Qu + Qux^T k;  Vxx = sym(Qxx + K^T Quu K + K^T Qux + Qux^T K)      (the unregularised Quu)
 * so the control update is du = alpha k + K dx, and the gain of a stationary LQR is -K_out[:, 0] with lx = lu = 0.  Computed in
 * float64, read and written as float32, all device arrays:
 *   A_q, A_v, Minv   [num_envs][P][nv][nv], P == T or P == 1 (the one point at every t)
 *   lxx, luu         [num_envs][PC][m][m], [num_envs][PC][nv][nv], PC == T or 1; lx [..][m], lu [..][nv], nullable = zero; no lux term
 *   lxx_T, lx_T      [num_envs][m][m], [num_envs][m] (nullable = zero)
 *   mu               [num_envs], nullable = 0
 *   K_out, k_out, dV [num_envs][T][nv][m], [num_envs][T][nv], [num_envs][2], each nullable
 *   status           [num_envs] int32, required: 0, or t + 1 of the first step whose factorisation failed; that env's K_out, k_out and
 *                    dV are then all zeros (raise mu and call again).  Nothing is left non-finite or unwritten.
 * DG_ERR_ARG (nothing launched, outputs untouched) for a NULL world, a body out of range, without joints or with more than 12,
 * T < 1, P or PC not in {1, T}, substeps < 1, a dt that is not finite or <= 0, a missing required array, and
 * num_envs x T x m x m beyond INT64_MAX / 4. */
int32_t dg_world_lq_backward(dg_world* w, int32_t body, int32_t T, int32_t P, int32_t PC, int32_t substeps, double dt,
                             const float* A_q, const float* A_v, const float* Minv, const float* lxx, const float* luu, const float* lx,
                             const float* lu, const float* lxx_T, const float* lx_T, const float* mu,
                             float* K_out, float* k_out, float* dV, int32_t* status, void* stream);

/* Per-env diagnostics of the last step: diag[num_envs][DG_DIAG_STRIDE] (int32), columns DG_DIAG_*: contact count and
 * Gauss-Seidel iterations of the final substep, the same two of the first substep, and the iterations each of the
 * scene's first DG_DIAG_N_IK inverse-kinematics ops ran for that env.  Optional; pass NULL to disable (default).  The
 * buffer must stay valid until changed. */
enum { DG_DIAG_CONTACTS = 0, DG_DIAG_PGS_ITERS = 1, DG_DIAG_PGS_ITERS_FIRST = 2, DG_DIAG_CONTACTS_FIRST = 3, DG_DIAG_IK_ITERS = 4,
       DG_DIAG_N_IK = 4, DG_DIAG_STRIDE = 8 };
int32_t dg_world_set_diag_buffer(dg_world* w, int32_t* diag);

/* Skip counter: skipped[num_envs] (int32, device memory) receives with every step, per env, how many of the step's substeps ran
 * without a narrow phase and the pose pass in front of it because the clearance the previous narrow phase measured exceeded what
 * the arms could have moved since (plan[DG_PLAN_NP_SKIP]; the decision is the workgroup's, so the 64 envs of a workgroup report
 * the same number).  Written by the four-wavefront step kernel only (0 where plan[DG_PLAN_NP_SKIP] is 0).  Optional; pass NULL to disable (default).  The buffer must stay
 * valid until changed. */
int32_t dg_world_set_skip_counter(dg_world* w, int32_t* skipped);

/* Diagnostic build of the step kernel with in-kernel cycle stamps (s_memtime): when `cycles` is
 * non-NULL, dg_world_step launches the stamped instantiation and lane 0 of every wavefront writes
 * cycles[workgroup][24]: entries 0..11 = shader cycles the (main) wavefront spent in {update ops (IK), kinematics, narrow phase, ABA passes,
 * M^-1 columns, row setup, PGS (rest), position update, output ops, PGS motor rows, PGS limit rows, PGS contact rows}; entries 12..23 (helper-wave kernel only) = cycles after which wavefronts
 * 1, 2, 3 reached {pose hand-over, end of the update phase, final hand-over, their end}.  Never used for timing quotes: the
 * stamps serialise the instruction stream.  Pass NULL (default) for the production kernel. */
int32_t dg_world_set_profile_buffer(dg_world* w, uint64_t* cycles);

/* Diagnostic, no device needed (the library loads and this call works on a machine without a GPU): what dg_world_create
 * would decide for `num_envs` copies of the scene blob on a GPU of `cu_count` compute units, under the environment's DG_*
 * switches -- the same planner, nothing allocated.  plan[DG_PLAN_COUNT] receives the decisions: workspace mode (as dims[7]),
 * LDS bytes per workgroup, helper-wave kernel, manifold kernels; the LDS plan in slots per env (total, transient region,
 * contact lists, widest body, total DoF, dense rows, contact row tail, base block of the transient region); the kernel form
 * (helper body, register-row bodies, narrow-phase wavefronts, split sweeps, early dynamics); floats of the global workspace and
 * of the hull polytope workspace (0 = not allocated; clamped to INT32_MAX); 1 + last body that is not frozen, 1 + last shape
 * that is not a box; word offsets of the device-only tables.  `table` (nullable, `table_cap` words) receives the first
 * plan[DG_PLAN_TABLE_WORDS] words of the plan table:
 *   per body [DG_PLAN_PLB_STRIDE]: slot of the base rotation (-1: frozen), of M^-1 (nv x nv), of the velocity change (nv), nv,
 *                                  1 for a fixed-base serial chain of <= 6 joints;
 *   per link [DG_PLAN_PLL_STRIDE]: slot of the pose (9), of the motor / limit rows (6), of the inertia accumulator (21, inside
 *                                  the transient region) or -1;
 *   then at DG_PLAN_PD_OFF / GD_OFF / SD_OFF / AM_OFF the pair, group and shape descriptors and the ancestor masks, and at
 *   DG_PLAN_RH_OFF one float per link: rho, the reach behind the joint that bounds how far a joint increment moves the chain
 *   (zero for bodies that are not fixed-base serial chains).  DG_PLAN_NP_SKIP: later substeps may skip their narrow phase. */
enum { DG_PLAN_LANES = 0, DG_PLAN_LDS_BYTES, DG_PLAN_PAR, DG_PLAN_MF, DG_PLAN_TOTAL_SLOTS, DG_PLAN_TR_OFF, DG_PLAN_TR_SLOTS, DG_PLAN_CONT_OFF,
       DG_PLAN_CONT2_OFF, DG_PLAN_NV_MAX, DG_PLAN_NT, DG_PLAN_DENSE, DG_PLAN_CROW_TAIL, DG_PLAN_AB_STRIDE, DG_PLAN_HELPER_BODY, DG_PLAN_REG_BODY0,
       DG_PLAN_REG_BODY1, DG_PLAN_COLL_WAVE, DG_PLAN_COLL_SPLIT, DG_PLAN_SPLIT_PGS, DG_PLAN_EARLY_DYN, DG_PLAN_GWS_FLOATS, DG_PLAN_HULL_WS_FLOATS,
       DG_PLAN_NBA, DG_PLAN_NSHA, DG_PLAN_PD_OFF, DG_PLAN_GD_OFF, DG_PLAN_SD_OFF, DG_PLAN_AM_OFF, DG_PLAN_TABLE_WORDS, DG_PLAN_NP_SKIP,
       DG_PLAN_RH_OFF, DG_PLAN_COUNT };
enum { DG_PLAN_PLB_STRIDE = 5, DG_PLAN_PLL_STRIDE = 3 };
int32_t dg_debug_plan(const int32_t* idata, int64_t n_i, const double* fdata, int64_t n_f, int32_t num_envs, int32_t cu_count,
                      int32_t* plan, int32_t* table, int64_t table_cap);

#ifdef __cplusplus
}
#endif
#endif
