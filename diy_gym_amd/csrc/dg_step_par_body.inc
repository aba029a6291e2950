// dg_step_par_body.inc -- body of the four-wavefront step kernel, included twice by dg_entry.h: as step_kernel_par<PROF>
// (DG_PAR_RESET 0) and as reset_kernel_par (DG_PAR_RESET 1: reset ops + the one hot-start step).  Textual inclusion, not
// a shared device function: routing the kernel's by-value scene through a function cost the step kernel 7 % (0.116 ->
// 0.124 ms, measured), and a run-time mode flag in the step kernel cost the same.
// Expects in scope: sc, mt, state, actions, mask, obs, rew, term, rew_sum, term_flag, diag, cycles, reset_mask, PROF.
  constexpr int reset_mode = DG_PAR_RESET;
  extern __shared__ float smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int env = blockIdx.x * 64 + lane; const bool exists = env < sc.num_envs; const int e = exists ? env : sc.num_envs - 1;
  // reset_mode (dg_world_reset of a scene with one hot-start step): the main wave runs the reset ops of the envs named by the
  // mask, then the four wavefronts run ONE step without update ops -- the hot-start step -- in which only those envs
  // store anything (`valid`); a workgroup without such an env leaves at once.  Every wavefront sees the same 64 envs, so
  // the exit and the extra barrier Br below are taken by all four or by none.
  const bool doit = exists && (!reset_mode || reset_mask == nullptr || reset_mask[e] != 0);
  if (reset_mode && !__any(doit)) return;
  const bool valid = reset_mode ? doit : exists;
  const float* act_row = actions ? actions + (size_t)e * sc.act_dim : nullptr;
  const unsigned long long t_start = PROF ? __builtin_amdgcn_s_memtime() : 0ull; (void)t_start;
  // ---- The opening pose pass and B0 ----------------------------------------------------------------------------------------
  // pose_ho (sc.early_dyn && sc.coll_split: wavefronts 2 and 3 both work during the update phase, an inverse-kinematics op exists,
  // every moving body is a register chain, no update op reads a link pose; DG_NO_EARLY_DYNAMICS=1 / DG_NO_COLLIDE_SPLIT=1 switch it
  // off): the two wavefronts that CONSUME the opening poses compute them -- wavefront 2 sc.reg_body[0]'s, wavefront 3
  // sc.helper_body's, instead of idling at B0 -- and the two inverse-kinematics wavefronts start their solve at once and pass B0
  // from inside it (Handover, dg_solver.h).  The base rotation (PLB_R0) of those two bodies is the one thing the solve reads from
  // LDS: the wavefront that runs the solve stores it itself (base_rot_to_lds, before the solve in program order: no barrier
  // needed), wavefronts 2 / 3 leave it alone (kinematics(.., base_rot = false)) and first read it behind B0 (dynamics_chain).  So
  // between kernel start and B0 every LDS slot has one writer: PLB_R0 of both arms and every pose of any other body the main wave
  // (the helper: its arm's PLB_R0), the link poses of the two arms wavefronts 2 / 3.
  // Barriers each wavefront executes, in order (k = 0 .. substeps-1; Bs only in a substep with a contact that splits its sweeps):
  //     [Br]  B0  B0'  { B1  B2  [Bs]  B3 } x substeps  B4
  // Wavefronts 2 / 3 execute B0 in this file on every path.  Wavefronts 0 / 1 execute it through `b0`, once, here:
  //   step with actions, packed IK (ur_high_5)    inside run_ik_chain_pk, between its set-up and its first forward kinematics
  //   DG_NO_FULL_IK=1                             the same place in run_ik_chain<6>
  //   a wavefront with no valid lane              the same place: it precedes the iteration loop, whose exits (no live lane at
  //                                               it == 0, every lane converged, sc.ik_iters) therefore do not matter
  //   the op's slot masked out by `mask`          behind run_update_ops below (no register-chain solve ran on this wavefront)
  //   actions == nullptr                          the same call below; run_update_ops is not entered
  //   a body under joint_controller               in a pose_ho scene: as for a masked-out op.  ur_high_5_joint has no IK op at all:
  //                                               early_dyn == 0, pose_ho == 0, the plain order (own pose pass, then B0, in this file)
  //   reset_kernel_par                            no env of the workgroup named: every wavefront returns before any barrier (above).
  //                                               Otherwise Br first (all four), then the hot-start step, which has no actions:
  //                                               the call below
  //   !pose_ho (any other scene or switch)        the plain order: the wavefront's own pose pass, then `b0` at once
  // `b0` is idempotent, so "again behind" never adds a barrier; see Handover for why its flag is wave-uniform.
  // sc.np_skip (substep_np_skip, dg_solver.h): every narrow-phase call below keeps its clearance and the wavefront stores it in its own
  // slot; at the top of a substep k >= 1 all four wavefronts read the same slots and decide alike whether the substep goes without
  // narrow phase and pose pass.  The barriers of a skipped substep are those of any other: B1, B2, B3.
  const int clr_slot = split_slots(sc) + NPS_CLEAR;
  const bool pose_ho = sc.early_dyn && sc.coll_split;
  if (wave == 3) {  // ---------------- second half of the narrow phase; in the early first substep, the dynamics of every second moving body
    Lane<64> ln(sc, mt, smem + lane, state + e, e, valid);
    if (reset_mode) __syncthreads();  // Br: the reset ops have written the state
    if (pose_ho) ln.kinematics(sc.helper_body, -1, false);  // the opening poses of the helper's arm (PLB_R0: the helper)
    DG_WAVE_STAMP(0); __syncthreads();  // B0
    if (sc.early_dyn) {  // (round 4: and the second half of the early narrow phase -- the third wavefront alone was 100 k cycles against the update ops' 91 k)
      early_dynamics(ln, 1);
      if (sc.coll_split) { float clr; collide<64, 64, 1, true>(ln, sc.npairs / 2, 0x7fffffff, sc.cont2_off, 0, &clr); ln.L(clr_slot + 1) = clr; }
    }
    DG_WAVE_STAMP(1); __syncthreads();  // B0'
    bool fused = false;
    for (int k = 0; k < sc.substeps; k++) {
      const bool skip = substep_np_skip(ln, fused);
      __syncthreads();  // B1
      if (skip) np_skip_follow(ln, 1, sc.cont2_off);
      else if (sc.coll_split && !(sc.early_dyn && k == 0)) { float clr; collide<64, 64, 1, true>(ln, sc.npairs / 2, 0x7fffffff, sc.cont2_off, 0, &clr); ln.L(clr_slot + 1) = clr; }  // (k == 0 with early_dyn: done above)
      __syncthreads();  // B2
      // (a substep without a contact in the workgroup has neither Bq nor Bs: the first two wavefronts run fused_free_halves)
      fused = substep_contact_free(ln);
      if (!fused && split_decide_follow(ln, 0u, false)) __syncthreads();  // Bs: the sweeps run on the first two wavefronts
      __syncthreads();  // B3
    }
    DG_WAVE_STAMP(2); __syncthreads();  // B4: every final pose is in LDS, every state row written
    run_output_ops(ln, nullptr, (valid && rew) ? rew + (size_t)e * sc.rew_dim : nullptr, (valid && term) ? term + (size_t)e * sc.term_dim : nullptr,
                   (valid && rew_sum) ? rew_sum + e : nullptr, (valid && term_flag) ? term_flag + e : nullptr, OUT_REW_TERM);
    DG_WAVE_STAMP(3);
    return;
  }
  if (wave == 2) {  // ---------------- narrow phase, concurrently with the two arms' dynamics (between B1 and B2)
    Lane<64> ln(sc, mt, smem + lane, state + e, e, valid);
    if (reset_mode) __syncthreads();  // Br
    if (pose_ho) ln.kinematics(sc.reg_body[0], -1, false);  // the opening poses of the main wave's arm (PLB_R0: the main wave)
    DG_WAVE_STAMP(0); __syncthreads();  // B0
    if (sc.early_dyn) {  // first substep: narrow phase and the arms' dynamics while the first two waves run the update ops
      { float clr; collide<64, 64, 1, true>(ln, 0, sc.coll_split ? sc.npairs / 2 : 0x7fffffff, -1, 0, &clr); ln.L(clr_slot) = clr; }  // (the fourth wavefront takes every second moving body's dynamics and the other half of the pair table)
      early_dynamics(ln, 0);
    }
    DG_WAVE_STAMP(1); __syncthreads();  // B0'
    bool fused = false;
    for (int k = 0; k < sc.substeps; k++) {
      const bool skip = substep_np_skip(ln, fused);
      __syncthreads();  // B1: every pose is in LDS
      if (skip) np_skip_follow(ln, 0, sc.cont_off);
      else if (sc.coll_wave && !(sc.early_dyn && k == 0)) { float clr; collide<64, 64, 1, true>(ln, 0, sc.coll_split ? sc.npairs / 2 : 0x7fffffff, -1, 0, &clr); ln.L(clr_slot) = clr; }  // contact list + count go to LDS; the main wave reads them after B2
      __syncthreads();  // B2
      fused = substep_contact_free(ln);
      if (!fused && split_decide_follow(ln, false, false)) __syncthreads();  // Bs
      __syncthreads();  // B3
    }
    DG_WAVE_STAMP(2); __syncthreads();  // B4
    run_output_ops(ln, (valid && obs) ? obs + (size_t)e * sc.obs_dim : nullptr, nullptr, nullptr, nullptr, nullptr, OUT_OBS_REST);
    DG_WAVE_STAMP(3);
    return;
  }
  if (wave == 1) {  // ---------------- helper
    Lane<64> ln(sc, mt, smem + lane, state + e, e, valid);
    if (reset_mode) __syncthreads();  // Br
    Handover b0([&]() { DG_WAVE_STAMP(0); __syncthreads(); }, false);  // B0: every pose is in LDS
    if (pose_ho) ln.base_rot_to_lds(sc.helper_body); else { ln.kinematics(sc.helper_body); b0(); }
    if (act_row) run_update_ops(ln, act_row, mask, sc.helper_body, -1, diag, b0);
    b0();  // (no register-chain inverse-kinematics op ran)
    DG_WAVE_STAMP(1); __syncthreads();  // B0'
    bool fused = false;
    for (int k = 0; k < sc.substeps; k++) { const bool skip = substep_np_skip(ln, fused); fused = helper_substep(ln, sc.early_dyn && k == 0, k == sc.substeps - 1, skip); }
    ln.kinematics(sc.helper_body);  // final pose of its body for the outputs
    DG_WAVE_STAMP(2); __syncthreads();  // B4
    // its arm's joint-state observations (state reads only; the main wave skips them)
    run_output_ops(ln, (valid && obs) ? obs + (size_t)e * sc.obs_dim : nullptr, nullptr, nullptr, nullptr, nullptr, OUT_JOINT_OF, sc.helper_body);
    DG_WAVE_STAMP(3);
    return;
  }
  Lane<64> ln(sc, mt, smem + lane, state + e, e, valid);
  Prof<PROF> prof; prof.start();
  if (reset_mode) { if (doit) { ln.Sset(DG_ST_STEP, 0.0f); run_reset_ops(ln); } __syncthreads(); }  // Br
  Handover b0([&]() { __syncthreads(); }, false);  // B0
  for (int b = 0; b < sc.nba; b++) if (b != sc.helper_body) { if (pose_ho && b == sc.reg_body[0]) ln.base_rot_to_lds(b); else ln.kinematics(b); }
  if (!pose_ho) b0();
  prof.stamp(PS_KIN);  // (pose_ho: B0 and whatever wait it holds count as PS_UPDATE; PS_KIN is the closing pose pass alone)
  if (act_row) run_update_ops(ln, act_row, mask, -1, sc.helper_body, diag, b0);
  b0();  // (no register-chain inverse-kinematics op ran)
  if (!reset_mode) ln.Sset(DG_ST_STEP, ln.S(DG_ST_STEP) + 1.0f);
  __syncthreads();  // B0': the helper's motor targets are in the state
  prof.stamp(PS_UPDATE);
  sim_step<64, PROF, true>(ln, diag, prof);
  for (int b = 0; b < sc.nba; b++) if (b != sc.helper_body) ln.kinematics(b);
  __syncthreads();  // B4: the helper's body too
  prof.stamp(PS_KIN);
  // the output phase is shared: this wave emits the joint states of its bodies, the helper its arm's, the third
  // wavefront the other observe ops, the fourth the reward / terminal ops and the collapsed outputs
  run_output_ops(ln, (valid && obs) ? obs + (size_t)e * sc.obs_dim : nullptr, nullptr, nullptr, nullptr, nullptr, OUT_JOINT_NOT_OF, sc.helper_body);
  prof.stamp(PS_OUTPUT);
  if constexpr (PROF) { if (lane == 0) for (int k = 0; k < PS_COUNT; k++) cycles[(size_t)blockIdx.x * PS_ROW + k] = prof.acc[k]; }
