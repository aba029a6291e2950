// dg_plan.hip -- the planner of dg_plan.h: host code only (compiled as HIP because DevScene's pointers are typed in the
// constant address space); no kernel lives here.
#include "dg_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dg_solver.h"  // SC_STRIDE, HH_WS_SLOTS, DG_IK_DEV_*

namespace dg {

PlanSwitches plan_switches_from_env() {
  PlanSwitches s;
#define X(name, field, doc) if (const char* v = getenv(#name)) { s.field.set = true; s.field.value = atoi(v); }
  DG_PLAN_SWITCHES(X)
#undef X
  if (const char* v = getenv("DG_NO_NP_SKIP")) { s.no_np_skip.set = true; s.no_np_skip.value = atoi(v); }  // (beside the table: dg_plan.h)
  return s;
}

namespace {

const int LDS_MAX = 160 * 1024;  // bytes of LDS a workgroup of gfx950 may use

// Bounds of the blob's tables against the array lengths the caller passed: a malformed blob must fail here, not read
// out of bounds on the host or the device.
const char* check_blob(const int32_t* I, int64_t n_i, int64_t n_f) {
  struct T { int off, count_idx, stride; bool is_f; const char* name; };
  const T tables[] = {
    {DG_H_OFF_BODY_I, DG_H_N_BODIES, DG_BI_STRIDE, false, "body ints"}, {DG_H_OFF_LINK_I, DG_H_N_LINKS, DG_LI_STRIDE, false, "link ints"},
    {DG_H_OFF_FRAME_I, DG_H_N_FRAMES, DG_FI_STRIDE, false, "frame ints"}, {DG_H_OFF_SHAPE_I, DG_H_N_SHAPES, DG_SI_STRIDE, false, "shape ints"},
    {DG_H_OFF_PAIR_I, DG_H_N_PAIRS, DG_PI_STRIDE, false, "pairs"}, {DG_H_OFF_GROUP_I, DG_H_N_GROUPS, DG_GI_STRIDE, false, "pair groups"},
    {DG_H_OFF_CAMERA_I, DG_H_N_CAMERAS, DG_CI_STRIDE, false, "camera ints"}, {DG_H_OFF_OP_I, DG_H_N_OPS, DG_OI_STRIDE, false, "op ints"},
    {DG_H_OFF_ILIST, DG_H_N_ILIST, 1, false, "int list"},
    {DG_H_OFF_BODY_F, DG_H_N_BODIES, DG_BF_STRIDE, true, "body floats"}, {DG_H_OFF_LINK_F, DG_H_N_LINKS, DG_LF_STRIDE, true, "link floats"},
    {DG_H_OFF_FRAME_F, DG_H_N_FRAMES, DG_FF_STRIDE, true, "frame floats"}, {DG_H_OFF_SHAPE_F, DG_H_N_SHAPES, DG_SF_STRIDE, true, "shape floats"},
    {DG_H_OFF_POINT_F, DG_H_N_POINTS, 3, true, "hull points"}, {DG_H_OFF_PLANE_F, DG_H_N_PLANES, 4, true, "hull planes"},
    {DG_H_OFF_CAMERA_F, DG_H_N_CAMERAS, DG_CF_STRIDE, true, "camera floats"}, {DG_H_OFF_OP_F, DG_H_N_OPS, DG_OF_STRIDE, true, "op floats"},
    {DG_H_OFF_FLIST, DG_H_N_FLIST, 1, true, "float list"},
    {DG_H_OFF_CONS_I, DG_H_N_CONSTRAINTS, DG_KI_STRIDE, false, "constraint ints"}, {DG_H_OFF_CONS_F, DG_H_N_CONSTRAINTS, DG_KF_STRIDE, true, "constraint floats"}};
  for (const T& t : tables) {
    const int64_t off = I[t.off], cnt = I[t.count_idx], lim = t.is_f ? n_f : n_i;
    if (cnt < 0 || off < (t.is_f ? DG_HF_FLOAT_COUNT : DG_H_INT_COUNT) || off + cnt * t.stride > lim) return t.name;
  }
  return nullptr;
}

// ---- facts about a body (B: its DG_BI_* row) that several rules share
bool is_fixed(const int32_t* B) { return (B[DG_BI_FLAGS] & DG_BODY_FIXED) != 0; }
// neither a base that moves nor a joint
bool is_static(const int32_t* B) { return is_fixed(B) && B[DG_BI_N_LINKS] == 0; }
// 1 .. max_joints joints, each the child of the one before it (LI: the scene's DG_LI_* table)
bool is_serial_chain(const int32_t* B, const int32_t* LI, int max_joints) {
  const int first = B[DG_BI_FIRST_LINK], n = B[DG_BI_N_LINKS];
  bool chain = n >= 1 && n <= max_joints;
  for (int i = 0; i < n && chain; i++) chain = LI[(first + i) * DG_LI_STRIDE + DG_LI_PARENT] == (i == 0 ? -1 : first + i - 1);
  return chain;
}
// a fixed base with at most six joints: its solver rows may live in registers (by length alone -- the chain order is
// PLB_CHAIN's business)
bool has_reg_rows(const int32_t* B) { return is_fixed(B) && B[DG_BI_N_LINKS] >= 1 && B[DG_BI_N_LINKS] <= 6; }
// some candidate pair tests two convex hulls against each other
bool has_hull_pairs(const int32_t* I) {
  const int32_t* PIh = I + I[DG_H_OFF_PAIR_I]; const int32_t* SIh = I + I[DG_H_OFF_SHAPE_I];
  for (int p = 0; p < I[DG_H_N_PAIRS]; p++)
    if (SIh[PIh[p * DG_PI_STRIDE + DG_PI_A] * DG_SI_STRIDE + DG_SI_TYPE] == DG_SHAPE_POINTS && SIh[PIh[p * DG_PI_STRIDE + DG_PI_B] * DG_SI_STRIDE + DG_SI_TYPE] == DG_SHAPE_POINTS) return true;
  return false;
}

// The workspace mode (envs per wavefront; 0 / -16: global workspace) of a scene that needs `total` slots per env.
// sliceable: all-dense scenes (every row indexed by global DoF, no register-chain body) can put spare lanes to work in the
// Gauss-Seidel sweeps, so for them 8 and 4 envs per wavefront are worth having; other scenes stop at 16
int choose_lanes(const PlanSwitches& sw, bool sliceable, int nt, int nl, int maxc, int total, int num_envs, int cu_count) {
  int lanes = 64;
  if (sw.max_lanes) { const int v = sw.max_lanes.value; if (v == 32 || v == 16 || v == 8 || v == 4 || v == 1) lanes = v; }
  int min_lanes = (sliceable && !sw.no_narrow_modes) ? 4 : 16;
  // One env per wavefront: a scene whose rows do not fit the register budget of the 4-envs-per-wavefront sweeps (more than
  // 16 links, or a contact budget above 12) at a batch that gives every SIMD at most one such wavefront -- every row of the
  // scene then sits in registers (pgs_wave_env) and four times as many SIMDs work.  (from_the_readme at 1 024 envs: 5.6 -> 3.8 ms.)
  if (sliceable && lanes > 1 && !sw.max_lanes && !sw.no_narrow_modes && !sw.no_wave_env && nt <= 32 && nl <= 32 && maxc <= 32 && (nl > 16 || maxc > 12) && total * 4 <= LDS_MAX) {
    if (num_envs <= 4 * cu_count) lanes = 1;
  }
  if (lanes == 1 && !(sliceable && nt <= 32 && nl <= 32 && maxc <= 32)) lanes = 4;  // (DG_MAX_LANES=1 on a scene the mode does not hold)
  if (sliceable && lanes == 1) min_lanes = 1;  // (asked for with DG_MAX_LANES=1, or picked above)
  while (lanes >= min_lanes && total * lanes * 4 > LDS_MAX) lanes >>= 1;
  // Latency: a big batch of a sliceable scene that still leaves SIMDs without a wavefront (fewer than FOUR one-wavefront
  // workgroups per CU) is cut into smaller workgroups -- the sweeps get more lanes per env, the rest loses nothing, and a scene
  // whose workspace lets only one or two workgroups of 32 envs share a CU's LDS gets three to eight of 16.  (Round 4: the target
  // was two per CU; at 16 384 envs one wavefront on EVERY SIMD measured drone_pilot 0.195 -> 0.168 ms per step and the 12-joint
  // UR5 + gripper tree 1.16 -> 0.84, marbles unchanged; two per SIMD -- 8 envs per wavefront -- is slower again for drone_pilot:
  // profiles/r4_workspace_modes_16384.txt.)
  if (sliceable && lanes >= min_lanes && num_envs >= 2048 && !sw.max_lanes && !sw.no_narrow_modes) {
    while (lanes > 8 && (num_envs + lanes - 1) / lanes < 4 * cu_count) lanes >>= 1;
  }
  if (lanes >= min_lanes) return lanes;
  // too big for LDS even at 16 envs per wavefront: per-env scratch moves to a global buffer
  // [workgroup][slot][lane] (coalesced, L2-resident); same kernels, Lane<0>.
  // all-dense scenes run 16 envs per wavefront instead, so that the other 48 lanes can share each env's solver rows; LDS
  // then only holds the accumulated impulses of those rows
  const int acc_rows = 3 * maxc + 3 * nl;
  return (sliceable && acc_rows * 16 * 4 <= 64 * 1024 && !sw.no_sliced_global) ? -16 : 0;
}

int fail(WorldPlan& out, int code, const char* fmt, ...) {
  char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  out.error = buf; return code;
}

}  // namespace

int plan_world(const int32_t* I, int64_t n_i, const double* F, int64_t n_f, int num_envs, int env_stride, int cu_count, uint64_t seed,
               int64_t env_index_base, const PlanSwitches& sw, WorldPlan& out) {
  if (!I || !F || n_i < DG_H_INT_COUNT) return fail(out, DG_ERR_ARG, "null or short scene arrays");
  if (I[DG_H_MAGIC] != DG_MAGIC || I[DG_H_VERSION] != DG_VERSION) return fail(out, DG_ERR_BAD_SCENE, "bad scene magic/version (%x, %d)", I[DG_H_MAGIC], I[DG_H_VERSION]);
  if (num_envs <= 0 || env_stride < num_envs) return fail(out, DG_ERR_ARG, "num_envs=%d env_stride=%d", num_envs, env_stride);
  const int nb = I[DG_H_N_BODIES], nl = I[DG_H_N_LINKS];
  if (nl > DG_MAX_LINKS) return fail(out, DG_ERR_UNSUPPORTED, "%d links > %d supported", nl, DG_MAX_LINKS);
  if (nb > DG_MAX_BODIES) return fail(out, DG_ERR_UNSUPPORTED, "%d bodies > %d supported", nb, DG_MAX_BODIES);
  if (n_f < DG_HF_FLOAT_COUNT) return fail(out, DG_ERR_BAD_SCENE, "float array shorter than its header");
  if (const char* bad = check_blob(I, n_i, n_f)) return fail(out, DG_ERR_BAD_SCENE, "scene table '%s' does not fit the arrays passed (n_i=%lld, n_f=%lld)", bad, (long long)n_i, (long long)n_f);
  if (I[DG_H_N_SHAPES] > 4096) return fail(out, DG_ERR_UNSUPPORTED, "%d shapes > 4096 supported", I[DG_H_N_SHAPES]);
  if (I[DG_H_N_CONSTRAINTS] > DG_MAX_CONSTRAINTS) return fail(out, DG_ERR_UNSUPPORTED, "%d fixed constraints > %d supported", I[DG_H_N_CONSTRAINTS], DG_MAX_CONSTRAINTS);
  for (int q = 0; q < I[DG_H_N_CONSTRAINTS]; q++) {
    const int32_t* ki = I + I[DG_H_OFF_CONS_I] + q * DG_KI_STRIDE;
    for (int k = 0; k < 2; k++) {
      const int b = ki[k == 0 ? DG_KI_BODY_A : DG_KI_BODY_B], gl = ki[k == 0 ? DG_KI_LINK_A : DG_KI_LINK_B];
      if (b < 0 || b >= nb) return fail(out, DG_ERR_BAD_SCENE, "constraint %d: body %d out of range", q, b);
      const int32_t* B = I + I[DG_H_OFF_BODY_I] + b * DG_BI_STRIDE;
      if (gl >= 0 && (gl < B[DG_BI_FIRST_LINK] || gl >= B[DG_BI_FIRST_LINK] + B[DG_BI_N_LINKS])) return fail(out, DG_ERR_BAD_SCENE, "constraint %d: link %d is not a link of body %d", q, gl, b);
    }
  }
  if (I[DG_H_N_TERM_GROUPS] > 64) return fail(out, DG_ERR_UNSUPPORTED, "%d receptors with terminal addons > 64 supported", I[DG_H_N_TERM_GROUPS]);
  const int32_t* BI = I + I[DG_H_OFF_BODY_I]; const int32_t* LI = I + I[DG_H_OFF_LINK_I]; const int32_t* OI = I + I[DG_H_OFF_OP_I];
  const int32_t* PIh = I + I[DG_H_OFF_PAIR_I]; const int32_t* SIh = I + I[DG_H_OFF_SHAPE_I];
  const int npairs = I[DG_H_N_PAIRS], nops = I[DG_H_N_OPS];
  DevScene& sc = out.sc; memset(&sc, 0, sizeof sc);
  // ---- LDS plan (slots per lane)
  std::vector<int32_t>& plan = out.table;
  plan.assign((size_t)nb * PLB_STRIDE + (size_t)nl * PLL_STRIDE, 0);
  plan.reserve(plan.size() + (size_t)npairs + 4 * (size_t)I[DG_H_N_GROUPS] + 1);  // pair descriptors are appended below; PLB / PLL must stay valid
  int32_t* PLB = plan.data(); int32_t* PLL = plan.data() + (size_t)nb * PLB_STRIDE;
  int slot = 0, nvmax = 0; bool any_float = false;
  for (int b = 0; b < nb; b++) {
    const int32_t* B = BI + b * DG_BI_STRIDE; const bool fx = is_fixed(B);
    const int nv = (fx ? 0 : 6) + B[DG_BI_N_LINKS];
    if (!fx) any_float = true;
    if (B[DG_BI_FLAGS] & DG_BODY_FROZEN) PLB[b * PLB_STRIDE + PLB_R0] = -1; else { PLB[b * PLB_STRIDE + PLB_R0] = slot; slot += 6; }
    PLB[b * PLB_STRIDE + PLB_MINV] = slot; slot += nv * nv;
    PLB[b * PLB_STRIDE + PLB_NV] = nv;
    PLB[b * PLB_STRIDE + PLB_CHAIN] = (fx && is_serial_chain(B, LI, 6)) ? 1 : 0;
    nvmax = std::max(nvmax, nv);
  }
  // velocity-change blocks of all bodies back to back, then nv_max slots of padding (branch-free contact sweeps)
  for (int b = 0; b < nb; b++) { PLB[b * PLB_STRIDE + PLB_DV] = slot; slot += PLB[b * PLB_STRIDE + PLB_NV]; }
  slot += nvmax + 8;  // chunked helpers read up to 7 slots past a vector
  for (int l = 0; l < nl; l++) { PLL[l * PLL_STRIDE + PLL_POSE] = slot; slot += 9; PLL[l * PLL_STRIDE + PLL_IAACC] = -1; }
  for (int l = 0; l < nl; l++) { PLL[l * PLL_STRIDE + PLL_MROW] = slot; slot += MR_STRIDE; }  // contiguous: pgs_rows_small strides through them
  const int maxc = I[DG_H_MAX_CONTACTS], ncons = I[DG_H_N_CONSTRAINTS];
  // (a fixed constraint keeps two pseudo contact slots behind the real ones: its linear and its angular rows, build_constraint_rows)
  const int cont_off = slot; slot += 1 + (maxc + 2 * ncons) * CL_STRIDE;
  const int ab_stride = any_float ? AB_FLOAT_STRIDE : AB_FIXED_STRIDE;
  // transient region: ABA workspace (+ inertia accumulators for links with a child that is not link+1),
  // contact rows, IK scratch -- never live at the same time
  const int tr_off = slot;
  int tr = 0;
  for (int b = 0; b < nb; b++) {
    const int32_t* B = BI + b * DG_BI_STRIDE; const int first = B[DG_BI_FIRST_LINK], n = B[DG_BI_N_LINKS];
    int need = ab_stride + n * AW_STRIDE;
    for (int i = 0; i < n; i++) {
      const int par = LI[(first + i) * DG_LI_STRIDE + DG_LI_PARENT];
      if (par >= 0 && par != first + i - 1 && PLL[par * PLL_STRIDE + PLL_IAACC] < 0) { PLL[par * PLL_STRIDE + PLL_IAACC] = tr_off + need; need += 21; }
    }
    tr = std::max(tr, need);
    if (n > 6) tr = std::max(tr, n * (n + 1) / 2 + 2 * n + 24);  // motor_guess_lds: packed factor + y + scaling, padded
  }
  // contact rows carry a second body's Jacobian / response only if some candidate pair has two moving bodies
  bool two_sided = ncons > 0;
  { auto moving = [&](int sh) { return !is_static(BI + SIh[sh * DG_SI_STRIDE + DG_SI_BODY] * DG_BI_STRIDE); };
    for (int p = 0; p < npairs; p++) if (moving(PIh[p * DG_PI_STRIDE + DG_PI_A]) && moving(PIh[p * DG_PI_STRIDE + DG_PI_B])) two_sided = true; }
  int nt = 0; for (int b = 0; b < nb; b++) nt += PLB[b * PLB_STRIDE + PLB_NV];
  const bool dense = nt <= 32 && ncons == 0;  // contact rows indexed by global DoF, swept with the velocity change in registers (fixed-constraint rows: generic sweeps only)
  const int crow_tail = dense ? 2 * nt : (two_sided ? 4 : 2) * nvmax;
  tr = std::max(tr, 3 * (maxc + 2 * ncons) * (crow_tail + 3));
  if (npairs > 0) tr = std::max(tr, (int)SC_STRIDE * I[DG_H_N_SHAPES]);  // narrow-phase shape cache
  for (int op = 0; op < nops; op++)
    if (OI[op * DG_OI_STRIDE + DG_OI_CODE] == DG_OP_IK_CONTROL) tr = std::max(tr, 9 * BI[OI[op * DG_OI_STRIDE + DG_OI_BODY] * DG_BI_STRIDE + DG_BI_N_LINKS]);
  slot += tr + 8;  // + padding for the chunked vector helpers
  const int total = slot;
  // bodies whose solver rows are held in registers by the step kernel
  sc.reg_body[0] = sc.reg_body[1] = -1;
  for (int b = 0, k = 0; b < nb && k < 2; b++) if (has_reg_rows(BI + b * DG_BI_STRIDE)) sc.reg_body[k++] = b;
  // ---- workspace mode
  const int lanes = choose_lanes(sw, dense && nt >= 1 && sc.reg_body[0] < 0, nt, nl, maxc, total, num_envs, std::max(cu_count, 1));
  const int per = envs_per_wave(lanes);
  if (lanes <= 0) out.gws_floats = (((size_t)num_envs + per - 1) / per) * (size_t)total * (size_t)per;  // [workgroup][slot][lane]
  out.lanes = lanes; out.lds_bytes = lanes > 0 ? total * lanes * 4 : (lanes < 0 ? (3 * maxc + 3 * nl) * 16 * 4 : 0);
  out.render_diag = (sw.render_no_cull ? 1 : 0) | sw.render_diag.value;
  if (sw.render_wpe) out.render_wpe = (sw.render_wpe.value == 3 || sw.render_wpe.value == 1) ? sw.render_wpe.value : 2;
  // ---- device tables (floats converted once)
  out.blob_f.resize((size_t)n_f); for (int64_t k = 0; k < n_f; k++) out.blob_f[(size_t)k] = (float)F[k];
  // device copy of the int tables, with device-only hints: IK ops on serial chains of <= 6 joints take the
  // register-resident solver
  out.blob_i.assign(I, I + n_i);
  for (int op = 0; op < nops; op++) {
    int32_t* oi = out.blob_i.data() + I[DG_H_OFF_OP_I] + op * DG_OI_STRIDE;
    if (oi[DG_OI_CODE] != DG_OP_IK_CONTROL) continue;
    const int32_t* B = BI + oi[DG_OI_BODY] * DG_BI_STRIDE; const int first = B[DG_BI_FIRST_LINK], n = B[DG_BI_N_LINKS];
    const bool chain = is_serial_chain(B, LI, 6);
    if (chain) oi[DG_OI_FLAGS] |= DG_IK_DEV_CHAIN;
    // six revolute joints with the end-effector frame on the last link: the fully specialised solve
    bool full = chain && n == 6 && I[I[DG_H_OFF_FRAME_I] + oi[DG_OI_FRAME] * DG_FI_STRIDE + DG_FI_LINK] == first + 5;
    for (int i = 0; i < n && full; i++) full = LI[(first + i) * DG_LI_STRIDE + DG_LI_TYPE] == 0;
    if (full && !sw.no_full_ik) oi[DG_OI_FLAGS] |= DG_IK_DEV_FULL;
  }
  // pair descriptors in canonical order (lower shape type first, a box always second), one word per pair
  out.pd_off = plan.size();
  for (int p = 0; p < npairs; p++) {
    const int sA = PIh[p * DG_PI_STRIDE + DG_PI_A], sB = PIh[p * DG_PI_STRIDE + DG_PI_B];
    const int tA = SIh[sA * DG_SI_STRIDE + DG_SI_TYPE], tB = SIh[sB * DG_SI_STRIDE + DG_SI_TYPE];
    const bool swap = tA == DG_SHAPE_BOX || (tB != DG_SHAPE_BOX && tA > tB);
    const int sa = swap ? sB : sA, sb = swap ? sA : sB, ta = swap ? tB : tA, tb = swap ? tA : tB;
    plan.push_back(sa | (sb << 12) | (ta << 24) | (tb << 26) | ((swap ? 1 : 0) << 28));
  }
  // group descriptors (broad phase), device-only: centre and reach of the group's static shape when that shape is frozen in
  // the world -- [x y z reach], reach = bound of the moving body + margin (+ hull margins) + extent of the shape; reach < 0: the narrow
  // phase works the group's bounds out from the tables (a moving partner)
  out.gd_off = plan.size();
  { const int32_t* GIh = I + I[DG_H_OFF_GROUP_I]; const double* SFh = F + I[DG_H_OFF_SHAPE_F]; const double* BFh = F + I[DG_H_OFF_BODY_F];
    for (int g = 0; g < I[DG_H_N_GROUPS]; g++) {
      const int32_t* gi = GIh + g * DG_GI_STRIDE; const int ss = gi[DG_GI_STATIC_SHAPE]; float d[4] = {0.f, 0.f, 0.f, -1.f};
      if (ss >= 0 && (SIh[ss * DG_SI_STRIDE + DG_SI_FLAGS] & DG_SHAPE_WORLD)) {
        const double* sf = SFh + ss * DG_SF_STRIDE; const int st = SIh[ss * DG_SI_STRIDE + DG_SI_TYPE];
        const float p0 = (float)sf[DG_SF_PARAMS], p1 = (float)sf[DG_SF_PARAMS + 1], p2 = (float)sf[DG_SF_PARAMS + 2];
        // (a hull: p2 = the radius around the fitted capsule's centre that holds its points; r + half alone lets points near the caps stick out)
        const float ext = st == DG_SHAPE_SPHERE ? p0 : st == DG_SHAPE_BOX ? sqrtf(p0 * p0 + p1 * p1 + p2 * p2) : st == DG_SHAPE_POINTS ? fmaxf(p0 + p1, p2) : p0 + p1;
        d[0] = (float)sf[DG_SF_POS]; d[1] = (float)sf[DG_SF_POS + 1]; d[2] = (float)sf[DG_SF_POS + 2];
        // (+ the two hull margins where hulls collide as hulls: their contacts exist out to margin + 2 x hull margin)
        d[3] = (float)BFh[gi[DG_GI_BODY_A] * DG_BF_STRIDE + DG_BF_BOUND] + (float)F[DG_HF_CONTACT_MARGIN] + (F[DG_HF_HULL_CONTACTS] > 0 ? 2.f * (float)F[DG_HF_HULL_MARGIN] : 0.f) + ext;
      }
      for (int k = 0; k < 4; k++) { int32_t bits; memcpy(&bits, &d[k], 4); plan.push_back(bits); }
    } }
  // shape frame descriptors, device-only, for narrow-phase lanes that each test a different shape: [LDS slot of the pose
  // of the shape's link (rotation columns, position at + 6) or of its body's base rotation | state offset of the base
  // position (base shapes) or -1 | first hull point | hull points]; slot -1: frozen in the world
  out.sd_off = plan.size();
  for (int s = 0; s < I[DG_H_N_SHAPES]; s++) {
    const int32_t* si = SIh + s * DG_SI_STRIDE; const int b = si[DG_SI_BODY], gl = si[DG_SI_LINK];
    const bool world = (si[DG_SI_FLAGS] & DG_SHAPE_WORLD) != 0;
    const int32_t rslot = world ? -1 : gl >= 0 ? plan[(size_t)nb * PLB_STRIDE + (size_t)gl * PLL_STRIDE + PLL_POSE] : plan[(size_t)b * PLB_STRIDE + PLB_R0];
    plan.push_back(rslot);
    plan.push_back((world || gl >= 0) ? -1 : BI[b * DG_BI_STRIDE + DG_BI_STATE_OFF]);
    plan.push_back(si[DG_SI_POINT_OFF]); plan.push_back(si[DG_SI_N_POINTS]);
  }
  // ancestor masks per link (body-local bits; bodies with more than 32 links get zeros and are never sliced)
  out.am_off = plan.size();
  for (int b = 0; b < nb; b++) {
    const int32_t* B = BI + b * DG_BI_STRIDE; const int first = B[DG_BI_FIRST_LINK], n = B[DG_BI_N_LINKS];
    for (int i = 0; i < n; i++) {
      uint32_t m = 0u;
      if (n <= 32) { m = 1u << i; const int par = LI[(first + i) * DG_LI_STRIDE + DG_LI_PARENT]; if (par >= 0) m |= (uint32_t)plan[out.am_off + (size_t)par]; }
      plan.push_back((int32_t)m);
    }
  }
  // rho per link, device-only (np_skip below): for joint i of a serial chain, the largest distance from the joint's origin that any
  // point of any shape on link i or a later link of the chain can have in any configuration -- over shapes s on link j >= i,
  // sum_{k = i+1 .. j} |LF_POS_k| + |centre of s in its link frame| + extent of s.  The extent is the bounding radius the narrow
  // phase uses (SC_BOUND), and for a hull at least the half length of the capsule that contains it (the ends of that capsule are
  // points the narrow phase measures from).  Rounded up.  A point of the chain then moves by at most sum_i |dq_i| rho_i when the
  // joints move by dq (revolute joints: each rotates everything behind it about an axis through its origin).  Other bodies: zeros.
  out.rh_off = plan.size();
  { const double* SFh = F + I[DG_H_OFF_SHAPE_F]; const double* LFh = F + I[DG_H_OFF_LINK_F];
    std::vector<float> rho((size_t)nl, 0.f);
    for (int b = 0; b < nb; b++) {
      const int32_t* B = BI + b * DG_BI_STRIDE; const int first = B[DG_BI_FIRST_LINK], n = B[DG_BI_N_LINKS];
      if (!is_fixed(B) || !is_serial_chain(B, LI, 6)) continue;
      for (int i = 0; i < n; i++) {
        double best = 0.0, along = 0.0;
        for (int j = i; j < n; j++) {
          if (j > i) { const double* lp = LFh + (first + j) * DG_LF_STRIDE + DG_LF_POS; along += std::sqrt(lp[0] * lp[0] + lp[1] * lp[1] + lp[2] * lp[2]); }
          for (int s = 0; s < I[DG_H_N_SHAPES]; s++) {
            const int32_t* si = SIh + s * DG_SI_STRIDE; if (si[DG_SI_BODY] != b || si[DG_SI_LINK] != first + j) continue;
            const double* sf = SFh + s * DG_SF_STRIDE; const int st = si[DG_SI_TYPE];
            const double p0 = sf[DG_SF_PARAMS], p1 = sf[DG_SF_PARAMS + 1], p2 = sf[DG_SF_PARAMS + 2];
            const double ext = st == DG_SHAPE_SPHERE ? p0 : st == DG_SHAPE_BOX ? std::sqrt(p0 * p0 + p1 * p1 + p2 * p2)
                             : st == DG_SHAPE_POINTS ? std::max(std::max(p0 + p1, p2), sf[DG_SF_HULL_HALF]) : p0 + p1;
            best = std::max(best, along + std::sqrt(sf[DG_SF_POS] * sf[DG_SF_POS] + sf[DG_SF_POS + 1] * sf[DG_SF_POS + 1] + sf[DG_SF_POS + 2] * sf[DG_SF_POS + 2]) + ext);
          }
        }
        rho[(size_t)(first + i)] = (float)(best * (1.0 + 1e-6));
      }
    }
    for (int l = 0; l < nl; l++) { int32_t bits; memcpy(&bits, &rho[(size_t)l], 4); plan.push_back(bits); } }
  PLB = plan.data(); PLL = plan.data() + (size_t)nb * PLB_STRIDE;  // (the appends above may have moved the vector)
  // ---- the scene as the kernels see it
  sc.nba = 0; for (int b = 0; b < nb; b++) if (!(BI[b * DG_BI_STRIDE + DG_BI_FLAGS] & DG_BODY_FROZEN)) sc.nba = b + 1;
  sc.nsha = 0; for (int s = 0; s < I[DG_H_N_SHAPES]; s++) if (SIh[s * DG_SI_STRIDE + DG_SI_TYPE] != DG_SHAPE_BOX) sc.nsha = s + 1;
  sc.no_minv_slices = sw.no_minv_slices ? 1 : 0; sc.no_chain_rows = sw.no_chain_rows ? 1 : 0; sc.no_sliced_reset = sw.no_sliced_reset ? 1 : 0;
  sc.debug_keep_ext = sw.debug_keep_ext ? 1 : 0;
  sc.nb = nb; sc.nl = nl; sc.nfr = I[DG_H_N_FRAMES]; sc.nsh = I[DG_H_N_SHAPES]; sc.npairs = npairs; sc.ngroups = I[DG_H_N_GROUPS]; sc.nops = nops;
  sc.act_dim = I[DG_H_ACT_DIM]; sc.obs_dim = I[DG_H_OBS_DIM]; sc.rew_dim = I[DG_H_REW_DIM]; sc.term_dim = I[DG_H_TERM_DIM];
  sc.substeps = I[DG_H_SUBSTEPS]; sc.iters = I[DG_H_SOLVER_ITERS]; sc.hot_start = I[DG_H_HOT_START]; sc.ik_iters = I[DG_H_IK_ITERS];
  sc.state_dim = I[DG_H_STATE_DIM]; sc.addon_off = I[DG_H_ADDON_STATE_OFF]; sc.max_contacts = maxc; sc.warm_off = I[DG_H_WARM_OFF]; sc.ncons = ncons;
  sc.term_mode = I[DG_H_TERM_MODE]; sc.n_term_groups = I[DG_H_N_TERM_GROUPS];
  sc.tr_off = tr_off; sc.tr_slots = tr; sc.cont_off = cont_off; sc.nv_max = nvmax; sc.total_slots = total; sc.ab_stride = ab_stride; sc.crow_tail = crow_tail; sc.nt = nt; sc.dense = dense ? 1 : 0; sc.dv_base = nb > 0 ? PLB[PLB_DV] : 0;
  sc.num_envs = num_envs; sc.stride = env_stride; sc.seed = seed; sc.env_base = env_index_base;
  sc.h = (float)F[DG_HF_DT]; sc.hm = (float)(F[DG_HF_DT] * F[DG_HF_MOTOR_IMPULSE_SCALE]); sc.gx = (float)F[DG_HF_GRAV_X]; sc.gy = (float)F[DG_HF_GRAV_Y]; sc.gz = (float)F[DG_HF_GRAV_Z];
  // ---- kernel form
  const bool hull_pairs = has_hull_pairs(I) && F[DG_HF_HULL_CONTACTS] > 0;  // the hull-hull narrow phase runs
  out.mf = hull_pairs && F[DG_HF_HULL_MANIFOLD] > 1;
  // helper wave: the LAST fixed-base chain body (so that wave 0 keeps the first arm), provided the scene has other
  // work to overlap with and every inverse-kinematics op on that body has the register-resident form
  sc.helper_body = -1;
  if (lanes == 64 && ncons == 0 && !out.mf && !sw.no_helper_wave) {  // (the manifold has no helper-wave form)
    int n_dyn = 0; for (int b = 0; b < nb; b++) if (!is_static(BI + b * DG_BI_STRIDE)) n_dyn++;
    for (int b = nb - 1; b >= 0 && n_dyn >= 2; b--) {
      if (!PLB[b * PLB_STRIDE + PLB_CHAIN]) continue;
      bool ok = true;
      for (int op = 0; op < nops; op++) {
        const int32_t* oi = out.blob_i.data() + I[DG_H_OFF_OP_I] + op * DG_OI_STRIDE;
        if (oi[DG_OI_BODY] == b && oi[DG_OI_CODE] == DG_OP_IK_CONTROL && !(oi[DG_OI_FLAGS] & DG_IK_DEV_CHAIN)) ok = false;
      }
      if (ok) { sc.helper_body = b; break; }
    }
  }
  out.par = sc.helper_body >= 0; out.no_par_reset = sw.no_par_reset.set;
  // polytope workspace of the hull-hull narrow phase: only worlds that collide two hulls
  if (hull_pairs) out.hull_ws_floats = (size_t)((num_envs + per - 1) / per) * (out.par ? 4 : 1) * (size_t)HH_WS_SLOTS * 64;
  // third wavefront for the narrow phase: it uses the transient region as its shape cache while the other two run
  // dynamics, so every moving body must have the register-resident (transient-free) dynamics
  sc.coll_wave = 0;
  if (out.par && npairs > 0 && !sw.no_collide_wave) {
    bool ok = true;
    for (int b = 0; b < nb; b++) if (!is_static(BI + b * DG_BI_STRIDE) && !PLB[b * PLB_STRIDE + PLB_CHAIN]) ok = false;
    sc.coll_wave = ok ? 1 : 0;
  }
  // sweeps split between the main and the helper wave: exactly two register-chain bodies, the second is the helper's,
  // and no other body carries joints (their rows would have to run on the main wave between the exchanges)
  sc.split_pgs = 0;
  if (out.par && !sw.no_split_sweeps) {
    int jointed = 0; for (int b = 0; b < nb; b++) if (BI[b * DG_BI_STRIDE + DG_BI_N_LINKS] > 0) jointed++;
    if (jointed == 2 && sc.reg_body[0] >= 0 && sc.reg_body[1] == sc.helper_body && sc.reg_body[0] != sc.helper_body) {
      sc.split_pgs = 1;
      // contact rows too when the dense DoF vector holds nothing but the two arms (no free body a contact could involve)
      if (dense && nt == PLB[sc.reg_body[0] * PLB_STRIDE + PLB_NV] + PLB[sc.reg_body[1] * PLB_STRIDE + PLB_NV] && !sw.no_split_contacts) sc.split_pgs = 2;
    }
  }
  if (!out.par && sw.no_reg_rows) sc.split_pgs = -1;  // ablation: the sliced sweeps keep their rows in LDS
  // a fourth wavefront for the second half of the pair table, if its contact list still fits LDS
  sc.coll_split = 0; sc.cont2_off = 0;
  if (sc.coll_wave && lanes == 64 && npairs >= 8 && !sw.no_collide_split) {
    const int extra = 1 + maxc * CL_STRIDE;
    if ((sc.total_slots + extra) * 64 * 4 <= LDS_MAX) {
      sc.cont2_off = sc.total_slots; sc.total_slots += extra; sc.coll_split = 1;
      out.lds_bytes = sc.total_slots * 64 * 4;
    }
  }
  // The update ops of such a scene (inverse kinematics above all) only write motor targets unless one of them is a
  // torque / force op; then the first substep's dynamics do not depend on them and can run alongside.
  sc.early_dyn = 0;
  if (sc.coll_wave && !sw.no_early_dynamics) {
    bool ok = true, long_update = false;  // worth it only when the update phase is long: an inverse-kinematics solve
    for (int op = 0; op < nops; op++) {
      const int32_t* oi = OI + op * DG_OI_STRIDE; const int code = oi[DG_OI_CODE];
      if (code == DG_OP_IK_CONTROL) long_update = true;
      if (code == DG_OP_EXTERNAL_FORCE || code == DG_OP_PROPELLOR || code == DG_OP_ADMITTANCE || (code == DG_OP_JOINT_CONTROL && oi[DG_OI_FLAGS] == DG_JC_TORQUE)) ok = false;
    }
    sc.early_dyn = (ok && long_update) ? 1 : 0;
  }
  // Later substeps without narrow phase and pose pass while the clearance lasts (substep_np_skip, dg_solver.h): the four-wavefront
  // kernel with both narrow-phase wavefronts and the fused contact-free substep, two fixed-base chains of six revolute joints
  // (rho above bounds rotations only) that are the scene's only moving bodies (nobody else reads a link pose between the
  // substeps, nothing else can come closer), and a second substep to skip.  The four workspace slots it needs are spare
  // slots of the padding behind the velocity-change blocks (split_slots), so the LDS plan does not grow.
  sc.np_skip = 0;
  if (sc.coll_wave && sc.coll_split && sc.split_pgs > 0 && ncons == 0 && sc.substeps >= 2 && !sw.no_np_skip && sc.total_slots * 64 * 4 <= LDS_MAX) {
    bool ok = sc.reg_body[0] >= 0 && sc.reg_body[1] == sc.helper_body;
    for (int k = 0; k < 2 && ok; k++) {
      const int32_t* B = BI + sc.reg_body[k] * DG_BI_STRIDE; const int first = B[DG_BI_FIRST_LINK];
      ok = is_fixed(B) && B[DG_BI_N_LINKS] == 6 && PLB[sc.reg_body[k] * PLB_STRIDE + PLB_CHAIN];
      for (int i = 0; i < 6 && ok; i++) ok = LI[(first + i) * DG_LI_STRIDE + DG_LI_TYPE] == 0;
    }
    for (int b = 0; b < nb && ok; b++) if (!is_static(BI + b * DG_BI_STRIDE) && b != sc.reg_body[0] && b != sc.reg_body[1]) ok = false;
    sc.np_skip = ok ? 1 : 0;
  }
  // ---- default velocity motors on every joint
  memset(&out.mt, 0, sizeof out.mt);
  for (int l = 0; l < nl; l++) { out.mt.v[3 * l] = 0.f; out.mt.v[3 * l + 1] = 1.f; out.mt.v[3 * l + 2] = -(float)F[DG_HF_DEFAULT_MOTOR_IMPULSE]; }
  for (int op = 0; op < nops; op++) {  // admittance_controller.py:34: its joints' velocity motors are switched off at construction
    const int32_t* oi = OI + op * DG_OI_STRIDE;
    if (oi[DG_OI_CODE] == DG_OP_ADMITTANCE) for (int k = 0; k < oi[DG_OI_N]; k++) out.mt.v[3 * (I[I[DG_H_OFF_ILIST] + oi[DG_OI_ILIST] + k]) + 2] = 0.f;
  }
  // ---- load-time state vector
  std::vector<float>& init = out.init; init.assign((size_t)sc.state_dim, 0.f);
  const double* BF = F + I[DG_H_OFF_BODY_F];
  for (int b = 0; b < nb; b++) {
    const int so = BI[b * DG_BI_STRIDE + DG_BI_STATE_OFF]; if (so < 0) continue;  // frozen: no state
    for (int k = 0; k < 3; k++) init[so + DG_BS_POS + k] = (float)BF[b * DG_BF_STRIDE + DG_BF_INIT_POS + k];
    for (int k = 0; k < 4; k++) init[so + DG_BS_QUAT + k] = (float)BF[b * DG_BF_STRIDE + DG_BF_INIT_QUAT + k];
  }
  for (int op = 0; op < nops; op++) {  // dynamics_randomizer state before its first draw: URDF masses, default damping
    const int32_t* oi = OI + op * DG_OI_STRIDE;
    if (oi[DG_OI_CODE] == DG_OP_RANDOMIZE_COLOR) {  // visual_randomizer: the configured colour, flat, until the first draw
      float* tx = init.data() + sc.addon_off + oi[DG_OI_STATE_OFF];
      for (int k = 0; k < 3; k++) tx[DG_TX_A + k] = tx[DG_TX_B + k] = (float)BF[oi[DG_OI_BODY] * DG_BF_STRIDE + DG_BF_COLOR + k];
      tx[DG_TX_FREQ] = 1.f; tx[DG_TX_KIND] = (float)DG_TEX_FLAT;
      continue;
    }
    if (oi[DG_OI_CODE] != DG_OP_RANDOMIZE_DYNAMICS) continue;
    const int so = sc.addon_off + oi[DG_OI_STATE_OFF];
    for (int k = 0; k < oi[DG_OI_N]; k++) init[so + k] = 1.f;
    init[so + oi[DG_OI_N]] = (float)F[DG_HF_ANG_DAMPING];
  }
  return DG_OK;
}

}  // namespace dg
