// dg_closestq.h -- batched closest-points query (pybullet's p.getClosestPoints(bodyA, bodyB, distance, linkIndexA, linkIndexB); the
// reference never calls it -- no addon of its own asks for a clearance -- so there is no call site to name: this is the query a
// pybullet user expects, and what the `proximity_sensor` addon is built on).  The contact query (dg_contactq.h) stops at the contact
// margin because every cull of collide is tied to it and the pair table has lost the statically pruned pairs; this one has a narrow
// phase of its own.  Two launches per call:
//   pose_kernel           (dg_render.h) without cameras or a mount row: world frame of every shape -> the caller's scratch, per env
//                         [nsh][RS_STRIDE].  It runs in the world's own workspace mode;
//   closest_query_kernel  one env per lane, workgroups of one wavefront.  It reads that table and the scene arrays only -- no LDS
//                         workspace, no Lane -- so it is ONE kernel for every workspace mode of the world.
// CANDIDATE PAIRS are decided here from SI, not from PI: side A is every shape whose id matches (body_a, link_a) in ascending shape
// index, side B every shape that matches (body_b, link_b) -- with DG_CONTACT_ANY every shape of another body -- in ascending index
// under each A shape.  Left out: two shapes of one body (a rigidly merged child is its parent's body), DG_SHAPE_NO_COLLIDE shapes,
// two shapes neither of which can move, box against box (the step has no routine for it either).  Pairs that static pruning took
// out of PI are in: that is the point of the query.  Both loops are wave-uniform; rows are written in pair order per lane.
// PER-PAIR GEOMETRY is the step's own model of the pair (the DGD functions of dg_solver.h / dg_hull.h), so the distance reaches the
// contact query's value as the pair closes:
//   round against round (sphere, capsule, a hull through its fitted capsule)  seg_seg / closest_on_seg + sphere_sphere
//   sphere / capsule against box      sphere_box on the centre / on the two end spheres, the nearer one (the first on a tie)
//   hull against box                  the nearest of the hull's points by sphere_box(.., 0, ..) (the first on a tie)
//   hull against hull, hull_contacts > 0   hull_hull with max_dist = distance + 2 x hull margin; distance = its result - 2 x hull
//                                     margin, witnesses moved by the hull margin as collide does: overlapping hulls report the
//                                     polytope depth, as the step does.  hull_contacts = 0: the fitted capsules.
// The box is side B inside the primitive; the result is flipped to the caller's A / B.
// CULLS, each a lower bound of the pair's distance in its model and each a wave-uniform __any skip:
//   bounding spheres (RS_C; radius: sphere r, box |half|, capsule r + half, hull max(r + half, DG_SF_PARAMS + 2) -- the sphere that
//   holds the fitted capsule AND every point, collide's SC_BOUND) against distance (+ 2 x hull margin for two hulls as hulls);
//   a round shape's bounding sphere against the box itself (a ground plane's own sphere reaches everything);
//   for hull against hull the capsules that CONTAIN the hulls (DG_SF_HULL_HALF), the test of collide with distance for the margin.
// The sphere tests are a hair wide (0.01 % + 10 um: a box's sphere touches its corners, the roots are 1 ulp).  no_cull (debug path,
// dg_debug_closest_no_cull) runs every candidate pair through its primitive; the tests show the same bits come back.
// POLYTOPE WORKSPACE.  DevScene::hull_ws is null in a world whose hull pairs were all pruned and is sized for the step grid, so the
// query brings its own: `hws`, ceil(num_envs / 64) x HH_WS_SLOTS x 64 floats behind the pose table in the caller's scratch.  Bound:
// the kernel is launched with ceil(num_envs / 64) workgroups of blockDim.x = 64, so hull_ws_of gives lane l of workgroup g the
// column g x HH_WS_SLOTS x 64 + l (blockDim.x >> 6 = 1, threadIdx.x >> 6 = 0) and HEpa reads and writes e[slot x 64].  Every slot
// hh_epa forms is below HH_WS_SLOTS: vertices HW_VW + 3 k + 2 and HW_VID + k with k < HH_EPA_MAXV (put(nv, ..) comes after the
// `nv >= HH_EPA_MAXV` break), faces HW_FV / HW_FN / HW_FD with f < nf <= HH_EPA_MAXF (`nf >= HH_EPA_MAXF` break before nf++), horizon
// edges HW_ED + t with t < ne <= HH_EPA_MAXE (`ne < HH_EPA_MAXE` guard), coplanar points HW_PW / HW_PID + np with np < HH_FACE_PTS
// (`np >= HH_FACE_PTS` break); HH_WS_SLOTS = HW_PID + HH_FACE_PTS is the end of the last array.  So the largest float index is
// g x HH_WS_SLOTS x 64 + 63 + (HH_WS_SLOTS - 1) x 64 < (g + 1) x HH_WS_SLOTS x 64 <= ceil(num_envs / 64) x HH_WS_SLOTS x 64.  The
// manifold buffers (MF_*) are not used: hull_manifold is never called here.
// Lanes of the last wavefront without an env are clamped to the last env and stay in every call (hull_hull and hull_tables vote and
// read lane tables wave-wide); only their stores are masked, as contact_query_kernel does.
// What bounds it: instruction issue of a lone wavefront per 64 envs (the GJK loop of the hull pairs that pass the culls); the
// output is 4-100 B per row.
#pragma once
#include "dg_render.h"
#include "dg_contactq.h"

namespace dg {

// world segment (centre, half axis) and radius of a round shape: sphere, capsule, or a hull's fitted capsule -- collide's SC_C / SC_H /
// SC_R.  `row` is the shape's row of the pose table (a hull's RS_R / RS_P is its LINK frame, the axis comes through DG_SF_ROT).
DGD void clq_round(const DevScene& sc, const float* row, int sh, int type, V3& c, V3& hax, float& r) {
  cfp sf = sc.SF + sh * DG_SF_STRIDE; c = v3(row[RS_C], row[RS_C + 1], row[RS_C + 2]); r = sf[DG_SF_PARAMS];
  if (type == DG_SHAPE_SPHERE) { hax = v3(0.f, 0.f, 0.f); return; }
  V3 ax = v3(row[RS_R + 2], row[RS_R + 5], row[RS_R + 8]);
  if (type == DG_SHAPE_POINTS) {
    M3 R; _Pragma("unroll") for (int q = 0; q < 9; q++) R.m[q] = row[RS_R + q];
    ax = mul(R, v3(sf[DG_SF_ROT + 2], sf[DG_SF_ROT + 5], sf[DG_SF_ROT + 8]));
  }
  hax = ax * sf[DG_SF_PARAMS + 1];
}
// radius of the sphere about RS_C that holds the shape in the model the pair is tested in
DGD float clq_bound(const DevScene& sc, int sh, int type) {
  cfp sf = sc.SF + sh * DG_SF_STRIDE; const float p0 = sf[DG_SF_PARAMS], p1 = sf[DG_SF_PARAMS + 1], p2 = sf[DG_SF_PARAMS + 2];
  return type == DG_SHAPE_SPHERE ? p0 : type == DG_SHAPE_BOX ? sqrtf(p0 * p0 + p1 * p1 + p2 * p2) : type == DG_SHAPE_POINTS ? fmaxf(p0 + p1, p2) : p0 + p1;
}
// can the shape's body move: collide's candidate rule (a fixed base without joints cannot, respawned or not)
DGD bool clq_moves(const DevScene& sc, int sh) {
  cip bi = sc.BI + sc.SI[sh * DG_SI_STRIDE + DG_SI_BODY] * DG_BI_STRIDE; return !((bi[DG_BI_FLAGS] & DG_BODY_FIXED) && bi[DG_BI_N_LINKS] == 0);
}

// table [num_envs][nsh][RS_STRIDE] (pose_kernel); hws: the polytope workspace (above); count [num_envs]; ids [num_envs][K][2], geom
// [num_envs][K][10], nearest_ids [num_envs][2], nearest_geom [num_envs][10] (each may be null).  Every slot is written.
__global__ __launch_bounds__(64) void closest_query_kernel(DevScene sc, const float* table, int body_a, int link_a, int body_b, int link_b, float distance, int K,
                                                            int no_cull, float* hws, int32_t* count, int32_t* ids, float* geom, int32_t* nearest_ids, float* nearest_geom) {
  const int lane = threadIdx.x, env = blockIdx.x * 64 + lane; const bool valid = env < sc.num_envs; const int e = valid ? env : sc.num_envs - 1;
  const int nsh = sc.nsh; const float* tb = table + (size_t)e * (size_t)(nsh * RS_STRIDE);
  const bool hull_mode = sc.HF[DG_HF_HULL_CONTACTS] > 0.f; const float hmg = sc.HF[DG_HF_HULL_MARGIN];
  const size_t row = (size_t)e * (size_t)K;
  int found = 0;  // pairs within `distance` so far; the first K of them are rows
  int bia = -1, bib = -1; float bd = distance; V3 bpa = v3(0.f, 0.f, 0.f), bpb = bpa, bn = bpa;  // the nearest pair
  for (int sa = 0; sa < nsh; sa++) {
    cip sia = sc.SI + sa * DG_SI_STRIDE; const int ida = cq_shape_id(sc, sa), ta = sia[DG_SI_TYPE];
    if ((sia[DG_SI_FLAGS] & DG_SHAPE_NO_COLLIDE) || !cq_match(ida, body_a, link_a)) continue;
    const bool a_moves = clq_moves(sc, sa); const float bnd_a = clq_bound(sc, sa, ta);
    const float* ra_row = tb + sa * RS_STRIDE;
    for (int sb = 0; sb < nsh; sb++) {
      cip sib = sc.SI + sb * DG_SI_STRIDE; const int idb = cq_shape_id(sc, sb), tbt = sib[DG_SI_TYPE];
      if (sib[DG_SI_BODY] == sia[DG_SI_BODY] || (sib[DG_SI_FLAGS] & DG_SHAPE_NO_COLLIDE) || !cq_match(idb, body_b, link_b)) continue;
      if (!(a_moves || clq_moves(sc, sb)) || (ta == DG_SHAPE_BOX && tbt == DG_SHAPE_BOX)) continue;
      const float* rb_row = tb + sb * RS_STRIDE;
      const bool as_hulls = hull_mode && ta == DG_SHAPE_POINTS && tbt == DG_SHAPE_POINTS;
      const V3 cca = v3(ra_row[RS_C], ra_row[RS_C + 1], ra_row[RS_C + 2]), ccb = v3(rb_row[RS_C], rb_row[RS_C + 1], rb_row[RS_C + 2]);
      const V3 dc = cca - ccb;
      const float lim = distance + (as_hulls ? 2.f * hmg : 0.f);  // what the pair's model distance is compared with
      { const float reach = (bnd_a + clq_bound(sc, sb, tbt) + lim) * 1.0001f + 1e-5f;
        if (!__any(no_cull || dot(dc, dc) < reach * reach)) continue; }
      Hit h; h.hit = false; h.dist = 0.f; h.n = v3(0.f, 0.f, 0.f); h.pa = h.n; h.pb = h.n;
      // Two shapes that are not boxes go through their primitive in SHAPE-INDEX order whichever side the caller named first, and the
      // result is flipped (sides swapped, normal negated: both exact), so (X, Y) and (Y, X) are the same bits mirrored -- GJK from
      // the other hull's frame, or seg_seg with its arguments exchanged, would differ in the last place.
      const bool rev = sb < sa; const int s1 = rev ? sb : sa, s2 = rev ? sa : sb, t1 = rev ? tbt : ta, t2 = rev ? ta : tbt;
      cip si1 = rev ? sib : sia; cip si2 = rev ? sia : sib; const float* row1 = rev ? rb_row : ra_row; const float* row2 = rev ? ra_row : rb_row;
      const V3 cc1 = rev ? ccb : cca, cc2 = rev ? cca : ccb;
      if (as_hulls) {
        // hull against hull: collide's branch, statement for statement, with `distance` for the contact margin
        HullPairD hp; V3 pla, plb;
        _Pragma("unroll") for (int q = 0; q < 9; q++) { hp.RA.m[q] = row1[RS_R + q]; hp.RB.m[q] = row2[RS_R + q]; }
        pla = v3(row1[RS_P], row1[RS_P + 1], row1[RS_P + 2]); plb = v3(row2[RS_P], row2[RS_P + 1], row2[RS_P + 2]);
        bool close = true;
        { cfp fa = sc.SF + s1 * DG_SF_STRIDE, fb = sc.SF + s2 * DG_SF_STRIDE;
          const V3 axa = mul(hp.RA, v3(fa[DG_SF_ROT + 2], fa[DG_SF_ROT + 5], fa[DG_SF_ROT + 8])) * fa[DG_SF_HULL_HALF];
          const V3 axb = mul(hp.RB, v3(fb[DG_SF_ROT + 2], fb[DG_SF_ROT + 5], fb[DG_SF_ROT + 8])) * fb[DG_SF_HULL_HALF];
          V3 qa, qb; seg_seg(cc1 - axa, cc1 + axa, cc2 - axb, cc2 + axb, qa, qb);
          const float cl = (fa[DG_SF_PARAMS] + fb[DG_SF_PARAMS] + lim) * 1.0001f + 1e-5f; const V3 dq = qa - qb;
          close = no_cull || dot(dq, dq) < cl * cl; }
        if (!__any(close)) continue;
        hp.pa = sc.PF + 3 * si1[DG_SI_POINT_OFF]; hp.na = si1[DG_SI_N_POINTS]; hp.pb = sc.PF + 3 * si2[DG_SI_POINT_OFF]; hp.nb = si2[DG_SI_N_POINTS];
        hp.tBA = plb - pla; hp.ew = hull_ws_of(hws);
        hull_tables(hp, hp.na <= 64 && hp.nb <= 64);  // (all 64 lanes are here)
        HullHit hh; hull_hull(hp, cc1 - cc2, lim, close, hh);
        h.dist = hh.dist - 2.f * hmg; h.hit = hh.hit && h.dist < distance; h.n = hh.n;
        h.pa = (hh.pa + pla) - hh.n * hmg; h.pb = (hh.pb + pla) + hh.n * hmg;
        if (rev) { const V3 t = h.pa; h.pa = h.pb; h.pb = t; h.n = -h.n; }
      } else if (ta != DG_SHAPE_BOX && tbt != DG_SHAPE_BOX) {
        // round against round: closest points of the two segments, then sphere-sphere
        V3 ca, ha, cb, hb; float ra, rb; clq_round(sc, row1, s1, t1, ca, ha, ra); clq_round(sc, row2, s2, t2, cb, hb, rb);
        const V3 a0 = ca - ha, a1 = ca + ha, b0 = cb - hb, b1 = cb + hb;
        V3 qa = a0, qb = b0;
        if (t1 == DG_SHAPE_SPHERE && t2 != DG_SHAPE_SPHERE) qb = closest_on_seg(b0, b1, a0);
        else if (t1 != DG_SHAPE_SPHERE) seg_seg(a0, a1, b0, b1, qa, qb);
        h = sphere_sphere(qa, ra, qb, rb, distance);
        if (rev) { const V3 t = h.pa; h.pa = h.pb; h.pb = t; h.n = -h.n; }
      } else {
        // one box: it is side B inside the primitive
        const bool a_is_box = ta == DG_SHAPE_BOX; const int sx = a_is_box ? sb : sa, sbx = a_is_box ? sa : sb, tx = a_is_box ? tbt : ta;
        const float* xr = a_is_box ? rb_row : ra_row; const float* br = a_is_box ? ra_row : rb_row;
        WShape bx; cfp bf = sc.SF + sbx * DG_SF_STRIDE;
        _Pragma("unroll") for (int q = 0; q < 9; q++) bx.R.m[q] = br[RS_R + q];
        bx.p = v3(br[RS_P], br[RS_P + 1], br[RS_P + 2]); bx.prm0 = bf[DG_SF_PARAMS]; bx.prm1 = bf[DG_SF_PARAMS + 1]; bx.prm2 = bf[DG_SF_PARAMS + 2];
        const V3 cx = a_is_box ? ccb : cca;
        { const Hit hb = sphere_box(cx, clq_bound(sc, sx, tx) * 1.0001f + 1e-5f, bx, distance); if (!__any(no_cull || hb.hit)) continue; }
        if (tx == DG_SHAPE_POINTS) {
          cip six = sc.SI + sx * DG_SI_STRIDE; const int poff = six[DG_SI_POINT_OFF], npts = six[DG_SI_N_POINTS];
          M3 Rl; _Pragma("unroll") for (int q = 0; q < 9; q++) Rl.m[q] = xr[RS_R + q];
          const V3 pl = v3(xr[RS_P], xr[RS_P + 1], xr[RS_P + 2]);
          for (int k2 = 0; k2 < npts; k2++) {
            cfp pp = sc.PF + 3 * (poff + k2);
            const Hit hk = sphere_box(pl + mul(Rl, v3(pp[0], pp[1], pp[2])), 0.f, bx, distance);
            if (k2 == 0 || hk.dist < h.dist) h = hk;
          }
        } else {
          V3 c, hax; float r; clq_round(sc, xr, sx, tx, c, hax, r);
          h = sphere_box(c - hax, r, bx, distance);
          if (tx == DG_SHAPE_CAPSULE && sc.SF[sx * DG_SF_STRIDE + DG_SF_PARAMS + 1] > 0.f) { const Hit h1 = sphere_box(c + hax, r, bx, distance); if (h1.dist < h.dist) h = h1; }
        }
        if (a_is_box) { const V3 t = h.pa; h.pa = h.pb; h.pb = t; h.n = -h.n; }
      }
      if (!as_hulls) h.hit = h.dist < distance;  // (one comparison for every primitive: the reported rule)
      if (!h.hit) continue;
      if (h.dist < bd) {  // (strict: a tie stays with the first pair)
        bd = h.dist; bia = ida; bib = idb; bpa = h.pa; bpb = h.pb; bn = h.n; }
      if (found < K && valid) {
        if (ids) { int32_t* o = ids + (row + found) * 2; o[0] = ida; o[1] = idb; }
        if (geom) {
          float* o = geom + (row + found) * CQ_GEOM_STRIDE;
          o[CQ_POS_A] = h.pa.x; o[CQ_POS_A + 1] = h.pa.y; o[CQ_POS_A + 2] = h.pa.z; o[CQ_POS_B] = h.pb.x; o[CQ_POS_B + 1] = h.pb.y; o[CQ_POS_B + 2] = h.pb.z;
          o[CQ_NORMAL] = h.n.x; o[CQ_NORMAL + 1] = h.n.y; o[CQ_NORMAL + 2] = h.n.z; o[CQ_DIST] = h.dist;
        }
      }
      found++;
    }
  }
  if (!valid) return;
  count[e] = found;
  for (int j = found; j < K; j++) {
    if (ids) { int32_t* o = ids + (row + j) * 2; o[0] = -1; o[1] = -1; }
    if (geom) { float* o = geom + (row + j) * CQ_GEOM_STRIDE; for (int t = 0; t < CQ_GEOM_STRIDE; t++) o[t] = 0.f; }
  }
  if (nearest_ids) { nearest_ids[2 * (size_t)e] = bia; nearest_ids[2 * (size_t)e + 1] = bib; }
  if (nearest_geom) {
    float* o = nearest_geom + (size_t)e * CQ_GEOM_STRIDE;
    o[CQ_POS_A] = bpa.x; o[CQ_POS_A + 1] = bpa.y; o[CQ_POS_A + 2] = bpa.z; o[CQ_POS_B] = bpb.x; o[CQ_POS_B + 1] = bpb.y; o[CQ_POS_B + 2] = bpb.z;
    o[CQ_NORMAL] = bn.x; o[CQ_NORMAL + 1] = bn.y; o[CQ_NORMAL + 2] = bn.z; o[CQ_DIST] = bd;
  }
}

}  // namespace dg
