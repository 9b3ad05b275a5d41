// mjpl_distance.h -- signed geom distances and clearance per configuration (mjpl_distances*, mjpl_clearance*).
//
// What it adds: how far a configuration is from touching anything -- the quantity MuJoCo users read from
// data.contact.dist or mj_geomDistance.  The numbers here are the exact Euclidean signed distance of the two
// solids (gap width when disjoint, minus the penetration depth when they overlap; a plane is a half-space),
// computed in float64 by the routines below.  They are geometry, not MuJoCo's solver output, and margins are
// not subtracted.
//
// Shape: k_contacts's (mjpl_contacts.h), one lane per configuration.
//   1. The lane runs the interpreter's float64 FK (run_config with EMIT) into the contacts scratch row.
//   2. It walks the candidate table in order with a wave-uniform pair index.  Per pair: a bound cull against
//      distmax (|c1 - c2| - rb1 - rb2, or the signed centre distance - rb for a plane), then -- if any lane of
//      the wave still needs it -- the pair's distance routine.
//   3. k_distance<DM_DIST> (distances) stores D[i][p] = min(d_p, distmax); k_distance<DM_CLEAR> (clearance) keeps
//      (min over non-allowed pairs of D - margin, its pair index) in registers and stores 12 bytes per
//      configuration; k_distance<DM_GRAD> (clearance gradients) does the same, then runs the epilogue of
//      mjpl_distance_grad.h once per lane; k_distance<DM_NEAR> (near pairs) lists every non-allowed pair below
//      distmax with its distance, witnesses and gradient (mjpl_distance_grad.h: near_step), up to K per lane;
//      k_distance<DM_SWEEP> (the bubble measurement of the certified edge checks, mjpl_sweep.h) is DM_CLEAR's walk
//      without the "cannot beat the best so far" skip and with two minima: D - margin, and D - margin minus how far
//      the pair can move while every planning column c travels at most HD[c] from q (the lever table W of
//      mjpl_compile.h: build_sweep_table).
// The walks of all five modes and of k_contacts load a pair's geoms with contact_load_pair (mjpl_contacts.h).
//
// The routines reduce every non-plane pair to core distance minus radii (sphere = point, capsule = segment,
// box = box).  Disjoint cores: the minimum over the feature pairs that can hold the closest points (end
// points, the box's 8 vertices and 12 edges); every candidate is a distance between two points of the sets,
// so the minimum is exact up to rounding.  Overlapping cores: the least normalised overlap over the separating
// axes of the pair (3 face normals of a box, 3 segment x box-axis crosses, 15 axes for two boxes), which is
// the penetration depth of two convex polytopes.
#pragma once

namespace mjpl {

// per-pair record of the distance table (mjpl_compile.h: build_distance_table), beside the candidate table of
// mjpl_contacts.h: rb1 + rb2 (geom_rbound; a plane's is 0) and whether the ruleset allows the pair
enum : int { DT_RBSUM = 0, DT_ALLOWED, DT_LEN = 2 };

// A pair is culled only when its bound exceeds distmax by this much, so that rounding of the bound can never
// hide a distance below distmax: a culled pair's exact distance is >= distmax + slack - (a few ulps).
constexpr double kDistCullSlack = 1e-9;
// squared lengths below this are degenerate segments (points)
constexpr double kDistTiny = 1e-30;

__device__ __forceinline__ double dist_clamp01(double x) { return fmin(fmax(x, 0.0), 1.0); }

// squared distance between the segments p1 + s d1 and p2 + t d2 (s, t in [0, 1]): closest points with each
// parameter optimal for the other after clamping; parallel and degenerate segments included.  c1, c2 (both or
// neither): the closest points, for the witness routines of mjpl_distance_grad.h.
__device__ __forceinline__ double seg_seg_d2(const double *p1, const double *d1, const double *p2, const double *d2,
                                             double *c1 = nullptr, double *c2 = nullptr) {
  const double r[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
  const double a = dot3(d1, d1), e = dot3(d2, d2), f = dot3(d2, r), c = dot3(d1, r), b = dot3(d1, d2);
  double s, t;
  if (e <= kDistTiny) {
    t = 0.0;
    s = a <= kDistTiny ? 0.0 : dist_clamp01(-c / a);
  } else {
    const double denom = a * e - b * b;
    s = (a > kDistTiny && denom > 0) ? dist_clamp01((b * f - c * e) / denom) : 0.0;
    t = (b * s + f) / e;
    if (t < 0) {
      t = 0.0;
      s = a <= kDistTiny ? 0.0 : dist_clamp01(-c / a);
    } else if (t > 1) {
      t = 1.0;
      s = a <= kDistTiny ? 0.0 : dist_clamp01((b - c) / a);
    }
  }
  double w2 = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double x1 = p1[k] + d1[k] * s, x2 = p2[k] + d2[k] * t;
    const double w = x1 - x2;
    w2 += w * w;
    if (c1) {
      c1[k] = x1;
      c2[k] = x2;
    }
  }
  return w2;
}

// squared distance from the point p to the segment q + t d, t in [0, 1]; c: the segment's closest point
__device__ __forceinline__ double pt_seg_d2(const double *p, const double *q, const double *d, double *c = nullptr) {
  const double r[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  const double dd = dot3(d, d);
  const double t = dd <= kDistTiny ? 0.0 : dist_clamp01(dot3(r, d) / dd);
  const double w[3] = {r[0] - d[0] * t, r[1] - d[1] * t, r[2] - d[2] * t};
  if (c) {
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = q[k] + d[k] * t;
  }
  return dot3(w, w);
}

// squared distance from the point p (box frame) to the box |x_k| <= s_k, 0 inside; c: the box's closest point
__device__ __forceinline__ double pt_box_d2(const double *p, const double *s, double *c = nullptr) {
  double w2 = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double x = fmin(fmax(p[k], -s[k]), s[k]);
    const double w = p[k] - x;
    w2 += w * w;
    if (c) c[k] = x;
  }
  return w2;
}

// min over the box's 12 edges of the squared distance to the segment p + t d (all in the box frame)
__device__ __forceinline__ double seg_box_edges_d2(const double *p, const double *d, const double *s) {
  double best = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
      double a[3], e[3];
      a[k] = -s[k];
      a[i] = (q & 1) ? s[i] : -s[i];
      a[j] = (q & 2) ? s[j] : -s[j];
      e[k] = 2 * s[k];
      e[i] = 0.0;
      e[j] = 0.0;
      best = fmin(best, seg_seg_d2(p, d, a, e));
    }
  }
  return best;
}

// squared distance between the segment p + t d and the box (box frame), valid when they are disjoint: the
// closest points are then an end point and the box, or the segment and one of the box's edges
__device__ __forceinline__ double seg_box_disjoint_d2(const double *p, const double *d, const double *s) {
  const double q[3] = {p[0] + d[0], p[1] + d[1], p[2] + d[2]};
  return fmin(fmin(pt_box_d2(p, s), pt_box_d2(q, s)), seg_box_edges_d2(p, d, s));
}

// Segment m +- h (box frame) against the box |x_k| <= s_k on the separating axes: the 3 face normals and
// h x e_k (skipped when h is nearly parallel to e_k, or zero).  Returns the least normalised overlap (the
// penetration depth when >= 0); *sep = some axis has a gap.
__device__ __forceinline__ double seg_box_sat(const double *m, const double *h, const double *s, bool *sep) {
  double depth = INFINITY;
  bool gap = false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double o = s[k] + fabs(h[k]) - fabs(m[k]);
    gap = gap || o < 0;
    depth = fmin(depth, o);
  }
  const double hh = dot3(h, h);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;
    // n = h x e_k: n_k = 0, n_i = h_j, n_j = -h_i
    const double nn = h[i] * h[i] + h[j] * h[j];
    if (nn > 1e-12 * hh) {
      const double rad = s[i] * fabs(h[j]) + s[j] * fabs(h[i]);
      const double o = (rad - fabs(h[j] * m[i] - h[i] * m[j])) / sqrt(nn);
      gap = gap || o < 0;
      depth = fmin(depth, o);
    }
  }
  *sep = gap;
  return depth;
}

// core of a sphere (point: seg = false) or capsule (segment) against a box: signed distance of the cores
__device__ __forceinline__ double core_box_distance(bool seg, const GeomT<double> &g, const double *sg,
                                                    const GeomT<double> &box, const double *sb) {
  const double tmp[3] = {g.pos[0] - box.pos[0], g.pos[1] - box.pos[1], g.pos[2] - box.pos[2]};
  double m[3];
  mul_matT_vec3(m, box.m, tmp);
  if (!seg) {  // (wave-uniform)
    const double d2 = pt_box_d2(m, sb);
    if (d2 > 0) return sqrt(d2) - sg[0];
    const double depth = fmin(fmin(sb[0] - fabs(m[0]), sb[1] - fabs(m[1])), sb[2] - fabs(m[2]));
    return -depth - sg[0];
  }
  const double axis[3] = {g.m[2], g.m[5], g.m[8]};
  double a[3], h[3];
  mul_matT_vec3(a, box.m, axis);
#pragma unroll
  for (int k = 0; k < 3; k++) h[k] = a[k] * sg[1];
  bool sep;
  const double depth = seg_box_sat(m, h, sb, &sep);
  if (!sep) return -depth - sg[0];
  const double p[3] = {m[0] - h[0], m[1] - h[1], m[2] - h[2]};
  const double d[3] = {2 * h[0], 2 * h[1], 2 * h[2]};
  return sqrt(seg_box_disjoint_d2(p, d, sb)) - sg[0];
}

// point or segment cores of two spheres / capsules: distance of the cores minus both radii
__device__ __forceinline__ double core_core_distance(const GeomT<double> &g1, const double *s1, bool seg1,
                                                     const GeomT<double> &g2, const double *s2, bool seg2) {
  const double h1 = seg1 ? s1[1] : 0.0, h2 = seg2 ? s2[1] : 0.0;
  double p1[3], d1[3], p2[3], d2[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    d1[k] = 2 * h1 * g1.m[3 * k + 2];
    d2[k] = 2 * h2 * g2.m[3 * k + 2];
    p1[k] = g1.pos[k] - h1 * g1.m[3 * k + 2];
    p2[k] = g2.pos[k] - h2 * g2.m[3 * k + 2];
  }
  double w2 = seg_seg_d2(p1, d1, p2, d2);
  if (seg1 && seg2) {  // (wave-uniform) end points against the other segment: robust to near-parallel axes
    const double q1[3] = {p1[0] + d1[0], p1[1] + d1[1], p1[2] + d1[2]};
    const double q2[3] = {p2[0] + d2[0], p2[1] + d2[1], p2[2] + d2[2]};
    w2 = fmin(w2, fmin(fmin(pt_seg_d2(p1, p2, d2), pt_seg_d2(q1, p2, d2)),
                       fmin(pt_seg_d2(p2, p1, d1), pt_seg_d2(q2, p1, d1))));
  }
  return sqrt(w2) - (s1[0] + s2[0]);
}

// two boxes: 15-axis SAT decides overlap (least normalised overlap = depth; an edge-pair axis with
// 1 - R_ij^2 < 1e-12 is skipped, as box_box does); disjoint boxes by feature enumeration: vertex against box
// (8 + 8, b2's as the end points of its edges) and edge against edge (12 x 12)
__device__ __forceinline__ double box_box_distance(const GeomT<double> &b1, const double *s1, const GeomT<double> &b2,
                                                   const double *s2) {
  const double dp[3] = {b2.pos[0] - b1.pos[0], b2.pos[1] - b1.pos[1], b2.pos[2] - b1.pos[2]};
  double R[9], t[3];  // (|R| enters as operand modifiers: no array of its own)
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) R[3 * i + j] = b1.m[i] * b2.m[j] + b1.m[3 + i] * b2.m[3 + j] + b1.m[6 + i] * b2.m[6 + j];
  mul_matT_vec3(t, b1.m, dp);
  double depth = INFINITY;
  bool sep = false;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double o = s1[i] + s2[0] * fabs(R[3 * i]) + s2[1] * fabs(R[3 * i + 1]) + s2[2] * fabs(R[3 * i + 2]) - fabs(t[i]);
    sep = sep || o < 0;
    depth = fmin(depth, o);
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double tj = t[0] * R[j] + t[1] * R[3 + j] + t[2] * R[6 + j];
    const double o = s1[0] * fabs(R[j]) + s1[1] * fabs(R[3 + j]) + s1[2] * fabs(R[6 + j]) + s2[j] - fabs(tj);
    sep = sep || o < 0;
    depth = fmin(depth, o);
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      const double len2 = 1 - R[3 * i + j] * R[3 * i + j];
      if (!(len2 < 1e-12)) {
        const double ra = s1[i1] * fabs(R[3 * i2 + j]) + s1[i2] * fabs(R[3 * i1 + j]);
        const double rb = s2[j1] * fabs(R[3 * i + j2]) + s2[j2] * fabs(R[3 * i + j1]);
        const double tl = t[i2] * R[3 * i1 + j] - t[i1] * R[3 * i2 + j];
        const double o = (ra + rb - fabs(tl)) / sqrt(len2);
        sep = sep || o < 0;
        depth = fmin(depth, o);
      }
    }
  }
  if (!sep) return -depth;
  double best = INFINITY;
  // b2's 12 edges in b1's frame (axis k of b2 is column k of R) against b1: their end points are b2's vertices.
  // One edge per trip, picked by selects between register copies (pinned: an indexed pick would put the
  // arrays in scratch memory).
  double c0 = R[0], c1 = R[3], c2 = R[6], c3 = R[1], c4 = R[4], c5 = R[7], c6 = R[2], c7 = R[5], c8 = R[8];
  double h0 = s2[0], h1 = s2[1], h2 = s2[2];
  pin(c0); pin(c1); pin(c2); pin(c3); pin(c4); pin(c5); pin(c6); pin(c7); pin(c8);
  pin(h0); pin(h1); pin(h2);
#pragma unroll 1
  for (int e = 0; e < 12; e++) {
    const int k = e >> 2;
    const double sa = (e & 1) ? 1.0 : -1.0, sb = (e & 2) ? 1.0 : -1.0;
    // v = -s2_k on axis k, sa s2_i on i = k + 1, sb s2_j on j = k + 2 (mod 3)
    const double v0 = k == 0 ? -h0 : (k == 1 ? sb * h0 : sa * h0);
    const double v1 = k == 1 ? -h1 : (k == 2 ? sb * h1 : sa * h1);
    const double v2 = k == 2 ? -h2 : (k == 0 ? sb * h2 : sa * h2);
    const double len = 2 * (k == 0 ? h0 : (k == 1 ? h1 : h2));
    const double p[3] = {t[0] + c0 * v0 + c3 * v1 + c6 * v2, t[1] + c1 * v0 + c4 * v1 + c7 * v2,
                         t[2] + c2 * v0 + c5 * v1 + c8 * v2};
    const double d[3] = {len * (k == 0 ? c0 : (k == 1 ? c3 : c6)), len * (k == 0 ? c1 : (k == 1 ? c4 : c7)),
                         len * (k == 0 ? c2 : (k == 1 ? c5 : c8))};
    best = fmin(best, seg_box_disjoint_d2(p, d, s1));
  }
  // b1's vertices in b2's frame: u = R^T (v - t)
#pragma unroll 1
  for (int c = 0; c < 8; c++) {
    const double v[3] = {(c & 1) ? s1[0] : -s1[0], (c & 2) ? s1[1] : -s1[1], (c & 4) ? s1[2] : -s1[2]};
    const double w[3] = {v[0] - t[0], v[1] - t[1], v[2] - t[2]};
    double u[3];
    mul_matT_vec3(u, R, w);
    best = fmin(best, pt_box_d2(u, s2));
  }
  return sqrt(best);
}

// a geom against a plane (half-space below the plane's z axis): signed height of the geom's lowest point
__device__ __forceinline__ double plane_distance(const GeomT<double> &pl, int type, const GeomT<double> &g,
                                                 const double *s) {
  const double n[3] = {pl.m[2], pl.m[5], pl.m[8]};
  const double dif[3] = {g.pos[0] - pl.pos[0], g.pos[1] - pl.pos[1], g.pos[2] - pl.pos[2]};
  const double h = dot3(dif, n);
  if (type == GT_SPHERE) return h - s[0];
  if (type == GT_CAPSULE) {
    const double axis[3] = {g.m[2], g.m[5], g.m[8]};
    return h - s[1] * fabs(dot3(axis, n)) - s[0];
  }
  // box: its lowest corner sits sum_k s_k |axis_k . n| below the centre
  double low = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double ak[3] = {g.m[k], g.m[3 + k], g.m[6 + k]};
    low += s[k] * fabs(dot3(ak, n));
  }
  return h - low;
}

// signed distance of one candidate pair (cur moving, par its partner; the types are wave-uniform)
__device__ __forceinline__ double pair_distance(int tcur, const GeomT<double> &cur, const double *scur, int tpar,
                                                const GeomT<double> &par, const double *spar) {
  if (tpar == GT_PLANE) return plane_distance(par, tcur, cur, scur);
  if (tcur == GT_BOX && tpar == GT_BOX) return box_box_distance(cur, scur, par, spar);
  if (tcur == GT_BOX) return core_box_distance(tpar == GT_CAPSULE, par, spar, cur, scur);
  if (tpar == GT_BOX) return core_box_distance(tcur == GT_CAPSULE, cur, scur, par, spar);
  return core_core_distance(cur, scur, tcur == GT_CAPSULE, par, spar, tpar == GT_CAPSULE);
}

// The kernel's five modes: distances, clearance, clearance with the gradient epilogue, the list of near pairs, and
// the bubble measurement.
enum : int { DM_DIST = 0, DM_CLEAR, DM_GRAD, DM_NEAR, DM_SWEEP };

// DM_GRAD's and DM_NEAR's scratch, tables and outputs (mjpl_distance_grad.h)
struct GradOut {
  double *xpos, *xquat;  // body pose scratch rows (nbody per row), written by the FK
  int nbody;
  const double *gcol, *gjnt, *gtin;  // column table [nplan][GC_LEN], joint table [njnt][JR_LEN], tin per geom
  // DM_GRAD: [N][nplan], [N][6] (may be null), [N][3] (may be null), [N]; DM_NEAR: the same per slot, N * K of each
  double *grad, *fromto, *normal;
  int *status;
};

// DM_NEAR's own scratch and outputs, beside GradOut's (mjpl_distance_grad.h: near_step)
struct NearOut {
  double *frames;  // column frames scratch [rows][nplan][6]: world axis, anchor of every planning column's joint
  int K;           // slots per configuration
  int *count;      // [N]
  int *pair;       // [N][K]
  double *dist;    // [N][K]
};

// DM_SWEEP's inputs and outputs beside clear / pair (which hold gap and its pair)
struct SweepIO {
  const double *W;   // lever table [P][nplan], read wave-uniformly
  const double *HD;  // [N][nplan] in the batch's layout: how far column c may move from q, >= 0
  double *slack;     // [N]
  int *slack_pair;   // [N]
};

// DM_GRAD's epilogue (mjpl_distance_grad.h)
__device__ __forceinline__ void grad_epilogue(const GradOut &go, const Carve<double> &c, IP ct, DP cd, DP wcull,
                                              DP wnarrow, const double *rx, const double *rm, int64_t i, int64_t row,
                                              int nplan, bool live, int bestp, bool bestcap);
// DM_NEAR's column frames, once per lane before the walk, and its per-pair step (mjpl_distance_grad.h)
__device__ __forceinline__ void near_park_frames(const GradOut &go, const NearOut &no, const Carve<double> &c,
                                                 int64_t row, int nplan, bool active);
__device__ __forceinline__ void near_step(const GradOut &go, const NearOut &no, const PairGeoms &g, int p, double D,
                                          int64_t slot, int64_t row, int nplan, bool put);

// Configurations [i0, i0 + n) of the batch Q (N rows, `layout`), FK scratch rows as k_contacts uses them.
// DM_DIST: dist[i * P + p] = min(d_p, distmax).  DM_CLEAR: clear[i] = min over non-allowed p of
// (min(d_p, distmax) - margin_p), pair[i] = its lowest index (distmax, -1 without such a pair).  DM_GRAD: clear and
// pair as DM_CLEAR, the body poses also written to go's scratch rows, then go's outputs at row i.  A row with a
// non-finite planning column gives NaN (and pair -1).  DM_NEAR: the non-allowed pairs with d_p < distmax in
// ascending p: no.count[i] of them (-1 for a non-finite row), the first no.K in slots i * K + k of no.pair, no.dist and
// go's outputs, no.pair = -1 in the row's remaining slots (nothing else of those is written).  DM_SWEEP: with
// B_p = sum over c in ascending order of HD[i][c] * W[p][c] (terms with W == 0 or HD == 0 skipped, so inf times 0 never
// arises; inf stays inf), clear[i] = min over non-allowed p of (min(d_p, distmax) - margin_p) and pair[i] exactly as
// DM_CLEAR gives them, sw.slack[i] = min over non-allowed p of (min(d_p, distmax) - margin_p - B_p) and sw.slack_pair[i]
// its lowest index (distmax, -1 without such a pair; NaN, -1 for a non-finite row).  HD sits in the second column set
// of the LDS carve.
template <int MODE>
__global__ void __launch_bounds__(kBlock)
k_distance(const int *__restrict__ gip, int nip, const double *__restrict__ gdp, int ndp,
           const int *__restrict__ gct, const double *__restrict__ gcd, const double *__restrict__ gdt, int P,
           const double *__restrict__ Q, int64_t N, int64_t i0, int64_t n, int layout, double distmax,
           double *__restrict__ gx, double *__restrict__ gm, int ngeom, double *__restrict__ dist,
           double *__restrict__ clear, int *__restrict__ pair, GradOut go, NearOut no, SweepIO sw) {
  extern __shared__ double smem[];
  const int B = blockDim.x;
  const int nplan = gip[H_NPLAN];
  Carve<double> c = carve_lds<double>(smem, gip, nip, gdp, ndp, nplan, MODE == DM_SWEEP ? 2 : 1, B);
  const int64_t r = (int64_t)blockIdx.x * B + threadIdx.x;
  const bool active = r < n;
  const int64_t i = i0 + (active ? r : 0);
  load_columns(c.col0 + threadIdx.x, B, Q, N, i, nplan, layout, active);
  if constexpr (MODE == DM_SWEEP) load_columns(c.col1 + threadIdx.x, B, sw.HD, N, i, nplan, layout, active);
  __syncthreads();
  bool finite = true;
  for (int k = 0; k < nplan; k++) finite = finite && __builtin_isfinite(c.col0[k * B + threadIdx.x]);
  const bool live = active && finite;

  // 1. forward kinematics into the scratch row (DM_GRAD, DM_NEAR: the body poses too, for the column frames)
  FkOut out = {};
  out.geom_xpos = gx;
  out.geom_xmat = gm;
  out.ngeom = ngeom;
  if (MODE == DM_GRAD || MODE == DM_NEAR) {
    out.xpos = go.xpos;
    out.xquat = go.xquat;
    out.nbody = go.nbody;
  }
  run_config<double, 1, true, true, true>(c.ip, c.tp, c.col0 + threadIdx.x, B, c.save + threadIdx.x, B, active, 0.0,
                                          out, active ? r : 0);
  const double *rx = gx + (active ? r : 0) * ngeom * 3;
  const double *rm = gm + (active ? r : 0) * ngeom * 9;
  // DM_NEAR: every planning column's frame, parked in scratch for the pairs that pass
  if constexpr (MODE == DM_NEAR) near_park_frames(go, no, c, active ? r : 0, nplan, active);

  // 2. every candidate pair, in table order
  IP ct = (IP)gct;
  DP cd = (DP)gcd;
  DP dt = (DP)gdt;
  DP wcull = c.tp + uni(c.ip[H_OFF_WCULL]);
  DP wnarrow = c.tp + uni(c.ip[H_OFF_WNARROW]);
  double best = distmax;  // DM_CLEAR / DM_GRAD: least D - margin so far, at pair index bestp
  int bestp = -1;
  bool bestcap = true;  // DM_GRAD: the winner's D is distmax (a cap: no geometry to differentiate)
  int cnt = 0;          // DM_NEAR: near pairs so far
  double sbest = distmax;  // DM_SWEEP: least D - margin - B so far, at pair index sbestp
  int sbestp = -1;
  for (int p = 0; p < P; p++) {
    // (uniform: allowed pairs take no part in the clearance)
    if (MODE != DM_DIST && uni((int)dt[p * DT_LEN + DT_ALLOWED]) != 0) continue;
    const PairGeoms g = contact_load_pair<true>(ct, cd, p, rx, rm, wcull, wnarrow, active);
    const double margin = cd[p * CD_LEN + CD_MARGIN];
    // lower bound of the distance: bounding spheres, or the centre's height above a plane minus rb
    double lb;
    {
      const double dif[3] = {g.cur.pos[0] - g.par.pos[0], g.cur.pos[1] - g.par.pos[1], g.cur.pos[2] - g.par.pos[2]};
      const double rb = dt[p * DT_LEN + DT_RBSUM];
      if (g.tpar == GT_PLANE) {
        const double nrm[3] = {g.par.m[2], g.par.m[5], g.par.m[8]};
        lb = dot3(dif, nrm) - rb;
      } else {
        lb = sqrt(dot3(dif, dif)) - rb;
      }
    }
    const bool far = lb >= distmax + kDistCullSlack;  // D = distmax, no routine
    bool need = live && !far;
    // a pair whose D - margin must exceed the least so far cannot change (C, pair)
    if (MODE == DM_CLEAR || MODE == DM_GRAD) need = need && !(bestp >= 0 && lb >= best + margin + kDistCullSlack);
    double D = distmax;
    if (__builtin_amdgcn_ballot_w64(need) != 0ull) {
      const double x = pair_distance(g.tcur, g.cur, g.scur, g.tpar, g.par, g.spar);
      if (need) D = x < distmax ? x : distmax;
    }
    if constexpr (MODE == DM_DIST) {
      if (active) dist[i * P + p] = live ? D : NAN;
    } else if constexpr (MODE == DM_NEAR) {
      // near: the comparison that made D the distance and not the cap.  Every near lane counts; the lanes with a
      // slot left take the witness step together (the pair's types are wave-uniform, only the lane mask differs).
      const bool near = need && D < distmax;
      const bool put = near && cnt < no.K;
      if (__builtin_amdgcn_ballot_w64(put) != 0ull) near_step(go, no, g, p, D, i * no.K + cnt, active ? r : 0, nplan, put);
      if (near) cnt++;
    } else if constexpr (MODE == DM_SWEEP) {
      const double v = D - margin;
      double bp = 0.0;
      for (int k = 0; k < nplan; k++) {
        const double w = sw.W[(int64_t)p * nplan + k];
        if (w != 0.0) {  // (uniform)
          const double hd = c.col1[k * B + threadIdx.x];
          if (hd != 0.0) bp += hd * w;
        }
      }
      const double s = v - bp;
      if (live && (bestp < 0 || v < best)) {
        best = v;
        bestp = p;
      }
      if (live && (sbestp < 0 || s < sbest)) {
        sbest = s;
        sbestp = p;
      }
    } else {
      const double v = D - margin;
      if (live && (need || far) && (bestp < 0 || v < best)) {
        best = v;
        bestp = p;
        bestcap = !(D < distmax);
      }
    }
  }
  if constexpr (MODE == DM_NEAR) {
    if (!active) return;
    for (int k = cnt; k < no.K; k++) no.pair[i * no.K + k] = -1;
    no.count[i] = live ? cnt : -1;
  } else if constexpr (MODE != DM_DIST) {
    if (!active) return;
    clear[i] = live ? best : NAN;
    pair[i] = live ? bestp : -1;
    if constexpr (MODE == DM_SWEEP) {
      sw.slack[i] = live ? sbest : NAN;
      sw.slack_pair[i] = live ? sbestp : -1;
    }
    // 3. DM_GRAD: the epilogue (lanes diverge from here on)
    if constexpr (MODE == DM_GRAD)
      grad_epilogue(go, c, ct, cd, wcull, wnarrow, rx, rm, i, r, nplan, live, bestp, bestcap);
  }
}

}  // namespace mjpl
