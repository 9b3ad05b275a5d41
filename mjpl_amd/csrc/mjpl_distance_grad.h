// mjpl_distance_grad.h -- clearance gradients and witness points per configuration (mjpl_clearance_grad*), and the
// same for every pair within distmax (mjpl_near_pairs*, at the end of the file).
//
// The clearance gradients are k_distance<DM_GRAD> (mjpl_distance.h): the clearance kernel's walk itself, with the
// body poses also written to scratch and this file's epilogue after it.
//   1. The walk is DM_CLEAR's (same FK, table walk, cull and winner's comparisons), so clear and pair come out
//      bit-identical to mjpl_clearance (tests/test_gpu_clearance_grad.py compares the bytes).
//   2. Once per lane, the winner's pair is measured again by a witness variant of its routine, which keeps the
//      argmin feature beside each minimum: (w_cur, w_par, n) with n the unit vector from cur towards par and
//      w_par - w_cur = D n.  The pair types differ per lane, so this step diverges once per lane.
//   3. grad_j = n . (v_j(w2) - v_j(w1)) over the planning columns, v_j(x) = axis_j x (x - anchor_j) (hinge) or
//      axis_j (slide), 0 unless column j's body is the point's body or an ancestor.  Axis and anchor come from
//      the body pose FK wrote to scratch and the per-engine column table (mjpl_compile.h: build_grad_table).
//
// Witnesses.  Disjoint cores: the closest points of the minimising feature pair (end point, segment interior,
// box vertex, box edge), pushed out by the radii along n.  Overlapping cores: the separating axis u of least
// overlap o is known; the core of par is moved by o u (it then touches cur's core), the closest points of the
// touching pair are found by the disjoint enumeration, and the moved point is moved back.  Those are the two ends
// of the shortest separating translation.  A plane: the geom's lowest point and its projection on the plane.
#pragma once

namespace mjpl {

// status of a configuration (include/mjpl_hip.h: MJPL_GRAD_*)
enum : int { GS_OK = 0, GS_FLAT = 1, GS_DEGENERATE = 2, GS_NONFINITE = 3 };
// a core gap below this (metres) has no direction: MJPL_GRAD_DEGENERATE
constexpr double kGradDegenerate = 1e-10;

// column table (per planning column) and joint table (per model joint), mjpl_compile.h: build_grad_table.
// A column's joint j sits on body GC_BODY; the body's joints after j (GC_NLATER of them, model joints
// j + 1 ...) are undone from the body's final pose to get the frame j moved.  GC_TIN / GC_TOUT: the body's
// subtree as an interval of DFS entry times (geom g is moved by the column iff tin(body(g)) lies in it).
enum : int { GC_BODY = 0, GC_JNT, GC_NLATER, GC_TIN, GC_TOUT, GC_LEN };
enum : int { JR_TYPE = 0, JR_AXIS, JR_POS = 4, JR_COL = 7, JR_Q0, JR_LEN };  // dq = q[col] - q0, or q0 (col < 0)

__device__ __forceinline__ void set3(double *o, const double *a) { o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; }
__device__ __forceinline__ void cross3(double *o, const double *a, const double *b) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// seg_box_disjoint_d2 with the closest points: cs on the segment p + t d, cb on the box (box frame).  (An enumeration
// of its own, as box_box_cp's: `x < best` keeps a NaN that comes first where seg_box_disjoint_d2's fmin drops it.)
__device__ __forceinline__ double seg_box_cp(const double *p, const double *d, const double *s, double *cs, double *cb) {
  const double q[3] = {p[0] + d[0], p[1] + d[1], p[2] + d[2]};
  double best = pt_box_d2(p, s, cb);
  set3(cs, p);
  {
    double c[3];
    const double x = pt_box_d2(q, s, c);
    if (x < best) { best = x; set3(cs, q); set3(cb, c); }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;
#pragma unroll 1
    for (int qq = 0; qq < 4; qq++) {
      double a[3], e[3], c1[3], c2[3];
      a[k] = -s[k];
      a[i] = (qq & 1) ? s[i] : -s[i];
      a[j] = (qq & 2) ? s[j] : -s[j];
      e[k] = 2 * s[k];
      e[i] = 0.0;
      e[j] = 0.0;
      const double x = seg_seg_d2(p, d, a, e, c1, c2);
      if (x < best) { best = x; set3(cs, c1); set3(cb, c2); }
    }
  }
  return best;
}

// unit vector from a to b; false (v untouched) when they are closer than kGradDegenerate
__device__ __forceinline__ bool unit_from_to(const double *a, const double *b, double *v) {
  const double w[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double len = sqrt(dot3(w, w));
  if (!(len >= kGradDegenerate)) return false;
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = w[k] / len;
  return true;
}

// Witnesses of point or segment cores (core_core_distance): wa on g1, wb on g2, n from g1 to g2.
__device__ __forceinline__ int core_core_witness(const GeomT<double> &g1, const double *s1, bool seg1,
                                                 const GeomT<double> &g2, const double *s2, bool seg2, double *wa,
                                                 double *wb, double *n) {
  const double h1 = seg1 ? s1[1] : 0.0, h2 = seg2 ? s2[1] : 0.0;
  double p1[3], d1[3], p2[3], d2[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    d1[k] = 2 * h1 * g1.m[3 * k + 2];
    d2[k] = 2 * h2 * g2.m[3 * k + 2];
    p1[k] = g1.pos[k] - h1 * g1.m[3 * k + 2];
    p2[k] = g2.pos[k] - h2 * g2.m[3 * k + 2];
  }
  double c1[3], c2[3];
  double w2 = seg_seg_d2(p1, d1, p2, d2, c1, c2);
  if (seg1 && seg2) {  // the end points against the other segment, as core_core_distance takes them
    const double q1[3] = {p1[0] + d1[0], p1[1] + d1[1], p1[2] + d1[2]};
    const double q2[3] = {p2[0] + d2[0], p2[1] + d2[1], p2[2] + d2[2]};
    double c[3], x;
    x = pt_seg_d2(p1, p2, d2, c);
    if (x < w2) { w2 = x; set3(c1, p1); set3(c2, c); }
    x = pt_seg_d2(q1, p2, d2, c);
    if (x < w2) { w2 = x; set3(c1, q1); set3(c2, c); }
    x = pt_seg_d2(p2, p1, d1, c);
    if (x < w2) { w2 = x; set3(c1, c); set3(c2, p2); }
    x = pt_seg_d2(q2, p1, d1, c);
    if (x < w2) { w2 = x; set3(c1, c); set3(c2, q2); }
  }
  if (!unit_from_to(c1, c2, n)) {  // (the core points themselves)
    set3(wa, c1);
    set3(wb, c2);
    return GS_DEGENERATE;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    wa[k] = c1[k] + s1[0] * n[k];
    wb[k] = c2[k] - s2[0] * n[k];
  }
  return GS_OK;
}

// Witnesses of a sphere / capsule core (g) against a box (core_box_distance): wa on g, wb on the box, n from g
// to the box.  Everything in the box frame until the end.
__device__ __forceinline__ int core_box_witness(bool seg, const GeomT<double> &g, const double *sg,
                                                const GeomT<double> &box, const double *sb, double *wa, double *wb,
                                                double *n) {
  const double tmp[3] = {g.pos[0] - box.pos[0], g.pos[1] - box.pos[1], g.pos[2] - box.pos[2]};
  double m[3];
  mul_matT_vec3(m, box.m, tmp);
  double h[3] = {0, 0, 0};
  if (seg) {
    const double axis[3] = {g.m[2], g.m[5], g.m[8]};
    double a[3];
    mul_matT_vec3(a, box.m, axis);
#pragma unroll
    for (int k = 0; k < 3; k++) h[k] = a[k] * sg[1];
  }
  // separating axes (seg_box_sat's, a point has only the face normals): least overlap o, its unit axis u
  // pointing from the box towards the core
  double o = INFINITY, u[3] = {0, 0, 0};
  bool sep = false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double ok = sb[k] + fabs(h[k]) - fabs(m[k]);
    sep = sep || ok < 0;
    if (ok < o) {
      o = ok;
      u[0] = u[1] = u[2] = 0.0;
      u[k] = m[k] >= 0 ? 1.0 : -1.0;
    }
  }
  if (seg) {
    const double hh = dot3(h, h);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int i = (k + 1) % 3, j = (k + 2) % 3;
      const double nn = h[i] * h[i] + h[j] * h[j];
      if (nn > 1e-12 * hh) {
        const double rad = sb[i] * fabs(h[j]) + sb[j] * fabs(h[i]);
        const double proj = h[j] * m[i] - h[i] * m[j];
        const double len = sqrt(nn);
        const double ok = (rad - fabs(proj)) / len;
        sep = sep || ok < 0;
        if (ok < o) {  // n = h x e_k: n_k = 0, n_i = h_j, n_j = -h_i
          o = ok;
          const double sg1 = proj >= 0 ? 1.0 : -1.0;
          u[k] = 0.0;
          u[i] = sg1 * h[j] / len;
          u[j] = -sg1 * h[i] / len;
        }
      }
    }
  }
  // core points (box frame): cs on the core, cb on the box
  double cs[3], cb[3];
  const double shift = sep ? 0.0 : o;  // overlapping: move the core out by o u, measure, move it back
  const double p[3] = {m[0] - h[0] + shift * u[0], m[1] - h[1] + shift * u[1], m[2] - h[2] + shift * u[2]};
  const double d[3] = {2 * h[0], 2 * h[1], 2 * h[2]};
  if (seg) {
    (void)seg_box_cp(p, d, sb, cs, cb);
  } else {
    (void)pt_box_d2(p, sb, cb);
    set3(cs, p);
  }
  int st = GS_OK;
  double nl[3];  // from the core towards the box
  if (sep) {
    if (!unit_from_to(cs, cb, nl)) st = GS_DEGENERATE;
  } else {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      nl[k] = -u[k];
      cs[k] -= shift * u[k];
    }
  }
  double la[3], lb[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    la[k] = st == GS_OK ? cs[k] + sg[0] * nl[k] : cs[k];
    lb[k] = cb[k];
  }
  mul_mat_vec3(wa, box.m, la);
  mul_mat_vec3(wb, box.m, lb);
  mul_mat_vec3(n, box.m, nl);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    wa[k] += box.pos[k];
    wb[k] += box.pos[k];
  }
  return st;
}

// closest points of two disjoint (or touching) boxes, in b1's frame: b2 = centre t, axes the columns of R
// (box_box_distance's enumeration): c1 on b1, c2 on b2
__device__ __forceinline__ void box_box_cp(const double *R, const double *t, const double *s1, const double *s2,
                                           double *c1, double *c2) {
  double best = INFINITY;
  double c0 = R[0], cc1 = R[3], c2r = R[6], c3 = R[1], c4 = R[4], c5 = R[7], c6 = R[2], c7 = R[5], c8 = R[8];
  double h0 = s2[0], h1 = s2[1], h2 = s2[2];
  pin(c0); pin(cc1); pin(c2r); pin(c3); pin(c4); pin(c5); pin(c6); pin(c7); pin(c8);
  pin(h0); pin(h1); pin(h2);
#pragma unroll 1
  for (int e = 0; e < 12; e++) {
    const int k = e >> 2;
    const double sa = (e & 1) ? 1.0 : -1.0, sb = (e & 2) ? 1.0 : -1.0;
    const double v0 = k == 0 ? -h0 : (k == 1 ? sb * h0 : sa * h0);
    const double v1 = k == 1 ? -h1 : (k == 2 ? sb * h1 : sa * h1);
    const double v2 = k == 2 ? -h2 : (k == 0 ? sb * h2 : sa * h2);
    const double len = 2 * (k == 0 ? h0 : (k == 1 ? h1 : h2));
    const double p[3] = {t[0] + c0 * v0 + c3 * v1 + c6 * v2, t[1] + cc1 * v0 + c4 * v1 + c7 * v2,
                         t[2] + c2r * v0 + c5 * v1 + c8 * v2};
    const double d[3] = {len * (k == 0 ? c0 : (k == 1 ? c3 : c6)), len * (k == 0 ? cc1 : (k == 1 ? c4 : c7)),
                         len * (k == 0 ? c2r : (k == 1 ? c5 : c8))};
    double cs[3], cb[3];
    const double x = seg_box_cp(p, d, s1, cs, cb);
    if (x < best) { best = x; set3(c2, cs); set3(c1, cb); }
  }
#pragma unroll 1
  for (int c = 0; c < 8; c++) {
    const double v[3] = {(c & 1) ? s1[0] : -s1[0], (c & 2) ? s1[1] : -s1[1], (c & 4) ? s1[2] : -s1[2]};
    const double w[3] = {v[0] - t[0], v[1] - t[1], v[2] - t[2]};
    double uu[3], cl[3];
    mul_matT_vec3(uu, R, w);
    const double x = pt_box_d2(uu, s2, cl);
    if (x < best) {
      best = x;
      set3(c1, v);
      double y[3];
      mul_mat_vec3(y, R, cl);
#pragma unroll
      for (int k = 0; k < 3; k++) c2[k] = t[k] + y[k];
    }
  }
}

// Witnesses of two boxes (box_box_distance): wa on b1, wb on b2, n from b1 to b2
__device__ __forceinline__ int box_box_witness(const GeomT<double> &b1, const double *s1, const GeomT<double> &b2,
                                               const double *s2, double *wa, double *wb, double *n) {
  const double dp[3] = {b2.pos[0] - b1.pos[0], b2.pos[1] - b1.pos[1], b2.pos[2] - b1.pos[2]};
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) R[3 * i + j] = b1.m[i] * b2.m[j] + b1.m[3 + i] * b2.m[3 + j] + b1.m[6 + i] * b2.m[6 + j];
  mul_matT_vec3(t, b1.m, dp);
  // the 15 axes of box_box_distance, least overlap o and its unit axis u (b1 frame) pointing from b1 to b2
  double o = INFINITY, u[3] = {0, 0, 0};
  bool sep = false;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double ok = s1[i] + s2[0] * fabs(R[3 * i]) + s2[1] * fabs(R[3 * i + 1]) + s2[2] * fabs(R[3 * i + 2]) - fabs(t[i]);
    sep = sep || ok < 0;
    if (ok < o) {
      o = ok;
      u[0] = u[1] = u[2] = 0.0;
      u[i] = t[i] >= 0 ? 1.0 : -1.0;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double tj = t[0] * R[j] + t[1] * R[3 + j] + t[2] * R[6 + j];
    const double ok = s1[0] * fabs(R[j]) + s1[1] * fabs(R[3 + j]) + s1[2] * fabs(R[6 + j]) + s2[j] - fabs(tj);
    sep = sep || ok < 0;
    if (ok < o) {
      o = ok;
      const double sg = tj >= 0 ? 1.0 : -1.0;
      u[0] = sg * R[j];
      u[1] = sg * R[3 + j];
      u[2] = sg * R[6 + j];
    }
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
        const double len = sqrt(len2);
        const double ok = (ra + rb - fabs(tl)) / len;
        sep = sep || ok < 0;
        if (ok < o) {  // axis e_i x (b2's axis j): component i1 = -R[i2][j], i2 = R[i1][j]
          o = ok;
          const double sg = tl >= 0 ? 1.0 : -1.0;
          u[i] = 0.0;
          u[i1] = -sg * R[3 * i2 + j] / len;
          u[i2] = sg * R[3 * i1 + j] / len;
        }
      }
    }
  }
  const double shift = sep ? 0.0 : o;  // overlapping: move b2 out by o u, measure, move it back
  const double ts[3] = {t[0] + shift * u[0], t[1] + shift * u[1], t[2] + shift * u[2]};
  double c1[3], c2[3];
  box_box_cp(R, ts, s1, s2, c1, c2);
  int st = GS_OK;
  double nl[3];
  if (sep) {
    if (!unit_from_to(c1, c2, nl)) st = GS_DEGENERATE;
  } else {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      nl[k] = u[k];
      c2[k] -= shift * u[k];
    }
  }
  mul_mat_vec3(wa, b1.m, c1);
  mul_mat_vec3(wb, b1.m, c2);
  mul_mat_vec3(n, b1.m, nl);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    wa[k] += b1.pos[k];
    wb[k] += b1.pos[k];
  }
  return st;
}

// Witnesses of a geom g against a plane (plane_distance): wa = g's lowest point, wb its projection on the plane,
// n from g to the plane (minus the plane's normal)
__device__ __forceinline__ void plane_witness(const GeomT<double> &pl, int type, const GeomT<double> &g, const double *s,
                                              double *wa, double *wb, double *n) {
  const double nz[3] = {pl.m[2], pl.m[5], pl.m[8]};
  double low[3] = {g.pos[0], g.pos[1], g.pos[2]};
  if (type == GT_CAPSULE) {
    const double axis[3] = {g.m[2], g.m[5], g.m[8]};
    const double sg = dot3(axis, nz) >= 0 ? s[1] : -s[1];
#pragma unroll
    for (int k = 0; k < 3; k++) low[k] -= sg * axis[k];
  } else if (type == GT_BOX) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const double ak[3] = {g.m[j], g.m[3 + j], g.m[6 + j]};
      const double sg = dot3(ak, nz) >= 0 ? s[j] : -s[j];
#pragma unroll
      for (int k = 0; k < 3; k++) low[k] -= sg * ak[k];
    }
  }
  if (type != GT_BOX) {  // sphere and capsule: the radius below the core point
#pragma unroll
    for (int k = 0; k < 3; k++) low[k] -= s[0] * nz[k];
  }
  const double dif[3] = {low[0] - pl.pos[0], low[1] - pl.pos[1], low[2] - pl.pos[2]};
  const double h = dot3(dif, nz);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    wa[k] = low[k];
    wb[k] = low[k] - h * nz[k];
    n[k] = -nz[k];
  }
}

// pair_distance's dispatch, witnesses in the cur / par orientation (n from cur to par)
__device__ __forceinline__ int pair_witness(int tcur, const GeomT<double> &cur, const double *scur, int tpar,
                                            const GeomT<double> &par, const double *spar, double *wc, double *wp,
                                            double *n) {
  if (tpar == GT_PLANE) {
    plane_witness(par, tcur, cur, scur, wc, wp, n);
    return GS_OK;
  }
  if (tcur == GT_BOX && tpar == GT_BOX) return box_box_witness(cur, scur, par, spar, wc, wp, n);
  if (tcur == GT_BOX) {
    const int st = core_box_witness(tpar == GT_CAPSULE, par, spar, cur, scur, wp, wc, n);
#pragma unroll
    for (int k = 0; k < 3; k++) n[k] = -n[k];
    return st;
  }
  if (tpar == GT_BOX) return core_box_witness(tcur == GT_CAPSULE, cur, scur, par, spar, wc, wp, n);
  return core_core_witness(cur, scur, tcur == GT_CAPSULE, par, spar, tpar == GT_CAPSULE, wc, wp, n);
}

// world axis and anchor of column j's joint: its body's final pose (scratch) with the body's later joints undone
__device__ __forceinline__ void column_frame(const GradOut &go, DP col, const double *q, int qstride, int64_t row,
                                             double *axis, double *anchor, int *type) {
  const int b = uni((int)col[GC_BODY]), jnt = uni((int)col[GC_JNT]), nlater = uni((int)col[GC_NLATER]);
  const double *xp = go.xpos + (row * go.nbody + b) * 3;
  const double *xq = go.xquat + (row * go.nbody + b) * 4;
  double p[3] = {xp[0], xp[1], xp[2]}, qt[4] = {xq[0], xq[1], xq[2], xq[3]};
  for (int k = nlater; k >= 1; k--) {  // (wave-uniform: the table is)
    DP jr = (DP)go.gjnt + (jnt + k) * JR_LEN;
    const int jt = uni((int)jr[JR_TYPE]), jc = uni((int)jr[JR_COL]);
    const double dq = jc >= 0 ? q[jc * qstride] - jr[JR_Q0] : jr[JR_Q0];
    const double ja[3] = {jr[JR_AXIS], jr[JR_AXIS + 1], jr[JR_AXIS + 2]};
    if (jt == JT_SLIDE) {  // p = p' + R a dq
      double x[3];
      rot_vec_quat(x, ja, qt);
#pragma unroll
      for (int m = 0; m < 3; m++) p[m] -= x[m] * dq;
    } else {  // R = R' Rloc: R' = R Rloc^T, anchor p + R jp kept
      const double jp[3] = {jr[JR_POS], jr[JR_POS + 1], jr[JR_POS + 2]};
      double x[3], y[3];
      rot_vec_quat(x, jp, qt);
      const double sn = sin(dq * 0.5), cs = cos(dq * 0.5);
      const double qinv[4] = {cs, -ja[0] * sn, -ja[1] * sn, -ja[2] * sn};
      double nq[4];
      mul_quat(nq, qt, qinv);
#pragma unroll
      for (int m = 0; m < 4; m++) qt[m] = nq[m];
      rot_vec_quat(y, jp, qt);
#pragma unroll
      for (int m = 0; m < 3; m++) p[m] += x[m] - y[m];
    }
  }
  DP jr = (DP)go.gjnt + jnt * JR_LEN;
  *type = uni((int)jr[JR_TYPE]);
  const double ja[3] = {jr[JR_AXIS], jr[JR_AXIS + 1], jr[JR_AXIS + 2]};
  const double jp[3] = {jr[JR_POS], jr[JR_POS + 1], jr[JR_POS + 2]};
  rot_vec_quat(axis, ja, qt);
  rot_vec_quat(anchor, jp, qt);
#pragma unroll
  for (int m = 0; m < 3; m++) anchor[m] += p[m];
}

// The epilogue, once per active lane after the walk: FLAT / NONFINITE rows when there is nothing to differentiate,
// otherwise the winner's witnesses, normal, status and gradient.
__device__ __forceinline__ void grad_epilogue(const GradOut &go, const Carve<double> &c, IP ct, DP cd, DP wcull,
                                              DP wnarrow, const double *rx, const double *rm, int64_t i, int64_t row,
                                              int nplan, bool live, int bestp, bool bestcap) {
  if (!live || bestp < 0 || bestcap) {
    for (int j = 0; j < nplan; j++) go.grad[i * nplan + j] = live ? 0.0 : NAN;
    if (go.fromto)
      for (int k = 0; k < 6; k++) go.fromto[i * 6 + k] = NAN;
    if (go.normal)
      for (int k = 0; k < 3; k++) go.normal[i * 3 + k] = NAN;
    go.status[i] = live ? GS_FLAT : GS_NONFINITE;
    return;
  }
  const int B = blockDim.x;
  double *grad = go.grad + i * nplan;
  // the winner, loaded as the walk loads it (the index differs per lane here)
  const PairGeoms g = contact_load_pair<false>(ct, cd, bestp, rx, rm, wcull, wnarrow, true);
  // (copies of their own: pair_witness picks between the two geoms per lane, which would keep g out of registers)
  const GeomT<double> cur = g.cur, par = g.par;
  const double scur[3] = {g.scur[0], g.scur[1], g.scur[2]}, spar[3] = {g.spar[0], g.spar[1], g.spar[2]};
  double wc[3], wp[3], n[3];
  const int st = pair_witness(g.tcur, cur, scur, g.tpar, par, spar, wc, wp, n);
  // the candidate table's orientation: g1 = par when CF_PFIRST
  const bool pfirst = (g.flags & CF_PFIRST) != 0;
  double w1[3], w2[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    w1[k] = pfirst ? wp[k] : wc[k];
    w2[k] = pfirst ? wc[k] : wp[k];
    n[k] = st != GS_OK ? NAN : (pfirst ? -n[k] : n[k]);
  }
  if (go.fromto)
    for (int k = 0; k < 3; k++) {
      go.fromto[i * 6 + k] = w1[k];
      go.fromto[i * 6 + 3 + k] = w2[k];
    }
  if (go.normal)
    for (int k = 0; k < 3; k++) go.normal[i * 3 + k] = n[k];
  go.status[i] = st;
  // dclear/dq_j = n . (v_j(w2) [g2 moved by j] - v_j(w1) [g1 moved by j])
  const double tin1 = go.gtin[pfirst ? g.gparid : g.gcur], tin2 = go.gtin[pfirst ? g.gcur : g.gparid];
  const double *q = c.col0 + threadIdx.x;
  for (int j = 0; j < nplan; j++) {
    DP col = (DP)go.gcol + j * GC_LEN;
    const double lo = col[GC_TIN], hi = col[GC_TOUT];
    const bool m1 = tin1 >= lo && tin1 < hi, m2 = tin2 >= lo && tin2 < hi;
    double gj = 0.0;
    if (m1 || m2) {
      double axis[3], anchor[3];
      int jt;
      column_frame(go, col, q, B, row, axis, anchor, &jt);
      double v1[3], v2[3];
      if (jt == JT_SLIDE) {
        set3(v1, axis);
        set3(v2, axis);
      } else {
        const double r1[3] = {w1[0] - anchor[0], w1[1] - anchor[1], w1[2] - anchor[2]};
        const double r2[3] = {w2[0] - anchor[0], w2[1] - anchor[1], w2[2] - anchor[2]};
        cross3(v1, axis, r1);
        cross3(v2, axis, r2);
      }
      gj = (m2 ? dot3(n, v2) : 0.0) - (m1 ? dot3(n, v1) : 0.0);
    }
    grad[j] = st != GS_OK ? NAN : gj;
  }
}

// ---- near pairs (mjpl_near_pairs*): k_distance<DM_NEAR>
// The distances' walk (DM_DIST's cull, allowed pairs skipped), and for every pair below distmax what the epilogue above
// gives for the winner alone.  The pair index is wave-uniform in the walk, so pair_witness runs here with uniform types:
// one routine per pair for the whole wave, under the mask of the lanes that list the pair -- not the per-lane type
// divergence of the epilogue.  What differs per lane is the configuration, so the column frames are made once per lane
// before the walk and parked in global scratch (54 doubles per lane at nplan = 9: too much for LDS beside the carve,
// and a runtime-indexed private array would live in scratch memory anyway).

// Before the walk: axis and anchor of every planning column's joint for this lane's configuration, to its scratch row
__device__ __forceinline__ void near_park_frames(const GradOut &go, const NearOut &no, const Carve<double> &c,
                                                 int64_t row, int nplan, bool active) {
  const double *q = c.col0 + threadIdx.x;
  double *fr = no.frames + row * nplan * 6;
  for (int j = 0; j < nplan; j++) {
    double axis[3], anchor[3];
    int jt;
    column_frame(go, (DP)go.gcol + j * GC_LEN, q, blockDim.x, row, axis, anchor, &jt);
    if (active) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        fr[j * 6 + k] = axis[k];
        fr[j * 6 + 3 + k] = anchor[k];
      }
    }
  }
}

// One near pair of the walk (g: the pair as the walk loaded it, p and its types wave-uniform; D: its distance), run by
// the whole wave when any lane lists it: witnesses, then the epilogue's orientation and gradient statements with the
// parked frames.  Lanes with `put` store slot `slot` (= i * K + the lane's count, below K); the others store nothing.
__device__ __forceinline__ void near_step(const GradOut &go, const NearOut &no, const PairGeoms &g, int p, double D,
                                          int64_t slot, int64_t row, int nplan, bool put) {
  // (copies of their own, as in the epilogue: pair_witness hands the two geoms to its routines in either order, and
  //  what that keeps out of registers should be these, made for a near pair only, not the walk's g)
  const GeomT<double> cur = g.cur, par = g.par;
  const double scur[3] = {g.scur[0], g.scur[1], g.scur[2]}, spar[3] = {g.spar[0], g.spar[1], g.spar[2]};
  double wc[3], wp[3], n[3];
  const int st = pair_witness(g.tcur, cur, scur, g.tpar, par, spar, wc, wp, n);
  // the candidate table's orientation: g1 = par when CF_PFIRST
  const bool pfirst = (g.flags & CF_PFIRST) != 0;
  double w1[3], w2[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    w1[k] = pfirst ? wp[k] : wc[k];
    w2[k] = pfirst ? wc[k] : wp[k];
    n[k] = st != GS_OK ? NAN : (pfirst ? -n[k] : n[k]);
  }
  if (put) {
    no.pair[slot] = p;
    no.dist[slot] = D;
    go.status[slot] = st;
    if (go.fromto)
      for (int k = 0; k < 3; k++) {
        go.fromto[slot * 6 + k] = w1[k];
        go.fromto[slot * 6 + 3 + k] = w2[k];
      }
    if (go.normal)
      for (int k = 0; k < 3; k++) go.normal[slot * 3 + k] = n[k];
  }
  // d d_p/dq_j = n . (v_j(w2) [g2 moved by j] - v_j(w1) [g1 moved by j]); which columns move the pair is wave-uniform
  const double tin1 = go.gtin[pfirst ? g.gparid : g.gcur], tin2 = go.gtin[pfirst ? g.gcur : g.gparid];
  const double *fr = no.frames + row * nplan * 6;
  for (int j = 0; j < nplan; j++) {
    DP col = (DP)go.gcol + j * GC_LEN;
    const double lo = col[GC_TIN], hi = col[GC_TOUT];
    const bool m1 = tin1 >= lo && tin1 < hi, m2 = tin2 >= lo && tin2 < hi;
    double gj = 0.0;
    if (m1 || m2) {
      const int jt = uni((int)((DP)go.gjnt + uni((int)col[GC_JNT]) * JR_LEN)[JR_TYPE]);
      const double axis[3] = {fr[j * 6], fr[j * 6 + 1], fr[j * 6 + 2]};
      const double anchor[3] = {fr[j * 6 + 3], fr[j * 6 + 4], fr[j * 6 + 5]};
      double v1[3], v2[3];
      if (jt == JT_SLIDE) {
        set3(v1, axis);
        set3(v2, axis);
      } else {
        const double r1[3] = {w1[0] - anchor[0], w1[1] - anchor[1], w1[2] - anchor[2]};
        const double r2[3] = {w2[0] - anchor[0], w2[1] - anchor[1], w2[2] - anchor[2]};
        cross3(v1, axis, r1);
        cross3(v2, axis, r2);
      }
      gj = (m2 ? dot3(n, v2) : 0.0) - (m1 ? dot3(n, v1) : 0.0);
    }
    if (put) go.grad[slot * nplan + j] = st != GS_OK ? NAN : gj;
  }
}

}  // namespace mjpl
