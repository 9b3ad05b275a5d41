// mjpl_sweep.h -- certified edge checks: no contact anywhere along an edge (mjpl_sweep_edges*, include/mjpl_hip.h).
//
// What it adds: a verdict for the whole segment q(t) = QA + t (QB - QA), t in [0, 1], not for samples of it.  The
// measuring is not here: every round evaluates its open nodes with one k_distance<DM_SWEEP> launch (mjpl_distance.h),
// exactly as mjpl_sweep_measure* launches it.  This header holds the step between two measurements and the two small
// kernels around the loop.
//
// A node (edge, t, h) stands for the interval [t - h, t + h] of its edge: its row is q(t), its travel
// HD_c = h |QB_c - QA_c|.  Round 0 of an edge holds its end points (0, 0), (1, 0) and the root (1/2, 1/2); every node
// of round k >= 1 has h = 2^-(k+1) and t = (2 m + 1) h, m = its ordinal.  k_sweep_step gives every node of a round one
// lane (DESIGN.md section 5.11 states the rule): a hit goes into the edge's key with one atomicMin, a certified slack
// into clear_lb with one atomicMin on the bits of the positive double, and a node that must be split writes its two
// children -- rows, travels, (edge, ordinal) -- into the other work buffer: one ballot per wave, one atomic add per
// wave on the device counter the host reads to size the next round.  The packed order follows the order the waves reach
// the atomic and may differ from run to run; every node's arithmetic is its own and every per-edge result is a minimum,
// a maximum, a sum of ones or an idempotent store, so no result depends on it.
//
// An edge's key: depth << 48 | ordinal << 32 | gap_pair of a hit node, ~0 without one.  Its minimum is the hit of the
// first depth that has one with the least t there (ordinals grow with t).  A node of an edge whose key holds an
// EARLIER depth is dropped by the step before it counts: children written in the round their edge was hit in are
// measured once more and ignored.  (Within a round the key may change under the reader, between ~0 and this round's
// depth: neither is an earlier depth.)
//
// Certified trajectories (mjpl_sweep_splines*) run the same loop over the PIECES of natural cubic
// splines: piece k of a path is q_k(B), B in [0, 1], the cubic mjpl_topp.h evaluates (topp_eval).  Only the nodes differ
// -- a node's row is q_k(t), its travel the extent of the Bezier control points of the cubic on [t - h, t + h] around the
// row, inflated for their rounding (spline_node) -- and the decision gains the two bound tests a curve that can leave
// [lo, hi] between its waypoints needs.  sweep_decide is the one statement of the decision, for both kinds of node.
#pragma once

#include "mjpl_topp.h"  // topp_eval: q and q' of a spline piece

namespace mjpl {

constexpr int kSweepBlock = 64;             // one wave per workgroup: the packing needs no LDS
constexpr double kSweepSlack = 1e-9;        // a node is certified iff slack - d_min >= this
constexpr int64_t kSweepNodes = (int64_t)1 << 22;  // open nodes of a chunk's deepest round, at most
constexpr int kSweepMaxDepth = 16;
constexpr unsigned long long kSweepNoHit = ~0ull;
constexpr unsigned kSweepPairRange = 0xfffffffeu;  // the pair of a "hit" that is a row outside the bounds: -2

struct SweepWork {
  double *rows, *hd;  // [n][nplan] each
  int *meta;          // [n][2]: edge (batch index), ordinal
  int *n;             // fill counter
};

struct SweepArgs {
  const double *QA, *QB;  // the call's edges, E of them in `layout`
  int64_t E;
  int layout, nplan;
  const double *lo, *hi;  // [nplan] each (-inf / +inf where the caller gave none)
  double d_min;
  int max_depth;
  // per edge: hit keys [E - i0 of the chunk: indexed by edge - i0], and the call's outputs
  unsigned long long *key;
  int64_t i0;
  int *status, *nodes, *depth, *pair;
  double *t_hit;
  unsigned long long *clear_bits;  // clear_lb, as the bits of a positive double while the loop runs
};

// The pieces of a call's splines (mjpl_sweep_splines*): W and M packed [rows][nplan]; per piece (call-wide index) the row
// of its first waypoint and n - 1 of its path
struct SweepSpline {
  const double *W, *M;
  const int64_t *piece;  // [pieces][2]
};

__device__ __forceinline__ double sweep_at(const double *Q, int64_t E, int64_t i, int nplan, int layout, int c) {
  return layout == MJPL_SOA ? Q[(int64_t)c * E + i] : Q[i * nplan + c];
}

// Lanes with `put` set reserve `per` consecutive slots each in a work buffer: the first slot of this lane.
__device__ __forceinline__ int64_t sweep_reserve(bool put, int per, int *counter) {
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(put);
  if (mask == 0ull) return 0;
  const int first = (int)__builtin_ctzll(mask);
  const int lane = (int)(threadIdx.x & 63);
  int base = 0;
  if (lane == first) base = atomicAdd(counter, per * (int)__popcll(mask));
  base = __shfl(base, first);
  const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
  return (int64_t)base + (int64_t)per * before;
}

// The decision on one measured node of round `round` (the two bound tests: 5.13) -> whether it must be
// split.  `outside`: the node's row lies outside the bounds, which counts as a hit with pair -2 and is tested before
// contact; `box_outside`: its box leaves them, where the lever table does not hold, so it is never certified.  A node of
// a straight edge between two end points inside the bounds is neither.
__device__ __forceinline__ bool sweep_decide(const SweepArgs &a, int round, int ej, int ord, double g, int g_pair, double s,
                                             bool outside, bool box_outside) {
  const int64_t i = a.i0 + ej;
  // (an edge hit at an earlier depth: this node was written before the hit was known, and does not count)
  if ((int)(a.key[ej] >> 48) < round) return false;
  atomicAdd(a.nodes + i, 1);
  atomicMax(a.depth + i, round);
  const bool endpoint = round == 0 && ord != 1;
  const unsigned long long at = (unsigned long long)round << 48 | (unsigned long long)ord << 32;
  if (outside) {
    atomicMin(a.key + ej, at | kSweepPairRange);
  } else if (g <= 0.0 || g < a.d_min) {
    atomicMin(a.key + ej, at | (unsigned)g_pair);
  } else if (!box_outside && s - a.d_min >= kSweepSlack) {
    atomicMin(a.clear_bits + i, (unsigned long long)__double_as_longlong(s));
  } else if (endpoint || round >= a.max_depth) {
    a.status[i] = MJPL_SWEEP_UNDECIDED;
  } else {
    return true;
  }
  return false;
}

// Round 0 of the chunk's edges [i0, i0 + n): per-edge state, and three nodes for every finite edge inside the bounds.
__global__ void __launch_bounds__(kSweepBlock)
k_sweep_init(SweepArgs a, int n, SweepWork w) {
  const int j = blockIdx.x * kSweepBlock + threadIdx.x;
  const int64_t i = a.i0 + j;
  bool put = false;
  if (j < n) {
    bool finite = true, inside = true;
    for (int c = 0; c < a.nplan; c++) {
      const double qa = sweep_at(a.QA, a.E, i, a.nplan, a.layout, c), qb = sweep_at(a.QB, a.E, i, a.nplan, a.layout, c);
      finite = finite && __builtin_isfinite(qa) && __builtin_isfinite(qb);
      inside = inside && qa >= a.lo[c] && qa <= a.hi[c] && qb >= a.lo[c] && qb <= a.hi[c];
    }
    put = finite && inside;
    a.status[i] = !finite ? MJPL_SWEEP_NONFINITE : (!inside ? MJPL_SWEEP_RANGE : MJPL_SWEEP_FREE);
    a.nodes[i] = 0;
    a.depth[i] = 0;
    a.key[j] = kSweepNoHit;
    a.clear_bits[i] = 0x7ff0000000000000ull;  // +inf
  }
  const int64_t slot = sweep_reserve(put, 3, w.n);
  if (!put) return;
  for (int k = 0; k < 3; k++) {  // t = 0, 1/2, 1
    for (int c = 0; c < a.nplan; c++) {
      const double qa = sweep_at(a.QA, a.E, i, a.nplan, a.layout, c), qb = sweep_at(a.QB, a.E, i, a.nplan, a.layout, c);
      const double d = qb - qa;
      w.rows[(slot + k) * a.nplan + c] = k == 0 ? qa : (k == 2 ? qb : qa + 0.5 * d);
      w.hd[(slot + k) * a.nplan + c] = k == 1 ? 0.5 * fabs(d) : 0.0;
    }
    w.meta[2 * (slot + k)] = (int)j;
    w.meta[2 * (slot + k) + 1] = k;
  }
}

// One lane per node of round `round` (n of them in `cur`, measured: gap, gap_pair, slack at the node's position).
__global__ void __launch_bounds__(kSweepBlock)
k_sweep_step(SweepArgs a, int round, int n, SweepWork cur, const double *__restrict__ gap, const int *__restrict__ gap_pair,
             const double *__restrict__ slack, SweepWork next) {
  const int j = blockIdx.x * kSweepBlock + threadIdx.x;
  bool split = false;
  int ej = 0, ord = 0;
  if (j < n) {
    ej = cur.meta[2 * j];
    ord = cur.meta[2 * j + 1];
    split = sweep_decide(a, round, ej, ord, gap[j], gap_pair[j], slack[j], false, false);
  }
  const int64_t slot = sweep_reserve(split, 2, next.n);
  if (!split) return;
  // children (t -+ h/2, h/2): depth round + 1, ordinals 2 m and 2 m + 1 (the root of round 0 is m = 0)
  const int m = round == 0 ? 0 : ord;
  const double h = ldexp(1.0, -(round + 2));
  const int64_t i = a.i0 + ej;
  for (int k = 0; k < 2; k++) {
    const int co = 2 * m + k;
    const double t = (double)(2 * co + 1) * h;
    for (int c = 0; c < a.nplan; c++) {
      const double qa = sweep_at(a.QA, a.E, i, a.nplan, a.layout, c), qb = sweep_at(a.QB, a.E, i, a.nplan, a.layout, c);
      const double d = qb - qa;
      next.rows[(slot + k) * a.nplan + c] = qa + t * d;
      next.hd[(slot + k) * a.nplan + c] = h * fabs(d);
    }
    next.meta[2 * (slot + k)] = ej;
    next.meta[2 * (slot + k) + 1] = co;
  }
}

// ---- spline pieces (mjpl_sweep_splines*)
constexpr double kSweepHullRel = 1.0 + 0x1p-30;  // the inflation of a hull travel: relative ...
constexpr double kSweepHullAbs = 0x1p-40;        // ... and per unit of the piece's coefficients

// The node (t, h) of one column of a piece (W0, W1, M0, M1; r = n - 1): row = q(t) and the travel that holds the cubic on
// [a, b] = [t - h, t + h].  The cubic lies in the hull of its Bezier control points P0 = q(a), P1 = P0 + (b - a)/3 q'(a)/r,
// P2 = P3 - (b - a)/3 q'(b)/r, P3 = q(b) (q' is with respect to s: one piece is 1/r of it), so |q(B) - row| is at most
// the largest |P_j - row|.  One IEEE operation per operation of tests/spline_sweep_reference.py, in its order.
__device__ __forceinline__ void spline_node(double W0, double W1, double M0, double M1, double r, double t, double h, double &row,
                                            double &hd) {
  const double a = t - h, b = t + h;
  double P0, P3, d0, d3, d1, q2;
  topp_eval(W0, W1, M0, M1, r, t, row, d1, q2);
  topp_eval(W0, W1, M0, M1, r, a, P0, d0, q2);
  topp_eval(W0, W1, M0, M1, r, b, P3, d3, q2);
  const double w = (b - a) / 3.0;
  const double P1 = P0 + w * (d0 / r), P2 = P3 - w * (d3 / r);
  const double far = fmax(fmax(fmax(fabs(P0 - row), fabs(P1 - row)), fabs(P2 - row)), fabs(P3 - row));
  hd = far * kSweepHullRel + kSweepHullAbs * ((fabs(W0) + fabs(W1)) + (fabs(M0) + fabs(M1)) / (6.0 * r * r));
}

// Round 0 of the chunk's pieces [i0, i0 + n): per-piece state, and three nodes for every finite piece whose waypoints lie
// inside the bounds.  (A non-finite waypoint anywhere in a path makes every interior M of the path non-finite, and every
// piece holds an interior knot or both waypoints: the test per piece is the test per path.)
__global__ void __launch_bounds__(kSweepBlock)
k_sweep_spline_init(SweepArgs a, SweepSpline sp, int n, SweepWork w) {
  const int j = blockIdx.x * kSweepBlock + threadIdx.x;
  const int64_t i = a.i0 + j;
  bool put = false;
  int64_t at = 0;
  double r = 1.0;
  if (j < n) {
    at = sp.piece[2 * i] * a.nplan;
    r = (double)sp.piece[2 * i + 1];
    bool finite = true, inside = true;
    for (int c = 0; c < a.nplan; c++) {
      const double W0 = sp.W[at + c], W1 = sp.W[at + a.nplan + c];
      finite = finite && __builtin_isfinite(W0) && __builtin_isfinite(W1) && __builtin_isfinite(sp.M[at + c]) &&
               __builtin_isfinite(sp.M[at + a.nplan + c]);
      inside = inside && W0 >= a.lo[c] && W0 <= a.hi[c] && W1 >= a.lo[c] && W1 <= a.hi[c];
    }
    put = finite && inside;
    a.status[i] = !finite ? MJPL_SWEEP_NONFINITE : (!inside ? MJPL_SWEEP_RANGE : MJPL_SWEEP_FREE);
    a.nodes[i] = 0;
    a.depth[i] = 0;
    a.key[j] = kSweepNoHit;
    a.clear_bits[i] = 0x7ff0000000000000ull;  // +inf
  }
  const int64_t slot = sweep_reserve(put, 3, w.n);
  if (!put) return;
  for (int c = 0; c < a.nplan; c++) {  // t = 0, 1/2, 1: the end points are the waypoints themselves
    const double W0 = sp.W[at + c], W1 = sp.W[at + a.nplan + c];
    double row, hd;
    spline_node(W0, W1, sp.M[at + c], sp.M[at + a.nplan + c], r, 0.5, 0.5, row, hd);
    w.rows[slot * a.nplan + c] = W0;
    w.rows[(slot + 1) * a.nplan + c] = row;
    w.rows[(slot + 2) * a.nplan + c] = W1;
    w.hd[slot * a.nplan + c] = 0.0;
    w.hd[(slot + 1) * a.nplan + c] = hd;
    w.hd[(slot + 2) * a.nplan + c] = 0.0;
  }
  for (int k = 0; k < 3; k++) {
    w.meta[2 * (slot + k)] = (int)j;
    w.meta[2 * (slot + k) + 1] = k;
  }
}

// k_sweep_step for spline pieces: the node's own row and travel (written by the round before) against the bounds, the
// decision, and the children's rows and hull travels from the piece's coefficients.
__global__ void __launch_bounds__(kSweepBlock)
k_sweep_spline_step(SweepArgs a, SweepSpline sp, int round, int n, SweepWork cur, const double *__restrict__ gap,
                    const int *__restrict__ gap_pair, const double *__restrict__ slack, SweepWork next) {
  const int j = blockIdx.x * kSweepBlock + threadIdx.x;
  bool split = false;
  int ej = 0, ord = 0;
  if (j < n) {
    ej = cur.meta[2 * j];
    ord = cur.meta[2 * j + 1];
    bool outside = false, box_outside = false;
    for (int c = 0; c < a.nplan; c++) {
      const double row = cur.rows[(int64_t)j * a.nplan + c], hd = cur.hd[(int64_t)j * a.nplan + c];
      outside = outside || !(row >= a.lo[c] && row <= a.hi[c]);
      box_outside = box_outside || row - hd < a.lo[c] || row + hd > a.hi[c];
    }
    split = sweep_decide(a, round, ej, ord, gap[j], gap_pair[j], slack[j], outside, box_outside);
  }
  const int64_t slot = sweep_reserve(split, 2, next.n);
  if (!split) return;
  const int m = round == 0 ? 0 : ord;
  const double h = ldexp(1.0, -(round + 2));
  const int64_t i = a.i0 + ej, at = sp.piece[2 * i] * a.nplan;
  const double r = (double)sp.piece[2 * i + 1];
  for (int k = 0; k < 2; k++) {
    const int co = 2 * m + k;
    const double t = (double)(2 * co + 1) * h;
    for (int c = 0; c < a.nplan; c++) {
      double row, hd;
      spline_node(sp.W[at + c], sp.W[at + a.nplan + c], sp.M[at + c], sp.M[at + a.nplan + c], r, t, h, row, hd);
      next.rows[(slot + k) * a.nplan + c] = row;
      next.hd[(slot + k) * a.nplan + c] = hd;
    }
    next.meta[2 * (slot + k)] = ej;
    next.meta[2 * (slot + k) + 1] = co;
  }
}

// The chunk's verdicts from the per-edge state.
__global__ void __launch_bounds__(256)
k_sweep_finish(SweepArgs a, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t i = a.i0 + j;
  const int s = a.status[i];
  const unsigned long long key = a.key[j];
  const bool measured = s != MJPL_SWEEP_NONFINITE && s != MJPL_SWEEP_RANGE;
  const bool hit = measured && key != kSweepNoHit;
  double t = NAN;
  if (hit) {
    const int k = (int)(key >> 48), ord = (int)((key >> 32) & 0xffffu);
    t = k == 0 ? 0.5 * ord : (double)(2 * ord + 1) * ldexp(1.0, -(k + 1));
    // (a spline piece whose row left the bounds there: RANGE, with pair -2)
    a.status[i] = (unsigned)(key & 0xffffffffu) == kSweepPairRange ? MJPL_SWEEP_RANGE : MJPL_SWEEP_HIT;
  }
  a.t_hit[i] = t;
  a.pair[i] = hit ? (int)(unsigned)(key & 0xffffffffu) : -1;
  if (!(measured && !hit && s == MJPL_SWEEP_FREE)) a.clear_bits[i] = 0x7ff8000000000000ull;  // NaN unless FREE
}

}  // namespace mjpl
