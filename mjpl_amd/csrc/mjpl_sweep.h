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
#pragma once

namespace mjpl {

constexpr int kSweepBlock = 64;             // one wave per workgroup: the packing needs no LDS
constexpr double kSweepSlack = 1e-9;        // a node is certified iff slack - d_min >= this
constexpr int64_t kSweepNodes = (int64_t)1 << 22;  // open nodes of a chunk's deepest round, at most
constexpr int kSweepMaxDepth = 16;
constexpr unsigned long long kSweepNoHit = ~0ull;

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
    const int64_t i = a.i0 + ej;
    // (an edge hit at an earlier depth: this node was written before the hit was known, and does not count)
    if ((int)(a.key[ej] >> 48) >= round) {
      atomicAdd(a.nodes + i, 1);
      atomicMax(a.depth + i, round);
      const double g = gap[j], s = slack[j];
      const bool endpoint = round == 0 && ord != 1;
      if (g <= 0.0 || g < a.d_min) {
        atomicMin(a.key + ej, (unsigned long long)round << 48 | (unsigned long long)ord << 32 | (unsigned)gap_pair[j]);
      } else if (s - a.d_min >= kSweepSlack) {
        atomicMin(a.clear_bits + i, (unsigned long long)__double_as_longlong(s));
      } else if (endpoint || round >= a.max_depth) {
        a.status[i] = MJPL_SWEEP_UNDECIDED;
      } else {
        split = true;
      }
    }
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
    a.status[i] = MJPL_SWEEP_HIT;
  }
  a.t_hit[i] = t;
  a.pair[i] = hit ? (int)(unsigned)(key & 0xffffffffu) : -1;
  if (!(measured && !hit && s == MJPL_SWEEP_FREE)) a.clear_bits[i] = 0x7ff8000000000000ull;  // NaN unless FREE
}

}  // namespace mjpl
