// mjpl_plan.h -- batched planning (mjpl_plan_paths*, include/mjpl_hip.h).
//
// What it adds: "these B start/goal pairs, planned in lockstep".  Every problem grows two trees, one from each end, by a
// bidirectional RRT whose rounds all problems take together: per round a problem proposes one connect edge (the closest
// pair between the nodes the other tree gained last round and the growing tree) and up to 64 extensions towards seeded
// uniform targets, every edge of every problem is validated by ONE launch of the edge pipeline (launch_edges,
// mjpl_hip.hip), and the problem commits: solved by the connect edge, or the valid extensions appended.
// tests/plan_reference.py is the NumPy statement of every number and decision below, operation for operation;
// DESIGN.md 5.16 has the reasoning.  All float64, -ffp-contract=off.  The only atomics are integer ones on the round's
// header (a sum, a maximum of bit patterns, a count): their results do not depend on the order.
//
// One wave per problem in every kernel, kPlanWaves problems per workgroup; no workgroup barrier anywhere.  The direct
// edge QI -> QG is validated as round -1: a round whose connect edge is given and which has no extensions.  Kernels, in
// launch order:
//   k_plan_init     the NaN / inf scan of the two ends, the roots T0[0] = QI and T1[0] = QG, the ends as two rows of the
//                   configuration batch (zeros for a non-finite problem: its verdict is not read), the counters.
//   (launch_configs: the ends' verdicts)
//   k_plan_propose  round -1: an invalid end retires the problem; the direct edge.  Round r >= 0: a full growing tree
//                   retires the problem (NODES); lane l = connect candidate l (the l-th of the nodes the other tree
//                   gained) and extension l.  Every lane walks the growing tree in index order with a strict <, so the
//                   lowest index wins a tie; the closest connect pair is found by a (d2, lane) minimum over the wave.
//                   Targets and new nodes live column-major per problem ([c][lane]: a wave reads and writes whole lines).
//                   Header: edges (sum), longest edge (max of the bits of a non-negative double), problems at work (count).
//   (rocprim::exclusive_scan of the per-problem counts: where each problem's edges start)
//   k_plan_gather   the problem's edges as one run of cnt * d doubles of the AoS edge batch, written 64 at a time: the
//                   connect edge first, then the extensions in lane order.
//   (launch_edges: the verdicts)
//   k_plan_commit   a valid connect edge: SOLVED, the junction kept.  Otherwise the valid extensions appended by ballot
//                   prefix, parent = the node they were stepped from.
//   k_plan_finish   the parent walks into P (tree 0 from its junction up, reversed; tree 1 from its junction up), status
//                   and counters.
#pragma once

#include "mjpl_shortcut.h"  // shortcut_mix (splitmix64's step), shortcut_below

namespace mjpl {

constexpr int kPlanWaves = 4;   // problems per workgroup
constexpr int kPlanLanes = 64;  // extensions per problem and round: one per lane
constexpr int kPlanSolved = 0, kPlanRounds = 1, kPlanNonFinite = 2, kPlanInvalidEnd = 3, kPlanNodes = 4;  // MJPL_PLAN_*
constexpr int kPlanActive = -1;  // (state of a problem still at work)

struct PlanBatch {
  const double *QI, *QG;  // [B][d]
  const double *box;      // lo [d], hi [d]
  int d, K, N, R;         // columns, candidates, node capacity of a tree, rounds of the call
  int b0, nb;             // the chunk: problems [b0, b0 + nb)
  int round;              // -1: the direct edge
  double epsilon;
  unsigned long long seed_mixed;  // splitmix64(seed)
  // per problem of the chunk
  double *T;    // [nb][2][N][d]
  int *par;     // [nb][2][N]
  double *ct;   // [nb][d][64]: the round's targets, then its new nodes
  int *ck;      // [nb][64]: the node each extension steps from
  int *n;       // [nb][2]
  int *state, *gained, *rused, *nedges;
  int *conn;    // [nb][3]: has a connect edge, its node of the other tree, its node of the growing tree
  int *jn;      // [nb][2]: the junction, per tree
  int *cnt, *off;  // [nb + 1]
  // the ends' batch and verdicts; the round's edges, verdicts and header {bits of the longest edge, edges, problems at work}
  double *cfg;  // [2 nb][d]
  const uint8_t *cvalid;
  double *QA, *QB;
  const uint8_t *valid;
  unsigned long long *head;
  // outputs (rounds_used, edges, tree_nodes: may be null)
  double *P;  // [B][R + 2][d], zeroed
  int32_t *n_out, *status, *rounds_used, *edges, *tree_nodes;
};

// d2(a, t): columns in order from 0.0, one rounding per operation; t[c] is at t[c * ts]
__device__ __forceinline__ double plan_d2(const double *a, const double *t, int ts, int d) {
  double s = 0.0;
  for (int c = 0; c < d; c++) {
    const double v = t[(int64_t)c * ts] - a[c];
    s += v * v;
  }
  return s;
}

// nearest(T, t) over n >= 1 rows: the lowest index of the least d2, and that d2
__device__ __forceinline__ int plan_nearest(const double *T, int n, const double *t, int ts, int d, double *best) {
  int k = 0;
  double b = plan_d2(T, t, ts, d);
  for (int i = 1; i < n; i++) {
    const double v = plan_d2(T + (int64_t)i * d, t, ts, d);
    if (v < b) {
      b = v;
      k = i;
    }
  }
  *best = b;
  return k;
}

// the chunk-local problem of this wave, or -1
__device__ __forceinline__ int plan_problem(const PlanBatch &a) {
  const int p = blockIdx.x * kPlanWaves + (threadIdx.x >> 6);
  return p < a.nb ? p : -1;
}

__device__ __forceinline__ double *plan_tree(const PlanBatch &a, int p, int g) { return a.T + ((int64_t)p * 2 + g) * a.N * a.d; }

__global__ void __launch_bounds__(64 * kPlanWaves) k_plan_init(PlanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  const double *qi = a.QI + (int64_t)(a.b0 + p) * a.d, *qg = a.QG + (int64_t)(a.b0 + p) * a.d;
  bool bad = false;
  for (int c = lane; c < a.d; c += 64) bad |= !isfinite(qi[c]) || !isfinite(qg[c]);
  const bool any_bad = __ballot(bad) != 0ull;
  double *t0 = plan_tree(a, p, 0), *t1 = plan_tree(a, p, 1), *cf = a.cfg + (int64_t)p * 2 * a.d;
  for (int c = lane; c < a.d; c += 64) {
    t0[c] = qi[c];
    t1[c] = qg[c];
    cf[c] = any_bad ? 0.0 : qi[c];
    cf[a.d + c] = any_bad ? 0.0 : qg[c];
  }
  if (lane == 0) {
    a.par[((int64_t)p * 2 + 0) * a.N] = -1;
    a.par[((int64_t)p * 2 + 1) * a.N] = -1;
    a.n[p * 2] = a.n[p * 2 + 1] = 0;  // (the trees exist once the direct edge has failed)
    a.state[p] = any_bad ? kPlanNonFinite : kPlanActive;
    a.gained[p] = 0;
    a.rused[p] = 0;
    a.nedges[p] = 0;
    a.conn[p * 3] = 0;
    a.jn[p * 2] = a.jn[p * 2 + 1] = 0;
    a.cnt[p] = 0;
    if (p == 0) a.cnt[a.nb] = 0;
  }
}

__global__ void __launch_bounds__(64 * kPlanWaves) k_plan_propose(PlanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  int st = a.state[p];
  const int r = a.round, g = r & 1, o = 1 - g;
  const int ng = a.n[p * 2 + g], no = a.n[p * 2 + o];
  if (st == kPlanActive) {
    if (r < 0 && !(a.cvalid[p * 2] && a.cvalid[p * 2 + 1])) st = kPlanInvalidEnd;
    if (r >= 0 && ng >= a.N) st = kPlanNodes;
    if (st != kPlanActive && lane == 0) {
      a.state[p] = st;
      a.rused[p] = r < 0 ? 0 : r;
    }
  }
  if (st != kPlanActive) {
    if (lane == 0) a.cnt[p] = 0;
    return;
  }
  const int d = a.d;
  const double *Tg = plan_tree(a, p, g), *To = plan_tree(a, p, o);
  double longest = 0.0;
  int count;
  if (r < 0) {  // the direct edge: QA = T0[0], QB = T1[0]
    longest = sqrt(plan_d2(Tg, To, 1, d));
    if (lane == 0) {
      a.conn[p * 3] = 1;
      a.conn[p * 3 + 1] = 0;
      a.conn[p * 3 + 2] = 0;
    }
    count = 1;
  } else {
    // connect: lane l holds the l-th node the other tree gained; the least d2 wins, ties to the lowest lane
    const int gained = a.gained[p];
    double cbest = 0.0;
    int cn = 0;
    if (lane < gained) cn = plan_nearest(Tg, ng, To + (int64_t)(no - gained + lane) * d, 1, d, &cbest);
    int csrc = -1;
    if (gained > 0) {
      double mb = cbest;
      int ml = lane < gained ? lane : 64;
      for (int w = 32; w > 0; w >>= 1) {
        const double ob = __shfl_xor(mb, w);
        const int ol = __shfl_xor(ml, w);
        if (ol < 64 && (ml == 64 || ob < mb || (ob == mb && ol < ml))) {
          mb = ob;
          ml = ol;
        }
      }
      csrc = ml;
      if (lane == csrc) {
        a.conn[p * 3] = 1;
        a.conn[p * 3 + 1] = no - gained + lane;
        a.conn[p * 3 + 2] = cn;
      }
      longest = sqrt(mb);
    } else if (lane == 0) {
      a.conn[p * 3] = 0;
    }
    // extensions
    const int room = a.N - ng, next = a.K < room ? a.K : room;
    if (lane < next) {
      double *t = a.ct + (int64_t)p * d * 64 + lane;
      unsigned long long z = shortcut_mix(shortcut_mix(a.seed_mixed ^ (unsigned long long)(a.b0 + p)) ^ (64ull * (unsigned long long)r + (unsigned long long)lane));
      for (int c = 0; c < d; c++) {
        const double u = (double)(z >> 11) * 0x1.0p-53;
        const double lo = a.box[c], w = a.box[d + c] - lo;
        t[c * 64] = lo + u * w;
        z = shortcut_mix(z);
      }
      double best;
      const int k = plan_nearest(Tg, ng, t, 64, d, &best);
      const double m = sqrt(best);
      const double *from = Tg + (int64_t)k * d;
      double len = m;
      if (!(m <= a.epsilon)) {
        double s = 0.0;  // the edge's own length, as the host form of mjpl_check_edges adds it
        for (int c = 0; c < d; c++) {
          const double q = from[c] + ((t[c * 64] - from[c]) / m) * a.epsilon;
          t[c * 64] = q;
          const double v = q - from[c];
          s += v * v;
        }
        len = sqrt(s);
      }
      a.ck[p * 64 + lane] = k;
      if (len > longest) longest = len;  // (NaN never compares greater)
    }
    for (int w = 32; w > 0; w >>= 1) {
      const double other = __shfl_xor(longest, w);
      if (other > longest) longest = other;
    }
    count = next + (gained > 0 ? 1 : 0);
  }
  if (lane == 0) {
    a.cnt[p] = count;
    a.nedges[p] += count;
    atomicMax(&a.head[0], (unsigned long long)__double_as_longlong(longest));
    atomicAdd(&a.head[1], (unsigned long long)count);
    atomicAdd(&a.head[2], 1ull);
  }
}

__global__ void __launch_bounds__(64 * kPlanWaves) k_plan_gather(PlanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  const int cnt = a.cnt[p];
  if (cnt == 0) return;
  const int d = a.d, r = a.round, g = r & 1, o = 1 - g;
  const int has = a.conn[p * 3], cp = a.conn[p * 3 + 1], cn = a.conn[p * 3 + 2];
  // round -1: T_o = T0 and T_g = T1 (g = 1), so the direct edge is QA = T0[0], QB = T1[0]
  const double *Tg = plan_tree(a, p, g), *To = plan_tree(a, p, o), *ct = a.ct + (int64_t)p * d * 64;
  const int64_t e0 = (int64_t)a.off[p] * d;  // (off[p] + cnt <= nb (K + 1): the batch is sized for that)
  for (int i = lane; i < cnt * d; i += 64) {
    const int j = i / d, c = i - j * d;
    double qa, qb;
    if (has && j == 0) {
      qa = To[(int64_t)cp * d + c];
      qb = Tg[(int64_t)cn * d + c];
    } else {
      const int l = j - has;
      qa = Tg[(int64_t)a.ck[p * 64 + l] * d + c];
      qb = ct[c * 64 + l];
    }
    a.QA[e0 + i] = qa;
    a.QB[e0 + i] = qb;
  }
}

__global__ void __launch_bounds__(64 * kPlanWaves) k_plan_commit(PlanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0 || a.state[p] != kPlanActive) return;
  const int cnt = a.cnt[p];
  if (cnt == 0) return;
  const int d = a.d, r = a.round, g = r & 1, o = 1 - g;
  const int has = a.conn[p * 3];
  const int64_t e0 = a.off[p];
  if (has && a.valid[e0] != 0) {
    if (lane == 0) {
      a.state[p] = kPlanSolved;
      a.rused[p] = r + 1;
      a.jn[p * 2 + o] = a.conn[p * 3 + 1];
      a.jn[p * 2 + g] = a.conn[p * 3 + 2];
    }
    return;
  }
  if (r < 0) {  // the trees of step 4
    if (lane == 0) a.n[p * 2] = a.n[p * 2 + 1] = 1;
    return;
  }
  const int next = cnt - has, ng = a.n[p * 2 + g];
  const bool ok = lane < next && a.valid[e0 + has + lane] != 0;
  const unsigned long long okmask = __ballot(ok);
  if (ok) {
    const int at = ng + __popcll(okmask & shortcut_below(lane));  // (< N: next <= N - ng)
    double *row = plan_tree(a, p, g) + (int64_t)at * d;
    const double *q = a.ct + (int64_t)p * d * 64 + lane;
    for (int c = 0; c < d; c++) row[c] = q[c * 64];
    a.par[((int64_t)p * 2 + g) * a.N + at] = a.ck[p * 64 + lane];
  }
  if (lane == 0) {
    a.n[p * 2 + g] = ng + __popcll(okmask);
    a.gained[p] = __popcll(okmask);
  }
}

// (P arrives zeroed)
__global__ void __launch_bounds__(64 * kPlanWaves) k_plan_finish(PlanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  const int b = a.b0 + p, d = a.d, cap = a.R + 2;
  const int st = a.state[p];
  int rows = 0;
  if (st == kPlanSolved) {
    const double *T0 = plan_tree(a, p, 0), *T1 = plan_tree(a, p, 1);
    const int *par0 = a.par + ((int64_t)p * 2 + 0) * a.N, *par1 = a.par + ((int64_t)p * 2 + 1) * a.N;
    double *P = a.P + (int64_t)b * cap * d;
    // a tree's depth is at most the rounds it grew in: len0 + len1 <= R + 2 (the guards keep a broken chain inside P)
    int len0 = 0;
    for (int k = a.jn[p * 2]; k >= 0 && len0 < cap; k = par0[k]) len0++;
    int i = len0 - 1;
    for (int k = a.jn[p * 2]; k >= 0 && i >= 0; k = par0[k], i--)
      for (int c = lane; c < d; c += 64) P[(int64_t)i * d + c] = T0[(int64_t)k * d + c];
    rows = len0;
    for (int k = a.jn[p * 2 + 1]; k >= 0 && rows < cap; k = par1[k], rows++)
      for (int c = lane; c < d; c += 64) P[(int64_t)rows * d + c] = T1[(int64_t)k * d + c];
  }
  if (lane == 0) {
    a.n_out[b] = rows;
    a.status[b] = st == kPlanActive ? kPlanRounds : st;
    if (a.rounds_used) a.rounds_used[b] = st == kPlanActive ? a.R : a.rused[p];
    if (a.edges) a.edges[b] = a.nedges[p];
    if (a.tree_nodes) {
      a.tree_nodes[(int64_t)b * 2] = a.n[p * 2];
      a.tree_nodes[(int64_t)b * 2 + 1] = a.n[p * 2 + 1];
    }
  }
}

}  // namespace mjpl
