// mjpl_shortcut.h -- batched path shortcutting (mjpl_shortcut_paths*, include/mjpl_hip.h).
//
// What it adds: "these B paths, shortcut in lockstep".  Every round each path proposes up to 64 shortcuts (i, j) of its
// live list, every proposal of every path is validated by ONE launch of the edge pipeline (launch_edges, mjpl_hip.hip),
// and each path commits the valid ones greedily by saving.  tests/shortcut_reference.py is the NumPy statement of every
// number and decision below, operation for operation; DESIGN.md 5.15 has the reasoning.  All float64, -ffp-contract=off.
// The only atomics are integer ones on the round's header (a sum, a maximum of bit patterns, a count): their results do
// not depend on the order, so two runs give the same bits.
//
// One wave per path in every kernel, kShortcutWaves paths per workgroup; no workgroup barrier anywhere (a wave whose
// path is retired returns at once).  Kernels, in launch order:
//   k_shortcut_init     the live list 0 .. n-1, the counters, and the NaN / inf scan of the path's rows.
//   k_shortcut_propose  retires a path of <= 2 live waypoints; the arc lengths L of the live list: the segment lengths
//                       come 64 at a time, one per lane, and are ADDED IN INDEX ORDER -- every lane runs the same chain
//                       on values broadcast from lane t, so the bits are those of a serial loop (a wave scan would
//                       associate differently); lane l = candidate l: the l-th pair of an exhaustive round, or the pair
//                       drawn from splitmix64(seed, path, round, l); its saving s = (L[j] - L[i]) - d(i, j); a ballot
//                       ranks the proposed ones.  Header: proposed edges (sum), longest proposed edge (max of the bits
//                       of a non-negative double), paths still at work (count).
//   (rocprim::exclusive_scan of the per-path counts: where each path's edges start)
//   k_shortcut_gather   lane = candidate: rows W[live[i]], W[live[j]] into the AoS edge batch at offset + rank.
//   (launch_edges: the verdicts)
//   k_shortcut_commit   the valid proposals ordered by (s descending, l ascending) -- every lane counts the lanes ahead
//                       of it, comparisons only --, then walked in that order: one is accepted iff it overlaps no
//                       accepted one (a ballot); an exhaustive round without a valid proposal retires the path as
//                       CONVERGED.  The live list is compacted in place, 64 entries at a time, by ballot prefix: a
//                       chunk is read whole before any of it is written, and what it writes lies below the next chunk.
//   k_shortcut_finish   keep flags, the count, the length (the same chain over the final live list), status, counters.
#pragma once

namespace mjpl {

constexpr int kShortcutWaves = 4;          // paths per workgroup
constexpr int kShortcutLanes = 64;         // candidates per path and round: one per lane
constexpr int kShortcutMaxRows = 1 << 16;  // waypoints per path
constexpr int kShortcutConverged = 0, kShortcutRounds = 1, kShortcutNonFinite = 2;  // MJPL_SHORTCUT_*
constexpr int kShortcutActive = -1;        // (state of a path still at work)

struct ShortcutBatch {
  const double *W;        // [wp_off[B]][d]
  const int64_t *wp_off;  // [B + 1], device
  int d, K;
  int b0, nb;             // the chunk: paths [b0, b0 + nb)
  int64_t row0;           // wp_off[b0]: the chunk's arrays by row start there
  int round, have_verdicts;
  double min_saving;
  unsigned long long seed_mixed;  // splitmix64(seed)
  // per row of the chunk
  int *live;
  double *L;
  // per path of the chunk
  int *m, *state, *nprop, *nacc, *cnt, *off;
  // per (path, lane)
  int *ci, *cj, *crank;
  double *cs;
  // the round's edges and header {bits of the longest proposed edge, proposed edges, paths at work}
  double *QA, *QB;
  const uint8_t *valid;
  unsigned long long *head;
  // outputs (length, proposed, accepted: may be null)
  uint8_t *keep;
  int32_t *n_out, *status, *proposed, *accepted;
  double *length;
};

__host__ __device__ __forceinline__ unsigned long long shortcut_mix(unsigned long long x) {  // splitmix64's step
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// d(a, b): columns in order from 0.0, one rounding per operation
__device__ __forceinline__ double shortcut_dist(const double *W, int64_t ra, int64_t rb, int d) {
  double s = 0.0;
  for (int c = 0; c < d; c++) {
    const double t = W[rb * d + c] - W[ra * d + c];
    s += t * t;
  }
  return sqrt(s);
}

__device__ __forceinline__ unsigned long long shortcut_below(int lane) { return (1ull << lane) - 1ull; }

// The arc lengths of a live list of mm >= 2 entries, added in index order; written to L if it is not null.  Returns L[mm - 1].
__device__ __forceinline__ double shortcut_arc(const double *W, int d, int64_t w0, const int *live, int mm, int lane, double *L) {
  double acc = 0.0;
  if (L && lane == 0) L[0] = 0.0;
  for (int c0 = 1; c0 < mm; c0 += 64) {
    const int k = c0 + lane;
    double dv = 0.0, mine = 0.0;
    if (k < mm) dv = shortcut_dist(W, w0 + live[k - 1], w0 + live[k], d);
    const int nn = mm - c0 < 64 ? mm - c0 : 64;
    for (int t = 0; t < nn; t++) {
      acc = acc + __shfl(dv, t);
      if (t == lane) mine = acc;
    }
    if (L && k < mm) L[k] = mine;
  }
  return acc;
}

// the chunk-local path of this wave, or -1
__device__ __forceinline__ int shortcut_path(const ShortcutBatch &a) {
  const int p = blockIdx.x * kShortcutWaves + (threadIdx.x >> 6);
  return p < a.nb ? p : -1;
}

__global__ void __launch_bounds__(64 * kShortcutWaves) k_shortcut_init(ShortcutBatch a) {
  const int p = shortcut_path(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  const int64_t w0 = a.wp_off[a.b0 + p];
  const int n = (int)(a.wp_off[a.b0 + p + 1] - w0);
  bool bad = false;
  const int64_t cells = (int64_t)n * a.d;
  for (int64_t k = lane; k < cells; k += 64) bad |= !isfinite(a.W[w0 * a.d + k]);
  const bool any_bad = __ballot(bad) != 0ull;
  int *live = a.live + (w0 - a.row0);
  for (int k = lane; k < n; k += 64) live[k] = k;
  if (lane == 0) {
    a.m[p] = n;
    a.state[p] = any_bad ? kShortcutNonFinite : kShortcutActive;
    a.nprop[p] = 0;
    a.nacc[p] = 0;
    a.cnt[p] = 0;
    if (p == 0) a.cnt[a.nb] = 0;
  }
}

__global__ void __launch_bounds__(64 * kShortcutWaves) k_shortcut_propose(ShortcutBatch a) {
  const int p = shortcut_path(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  const int mm = a.m[p];
  if (a.state[p] != kShortcutActive || mm <= 2) {
    if (lane == 0) {
      if (a.state[p] == kShortcutActive) a.state[p] = kShortcutConverged;
      a.cnt[p] = 0;
    }
    return;
  }
  const int b = a.b0 + p;
  const int64_t w0 = a.wp_off[b];
  const int *live = a.live + (w0 - a.row0);
  double *L = a.L + (w0 - a.row0);
  shortcut_arc(a.W, a.d, w0, live, mm, lane, L);
  __threadfence_block();  // (L is read back below by other lanes of this wave)
  const int64_t npairs = (int64_t)(mm - 1) * (mm - 2) / 2;
  bool has = false;
  int i = 0, j = 0;
  if (lane < a.K) {
    if (npairs <= a.K) {  // exhaustive: the lane-th pair with j >= i + 2, lexicographic
      if (lane < npairs) {
        int rem = lane;
        while (rem >= mm - 2 - i) {
          rem -= mm - 2 - i;
          i++;
        }
        j = i + 2 + rem;
        has = true;
      }
    } else {
      const unsigned long long z =
          shortcut_mix(shortcut_mix(a.seed_mixed ^ (unsigned long long)b) ^ (64ull * (unsigned long long)a.round + (unsigned long long)lane));
      i = (int)(((z & 0xffffffffull) * (unsigned long long)(mm - 2)) >> 32);
      j = i + 2 + (int)(((z >> 32) * (unsigned long long)(mm - 2 - i)) >> 32);
      has = true;
    }
  }
  double s = 0.0, dd = 0.0;
  bool prop = false;
  if (has) {
    dd = shortcut_dist(a.W, w0 + live[i], w0 + live[j], a.d);
    s = (L[j] - L[i]) - dd;
    prop = s > a.min_saving;
  }
  const unsigned long long mask = __ballot(prop);
  const int at = p * kShortcutLanes + lane;
  a.ci[at] = i;
  a.cj[at] = j;
  a.cs[at] = s;
  a.crank[at] = prop ? __popcll(mask & shortcut_below(lane)) : -1;
  double mx = prop ? dd : 0.0;  // (a proposed edge has a finite length: s would not compare greater otherwise)
  for (int o = 32; o > 0; o >>= 1) {
    const double other = __shfl_xor(mx, o);
    if (other > mx) mx = other;
  }
  if (lane == 0) {
    const int count = __popcll(mask);
    a.cnt[p] = count;
    a.nprop[p] += count;
    if (count) {
      atomicMax(&a.head[0], (unsigned long long)__double_as_longlong(mx));
      atomicAdd(&a.head[1], (unsigned long long)count);
    }
    atomicAdd(&a.head[2], 1ull);
  }
}

__global__ void __launch_bounds__(64 * kShortcutWaves) k_shortcut_gather(ShortcutBatch a) {
  const int p = shortcut_path(a), lane = threadIdx.x & 63;
  if (p < 0 || a.cnt[p] == 0) return;
  const int at = p * kShortcutLanes + lane, rank = a.crank[at];
  if (rank < 0) return;
  const int64_t w0 = a.wp_off[a.b0 + p];
  const int *live = a.live + (w0 - a.row0);
  const int64_t e = (int64_t)a.off[p] + rank;  // (< nb K: the batch is sized for K edges of every path)
  const double *ra = a.W + (w0 + live[a.ci[at]]) * a.d, *rb = a.W + (w0 + live[a.cj[at]]) * a.d;
  for (int c = 0; c < a.d; c++) {
    a.QA[e * a.d + c] = ra[c];
    a.QB[e * a.d + c] = rb[c];
  }
}

__global__ void __launch_bounds__(64 * kShortcutWaves) k_shortcut_commit(ShortcutBatch a) {
  const int p = shortcut_path(a), lane = threadIdx.x & 63;
  if (p < 0 || a.state[p] != kShortcutActive) return;
  const int mm = a.m[p];
  const int at = p * kShortcutLanes + lane, rank = a.crank[at];
  const int i = a.ci[at], j = a.cj[at];
  const double s = a.cs[at];
  const bool ok = rank >= 0 && a.have_verdicts && a.valid[(int64_t)a.off[p] + rank] != 0;
  const unsigned long long okmask = __ballot(ok);
  if (okmask == 0ull) {
    if (lane == 0 && (int64_t)(mm - 1) * (mm - 2) / 2 <= a.K) a.state[p] = kShortcutConverged;
    return;
  }
  int ord = 0;  // valid proposals ahead of this one by (s descending, lane ascending)
  for (int t = 0; t < 64; t++) {
    const double st = __shfl(s, t);
    if (((okmask >> t) & 1ull) && (st > s || (st == s && t < lane))) ord++;
  }
  unsigned long long accmask = 0ull;
  const int nv = __popcll(okmask);
  for (int q = 0; q < nv; q++) {
    const int src = __ffsll((unsigned long long)__ballot(ok && ord == q)) - 1;
    const int ai = __shfl(i, src), aj = __shfl(j, src);
    const bool clash = ((accmask >> lane) & 1ull) && !(aj <= i || j <= ai);
    if (__ballot(clash) == 0ull) accmask |= 1ull << src;
  }
  const int64_t w0 = a.wp_off[a.b0 + p];
  int *live = a.live + (w0 - a.row0);
  int out = 0;
  for (int c0 = 0; c0 < mm; c0 += 64) {
    const int k = c0 + lane;
    const int v = k < mm ? live[k] : 0;
    bool keepk = k < mm;
    for (unsigned long long mk = accmask; mk; mk &= mk - 1ull) {
      const int t = __ffsll(mk) - 1;
      const int ai = __shfl(i, t), aj = __shfl(j, t);
      if (ai < k && k < aj) keepk = false;
    }
    const unsigned long long km = __ballot(keepk);
    if (keepk) live[out + __popcll(km & shortcut_below(lane))] = v;
    out += __popcll(km);
  }
  if (lane == 0) {
    a.m[p] = out;
    a.nacc[p] += __popcll(accmask);
  }
}

// (keep arrives zeroed)
__global__ void __launch_bounds__(64 * kShortcutWaves) k_shortcut_finish(ShortcutBatch a) {
  const int p = shortcut_path(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  const int b = a.b0 + p;
  const int64_t w0 = a.wp_off[b];
  const int n = (int)(a.wp_off[b + 1] - w0);
  const int st = a.state[p];
  const int *live = a.live + (w0 - a.row0);
  const int mm = st == kShortcutNonFinite ? n : a.m[p];
  for (int k = lane; k < mm; k += 64) a.keep[w0 + (st == kShortcutNonFinite ? k : live[k])] = 1;
  double len = __longlong_as_double(0x7FF8000000000000ll);  // (a path left untouched has no length)
  if (st != kShortcutNonFinite) len = shortcut_arc(a.W, a.d, w0, live, mm, lane, nullptr);
  if (lane == 0) {
    a.n_out[b] = mm;
    a.status[b] = st == kShortcutActive ? kShortcutRounds : st;
    if (a.length) a.length[b] = len;
    if (a.proposed) a.proposed[b] = a.nprop[p];
    if (a.accepted) a.accepted[b] = a.nacc[p];
  }
}

}  // namespace mjpl
