// mjpl_roadmap.h -- multi-query planning on a roadmap (mjpl_roadmap_build*, mjpl_roadmap_query*, include/mjpl_hip.h).
//
// What it adds: "validate the edges of this scene once, then answer many queries".  Build takes N configurations, finds
// every node's k nearest valid nodes within a radius, validates each candidate pair once by the edge pipeline
// (launch_edges, mjpl_hip.hip) and writes the valid ones as a symmetric CSR adjacency into the caller's arrays.  A query
// attaches each end to its nearest nodes, validates the direct edge and the attachments of EVERY problem in one edge
// launch, and finds the shortest path through the graph.  tests/roadmap_reference.py is the NumPy statement of every
// number and decision below; DESIGN.md 5.17 has the reasoning.  All float64, -ffp-contract=off.  The only atomics are
// integer ones on the call's header (a sum, maxima of bit patterns): their results do not depend on the order.
//
// Kernels, in launch order.  Build:
//   k_rm_finite     the NaN / inf scan of the rows and the configuration batch (zeros for a non-finite row).
//   (launch_configs: the rows' verdicts; k_rm_mask: valid = finite and free)
//   k_rm_knn        brute force, one lane per query row: the candidate rows pass through LDS in tiles of 64, every lane
//                   keeps its sorted (d2, j) list of at most 32 entries in LDS ([entry][lane]: no bank conflict) and
//                   the list's last entry in registers, so a candidate that does not enter costs no LDS access.  A
//                   strict < on (d2, j) decides, so neither the tile size nor the order of the tiles can change a list.
//   k_rm_pair_keys  (min << 32 | max) per list entry; rocprim::radix_sort_keys; k_rm_unique, rocprim::exclusive_scan and
//                   k_rm_compact leave each candidate pair once, ascending by (i, j).
//   k_rm_longest    the longest edge of every launch (the long_edges rule of mjpl_check_edges), one copy for all.
//   k_rm_edge_rows  a launch's edge batch, lower index first.  (launch_edges: the verdicts)
//   k_rm_dir_keys   (src << 32 | dst) for both directions of a valid edge; rocprim::radix_sort_keys; k_rm_row_off (a
//                   binary search per row: the invalid edges' keys sort behind every row) and k_rm_csr.
// Query:
//   k_rm_finite     the ends, two rows per problem (both zeros if either holds a NaN / inf).
//   (launch_configs) k_rm_knn over the 2 B ends, no lower bound.
//   k_rm_q_count    status so far and the problem's edge count; rocprim::exclusive_scan; k_rm_q_gather: the direct edge, the
//                   start attachments QI -> Q[v], the goal attachments Q[v] -> QG.  (ONE launch_edges)
//   k_rm_search     one workgroup per problem: the direct edge, or pull relaxation over the CSR until a sweep changes
//                   nothing (dist in LDS when N doubles fit, in the chunk's workspace otherwise), the goal choice and the
//                   walk back into P by lane 0.
#pragma once

#include "mjpl_plan.h"  // plan_d2

namespace mjpl {

constexpr int kRmMaxK = 32;      // list entries per lane: k of a build, connections of a query
constexpr int kRmTile = 64;      // candidate rows per LDS tile, and lanes per workgroup of k_rm_knn
constexpr int kRmBlock = 256;    // threads of the flat kernels
constexpr int kRmSolved = 0, kRmNoPath = 1, kRmNonFinite = 2, kRmInvalidEnd = 3, kRmLong = 4;  // MJPL_ROADMAP_*
constexpr int kRmActive = -1;    // (state of a problem that goes on to the edge launch)

// rows X0[i] (and X1[i], if given: a problem's two ends) -> the configuration batch, zeros for a group that holds a NaN / inf
__global__ void __launch_bounds__(kRmBlock) k_rm_finite(const double *X0, const double *X1, int n, int d, double *cfg, uint8_t *fin) {
  const int i = blockIdx.x * kRmBlock + threadIdx.x;
  if (i >= n) return;
  const double *x0 = X0 + (int64_t)i * d, *x1 = X1 ? X1 + (int64_t)i * d : nullptr;
  bool ok = true;
  for (int c = 0; c < d; c++) ok &= isfinite(x0[c]) && (!x1 || isfinite(x1[c]));
  double *out = cfg + (int64_t)i * d * (x1 ? 2 : 1);
  for (int c = 0; c < d; c++) {
    out[c] = ok ? x0[c] : 0.0;
    if (x1) out[d + c] = ok ? x1[c] : 0.0;
  }
  fin[i] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(kRmBlock) k_rm_mask(uint8_t *valid, const uint8_t *fin, int n) {
  const int i = blockIdx.x * kRmBlock + threadIdx.x;
  if (i < n) valid[i] = valid[i] && fin[i] ? 1 : 0;
}

struct RmKnn {
  const double *X;     // [M][d] query rows
  const uint8_t *xok;  // [M] or null: a row with 0 gets an empty list
  int M;
  const double *Q;     // [N][d] nodes
  const uint8_t *qok;  // [N]
  int N, d, k;
  double r2, lo2;
  int self;            // query row i IS node i: j = i is left out and the lower bound lo2 applies
  int32_t *nn_j;       // [M][k], -1 past the count
  double *nn_d2;       // [M][k], 0 past the count
  int32_t *nn_cnt;     // [M]
};

// LDS: the lists' d2 [32][64], the query rows [d][64], the tile [64][d], the lists' j [32][64], the tile's valid flags [64]
__host__ __device__ inline size_t rm_knn_lds(int d) {
  return ((size_t)kRmMaxK * 64 + 2 * (size_t)d * 64) * sizeof(double) + (size_t)kRmMaxK * 64 * sizeof(int) + 64;
}

__global__ void __launch_bounds__(kRmTile) k_rm_knn(RmKnn a) {
  extern __shared__ double rm_knn_smem[];
  const int lane = threadIdx.x, d = a.d, k = a.k;
  double *ld2 = rm_knn_smem, *xq = ld2 + kRmMaxK * 64, *tile = xq + d * 64;
  int *lj = reinterpret_cast<int *>(tile + kRmTile * d);
  uint8_t *tok = reinterpret_cast<uint8_t *>(lj + kRmMaxK * 64);
  const int q = blockIdx.x * kRmTile + lane;
  const bool live = q < a.M && (!a.xok || a.xok[q] != 0);
  for (int c = 0; c < d; c++) xq[c * 64 + lane] = q < a.M ? a.X[(int64_t)q * d + c] : 0.0;
  int cnt = 0, wj = 0;  // the list's size and its last entry (wd, wj)
  double wd = 0.0;
  for (int t0 = 0; t0 < a.N; t0 += kRmTile) {
    const int nt = a.N - t0 < kRmTile ? a.N - t0 : kRmTile;
    __syncthreads();
    for (int i = lane; i < nt * d; i += kRmTile) tile[i] = a.Q[(int64_t)t0 * d + i];
    tok[lane] = lane < nt ? a.qok[t0 + lane] : 0;
    __syncthreads();
    if (!live) continue;
    for (int r = 0; r < nt; r++) {
      if (!tok[r]) continue;  // (the same in every lane)
      const int j = t0 + r;
      double v = 0.0;
      for (int c = 0; c < d; c++) {
        const double t = tile[r * d + c] - xq[c * 64 + lane];
        v += t * t;
      }
      if (!(v <= a.r2)) continue;  // (NaN never enters)
      if (a.self && (j == q || v < a.lo2)) continue;
      if (cnt == k && !(v < wd || (v == wd && j < wj))) continue;
      int p = cnt < k ? cnt : k - 1;  // (a full list drops its last entry)
      for (; p > 0; p--) {
        const double pd = ld2[(p - 1) * 64 + lane];
        const int pj = lj[(p - 1) * 64 + lane];
        if (pd < v || (pd == v && pj < j)) break;
        ld2[p * 64 + lane] = pd;
        lj[p * 64 + lane] = pj;
      }
      ld2[p * 64 + lane] = v;
      lj[p * 64 + lane] = j;
      if (cnt < k) cnt++;
      wd = ld2[(cnt - 1) * 64 + lane];
      wj = lj[(cnt - 1) * 64 + lane];
    }
  }
  if (q >= a.M) return;
  for (int e = 0; e < k; e++) {
    a.nn_j[(int64_t)q * k + e] = e < cnt ? lj[e * 64 + lane] : -1;
    a.nn_d2[(int64_t)q * k + e] = e < cnt ? ld2[e * 64 + lane] : 0.0;
  }
  a.nn_cnt[q] = cnt;
}

// ---- build: the candidate pairs and the CSR

// key of list entry p (row p / k): lower index in the high word; an empty entry sorts behind every pair
__global__ void __launch_bounds__(kRmBlock) k_rm_pair_keys(const int32_t *nn_j, int64_t n, int k, unsigned long long none, unsigned long long *keys) {
  const int64_t p = (int64_t)blockIdx.x * kRmBlock + threadIdx.x;
  if (p >= n) return;
  const int j = nn_j[p], i = (int)(p / k);
  const unsigned lo = (unsigned)(i < j ? i : j), hi = (unsigned)(i < j ? j : i);
  keys[p] = j < 0 ? none : ((unsigned long long)lo << 32 | hi);
}

// flag [n + 1]: sorted key p is a pair and the first of its value (flag[n] = 0: the scan's total lands in pos[n])
__global__ void __launch_bounds__(kRmBlock) k_rm_unique(const unsigned long long *keys, int64_t n, unsigned long long none, int *flag) {
  const int64_t p = (int64_t)blockIdx.x * kRmBlock + threadIdx.x;
  if (p > n) return;
  flag[p] = p < n && keys[p] != none && (p == 0 || keys[p] != keys[p - 1]) ? 1 : 0;
}

__global__ void __launch_bounds__(kRmBlock) k_rm_compact(const unsigned long long *keys, int64_t n, const int *flag, const int *pos, unsigned long long *out) {
  const int64_t p = (int64_t)blockIdx.x * kRmBlock + threadIdx.x;
  if (p < n && flag[p]) out[pos[p]] = keys[p];
}

// the longest edge of every launch of `chunk` pairs: a maximum of the bits of non-negative doubles
__global__ void __launch_bounds__(kRmBlock) k_rm_longest(const unsigned long long *pairs, int64_t E, int64_t chunk, const double *Q, int d, unsigned long long *cmax) {
  const int64_t e = (int64_t)blockIdx.x * kRmBlock + threadIdx.x;
  if (e >= E) return;
  const unsigned long long key = pairs[e];
  const double len = sqrt(plan_d2(Q + (int64_t)(key >> 32) * d, Q + (int64_t)(key & 0xffffffffull) * d, 1, d));
  atomicMax(&cmax[e / chunk], (unsigned long long)__double_as_longlong(len));
}

// pairs [e0, e0 + ne) as the AoS edge batch: one thread per double
__global__ void __launch_bounds__(kRmBlock) k_rm_edge_rows(const unsigned long long *pairs, int64_t e0, int64_t ne, const double *Q, int d, double *QA, double *QB) {
  const int64_t t = (int64_t)blockIdx.x * kRmBlock + threadIdx.x;
  if (t >= ne * d) return;
  const int64_t e = t / d;
  const int c = (int)(t - e * d);
  const unsigned long long key = pairs[e0 + e];
  QA[t] = Q[(int64_t)(key >> 32) * d + c];
  QB[t] = Q[(int64_t)(key & 0xffffffffull) * d + c];
}

__global__ void __launch_bounds__(kRmBlock) k_rm_dir_keys(const unsigned long long *pairs, const uint8_t *valid, int64_t E, unsigned long long none, unsigned long long *keys) {
  const int64_t e = (int64_t)blockIdx.x * kRmBlock + threadIdx.x;
  if (e >= E) return;
  const unsigned long long key = pairs[e];
  const bool ok = valid[e] != 0;
  keys[2 * e] = ok ? key : none;
  keys[2 * e + 1] = ok ? (key << 32 | key >> 32) : none;
}

// row_off[v], v = 0 .. N: the first sorted key not below (v << 32).  `none` = N << 32, so row_off[N] counts the entries.
__global__ void __launch_bounds__(kRmBlock) k_rm_row_off(const unsigned long long *keys, int64_t n, int N, int32_t *row_off) {
  const int v = blockIdx.x * kRmBlock + threadIdx.x;
  if (v > N) return;
  const unsigned long long want = (unsigned long long)v << 32;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  row_off[v] = (int32_t)lo;
}

// adj, w [cap]: the sorted directed keys, then -1 / 0.  w = sqrt(d2(Q[src], Q[dst])): the same bits in both directions.
__global__ void __launch_bounds__(kRmBlock) k_rm_csr(const unsigned long long *keys, int64_t n, int64_t cap, unsigned long long none, const double *Q, int d, int32_t *adj, double *w) {
  const int64_t p = (int64_t)blockIdx.x * kRmBlock + threadIdx.x;
  if (p >= cap) return;
  const unsigned long long key = p < n ? keys[p] : none;
  if (key == none) {
    adj[p] = -1;
    w[p] = 0.0;
    return;
  }
  const int64_t src = (int64_t)(key >> 32), dst = (int64_t)(key & 0xffffffffull);
  adj[p] = (int32_t)dst;
  w[p] = sqrt(plan_d2(Q + src * d, Q + dst * d, 1, d));
}

// ---- query

struct RmQuery {
  const double *Q;  // [N][d]
  const int32_t *row_off, *adj;
  const double *w;
  int N, d, C, max_rows;  // C: connections
  const double *QI, *QG;  // [B][d]
  int B, b0, nb;          // the search launch's problems [b0, b0 + nb)
  const uint8_t *fin;     // [B]
  const uint8_t *cvalid;  // [2 B]
  int32_t *state;         // [B]
  const int32_t *att_j;   // [2 B][C]: row 2 b the start's attachments, row 2 b + 1 the goal's
  const double *att_d2;
  const int32_t *att_cnt;
  int *cnt, *off;         // [B + 1]
  double *QA, *QB;
  const uint8_t *valid;
  double *dist;           // [nb][N], or null: in LDS
  unsigned long long *head;  // {bits of the longest edge, edges, sweeps}
  double *P;              // [B][max_rows][d], zeroed
  int32_t *n_out, *status;
  double *cost;           // may be null
};

__global__ void __launch_bounds__(kRmBlock) k_rm_q_count(RmQuery a) {
  const int b = blockIdx.x * kRmBlock + threadIdx.x;
  if (b > a.B) return;
  int st = kRmActive, count = 0;
  if (b < a.B) {
    if (!a.fin[b]) st = kRmNonFinite;
    else if (!(a.cvalid[2 * b] && a.cvalid[2 * b + 1])) st = kRmInvalidEnd;
    if (st == kRmActive) count = 1 + a.att_cnt[2 * b] + a.att_cnt[2 * b + 1];
    a.state[b] = st;
  }
  a.cnt[b] = count;  // (cnt[B] = 0: the scan's total lands in off[B])
  if (count) atomicAdd(&a.head[1], (unsigned long long)count);
}

// one wave per problem: its edges as one run of cnt * d doubles, 64 at a time; the longest of them
__global__ void __launch_bounds__(kRmBlock) k_rm_q_gather(RmQuery a) {
  const int b = blockIdx.x * (kRmBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= a.B) return;
  const int cnt = a.cnt[b];
  if (cnt == 0) return;
  const int d = a.d, cs = a.att_cnt[2 * b];
  const double *qi = a.QI + (int64_t)b * d, *qg = a.QG + (int64_t)b * d;
  const int32_t *aj = a.att_j + (int64_t)2 * b * a.C;
  const double *ad = a.att_d2 + (int64_t)2 * b * a.C;
  const int64_t e0 = (int64_t)a.off[b] * d;
  for (int i = lane; i < cnt * d; i += 64) {
    const int j = i / d, c = i - j * d;
    double qa, qb;
    if (j == 0) {
      qa = qi[c];
      qb = qg[c];
    } else if (j <= cs) {
      qa = qi[c];
      qb = a.Q[(int64_t)aj[j - 1] * d + c];
    } else {
      qa = a.Q[(int64_t)aj[a.C + j - 1 - cs] * d + c];
      qb = qg[c];
    }
    a.QA[e0 + i] = qa;
    a.QB[e0 + i] = qb;
  }
  double longest = 0.0;
  for (int j = lane; j < cnt; j += 64) {
    const double d2 = j == 0 ? plan_d2(qi, qg, 1, d) : j <= cs ? ad[j - 1] : ad[a.C + j - 1 - cs];
    const double len = sqrt(d2);
    if (len > longest) longest = len;
  }
  for (int s = 32; s > 0; s >>= 1) {
    const double other = __shfl_xor(longest, s);
    if (other > longest) longest = other;
  }
  if (lane == 0) atomicMax(&a.head[0], (unsigned long long)__double_as_longlong(longest));
}

// One workgroup per problem.  dist is only ever lowered, and every value it holds is the left-to-right rounded length of
// a real path from QI, so a lane that reads a neighbour's entry while another lane lowers it changes no final bit: the
// sweeps end at the one fixed point.  Aligned 8-byte accesses only.
template <bool kLds>
__global__ void __launch_bounds__(1024) k_rm_search(RmQuery a) {
  extern __shared__ double rm_dist_smem[];
  const int b = a.b0 + blockIdx.x, tid = threadIdx.x, nth = blockDim.x, d = a.d, N = a.N;
  const int st = a.state[b];
  if (st != kRmActive) {  // (the same in every lane of the workgroup)
    if (tid == 0) {
      a.n_out[b] = 0;
      a.status[b] = st;
      if (a.cost) a.cost[b] = 0.0;
    }
    return;
  }
  const double *qi = a.QI + (int64_t)b * d, *qg = a.QG + (int64_t)b * d;
  double *P = a.P + (int64_t)b * a.max_rows * d;
  const int64_t e0 = a.off[b];
  if (a.valid[e0] != 0) {  // the direct edge
    for (int c = tid; c < d; c += nth) {
      P[c] = qi[c];
      P[d + c] = qg[c];
    }
    if (tid == 0) {
      a.n_out[b] = 2;
      a.status[b] = kRmSolved;
      if (a.cost) a.cost[b] = sqrt(plan_d2(qi, qg, 1, d));
    }
    return;
  }
  const int cs = a.att_cnt[2 * b], cg = a.att_cnt[2 * b + 1];
  const int32_t *sj = a.att_j + (int64_t)2 * b * a.C, *gj = sj + a.C;
  const double *sd = a.att_d2 + (int64_t)2 * b * a.C, *gd = sd + a.C;
  const uint8_t *sv = a.valid + e0 + 1, *gv = sv + cs;
  double *dist = kLds ? rm_dist_smem : a.dist + (int64_t)blockIdx.x * N;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  for (int v = tid; v < N; v += nth) dist[v] = inf;
  __syncthreads();
  if (tid < cs && sv[tid] != 0) dist[sj[tid]] = sqrt(sd[tid]);  // init (the attachments are different nodes)
  __syncthreads();
  int sweeps = 0;
  while (sweeps < N) {
    int changed = 0;
    for (int v = tid; v < N; v += nth) {
      const int r0 = a.row_off[v], r1 = a.row_off[v + 1];
      if (r0 >= r1) continue;
      const double cur = dist[v];
      double best = cur;
      for (int p = r0; p < r1; p++) {
        const int u = a.adj[p];
        if ((unsigned)u >= (unsigned)N) continue;
        const double c = dist[u] + a.w[p];
        if (c < best) best = c;
      }
      if (best < cur) {
        dist[v] = best;
        changed = 1;
      }
    }
    sweeps++;
    if (!__syncthreads_or(changed)) break;
  }
  if (tid != 0) return;
  atomicAdd(&a.head[2], (unsigned long long)sweeps);
  // the goal choice: the least rounded total, ties to the lowest rank
  double total = inf;
  int g = -1;
  for (int j = 0; j < cg; j++) {
    if (gv[j] == 0) continue;
    const double c = dist[gj[j]] + sqrt(gd[j]);
    if (c < total) {
      total = c;
      g = gj[j];
    }
  }
  int rows = 0, status = kRmNoPath;
  if (g >= 0) {
    // the walk back, twice: its length, then its rows in travel order.  At v: stop where init[v] == dist[v], otherwise
    // on to the lowest u of row v with dist[u] + w == dist[v] (the rows ascend).
    for (int pass = 0; pass < 2; pass++) {
      int v = g, len = 1;
      for (int steps = 0; steps < N; steps++) {
        if (pass == 1)
          for (int c = 0; c < d; c++) P[(int64_t)(rows - 1 - len) * d + c] = a.Q[(int64_t)v * d + c];
        const double dv = dist[v];
        bool at_start = false;
        for (int j = 0; j < cs; j++) at_start |= sv[j] != 0 && sj[j] == v && sqrt(sd[j]) == dv;
        if (at_start) break;
        int next = -1;
        for (int p = a.row_off[v]; p < a.row_off[v + 1] && next < 0; p++) {
          const int u = a.adj[p];
          if ((unsigned)u < (unsigned)N && dist[u] + a.w[p] == dv) next = u;
        }
        if (next < 0) break;  // (a graph that is not the build's: the chain ends here)
        v = next;
        len++;
      }
      if (pass == 1) break;
      rows = len + 2;
      if (rows > a.max_rows) break;
    }
    if (rows > a.max_rows) {
      status = kRmLong;
      rows = 0;
    } else {
      status = kRmSolved;
      for (int c = 0; c < d; c++) {
        P[c] = qi[c];
        P[(int64_t)(rows - 1) * d + c] = qg[c];
      }
    }
  }
  a.n_out[b] = rows;
  a.status[b] = status;
  if (a.cost) a.cost[b] = status == kRmSolved ? total : 0.0;
}

}  // namespace mjpl
