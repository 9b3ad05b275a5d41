// mjpl_push.h -- push configurations out to a minimum clearance (mjpl_push_out*, include/mjpl_hip.h).
//
// What it adds: "this configuration, moved to at least d_min from everything".  The measuring is not here: every
// iteration lists the active rows' near pairs with k_distance<DM_NEAR> (mjpl_distance.h) and the call ends with one
// k_distance<DM_CLEAR> launch over Q_out, both exactly as mjpl_near_pairs* and mjpl_clearance* launch them.  This
// header holds the step between two measurements and the two small kernels around the loop.
//
// Shape: the rows of a chunk (at most kContactRows) sit packed in a work buffer, [n][NP] with their row ids beside
// them; the near-pair outputs of a launch are indexed by the position in that buffer.  k_push_step gives every
// active row one lane.  The lane reads its K slots, sums the damped normal equations of the violated ones
//   A = damping I + sum g_p g_p^T,   b = sum r_p g_p,   r_p = d_min + overshoot - (dist_p - margin_p)
// in ascending slot order, solves A delta = b by a Cholesky factorisation in registers (NP is a constant of the
// instantiation: every loop below unrolls and no array is indexed by a run-time value), scales delta to step_max in
// the largest component, adds and clamps.  A row that ends -- nothing violated, a violated slot without a normal, a
// non-finite row, or the last iteration -- writes Q_out, iters and its flag at its own row id; a row that goes on is
// packed into the other work buffer: one ballot per wave, one atomic add per wave on the device counter the host
// reads to size the next launches.  The packed order follows the order the waves reach the atomic and may differ from
// run to run; every row's arithmetic is its own, so no result depends on it.
#pragma once

namespace mjpl {

constexpr int kPushBlock = 64;    // one wave per workgroup: the packing needs no LDS
constexpr int kPushMaxPlan = 16;  // planning columns k_push_step is instantiated for (1..16)

template <int NP>
struct PushBounds {
  double lo[NP], hi[NP];  // (-inf / +inf where the caller gave none)
};

struct PushStep {
  // the active rows, packed: [n][NP] and the row's index in its chunk
  const double *rows;
  const int *ids;
  int n;
  // the other work buffer and its fill counter
  double *next_rows;
  int *next_ids;
  int *next_n;
  // near pairs of the active rows (k_distance<DM_NEAR> on `rows`): K slots per row
  int K;
  const int *count, *pair, *slot_status;
  const double *dist, *grad;
  const double *cd;  // candidate table records (mjpl_contacts.h: CD_MARGIN)
  double d_min, overshoot, damping, step_max;
  int it;     // steps every active row has taken so far
  bool last;  // this is step max_iter: a row that moves ends with it
  // the call's outputs: Q_out in `layout` with N rows, chunk rows start at i0
  double *Q_out;
  int64_t N, i0;
  int layout;
  int *iters, *flag;  // (flag: the caller's status array holds MJPL_PUSH_DEGENERATE / NONFINITE until k_push_status settles it)
};

// Work buffer of a chunk: rows [i0, i0 + n) of Q as [n][nplan], ids 0..n-1.
__global__ void __launch_bounds__(256)
k_push_gather(const double *__restrict__ Q, int64_t N, int64_t i0, int n, int nplan, int layout, double *__restrict__ rows,
              int *__restrict__ ids) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int64_t i = i0 + r;
  for (int k = 0; k < nplan; k++) rows[(int64_t)r * nplan + k] = layout == MJPL_SOA ? Q[(int64_t)k * N + i] : Q[i * nplan + k];
  ids[r] = r;
}

// delta = A^-1 b for the symmetric positive definite A (lower triangle read), by Cholesky: A = L L^T in place
template <int NP>
__device__ __forceinline__ void push_solve(double (&A)[NP][NP], double (&b)[NP]) {
#pragma unroll
  for (int j = 0; j < NP; j++) {
    double s = A[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) s -= A[j][k] * A[j][k];
    const double ljj = sqrt(s);
    A[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < NP; i++) {
      double t = A[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) t -= A[i][k] * A[j][k];
      A[i][j] = t / ljj;
    }
  }
#pragma unroll
  for (int i = 0; i < NP; i++) {  // L y = b
    double t = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) t -= A[i][k] * b[k];
    b[i] = t / A[i][i];
  }
#pragma unroll
  for (int i = NP - 1; i >= 0; i--) {  // L^T x = y
    double t = b[i];
#pragma unroll
    for (int k = i + 1; k < NP; k++) t -= A[k][i] * b[k];
    b[i] = t / A[i][i];
  }
}

template <int NP>
__global__ void __launch_bounds__(kPushBlock)
k_push_step(PushStep a, PushBounds<NP> bd) {
  const int j = blockIdx.x * kPushBlock + threadIdx.x;
  const bool on = j < a.n;
  bool go = false;
  int r = 0;
  double q[NP];
#pragma unroll
  for (int k = 0; k < NP; k++) q[k] = 0.0;
  if (on) {
    r = a.ids[j];
    const int64_t i = a.i0 + r;
#pragma unroll
    for (int k = 0; k < NP; k++) q[k] = a.rows[(int64_t)j * NP + k];
    const int cnt = a.count[j];
    if (cnt < 0) {
      // a non-finite planning column: Q_out holds the caller's row already, iters 0
      a.flag[i] = MJPL_PUSH_NONFINITE;
    } else {
      double A[NP][NP], b[NP];
#pragma unroll
      for (int c = 0; c < NP; c++) {
        b[c] = 0.0;
#pragma unroll
        for (int d = 0; d <= c; d++) A[c][d] = c == d ? a.damping : 0.0;
      }
      bool violated = false, degenerate = false;
      const int m = cnt < a.K ? cnt : a.K;
      for (int s = 0; s < m; s++) {
        const int64_t at = (int64_t)j * a.K + s;
        const double v = a.dist[at] - a.cd[a.pair[at] * CD_LEN + CD_MARGIN];
        if (!(v < a.d_min)) continue;
        violated = true;
        if (a.slot_status[at] == GS_DEGENERATE) {
          degenerate = true;
          continue;
        }
        const double res = a.d_min + a.overshoot - v;
        double g[NP];
#pragma unroll
        for (int c = 0; c < NP; c++) g[c] = a.grad[at * NP + c];
#pragma unroll
        for (int c = 0; c < NP; c++) {
          b[c] += res * g[c];
#pragma unroll
          for (int d = 0; d <= c; d++) A[c][d] += g[c] * g[d];
        }
      }
      int steps = a.it;
      bool ends = true;
      if (degenerate) {
        a.flag[i] = MJPL_PUSH_DEGENERATE;
      } else if (violated) {
        push_solve<NP>(A, b);
        double big = 0.0;
#pragma unroll
        for (int c = 0; c < NP; c++) big = fmax(big, fabs(b[c]));
        const double scale = big > a.step_max ? a.step_max / big : 1.0;
#pragma unroll
        for (int c = 0; c < NP; c++) {
          const double d = big > a.step_max ? b[c] * scale : b[c];
          q[c] = fmin(fmax(q[c] + d, bd.lo[c]), bd.hi[c]);
        }
        steps = a.it + 1;
        ends = a.last;
      }
      if (ends) {
#pragma unroll
        for (int c = 0; c < NP; c++) a.Q_out[a.layout == MJPL_SOA ? (int64_t)c * a.N + i : i * NP + c] = q[c];
        a.iters[i] = steps;
      } else {
        go = true;
      }
    }
  }
  // the rows that go on, packed into the other buffer: one atomic per wave
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(go);
  if (mask == 0ull) return;
  const int first = (int)__builtin_ctzll(mask);
  const int lane = (int)(threadIdx.x & 63);
  int base = 0;
  if (lane == first) base = atomicAdd(a.next_n, (int)__popcll(mask));
  base = __shfl(base, first);
  if (go) {
    const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    const int64_t slot = base + before;
#pragma unroll
    for (int c = 0; c < NP; c++) a.next_rows[slot * NP + c] = q[c];
    a.next_ids[slot] = r;
  }
}

// The status rule: MJPL_PUSH_OK iff clear >= d_min; otherwise what the loop flagged (DEGENERATE) or STUCK.  A
// NONFINITE row keeps its flag (its clear is NaN).
__global__ void __launch_bounds__(256)
k_push_status(int64_t N, const double *__restrict__ clear, double d_min, int *__restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int f = status[i];
  if (f == MJPL_PUSH_NONFINITE) return;
  status[i] = clear[i] >= d_min ? MJPL_PUSH_OK : (f == MJPL_PUSH_DEGENERATE ? MJPL_PUSH_DEGENERATE : MJPL_PUSH_STUCK);
}

}  // namespace mjpl
