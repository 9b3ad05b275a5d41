// mjpl_topp.h -- batched time-optimal path parameterisation (mjpl_topp_profile*, mjpl_topp_sample*, include/mjpl_hip.h).
//
// What it adds: "this path, as fast as the velocity and acceleration limits allow".  tests/trajectory_reference.py is
// the NumPy statement of every number below, operation for operation; DESIGN.md 5.12 has the derivation.  All float64,
// no atomics: every result has one writer and one order of operations, so two runs give the same bits.
//
// Per path: a natural cubic spline through the n waypoints at the knots k / (n-1), a grid of N = (n-1) G intervals of
// width D = 1/N, x_i = sdot^2 at the grid points, u_i = sddot on interval i.  The constraints of interval i are lines
// in (u, x): per ROW r < 2d (column r % d at the left end of the interval for r < d, at the right end otherwise) a
// lower line u >= p + rho x and an upper line u <= P + rho x, and the reachability lines 0 <= x + 2D u <= K_{i+1}.
//
// Kernels, in launch order:
//   k_topp_spline  one lane per (path, column): the Thomas recurrence for the knot second derivatives M.
//   k_topp_lines   one lane per (grid point, row): the row's upper line (P, rho) into the workspace.
//   k_topp_pairs   one lane per (grid point, row): the row's own lower line again, its operands (pp, g) of the one
//                  quotient that depends on K_{i+1}, and s = the least of everything that does not -- the row's lower
//                  line against every row's upper line (read from the workspace), its upper line against u >= -x / 2D,
//                  its column's velocity cap, its own cap if it has no u.
//   k_topp_sweep   one wave per path.  Backward: lane r < 2d holds min(s_r, (K_{i+1} - pp_r) g_r), one wave-wide min
//                  gives K_i: a subtraction, a product and the reduction are the whole serial chain of a grid point.
//                  Forward: lane r holds P_r + rho_r x_i, the wave-wide min is u_i.  Per-point data comes from the
//                  workspace (a path of hundreds of waypoints does not fit the LDS), loaded one step ahead of its use.
//                  x, u and the interval times leave in blocks of 64 grid points, one lane each; the time prefix is
//                  summed in grid order inside the same wave.
//   k_topp_sample  one lane per sample of the whole batch: a binary search for its path, one in t for its interval.
// The workspace is sized per chunk of paths (launch_topp_profile), so its size bounds no batch.
#pragma once

namespace mjpl {

constexpr int kToppMaxCols = 16;   // columns per waypoint (2 d <= 32 rows: half a wave)
constexpr int kToppSweepWaves = 4; // paths per workgroup of k_topp_sweep
constexpr int kToppOk = 0, kToppStalled = 1, kToppNonFinite = 2;  // MJPL_TOPP_*

struct ToppBatch {
  const double *W;        // [wp_off[B]][d]
  const int64_t *wp_off;  // [B + 1], device
  int B, d, G;
  const double *lim;      // [4][d]: vmin, vmax, amin, amax
  const double *cp;       // c' of the Thomas recurrence, [>= the longest path]
  double *M;              // [wp_off[B]][d]
  // the chunk: paths [b0, b1), grid points [g0, g0 + pts); workspace arrays [pts][2d] and K [pts]
  int b0, b1;
  int64_t g0, pts;
  double *wP, *wrho, *wpp, *wg, *ws, *wK;
  // outputs, packed at g_off
  double *x, *u, *t;
  int32_t *status;
};

// first grid point of path b: every path before it holds G (n - 1) + 1 of them
__device__ __forceinline__ int64_t topp_g_off(const int64_t *wp_off, int G, int b) { return (int64_t)G * (wp_off[b] - b) + b; }

// the path in [b0, b1) that holds grid point pt (g_off(b0) <= pt < g_off(b1))
__device__ __forceinline__ int topp_path_of(const int64_t *wp_off, int G, int b0, int b1, int64_t pt) {
  int lo = b0, hi = b1 - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (topp_g_off(wp_off, G, mid) <= pt) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// q, q', q'' of one column on segment k at the local coordinate Bc (W0 = W[k][j], ...; r = n - 1)
__device__ __forceinline__ void topp_eval(double W0, double W1, double M0, double M1, double r, double Bc, double &q, double &q1,
                                          double &q2) {
  const double A = 1.0 - Bc;
  q = (A * W0 + Bc * W1) + ((A * A * A - A) * M0 + (Bc * Bc * Bc - Bc) * M1) / (6.0 * r * r);
  q1 = (W1 - W0) * r + ((3.0 * Bc * Bc - 1.0) * M1 - (3.0 * A * A - 1.0) * M0) / (6.0 * r);
  q2 = A * M0 + Bc * M1;
}

// a = q', b = q'' of column j at grid point i of a path of n waypoints starting at row w0
__device__ __forceinline__ void topp_grid_ab(const ToppBatch &a, int64_t w0, int n, int64_t i, int j, double &qa, double &qb) {
  int64_t k = i / a.G;
  if (k > n - 2) k = n - 2;
  const double Bc = (double)(i - k * a.G) / (double)a.G;
  const int64_t at = (w0 + k) * a.d + j;
  double q;
  topp_eval(a.W[at], a.W[at + a.d], a.M[at], a.M[at + a.d], (double)(n - 1), Bc, q, qa, qb);
}

// One row of one interval: its lines u >= p + rho x, u <= P + rho x (a row without u: p = -inf, P = +inf, rho = 0,
// alive false) and what else the row puts on x by itself (cap: the velocity cap of a left-end row, the cap of a row
// without u)
struct ToppRow {
  double p, P, rho, cap;
  bool alive;
};

__device__ __forceinline__ ToppRow topp_row(const ToppBatch &a, int64_t w0, int n, int64_t i, int row, double twoD) {
  const int e = row >= a.d ? 1 : 0, j = row - e * a.d;
  double qa, qb;
  topp_grid_ab(a, w0, n, i + e, j, qa, qb);
  const double c = e ? qa + twoD * qb : qa;
  const double amin = a.lim[2 * a.d + j], amax = a.lim[3 * a.d + j];
  ToppRow r;
  r.alive = c != 0.0;
  r.cap = INFINITY;
  if (r.alive) {
    r.p = (c > 0.0 ? amin : amax) / c;
    r.P = (c > 0.0 ? amax : amin) / c;
    r.rho = -(qb / c);
  } else {
    r.p = -INFINITY;
    r.P = INFINITY;
    r.rho = 0.0;
    if (qb != 0.0) r.cap = (qb > 0.0 ? amax : amin) / qb;
  }
  if (!e && qa != 0.0) {
    const double v = (qa > 0.0 ? a.lim[a.d + j] : a.lim[j]) / qa;
    r.cap = fmin(r.cap, v * v);
  }
  return r;
}

// ---- spline: one lane per (path, column)
__global__ void __launch_bounds__(256) k_topp_spline(ToppBatch a) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)a.B * a.d) return;
  const int b = (int)(idx / a.d), j = (int)(idx - (int64_t)b * a.d);
  const int64_t w0 = a.wp_off[b];
  const int n = (int)(a.wp_off[b + 1] - w0);
  const double *W = a.W + w0 * a.d + j;
  double *M = a.M + w0 * a.d + j;
  const int64_t d = a.d;
  M[0] = 0.0;
  M[(n - 1) * d] = 0.0;
  if (n == 2) return;
  const double scale = (double)(6 * (int64_t)(n - 1) * (int64_t)(n - 1));
  double prev = 0.0, w_lo = W[0], w_mid = W[d];
  for (int k = 1; k < n - 1; k++) {
    const double w_hi = W[(k + 1) * d];
    const double rhs = ((w_hi - w_mid) - (w_mid - w_lo)) * scale;
    prev = (rhs - prev) / (4.0 - a.cp[k - 1]);
    M[k * d] = prev;
    w_lo = w_mid;
    w_mid = w_hi;
  }
  for (int k = n - 3; k >= 1; k--) {
    prev = M[k * d] - a.cp[k] * prev;
    M[k * d] = prev;
  }
}

// (grid point, row) of a lane of the two grid kernels; false: nothing to do (past the chunk, or the path's last point)
__device__ __forceinline__ bool topp_lane(const ToppBatch &a, int64_t &slot, int64_t &w0, int &n, int64_t &i, int &row, double &twoD) {
  const int rows = 2 * a.d;
  slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= a.pts * rows) return false;
  const int64_t pl = slot / rows;
  row = (int)(slot - pl * rows);
  const int b = topp_path_of(a.wp_off, a.G, a.b0, a.b1, a.g0 + pl);
  w0 = a.wp_off[b];
  n = (int)(a.wp_off[b + 1] - w0);
  i = a.g0 + pl - topp_g_off(a.wp_off, a.G, b);
  const int64_t N = (int64_t)(n - 1) * a.G;
  twoD = 2.0 * (1.0 / (double)N);
  return i < N;
}

__global__ void __launch_bounds__(256) k_topp_lines(ToppBatch a) {
  int64_t slot, w0, i;
  int n, row;
  double twoD;
  if (!topp_lane(a, slot, w0, n, i, row, twoD)) return;
  const ToppRow r = topp_row(a, w0, n, i, row, twoD);
  a.wP[slot] = r.P;
  a.wrho[slot] = r.rho;
}

__global__ void __launch_bounds__(256) k_topp_pairs(ToppBatch a) {
  int64_t slot, w0, i;
  int n, row;
  double twoD;
  if (!topp_lane(a, slot, w0, n, i, row, twoD)) return;
  const ToppRow r = topp_row(a, w0, n, i, row, twoD);
  double s = r.cap;
  double pp = -INFINITY, g = 1.0;
  if (r.alive) {
    // the row's lower line against every row's upper line
    const int rows = 2 * a.d;
    const int64_t base = slot - row;
    for (int l = 0; l < rows; l++) {
      const double Pl = a.wP[base + l], D = r.rho - a.wrho[base + l];
      if (Pl < INFINITY && D > 0.0) s = fmin(s, (Pl - r.p) / D);
    }
    // its upper line against u >= -x / 2D
    const double e = -(1.0 / twoD) - r.rho;
    if (e > 0.0) s = fmin(s, r.P / e);
    // its lower line against u <= (K - x) / 2D: x = (K - pp) g
    const double den = 1.0 + twoD * r.rho;
    if (den > 0.0) {
      pp = r.p * twoD;
      g = 1.0 / den;
    }
  }
  a.wpp[slot] = pp;
  a.wg[slot] = g;
  a.ws[slot] = s;
}

// ---- cross-lane helpers of the sweeps (wave64; every lane active)
template <int CTRL>
__device__ __forceinline__ double topp_dpp(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double topp_readlane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// min over lanes 0..31, the same value in every lane: four DPP steps inside each row of 16 lanes (swap neighbours,
// swap pairs, mirror the half row, mirror the row), then the two rows' results from lanes 0 and 16
__device__ __forceinline__ double topp_min32(double v) {
  v = fmin(v, topp_dpp<0xB1>(v));   // quad_perm [1, 0, 3, 2]
  v = fmin(v, topp_dpp<0x4E>(v));   // quad_perm [2, 3, 0, 1]
  v = fmin(v, topp_dpp<0x141>(v));  // row_half_mirror
  v = fmin(v, topp_dpp<0x140>(v));  // row_mirror
  return fmin(topp_readlane(v, 0), topp_readlane(v, 16));
}

// ---- sweeps: one wave per path
__global__ void __launch_bounds__(64 * kToppSweepWaves) k_topp_sweep(ToppBatch a) {
  const int lane = threadIdx.x & 63;
  const int b = a.b0 + (int)blockIdx.x * kToppSweepWaves + (int)(threadIdx.x >> 6);
  if (b >= a.b1) return;  // (wave-uniform)
  const int64_t w0 = a.wp_off[b];
  const int n = (int)(a.wp_off[b + 1] - w0);
  const int N = (n - 1) * a.G;
  const int64_t go = topp_g_off(a.wp_off, a.G, b);  // in the outputs
  const int64_t gl = go - a.g0;                     // in the workspace
  const int rows = 2 * a.d;
  const int64_t nw = (int64_t)n * a.d;
  double *x = a.x + go, *u = a.u + go, *t = a.t + go;

  bool bad = false;
  for (int64_t k = lane; k < nw; k += 64) bad |= !isfinite(a.W[w0 * a.d + k]);
  if (__ballot(bad) != 0ull) {
    for (int64_t k = lane; k < nw; k += 64) a.M[w0 * a.d + k] = NAN;
    for (int k = lane; k <= N; k += 64) x[k] = u[k] = t[k] = NAN;
    if (lane == 0) a.status[b] = kToppNonFinite;
    return;
  }
  for (int64_t k = lane; k < nw; k += 64) bad |= !isfinite(a.M[w0 * a.d + k]);

  const bool mine = lane < rows;
  const double twoD = 2.0 * (1.0 / (double)N);

  // backward: K_N = 0, K_i = max(0, min over the rows of min(s, (K_{i+1} - pp) g)).  Every lane loads (lanes past the
  // rows read row 0 and drop it; the step before the first reads the first again): a load under a branch would have to
  // land before the branch closes, and the next step's operands are meant to be in flight during this step's chain
  const int ln = mine ? lane : 0;
  double K = 0.0;
  if (lane == 0) a.wK[gl + N] = 0.0;
  {
    int64_t at = (gl + N - 1) * rows + ln;
    double pp = a.wpp[at], g = a.wg[at], s = a.ws[at];
    for (int i = N - 1; i >= 0; i--) {
      at = (gl + max(i - 1, 0)) * rows + ln;
      const double pp_n = a.wpp[at], g_n = a.wg[at], s_n = a.ws[at];
      K = fmax(0.0, topp_min32(mine ? fmin(s, (K - pp) * g) : INFINITY));
      if (lane == 0) a.wK[gl + i] = K;
      pp = pp_n; g = g_n; s = s_n;
    }
  }
  __threadfence();  // K was written by lane 0 and is read below by every lane

  // forward, 64 intervals at a time: lane k of a block keeps x at both ends of interval base + k
  double xi = 0.0, tacc = 0.0;
  bool stalled = false;
  if (lane == 0) t[0] = 0.0;
  {
    int64_t at = gl * rows + ln;
    double P = a.wP[at], rho = a.wrho[at];
    for (int base = 0; base < N; base += 64) {
      const int cnt = min(64, N - base);
      const double Kblk = lane < cnt ? a.wK[gl + base + lane + 1] : 0.0;
      double xl = 0.0, xr = 0.0;
      for (int k = 0; k < cnt; k++) {
        const int i = base + k;
        at = (gl + min(i + 1, N - 1)) * rows + ln;
        const double P_n = a.wP[at], rho_n = a.wrho[at];
        const double um = topp_min32(mine ? P + rho * xi : INFINITY);
        const double xn = fmin(fmax(xi + twoD * um, 0.0), topp_readlane(Kblk, k));
        if (lane == k) { xl = xi; xr = xn; }
        xi = xn;
        P = P_n; rho = rho_n;
      }
      const bool have = lane < cnt;
      double dti = 0.0, ui = 0.0;
      if (have) {
        ui = (xr - xl) / twoD;
        dti = twoD / (sqrt(xl) + sqrt(xr));
        stalled |= xl == 0.0 && xr == 0.0;
      }
      double tk = 0.0;
      for (int k = 0; k < 64; k++) {  // the prefix in grid order (lanes past the block add 0)
        tacc = tacc + topp_readlane(dti, k);
        if (lane == k) tk = tacc;
      }
      if (have) {
        x[base + lane] = xl;
        u[base + lane] = ui;
        t[base + lane + 1] = tk;
        bad |= !isfinite(xl) || !isfinite(ui) || !isfinite(tk);
      }
    }
  }
  if (lane == 0) {
    x[N] = xi;
    u[N] = 0.0;
  }
  bad |= !isfinite(xi);
  const bool any_stalled = __ballot(stalled) != 0ull, any_bad = __ballot(bad) != 0ull;
  if (lane == 0) a.status[b] = any_stalled ? kToppStalled : any_bad ? kToppNonFinite : kToppOk;
}

// ---- sampling: one lane per sample of the whole batch
struct ToppSamples {
  const double *W, *M, *x, *u, *t;
  const int64_t *wp_off, *samp_off;  // [B + 1] each, device
  int B, d, G;
  double dt;
  double *pos, *vel, *acc;  // [samp_off[B]][d]
};

__global__ void __launch_bounds__(256) k_topp_sample(ToppSamples a) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.samp_off[a.B]) return;
  int lo = 0, hi = a.B - 1;  // the path: the last b with samp_off[b] <= idx (paths without samples are passed over)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.samp_off[mid] <= idx) lo = mid;
    else hi = mid - 1;
  }
  const int b = lo;
  const int64_t w0 = a.wp_off[b];
  const int n = (int)(a.wp_off[b + 1] - w0);
  const int N = (n - 1) * a.G;
  const int64_t go = topp_g_off(a.wp_off, a.G, b);
  const double *t = a.t + go;
  const double tk = fmin((double)(idx - a.samp_off[b] + 1) * a.dt, t[N]);
  lo = 0;
  hi = N - 1;  // the interval: the last i <= N - 1 with t_i <= tk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid] <= tk) lo = mid;
    else hi = mid - 1;
  }
  const int i = lo;
  const double tau = tk - t[i], r = sqrt(a.x[go + i]), ui = a.u[go + i];
  const double sd = r + ui * tau;
  const double s = (double)i / (double)N + (r * tau + 0.5 * ui * tau * tau);
  const double z = fmin(fmax(s, 0.0), 1.0) * (double)(n - 1);
  int k = (int)floor(z);
  if (k > n - 2) k = n - 2;
  const double Bc = z - (double)k;
  for (int j = 0; j < a.d; j++) {
    const int64_t at = (w0 + k) * a.d + j;
    double q, q1, q2;
    topp_eval(a.W[at], a.W[at + a.d], a.M[at], a.M[at + a.d], (double)(n - 1), Bc, q, q1, q2);
    a.pos[idx * a.d + j] = q;
    a.vel[idx * a.d + j] = q1 * sd;
    a.acc[idx * a.d + j] = q2 * (sd * sd) + q1 * ui;
  }
}

}  // namespace mjpl
