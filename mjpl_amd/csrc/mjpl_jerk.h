// mjpl_jerk.h -- batched jerk-limited path parameterisation (mjpl_jerk_profile*, mjpl_jerk_sample*, include/mjpl_hip.h).
//
// What it adds: "this path without stopping, every column's velocity, acceleration and jerk within its limit at every
// instant".  tests/jerk_reference.py is the NumPy statement of every number below, operation for operation; DESIGN.md
// 5.14 has the derivation and the proof of the guarantee.  All float64, no atomics: every result has one writer and one
// order of operations, so two runs give the same bits.
//
// Per path: the natural cubic spline of mjpl_topp.h (k_topp_spline's M, topp_eval), a grid of N = (n-1) G intervals of
// width D = 1/N whose grid points are the junctions.  At junction i the path speed is v_i and the path acceleration 0.
// Interval i has scalar limits (V_i, A_i, J_i) on (sdot, |sddot|, |sdddot|) under which every column keeps its limits;
// inside it the speed ramps from v_i up to vp_i, cruises for tc_i and ramps down to v_{i+1}, seven phases of constant
// path jerk.
//
// Kernels, in launch order (after k_topp_spline):
//   k_jerk_bounds     one lane per (interval, column), sixteen lanes per interval: the exact maxima p1, p2, p3 of |q'|,
//                     |q''|, |q'''| over the interval, then V, A, J one after the other, each a minimum over the row of
//                     sixteen lanes by DPP (each depends on the one before: one kernel keeps p1, p2, p3 in registers
//                     where three launches would compute or store them three times).
//   k_jerk_sweep      one wave per path: the junction speeds, backward then forward.  Every step is one section search
//                     (jerk_search) whose 64 candidates are the wave's 64 lanes; v leaves in blocks of 64 junctions.
//   k_jerk_intervals  one wave per interval: the peak speed by the same search, the cruise time, the interval's duration.
//   k_jerk_times      one wave per path: the prefix of the durations in grid order, in blocks of 64, and the status.
//   k_jerk_sample     one lane per sample of the whole batch: its path, its interval, the phase walk, the spline.
#pragma once

namespace mjpl {

constexpr int kJerkSweepWaves = 4;  // paths per workgroup of k_jerk_sweep and k_jerk_times, intervals of k_jerk_intervals
constexpr int kJerkRounds = 10;     // rounds of a section search: the bracket shrinks by 64 in each
constexpr int kJerkCbrtSteps = 8;   // Newton steps of jerk_cbrt

struct JerkBatch {
  const double *W;        // [wp_off[B]][d]
  const int64_t *wp_off;  // [B + 1], device
  int B, d, G;
  const double *lim;      // [3][d]: velocity, acceleration, jerk (magnitudes)
  double *M;              // [wp_off[B]][d] (k_topp_spline's; NaN-filled for a path that is not finite)
  int64_t pts;            // g_off[B]: the grid points of the batch
  // outputs, packed at g_off: L [pts][3] = (V, A, J) per interval, v per junction, vp and tc per interval
  double *L, *v, *vp, *tc, *t;
  int32_t *status;
};

// The cube root of x > 0 (0, inf and NaN come back as they are): the seed 2^ceil(e / 3) for x = m 2^e, 0.5 <= m < 1, is at
// most twice the root, and kJerkCbrtSteps Newton steps from above end within an ulp or two of it.  The statement does the
// same operations, so both sides agree to the bit where the library's cbrt and NumPy's need not.
__device__ __forceinline__ double jerk_cbrt(double x) {
  if (!(x > 0.0) || !(x < INFINITY)) return x;
  int e;
  (void)frexp(x, &e);
  double y = ldexp(1.0, e > 0 ? (e + 2) / 3 : -((-e) / 3));
  for (int k = 0; k < kJerkCbrtSteps; k++) y = (2.0 * y + x / (y * y)) / 3.0;
  return y;
}

// min over each row of 16 lanes, the same value in all 16 (every lane of the wave active)
__device__ __forceinline__ double jerk_min16(double v) {
  v = fmin(v, topp_dpp<0xB1>(v));   // quad_perm [1, 0, 3, 2]
  v = fmin(v, topp_dpp<0x4E>(v));   // quad_perm [2, 3, 0, 1]
  v = fmin(v, topp_dpp<0x141>(v));  // row_half_mirror
  v = fmin(v, topp_dpp<0x140>(v));  // row_mirror
  return v;
}

// ---- bounds: sixteen lanes per grid point of the batch, lane j < d its column.  No lane leaves before the reductions.
__global__ void __launch_bounds__(256) k_jerk_bounds(JerkBatch a) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t pt = slot >> 4;
  const int j = (int)(slot & 15);
  const bool row = pt < a.pts;
  int64_t w0 = 0, i = 0;
  int n = 2;
  if (row) {
    const int b = topp_path_of(a.wp_off, a.G, 0, a.B, pt);
    w0 = a.wp_off[b];
    n = (int)(a.wp_off[b + 1] - w0);
    i = pt - topp_g_off(a.wp_off, a.G, b);
  }
  const int64_t N = (int64_t)(n - 1) * a.G;
  const bool live = row && i < N && j < a.d;  // (i == N: the path's last grid point starts no interval)
  double p1 = 0.0, p2 = 0.0, p3 = 0.0, vl = 1.0, al = 1.0, jl = 1.0;
  if (live) {
    const int64_t k = i / a.G;  // (i < N: k <= n - 2)
    const double r = (double)(n - 1);
    const double B0 = (double)(i - k * a.G) / (double)a.G, B1 = (double)(i + 1 - k * a.G) / (double)a.G;
    const int64_t at = (w0 + k) * a.d + j;
    const double W0 = a.W[at], W1 = a.W[at + a.d], M0 = a.M[at], M1 = a.M[at + a.d];
    double q, a0, b0, a1, b1;
    topp_eval(W0, W1, M0, M1, r, B0, q, a0, b0);
    topp_eval(W0, W1, M0, M1, r, B1, q, a1, b1);
    p1 = fmax(fabs(a0), fabs(a1));
    if (b0 * b1 < 0.0) {  // q'' changes sign: q' has its vertex inside
      const double Bv = B0 + (b0 / (b0 - b1)) * (B1 - B0);
      double av, bv;
      topp_eval(W0, W1, M0, M1, r, Bv, q, av, bv);
      p1 = fmax(p1, fabs(av));
    }
    p2 = fmax(fabs(b0), fabs(b1));
    p3 = fabs(M1 - M0) * r;
    vl = a.lim[j];
    al = a.lim[a.d + j];
    jl = a.lim[2 * a.d + j];
  }
  // (a lane that is not live has p1 = p2 = p3 = 0: every term of it is +inf.  NaN is kept: fmin would drop it.)
  const bool nan = p1 != p1 || p2 != p2 || p3 != p3;
  double c = INFINITY;
  if (p1 != 0.0) c = fmin(c, vl / p1);
  if (p2 != 0.0) c = fmin(c, sqrt(al / (2.0 * p2)));
  if (p3 != 0.0) c = fmin(c, jerk_cbrt(jl / (3.0 * p3)));
  const double V = jerk_min16(c);
  double A = INFINITY, J = INFINITY;
  if (V < INFINITY) {  // (row-uniform)
    c = INFINITY;
    if (p1 != 0.0) c = fmin(c, (al - p2 * (V * V)) / p1);
    if (p2 != 0.0) c = fmin(c, jl / ((9.0 * p2) * V));
  }
  const double Am = jerk_min16(c);
  if (V < INFINITY) {
    A = Am;
    c = INFINITY;
    if (p1 != 0.0) c = fmin(c, ((jl - p3 * ((V * V) * V)) - ((3.0 * p2) * V) * A) / p1);
  }
  const double Jm = jerk_min16(c);
  if (V < INFINITY) J = Jm;
  const double any_nan = jerk_min16(nan ? 0.0 : 1.0);
  if (row && j == 0) {
    double *L = a.L + 3 * pt;
    if (i >= N) L[0] = L[1] = L[2] = 0.0;
    else if (any_nan == 0.0) L[0] = L[1] = L[2] = NAN;
    else { L[0] = V; L[1] = A; L[2] = J; }
  }
}

// ---- ramps: a speed change dv >= 0 with zero path acceleration at both ends, under |sddot| <= A and |sdddot| <= J
__device__ __forceinline__ double jerk_ramp_time(double dv, double A, double J) {
  return dv >= (A * A) / J ? dv / A + A / J : 2.0 * sqrt(dv / J);
}

// the length of the ramp between the speeds va <= vb
__device__ __forceinline__ double jerk_ramp_len(double va, double vb, double A, double J) {
  return ((va + vb) * 0.5) * jerk_ramp_time(vb - va, A, J);
}

// the ramp as phases: tj of jerk +-J, ta of constant acceleration, tj of jerk -+J
__device__ __forceinline__ void jerk_ramp_phases(double dv, double A, double J, double &tj, double &ta) {
  if (dv >= (A * A) / J) {
    tj = A / J;
    ta = dv / A - tj;
  } else {
    tj = sqrt(dv / J);
    ta = 0.0;
  }
}

// ---- the section search: the largest x in [lo, hi] with f(x) <= h, for a monotone f with f(lo) <= h.  One wave, every
// lane active, lo / hi / h the same in all of them.  A round takes the 64 candidates lo + (hi - lo) (l + 1) / 64, one f
// per lane; the ballot counts the leading feasible ones and the new bracket ends are read from the two lanes at the
// boundary.  The result is a feasible candidate (or lo).  A NaN anywhere is infeasible: the rounds still end.
template <class F>
__device__ __forceinline__ double jerk_search(const F &f, double lo, double hi, double h, int lane) {
  if (f(hi) <= h) return hi;
  const double frac = (double)(lane + 1) / 64.0;
  for (int r = 0; r < kJerkRounds; r++) {
    const double c = lo + (hi - lo) * frac;
    const unsigned long long ok = __ballot(f(c) <= h);
    const int m = __builtin_amdgcn_readfirstlane(ok == ~0ull ? 64 : __ffsll((long long)~ok) - 1);
    const double below = topp_readlane(c, max(m - 1, 0)), above = topp_readlane(c, min(m, 63));
    if (m > 0) lo = below;
    if (m < 64) hi = above;
  }
  return lo;
}

// What a path that is not finite leaves: NaN everywhere (its neighbours in the batch are not touched)
__device__ __forceinline__ void jerk_fill_nan(const JerkBatch &a, int64_t w0, int64_t nw, int64_t go, int N, int lane) {
  for (int64_t k = lane; k < nw; k += 64) a.M[w0 * a.d + k] = NAN;
  for (int k = lane; k <= N; k += 64) {
    a.L[3 * (go + k)] = a.L[3 * (go + k) + 1] = a.L[3 * (go + k) + 2] = NAN;
    a.v[go + k] = a.vp[go + k] = a.tc[go + k] = a.t[go + k] = NAN;
  }
}

// ---- junction speeds: one wave per path
__global__ void __launch_bounds__(64 * kJerkSweepWaves) k_jerk_sweep(JerkBatch a) {
  const int lane = threadIdx.x & 63;
  const int b = (int)blockIdx.x * kJerkSweepWaves + (int)(threadIdx.x >> 6);
  if (b >= a.B) return;  // (wave-uniform)
  const int64_t w0 = a.wp_off[b];
  const int n = (int)(a.wp_off[b + 1] - w0);
  const int N = (n - 1) * a.G;
  const int64_t go = topp_g_off(a.wp_off, a.G, b);
  const int64_t nw = (int64_t)n * a.d;
  const double *L = a.L + 3 * go;
  double *v = a.v + go;

  bool bad = false, still = false;
  for (int64_t k = lane; k < nw; k += 64) bad |= !isfinite(a.W[w0 * a.d + k]) || !isfinite(a.M[w0 * a.d + k]);
  for (int k = lane; k < N; k += 64) {
    const double Vk = L[3 * k], Ak = L[3 * k + 1], Jk = L[3 * k + 2];
    bad |= Vk != Vk || Ak != Ak || Jk != Jk;
    still |= Vk == INFINITY;
  }
  if (__ballot(bad) != 0ull) {
    jerk_fill_nan(a, w0, nw, go, N, lane);
    if (lane == 0) a.status[b] = kToppNonFinite;
    return;
  }
  if (__ballot(still) != 0ull) {  // some interval on which nothing moves: it takes for ever
    for (int k = lane; k <= N; k += 64) {
      v[k] = 0.0;
      a.vp[go + k] = 0.0;
      a.tc[go + k] = k < N ? INFINITY : 0.0;
      a.t[go + k] = k > 0 ? INFINITY : 0.0;
    }
    if (lane == 0) a.status[b] = kToppStalled;
    return;
  }
  const double D = 1.0 / (double)N;

  // backward: v_N = 0; v_i = its cap c_i = min(V_{i-1}, V_i) (c_0 = 0) where that is no faster than v_{i+1}, else the
  // fastest speed from which a ramp down to v_{i+1} fits the interval.  Lane k of a block holds interval base + k.
  double vnext = 0.0;
  if (lane == 0) v[N] = 0.0;
  for (int base = ((N - 1) >> 6) << 6; base >= 0; base -= 64) {
    const int cnt = min(64, N - base), idx = base + min(lane, cnt - 1);
    const double Vk = L[3 * idx], Ak = L[3 * idx + 1], Jk = L[3 * idx + 2];
    const double Vprev = L[3 * max(idx - 1, 0)];
    const double ck = idx == 0 ? 0.0 : fmin(Vprev, Vk);
    double vk = 0.0;
    for (int k = cnt - 1; k >= 0; k--) {
      const double c = topp_readlane(ck, k), A = topp_readlane(Ak, k), J = topp_readlane(Jk, k);
      double vi = c;
      if (!(c <= vnext)) {
        const double vn = vnext;
        vi = jerk_search([=](double x) { return jerk_ramp_len(vn, x, A, J); }, vn, c, D, lane);
      }
      if (lane == k) vk = vi;
      vnext = vi;
    }
    if (lane < cnt) v[base + lane] = vk;
  }
  __threadfence();  // v was written a lane per junction and is read below by other lanes

  // forward: v_0 = 0; where v_{i+1} > v_i, no faster than a ramp up from v_i within the interval reaches.  Lane k of a
  // block holds interval base + k and junction base + k + 1.
  double vcur = 0.0;
  for (int base = 0; base < N; base += 64) {
    const int cnt = min(64, N - base), idx = base + min(lane, cnt - 1);
    const double Ak = L[3 * idx + 1], Jk = L[3 * idx + 2], vb = v[idx + 1];
    double vk = 0.0;
    for (int k = 0; k < cnt; k++) {
      const double A = topp_readlane(Ak, k), J = topp_readlane(Jk, k);
      double vn = topp_readlane(vb, k);
      if (vn > vcur) {
        const double vc = vcur;
        vn = jerk_search([=](double x) { return jerk_ramp_len(vc, x, A, J); }, vc, vn, D, lane);
      }
      if (lane == k) vk = vn;
      vcur = vn;
    }
    if (lane < cnt) v[base + 1 + lane] = vk;
  }
  if (lane == 0) a.status[b] = kToppOk;  // (k_jerk_times has the last word)
}

// ---- interval profiles: one wave per grid point of the batch
__global__ void __launch_bounds__(64 * kJerkSweepWaves) k_jerk_intervals(JerkBatch a) {
  const int lane = threadIdx.x & 63;
  const int64_t pt = (int64_t)blockIdx.x * kJerkSweepWaves + (int64_t)(threadIdx.x >> 6);
  if (pt >= a.pts) return;  // (wave-uniform, like everything up to the search)
  const int b = topp_path_of(a.wp_off, a.G, 0, a.B, pt);
  if (a.status[b] != kToppOk) return;  // k_jerk_sweep has filled the path's outputs
  const int64_t w0 = a.wp_off[b];
  const int N = (int)(a.wp_off[b + 1] - w0 - 1) * a.G;
  const int64_t i = pt - topp_g_off(a.wp_off, a.G, b);
  if (i >= N) {  // the path's last grid point starts no interval
    if (lane == 0) {
      a.vp[pt] = 0.0;
      a.tc[pt] = 0.0;
    }
    return;
  }
  const double D = 1.0 / (double)N;
  const double v0 = a.v[pt], v1 = a.v[pt + 1], V = a.L[3 * pt], A = a.L[3 * pt + 1], J = a.L[3 * pt + 2];
  const auto both = [=](double x) { return jerk_ramp_len(v0, x, A, J) + jerk_ramp_len(v1, x, A, J); };
  const double vp = jerk_search(both, fmax(v0, v1), V, D, lane);
  const double tc = fmax((D - both(vp)) / vp, 0.0);
  const double dur = (jerk_ramp_time(vp - v0, A, J) + tc) + jerk_ramp_time(vp - v1, A, J);
  if (lane == 0) {
    a.vp[pt] = vp;
    a.tc[pt] = tc;
    a.t[pt + 1] = dur;  // (k_jerk_times turns the durations into times)
  }
}

// ---- times: one wave per path.  t_0 = 0, t_{i+1} = t_i + the duration of interval i, summed in grid order
__global__ void __launch_bounds__(64 * kJerkSweepWaves) k_jerk_times(JerkBatch a) {
  const int lane = threadIdx.x & 63;
  const int b = (int)blockIdx.x * kJerkSweepWaves + (int)(threadIdx.x >> 6);
  if (b >= a.B) return;  // (wave-uniform)
  if (a.status[b] != kToppOk) return;
  const int64_t w0 = a.wp_off[b];
  const int n = (int)(a.wp_off[b + 1] - w0);
  const int N = (n - 1) * a.G;
  const int64_t go = topp_g_off(a.wp_off, a.G, b);
  double *t = a.t + go;
  double tacc = 0.0;
  bool bad = false;
  if (lane == 0) t[0] = 0.0;
  for (int base = 0; base < N; base += 64) {
    const int cnt = min(64, N - base);
    const bool have = lane < cnt;
    const double dti = have ? t[base + lane + 1] : 0.0;
    double tk = 0.0;
    for (int k = 0; k < 64; k++) {  // the prefix in grid order (lanes past the block add 0)
      tacc = tacc + topp_readlane(dti, k);
      if (lane == k) tk = tacc;
    }
    if (have) {
      t[base + lane + 1] = tk;
      bad |= !isfinite(tk) || !isfinite(a.v[go + base + lane]) || !isfinite(a.vp[go + base + lane]) || !isfinite(a.tc[go + base + lane]);
    }
  }
  if (__ballot(bad) != 0ull) {  // a result that is not finite
    jerk_fill_nan(a, w0, (int64_t)n * a.d, go, N, lane);
    if (lane == 0) a.status[b] = kToppNonFinite;
  }
}

// ---- sampling: one lane per sample of the whole batch
struct JerkSamples {
  const double *W, *M, *L, *v, *vp, *tc, *t;
  const int64_t *wp_off, *samp_off;  // [B + 1] each, device
  int B, d, G;
  double dt;
  double *pos, *vel, *acc;  // [samp_off[B]][d]
};

// (s, sdot, sddot) after the time h of constant path jerk jk
__device__ __forceinline__ void jerk_advance(double &s, double &sd, double &sdd, double h, double jk) {
  const double h2 = h * h;
  s = s + ((sd * h + (0.5 * sdd) * h2) + (jk * (h2 * h)) / 6.0);
  sd = sd + (sdd * h + (0.5 * jk) * h2);
  sdd = sdd + jk * h;
}

__global__ void __launch_bounds__(256) k_jerk_sample(JerkSamples a) {
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
  const double D = 1.0 / (double)N;
  const double v0 = a.v[go + i], v1 = a.v[go + i + 1], A = a.L[3 * (go + i) + 1], J = a.L[3 * (go + i) + 2];
  const double vp = a.vp[go + i];
  double h[7], jk[7];
  jerk_ramp_phases(vp - v0, A, J, h[0], h[1]);
  jerk_ramp_phases(vp - v1, A, J, h[4], h[5]);
  h[2] = h[0];
  h[3] = a.tc[go + i];
  h[6] = h[4];
  jk[0] = J; jk[1] = 0.0; jk[2] = -J; jk[3] = 0.0; jk[4] = -J; jk[5] = 0.0; jk[6] = J;
  // walk the phases from (0, v_i, 0) to the one that holds tau; at or past the interval's end: (D, v_{i+1}, 0)
  double tau = tk - t[i], s = 0.0, sd = v0, sdd = 0.0, jin = 0.0;
  bool inside = false;
  if (!(tau >= t[i + 1] - t[i])) {
#pragma unroll
    for (int p = 0; p < 7; p++) {
      if (!inside) {
        if (tau < h[p]) {
          inside = true;
          jin = jk[p];
        } else {
          jerk_advance(s, sd, sdd, h[p], jk[p]);
          tau = tau - h[p];
        }
      }
    }
  }
  if (inside) {
    jerk_advance(s, sd, sdd, tau, jin);
  } else {
    s = D;
    sd = v1;
    sdd = 0.0;
  }
  s = (double)i / (double)N + fmin(fmax(s, 0.0), D);
  const double z = fmin(fmax(s, 0.0), 1.0) * (double)(n - 1);
  int k = (int)floor(z);
  if (k > n - 2) k = n - 2;
  if (k < 0) k = 0;
  const double Bc = z - (double)k;
  for (int j = 0; j < a.d; j++) {
    const int64_t at = (w0 + k) * a.d + j;
    double q, q1, q2;
    topp_eval(a.W[at], a.W[at + a.d], a.M[at], a.M[at + a.d], (double)(n - 1), Bc, q, q1, q2);
    a.pos[idx * a.d + j] = q;
    a.vel[idx * a.d + j] = q1 * sd;
    a.acc[idx * a.d + j] = q2 * (sd * sd) + q1 * sdd;
  }
}

}  // namespace mjpl
