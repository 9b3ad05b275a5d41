// mjpl_pose_probe.hip -- the binary32 pose helpers of mjpl_pose_f32.h (pose_lin3 .. pose_rot_vec, sincos_half_f32) behind a
// C interface, for tests/test_pose_fma.py and tests/test_gpu_pose_fma.py.  Built twice by build.build_pose_probe():
//   libmjpl_pose_probe.so   every helper over arrays on the host, beside the UNFUSED statement the generated text held
//                           before (one rounding per operation: the translation unit's -ffp-contract=off), and
//                           sincos_half_f32 over an array on the device;
//   mjpl_pose_probe         (-DMJPL_PROBE_MAIN, host code only) the sweep of sincos_half_f32 against binary64 sin / cos:
//                           mjpl_pose_probe STRIDE THREADS -> one JSON line (STRIDE 1: every binary32 of [-3.3, 3.3]).
#include "mjpl_pose_f32.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

namespace {

#ifndef MJPL_PROBE_MAIN
__global__ void k_sincos(const float *x, float *s, float *c, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mjpl::sincos_half_f32(x[i], &s[i], &c[i]);
}
#endif

// the statements of the generated text before the helpers: plain expressions, left to right
void plain_mul_quat(float *r, const float *a, const float *b) {
  r[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  r[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  r[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  r[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

void plain_quat2mat(float *R, float q0, float q1, float q2, float q3) {
  R[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3; R[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3;
  R[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3; R[1] = 2.0f * (q1 * q2 - q0 * q3); R[2] = 2.0f * (q1 * q3 + q0 * q2);
  R[3] = 2.0f * (q1 * q2 + q0 * q3); R[5] = 2.0f * (q2 * q3 - q0 * q1); R[6] = 2.0f * (q1 * q3 - q0 * q2);
  R[7] = 2.0f * (q2 * q3 + q0 * q1);
}

void plain_rot_vec(float *r, const float *v, const float *q) {
  const float t0 = v[0] * q[0] + v[2] * q[2] - v[1] * q[3];
  const float t1 = v[1] * q[0] + v[0] * q[3] - v[2] * q[1];
  const float t2 = v[2] * q[0] + v[1] * q[1] - v[0] * q[2];
  r[0] = v[0] + 2.0f * (q[2] * t2 - q[3] * t1);
  r[1] = v[1] + 2.0f * (q[3] * t0 - q[1] * t2);
  r[2] = v[2] + 2.0f * (q[1] * t1 - q[2] * t0);
}

}  // namespace

#ifndef MJPL_PROBE_MAIN
extern "C" {

// in: n rows [base c0 x0 c1 x1 c2 x2]
void mjpl_probe_lin3(const float *in, float *out, long n, int fused) {
  for (long i = 0; i < n; i++) {
    const float *r = in + 7 * i;
    out[i] = fused ? mjpl::pose_lin3(r[0], r[1], r[2], r[3], r[4], r[5], r[6]) : r[0] + (r[1] * r[2] + r[3] * r[4] + r[5] * r[6]);
  }
}

void mjpl_probe_mul_quat(const float *a, const float *b, float *out, long n, int fused) {
  for (long i = 0; i < n; i++) {
    if (fused) mjpl::pose_mul_quat(out + 4 * i, a + 4 * i, b + 4 * i);
    else plain_mul_quat(out + 4 * i, a + 4 * i, b + 4 * i);
  }
}

// q (x) (cs, axis sn), rows of q[4], axis[3], sc = [sn cs]
void mjpl_probe_hinge(const float *q, const float *axis, const float *sc, float *out, long n, int fused) {
  for (long i = 0; i < n; i++) {
    const float *ax = axis + 3 * i, sn = sc[2 * i], cs = sc[2 * i + 1];
    if (fused) {
      memcpy(out + 4 * i, q + 4 * i, 4 * sizeof(float));
      mjpl::pose_hinge(out + 4 * i, ax, sn, cs);
    } else {
      const float b[4] = {cs, ax[0] * sn, ax[1] * sn, ax[2] * sn};
      plain_mul_quat(out + 4 * i, q + 4 * i, b);
    }
  }
}

void mjpl_probe_normalize(const float *q, float *out, long n, int fused) {
  for (long i = 0; i < n; i++) {
    const float *v = q + 4 * i;
    const float inv = fused ? mjpl::pose_inv_norm(v[0], v[1], v[2], v[3]) : 1.0f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
    for (int k = 0; k < 4; k++) out[4 * i + k] = v[k] * inv;
  }
}

// out: n rows of 9 (the matrix) + 3 (pose_quat2zaxis; the plain build repeats the third column)
void mjpl_probe_quat2mat(const float *q, float *out, long n, int fused) {
  for (long i = 0; i < n; i++) {
    const float *v = q + 4 * i;
    float *o = out + 12 * i;
    if (fused) {
      mjpl::pose_quat2mat(o, v[0], v[1], v[2], v[3]);
      mjpl::pose_quat2zaxis(o + 9, v[0], v[1], v[2], v[3]);
    } else {
      plain_quat2mat(o, v[0], v[1], v[2], v[3]);
      o[9] = o[2]; o[10] = o[5]; o[11] = o[8];
    }
  }
}

void mjpl_probe_rot_vec(const float *v, const float *q, float *out, long n, int fused) {
  for (long i = 0; i < n; i++) {
    if (fused) mjpl::pose_rot_vec(out + 3 * i, v + 3 * i, q + 4 * i);
    else plain_rot_vec(out + 3 * i, v + 3 * i, q + 4 * i);
  }
}

void mjpl_probe_sincos_host(const float *x, float *s, float *c, long n) {
  for (long i = 0; i < n; i++) mjpl::sincos_half_f32(x[i], &s[i], &c[i]);
}

// one launch over n values; returns the HIP status
int mjpl_probe_sincos_device(const float *x, float *s, float *c, long n) {
  float *d = nullptr;
  hipError_t e = hipMalloc(&d, 3 * n * sizeof(float));
  if (e != hipSuccess) return (int)e;
  e = hipMemcpy(d, x, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    k_sincos<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(d, d + n, d + 2 * n, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(s, d + n, n * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(c, d + 2 * n, n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return (int)e;
}

}  // extern "C"

#else  // MJPL_PROBE_MAIN

namespace {

struct Worst {
  double es = 0, ec = 0;
  float xs = 0, xc = 0;
  long count = 0, nan = 0;
  void at(float x) {
    float s, c;
    mjpl::sincos_half_f32(x, &s, &c);
    if (s != s || c != c) nan++;
    const double ds = fabs((double)s - sin((double)x)), dc = fabs((double)c - cos((double)x));
    if (ds > es) { es = ds; xs = x; }
    if (dc > ec) { ec = dc; xc = x; }
    count++;
  }
  void merge(const Worst &o) {
    if (o.es > es) { es = o.es; xs = o.xs; }
    if (o.ec > ec) { ec = o.ec; xc = o.xc; }
    count += o.count; nan += o.nan;
  }
};

uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
float from_bits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

}  // namespace

int main(int argc, char **argv) {
  const uint32_t stride = argc > 1 ? (uint32_t)atol(argv[1]) : 64;
  const int nthreads = argc > 2 ? atoi(argv[2]) : 4;
  const float kRange = 3.3f;
  const uint32_t top = bits(kRange);  // binary32 magnitudes 0 .. top, both signs
  std::vector<Worst> part(nthreads);
  std::vector<std::thread> pool;
  for (int t = 0; t < nthreads; t++)
    pool.emplace_back([&, t] {
      Worst w;
      const uint32_t steps = top / stride + 1, lo = (uint32_t)((uint64_t)steps * t / nthreads), hi = (uint32_t)((uint64_t)steps * (t + 1) / nthreads);
      for (uint32_t k = lo; k < hi; k++) {
        const float x = from_bits(k * stride);
        w.at(x);
        w.at(-x);
      }
      part[t] = w;
    });
  for (auto &th : pool) th.join();
  Worst w;
  for (const Worst &p : part) w.merge(p);
  // the 4 096 binary32 either side of every multiple of pi/4 in range: where the quadrant changes and where the reduced
  // argument is largest
  for (int m = -4; m <= 4; m++) {
    const float centre = (float)(m * 0.78539816339744830962);
    float up = centre, down = centre;
    for (int k = 0; k <= 4096; k++) {
      if (fabsf(up) <= kRange) w.at(up);
      if (fabsf(down) <= kRange) w.at(down);
      up = nextafterf(up, INFINITY);
      down = nextafterf(down, -INFINITY);
    }
  }
  // arguments a lane with `far` set may bring: anything may come back, but the call returns
  const float special[] = {INFINITY, -INFINITY, NAN, 1e30f, -1e30f, 3.4e38f};
  int returned = 0;
  for (float x : special) {
    float s, c;
    mjpl::sincos_half_f32(x, &s, &c);
    returned++;
  }
  printf("{\"stride\": %u, \"count\": %ld, \"nan\": %ld, \"max_err_sin\": %.9e, \"arg_sin\": %.9e, \"max_err_cos\": %.9e, \"arg_cos\": %.9e, "
         "\"special_returned\": %d}\n", stride, w.count, w.nan, w.es, (double)w.xs, w.ec, (double)w.xc, returned);
  return 0;
}
#endif
