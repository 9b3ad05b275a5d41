// mjpl_pose_f32.h -- the binary32 pose arithmetic of the generated checks, fused, and the bounded-range sincos of a
// hinge's half angle.  Included by a generated translation unit whose text calls these (specialise.Options.pose_fma /
// .sincos, which specialise.build() turns on).  NOT a stamped header, like mjpl_overlay.h and for the same reason: it
// holds no layout, table or kernel shared with libmjpl_hip.so, so stamp and program hashes stay what they are, and a
// library generated without it is slower, not wrong (tests/test_gpu_pose_fma.py compares the two).
#pragma once

#include "../../include/mjpl_hip.h"  // (mjpl_device.h reads the layout constants; mjpl_filter.h includes the two in this order)
#include "mjpl_device.h"

namespace mjpl {

// The pose statements of the generated checks (specialise.py emits calls to these; where a literal coefficient is an
// exact 0 or +-1 the emitter spells the same chain itself with that term folded).  Every multiply-add is a
// __builtin_fmaf in one fixed association order -- the order of the unfused statement, left to right -- so the value
// of those chains does not depend on what a compiler contracts and a host build returns the device's bits for them
// (not for pose_inv_norm: rdiv / rsqrt_val are v_rcp_f32 / v_sqrt_f32 on the device and 1 / sqrt on the host).  Each fused operation
// drops one rounding from a sum DESIGN.md 5.1b bounds operation by operation: the bound holds as it stands.

// base + c0 x0 + c1 x1 + c2 x2: a body's origin or a geom's centre (base = the parent's coordinate, c = the literal
// local position, x = a row of the rotation matrix).  The products are summed first and the world coordinate is added
// once: a chain of three multiply-adds onto `base` would round three times at the magnitude of a world coordinate,
// where 5.1b counts one such rounding per body (eps C).  (With a single term left after folding, the emitter's
// fma(c, x, base) is that one rounding.)
MJPL_HD float pose_lin3(float base, float c0, float x0, float c1, float x1, float c2, float x2) {
  return base + __builtin_fmaf(c2, x2, __builtin_fmaf(c1, x1, c0 * x0));
}

// res = a (x) b (mju_mulQuat); the generated text calls it with b a literal quaternion
MJPL_HD void pose_mul_quat(float *res, const float *a, const float *b) {
  const float t0 = __builtin_fmaf(-a[3], b[3], __builtin_fmaf(-a[2], b[2], __builtin_fmaf(-a[1], b[1], a[0] * b[0])));
  const float t1 = __builtin_fmaf(-a[3], b[2], __builtin_fmaf(a[2], b[3], __builtin_fmaf(a[1], b[0], a[0] * b[1])));
  const float t2 = __builtin_fmaf(a[3], b[1], __builtin_fmaf(a[2], b[0], __builtin_fmaf(-a[1], b[3], a[0] * b[2])));
  const float t3 = __builtin_fmaf(a[3], b[0], __builtin_fmaf(-a[2], b[1], __builtin_fmaf(a[1], b[2], a[0] * b[3])));
  res[0] = t0; res[1] = t1; res[2] = t2; res[3] = t3;
}

// q = q (x) (cs, axis sn): a hinge about a literal axis; the products axis[k] * sn are rounded once each, as in the
// unfused statement
MJPL_HD void pose_hinge(float *q, const float *axis, float sn, float cs) {
  const float s0 = axis[0] * sn, s1 = axis[1] * sn, s2 = axis[2] * sn;
  const float t0 = __builtin_fmaf(-q[3], s2, __builtin_fmaf(-q[2], s1, __builtin_fmaf(-q[1], s0, q[0] * cs)));
  const float t1 = __builtin_fmaf(-q[3], s1, __builtin_fmaf(q[2], s2, __builtin_fmaf(q[1], cs, q[0] * s0)));
  const float t2 = __builtin_fmaf(q[3], s0, __builtin_fmaf(q[2], cs, __builtin_fmaf(-q[1], s2, q[0] * s1)));
  const float t3 = __builtin_fmaf(q[3], cs, __builtin_fmaf(-q[2], s0, __builtin_fmaf(q[1], s1, q[0] * s2)));
  q[0] = t0; q[1] = t1; q[2] = t2; q[3] = t3;
}

// 1 / |q|: the normalisation's factor (the filter always rescales, see normalize4)
MJPL_HD float pose_inv_norm(float q0, float q1, float q2, float q3) {
  return rdiv(1.0f, rsqrt_val(__builtin_fmaf(q3, q3, __builtin_fmaf(q2, q2, __builtin_fmaf(q1, q1, q0 * q0)))));
}

// mju_quat2Mat.  The doublings are exact, so an off-diagonal element is 2 (q_i q_j -+ fl(q_0 q_k)) rounded once.
MJPL_HD void pose_quat2mat(float *R, float q0, float q1, float q2, float q3) {
  const float q00 = q0 * q0, sum01 = __builtin_fmaf(q1, q1, q00), dif01 = __builtin_fmaf(-q1, q1, q00);
  R[0] = __builtin_fmaf(-q3, q3, __builtin_fmaf(-q2, q2, sum01));
  R[4] = __builtin_fmaf(-q3, q3, __builtin_fmaf(q2, q2, dif01));
  R[8] = __builtin_fmaf(q3, q3, __builtin_fmaf(-q2, q2, dif01));
  const float d0 = q0 + q0, d1 = q1 + q1, d2 = q2 + q2;
  const float m03 = d0 * q3, m02 = d0 * q2, m01 = d0 * q1;
  R[1] = __builtin_fmaf(d1, q2, -m03);
  R[3] = __builtin_fmaf(d1, q2, m03);
  R[2] = __builtin_fmaf(d1, q3, m02);
  R[6] = __builtin_fmaf(d1, q3, -m02);
  R[5] = __builtin_fmaf(d2, q3, -m01);
  R[7] = __builtin_fmaf(d2, q3, m01);
}

// third column of pose_quat2mat only (a capsule's axis): R[2], R[5], R[8]
MJPL_HD void pose_quat2zaxis(float *z, float q0, float q1, float q2, float q3) {
  const float d0 = q0 + q0;
  z[0] = __builtin_fmaf(q1 + q1, q3, d0 * q2);
  z[1] = __builtin_fmaf(q2 + q2, q3, -(d0 * q1));
  z[2] = __builtin_fmaf(q3, q3, __builtin_fmaf(-q2, q2, __builtin_fmaf(-q1, q1, q0 * q0)));
}

// mju_rotVecQuat for a literal vector: v + 2 cross(q_xyz, q_w v + cross(q_xyz, v))
MJPL_HD void pose_rot_vec(float *res, const float *v, const float *q) {
  const float t0 = __builtin_fmaf(-v[1], q[3], __builtin_fmaf(v[2], q[2], v[0] * q[0]));
  const float t1 = __builtin_fmaf(-v[2], q[1], __builtin_fmaf(v[0], q[3], v[1] * q[0]));
  const float t2 = __builtin_fmaf(-v[0], q[2], __builtin_fmaf(v[1], q[1], v[2] * q[0]));
  res[0] = __builtin_fmaf(2.0f, __builtin_fmaf(q[2], t2, -(q[3] * t1)), v[0]);
  res[1] = __builtin_fmaf(2.0f, __builtin_fmaf(q[3], t0, -(q[1] * t2)), v[1]);
  res[2] = __builtin_fmaf(2.0f, __builtin_fmaf(q[1], t1, -(q[2] * t0)), v[2]);
}

// sin and cos of a hinge's half angle, |x| <= kFilterMaxAngle / 2 = 3.25 (a lane beyond that has `far` set and its verdict
// is V_UNSURE whatever this returns; the routine has no loop, no branch and no integer conversion that could trap, so
// infinities, NaN and huge arguments run through it like any other).  k = the nearest multiple of pi/2 by the
// add-and-subtract of 1.5 * 2^23 (its low bits are the quadrant), a two-constant Cody-Waite reduction -- k in -2 .. 2
// and the high constant is binary32(pi/2), so the first step is exact and the second rounds once -- then the single
// precision kernels of Cephes' sinf / cosf on [-pi/4, pi/4] with fused multiply-adds, and the quadrant by integer
// operations on the sign bits.  Measured over every binary32 of [-3.3, 3.3] against binary64 sin / cos: profiles/README.md.
MJPL_HD void sincos_half_f32(float x, float *s, float *c) {
  const float kMagic = 12582912.0f;  // 1.5 * 2^23
  const float kf = __builtin_fmaf(x, 0x1.45f306p-1f, kMagic);
  const unsigned quad = __builtin_bit_cast(unsigned, kf);
  const float k = kf - kMagic;
  float r = __builtin_fmaf(k, -0x1.921fb6p+0f, x);
  r = __builtin_fmaf(k, 0x1.777a5cp-25f, r);  // binary32(pi/2) - pi/2 = 4.371139e-8
  const float z = r * r;
  float ps = __builtin_fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
  ps = __builtin_fmaf(z, ps, -1.6666654611e-1f);
  const float sr = __builtin_fmaf(z * r, ps, r);
  float pc = __builtin_fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
  pc = __builtin_fmaf(z, pc, 4.166664568298827e-2f);
  const float cr = __builtin_fmaf(z * z, pc, __builtin_fmaf(z, -0.5f, 1.0f));
  const bool swap = (quad & 1u) != 0;
  const unsigned us = __builtin_bit_cast(unsigned, swap ? cr : sr) ^ ((quad & 2u) << 30);
  const unsigned uc = __builtin_bit_cast(unsigned, swap ? sr : cr) ^ (((quad + 1u) & 2u) << 30);
  *s = __builtin_bit_cast(float, us);
  *c = __builtin_bit_cast(float, uc);
}

}  // namespace mjpl
