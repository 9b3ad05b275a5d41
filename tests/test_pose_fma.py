"""The binary32 pose helpers of mjpl_amd/csrc/mjpl_pose_f32.h the generated checks call (pose_lin3, pose_mul_quat, pose_hinge,
pose_inv_norm, pose_quat2mat / pose_quat2zaxis, pose_rot_vec, sincos_half_f32) on the host: no GPU.  build() compiles
mjpl_pose_probe.hip into a library (the helpers over arrays, beside the unfused statements the generated text held before
them) and a stand-alone sweep program.

Tolerances are those of DESIGN.md / profiles/NOTEBOOK.md 5.1b, eps = 2^-24, against the same expression evaluated in
binary64 on the same binary32 inputs:
  sincos of the half angle   4 eps absolute, both results
  a quaternion product       8 eps in the 2-norm (a hinge: against the product with the binary32 quaternion (cs, axis sn) it forms)
  the normalisation          3 eps in the 2-norm
  a rotated vector           8 eps |v| in the 2-norm (no input error here: the reference takes the same binary32 quaternion)
  a body origin / geom centre  3 eps |c| for the product R c (5.1b: 3 eps L_b) + eps C for the addition of world coordinates,
                             C = the larger of |base| and |result|
  an element of the rotation matrix  4 eps: an off-diagonal element is 2 (ab -+ cd) with |ab|, |cd|, |ab -+ cd| <= 1/2 -- three
                             roundings of at most eps / 2, doubled; a diagonal element is four squares that sum to 1 (eps in all)
                             and three additions of partial sums within [-1, 1] (eps each)
pose_inv_norm is v_sqrt_f32 / v_rcp_f32 on the device and 1 / sqrt here: the normalisation's test holds the host's
statement, whose two roundings are each within the device instructions' 1 ulp; the device's is covered by the GPU tests.
The UNFUSED statements are held to the same numbers on the same inputs: the bound is the one 5.1b derives for them, and a
fused multiply-add only drops roundings from it."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from mjpl_amd import build as _build

EPS = 2.0 ** -24
N = 100_000
F = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(_build.POSE_PROBE_LIB), f"{_build.POSE_PROBE_LIB}: run __graft_entry__.build()"
    return C.CDLL(_build.POSE_PROBE_LIB)


def _call(fn, arrays, out_shape, fused):
    arrays = [np.ascontiguousarray(a, np.float32) for a in arrays]
    out = np.zeros(out_shape, np.float32)
    fn.restype = None
    fn(*[a.ctypes.data_as(F) for a in arrays], out.ctypes.data_as(F), C.c_long(out_shape[0]), C.c_int(fused))
    return out.astype(np.float64)


def _unit(rng, n, k):
    v = rng.normal(size=(n, k))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _coefs(rng, shape, scale):
    """uniform in +-scale with exact 0, 1 and -1 mixed in (the coefficients the emitter folds)"""
    c = rng.uniform(-scale, scale, size=shape)
    pick = rng.integers(0, 10, size=shape)
    c[pick == 0], c[pick == 1], c[pick == 2] = 0.0, 1.0, -1.0
    return c.astype(np.float32)


def _mul_quat64(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2] - a[:, 3] * b[:, 3],
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0] + a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2],
                     a[:, 0] * b[:, 2] - a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0] + a[:, 3] * b[:, 1],
                     a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1] + a[:, 3] * b[:, 0]], axis=1)


def _both(fn, arrays, out_shape, want, tol, norm2, what):
    """The helper and the unfused statement within `tol` of `want` (per row in the 2-norm, or per element); the two differ
    somewhere (the comparison is not of a statement with itself)."""
    got = {}
    for fused in (1, 0):
        got[fused] = _call(fn, arrays, out_shape, fused)
        err = got[fused] - want
        err = np.linalg.norm(err.reshape(len(err), -1), axis=1) if norm2 else np.abs(err)
        worst = float(np.max(err / tol))
        print(f"{what}, {'fused' if fused else 'unfused'}: worst error / tolerance = {worst:.3f}")
        assert np.isfinite(got[fused]).all() and worst <= 1.0, (what, fused, worst)
    assert (got[1] != got[0]).any(), what
    return got[1]


def test_sincos_half_sweep():
    """Every 64th binary32 of [-3.3, 3.3] and the 4 096 either side of every multiple of pi/4, against binary64 sin / cos."""
    assert os.path.exists(_build.POSE_PROBE_EXE), f"{_build.POSE_PROBE_EXE}: run __graft_entry__.build()"
    out = subprocess.run([_build.POSE_PROBE_EXE, "64", "4"], check=True, capture_output=True, text=True, timeout=120).stdout
    r = json.loads(out)
    print(r)
    assert r["count"] > 33_000_000 and r["nan"] == 0
    assert r["max_err_sin"] <= 4 * EPS and r["max_err_cos"] <= 4 * EPS, r
    assert r["special_returned"] == 6  # +-inf, NaN, +-1e30, 3.4e38: the call came back


def test_sincos_half_quadrants_and_zero(probe):
    x = np.array([0.0, -0.0, np.pi / 4, -np.pi / 4, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 3.25, -3.25, 1e-30, 3 * np.pi / 4], np.float32)
    s, c = np.zeros_like(x), np.zeros_like(x)
    probe.mjpl_probe_sincos_host(x.ctypes.data_as(F), s.ctypes.data_as(F), c.ctypes.data_as(F), C.c_long(len(x)))
    assert np.abs(s - np.sin(x.astype(np.float64))).max() <= 4 * EPS and np.abs(c - np.cos(x.astype(np.float64))).max() <= 4 * EPS
    assert s[0] == 0.0 and c[0] == 1.0 and s[10] == x[10]


def test_lin3(probe):
    rng = np.random.default_rng(11)
    base = rng.uniform(-6, 6, size=(N, 1)).astype(np.float32)
    c = _coefs(rng, (N, 3), 2.0)
    x = _unit(rng, N, 3)  # a row of a rotation matrix
    rows = np.concatenate([base, np.stack([c[:, 0], x[:, 0], c[:, 1], x[:, 1], c[:, 2], x[:, 2]], axis=1)], axis=1)
    want = base[:, 0].astype(np.float64) + (c.astype(np.float64) * x.astype(np.float64)).sum(axis=1)
    tol = 3 * EPS * np.linalg.norm(c.astype(np.float64), axis=1) + EPS * np.maximum(np.abs(base[:, 0]), np.abs(want))
    _both(probe.mjpl_probe_lin3, [rows], (N,), want, tol, False, "lin3")


def test_mul_quat(probe):
    rng = np.random.default_rng(12)
    a, b = _unit(rng, N, 4), _unit(rng, N, 4)
    b[::7] = np.array([np.sqrt(0.5), -np.sqrt(0.5), 0, 0], np.float32)  # (the kind of literal a model holds)
    b[1::7] = np.array([1, 0, 0, 0], np.float32)
    _both(probe.mjpl_probe_mul_quat, [a, b], (N, 4), _mul_quat64(a, b), 8 * EPS, True, "mul_quat")


def test_hinge(probe):
    rng = np.random.default_rng(13)
    q, axis = _unit(rng, N, 4), _unit(rng, N, 3)
    axis[::3] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, size=len(axis[::3]))] * rng.choice([-1.0, 1.0], size=(len(axis[::3]), 1)).astype(np.float32)
    half = rng.uniform(-3.25, 3.25, size=N)
    sc = np.stack([np.sin(half), np.cos(half)], axis=1).astype(np.float32)
    # the reference takes the quaternion (cs, binary32(axis sn)) both statements form before the product: its rounding is
    # an input's, not the product's
    b = np.concatenate([sc[:, 1:2], axis * sc[:, 0:1]], axis=1)
    assert b.dtype == np.float32
    _both(probe.mjpl_probe_hinge, [q, axis, sc], (N, 4), _mul_quat64(q, b), 8 * EPS, True, "hinge")


def test_normalize(probe):
    rng = np.random.default_rng(14)
    q = (_unit(rng, N, 4).astype(np.float64) * (1.0 + rng.uniform(-1e-5, 1e-5, size=(N, 1)))).astype(np.float32)
    want = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    got = _both(probe.mjpl_probe_normalize, [q], (N, 4), want, 3 * EPS, True, "normalize")
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 3 * EPS


def test_quat2mat(probe):
    rng = np.random.default_rng(15)
    q = _unit(rng, N, 4)
    q0, q1, q2, q3 = (q[:, k].astype(np.float64) for k in range(4))
    R = np.stack([q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2),
                  2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1),
                  2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3], axis=1)
    want = np.concatenate([R, R[:, [2, 5, 8]]], axis=1)
    got = _both(probe.mjpl_probe_quat2mat, [q], (N, 12), want, 4 * EPS, False, "quat2mat")
    assert np.array_equal(got[:, 9:], got[:, [2, 5, 8]])  # pose_quat2zaxis IS the third column, bit for bit


def test_rot_vec(probe):
    rng = np.random.default_rng(16)
    v, q = _coefs(rng, (N, 3), 6.0), _unit(rng, N, 4)
    v64, w, u = v.astype(np.float64), q[:, 0:1].astype(np.float64), q[:, 1:].astype(np.float64)
    want = v64 + 2 * np.cross(u, w * v64 + np.cross(u, v64))
    tol = 8 * EPS * np.maximum(np.linalg.norm(v64, axis=1), 1e-30)
    _both(probe.mjpl_probe_rot_vec, [v, q], (N, 3), want, tol, True, "rot_vec")
