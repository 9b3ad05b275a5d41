"""The chains the EMITTER spells itself where a literal coefficient folds (an exact 0 or +-1): specialise.flin, _lin3, the
fused constant quaternion product, the folded hinge rows of _emit_body_fk and the folded _Gen.rot_vec_quat -- what the
benchmark model's text consists of (every hinge axis of the Franka is a coordinate axis).  The emitted C expressions are
evaluated here in binary32, operation by operation (numpy's float32 arithmetic; __builtin_fmaf exactly, through
fractions), and must equal the value of the header's general helper (mjpl_pose_f32.h, through the probe library) called
with the same coefficients: a folded term is one the helper multiplies by 0 or 1, which changes no value (`==`: the sign
of an exact zero may differ).  One exception, by design: a body origin with a single surviving term is one
fma(c, x, base) -- one rounding where pose_lin3 has two -- and is held to 5.1b's allowance against binary64 instead.
Host only: no GPU, no compiler (build() made the probe library)."""
import ctypes as C
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

from mjpl_amd import build as _build
from mjpl_amd import specialise as sp
from mjpl_amd.program import JT_HINGE, PARENT_STATIC

F32 = np.float32
EPS = 2.0 ** -24
FP = C.POINTER(C.c_float)
FUSED = sp.Options(pose_fma=True)
ROWS = 400


def fma32(a, b, c):
    """binary32 fused multiply-add, correctly rounded: the exact value, then the nearest of the float32 around it."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    near = F32(float(exact))
    cands = {near, np.nextafter(near, F32(np.inf)), np.nextafter(near, F32(-np.inf))}
    best = min(cands, key=lambda f: (abs(Fraction(float(f)) - exact), int(np.float32(f).view(np.uint32)) & 1))
    return F32(best)


def evaluate(expr, env):
    """A C float expression of the generator's making (hex literals, decimal literals with f, __builtin_fmaf) in binary32."""
    py = re.sub(r"0x[0-9a-f]\.[0-9a-f]+p[+-]?\d+f", lambda m: f'F32(float.fromhex("{m.group(0)[:-1]}"))', expr)
    py = re.sub(r"(?<![\w.\"])(\d+\.\d+)f", r"F32(\1)", py)
    return F32(eval(py, {"F32": F32, "__builtin_fmaf": fma32}, dict(env)))


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(_build.POSE_PROBE_LIB), f"{_build.POSE_PROBE_LIB}: run __graft_entry__.build()"
    return C.CDLL(_build.POSE_PROBE_LIB)


def helper(fn, arrays, out_len):
    arrays = [np.ascontiguousarray(a, F32).reshape(-1) for a in arrays]
    out = np.zeros(out_len, F32)
    fn.restype = None
    fn(*[a.ctypes.data_as(FP) for a in arrays], out.ctypes.data_as(FP), C.c_long(1), C.c_int(1))
    return out


def folded(rng, n, scale):
    """n coefficients uniform in +-scale, each with probability 1/2 an exact 0, 1 or -1 instead"""
    c = rng.uniform(-scale, scale, size=n).astype(F32)
    for k in range(n):
        if rng.random() < 0.5:
            c[k] = rng.choice([0.0, 1.0, -1.0])
    return c


def unit(rng, k):
    v = rng.normal(size=k)
    return (v / np.linalg.norm(v)).astype(F32)


def test_the_evaluator_itself():
    assert evaluate("__builtin_fmaf(0x1.8000000000000p+0f, x, (2.0f * y))", {"x": F32(3), "y": F32(0.25)}) == F32(5)
    a, b = F32(1 + 2.0 ** -23), F32(1 - 2.0 ** -23)   # a b = 1 - 2^-46: fma keeps what a * b rounds away
    assert fma32(a, b, F32(-1)) == F32(-2.0 ** -46) and a * b - F32(1) == F32(0)
    assert sp.flin([(0.0, "x"), (1.0, "y")]) == "y" and sp.flin([(0.0, "x")]) == "0.0f" and sp.flin([(-1.0, "x")], "b") == "(b - x)"


def test_body_origin_rows(probe):
    rng = np.random.default_rng(21)
    g = sp._Gen(FUSED)
    seen = set()
    for _ in range(ROWS):
        c, x, base = folded(rng, 3, 2.0), unit(rng, 3), F32(rng.uniform(-6, 6))
        r = int(rng.integers(0, 3))
        env = {f"R{3 * r + k}": x[k] for k in range(3)} | {"p": base}
        text = sp._lin3(g, "p", c, r)
        if text.startswith("mjpl::pose_lin3("):  # (nothing folds: the helper's own call, tests/test_pose_fma.py)
            assert sp._general(c)
            continue
        assert not sp._general(c)
        got = evaluate(text, env)
        left = int(np.count_nonzero(c))
        seen.add(left)
        if left >= 2:
            want = helper(probe.mjpl_probe_lin3, [np.array([base, c[0], x[0], c[1], x[1], c[2], x[2]])], 1)[0]
            assert got == want, (c, x, base)
        else:  # one multiply-add onto the world coordinate (or the coordinate itself): 5.1b's allowance against binary64
            exact = float(base) + float(np.dot(c.astype(np.float64), x.astype(np.float64)))
            assert abs(float(got) - exact) <= 3 * EPS * float(np.linalg.norm(c)) + EPS * max(abs(float(base)), abs(exact)), (c, x, base)
    assert seen == {0, 1, 2, 3}


def test_constant_quaternion_product(probe):
    rng = np.random.default_rng(22)
    names = ["q0", "q1", "q2", "q3"]
    for _ in range(ROWS):
        a, b = unit(rng, 4), folded(rng, 4, 1.0)
        got = [evaluate(e, dict(zip(names, a))) for e in sp.quat_mul_const_right_fused(names, b)]
        want = helper(probe.mjpl_probe_mul_quat, [a, b], 4)
        assert all(x == y for x, y in zip(got, want)), (a, b)


def _hinge_text(axis):
    """The hinge statement _emit_body_fk writes for a body welded to the world with one hinge about `axis`."""
    dp = np.zeros(64)
    dp[3], dp[10], dp[14], dp[18], dp[22] = 1, 1, 1, 1, 1  # body and parent quaternions, the parent's matrix: identities
    dp[32:35] = axis
    body = types.SimpleNamespace(doff=0, parent=PARENT_STATIC, joints=[(JT_HINGE, 0, 0, 32)], save=-1)
    g = sp._Gen(FUSED)
    sp._emit_body_fk(g, body, dp)
    line = next(ln for ln in g.lines if "const float t0 = " in ln)
    return re.findall(r"t\d = (.*?)(?:, (?=t\d = )|;)", line)


def test_folded_hinge_rows(probe):
    rng = np.random.default_rng(23)
    axes = [np.eye(3, dtype=F32)[k] * s for k in range(3) for s in (F32(1), F32(-1))]
    axes += [np.array(v, F32) for v in ((0, 0.6, 0.8), (0.6, 0, -0.8), (-0.8, 0.6, 0), (1, 0, 0.5), (0, -1, 0.25))]
    for axis in axes:
        exprs = _hinge_text(axis)
        assert len(exprs) == 4 and "mjpl::pose_hinge" not in "".join(exprs), axis
        for _ in range(40):
            q, half = unit(rng, 4), rng.uniform(-3.25, 3.25)
            sn, cs = F32(np.sin(half)), F32(np.cos(half))
            env = {"nq0": q[0], "nq1": q[1], "nq2": q[2], "nq3": q[3], "sn": sn, "cs": cs}
            got = [evaluate(e, env) for e in exprs]
            want = helper(probe.mjpl_probe_hinge, [q, axis, np.array([sn, cs])], 4)
            assert all(x == y for x, y in zip(got, want)), (axis, q, half)


def test_folded_rot_vec_quat(probe):
    rng = np.random.default_rng(24)
    qn = ["nq0", "nq1", "nq2", "nq3"]
    done = 0
    while done < 200:
        v = folded(rng, 3, 6.0)
        if sp._general(v):
            continue
        done += 1
        g = sp._Gen(FUSED)
        g.rot_vec_quat("xa", v, qn)
        text = " ".join(g.lines)
        assert "mjpl::pose_rot_vec" not in text
        q = unit(rng, 4)
        env = dict(zip(qn, q))
        for name, expr in re.findall(r"(?:const float )?(\w+) = (.*?);", text):
            env[name] = evaluate(expr, env)
        want = helper(probe.mjpl_probe_rot_vec, [v, q], 3)
        assert all(env[f"xa{k}"] == want[k] for k in range(3)), (v, q)
