"""Clearance gradients, the parts that need no GPU: the C ABI of mjpl_clearance_grad* (declared in
include/mjpl_hip.h, exported by the built library, bound by mjpl_amd.engine), and the NumPy point Jacobian of
tests/gradient_reference.py against central differences of the CPU oracle's forward kinematics."""
import ctypes
import os
import re

import numpy as np
import pytest

import gradient_reference as gref
from mjpl_amd import build as _build
from mjpl_amd import engine, scenes
from test_gpu_models import random_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mjpl_clearance_grad", "mjpl_clearance_grad_dev")


def test_symbols_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "mjpl_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(_build.build_hip())
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in engine.ABI, f"{name} is not bound"
    # status values: the header's and the binding's
    for k, v in (("OK", 0), ("FLAT", 1), ("DEGENERATE", 2), ("NONFINITE", 3)):
        assert re.search(rf"#define MJPL_GRAD_{k}\s+{v}\b", header)
        assert getattr(engine, f"GRAD_{k}") == v


def _fk_points(orc, model, Q, bodies, local):
    """world positions of points given in their bodies' frames, at Q [N, nq]"""
    k = orc.fk(Q)
    n = len(Q)
    xpos, xquat = k["xpos"][np.arange(n), bodies], k["xquat"][np.arange(n), bodies]
    return xpos + gref._qrot(xquat, local)


def _models():
    yield "franka_p", scenes.franka_p(obstacles=True)
    yield "ur5e", scenes.ur5e()
    for seed in (3, 7, 11):  # (bodies with two joints among them)
        yield f"random{seed}", random_model(seed)[0]


@pytest.mark.parametrize("name,model", list(_models()), ids=lambda x: x if isinstance(x, str) else "")
def test_point_jacobian_matches_central_differences(name, model):
    from oracle import pyoracle
    orc = pyoracle.Oracle(model)
    rng = np.random.default_rng(5)
    n = 64
    lo, hi = model.jnt_range[:, 0], model.jnt_range[:, 1]
    lo, hi = np.where(lo < hi, lo, -1.0), np.where(lo < hi, hi, 1.0)
    Q = rng.uniform(lo, hi, size=(n, model.nq))
    bodies = rng.integers(1, model.nbody, size=n)
    local = rng.uniform(-0.2, 0.2, size=(n, 3))
    fk = orc.fk(Q)
    axes, anchors = gref.joint_frames(model, Q, fk)
    x = _fk_points(orc, model, Q, bodies, local)
    J = gref.point_jacobian(model, axes, anchors, bodies, x)
    h = 1e-6
    for j in range(model.nq):
        Qp, Qm = Q.copy(), Q.copy()
        Qp[:, j] += h
        Qm[:, j] -= h
        fd = (_fk_points(orc, model, Qp, bodies, local) - _fk_points(orc, model, Qm, bodies, local)) / (2 * h)
        err = np.abs(fd - J[:, :, j]).max()
        assert err <= 1e-8, f"{name}: column {j}: |J - central difference| = {err:.3e}"


def test_multi_joint_bodies_are_covered():
    """the random models above hold a body with two joints: the frame a later joint leaves matters"""
    assert any(np.any(np.asarray(random_model(s)[0].body_jntnum) > 1) for s in (3, 7, 11))
