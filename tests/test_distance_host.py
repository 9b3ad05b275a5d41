"""Signed geom distances, the parts that need no GPU: the NumPy reference of tests/distance_reference.py against
closed-form cases and against brute-force sampling of both surfaces, and the C ABI of mjpl_distances* /
mjpl_clearance* (declared in include/mjpl_hip.h, exported by the built library, bound by mjpl_amd.engine)."""
import os
import re

import numpy as np
import pytest

import distance_reference as ref
from mjpl_amd import build as _build
from mjpl_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mjpl_distances", "mjpl_distances_dev", "mjpl_clearance", "mjpl_clearance_dev")
I9 = np.eye(3).ravel()


def rot(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).ravel()


def d(t1, p1, m1, s1, t2, p2, m2, s2):
    s1 = np.resize(np.asarray(s1, float), 3)
    s2 = np.resize(np.asarray(s2, float), 3)
    return float(ref.geom_distance(t1, np.asarray(p1, float), np.asarray(m1, float), s1,
                                   t2, np.asarray(p2, float), np.asarray(m2, float), s2))


# ---- 1. closed forms
def test_sphere_sphere():
    assert d(ref.SPHERE, [0, 0, 0], I9, [0.1, 0, 0], ref.SPHERE, [0.5, 0, 0], I9, [0.2, 0, 0]) == pytest.approx(0.2, abs=1e-15)
    assert d(ref.SPHERE, [0, 0, 0], I9, [0.1, 0, 0], ref.SPHERE, [0, 0.25, 0], I9, [0.2, 0, 0]) == pytest.approx(-0.05, abs=1e-15)


def test_sphere_above_plane():
    assert d(ref.PLANE, [0, 0, 0.1], I9, [0, 0, 0], ref.SPHERE, [3, -2, 0.4], I9, [0.1, 0, 0]) == pytest.approx(0.2, abs=1e-15)
    # the geom order does not matter, and a sphere below the surface has a negative height
    assert d(ref.SPHERE, [3, -2, 0.05], I9, [0.1, 0, 0], ref.PLANE, [0, 0, 0.1], I9, [0, 0, 0]) == pytest.approx(-0.15, abs=1e-15)


def test_box_resting_on_plane_corner_height():
    th = 0.3
    s = [0.1, 0.2, 0.3]
    z = 0.5
    want = z - s[1] * abs(np.sin(th)) - s[2] * abs(np.cos(th))
    assert d(ref.PLANE, [0, 0, 0], I9, [0, 0, 0], ref.BOX, [0.7, 0.1, z], rot([1, 0, 0], th), s) == pytest.approx(want, abs=1e-15)


def test_boxes_face_to_face_and_edge_to_edge():
    gap = 0.037
    assert d(ref.BOX, [0, 0, 0], I9, [0.1, 0.2, 0.3], ref.BOX, [0.1 + 0.15 + gap, 0.05, -0.02], I9,
             [0.15, 0.1, 0.1]) == pytest.approx(gap, abs=1e-15)
    # crossed at 90 degrees: b1's top edge runs along x, b2's bottom edge along y
    z0 = 0.5
    want = z0 - 2 * 0.1 * np.sqrt(2)
    got = d(ref.BOX, [0, 0, 0], rot([1, 0, 0], np.pi / 4), [0.5, 0.1, 0.1],
            ref.BOX, [0, 0, z0], rot([0, 1, 0], np.pi / 4), [0.1, 0.5, 0.1])
    assert got == pytest.approx(want, abs=1e-14)


def test_overlapping_boxes_depth():
    assert d(ref.BOX, [0, 0, 0], I9, [0.2, 0.2, 0.2], ref.BOX, [0.35, 0.01, -0.02], I9, [0.2, 0.2, 0.2]) == \
        pytest.approx(-0.05, abs=1e-15)


def test_sphere_centre_inside_box():
    assert d(ref.SPHERE, [0.1, 0, 0.02], I9, [0.05, 0, 0], ref.BOX, [0, 0, 0], I9, [0.3, 0.2, 0.1]) == \
        pytest.approx(-0.13, abs=1e-15)


def test_capsules_parallel_and_crossing():
    # both along z (identity), side by side: 0.3 apart, shifted along the axis
    assert d(ref.CAPSULE, [0, 0, 0], I9, [0.05, 0.2, 0], ref.CAPSULE, [0, 0.3, 0.1], I9, [0.05, 0.2, 0]) == \
        pytest.approx(0.2, abs=1e-15)
    # end to end along the common axis
    assert d(ref.CAPSULE, [0, 0, 0], I9, [0.05, 0.2, 0], ref.CAPSULE, [0, 0, 0.7], I9, [0.05, 0.2, 0]) == \
        pytest.approx(0.2, abs=1e-15)
    # crossing: one along x, one along y, 0.25 apart in z
    assert d(ref.CAPSULE, [0, 0, 0], rot([0, 1, 0], np.pi / 2), [0.05, 0.3, 0],
             ref.CAPSULE, [0.1, -0.05, 0.25], rot([1, 0, 0], np.pi / 2), [0.05, 0.3, 0]) == pytest.approx(0.15, abs=1e-15)
    # crossing and overlapping: depth = r1 + r2 - core distance
    assert d(ref.CAPSULE, [0, 0, 0], rot([0, 1, 0], np.pi / 2), [0.1, 0.3, 0],
             ref.CAPSULE, [0.1, -0.05, 0.15], rot([1, 0, 0], np.pi / 2), [0.1, 0.3, 0]) == pytest.approx(-0.05, abs=1e-15)


def test_capsule_through_a_box():
    # a capsule whose segment crosses the box: depth is the least projected overlap plus the radius
    got = d(ref.CAPSULE, [0, 0.15, 0], rot([0, 1, 0], np.pi / 2), [0.02, 1.0, 0], ref.BOX, [0, 0, 0], I9, [0.3, 0.2, 0.1])
    assert got == pytest.approx(-(0.05 + 0.02), abs=1e-15)


# ---- 2. brute force: sampled surfaces of random disjoint pairs
def _fib_sphere(n):
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], axis=1)


def _surface(t, pos, mat, size, h):
    """points of the geom's surface no farther than ~h from any surface point (world frame)"""
    R = mat.reshape(3, 3)
    if t == ref.SPHERE:
        n = int(4 * np.pi * size[0] ** 2 / h ** 2 * 2) + 64
        loc = _fib_sphere(n) * size[0]
    elif t == ref.CAPSULE:
        r, L = size[0], size[1]
        n = int(4 * np.pi * r * r / h ** 2 * 2) + 64
        s = _fib_sphere(n) * r
        top, bot = s[s[:, 2] >= 0] + [0, 0, L], s[s[:, 2] < 0] - [0, 0, L]
        nz, na = int(2 * L / h) + 2, int(2 * np.pi * r / h) + 8
        z, a = np.meshgrid(np.linspace(-L, L, nz), np.linspace(0, 2 * np.pi, na, endpoint=False))
        side = np.stack([r * np.cos(a).ravel(), r * np.sin(a).ravel(), z.ravel()], axis=1)
        loc = np.concatenate([top, bot, side])
    else:
        faces = []
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            u, v = np.meshgrid(np.linspace(-size[i], size[i], int(2 * size[i] / h) + 2),
                               np.linspace(-size[j], size[j], int(2 * size[j] / h) + 2))
            for sgn in (-1, 1):
                f = np.zeros((u.size, 3))
                f[:, i], f[:, j], f[:, k] = u.ravel(), v.ravel(), sgn * size[k]
                faces.append(f)
        loc = np.concatenate(faces)
    return pos + loc @ R.T


def _random_geom(rng, t):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    mat = np.array([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                    2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                    2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)])
    size = np.array([rng.uniform(0.03, 0.1), rng.uniform(0.03, 0.12), rng.uniform(0.03, 0.1)])
    if t == ref.SPHERE:
        size[1:] = 0
    if t == ref.CAPSULE:
        size[2] = 0
    return rng.uniform(-0.15, 0.15, 3), mat, size


@pytest.mark.parametrize("types", [(ref.SPHERE, ref.SPHERE), (ref.SPHERE, ref.CAPSULE), (ref.CAPSULE, ref.CAPSULE),
                                   (ref.SPHERE, ref.BOX), (ref.CAPSULE, ref.BOX), (ref.BOX, ref.BOX)],
                         ids=lambda t: str(t))
def test_reference_against_sampled_surfaces(types):
    rng = np.random.default_rng(7 + 10 * types[0] + types[1])
    h = 0.004
    checked = 0
    for _ in range(40):
        p1, m1, s1 = _random_geom(rng, types[0])
        p2, m2, s2 = _random_geom(rng, types[1])
        want = float(ref.geom_distance(types[0], p1, m1, s1, types[1], p2, m2, s2))
        if want <= 0.005:  # disjoint pairs only (the sampled minimum says nothing of a depth)
            continue
        A, B = _surface(types[0], p1, m1, s1, h), _surface(types[1], p2, m2, s2, h)
        got = np.inf
        for k in range(0, len(A), 2048):
            diff = A[k:k + 2048, None, :] - B[None, :, :]
            got = min(got, float(np.sqrt(np.min(np.einsum("ijk,ijk->ij", diff, diff)))))
        # the true minimum is no larger than any sampled pair, and the samples come within ~h of it on each side
        assert got >= want - 1e-12, (types, got, want)
        assert got <= want + 2 * h, (types, got, want)
        checked += 1
        if checked == 8:
            break
    assert checked >= 4


# ---- 3. the C ABI
def test_distance_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpl_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, text), f"{name} is not declared in include/mjpl_hip.h"
        assert name in engine.ABI
    _build.build_hip()
    lib = engine.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by libmjpl_hip.so"
    from mjpl_amd.constraint import CollisionConstraint
    for name in ("pair_distances", "distances_batch", "clearance", "clearance_batch"):
        assert callable(getattr(CollisionConstraint, name))
    for name in ("distances", "distances_dev", "clearance", "clearance_dev"):
        assert callable(getattr(engine.Engine, name))
