"""Clearance gradients and witness points on the GPU (include/mjpl_hip.h: mjpl_clearance_grad*;
CollisionConstraint.clearance_gradient*): the clearance is mjpl_clearance's byte for byte, closed forms on small
hand-built models, witness points on the geoms' surfaces, the Jacobian identity against the NumPy reference of
tests/gradient_reference.py, central differences of mjpl_clearance, and the entry points' forms and statuses."""
import numpy as np
import pytest

import distance_reference as ref
import gradient_reference as gref
from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes
from mjpl_amd.constraint import CollisionConstraint
from mjpl_amd.model import ModelBuilder
from helpers import uniform_configs
from test_gpu_models import random_model

pytestmark = pytest.mark.gpu

E_ARG = -1  # MJPL_E_ARG
INF = float("inf")
ALLOWED = (("link5", "hand"), ("link0", "link6"), ("world", "left_finger"))
R2 = np.sqrt(2)


def quat(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def g(type, size, pos=(0, 0, 0), q=(1, 0, 0, 0)):
    return dict(type=type, size=size, pos=pos, quat=q)


def one_pair(static, moving, jtype="slide", axis=(1, 0, 0), body_pos=(0, 0, 0)):
    mb = ModelBuilder()
    mb.add_body("m", pos=body_pos)
    mb.add_joint("m", "j", type=jtype, axis=axis, range=(-2, 2))
    mb.add_geom("world", **static)
    mb.add_geom("m", **moving)
    return mb.compile()


def grad_of(m, Q, distmax=INF):
    e = eng_mod.Engine(m)
    return e, e.clearance_grad(np.atleast_2d(np.asarray(Q, float)), distmax)


# ---- 1. the same clearance as mjpl_clearance
@pytest.fixture(scope="module")
def franka():
    m = scenes.franka_p(obstacles=True)
    return m, uniform_configs(m, 65536, seed=31)


@pytest.mark.parametrize("distmax", [INF, 0.05], ids=["inf", "0.05"])
@pytest.mark.parametrize("allowed", [(), ALLOWED], ids=["no allowed pairs", "allowed pairs"])
def test_same_clearance_as_mjpl_clearance(franka, allowed, distmax):
    m, Q = franka
    e = eng_mod.Engine(m, list(allowed))
    C, pair = e.clearance(Q, distmax)
    C2, pair2, grad, fromto, normal, status = e.clearance_grad(Q, distmax)
    assert C2.tobytes() == C.tobytes() and pair2.tobytes() == pair.tobytes()
    ok = status == eng_mod.GRAD_OK
    flat = status == eng_mod.GRAD_FLAT
    # flat exactly where the winner is capped at distmax: gradient 0, no witnesses
    capped = C == distmax - ref.pair_margins(m, e.contact_pairs()[0][pair])
    assert np.array_equal(flat, capped)
    assert np.all(grad[flat] == 0) and np.isnan(fromto[flat]).all() and np.isnan(normal[flat]).all()
    if distmax == INF:
        assert ok.mean() > 0.99, np.bincount(status)
    assert np.isfinite(grad[ok]).all() and np.isfinite(fromto[ok]).all()


# ---- 2. closed forms
def test_sphere_on_slide_facing_box_face():
    for sgn in (1.0, -1.0):
        m = one_pair(g("box", (0.2, 0.2, 0.2)), g("sphere", (0.1,), (0.5, 0, 0)), axis=(sgn, 0, 0))
        e, (C, pair, grad, fromto, normal, st) = grad_of(m, [[0.0]])
        assert st[0] == eng_mod.GRAD_OK and pair[0] == 0
        assert abs(C[0] - 0.2) <= 1e-12
        g1, g2 = e.contact_pairs()[0][0]
        assert m.geom_type[g1] == ref.SPHERE  # smaller type first: the sphere is g1
        np.testing.assert_allclose(grad[0], [sgn], atol=1e-12)
        np.testing.assert_allclose(fromto[0], [0.4, 0, 0, 0.2, 0, 0], atol=1e-12)
        np.testing.assert_allclose(normal[0], [-1, 0, 0], atol=1e-12)


def test_capsule_on_hinge_above_plane():
    # capsule along the body's x axis (r 0.05, half length 0.2), body 0.5 above the plane, hinge about y:
    # the +x end goes down by 0.2 sin q, D = 0.45 - 0.2 |sin q|
    m = one_pair(g("plane", (1, 1, 0.1)), g("capsule", (0.05, 0.2), q=quat((0, 1, 0), np.pi / 2)),
                 jtype="hinge", axis=(0, 1, 0), body_pos=(0, 0, 0.5))
    for q in (0.3, -0.7):
        e, (C, pair, grad, fromto, normal, st) = grad_of(m, [[q]])
        assert st[0] == eng_mod.GRAD_OK
        s = np.sign(q)
        assert abs(C[0] - (0.45 - 0.2 * abs(np.sin(q)))) <= 1e-12
        np.testing.assert_allclose(grad[0], [-0.2 * np.cos(q) * s], atol=1e-12)
        end = np.array([0, 0, 0.5]) + s * 0.2 * np.array([np.cos(q), 0, -np.sin(q)])
        low = end - [0, 0, 0.05]
        np.testing.assert_allclose(fromto[0], np.concatenate([[low[0], low[1], 0.0], low]), atol=1e-12)
        np.testing.assert_allclose(normal[0], [0, 0, 1], atol=1e-12)


def test_sphere_capsule():
    m = one_pair(g("capsule", (0.05, 0.3), q=quat((0, 1, 0), np.pi / 2)), g("sphere", (0.1,), (0.1, 0, 0.4)),
                 axis=(0, 0, 1))
    for q, want in ((0.0, 0.25), (-0.3, -0.05)):
        e, (C, pair, grad, fromto, normal, st) = grad_of(m, [[q]])
        assert st[0] == eng_mod.GRAD_OK
        assert abs(C[0] - want) <= 1e-12
        np.testing.assert_allclose(grad[0], [1.0], atol=1e-12)
        z = 0.4 + q
        np.testing.assert_allclose(fromto[0], [0.1, 0, z - 0.1, 0.1, 0, 0.05], atol=1e-12)
        np.testing.assert_allclose(normal[0], [0, 0, -1], atol=1e-12)


def test_boxes_overlapping_through_a_face_axis():
    m = one_pair(g("box", (0.2, 0.2, 0.2)), g("box", (0.2, 0.2, 0.2), (0.35, 0.01, -0.02)))
    e, (C, pair, grad, fromto, normal, st) = grad_of(m, [[0.0]])
    assert st[0] == eng_mod.GRAD_OK
    assert abs(C[0] + 0.05) <= 1e-12
    np.testing.assert_allclose(grad[0], [1.0], atol=1e-12)
    np.testing.assert_allclose(normal[0], [1, 0, 0], atol=1e-12)
    w1, w2 = fromto[0, :3], fromto[0, 3:]
    assert abs(w1[0] - 0.2) <= 1e-12 and abs(w2[0] - 0.15) <= 1e-12
    np.testing.assert_allclose(w1[1:], w2[1:], atol=1e-12)
    assert np.all(np.abs(w1[1:]) <= 0.2 + 1e-12) and np.all(np.abs(w2[1:] - [0.01, -0.02]) <= 0.2 + 1e-12)


def test_boxes_overlapping_through_an_edge_edge_axis():
    m = one_pair(g("box", (0.5, 0.1, 0.1), q=quat((1, 0, 0), np.pi / 4)),
                 g("box", (0.1, 0.5, 0.1), (0, 0, 0.5), quat((0, 1, 0), np.pi / 4)), axis=(0, 0, 1))
    q = -0.25
    e, (C, pair, grad, fromto, normal, st) = grad_of(m, [[q]])
    assert st[0] == eng_mod.GRAD_OK
    assert abs(C[0] - (0.5 + q - 0.2 * R2)) <= 1e-12
    np.testing.assert_allclose(grad[0], [1.0], atol=1e-12)
    np.testing.assert_allclose(normal[0], [0, 0, 1], atol=1e-12)
    np.testing.assert_allclose(fromto[0], [0, 0, 0.1 * R2, 0, 0, 0.5 + q - 0.1 * R2], atol=1e-12)


# ---- 3-5. models: witnesses, the Jacobian identity, central differences
def _model_cases():
    yield "franka_p", scenes.franka_p(obstacles=True), ()
    yield "franka_pads", scenes.franka_p(obstacles=True, pads=True), ()
    yield "ur5e", scenes.ur5e(), ()
    for seed in range(50):
        m, allowed = random_model(seed)
        yield f"random{seed}", m, allowed


MODELS = list(_model_cases())


def _configs(label, m, n, seed):
    if label.startswith("franka"):  # (the fingers as the benchmark holds them)
        return uniform_configs(m, n, seed=seed)
    rng = np.random.default_rng(seed)
    return rng.uniform(m.jnt_range[:, 0], m.jnt_range[:, 1], size=(n, m.nq))


def _check_witnesses(m, e, Q, C, pair, fromto, normal, status, label):
    ok = status == eng_mod.GRAD_OK
    if not ok.any():
        return 0
    pairs = e.contact_pairs()[0]
    P = pairs[pair[ok]]
    D = C[ok] + ref.pair_margins(m, pairs)[pair[ok]]
    k = gref_fk(m, Q[ok])
    gt = np.asarray(m.geom_type)
    gs = np.asarray(m.geom_size, float).reshape(-1, 3)
    idx = np.arange(len(P))
    w1, w2, n = fromto[ok, :3], fromto[ok, 3:], normal[ok]
    for col, w in ((0, w1), (1, w2)):
        for t in np.unique(gt[P[:, col]]):
            r = gt[P[:, col]] == t
            gg = P[r, col]
            sd = gref.point_geom_distance(int(t), k["geom_xpos"][idx[r], gg], k["geom_xmat"][idx[r], gg], gs[gg], w[r])
            assert np.abs(sd).max() <= 1e-9, f"{label}: witness {col + 1} off its geom (type {t}) by {np.abs(sd).max():.3e}"
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-12, label
    err = np.abs((w2 - w1) - D[:, None] * n).max()
    assert err <= 1e-9, f"{label}: |w2 - w1 - D n| = {err:.3e}"
    pos = D > 0
    if pos.any():
        err = np.abs(np.linalg.norm(w2[pos] - w1[pos], axis=1) - D[pos]).max()
        assert err <= 1e-9, f"{label}: |w2 - w1| != D by {err:.3e}"
    return int(ok.sum())


def gref_fk(m, Q):
    from oracle import pyoracle
    return pyoracle.Oracle(m).fk(Q)


@pytest.mark.parametrize("label,m,allowed", MODELS, ids=[c[0] for c in MODELS])
def test_witnesses_and_jacobian_identity(label, m, allowed):
    e = eng_mod.Engine(m, list(allowed))
    n = 8192 if label.startswith("franka") else 1024
    Q = _configs(label, m, n, seed=41)
    C, pair, grad, fromto, normal, status = e.clearance_grad(Q)
    _check_witnesses(m, e, Q, C, pair, fromto, normal, status, label)
    ok = status == eng_mod.GRAD_OK
    if ok.any():
        pairs = e.contact_pairs()[0]
        want = gref.clearance_gradient(m, Q[ok], pairs[pair[ok]], fromto[ok], normal[ok])
        err = np.abs(grad[ok] - want).max()
        assert err <= 1e-9, f"{label}: |grad - n . (J2 - J1)| = {err:.3e}"
    # the other statuses carry what the header says
    deg = status == eng_mod.GRAD_DEGENERATE
    assert np.isnan(grad[deg]).all() and np.isnan(normal[deg]).all() and np.isfinite(fromto[deg]).all()
    assert np.all((status == eng_mod.GRAD_OK) | deg | (status == eng_mod.GRAD_FLAT))


def _central_differences(e, Q, h):
    """(fd [N, nq] at step h and h/2 each, same-pair flag [N]) from one batched mjpl_clearance launch"""
    n, nq = Q.shape
    steps = np.array([h, -h, h / 2, -h / 2])
    S = np.repeat(Q[:, None, None, :], 4, axis=1).repeat(nq, axis=2)  # [N, 4, nq, nq]
    for j in range(nq):
        S[:, :, j, j] += steps[None, :]
    C, pair = e.clearance(S.reshape(-1, nq))
    C, pair = C.reshape(n, 4, nq), pair.reshape(n, 4, nq)
    fd_h = (C[:, 0] - C[:, 1]) / (2 * h)
    fd_h2 = (C[:, 2] - C[:, 3]) / h
    return fd_h, fd_h2, pair


def _fd_check(label, m, allowed, n):
    e = eng_mod.Engine(m, list(allowed))
    Q = _configs(label, m, n, seed=43)
    C, pair, grad, fromto, normal, status = e.clearance_grad(Q)
    ok = status == eng_mod.GRAD_OK
    fd_h, fd_h2, spair = _central_differences(e, Q[ok], 1e-6)
    same = np.all(spair == pair[ok][:, None, None], axis=(1, 2))
    steady = np.all(np.abs(fd_h - fd_h2) <= 1e-8, axis=1)
    keep = same & steady
    if keep.any():
        err = np.abs(grad[ok][keep] - fd_h2[keep]).max()
        assert err <= 1e-6, f"{label}: |grad - central difference| = {err:.3e}"
    return int(keep.sum()), int(ok.sum())


def test_central_differences_franka():
    kept, ok = _fd_check("franka_p", scenes.franka_p(obstacles=True), (), 2048)
    assert ok > 1000 and kept >= 0.9 * ok, (kept, ok)


@pytest.mark.parametrize("label,m,allowed", MODELS[1:], ids=[c[0] for c in MODELS[1:]])
def test_central_differences_other_models(label, m, allowed):
    kept, ok = _fd_check(label, m, allowed, 256)
    assert ok == 0 or kept > 0, (label, kept, ok)


# ---- 6. entry points, layouts, planning, statuses, errors
def _host_dev(e, Q, n, layout, distmax=INF, witnesses=True):
    host = e.clearance_grad(Q, distmax, layout=layout)
    npl = e.nplan
    dQ = e.alloc(max(Q.nbytes, 8)).upload(Q)
    dc, dp, dg, ds = e.alloc(max(n * 8, 8)), e.alloc(max(n * 4, 8)), e.alloc(max(n * npl * 8, 8)), e.alloc(max(n * 4, 8))
    df, dn = (e.alloc(max(n * 48, 8)), e.alloc(max(n * 24, 8))) if witnesses else (None, None)
    e.clearance_grad_dev(dQ.ptr, n, layout, dc.ptr, dp.ptr, dg.ptr, ds.ptr, df.ptr if df else None,
                         dn.ptr if dn else None, distmax=distmax)
    dev = [dc.download(np.float64, n), dp.download(np.int32, n), dg.download(np.float64, n * npl).reshape(n, npl)]
    if witnesses:
        dev += [df.download(np.float64, n * 6).reshape(n, 6), dn.download(np.float64, n * 3).reshape(n, 3)]
    dev.append(ds.download(np.int32, n))
    for b in (dQ, dc, dp, dg, ds, df, dn):
        if b is not None:
            b.free()
    want = host if witnesses else host[:3] + host[5:]
    for a, b in zip(want, dev):
        assert a.tobytes() == b.tobytes()
    return host


@pytest.mark.parametrize("n", [0, 1, 63, 65, 100003])
def test_device_and_host_entry_points_agree(n):
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    Q = uniform_configs(m, n, seed=33 + n)
    aos = _host_dev(e, Q, n, eng_mod.AOS)
    soa = _host_dev(e, np.ascontiguousarray(Q.T), n, eng_mod.SOA)
    for a, b in zip(aos, soa):
        assert a.tobytes() == b.tobytes()
    assert aos[2].shape == (n, m.nq)
    _host_dev(e, Q, n, eng_mod.AOS, witnesses=False)  # fromto / normal NULL
    if n == 100003:  # across the 2^16-row chunk: the rows of the second launch equal a launch of their own
        tail = e.clearance_grad(Q[65536:65536 + 1000])
        for a, b in zip(tail, aos):
            assert a.tobytes() == b[65536:65536 + 1000].tobytes()


def test_host_form_without_witnesses():
    import ctypes as C
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    Q = uniform_configs(m, 100, seed=34)
    want = e.clearance_grad(Q)
    c, p, gr, st = np.zeros(100), np.zeros(100, np.int32), np.zeros((100, m.nq)), np.zeros(100, np.int32)
    F, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = e.lib.mjpl_clearance_grad(e.h, Q.ctypes.data_as(F), 100, eng_mod.AOS, INF, c.ctypes.data_as(F),
                                   p.ctypes.data_as(I), gr.ctypes.data_as(F), None, None, st.ctypes.data_as(I))
    assert rc == 0
    for a, b in zip((c, p, gr, st), want[:3] + want[5:]):
        assert a.tobytes() == b.tobytes()


def test_after_set_planning_and_fresh_engine():
    m = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS)
    sub = arm[[0, 2, 3, 5]]
    base = m.keyframe("home").qpos.copy()
    base[arm[1]] += 0.2
    e = eng_mod.Engine(m)
    e.clearance_grad(uniform_configs(m, 100, seed=35))  # (a launch with the full planning set first)
    e.set_planning(sub, base)
    full = uniform_configs(m, 4096, seed=36)
    Qp = np.ascontiguousarray(full[:, sub])
    got = _host_dev(e, Qp, len(Qp), eng_mod.AOS)
    assert got[2].shape == (len(Qp), len(sub))
    f = eng_mod.Engine(m)
    f.set_planning(sub, base)
    for a, b in zip(f.clearance_grad(Qp), got):
        assert a.tobytes() == b.tobytes()
    # the planning columns' gradient is the full gradient's columns at the same configuration
    held = base.copy()
    Qf = np.repeat(held[None, :], len(Qp), axis=0)
    Qf[:, sub] = Qp
    e2 = eng_mod.Engine(m)
    full_out = e2.clearance_grad(Qf)
    assert full_out[0].tobytes() == got[0].tobytes() and full_out[1].tobytes() == got[1].tobytes()
    ok = got[5] == eng_mod.GRAD_OK
    np.testing.assert_allclose(got[2][ok], full_out[2][ok][:, sub], rtol=0, atol=1e-12)
    # CollisionConstraint: the planning form and the full form
    c = CollisionConstraint(m)
    c.set_planning(sub, base)
    pl = c.clearance_gradient_planning(Qp)
    assert pl[0].tobytes() == got[0].tobytes() and pl[2].tobytes() == got[2].tobytes()
    one = c.clearance_gradient(Qf[0])
    C0, pair0 = c.clearance(Qf[0])
    assert one.clearance == C0 and one.pair == pair0 and one.gradient.shape == (m.nq,)


def test_nonfinite_rows():
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    Q = uniform_configs(m, 200, seed=37)
    Q[3, 2], Q[77, 0], Q[150, 8] = np.nan, np.inf, -np.inf
    C, pair, grad, fromto, normal, status = e.clearance_grad(Q)
    bad = np.zeros(200, bool)
    bad[[3, 77, 150]] = True
    assert np.all(status[bad] == eng_mod.GRAD_NONFINITE) and np.all(pair[bad] == -1)
    assert np.isnan(C[bad]).all() and np.isnan(grad[bad]).all() and np.isnan(fromto[bad]).all()
    assert np.isnan(normal[bad]).all() and not np.any(status[~bad] == eng_mod.GRAD_NONFINITE)


def test_capped_winner_is_flat():
    m = one_pair(g("sphere", (0.1,)), g("sphere", (0.2,), (0.5, 0, 0)))
    e, (C, pair, grad, fromto, normal, st) = grad_of(m, [[0.0], [-0.25]], distmax=0.1)
    assert C[0] == 0.1 and pair[0] == 0 and st[0] == eng_mod.GRAD_FLAT and grad[0, 0] == 0
    assert np.isnan(fromto[0]).all() and np.isnan(normal[0]).all()
    assert abs(C[1] + 0.05) <= 1e-12 and st[1] == eng_mod.GRAD_OK and abs(grad[1, 0] - 1) <= 1e-12


def test_only_allowed_pairs_is_flat():
    mb = ModelBuilder()
    mb.add_body("m")
    mb.add_joint("m", "j", type="slide", axis=(1, 0, 0), range=(-2, 2))
    mb.add_geom("world", type="sphere", size=(0.1,))
    mb.add_geom("m", type="sphere", size=(0.1,), pos=(0.5, 0, 0))
    m = mb.compile()
    e = eng_mod.Engine(m, [("world", "m")])
    assert e.contact_pairs()[1].all()
    C, pair, grad, fromto, normal, status = e.clearance_grad(np.array([[0.0], [0.3]]))
    assert np.all(status == eng_mod.GRAD_FLAT) and np.all(pair == -1) and np.all(C == INF)
    assert np.all(grad == 0) and np.isnan(fromto).all() and np.isnan(normal).all()


def test_empty_candidate_table_is_flat():
    from test_gpu_distance import no_pair_model
    e = eng_mod.Engine(no_pair_model())
    for distmax in (INF, 0.05):
        C, pair, grad, fromto, normal, status = e.clearance_grad(np.linspace(-1, 1, 5)[:, None], distmax)
        assert np.all(status == eng_mod.GRAD_FLAT) and np.all(pair == -1) and np.all(C == distmax)
        assert grad.shape == (5, 1) and np.all(grad == 0) and np.isnan(fromto).all() and np.isnan(normal).all()


def test_argument_errors():
    import ctypes as C
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    Q = uniform_configs(m, 4, seed=38)
    F, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    c, p, gr, st = np.zeros(4), np.zeros(4, np.int32), np.zeros((4, m.nq)), np.zeros(4, np.int32)
    args = [c.ctypes.data_as(F), p.ctypes.data_as(I), gr.ctypes.data_as(F), None, None, st.ctypes.data_as(I)]
    qp = Q.ctypes.data_as(F)
    f = e.lib.mjpl_clearance_grad
    assert f(e.h, qp, 4, eng_mod.AOS, INF, *args) == 0
    for dm in (0.0, -1.0, float("nan")):
        assert f(e.h, qp, 4, eng_mod.AOS, dm, *args) == E_ARG
    assert f(e.h, qp, 4, 7, INF, *args) == E_ARG  # unknown layout
    assert f(e.h, qp, -1, eng_mod.AOS, INF, *args) == E_ARG
    for k in (0, 1, 2, 5):  # clear, pair, grad, status are required
        a = list(args)
        a[k] = None
        assert f(e.h, qp, 4, eng_mod.AOS, INF, *a) == E_ARG
    assert f(e.h, qp, 0, eng_mod.AOS, INF, None, None, None, None, None, None) == 0  # N = 0: nothing to write
    assert e.lib.mjpl_clearance_grad_dev(e.h, None, 4, eng_mod.AOS, INF, None, None, None, None, None, None) == E_ARG
