"""Near pairs on the GPU (include/mjpl_hip.h: mjpl_near_pairs*; CollisionConstraint.near_pairs*): closed forms on
hand-built scenes, the two-wall case the clearance's gradient cannot express, the list and its distances against
mjpl_distances bit for bit, the clearance and the clearance's gradient rebuilt from the list bit for bit, the NumPy
statements of tests/near_reference.py and tests/gradient_reference.py, central differences of mjpl_distances per pair,
truncation at K, and the entry points' forms, statuses and argument errors."""
import ctypes as C
import functools

import numpy as np
import pytest

import distance_reference as ref
import gradient_reference as gref
import near_reference as nref
from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes
from mjpl_amd.constraint import CollisionConstraint
from mjpl_amd.model import ModelBuilder
from helpers import uniform_configs
from test_gpu_clearance_grad import g, one_pair, quat
from test_gpu_models import random_model
from test_near_pairs_host import FD_DISTMAX, FD_H, FD_ROWS, FD_SEED

pytestmark = pytest.mark.gpu

E_ARG = -1  # MJPL_E_ARG
INF = float("inf")
F, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
NAMES = ("count", "pair", "dist", "grad", "fromto", "normal", "status")


def near_of(m, Q, distmax, K=4):
    e = eng_mod.Engine(m)
    return e, e.near_pairs(np.atleast_2d(np.asarray(Q, float)), distmax, K)


# ---- 1. closed forms, one-pair scenes
def test_sphere_on_slide_facing_box_face():
    for sgn in (1.0, -1.0):
        m = one_pair(g("box", (0.2, 0.2, 0.2)), g("sphere", (0.1,), (0.5, 0, 0)), axis=(sgn, 0, 0))
        e, (count, pair, dist, grad, fromto, normal, st) = near_of(m, [[0.0]], INF)
        assert count[0] == 1 and pair[0, 0] == 0 and np.all(pair[0, 1:] == -1) and st[0, 0] == eng_mod.GRAD_OK
        assert abs(dist[0, 0] - 0.2) <= 1e-12
        np.testing.assert_allclose(grad[0, 0], [sgn], atol=1e-12)
        np.testing.assert_allclose(fromto[0, 0], [0.4, 0, 0, 0.2, 0, 0], atol=1e-12)
        np.testing.assert_allclose(normal[0, 0], [-1, 0, 0], atol=1e-12)
        # distmax below the distance: nothing is listed
        _, (count, pair, dist, grad, fromto, normal, st) = near_of(m, [[0.0]], 0.15)
        assert count[0] == 0 and np.all(pair == -1) and np.isnan(dist).all() and np.isnan(grad).all()


def test_capsule_on_hinge_above_plane():
    m = one_pair(g("plane", (1, 1, 0.1)), g("capsule", (0.05, 0.2), q=quat((0, 1, 0), np.pi / 2)),
                 jtype="hinge", axis=(0, 1, 0), body_pos=(0, 0, 0.5))
    for q in (0.3, -0.7):
        e, (count, pair, dist, grad, fromto, normal, st) = near_of(m, [[q]], 1.0)
        assert count[0] == 1 and pair[0, 0] == 0 and st[0, 0] == eng_mod.GRAD_OK
        s = np.sign(q)
        want = 0.45 - 0.2 * abs(np.sin(q))
        assert abs(dist[0, 0] - want) <= 1e-12
        np.testing.assert_allclose(grad[0, 0], [-0.2 * np.cos(q) * s], atol=1e-12)
        end = np.array([0, 0, 0.5]) + s * 0.2 * np.array([np.cos(q), 0, -np.sin(q)])
        low = end - [0, 0, 0.05]
        np.testing.assert_allclose(fromto[0, 0], np.concatenate([[low[0], low[1], 0.0], low]), atol=1e-12)
        np.testing.assert_allclose(normal[0, 0], [0, 0, 1], atol=1e-12)
        _, (count, pair, *_rest) = near_of(m, [[q]], want - 0.01)
        assert count[0] == 0 and np.all(pair == -1)


def test_boxes_overlapping_through_a_face_axis():
    m = one_pair(g("box", (0.2, 0.2, 0.2)), g("box", (0.2, 0.2, 0.2), (0.35, 0.01, -0.02)))
    # (an overlap is below every distmax > 0: the smallest the header admits still lists it)
    for distmax in (INF, 1e-300):
        e, (count, pair, dist, grad, fromto, normal, st) = near_of(m, [[0.0]], distmax)
        assert count[0] == 1 and pair[0, 0] == 0 and st[0, 0] == eng_mod.GRAD_OK
        assert abs(dist[0, 0] + 0.05) <= 1e-12
        np.testing.assert_allclose(grad[0, 0], [1.0], atol=1e-12)
        np.testing.assert_allclose(normal[0, 0], [1, 0, 0], atol=1e-12)
        w1, w2 = fromto[0, 0, :3], fromto[0, 0, 3:]
        assert abs(w1[0] - 0.2) <= 1e-12 and abs(w2[0] - 0.15) <= 1e-12
        np.testing.assert_allclose(w1[1:], w2[1:], atol=1e-12)
        assert np.all(np.abs(w1[1:]) <= 0.2 + 1e-12) and np.all(np.abs(w2[1:] - [0.01, -0.02]) <= 0.2 + 1e-12)


# ---- 2. the motivating case: a sphere halfway between two walls
def two_walls():
    mb = ModelBuilder()
    mb.add_body("m")
    mb.add_joint("m", "j", type="slide", axis=(1, 0, 0), range=(-2, 2))
    mb.add_geom("world", **g("box", (0.2, 1, 1), (-1.2, 0, 0)))  # faces at x = -1 and x = +1
    mb.add_geom("world", **g("box", (0.2, 1, 1), (1.2, 0, 0)))
    mb.add_geom("m", **g("sphere", (0.1,)))
    return mb.compile()


def test_sphere_between_two_walls():
    m = two_walls()
    c = CollisionConstraint(m)
    e = c.engine
    pairs = e.contact_pairs()[0]
    assert len(pairs) == 2
    count, pair, dist, grad, fromto, normal, st = e.near_pairs(np.zeros((1, 1)), INF, 4)
    assert count[0] == 2 and pair[0].tolist() == [0, 1, -1, -1] and np.all(st[0, :2] == eng_mod.GRAD_OK)
    np.testing.assert_allclose(dist[0, :2], [0.9, 0.9], atol=1e-12)
    # moving towards +x closes the gap to the wall at +1 and opens the other
    wall_x = np.asarray(m.geom_pos, float).reshape(-1, 3)[pairs[:, 1], 0]  # (the sphere is g1: smaller type first)
    np.testing.assert_allclose(grad[0, :2, 0], -np.sign(wall_x), atol=1e-12)
    assert sorted(grad[0, :2, 0].round(9).tolist()) == [-1.0, 1.0]
    # the clearance's gradient is exactly one of the two
    C_, cp, cg, cf, cn, cs = e.clearance_grad(np.zeros((1, 1)))
    assert cp[0] in (0, 1) and cs[0] == eng_mod.GRAD_OK
    assert cg[0].tobytes() == grad[0, cp[0]].tobytes() and C_[0] == dist[0, cp[0]]
    # the constraint's form
    near = c.near_pairs(np.zeros(1), 1.0)
    assert [n.pair for n in near] == [tuple(int(x) for x in r) for r in pairs]
    assert near[0].distance == dist[0, 0] and near[1].gradient.tobytes() == grad[0, 1].tobytes()
    assert near[0].fromto.shape == (6,) and near[0].normal.shape == (3,) and near[0].status == eng_mod.GRAD_OK
    assert c.near_pairs(np.zeros(1), 0.5) == []
    assert len(c.near_pairs(np.array([0.5]), 0.5)) == 1
    with pytest.raises(ValueError):
        c.near_pairs(np.array([np.nan]), 1.0)


# ---- 3-6. models
def _model_cases():
    yield "franka_p", scenes.franka_p(obstacles=True), ()
    yield "franka_pads", scenes.franka_p(obstacles=True, pads=True), ()
    yield "ur5e", scenes.ur5e(), ()
    for seed in range(12):
        m, allowed = random_model(seed)
        yield f"random{seed}", m, tuple(allowed)


MODELS = {c[0]: c for c in _model_cases()}
ROWS = 256


@functools.lru_cache(maxsize=None)
def model_setup(label):
    """(model, engine, Q, pairs, allowed flags, margins, mjpl_distances at distmax = inf): made once per model"""
    _, m, allowed = MODELS[label]
    e = eng_mod.Engine(m, list(allowed))
    if label.startswith("franka"):
        Q = uniform_configs(m, ROWS, seed=41)
    else:
        Q = np.random.default_rng(41).uniform(m.jnt_range[:, 0], m.jnt_range[:, 1], size=(ROWS, m.nq))
    pairs, flags = e.contact_pairs()
    return m, e, Q, pairs, flags, ref.pair_margins(m, pairs), e.distances(Q)


@functools.lru_cache(maxsize=None)
def model_run(label, distmax):
    """near_pairs with a slot for every non-allowed pair: made once per (model, distmax), shared and left unchanged"""
    m, e, Q, pairs, flags, margins, Dfull = model_setup(label)
    K = max(int((~flags).sum()), 1)
    out = e.near_pairs(Q, distmax, K)
    for a in out:
        a.setflags(write=False)
    return K, out


def listed(count, K):
    """bool [N, K]: slot k of row i is listed"""
    return np.arange(K)[None, :] < np.minimum(count, K)[:, None]


@pytest.mark.parametrize("distmax", [0.05, INF], ids=["0.05", "inf"])
@pytest.mark.parametrize("label", list(MODELS))
def test_list_and_distances_equal_mjpl_distances(label, distmax):
    m, e, Q, pairs, flags, margins, Dfull = model_setup(label)
    K, (count, pair, dist, grad, fromto, normal, status) = model_run(label, distmax)
    want = ~flags[None, :] & (Dfull < distmax)  # [N, P]
    assert np.array_equal(count, want.sum(axis=1))
    order = np.argsort(~want, axis=1, kind="stable")[:, :K]  # the True columns first, ascending
    L = listed(count, K)
    if order.shape[1] < K:  # (P = 0: K = 1)
        order = np.full((len(Q), K), -1)
    assert np.array_equal(pair, np.where(L, order, -1))
    ii = np.nonzero(L)[0]
    assert dist[L].tobytes() == Dfull[ii, pair[L]].tobytes()
    assert np.all((status[L] == eng_mod.GRAD_OK) | (status[L] == eng_mod.GRAD_DEGENERATE))
    # unlisted slots are the binding's fill
    assert np.isnan(dist[~L]).all() and np.isnan(grad[~L]).all() and np.all(status[~L] == -1)


@pytest.mark.parametrize("distmax", [0.05, INF], ids=["0.05", "inf"])
@pytest.mark.parametrize("label", list(MODELS))
def test_clearance_rebuilt_from_the_list(label, distmax):
    m, e, Q, pairs, flags, margins, Dfull = model_setup(label)
    K, (count, pair, dist, *_rest) = model_run(label, distmax)
    C_, cp = e.clearance(Q, distmax)
    free = np.flatnonzero(~flags)
    if len(free) == 0:
        assert np.all(count == 0) and np.all(cp == -1) and np.all(C_ == distmax)
        return
    # listed pairs at dist - margin, every other non-allowed pair at distmax - margin; the lowest index on ties
    V = np.repeat((distmax - margins)[None, :], len(Q), axis=0)
    L = listed(count, K)
    ii = np.nonzero(L)[0]
    V[ii, pair[L]] = dist[L] - margins[pair[L]]
    V = V[:, free]
    arg = np.argmin(V, axis=1)
    assert V[np.arange(len(Q)), arg].tobytes() == C_.tobytes()
    assert np.array_equal(free[arg].astype(np.int32), cp)


@pytest.mark.parametrize("distmax", [0.05, INF], ids=["0.05", "inf"])
@pytest.mark.parametrize("label", list(MODELS))
def test_winner_slot_equals_clearance_grad(label, distmax):
    m, e, Q, pairs, flags, margins, Dfull = model_setup(label)
    K, (count, pair, dist, grad, fromto, normal, status) = model_run(label, distmax)
    C_, cp, cg, cf, cn, cs = e.clearance_grad(Q, distmax)
    rows = np.flatnonzero((cs == eng_mod.GRAD_OK) | (cs == eng_mod.GRAD_DEGENERATE))
    hit = pair[rows] == cp[rows, None]
    assert np.all(hit.sum(axis=1) == 1), f"{label}: the clearance's pair is not listed once"
    k = np.argmax(hit, axis=1)
    for name, a, b in (("grad", grad, cg), ("fromto", fromto, cf), ("normal", normal, cn), ("status", status, cs)):
        assert a[rows, k].tobytes() == b[rows].tobytes(), f"{label}: {name} differs from mjpl_clearance_grad"
    assert (dist[rows, k] - margins[cp[rows]]).tobytes() == C_[rows].tobytes()


@pytest.mark.parametrize("label", list(MODELS))
def test_against_numpy(label):
    distmax = 0.1
    m, e, Q, pairs, flags, margins, Dfull = model_setup(label)
    K, (count, pair, dist, grad, fromto, normal, status) = model_run(label, distmax)
    assert np.all(count <= K)
    rows_ref, Dref = nref.near_pairs(m, Q, pairs, flags, distmax)
    P = len(pairs)
    L = listed(count, K)
    ii, kk = np.nonzero(L)
    pp = pair[L]
    got = np.zeros((len(Q), P), bool)
    got[ii, pp] = True
    want = np.zeros((len(Q), P), bool)
    ri, rp, rd = nref.flatten(rows_ref)
    want[ri, rp] = True
    clear_cut = np.abs(Dref - distmax) > 1e-9
    assert np.array_equal(got[clear_cut], want[clear_cut]), f"{label}: the list differs from the reference's"
    if len(pp) == 0:
        return
    err = np.abs(dist[L] - Dref[ii, pp]).max()
    assert err <= 1e-9, f"{label}: |dist - reference| = {err:.3e}"
    assert np.all(np.diff(pair, axis=1)[L[:, 1:]] > 0), f"{label}: a row is not ascending"
    # witnesses on their geoms, |n| = 1, w2 - w1 = D n, the gradient: on the OK slots, flattened
    ok = status[L] == eng_mod.GRAD_OK
    deg = status[L] == eng_mod.GRAD_DEGENERATE
    assert np.all(ok | deg)
    assert np.isnan(grad[L][deg]).all() and np.isnan(normal[L][deg]).all() and np.isfinite(fromto[L][deg]).all()
    if not ok.any():
        return
    i, p, D = ii[ok], pp[ok], dist[L][ok]
    ft, n, gr = fromto[L][ok], normal[L][ok], grad[L][ok]
    from oracle import pyoracle
    fk = pyoracle.Oracle(m).fk(Q[i])
    gt = np.asarray(m.geom_type)
    gs = np.asarray(m.geom_size, float).reshape(-1, 3)
    idx = np.arange(len(i))
    G = pairs[p]
    for col, w in ((0, ft[:, :3]), (1, ft[:, 3:])):
        for t in np.unique(gt[G[:, col]]):
            r = gt[G[:, col]] == t
            gg = G[r, col]
            sd = gref.point_geom_distance(int(t), fk["geom_xpos"][idx[r], gg], fk["geom_xmat"][idx[r], gg], gs[gg], w[r])
            assert np.abs(sd).max() <= 1e-9, f"{label}: witness {col + 1} off its geom (type {t}) by {np.abs(sd).max():.3e}"
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-12, label
    err = np.abs((ft[:, 3:] - ft[:, :3]) - D[:, None] * n).max()
    assert err <= 1e-9, f"{label}: |w2 - w1 - D n| = {err:.3e}"
    want_g = gref.clearance_gradient(m, Q[i], G, ft, n, fk=fk)
    err = np.abs(gr - want_g).max()
    assert err <= 1e-9, f"{label}: |grad - n . (J2 - J1)| = {err:.3e}"


# ---- 7. central differences of mjpl_distances, per listed pair
@pytest.fixture(scope="module")
def franka512():
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    Q = uniform_configs(m, 512, seed=FD_SEED)
    out = e.near_pairs(Q, FD_DISTMAX, 32)
    for a in out:
        a.setflags(write=False)
    assert out[0].max() <= 32  # (25 by the reference: K = 32 cuts nothing)
    return m, e, Q, out


def test_central_differences_per_pair(franka512):
    m, e, Q512, _ = franka512
    Q = Q512[:FD_ROWS]  # (uniform_configs draws row by row: the first rows of the 512 are the study's 96)
    assert np.array_equal(Q, uniform_configs(m, FD_ROWS, seed=FD_SEED))
    count, pair, dist, grad, fromto, normal, status = e.near_pairs(Q, FD_DISTMAX, 32)
    L = listed(count, 32)
    ii = np.nonzero(L)[0]
    pp = pair[L]
    fd_h, fd_h2 = nref.central_differences(e.distances, Q, FD_H)  # one mjpl_distances call: 4 * 9 * 96 rows
    a, b = fd_h[ii, :, pp], fd_h2[ii, :, pp]
    ok = status[L] == eng_mod.GRAD_OK
    keep = ok & np.all(np.abs(a - b) <= 1e-8, axis=1)
    print(f"listed {len(pp)}, OK {int(ok.sum())}, kept {int(keep.sum())}")
    assert ok.sum() > 500
    err = np.abs(grad[L][keep] - b[keep]).max()
    print(f"|grad - central difference| = {err:.3e}")
    assert err <= 1e-6, f"|grad - central difference| = {err:.3e}"
    assert keep.sum() >= 0.9 * ok.sum(), (int(keep.sum()), int(ok.sum()))


# ---- 8. truncation
SENT_F, SENT_I = -12345.678, 777


def raw_call(e, Q, distmax, K, layout=eng_mod.AOS, witnesses=True, fn=None):
    """mjpl_near_pairs on host arrays pre-filled with a sentinel -> (rc, arrays in NAMES order)"""
    n = Q.shape[0] if layout == eng_mod.AOS else Q.shape[1]
    out = dict(count=np.full(n, SENT_I, np.int32), pair=np.full((n, K), SENT_I, np.int32),
               dist=np.full((n, K), SENT_F), grad=np.full((n, K, e.nplan), SENT_F), fromto=np.full((n, K, 6), SENT_F),
               normal=np.full((n, K, 3), SENT_F), status=np.full((n, K), SENT_I, np.int32))
    p = {k: v.ctypes.data_as(I if v.dtype == np.int32 else F) for k, v in out.items()}
    if not witnesses:
        p["fromto"] = p["normal"] = None
    Q = np.ascontiguousarray(Q, float)
    rc = (fn or e.lib.mjpl_near_pairs)(e.h, Q.ctypes.data_as(F), n, layout, distmax, K, p["count"], p["pair"], p["dist"],
                                       p["grad"], p["fromto"], p["normal"], p["status"])
    return rc, [out[k] for k in NAMES]


@pytest.mark.parametrize("K", [1, 8])
def test_truncation(franka512, K):
    m, e, Q, full = franka512
    rc, got = raw_call(e, Q, FD_DISTMAX, K)
    assert rc == 0
    count = got[0]
    assert np.array_equal(count, full[0])
    assert np.mean(count > K) > 0.2  # many rows overflow
    L = listed(count, K)
    for name, a, b in zip(NAMES[1:], got[1:], full[1:]):
        assert a[L].tobytes() == b[:, :K][L].tobytes(), name
        want = -1 if name == "pair" else (SENT_I if name == "status" else SENT_F)
        assert np.all(a[~L] == want), f"{name}: a slot past the list was written"


# ---- 9. shapes and entry points
def _dev_call(e, Q, n, layout, distmax, K, witnesses=True):
    """mjpl_near_pairs_dev on device buffers pre-filled with the sentinel of raw_call"""
    npl = e.nplan
    shapes = dict(count=(n,), pair=(n, K), dist=(n, K), grad=(n, K, npl), fromto=(n, K, 6), normal=(n, K, 3),
                  status=(n, K))
    dQ = e.alloc(max(Q.nbytes, 8)).upload(Q)
    bufs = {}
    for k, shp in shapes.items():
        dt = np.int32 if k in ("count", "pair", "status") else np.float64
        fill = np.full(shp, SENT_I if dt == np.int32 else SENT_F, dt)
        bufs[k] = e.alloc(max(fill.nbytes, 8)).upload(fill)
    e.near_pairs_dev(dQ.ptr, n, layout, distmax, K, bufs["count"].ptr, bufs["pair"].ptr, bufs["dist"].ptr,
                     bufs["grad"].ptr, bufs["status"].ptr, bufs["fromto"].ptr if witnesses else None,
                     bufs["normal"].ptr if witnesses else None)
    out = []
    for k in NAMES:
        dt = np.int32 if k in ("count", "pair", "status") else np.float64
        out.append(bufs[k].download(dt, int(np.prod(shapes[k]))).reshape(shapes[k]))
    for b in [dQ, *bufs.values()]:
        b.free()
    return out


def _host_dev(e, Q, n, layout, distmax=0.1, K=2):
    rc, host = raw_call(e, Q, distmax, K, layout)
    assert rc == 0
    dev = _dev_call(e, Q, n, layout, distmax, K)
    for name, a, b in zip(NAMES, host, dev):
        assert a.tobytes() == b.tobytes(), name
    # fromto / normal NULL: the rest unchanged, in both forms
    rc, host_nw = raw_call(e, Q, distmax, K, layout, witnesses=False)
    assert rc == 0
    dev_nw = _dev_call(e, Q, n, layout, distmax, K, witnesses=False)
    for k, name in enumerate(NAMES):
        if name in ("fromto", "normal"):
            assert np.all(host_nw[k] == SENT_F) and np.all(dev_nw[k] == SENT_F)
        else:
            assert host_nw[k].tobytes() == host[k].tobytes() and dev_nw[k].tobytes() == host[k].tobytes(), name
    return host


@pytest.mark.parametrize("n", [0, 1, 63, 65, 257, 65539])
def test_device_and_host_entry_points_agree(n):
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    Q = uniform_configs(m, n, seed=53 + n)
    aos = _host_dev(e, Q, n, eng_mod.AOS)
    soa = _host_dev(e, np.ascontiguousarray(Q.T), n, eng_mod.SOA)
    for a, b in zip(aos, soa):
        assert a.tobytes() == b.tobytes()
    assert aos[3].shape == (n, 2, m.nq)
    if n:
        assert np.all(aos[0] >= 0) and np.all((aos[1] >= 0) == listed(aos[0], 2))
    if n == 65539:  # across the 2^16-row chunk: the rows of the second launch equal a launch of their own
        rc, tail = raw_call(e, Q[65536:], 0.1, 2)
        for a, b in zip(tail, aos):
            assert a.tobytes() == b[65536:].tobytes()
        assert aos[0][65536:].max() > 0


def test_after_set_planning_and_fresh_engine():
    m = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS)
    sub = arm[[0, 2, 3, 5]]
    base = m.keyframe("home").qpos.copy()
    base[arm[1]] += 0.2
    e = eng_mod.Engine(m)
    e.near_pairs(uniform_configs(m, 100, seed=55), 0.1, 8)  # (a launch with the full planning set first)
    e.set_planning(sub, base)
    full = uniform_configs(m, 1024, seed=56)
    Qp = np.ascontiguousarray(full[:, sub])
    got = e.near_pairs(Qp, 0.1, 16)
    assert got[3].shape == (len(Qp), 16, len(sub)) and got[0].max() > 0
    f = eng_mod.Engine(m)
    f.set_planning(sub, base)
    for a, b in zip(f.near_pairs(Qp, 0.1, 16), got):
        assert a.tobytes() == b.tobytes()
    # the planning columns' gradient is the full gradient's columns at the same configuration
    Qf = np.repeat(base[None, :], len(Qp), axis=0)
    Qf[:, sub] = Qp
    c = CollisionConstraint(m)
    fo = c.near_pairs_batch(Qf, 0.1, 16)
    assert fo[0].tobytes() == got[0].tobytes() and fo[1].tobytes() == got[1].tobytes()
    assert fo[2].tobytes() == got[2].tobytes()
    ok = got[6] == eng_mod.GRAD_OK
    np.testing.assert_allclose(got[3][ok], fo[3][ok][:, sub], rtol=0, atol=1e-12)
    c.set_planning(sub, base)
    pl = c.near_pairs_planning(Qp, 0.1, 16)
    for a, b in zip(pl, got):
        assert a.tobytes() == b.tobytes()


def test_nonfinite_rows():
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    Q = uniform_configs(m, 200, seed=57)
    want = e.near_pairs(Q, 0.1, 8)
    Q[3, 2], Q[77, 0], Q[150, 8] = np.nan, np.inf, -np.inf
    got = e.near_pairs(Q, 0.1, 8)
    bad = np.zeros(200, bool)
    bad[[3, 77, 150]] = True
    assert np.all(got[0][bad] == -1) and np.all(got[1][bad] == -1)
    assert np.isnan(got[2][bad]).all() and np.isnan(got[3][bad]).all() and np.all(got[6][bad] == -1)
    for a, b in zip(got, want):
        assert a[~bad].tobytes() == b[~bad].tobytes()
    assert want[0].max() > 0


def test_only_allowed_pairs_and_empty_table():
    mb = ModelBuilder()
    mb.add_body("m")
    mb.add_joint("m", "j", type="slide", axis=(1, 0, 0), range=(-2, 2))
    mb.add_geom("world", type="sphere", size=(0.1,))
    mb.add_geom("m", type="sphere", size=(0.1,), pos=(0.5, 0, 0))
    e = eng_mod.Engine(mb.compile(), [("world", "m")])
    assert e.contact_pairs()[1].all()
    Q = np.array([[0.0], [0.3], [np.nan]])
    count, pair, dist, grad, fromto, normal, status = e.near_pairs(Q, INF, 3)
    assert count.tolist() == [0, 0, -1] and np.all(pair == -1) and np.isnan(dist).all() and np.all(status == -1)
    from test_gpu_distance import no_pair_model
    e = eng_mod.Engine(no_pair_model())
    for distmax in (INF, 0.05):
        count, pair, dist, grad, *_rest = e.near_pairs(np.linspace(-1, 1, 5)[:, None], distmax, 2)
        assert np.all(count == 0) and np.all(pair == -1) and grad.shape == (5, 2, 1) and np.isnan(dist).all()
    assert CollisionConstraint(no_pair_model()).near_pairs(np.zeros(1), INF) == []


def test_argument_errors():
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    Q = uniform_configs(m, 4, seed=58)
    rc, good = raw_call(e, Q, 0.1, 2)
    assert rc == 0 and good[0].min() >= 0

    def untouched(out):
        return all(np.all(a == (SENT_I if a.dtype == np.int32 else SENT_F)) for a in out)

    for dm in (0.0, -1.0, float("nan")):
        rc, out = raw_call(e, Q, dm, 2)
        assert rc == E_ARG and untouched(out)
    for K in (0, -3):
        rc, out = raw_call(e, Q, 0.1, max(K, 1), fn=lambda h, q, n, lay, dm, _k, *a: e.lib.mjpl_near_pairs(h, q, n, lay, dm, K, *a))
        assert rc == E_ARG and untouched(out)
    rc, out = raw_call(e, Q, 0.1, 2, fn=lambda h, q, n, lay, *a: e.lib.mjpl_near_pairs(h, q, n, 7, *a))
    assert rc == E_ARG and untouched(out)  # unknown layout
    rc, out = raw_call(e, Q, 0.1, 2, fn=lambda h, q, n, *a: e.lib.mjpl_near_pairs(h, q, -1, *a))
    assert rc == E_ARG and untouched(out)
    for k in (0, 1, 2, 3, 6):  # count, pair, dist, grad and status are required

        def drop(h, q, n, lay, dm, K, *a, k=k):
            a = list(a)
            a[k] = None
            return e.lib.mjpl_near_pairs(h, q, n, lay, dm, K, *a)

        rc, out = raw_call(e, Q, 0.1, 2, fn=drop)
        assert rc == E_ARG and untouched(out), NAMES[k]
    f = e.lib.mjpl_near_pairs
    assert f(e.h, Q.ctypes.data_as(F), 0, eng_mod.AOS, 0.1, 2, None, None, None, None, None, None, None) == 0  # N = 0
    assert e.lib.mjpl_near_pairs_dev(e.h, None, 4, eng_mod.AOS, 0.1, 2, None, None, None, None, None, None, None) == E_ARG
    assert e.lib.mjpl_near_pairs_dev(e.h, None, 0, eng_mod.AOS, 0.1, 0, None, None, None, None, None, None, None) == E_ARG
    with pytest.raises(eng_mod.MjplError) as ei:
        e.near_pairs(Q, 0.1, 0)
    assert ei.value.code == E_ARG
