"""Signed geom distances and clearance on the GPU (include/mjpl_hip.h: mjpl_distances* / mjpl_clearance*;
CollisionConstraint.pair_distances / clearance): closed-form scenes, the NumPy reference of
tests/distance_reference.py on the benchmark scene, moving boxes, UR5e and random models, the contact and
validity invariants, distmax, and the agreement of the host and device entry points."""
import numpy as np
import pytest

import distance_reference as ref
from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes
from mjpl_amd.constraint import CollisionConstraint
from mjpl_amd.constraint.collision_constraint import contact_hits
from mjpl_amd.model import ModelBuilder
from helpers import uniform_configs
from test_gpu_models import random_model

pytestmark = pytest.mark.gpu

E_ARG = -1  # MJPL_E_ARG
E_PAIRTYPE = -3  # MJPL_E_PAIRTYPE
TOL = 1e-9
INF = float("inf")
ALLOWED = (("link5", "hand"), ("link0", "link6"), ("world", "left_finger"))


def quat(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def pair_model(static, moving, axis=(1, 0, 0)):
    """One static geom and one geom on a body with a slide joint (q = 0: the body at the origin)."""
    mb = ModelBuilder()
    mb.add_body("m")
    mb.add_joint("m", "j", type="slide", axis=axis, range=(-2, 2))
    mb.add_geom("world", **static)
    mb.add_geom("m", **moving)
    return mb.compile()


def g(type, size, pos=(0, 0, 0), q=(1, 0, 0, 0)):
    return dict(type=type, size=size, pos=pos, quat=q)


R2 = np.sqrt(2)
# (label, static geom, moving geom, slide axis, q, distance)
KNOWN = [
    ("sphere-sphere gap", g("sphere", (0.1,)), g("sphere", (0.2,), (0.5, 0, 0)), (1, 0, 0), 0.0, 0.2),
    ("sphere-sphere overlap", g("sphere", (0.1,)), g("sphere", (0.2,), (0.5, 0, 0)), (1, 0, 0), -0.25, -0.05),
    ("sphere above plane", g("plane", (1, 1, 0.1)), g("sphere", (0.1,), (0.3, -0.2, 0.3)), (0, 0, 1), 0.0, 0.2),
    ("box resting on plane", g("plane", (1, 1, 0.1)), g("box", (0.1, 0.2, 0.3), (0.2, 0.1, 0.5), quat((1, 0, 0), 0.3)),
     (0, 0, 1), 0.0, 0.5 - 0.2 * np.sin(0.3) - 0.3 * np.cos(0.3)),
    ("boxes face to face", g("box", (0.1, 0.2, 0.3)), g("box", (0.15, 0.1, 0.1), (0.3, 0.05, -0.02)), (1, 0, 0), 0.0,
     0.3 - 0.25),
    ("boxes edge to edge, crossed", g("box", (0.5, 0.1, 0.1), q=quat((1, 0, 0), np.pi / 4)),
     g("box", (0.1, 0.5, 0.1), (0, 0, 0.5), quat((0, 1, 0), np.pi / 4)), (0, 0, 1), 0.0, 0.5 - 0.2 * R2),
    ("boxes overlapping", g("box", (0.2, 0.2, 0.2)), g("box", (0.2, 0.2, 0.2), (0.35, 0.01, -0.02)), (1, 0, 0), 0.0,
     -0.05),
    ("sphere centre inside box", g("box", (0.3, 0.2, 0.1)), g("sphere", (0.05,), (0.1, 0, 0.02)), (1, 0, 0), 0.0,
     -0.13),
    ("capsules parallel", g("capsule", (0.05, 0.2)), g("capsule", (0.05, 0.2), (0, 0.3, 0.1)), (1, 0, 0), 0.0, 0.2),
    ("capsules crossing", g("capsule", (0.05, 0.3), q=quat((0, 1, 0), np.pi / 2)),
     g("capsule", (0.05, 0.3), (0.1, -0.05, 0.25), quat((1, 0, 0), np.pi / 2)), (1, 0, 0), 0.0, 0.15),
    ("capsule through box", g("box", (0.3, 0.2, 0.1)),
     g("capsule", (0.02, 1.0), (0, 0.15, 0), quat((0, 1, 0), np.pi / 2)), (0, 0, 1), 0.0, -0.07),
]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c[0])
def test_known_answers(case):
    label, static, moving, axis, q, want = case
    m = pair_model(static, moving, axis)
    e = eng_mod.Engine(m)
    assert len(e.contact_pairs()[0]) == 1
    D = e.distances(np.array([[q]]))
    assert D.shape == (1, 1)
    assert abs(D[0, 0] - want) <= 1e-12, (label, D[0, 0], want)
    # the reference says the same, and clearance is the one pair's distance
    R = ref.reference_distances(m, np.array([[q]]), e.contact_pairs()[0])
    assert abs(R[0, 0] - want) <= 1e-12
    C, pair = e.clearance(np.array([[q]]))
    assert C[0] == D[0, 0] and pair[0] == 0


# ---- the benchmark scene
@pytest.fixture(scope="module")
def franka():
    m = scenes.franka_p(obstacles=True)
    Q = uniform_configs(m, 65536, seed=21)
    return m, Q


def _check_reference(m, Q, D, pairs, label):
    R = ref.reference_distances(m, Q, pairs)
    err = np.abs(D - R)
    worst = np.unravel_index(np.argmax(err), err.shape) if err.size else None
    assert err.size == 0 or err.max() <= TOL, \
        f"{label}: |D - reference| = {err.max():.3e} at configuration {worst[0]}, pair {pairs[worst[1]].tolist()}"


def _check_contacts(e, m, Q, D, pairs, allowed_flags, label):
    """contact bit <=> D <= margin (boxes against boxes with a margin: only D <= margin => contact)."""
    hits = contact_hits(e.contacts(Q), len(pairs))
    marg = ref.pair_margins(m, pairs)
    gt = np.asarray(m.geom_type)
    boxbox = (gt[pairs[:, 0]] == ref.BOX) & (gt[pairs[:, 1]] == ref.BOX) & (marg > 0)
    S = D - marg
    clear_cut = np.abs(S) > TOL
    touch = S <= 0
    exact = clear_cut & ~boxbox[None, :]
    assert np.array_equal(hits[exact], touch[exact]), f"{label}: contact bits disagree with D <= margin"
    assert np.all(hits[touch & clear_cut]), f"{label}: D <= margin without a contact"


def _check_clearance(c, Q, D, pairs, allowed_flags, margins, label):
    C, pair = c.clearance_batch(Q)
    want_C, want_pair = ref.clearance_from(D, margins, allowed_flags)
    if want_C is None:
        assert np.all(pair == -1) and np.all(C == INF)
        return
    assert C.tobytes() == want_C.tobytes(), f"{label}: clearance is not the min of D - margin"
    np.testing.assert_array_equal(pair, want_pair)
    valid = c.valid_configs(Q)
    away = np.abs(C) > TOL
    m = c.model
    gt = np.asarray(m.geom_type)
    conservative = (gt[pairs[:, 0]] == ref.BOX) & (gt[pairs[:, 1]] == ref.BOX) & (margins > 0) & ~allowed_flags
    if conservative.any():  # the check's box-box test with a margin may call a pair farther than it touching
        assert not np.any(valid & away & (C < 0)), f"{label}: a valid configuration with C < 0"
    else:
        assert np.array_equal((C > 0)[away], valid[away]), f"{label}: C > 0 disagrees with valid_configs"


@pytest.mark.parametrize("allowed", [(), ALLOWED], ids=["no allowed pairs", "allowed pairs"])
def test_franka_obstacles_64k(franka, allowed):
    m, Q = franka
    c = CollisionConstraint(m, list(allowed))
    e = c.engine
    pairs, flags = e.contact_pairs()
    assert bool(np.any(flags)) == bool(allowed)
    D = c.distances_batch(Q)
    assert D.shape == (len(Q), len(pairs)) and np.all(np.isfinite(D))
    idx = np.random.default_rng(5).choice(len(Q), 4096, replace=False)
    _check_reference(m, Q[idx], D[idx], pairs, "franka_p+16obs")
    assert np.mean(D < 0) > 0  # overlapping and disjoint pairs both occur
    _check_contacts(e, m, Q, D, pairs, flags, "franka_p+16obs")
    margins = ref.pair_margins(m, pairs)
    _check_clearance(c, Q, D, pairs, flags, margins, "franka_p+16obs")
    valid = c.valid_configs(Q)
    assert 0.05 < valid.mean() < 0.95


def test_clearance_is_the_min_of_distances_with_distmax(franka):
    m, Q = franka
    c = CollisionConstraint(m, list(ALLOWED))
    pairs, flags = c.engine.contact_pairs()
    margins = ref.pair_margins(m, pairs)
    for distmax in (0.05, 0.3, INF):
        D = c.distances_batch(Q, distmax)
        C, pair = c.clearance_batch(Q, distmax)
        want_C, want_pair = ref.clearance_from(D, margins, flags)
        assert C.tobytes() == want_C.tobytes(), distmax
        np.testing.assert_array_equal(pair, want_pair)


def test_distmax(franka):
    m, Q = franka
    Q = Q[:16384]
    e = eng_mod.Engine(m)
    Dinf = e.distances(Q)
    for distmax in (0.02, 0.05, 0.4):
        D = e.distances(Q, distmax)
        below = Dinf < distmax
        assert 0 < below.mean() < 1
        assert np.all(D[~below] == distmax)
        assert D[below].tobytes() == Dinf[below].tobytes()
        C, pair = e.clearance(Q, distmax)
        Cinf, pinf = e.clearance(Q)
        low = Cinf < distmax  # (franka's margins are 0)
        assert C[low].tobytes() == Cinf[low].tobytes()
        np.testing.assert_array_equal(pair[low], pinf[low])
        assert np.all(C[~low] == distmax)
    q = np.ascontiguousarray(Q[:4])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(eng_mod.MjplError) as ei:
            e.distances(q, bad)
        assert ei.value.code == E_ARG
        with pytest.raises(eng_mod.MjplError) as ei:
            e.clearance(q, bad)
        assert ei.value.code == E_ARG


def test_argument_errors():
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    lib, h = e.lib, e.h
    F64, I32 = eng_mod._F64P, eng_mod._I32P
    q = np.zeros((1, m.nq))
    P = len(e.contact_pairs()[0])
    out = np.zeros((1, P))
    cl, pr = np.zeros(1), np.zeros(1, np.int32)
    assert lib.mjpl_distances(h, q.ctypes.data_as(F64), 1, 1, INF, None) == E_ARG
    assert lib.mjpl_distances(h, q.ctypes.data_as(F64), 1, 7, INF, out.ctypes.data_as(F64)) == E_ARG
    assert lib.mjpl_distances(h, q.ctypes.data_as(F64), -1, 1, INF, out.ctypes.data_as(F64)) == E_ARG
    assert lib.mjpl_distances_dev(h, None, 1, 1, INF, None) == E_ARG
    assert lib.mjpl_clearance(h, q.ctypes.data_as(F64), 1, 1, INF, cl.ctypes.data_as(F64), None) == E_ARG
    assert lib.mjpl_clearance(h, q.ctypes.data_as(F64), 1, 1, INF, None, pr.ctypes.data_as(I32)) == E_ARG
    assert lib.mjpl_clearance_dev(h, None, 1, 1, INF, None, None) == E_ARG
    assert lib.mjpl_distances(h, q.ctypes.data_as(F64), 0, 1, INF, None) == 0
    assert lib.mjpl_clearance(h, q.ctypes.data_as(F64), 0, 1, INF, None, None) == 0


def no_pair_model():
    """Two spheres whose contype / conaffinity never meet: an empty candidate table (P = 0)."""
    mb = ModelBuilder()
    mb.add_body("a")
    mb.add_joint("a", "ja", range=(-1, 1))
    mb.add_geom("a", "sphere", (0.1,), contype=1, conaffinity=0)
    mb.add_geom("world", "sphere", (0.1,), contype=1, conaffinity=0)
    return mb.compile()


def test_empty_candidate_table():
    e = eng_mod.Engine(no_pair_model())
    assert e.contact_pairs()[0].shape == (0, 2)
    Q = np.linspace(-1, 1, 5)[:, None]
    assert e.distances(Q).shape == (5, 0)
    for distmax in (INF, 0.05):
        C, pair = e.clearance(Q, distmax)
        assert np.all(C == distmax) and np.all(pair == -1)


def test_unsupported_pair_type_is_refused_by_every_query():
    # a cylinder (no routine here) that only meets an allowed body: the engine creates, every pair query refuses
    mb = ModelBuilder()
    mb.add_body("m")
    mb.add_joint("m", "j", type="slide", axis=(1, 0, 0), range=(-2, 2))
    mb.add_geom("world", type="cylinder", size=(0.1, 0.2))
    mb.add_geom("m", type="sphere", size=(0.1,), pos=(0.5, 0, 0))
    e = eng_mod.Engine(mb.compile(), [("world", "m")])
    assert e.contact_pairs()[0].shape == (1, 2) and e.contact_pairs()[1].all()
    Q = np.zeros((3, 1))
    for query in (e.contacts, e.distances, e.clearance, e.clearance_grad):
        with pytest.raises(eng_mod.MjplError) as ei:
            query(Q)
        assert ei.value.code == E_PAIRTYPE, query.__name__


# ---- other models
def _other_cases():
    cases = [("franka_p+16obs+10 pads (moving boxes)", scenes.franka_p(obstacles=True, pads=True), (), 1024),
             ("ur5e_c", scenes.ur5e(), (), 2048)]
    for seed in range(50):
        model, allowed = random_model(seed, moving_boxes=seed % 2 == 0)
        cases.append((f"random_model({seed}, moving_boxes={seed % 2 == 0})", model, tuple(allowed), 256))
    return cases


@pytest.mark.parametrize("case", _other_cases(), ids=lambda c: c[0])
def test_models_equal_reference(case):
    label, m, allowed, n = case
    c = CollisionConstraint(m, list(allowed))
    e = c.engine
    pairs, flags = e.contact_pairs()
    Q = uniform_configs(m, n, seed=301)
    Q[::97] = m.qpos0
    D = c.distances_batch(Q)
    assert D.shape == (n, len(pairs))
    _check_reference(m, Q, D, pairs, label)
    _check_contacts(e, m, Q, D, pairs, flags, label)
    margins = ref.pair_margins(m, pairs)
    _check_clearance(c, Q, D, pairs, flags, margins, label)
    if "pads" in label:
        gt = np.asarray(m.geom_type)
        boxbox = (gt[pairs[:, 0]] == ref.BOX) & (gt[pairs[:, 1]] == ref.BOX)
        assert boxbox.any() and np.any(D[:, boxbox] < 1.0)


# ---- entry-point forms
def _host_dev(e, Q, n, layout, distmax=INF):
    P = len(e.contact_pairs()[0])
    host = e.distances(Q, distmax, layout=layout)
    hc, hp = e.clearance(Q, distmax, layout=layout)
    dQ = e.alloc(max(Q.nbytes, 8)).upload(Q)
    dd = e.alloc(max(n * P * 8, 8))
    dc, dp = e.alloc(max(n * 8, 8)), e.alloc(max(n * 4, 8))
    e.distances_dev(dQ.ptr, n, layout, dd.ptr, distmax)
    e.clearance_dev(dQ.ptr, n, layout, dc.ptr, dp.ptr, distmax)
    dev = dd.download(np.float64, n * P).reshape(n, P)
    devc, devp = dc.download(np.float64, n), dp.download(np.int32, n)
    for b in (dQ, dd, dc, dp):
        b.free()
    assert host.shape == (n, P)
    assert dev.tobytes() == host.tobytes()
    assert devc.tobytes() == hc.tobytes() and devp.tobytes() == hp.tobytes()
    return host, hc, hp


@pytest.mark.parametrize("n", [0, 1, 63, 65, 100003])
def test_device_and_host_entry_points_agree(n):
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    Q = uniform_configs(m, n, seed=23 + n)
    aos = _host_dev(e, Q, n, eng_mod.AOS)
    soa = _host_dev(e, np.ascontiguousarray(Q.T), n, eng_mod.SOA)
    for a, b in zip(aos, soa):
        assert a.tobytes() == b.tobytes()
    if n == 100003:  # across the 2^16-row chunk: the rows of the second launch equal a launch of their own
        tail = e.distances(Q[65536:65536 + 1000])
        assert tail.tobytes() == aos[0][65536:65536 + 1000].tobytes()


def test_after_set_planning_and_fresh_engine():
    m = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS)
    base = m.keyframe("home").qpos.copy()
    e = eng_mod.Engine(m)
    full = uniform_configs(m, 4096, seed=24)
    held = np.setdiff1d(np.arange(m.nq), arm)
    full[:, held] = base[held]
    want = e.distances(full)
    wc, wp = e.clearance(full)
    e.distances(full[:100], 0.1)  # (a launch in between, other distmax)
    e.set_planning(arm, base)
    Qp = np.ascontiguousarray(full[:, arm])
    got, gc, gp = _host_dev(e, Qp, len(Qp), eng_mod.AOS)
    assert got.tobytes() == want.tobytes()
    assert gc.tobytes() == wc.tobytes() and gp.tobytes() == wp.tobytes()
    # a fresh engine made directly in the same state
    f = eng_mod.Engine(m)
    f.set_planning(arm, base)
    assert f.distances(Qp).tobytes() == got.tobytes()
    fc, fp = f.clearance(Qp)
    assert fc.tobytes() == gc.tobytes() and fp.tobytes() == gp.tobytes()
    # another base pose: the held joints move the geoms, and the live engine follows
    base2 = base.copy()
    base2[held] = 0.01
    e.set_planning(arm, base2)
    f2 = eng_mod.Engine(m)
    f2.set_planning(arm, base2)
    got2, gc2, gp2 = _host_dev(e, Qp, len(Qp), eng_mod.AOS)
    assert f2.distances(Qp).tobytes() == got2.tobytes()
    assert f2.clearance(Qp)[0].tobytes() == gc2.tobytes()
    full2 = full.copy()
    full2[:, held] = base2[held]
    assert CollisionConstraint(m).distances_batch(full2).tobytes() == got2.tobytes()


def test_non_finite_rows():
    m = scenes.franka_p(obstacles=True)
    c = CollisionConstraint(m)
    Q = uniform_configs(m, 300, seed=25)
    clean_D = c.distances_batch(Q)
    clean_C, clean_p = c.clearance_batch(Q)
    bad = [3, 64, 65, 299]
    Qb = Q.copy()
    Qb[3, 0] = np.nan
    Qb[64, 6] = np.inf
    Qb[65, 2] = -np.inf
    Qb[299, 8] = np.nan  # (a finger column: a planning column all the same)
    for distmax in (INF, 0.05):
        D = c.distances_batch(Qb, distmax)
        C, p = c.clearance_batch(Qb, distmax)
        assert np.all(np.isnan(D[bad])) and np.all(np.isnan(C[bad])) and np.all(p[bad] == -1)
        keep = np.setdiff1d(np.arange(len(Q)), bad)
        if distmax == INF:
            assert D[keep].tobytes() == clean_D[keep].tobytes()
            assert C[keep].tobytes() == clean_C[keep].tobytes()
            np.testing.assert_array_equal(p[keep], clean_p[keep])
        else:
            assert np.all(np.isfinite(D[keep]))


def test_constraint_surface():
    m = scenes.franka_p(obstacles=True)
    c = CollisionConstraint(m)
    pairs, _ = c.engine.contact_pairs()
    Q = uniform_configs(m, 64, seed=26)
    D = c.distances_batch(Q)
    C, p = c.clearance_batch(Q)
    for i in range(8):
        np.testing.assert_array_equal(c.pair_distances(Q[i]), D[i])
        ci, gpair = c.clearance(Q[i])
        assert ci == C[i] and gpair == tuple(int(x) for x in pairs[p[i]])
        assert (ci > 0) == c.valid_config(Q[i])
    # no candidate pair: clearance is distmax and no pair
    mb = ModelBuilder()
    mb.add_body("a")
    mb.add_joint("a", "ja", range=(-1, 1))
    mb.add_geom("a", "sphere", (0.1,), contype=1, conaffinity=0)
    mb.add_geom("world", "sphere", (0.1,), contype=1, conaffinity=0)
    m0 = mb.compile()
    c0 = CollisionConstraint(m0)
    assert c0.distances_batch(np.zeros((5, 1))).shape == (5, 0)
    assert c0.clearance(np.zeros(1)) == (INF, None)
    assert c0.clearance(np.zeros(1), distmax=0.5) == (0.5, None)
