"""Per-pair contacts on the GPU (include/mjpl_hip.h: mjpl_contact_pairs / mjpl_contacts*; CollisionConstraint.contacts):
the candidate table against the model's own tables, and the contact list of every configuration against the CPU
oracle's ``orc_collision`` row for row, order included -- every narrowphase routine on every pair, not only the AND
over pairs that the verdict tests compare."""
import numpy as np
import pytest

from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes
from mjpl_amd.constraint import CollisionConstraint, CollisionRuleset
from mjpl_amd.constraint.collision_constraint import contact_csr
from helpers import uniform_configs
from spec_models import spec_models
from test_gpu_models import random_model

pytestmark = pytest.mark.gpu

GEOM_PLANE, GEOM_HFIELD = 0, 1
E_ARG = -1  # MJPL_E_ARG


def candidate_table(model, allowed=()):
    """The candidates of mj_collision restated from the model's tables (oracle/mjpl_oracle.c: orc_collision walks
    g1 < g2, skips what pair_filtered or has_collision_fn reject, writes rows smaller geom type first)."""
    bid, weld, parent = (np.asarray(a) for a in (model.geom_bodyid, model.body_weldid, model.body_parentid))
    ct, ca, gt = (np.asarray(a) for a in (model.geom_contype, model.geom_conaffinity, model.geom_type))
    allowed_ids = {tuple(sorted((model.body(a).id, model.body(b).id))) for a, b in allowed}
    pairs, flags = [], []
    for g1 in range(model.ngeom):
        for g2 in range(g1 + 1, model.ngeom):
            if not (ct[g1] & ca[g2]) and not (ct[g2] & ca[g1]):
                continue
            w1, w2 = weld[bid[g1]], weld[bid[g2]]
            if w1 == w2:
                continue
            if w1 != 0 and w2 != 0 and (w1 == weld[parent[w2]] or w2 == weld[parent[w1]]):
                continue
            t1, t2 = sorted((gt[g1], gt[g2]))
            if t1 == GEOM_PLANE and t2 in (GEOM_PLANE, GEOM_HFIELD):
                continue
            pairs.append((g2, g1) if gt[g1] > gt[g2] else (g1, g2))
            flags.append(tuple(sorted((int(bid[g1]), int(bid[g2])))) in allowed_ids)
    return np.array(pairs, np.int32).reshape(-1, 2), np.array(flags, bool)


def oracle_csr(orc, Q):
    rows = [orc.contacts(q) for q in Q]
    offsets = np.zeros(len(Q) + 1, np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return offsets, (np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 2), np.int32))


def assert_same_contacts(model, Q, got, want, label=""):
    """CSR equality; on a mismatch the configuration, the pair and both geoms' world poses go into the message."""
    (go, gp), (wo, wp) = got, want
    if np.array_equal(go, wo) and np.array_equal(gp, wp):
        return
    for i in range(len(Q)):
        a, b = gp[go[i]:go[i + 1]], wp[wo[i]:wo[i + 1]]
        if not np.array_equal(a, b):
            sa, sb = {tuple(r) for r in a.tolist()}, {tuple(r) for r in b.tolist()}
            from oracle import pyoracle
            k = pyoracle.Oracle(model).kinematics(Q[i])
            detail = [(p, k["geom_xpos"][list(p)].tolist(), k["geom_xmat"][list(p)].tolist())
                      for p in sorted(sa ^ sb)] or "order differs"
            pytest.fail(f"{label}: configuration {i} q={Q[i].tolist()}: gpu {a.tolist()} oracle {b.tolist()}; "
                        f"differing pairs with (geom_xpos, geom_xmat): {detail}")


def _models():
    out = [("franka_p+16obs", scenes.franka_p(obstacles=True), ()),
           ("franka_p+16obs, hand-fingers and link0-floor allowed", scenes.franka_p(obstacles=True),
            (("hand", "left_finger"), ("hand", "right_finger"), ("link0", "world"))),
           ("ur5e_c", scenes.ur5e(), ())]
    out += [(name, m, tuple(allowed)) for name, m, allowed, _, _ in spec_models()]
    return out


@pytest.mark.parametrize("case", _models(), ids=lambda c: c[0])
def test_candidate_table_matches_model_tables(case):
    _, model, allowed = case
    e = eng_mod.Engine(model, allowed)
    pairs, flags = e.contact_pairs()
    want_pairs, want_flags = candidate_table(model, allowed)
    np.testing.assert_array_equal(pairs, want_pairs)
    np.testing.assert_array_equal(flags, want_flags)
    assert e.contact_words() == (len(pairs) + 63) // 64
    # the table depends on the model alone
    e.set_planning(np.arange(model.nq - 1, dtype=np.int32), np.asarray(model.qpos0, float))
    p2, f2 = e.contact_pairs()
    np.testing.assert_array_equal(p2, pairs)
    np.testing.assert_array_equal(f2, flags)


def test_kat_two_dof_ball(oracle_mod):
    m = scenes.two_dof_ball()
    c = CollisionConstraint(m)
    orc = oracle_mod.Oracle(m)
    touching = c.contacts(np.array([0.6, 0.0]))
    assert len(touching) > 0
    np.testing.assert_array_equal(touching, orc.contacts(np.array([0.6, 0.0])))
    assert c.contacts(np.array([0.0, 0.0])).shape == (0, 2)
    assert c.colliding_bodies(np.array([0.0, 0.0])) == []
    assert len(c.colliding_bodies(np.array([0.6, 0.0]))) > 0


def test_franka_obstacles_64k_equal_oracle_row_for_row(oracle_mod):
    m = scenes.franka_p(obstacles=True)
    c = CollisionConstraint(m)
    orc = oracle_mod.Oracle(m)
    Q = uniform_configs(m, 65536, seed=11)
    got = c.contacts_batch(Q)
    want = oracle_csr(orc, Q)
    assert 0.05 < np.mean(np.diff(want[0]) == 0) < 0.95  # both free and touching configurations
    assert_same_contacts(m, Q, got, want, "franka_p+16obs")
    # capsule-box pairs are among the touching ones (the routine 80 of this scene's pairs go through)
    gt = np.asarray(m.geom_type)
    assert np.any((gt[got[1][:, 0]] == 3) & (gt[got[1][:, 1]] == 6))


def test_allowed_pairs_obey_ruleset_like_the_check(oracle_mod):
    m = scenes.franka_p(obstacles=True)
    # body pairs whose geoms are candidates and touch in a good share of uniform configurations (hand and fingers,
    # link0 and the world are no candidates at all: parent-child and same-weld filters)
    allowed = [("link5", "hand"), ("link0", "link6"), ("world", "left_finger")]
    c = CollisionConstraint(m, allowed)
    rs = CollisionRuleset(m, allowed)
    Q = uniform_configs(m, 65536, seed=12)
    offsets, rows = c.contacts_batch(Q)
    valid = c.valid_configs(Q)
    obeys = np.array([rs.obeys_ruleset(rows[offsets[i]:offsets[i + 1]]) for i in range(len(Q))])
    np.testing.assert_array_equal(obeys, valid)
    # allowed pairs stay in the list, as in MuJoCo's
    pairs, flags = c.engine.contact_pairs()
    allowed_rows = {tuple(p) for p in pairs[flags].tolist()}
    assert len(allowed_rows) > 0
    assert any(tuple(r) in allowed_rows for r in rows.tolist())
    # ... and the allowed pairs make configurations valid that the same batch without them has not
    assert valid.mean() > CollisionConstraint(m).valid_configs(Q).mean()
    for i in np.flatnonzero(~valid)[:64]:
        assert len(c.colliding_bodies(Q[i])) > 0
    for i in np.flatnonzero(valid)[:64]:
        assert c.colliding_bodies(Q[i]) == []


def _oracle_cases():
    cases = [("franka_p+16obs+10 pads (moving boxes)", scenes.franka_p(obstacles=True, pads=True), (), 8192),
             ("ur5e_c", scenes.ur5e(), (), 8192)]
    for seed in range(50):
        model, allowed = random_model(seed, moving_boxes=seed % 2 == 0)
        cases.append((f"random_model({seed}, moving_boxes={seed % 2 == 0})", model, tuple(allowed), 1024))
    return cases


@pytest.mark.parametrize("case", _oracle_cases(), ids=lambda c: c[0])
def test_models_equal_oracle(oracle_mod, case):
    label, model, allowed, n = case
    c = CollisionConstraint(model, list(allowed))
    orc = oracle_mod.Oracle(model, allowed)
    Q = uniform_configs(model, n, seed=300)
    Q[::97] = model.qpos0
    assert_same_contacts(model, Q, c.contacts_batch(Q), oracle_csr(orc, Q), label)
    # the verdict invariant on the same batch
    offsets, rows = c.contacts_batch(Q)
    valid = c.valid_configs(Q)
    obeys = np.array([c.cr.obeys_ruleset(rows[offsets[i]:offsets[i + 1]]) for i in range(len(Q))])
    np.testing.assert_array_equal(obeys, valid)


@pytest.mark.parametrize("n", [0, 1, 63, 65, 100003])
def test_device_and_host_entry_points_agree(n):
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    W = e.contact_words()
    Q = uniform_configs(m, n, seed=13 + n)
    host = e.contacts(Q)
    assert host.shape == (n, W) and host.dtype == np.uint64
    dQ = e.alloc(max(Q.nbytes, 8)).upload(Q)
    dbits = e.alloc(max(n * W * 8, 8))
    for layout, Qin in ((eng_mod.AOS, Q), (eng_mod.SOA, np.ascontiguousarray(Q.T))):
        if layout == eng_mod.SOA:
            dQ.upload(Qin)
            np.testing.assert_array_equal(e.contacts(Qin, layout=eng_mod.SOA), host)
        e.contacts_dev(dQ.ptr, n, layout, dbits.ptr)
        dev = dbits.download(np.uint64, n * W).reshape(n, W)
        assert dev.tobytes() == host.tobytes()
    dQ.free()
    dbits.free()


def test_planning_columns_after_set_planning(oracle_mod):
    m = scenes.franka_p(obstacles=True)
    arm = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS)
    base = m.keyframe("home").qpos.copy()
    e = eng_mod.Engine(m)
    pairs, _ = e.contact_pairs()
    full = uniform_configs(m, 4096, seed=14)
    held = np.setdiff1d(np.arange(m.nq), arm)
    full[:, held] = base[held]
    want = e.contacts(full)
    e.set_planning(arm, base)
    Qp = np.ascontiguousarray(full[:, arm])
    got = e.contacts(Qp)
    assert got.tobytes() == want.tobytes()
    dQ = e.alloc(Qp.nbytes).upload(Qp)
    dbits = e.alloc(got.nbytes)
    e.contacts_dev(dQ.ptr, len(Qp), eng_mod.AOS, dbits.ptr)
    assert dbits.download(np.uint64, got.size).tobytes() == got.tobytes()
    # and the rows are the oracle's
    orc = oracle_mod.Oracle(m)
    assert_same_contacts(m, full[:512], contact_csr(got[:512], pairs), oracle_csr(orc, full[:512]), "planning columns")
    dQ.free()
    dbits.free()


def test_argument_errors():
    m = scenes.franka_p(obstacles=True)
    e = eng_mod.Engine(m)
    lib, h = e.lib, e.h
    P = lib.mjpl_contact_pair_count(h)
    assert P == len(e.contact_pairs()[0]) > 64
    g = np.zeros(P, np.int32)
    a = np.zeros(P, np.uint8)
    I32 = eng_mod._I32P
    assert lib.mjpl_contact_pairs(h, g.ctypes.data_as(I32), g.ctypes.data_as(I32), a.ctypes.data_as(eng_mod._U8P),
                                  P - 1) == E_ARG
    q = np.zeros((1, m.nq))
    out = np.zeros((1, e.contact_words()), np.uint64)
    F64, U64 = eng_mod._F64P, eng_mod._U64P
    assert lib.mjpl_contacts(h, q.ctypes.data_as(F64), -1, 1, out.ctypes.data_as(U64)) == E_ARG
    assert lib.mjpl_contacts(h, q.ctypes.data_as(F64), 1, 7, out.ctypes.data_as(U64)) == E_ARG
    assert lib.mjpl_contacts(h, None, 1, 1, out.ctypes.data_as(U64)) == E_ARG
    assert lib.mjpl_contacts(h, q.ctypes.data_as(F64), 1, 1, None) == E_ARG
    assert lib.mjpl_contacts_dev(h, None, 1, 1, None) == E_ARG
    assert lib.mjpl_contacts(h, q.ctypes.data_as(F64), 0, 1, None) == 0


def test_no_candidate_pairs():
    from mjpl_amd.model import ModelBuilder
    mb = ModelBuilder()
    mb.add_body("a")
    mb.add_joint("a", "ja", range=(-1, 1))
    mb.add_geom("a", "sphere", (0.1,), contype=1, conaffinity=0)
    mb.add_geom("world", "sphere", (0.1,), contype=1, conaffinity=0)
    m = mb.compile()
    e = eng_mod.Engine(m)
    assert e.contact_pairs()[0].shape == (0, 2) and e.contact_words() == 0
    out = e.contacts(np.zeros((5, 1)))
    assert out.shape == (5, 0)
    c = CollisionConstraint(m)
    offsets, rows = c.contacts_batch(np.zeros((5, 1)))
    assert offsets.tolist() == [0] * 6 and rows.shape == (0, 2)
