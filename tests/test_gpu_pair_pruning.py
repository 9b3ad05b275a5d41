"""Pair pruning on the GPU (option "prune_pairs"): the program without the pairs proved out of reach
decides what the full program decides -- verdicts, first-bad indices and the filter's own counters, since neither cull
of a dropped pair could have passed -- on the benchmark model, for the interpreting kernels and the generated library,
inside the joint ranges and at angles up to +-6.5 rad, and the contact table keeps every candidate pair."""
import numpy as np
import pytest

from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes
from mjpl_amd.constraint.collision_constraint import contact_hits
from oracle import pyoracle

pytestmark = pytest.mark.gpu

EPS, STEP = 0.05, 0.01
ONE_ROUND, TWO_ROUND, NCONFIG, NWIDE, NCONTACT = 2048, 36864, 8192, 4096, 1024


def make_edges(model, qidx, n, seed):
    """As bench.py draws them: q_a uniform in the joint ranges, q_b = q_a + EPS * unit direction, clipped."""
    rng = np.random.default_rng(seed)
    lo, hi = model.jnt_range[qidx, 0], model.jnt_range[qidx, 1]
    qa = rng.uniform(lo, hi, size=(n, len(qidx)))
    d = rng.normal(size=qa.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return qa, np.clip(qa + EPS * d, lo, hi)


class Bench:
    """The benchmark model, its batches and the oracle's answers: made once, shared, never written to."""

    def __init__(self):
        self.model = scenes.franka_p(obstacles=True)
        self.qidx = scenes.planning_index(self.model, scenes.FRANKA_ARM_JOINTS)
        self.base = self.model.keyframe("home").qpos.copy()
        self.orc = pyoracle.Oracle(self.model, planning_qidx=self.qidx, qpos_base=self.base)
        self.edges, self.edge_want = {}, {}
        for n, seed in ((ONE_ROUND, 11), (TWO_ROUND, 12)):
            self.edges[n] = make_edges(self.model, self.qidx, n, seed)
            valid, first_bad, _ = self.orc.valid_edges(*self.edges[n], STEP, nthreads=8, info=True)
            self.edge_want[n] = (valid, first_bad)
        # ... and as many edges the oracle finds VALID, drawn the same way: on these every waypoint is checked, so the count
        # of undecided pairs is the same from launch to launch (behind an edge's first bad waypoint it depends on the
        # order the waves take waypoints in: tests/test_gpu_spec.py)
        self.valid_edges = {}
        for n, seed in ((ONE_ROUND, 21), (TWO_ROUND, 22)):
            qa, qb = make_edges(self.model, self.qidx, 3 * n, seed)
            keep = np.flatnonzero(self.orc.valid_edges(qa, qb, STEP, nthreads=8))[:n]
            assert len(keep) == n
            self.valid_edges[n] = (np.ascontiguousarray(qa[keep]), np.ascontiguousarray(qb[keep]))
        rng = np.random.default_rng(13)
        lo, hi = self.model.jnt_range[self.qidx, 0], self.model.jnt_range[self.qidx, 1]
        self.configs = rng.uniform(lo, hi, size=(NCONFIG, len(self.qidx)))
        self.configs_want = self.orc.valid_configs(self.configs, nthreads=8)
        self.wide = rng.uniform(-6.5, 6.5, size=(NWIDE, len(self.qidx)))
        self.wide_want = self.orc.valid_configs(self.wide, nthreads=8)
        for a in (*self.edges[ONE_ROUND], *self.edges[TWO_ROUND], *self.valid_edges[ONE_ROUND], *self.valid_edges[TWO_ROUND], self.configs, self.wide):
            a.setflags(write=False)

    def engine(self, prune, spec):
        e = eng_mod.Engine(self.model, options={"prune_pairs": prune, "spec": spec})
        e.set_planning(self.qidx, self.base)
        assert e.get_option("prune_pairs") == prune
        assert (e.get_option("pairs_pruned") > 0) == bool(prune)
        assert e.spec_loaded() == bool(spec), "the benchmark model's library of this program was not found"
        return e


@pytest.fixture(scope="module")
def bench():
    return Bench()


def _run_edges(e, qa, qb):
    valid, first_bad = e.check_edges(qa, qb, STEP, first_bad=True)
    return valid, first_bad, e.last_undecided(), e.last_items(), e.last_interior_edges()


def _assert_oracle(got_valid, got_first_bad, want, label):
    valid, first_bad = want
    np.testing.assert_array_equal(got_valid, valid, err_msg=label)
    bad = valid == 0
    np.testing.assert_array_equal(got_first_bad[bad], first_bad[bad], err_msg=label)


@pytest.mark.parametrize("n", [ONE_ROUND, TWO_ROUND])
def test_interpreting_kernels_decide_the_same_with_and_without(bench, n):
    qa, qb = bench.edges[n]
    on, off = bench.engine(1, 0), bench.engine(0, 0)
    assert on.info()["npairs"] == off.info()["npairs"] and on.info()["npairs_world"] == off.info()["npairs_world"]
    assert off.get_option("pairs_pruned") == 0 and on.get_option("pairs_pruned") >= 59
    got_on, got_off = _run_edges(on, qa, qb), _run_edges(off, qa, qb)
    np.testing.assert_array_equal(got_on[0], got_off[0])
    np.testing.assert_array_equal(got_on[1], got_off[1])
    assert got_on[3:] == got_off[3:], "items, interior edges"
    _assert_oracle(got_on[0], got_on[1], bench.edge_want[n], "interpreter, pruned")
    _assert_oracle(got_off[0], got_off[1], bench.edge_want[n], "interpreter, full")
    # ... and with the self pairs pruned as well (level 2 of the option)
    both = bench.engine(2, 0)
    assert both.get_option("pairs_pruned") > on.get_option("pairs_pruned")
    got_both = _run_edges(both, qa, qb)
    np.testing.assert_array_equal(got_both[0], got_off[0])
    np.testing.assert_array_equal(got_both[1], got_off[1])
    assert got_both[3:] == got_off[3:]
    # the undecided pairs, counted where the count does not depend on the order of the waves: n valid edges
    va, vb = bench.valid_edges[n]
    counts = [_run_edges(e, va, vb) for e in (on, off, both)]
    for c in counts:
        assert c[0].all()
    print("undecided, items, interior edges on valid edges (pruned, full, self pairs too):", [c[2:] for c in counts])
    assert counts[0][2:] == counts[1][2:] == counts[2][2:]


def test_interpreting_kernels_decide_the_same_configurations(bench):
    on, off, both = bench.engine(1, 0), bench.engine(0, 0), bench.engine(2, 0)
    got_on, got_off = on.check_configs(bench.configs), off.check_configs(bench.configs)
    und_on, und_off = on.last_undecided(), off.last_undecided()
    np.testing.assert_array_equal(got_on, got_off)
    assert und_on == und_off
    np.testing.assert_array_equal(both.check_configs(bench.configs), got_off)
    assert both.last_undecided() == und_off
    np.testing.assert_array_equal(got_on, bench.configs_want)


@pytest.mark.parametrize("n", [ONE_ROUND, TWO_ROUND])
def test_generated_library_of_the_pruned_program(bench, n):
    qa, qb = bench.edges[n]
    lib, interp = bench.engine(1, 1), bench.engine(0, 0)
    got_lib, got_int = _run_edges(lib, qa, qb), _run_edges(interp, qa, qb)
    np.testing.assert_array_equal(got_lib[0], got_int[0])
    np.testing.assert_array_equal(got_lib[1], got_int[1])
    _assert_oracle(got_lib[0], got_lib[1], bench.edge_want[n], "generated library, pruned")
    _assert_oracle(got_int[0], got_int[1], bench.edge_want[n], "interpreter, full")
    np.testing.assert_array_equal(lib.check_configs(bench.configs), bench.configs_want)


@pytest.mark.parametrize("spec", [0, 1], ids=["interpreter", "library"])
def test_configurations_outside_the_joint_ranges(bench, spec):
    for prune in ((2, 1, 0) if spec == 0 else (1,)):
        e = bench.engine(prune, spec)
        np.testing.assert_array_equal(e.check_configs(bench.wide), bench.wide_want, err_msg=f"prune_pairs={prune}")
    assert 0 < int(bench.wide_want.sum()) < NWIDE


def test_contact_table_keeps_every_pair(bench):
    on, off = bench.engine(1, 1), bench.engine(0, 0)
    pairs_on, allowed_on = on.contact_pairs()
    pairs_off, allowed_off = off.contact_pairs()
    np.testing.assert_array_equal(pairs_on, pairs_off)
    np.testing.assert_array_equal(allowed_on, allowed_off)
    assert len(pairs_on) == on.info()["npairs"]  # (nothing is allowed in this model: candidates = enabled pairs)
    Qp = bench.configs[:NCONTACT]  # (planning columns: the engines' contacts take what their checks take)
    full = pyoracle.Oracle(bench.model)
    hits = contact_hits(on.contacts(Qp), len(pairs_on))
    np.testing.assert_array_equal(hits, contact_hits(off.contacts(Qp), len(pairs_off)))
    valid = on.check_configs(Qp)
    for i in range(NCONTACT):
        assert full.obeys_ruleset(pairs_on[hits[i]].reshape(-1, 2)) == bool(valid[i]), i
    np.testing.assert_array_equal(valid, bench.configs_want[:NCONTACT])
