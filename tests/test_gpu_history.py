"""History independence: an engine brought into a state by any sequence of calls must return exactly what a fresh
engine made directly in that state returns -- verdicts, first-bad indices, contact bits and the introspection getters
-- and the fresh engine must equal the float64 oracle on a sample.

Every other parity test builds a fresh engine for the state it tests.  A long-lived planner does not: it calls
set_planning again for every base pose or joint subset, flips set_spec / set_filter / set_option on a live engine, and
sends batches whose sizes cross the dispatch thresholds of launch_edges (fused_single_max, fused_cert_min_edges) and
grow the scratch buffers, which never shrink.  Each of those leaves state behind in mjpl_engine; this file checks it.

A small driver runs a list of steps on one engine.  After each launch it makes the reference engine from scratch with
the same effective state.  Options go in through Engine(options=...) and are read back with get_option, and no MJPL_*
variable of the caller's shell reaches either engine."""
import os

import numpy as np
import pytest

from mjpl_amd import engine as eng_mod
from mjpl_amd import scenes
from mjpl_amd.constraint.collision_constraint import contact_csr
from helpers import random_edges
from spec_models import generic_scenes
from test_gpu_contacts import assert_same_contacts, oracle_csr

pytestmark = pytest.mark.gpu

STEP = 0.01
SAMPLE = 20000          # rows of every launch compared with the oracle
CONTACT_SAMPLE = 1000   # ... of a contacts launch (the oracle walks those one configuration at a time)
# options that shape the compiled program: they take effect at the next compile (set_planning / set_spec / set_filter),
# the others at the next launch (the comment above kEngineOptions in mjpl_hip.hip)
COMPILE_TIME = {"force_immediate", "filter_tol"}


@pytest.fixture(autouse=True)
def _no_shell_options(monkeypatch):
    """Neither engine of a comparison may pick anything up from the caller: no MJPL_* variables, no default options,
    per-model libraries from their default directory."""
    for k in list(os.environ):
        if k.startswith("MJPL_"):
            monkeypatch.delenv(k)
    monkeypatch.setattr(eng_mod, "DEFAULT_OPTIONS", {})
    monkeypatch.setattr(eng_mod.Engine, "_spec_dir_from_env", None, raising=False)
    eng_mod.set_spec_dir(None)


def _franka():
    m = scenes.franka_p(obstacles=True)
    return m, scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS), m.keyframe("home").qpos.copy()


def _narrow(base):
    """The home keyframe with the fingers closed further (0.04 -> 0.01): same columns, another program."""
    b = base.copy()
    b[7] = 0.01
    return b


class Driver:
    """One live engine and the state a fresh engine would need to be in to match it."""

    def __init__(self, oracle_mod, m, qidx, base, allowed=(), options=None, spec=1, label=""):
        self.orc_mod, self.m, self.allowed, self.label = oracle_mod, m, tuple(allowed), label
        self.qidx, self.base = np.asarray(qidx, np.int32), np.asarray(base, float).copy()
        self.spec, self.opts = spec, dict(options or {})
        self.history = [f"Engine(options={self.opts}, spec={spec}) + set_planning({self.qidx.tolist()})"]
        self.e = self._fresh()
        self._batches, self._oracle = {}, {}
        self.prev_program = None  # (qidx, base) before the last set_planning that changed the base

    def close(self):
        self.e.close()

    # ---- engines
    def _fresh(self):
        opts = dict(self.opts)
        if self.spec == 0:
            opts["spec"] = 0
        e = eng_mod.Engine(self.m, self.allowed, options=opts)
        e.set_planning(self.qidx, self.base)
        if self.spec == 2:
            e.set_spec(2)
        self._assert_options(e, "fresh")
        return e

    def _assert_options(self, e, who):
        for k, v in self.opts.items():
            assert e.get_option(k) == pytest.approx(float(v), rel=1e-6), (who, k, e.get_option(k), v)

    # ---- steps
    def run(self, steps):
        for s in steps:
            getattr(self, s[0])(*s[1:])
        return self

    def planning(self, qidx, base):
        qidx, base = np.asarray(qidx, np.int32), np.asarray(base, float)
        self.prev_program = (self.qidx, self.base) if len(qidx) == len(self.qidx) and not np.array_equal(base, self.base) else None
        self.e.set_planning(qidx, base)
        self.qidx, self.base = qidx, base.copy()
        self.history.append(f"set_planning({qidx.tolist()}, base[7]={base[7] if len(base) > 7 else None})")

    def set_spec(self, k):
        self.e.set_spec(k)
        self.spec = k
        self.history.append(f"set_spec({k})")

    def set_filter(self, on, tol=None):
        if on:
            self.e.set_filter(True, tol)
            self.opts["filter_tol"] = tol
        else:
            self.e.set_filter(False)
        self.opts["filter"] = 1 if on else 0
        self.history.append(f"set_filter({on}, {tol})")

    def option(self, name, v):
        self.e.set_option(name, v)
        if name in COMPILE_TIME:
            self.e.set_planning(self.qidx, self.base)
        self.opts[name] = v
        self.history.append(f"set_option({name}, {v})" + (" + set_planning(same)" if name in COMPILE_TIME else ""))

    # ---- batches (one per planning set and size) and the oracle's answers (one per program and batch)
    def _edges(self, n):
        key = ("edges", tuple(self.qidx.tolist()), n)
        if key not in self._batches:
            self._batches[key] = random_edges(self.m, self.qidx, n, seed=1000 + n % 997)
        return self._batches[key]

    def _configs(self, n):
        key = ("configs", tuple(self.qidx.tolist()), n)
        if key not in self._batches:
            qa, _ = random_edges(self.m, self.qidx, n, seed=2000 + n % 997)
            self._batches[key] = qa
        return self._batches[key]

    def _oracle_edges(self, qidx, base, n):
        key = ("edges", tuple(qidx.tolist()), base.tobytes(), n)
        if key not in self._oracle:
            qa, qb = self._edges(n)
            k = min(n, SAMPLE)
            with self.orc_mod.portable_trig():
                orc = self.orc_mod.Oracle(self.m, self.allowed, planning_qidx=qidx, qpos_base=base)
                ov, ofb, _ = orc.valid_edges(qa[:k], qb[:k], STEP, nthreads=8, info=True)
            self._oracle[key] = (ov, ofb)
        return self._oracle[key]

    # ---- launches
    def _launch(self, e, kind, n, layout, interior_only, dev):
        flags = eng_mod.EDGE_INTERIOR_ONLY if interior_only else 0
        if kind == "edges":
            qa, qb = self._edges(n)
            if layout == eng_mod.SOA:
                qa, qb = np.ascontiguousarray(qa.T), np.ascontiguousarray(qb.T)
            if not dev:
                return e.check_edges(qa, qb, STEP, layout=layout, first_bad=True, interior_only=interior_only)
            dA, dB = e.alloc(max(qa.nbytes, 8)).upload(qa), e.alloc(max(qb.nbytes, 8)).upload(qb)
            dv, dfb = e.alloc(max(n, 8)), e.alloc(max(4 * n, 8))
            e.check_edges_dev(dA.ptr, dB.ptr, n, STEP, layout, dv.ptr, dfb.ptr, flags)
            out = (dv.download(np.uint8, n), dfb.download(np.int32, n))
            for b in (dA, dB, dv, dfb):
                b.free()
            return out
        Q = self._configs(n)
        if layout == eng_mod.SOA:
            Q = np.ascontiguousarray(Q.T)
        if kind == "configs":
            return (e.check_configs(Q, layout=layout),)
        assert kind == "contacts"
        if not dev:
            return (e.contacts(Q, layout=layout),)
        W = e.contact_words()
        dQ, dbits = e.alloc(max(Q.nbytes, 8)).upload(Q), e.alloc(max(8 * n * W, 8))
        e.contacts_dev(dQ.ptr, n, layout, dbits.ptr)
        out = (dbits.download(np.uint64, n * W).reshape(n, W),)
        dQ.free()
        dbits.free()
        return out

    def _meta(self, e, kind, counters=False):
        meta = {"spec_kind": e.spec_kind(), "spec_cert_loaded": e.get_option("spec_cert_loaded")}
        if kind == "edges":
            meta["certified"] = e.last_certified() > 0
        if counters:
            meta.update(last_items=e.last_items(), last_interior_edges=e.last_interior_edges(), info=e.info())
        return meta

    def long_edges(self, n):
        """A host-pointer launch of n edges, the first of them longer than 64 steps, against a fresh engine."""
        qa, qb = (x.copy() for x in self._edges(n))
        lo, hi = self.m.jnt_range[self.qidx, 0], self.m.jnt_range[self.qidx, 1]
        qa[0], qb[0] = lo + 0.1 * (hi - lo), lo + 0.9 * (hi - lo)
        assert np.linalg.norm(qb[0] - qa[0]) > 64 * STEP
        msg = f"{self.label}: long_edges({n}) after " + " -> ".join(self.history)
        got = self.e.check_edges(qa, qb, STEP, first_bad=True)
        ref = self._fresh()
        try:
            want = ref.check_edges(qa, qb, STEP, first_bad=True)
        finally:
            ref.close()
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x, y, err_msg=msg)
        self.history.append(f"long_edges({n})")

    def launch(self, kind, n, layout=eng_mod.AOS, interior_only=False, dev=False, expect=None, counters=False):
        """One launch on the live engine, then the same launch on a fresh engine, the other entry point (host or
        device pointers) on the live engine, and the oracle on a sample.  `expect`: getters asserted outright;
        `counters`: the item and interior-edge counters and mjpl_get_info are compared with the fresh engine's, too."""
        what = f"{kind}({n}, layout={layout}, interior_only={interior_only}, dev={dev})"
        msg = f"{self.label}: {what} after " + " -> ".join(self.history)
        got = self._launch(self.e, kind, n, layout, interior_only, dev)
        meta = self._meta(self.e, kind, counters)
        self._assert_options(self.e, "live")
        ref = self._fresh()
        try:
            want = self._launch(ref, kind, n, layout, interior_only, dev)
            ref_meta = self._meta(ref, kind, counters)
        finally:
            ref.close()
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x, y, err_msg=msg)
        assert meta == ref_meta, (msg, meta, ref_meta)
        for k, v in (expect or {}).items():
            assert meta[k] == v, (msg, k, meta[k], v)
        if kind in ("edges", "contacts"):  # the other entry point, on the same engine
            other = self._launch(self.e, kind, n, layout, interior_only, not dev)
            for x, y in zip(other, got):
                np.testing.assert_array_equal(x, y, err_msg="host vs device pointers: " + msg)
        self._check_oracle(kind, n, got, msg, interior_only)
        self.history.append(what)
        return got

    def _check_oracle(self, kind, n, got, msg, interior_only):
        if n == 0:
            return
        if kind == "edges":
            if interior_only:  # (endpoints are not looked at: the fresh engine is the reference of this launch)
                return
            ov, ofb = self._oracle_edges(self.qidx, self.base, n)
            k = len(ov)
            np.testing.assert_array_equal(got[0][:k], ov, err_msg="oracle: " + msg)
            np.testing.assert_array_equal(got[1][:k], ofb, err_msg="oracle first-bad: " + msg)
            if k >= 32:
                assert 0 < ov.mean() < 1, ("oracle verdicts all alike", msg)
            if self.prev_program is not None and n >= 32:  # a program change the batch can see
                pv, _ = self._oracle_edges(*self.prev_program, n)
                assert (pv != ov).any(), ("both programs give the same verdicts on this batch", msg)
            return
        Q = self._configs(n)
        k = min(n, SAMPLE if kind == "configs" else CONTACT_SAMPLE)
        with self.orc_mod.portable_trig():
            orc = self.orc_mod.Oracle(self.m, self.allowed, planning_qidx=self.qidx, qpos_base=self.base)
            if kind == "configs":
                ov = orc.valid_configs(Q[:k], nthreads=8)
                np.testing.assert_array_equal(got[0][:k], ov, err_msg="oracle: " + msg)
                if k >= 32:
                    assert 0 < ov.mean() < 1, ("oracle verdicts all alike", msg)
                return
            full = np.tile(self.base, (k, 1))
            full[:, self.qidx] = Q[:k]
            pairs, _ = self.e.contact_pairs()
            assert_same_contacts(self.m, full, contact_csr(got[0][:k], pairs), oracle_csr(orc, full), msg)
            rows = got[0][:k]
            assert rows.any() and len({r.tobytes() for r in rows}) > 1, ("contact rows all alike", msg)


def _cert_driver(oracle_mod, label):
    m, qidx, base = _franka()
    d = Driver(oracle_mod, m, qidx, base, options={"fused_cert_min_edges": 100000}, label=label)
    if not d.e.get_option("spec_cert_loaded"):
        d.close()
        pytest.skip("no certificate build beside the default library (python -c 'import __graft_entry__ as g; g.build()')")
    return d, qidx, base


def test_certificate_after_spec_toggles(oracle_mod):
    """(a) set_spec(0) must drop the certificate build with the default library: a big batch after it runs the
    interpreter and certifies nothing; set_spec(1) brings both back, set_spec(2) leaves the certificate out."""
    d, _, _ = _cert_driver(oracle_mod, "certificate after spec toggles")
    on = {"spec_kind": 1, "spec_cert_loaded": 1, "certified": True}
    d.run([("launch", "edges", 150000, eng_mod.AOS, False, False, on),
           ("set_spec", 0),
           ("launch", "edges", 150000, eng_mod.AOS, False, False, {"spec_kind": 0, "spec_cert_loaded": 0, "certified": False}),
           ("set_spec", 1),
           ("launch", "edges", 150000, eng_mod.AOS, False, False, on),
           ("set_spec", 2),
           ("launch", "edges", 150000, eng_mod.AOS, False, True, {"spec_cert_loaded": 0, "certified": False}),
           ("set_spec", 1),
           ("launch", "edges", 150000, eng_mod.AOS, False, True, on)])
    d.close()


def test_no_stale_library_on_a_new_program(oracle_mod):
    """(b) With spec off, set_planning to another base pose (same columns, other float64 constants) must not keep the
    old program's certificate build: a big batch equals a fresh engine for the new program and the oracle.  Back on
    the home program with spec on, its own library and certificate are loaded again."""
    d, qidx, base = _cert_driver(oracle_mod, "stale library on a new program")
    d.run([("launch", "edges", 150000),
           ("set_spec", 0),
           ("planning", qidx, _narrow(base)),
           ("launch", "edges", 150000, eng_mod.AOS, False, False, {"spec_kind": 0, "spec_cert_loaded": 0, "certified": False}),
           ("launch", "edges", 150000, eng_mod.AOS, False, True),
           ("planning", qidx, base),
           ("set_spec", 1),
           ("launch", "edges", 150000, eng_mod.AOS, False, False, {"spec_kind": 1, "spec_cert_loaded": 1, "certified": True})])
    d.close()


SIZES = (300000, 1, 0, 65, 32768, 32769, 100000, 150000, 63)


@pytest.mark.parametrize("variant", [
    # (options, spec): the fused kernel with the certificate build taking batches from 100 000 edges on ...
    ({"fused_cert_min_edges": 100000}, 1),
    # ... every launch in two rounds, on the interpreter ...
    ({"fused_single": 0}, 0),
    # ... and the two persistent kernels in place of the fused one
    ({"fused": 0}, 1)], ids=["fused-cert", "fused_single0-interp", "unfused"])
def test_sizes_across_the_thresholds_on_one_engine(oracle_mod, variant):
    """(c) Batch sizes back and forth across fused_single_max (32 768), fused_cert_min_edges and the grow-only scratch
    capacities; after the first (largest) batch the hand-over and item buffers are capped small, as the fresh engine
    has them from the start.  One launch with only the interior waypoints, one in the SOA layout."""
    opts, spec = variant
    m, qidx, base = _franka()
    d = Driver(oracle_mod, m, qidx, base, options=opts, spec=spec, label=f"sizes {opts} spec={spec}")
    for i, n in enumerate(SIZES):
        layout = eng_mod.SOA if n == 32769 else eng_mod.AOS
        d.launch("edges", n, layout=layout, interior_only=(n == 65), dev=(i % 2 == 1))
        if i == 0:
            d.option("uc_cap", 16)
            if "fused" in opts:
                d.option("item_cap", 3000)
    d.launch("configs", 65)
    d.close()


@pytest.mark.parametrize("spec", [0, 1])
def test_recompiling_transitions(oracle_mod, spec):
    """(d) Transitions that compile the program again: another filter tolerance, the filter off and on, the immediate
    interpreter forced and released, a planning set of fewer columns and back."""
    m, qidx, base = _franka()
    d = Driver(oracle_mod, m, qidx, base, spec=spec, label=f"recompiling spec={spec}")
    n = 20000
    d.run([("launch", "edges", n),
           ("set_filter", True, 2e-4), ("launch", "edges", n),
           ("set_filter", False), ("launch", "edges", n), ("launch", "configs", n),
           ("set_filter", True, 1e-4), ("launch", "edges", n, eng_mod.SOA),
           ("option", "force_immediate", 1), ("launch", "edges", n), ("launch", "configs", n),
           ("option", "force_immediate", 0), ("launch", "edges", n),
           ("planning", qidx[:-1], base), ("launch", "edges", n), ("launch", "contacts", 4096),
           ("planning", qidx, base), ("launch", "edges", n, eng_mod.AOS, False, True), ("launch", "contacts", 4096, eng_mod.AOS, False, True)])
    if spec:
        assert d.e.spec_kind() == 1
    d.close()


def test_moving_boxes_short_sequence(oracle_mod):
    """(f) Franka-P with the finger-pad boxes (moving boxes: the exact path is the general one, so forcing the immediate
    interpreter changes the program): spec toggles through every kind, a set_planning round trip."""
    m = scenes.franka_p(True, True)
    qidx, base = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS), m.keyframe("home").qpos.copy()
    d = Driver(oracle_mod, m, qidx, base, label="moving boxes")
    n = 20000
    d.run([("launch", "edges", n),
           ("set_spec", 0), ("launch", "edges", n),
           ("set_spec", 2), ("launch", "edges", n),
           ("set_spec", 1), ("launch", "edges", n, eng_mod.AOS, False, False, {"spec_kind": 1}),
           ("option", "force_immediate", 1), ("launch", "edges", n),
           ("option", "force_immediate", 0), ("launch", "configs", n),
           ("planning", qidx, _narrow(base)), ("launch", "edges", n),
           ("planning", qidx, base), ("launch", "edges", n, eng_mod.AOS, False, True, {"spec_kind": 1}),
           ("launch", "contacts", 4096)])
    d.close()


def test_scene_generic_robot_short_sequence(oracle_mod):
    """(f) A scene served by the robot's scene-generic library (spec kind 2): spec toggles, a planning set of fewer
    columns and back."""
    name, m, kind = generic_scenes()[2]
    assert kind == 2, name
    qidx, base = scenes.planning_index(m, scenes.FRANKA_ARM_JOINTS), m.keyframe("home").qpos.copy()
    d = Driver(oracle_mod, m, qidx, base, label=name)
    n = 20000
    d.run([("launch", "edges", n, eng_mod.AOS, False, False, {"spec_kind": 2}),
           ("set_spec", 0), ("launch", "edges", n),
           ("set_spec", 1), ("launch", "edges", n, eng_mod.AOS, False, True, {"spec_kind": 2}),
           ("planning", qidx[:-1], base), ("launch", "edges", n),
           ("planning", qidx, base), ("launch", "edges", n, eng_mod.AOS, False, False, {"spec_kind": 2}),
           ("launch", "contacts", 4096),
           ("set_spec", 2), ("launch", "configs", n)])
    d.close()


def test_long_edges_with_the_filter_off_leave_nothing_behind(oracle_mod):
    """(g) What a host-pointer launch learns about ITS batch -- here: it holds an edge of more than 64 steps, made with
    the filter off -- must not shape a later launch: with the filter on again, an ordinary batch of more than
    fused_single_max edges through device pointers gives a fresh engine's verdicts, first-bad indices, item and
    interior-edge counters and mjpl_get_info."""
    m, qidx, base = _franka()
    d = Driver(oracle_mod, m, qidx, base, label="long edges with the filter off")
    n = 40000
    assert n > d.e.get_option("fused_single")
    d.run([("set_filter", False),
           ("long_edges", 64),
           ("set_filter", True, 1e-4),
           ("launch", "edges", n, eng_mod.AOS, False, True, None, True)])
    d.close()


# ---- the nearest-neighbour look-up: one scratch per engine, whatever path the look-up before took

NN_N0 = 1000                 # nodes every ranged look-up below already has an answer for
NN_MFMA = 8192 + 5           # a range of that many nodes behind a bound, 4 096 queries or more: the matrix-core screen
NN_CELLS = 16384 + 13        # ... with option nn_cells_min_nodes = 16 384: the cell-ordered scan (64 sub-chunks of 256)


def _nn_chain(njnt):
    """A chain of `njnt` hinges, a sphere on every link: planning sets beyond Franka-P's nine joints."""
    from mjpl_amd.model import ModelBuilder
    mb = ModelBuilder()
    parent = "world"
    for k in range(njnt):
        parent = mb.add_body(f"link{k}", parent, pos=(0, 0, 0.2))
        mb.add_joint(parent, f"hinge{k}", axis=((1, 0, 0), (0, 1, 0), (0, 0, 1))[k % 3], range=(-2.9, 2.9))
        mb.add_geom(parent, "sphere", (0.03,), pos=(0, 0, 0.1))
    mb.add_keyframe("home", np.zeros(njnt))
    return mb.compile()


def _nn_engine(nplan=7, model=None, **options):
    m = scenes.franka_p() if model is None else model
    adr = np.sort(np.asarray(m.jnt_qposadr, dtype=np.int32))
    if nplan > len(adr):
        return None
    e = eng_mod.Engine(m)
    e.set_planning(adr[:nplan], m.keyframe("home").qpos)  # (Franka-P: the seven arm joints first, then the fingers)
    e.set_option("nn_cells_min_nodes", 16384)
    for k, v in options.items():
        e.set_option(k, v)
    return e


def _nn_reference(nodes, qs, counts):
    """NumPy's float64 answer for every query over nodes [0, c), c in counts: the sum over the coordinates in the kernel's
    order, the lowest index wins -- in slices of 256 queries."""
    M = qs.shape[1]
    out = {c: (np.empty(M, np.int32), np.empty(M)) for c in counts}
    for j in range(0, M, 256):
        s = np.zeros((min(256, M - j), max(counts)))
        for c in range(nodes.shape[0]):
            d = nodes[c][None, :max(counts)] - qs[c][j:j + 256][:, None]
            s = s + d * d
        for c in counts:
            out[c][0][j:j + 256] = s[:, :c].argmin(1)
            out[c][1][j:j + 256] = s[:, :c].min(1)
    return out


def _nn_data(nplan, n, M, seed):
    """A tree of n nodes (column stride n + 77) and M queries; among the nodes above NN_N0 an exact duplicate of an old
    node, with a query beside it, and a node ON a query; an old node on a query as well."""
    rng = np.random.default_rng(seed)
    nodes = np.zeros((nplan, n + 77))
    nodes[:, :n] = rng.uniform(-2.9, 2.9, size=(nplan, n))
    qs = rng.uniform(-2.9, 2.9, size=(nplan, M))
    if n > NN_N0 + 8:
        nodes[:, NN_N0 + 7] = nodes[:, 17]
        qs[:, 3] = nodes[:, 17] + 1e-9
        nodes[:, NN_N0 + 1] = qs[:, 4]
        qs[:, 5] = nodes[:, 40]
    return nodes, qs


def _nn_lookup(e, nodes, qs, n0, n, prev=None):
    """One look-up over nodes [n0, n) behind the answer `prev` for the nodes below n0 -> indices, squared distances."""
    nodes, qs = np.ascontiguousarray(nodes), np.ascontiguousarray(qs)
    cap, M = nodes.shape[1], qs.shape[1]
    dn, dq, di, dd = e.alloc(nodes.nbytes).upload(nodes), e.alloc(qs.nbytes).upload(qs), e.alloc(4 * M), e.alloc(8 * M)
    if prev is None:
        e.nearest_dev(dn.ptr, n, cap, dq.ptr, M, di.ptr, dd.ptr)
    else:
        pi, pd = e.alloc(4 * M).upload(np.ascontiguousarray(prev[0])), e.alloc(8 * M).upload(np.ascontiguousarray(prev[1]))
        e.nearest_range_dev(dn.ptr, n0, n, cap, dq.ptr, M, di.ptr, dd.ptr, pi.ptr, pd.ptr)
    return di.download(np.int32, M), dd.download(np.float64, M)


def test_what_the_last_lookup_did_follows_the_last_lookup():
    """(h) mjpl_nearest_last_screen and the read-only options nn_last_cells / nn_last_candidate_fraction speak of the LAST
    look-up on the engine's scratch: after a cell-ordered scan, a small look-up (plain float64 scan) must leave none of
    the cell-ordered scan's record behind."""
    e = _nn_engine()
    n, M = NN_N0 + NN_CELLS, 4101
    nodes, qs = _nn_data(7, n, M, seed=1)
    prev = _nn_lookup(e, nodes, qs, 0, NN_N0)
    _nn_lookup(e, nodes, qs, NN_N0, n, prev)
    assert e.get_option("nn_last_cells") == 1
    assert e.nearest_last_screen() == 2
    assert 0 < e.get_option("nn_last_candidate_fraction") <= 1
    _nn_lookup(e, nodes[:, :500 + 77], qs[:, :10], 0, 500)
    assert e.get_option("nn_last_cells") == 0
    assert e.nearest_last_screen() == 0
    assert e.get_option("nn_last_candidate_fraction") == -1
    e.close()


def test_a_reused_nearest_neighbour_scratch_answers_like_a_fresh_one():
    """(i) One engine takes the look-up's paths in turn -- plain scan, matrix-core screen, cell-ordered scan, matrix-core
    screen with more queries (a larger query side in the same arena), binary32 screen --: every call's indices and squared
    distances are those of a fresh engine that makes only that call, byte for byte, and NumPy's float64 argmin's for every
    query (n and M ragged against 32, 128 and 512; ties and zero distances in the data)."""
    n_mfma, n_cells = NN_N0 + NN_MFMA, NN_N0 + NN_CELLS
    nodes, qs = _nn_data(7, n_cells, 4613, seed=2)
    ref = _nn_reference(nodes, qs, (NN_N0, 3000, n_mfma, n_cells))
    # (options, first node, nodes, queries, what nearest_last_screen and nn_last_cells say afterwards)
    calls = [({}, 0, 3000, 700, 0, 0),
             ({}, NN_N0, n_mfma, 4101, 2, 0),
             ({}, NN_N0, n_cells, 4101, 2, 1),
             ({}, NN_N0, n_mfma, 4613, 2, 0),
             ({"nn_mfma": 0}, NN_N0, n_mfma, 4613, 1, 0)]
    live = _nn_engine()
    for options, n0, n, M, screen, cells in calls:
        prev = (ref[NN_N0][0][:M], ref[NN_N0][1][:M]) if n0 else None
        fresh = _nn_engine(**options)
        for k, v in options.items():
            live.set_option(k, v)
        got = _nn_lookup(live, nodes, qs[:, :M], n0, n, prev)
        want = _nn_lookup(fresh, nodes, qs[:, :M], n0, n, prev)
        msg = f"nodes [{n0}, {n}), {M} queries, {options}"
        for eng in (live, fresh):
            assert (eng.nearest_last_screen(), eng.get_option("nn_last_cells")) == (screen, cells), msg
        fresh.close()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), msg
        np.testing.assert_array_equal(got[0], ref[n][0][:M], err_msg=msg)
        np.testing.assert_array_equal(got[1], ref[n][1][:M], err_msg=msg)
        if n0:
            assert got[0][3] == 17 and got[0][4] == NN_N0 + 1 and got[1][4] == 0.0 and got[0][5] == 40, msg
    live.close()


@pytest.mark.parametrize("nplan", [2, 7, 8, 9])
def test_nearest_neighbour_planning_dimensions(nplan):
    """(j) The look-up's kernels are instantiated per planning dimension: the matrix-core screen for 2..7 columns (its
    ends here), the binary32 screen for 8 and 9 (the arm and the fingers).  A ranged look-up of the screened shape
    answers like NumPy's float64 argmin for every query."""
    e = _nn_engine(nplan)
    if e is None:
        pytest.skip(f"Franka-P has fewer than {nplan} joints to plan over")
    n, M = NN_N0 + NN_MFMA, 4101
    nodes, qs = _nn_data(nplan, n, M, seed=10 + nplan)
    ref = _nn_reference(nodes, qs, (NN_N0, n))
    got = _nn_lookup(e, nodes, qs, NN_N0, n, ref[NN_N0])
    assert e.nearest_last_screen() == (2 if nplan <= 7 else 1)
    np.testing.assert_array_equal(got[0], ref[n][0])
    np.testing.assert_array_equal(got[1], ref[n][1])
    e.close()


@pytest.mark.parametrize("nplan", [1, 12, 16])
def test_nearest_neighbour_generic_planning_dimension(nplan):
    """(k) Planning sets without an instantiation of their own -- one column, ten to sixteen -- take the plain scan's
    generic kernel: a small look-up answers like NumPy's.  (Franka-P has nine joints: the sets above nine are those of
    a chain of hinges.)"""
    e = _nn_engine(nplan, model=_nn_chain(nplan) if nplan > 9 else None)
    nodes, qs = _nn_data(nplan, 300, 40, seed=20 + nplan)
    ref = _nn_reference(nodes, qs, (300,))
    got = _nn_lookup(e, nodes, qs, 0, 300)
    assert e.nearest_last_screen() == 0
    np.testing.assert_array_equal(got[0], ref[300][0])
    np.testing.assert_array_equal(got[1], ref[300][1])
    e.close()
