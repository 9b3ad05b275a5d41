"""What mjpl_shortcut_paths*, mjpl_plan_paths*, mjpl_plan_paths_constrained* and the roadmap calls share on the host
(mjpl_amd/csrc/mjpl_hip.hip: one arena per family, one round loop, one phase timer, one reset per family): calls in
sequence on one engine give the bits of the same call made first on a fresh engine, the phase times are there when
asked for, and an empty call leaves no statistic of an earlier one.  Needs the MI355X."""
from types import SimpleNamespace

import numpy as np
import pytest

import plan_cases
import shortcut_cases
from mjpl_amd import PoseConstraint, engine, site_pose

pytestmark = pytest.mark.gpu

STEP = 0.05
SHORTCUT_STEP = 0.02
RADIUS = 3.0
SHORTCUT_MS = ("shortcut_last_propose_ms", "shortcut_last_validate_ms", "shortcut_last_commit_ms")
PLAN_MS = ("plan_last_propose_ms", "plan_last_validate_ms", "plan_last_commit_ms", "plan_last_project_ms")
ROADMAP_MS = tuple(f"roadmap_last_phase{k}_ms" for k in range(4))
SHORTCUT_LAST = ("shortcut_last_chunks", "shortcut_last_rounds", "shortcut_last_edges") + SHORTCUT_MS
PLAN_LAST = ("plan_last_chunks", "plan_last_rounds", "plan_last_edges") + PLAN_MS
ROADMAP_LAST = ("roadmap_last_edges", "roadmap_last_chunks", "roadmap_last_sweeps") + ROADMAP_MS


def shortcut(W, off):
    return lambda e, pose: e.shortcut_paths(W, off, SHORTCUT_STEP, rounds=4, candidates=16, seed=5)


def plan(QI, QG, lo, hi, nodes=512):
    return lambda e, pose: e.plan_paths(QI, QG, lo, hi, STEP, 1.0, rounds=6, candidates=16, nodes=nodes, seed=2)


def cplan(QI, QG, lo, hi):
    return lambda e, pose: e.plan_paths_constrained(pose, QI, QG, lo, hi, STEP, 0.1, rounds=8, candidates=16, nodes=256, chain=4, seed=3,
                                                    extend=3)


def build(Q):
    return lambda e, pose: e.roadmap_build(Q, RADIUS, STEP, 8)


def query(Q, graph, QI, QG):
    return lambda e, pose: e.roadmap_query(Q, *graph, QI, QG, RADIUS, STEP, 4, 64)


def engine_and_pose(model, qidx, base):
    """An engine on the planning columns and a PoseConstraint of it: the end effector within 0.1 rad of upright in roll
    and pitch, as in tests/test_gpu_cplan.py."""
    e = engine.Engine(model, device=0)
    pose = PoseConstraint(model, "ee_site", site_pose(model, base, "ee_site", engine=e), roll=(-0.1, 0.1), pitch=(-0.1, 0.1),
                          q_step=0.1, engine=e)
    e.set_planning(qidx, base)
    return e, pose


def on_a_fresh_engine(s, call):
    e, pose = engine_and_pose(s.model, s.qidx, s.base)
    try:
        return call(e, pose)
    finally:
        e.close()


@pytest.fixture(scope="module")
def franka():
    """The headline scene over the 7 arm columns: one engine, one PoseConstraint on it, and 24 seeded pairs on the
    constraint's manifold (uniform draws projected with q_step = inf, kept where they lie in the box and are
    collision-valid and pose-valid)."""
    model, qidx, base, lo, hi = plan_cases.franka_planning()
    e, pose = engine_and_pose(model, qidx, base)

    def full(Q):
        F = np.tile(base, (len(Q), 1))
        F[:, qidx] = Q
        return F
    rng = np.random.default_rng(23)
    pose.q_step = np.inf
    rows = np.zeros((0, len(qidx)))
    while len(rows) < 48:
        X = full(rng.uniform(lo, hi, size=(96, len(qidx))))
        Y, ok, _ = pose.apply_batch(X, X)
        Y = np.ascontiguousarray(Y[:, qidx])
        ok &= (Y >= lo).all(axis=1) & (Y <= hi).all(axis=1)
        Y = Y[ok]
        rows = np.concatenate([rows, Y[e.check_configs(Y).astype(bool) & pose.valid_configs(full(Y))]])
    pose.q_step = 0.1
    yield SimpleNamespace(model=model, e=e, pose=pose, qidx=np.asarray(qidx), base=base, lo=lo, hi=hi, QI=rows[:24].copy(), QG=rows[24:48].copy())
    e.close()


@pytest.fixture(scope="module")
def calls(franka):
    """name -> (the call, its result as the first call of a fresh engine), on the headline scene's planning columns:
    computed once, shared, never changed."""
    s = franka
    valid = lambda Q: s.e.check_configs(Q).astype(bool)  # noqa: E731
    W, off = shortcut_cases.pack(shortcut_cases.random_walks(s.lo, s.hi, valid, [12, 16, 20, 24, 28, 32, 36, 40], seed=11))
    QI, QG = plan_cases.random_ends(s.lo, s.hi, valid, 37, seed=11)
    Q = np.concatenate(plan_cases.random_ends(s.lo, s.hi, valid, 128, seed=29, repeats=()))
    assert len(Q) == 256
    made = {"shortcut": shortcut(W, off), "plan": plan(QI, QG, s.lo, s.hi), "cplan": cplan(s.QI, s.QG, s.lo, s.hi), "build": build(Q)}
    first = {name: on_a_fresh_engine(s, call) for name, call in made.items()}
    made["query"] = query(Q, first["build"], QI[:16], QG[:16])
    made["plan, 5 pairs"] = plan(QI[:5], QG[:5], s.lo, s.hi)
    made["plan, 2048 nodes"] = plan(QI, QG, s.lo, s.hi, nodes=2048)
    for name in ("query", "plan, 5 pairs", "plan, 2048 nodes"):
        first[name] = on_a_fresh_engine(s, made[name])
    return {name: (made[name], first[name]) for name in made}


def same_bits(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        bad = np.flatnonzero(np.ascontiguousarray(a).reshape(-1).view(np.uint8) != np.ascontiguousarray(b).reshape(-1).view(np.uint8))
        assert len(bad) == 0, f"{what}, output {k}: {len(bad)} bytes differ, first at {bad[:5].tolist()}"


def test_calls_in_sequence_are_the_first_calls_of_a_fresh_engine(franka, calls):
    s = franka
    five = ("shortcut", "plan", "cplan", "build", "query")
    # (after the five and the five in reverse: a batch the arena is larger than needed for, then one it must grow for)
    for at, name in enumerate(five + five[::-1] + ("plan, 5 pairs", "plan, 2048 nodes")):
        call, first = calls[name]
        same_bits(call(s.e, s.pose), first, f"call {at} ({name})")
    # the calls did work worth comparing
    assert (calls["shortcut"][1][5] > 0).any() and (calls["plan"][1][3] > 0).any() and (calls["cplan"][1][3] > 0).any()
    assert calls["build"][1][1][-1] > 0 and (calls["query"][1][1] >= 2).any()


def timed(e, call, pose, names):
    e.set_option("kernel_timer", 1)  # (setting it also returns the events to the pool)
    try:
        call(e, pose)
        return {n: e.get_option(n) for n in names}
    finally:
        e.set_option("kernel_timer", 0)


def test_phase_times(franka, calls):
    e, pose = franka.e, franka.pose
    ms = timed(e, calls["plan"][0], pose, PLAN_MS)
    print("plan", ms)
    assert all(ms[n] > 0 for n in PLAN_MS[:3]) and ms["plan_last_project_ms"] == 0
    ms = timed(e, calls["cplan"][0], pose, PLAN_MS)
    print("constrained plan", ms)
    assert all(ms[n] > 0 for n in PLAN_MS)
    ms = timed(e, calls["shortcut"][0], pose, SHORTCUT_MS)
    print("shortcut", ms)
    assert all(ms[n] > 0 for n in SHORTCUT_MS)
    ms = timed(e, calls["build"][0], pose, ROADMAP_MS + ("roadmap_last_edges",))
    print("roadmap build", ms)
    assert ms["roadmap_last_edges"] >= 1 and all(ms[n] > 0 for n in ROADMAP_MS)
    ms = timed(e, calls["query"][0], pose, ROADMAP_MS)
    print("roadmap query", ms)
    assert all(ms[n] > 0 for n in ROADMAP_MS[:3]) and ms["roadmap_last_phase3_ms"] == 0
    # without the option no phase is timed, whatever the call before left
    assert e.get_option("kernel_timer") == 0
    for name, names in (("plan", PLAN_MS), ("cplan", PLAN_MS), ("shortcut", SHORTCUT_MS), ("build", ROADMAP_MS), ("query", ROADMAP_MS)):
        calls[name][0](e, pose)
        assert [e.get_option(n) for n in names] == [0.0] * len(names), name


def test_an_empty_call_resets_its_family(franka, calls):
    s = franka
    e, pose, d = s.e, s.pose, len(s.qidx)
    none = np.zeros((0, d))
    graph = calls["build"][1]
    Q = np.zeros((256, d))  # (the graph's arrays alone say how many nodes there are: B = 0 reads no row)
    empty = {
        "shortcut": (shortcut(none, np.zeros(1, np.int64)), SHORTCUT_LAST),
        "plan": (plan(none, none, s.lo, s.hi), PLAN_LAST),
        "cplan": (cplan(none, none, s.lo, s.hi), PLAN_LAST),
        "build": (build(none), ROADMAP_LAST),
        "query": (query(Q, graph, none, none), ROADMAP_LAST),
    }
    for name, (call, names) in empty.items():
        before = timed(e, calls[name][0], pose, names)
        assert before[names[0]] > 0 and any(before[n] > 0 for n in names[3:]), (name, before)
        out = call(e, pose)
        # (every output is empty, but for the row offsets of a graph without nodes: [0])
        assert all(a.tolist() == [0] if (name, k) == ("build", 1) else len(a) == 0 for k, a in enumerate(out)), name
        after = {n: e.get_option(n) for n in names}
        assert all(v == 0 for v in after.values()), (name, after)
