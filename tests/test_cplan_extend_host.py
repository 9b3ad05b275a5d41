"""Chained extensions without a GPU: the ABI of mjpl_plan_paths_constrained_ext*, and their NumPy statement
(tests/cplan_extend_reference.py) held to tests/cplan_reference.py at extend = 1 and to the algorithm's invariants beyond
it, on the CPU stand-in of scenes.two_dof_ball() of tests/test_cplan_host.py."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import cplan_cases as cases
import cplan_extend_reference as xref
import cplan_reference as ref
import mjpl_amd
from mjpl_amd import build, engine
from test_cplan_host import VERDICTS, ball_edges, ball_pose_valid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("P", "n_out", "status", "rounds_used", "edges", "tree_nodes", "junction")
# the parameter sets the statement was prototyped on: each replaces entries of BALL_PARAMS
PARAMETER_SETS = ({}, dict(chain=1), dict(candidates=1), dict(nodes=12), dict(max_rows=16), dict(nodes=12, chain=32))


def run(extend, rounds=32, seed=0, **kw):
    QI, QG = cases.ball_ends()
    return xref.plan_paths_constrained(QI, QG, cases.BALL_LO, cases.BALL_HI, *VERDICTS, rounds=rounds, seed=seed, extend=extend,
                                       **{**cases.BALL_PARAMS, **kw})


def invariants(res, max_rows=256):
    QI, QG = cases.ball_ends()
    cases.check_invariants(QI, QG, res, ball_edges, ball_pose_valid, cases.BALL_PARAMS["epsilon"], cases.BALL_QSTEP, max_rows)


def same_trees(mine, theirs):
    assert (mine is None) == (theirs is None)
    if mine is not None:
        for k in range(4):
            assert np.asarray(mine[k]).tobytes() == np.asarray(theirs[k]).tobytes(), k


def test_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mjpl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    build.build_hip()
    lib = C.CDLL(build.LIB_PATH)
    for name, old in (("mjpl_plan_paths_constrained_ext", "mjpl_plan_paths_constrained"),
                      ("mjpl_plan_paths_constrained_ext_dev", "mjpl_plan_paths_constrained_dev")):
        assert re.search(rf"\b{name}\s*\(\s*struct mjpl_pose \*p, const mjpl_cplan_desc \*desc, int32_t extend,", code), name
        assert hasattr(lib, name), name
        assert name in engine.ABI, name
        # `extend` beside the descriptor, the rest as the old entry point
        args, old_args = engine.ABI[name][1], engine.ABI[old][1]
        assert args[2] is C.c_int32 and args[:2] + args[3:] == old_args, name
    assert "tests/cplan_extend_reference.py" in text
    assert C.sizeof(engine.CplanDesc) == 48  # the descriptor does not grow: `extend` travels beside it
    for f in (engine.Engine.plan_paths_constrained, engine.Engine.plan_paths_constrained_dev, mjpl_amd.planning.plan_paths_constrained):
        last = list(inspect.signature(f).parameters.values())[-1]
        assert last.name == "extend" and last.default == 1, f
    assert "extend" not in inspect.signature(engine.Engine.cplan_desc).parameters


@pytest.mark.parametrize("extend", [0, 33])
def test_bad_extend_is_refused(extend):
    # the Python surface: before any engine work (no engine exists here; the check takes no `self`)
    with pytest.raises(ValueError):
        engine.Engine.plan_paths_constrained(None, None, None, None, None, None, 0.01, 0.05, extend=extend)
    with pytest.raises(ValueError):
        engine.Engine.plan_paths_constrained_dev(None, None, None, None, 0, None, None, 0.01, 0.05, None, None, None, extend=extend)
    nothing = object()  # (stands where an engine would: the refusal comes before it is used)
    model = SimpleNamespace(nq=2, jnt_range=np.array([[-2.0, 2.0], [-2.0, 2.0]]))
    collision, pose = SimpleNamespace(model=model, engine=nothing), SimpleNamespace(engine=nothing)
    assert mjpl_amd.plan_paths_constrained([], [], collision, pose, 0.01, epsilon=0.05, extend=1) == []
    with pytest.raises(ValueError):
        mjpl_amd.plan_paths_constrained([], [], collision, pose, 0.01, epsilon=0.05, extend=extend)
    with pytest.raises(ValueError):
        run(extend, rounds=1)
    # the library: MJPL_E_ARG before anything else is touched -- a NULL handle, a NULL descriptor and B = 0 with it
    build.build_hip()
    lib = C.CDLL(build.LIB_PATH)
    for name in ("mjpl_plan_paths_constrained_ext", "mjpl_plan_paths_constrained_ext_dev"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = engine.ABI[name]
        assert fn(None, None, extend, None, None, 0, None, None, None, None, None, None, None, None) == -1, name
        lib.mjpl_last_error.restype = C.c_char_p
        assert b"extend" in lib.mjpl_last_error(), name


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
@pytest.mark.parametrize("params", PARAMETER_SETS, ids=lambda p: " ".join(f"{k}={v}" for k, v in p.items()) or "defaults")
def test_extend_one_is_the_old_statement(params, seed):
    QI, QG = cases.ball_ends()
    want = ref.plan_paths_constrained(QI, QG, cases.BALL_LO, cases.BALL_HI, *VERDICTS, rounds=32, seed=seed,
                                      **{**cases.BALL_PARAMS, **params})
    got = run(1, seed=seed, **params)
    for f in OUTPUTS:
        assert got[f].dtype == want[f].dtype and got[f].tobytes() == want[f].tobytes(), f
    assert got["forward"] == want["forward"]
    for mine, theirs in zip(got["trees"], want["trees"]):
        same_trees(mine, theirs)


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
@pytest.mark.parametrize("extend", [2, 5, 8, 32])
def test_invariants(extend, seed):
    for params in PARAMETER_SETS:
        res = run(extend, seed=seed, **params)
        invariants(res, params.get("max_rows", 256))
        n = params.get("nodes", cases.BALL_PARAMS["nodes"])
        assert (res["tree_nodes"] <= n).all(), params
        # every node but a root has a parent that was appended before it
        for t in (t for t in res["trees"] if t is not None):
            for par in (t[1], t[3]):
                assert par[0] == -1 and all(0 <= p < k for k, p in enumerate(par) if k), params


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
def test_rounds_prefix(seed):
    """The state after rounds = R equals the state of a longer run after R rounds, at extend = 5."""
    long_run = run(5, seed=seed)
    for R1 in (1, 2, 5):
        short = run(5, rounds=R1, seed=seed)
        for b in range(len(cases.BALL_PROBLEMS)):
            ls, lr = int(long_run["status"][b]), int(long_run["rounds_used"][b])
            settled = (ls in (ref.NONFINITE, ref.INVALID_END) or (ls in (ref.SOLVED, ref.LONG) and lr <= R1) or
                       (ls == ref.NODES and lr < R1))
            if settled:
                for f in OUTPUTS:
                    assert short[f][b].tobytes() == long_run[f][b].tobytes(), (R1, b, f)
                same_trees(short["trees"][b], long_run["trees"][b])
                continue
            assert short["status"][b] == ref.ROUNDS and short["rounds_used"][b] == R1 and short["n_out"][b] == 0, (R1, b)
            assert short["edges"][b] <= long_run["edges"][b]
            for k in range(4):  # nodes and parents are only ever appended
                mine, theirs = short["trees"][b][k], long_run["trees"][b][k]
                assert len(mine) <= len(theirs), (R1, b)
                assert np.asarray(mine).tobytes() == np.asarray(theirs[:len(mine)]).tobytes(), (R1, b, k)
    assert (long_run["rounds_used"] > 2).any()  # (some problem was still live at the prefixes compared)


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
@pytest.mark.parametrize("extend", [5, 32])
def test_node_capacity_is_met_exactly(extend, seed):
    res = run(extend, seed=seed, nodes=12)
    sizes = [len(t[k]) for t in res["trees"] if t is not None for k in (0, 2)]
    print("tree sizes", sizes, "status", res["status"])
    assert max(sizes) == 12 and res["tree_nodes"].max() == 12
    assert all(len(t[0]) == len(t[1]) and len(t[2]) == len(t[3]) for t in res["trees"] if t is not None)
    invariants(res)


@pytest.mark.parametrize("seed", cases.BALL_SEEDS)
def test_chained_extensions_explore_in_fewer_rounds(seed):
    res = run(8, seed=seed)
    print("status", res["status"], "rounds", res["rounds_used"], "rows", res["n_out"], "edges", res["edges"], "nodes", res["tree_nodes"].tolist())
    assert tuple(res["status"]) == cases.BALL_STATUS
    assert res["rounds_used"].max() <= 5  # (12 and 15 at extend = 1: tests/test_cplan_host.py)
    invariants(res)


def test_a_chain_is_one_project_call_per_step():
    calls = []

    def pj(A, X):
        calls.append(len(A))
        return VERDICTS[2](A, X)

    QI, QG = cases.ball_ends()
    res = xref.plan_paths_constrained(QI, QG, cases.BALL_LO, cases.BALL_HI, VERDICTS[0], VERDICTS[1], pj, VERDICTS[3], rounds=1, seed=0,
                                      extend=5, **cases.BALL_PARAMS)
    live = int((res["status"] != ref.INVALID_END).sum())
    # round 0: at most `chain` calls for the bridges (never more than `live` rows), then at most 5 for the chains: the
    # first over every candidate, each later one over no more rows than the one before it
    every = live * cases.BALL_PARAMS["candidates"]
    assert every in calls
    first = calls.index(every)
    assert first <= cases.BALL_PARAMS["chain"] and 2 <= len(calls) - first <= 5
    assert all(a >= b for a, b in zip(calls[first:], calls[first + 1:])), calls
