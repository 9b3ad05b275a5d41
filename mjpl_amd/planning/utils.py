"""CBiRRT building blocks (reference src/mjpl/planning/utils.py:9-249): constrained extend,
edge interval check, path shortcutting.  Same names, arguments, return values and errors as
the reference; the interval check goes to the engine in ONE launch when the constraint
offers ``valid_interval`` (mjpl_amd.CollisionConstraint does).
"""
from __future__ import annotations

import numpy as np

from ..constraint.constraint_interface import Constraint
from ..constraint.utils import apply_constraints
from .tree import Node, Tree


def path_length(waypoints: list[np.ndarray]) -> float:
    """Sum of Euclidean segment lengths in configuration space (:90-102)."""
    pts = np.asarray(waypoints, dtype=np.float64)
    if len(pts) < 2:
        return 0.0
    return float(np.linalg.norm(pts[1:] - pts[:-1], axis=1).sum())


def _step(start: np.ndarray, target: np.ndarray, max_step_dist: float) -> np.ndarray:
    """Move ``start`` toward ``target`` by at most ``max_step_dist`` (:167-185)."""
    if max_step_dist <= 0.0:
        raise ValueError("`max_step_dist` must be > 0.0")
    if np.array_equal(start, target):
        return start.copy()
    delta = target - start
    dist = np.linalg.norm(delta)
    return start + (delta / dist) * min(max_step_dist, dist)


def _valid_collision_interval(start: np.ndarray, end: np.ndarray, step_dist: float,
                              constraint) -> bool:
    """Do the configurations strictly between ``start`` and ``end``, ``step_dist`` apart, obey
    ``constraint``?  (:188-216).  End points are not checked."""
    if step_dist <= 0.0:
        raise ValueError("`step_dist` must be > 0")
    batched = getattr(constraint, "valid_interval", None)
    if batched is not None:
        return bool(batched(start, end, step_dist))
    # generic constraint: walk the interval on the host, stop at the first violation
    cur = _step(start, end, step_dist)
    while not np.array_equal(cur, end):
        if not constraint.valid_config(cur):
            return False
        cur = _step(cur, end, step_dist)
    return True


def _batch_capable(constraints: list[Constraint], collision_interval_check) -> bool:
    """True when a whole extension can be validated in batched launches: no constraint projects
    (``projects`` is False) and every one offers row-wise ``valid_configs`` (and the interval
    constraint row-wise ``valid_intervals``)."""
    for c in constraints:
        if getattr(c, "projects", True) or not hasattr(c, "valid_configs"):
            return False
    return collision_interval_check is None or hasattr(collision_interval_check[1], "valid_intervals")


def _constrained_extend_batched(q_target: np.ndarray, tree: Tree, eps: float, constraints: list[Constraint],
                                collision_interval_check, equality_threshold: float) -> np.ndarray:
    """``_constrained_extend`` when no constraint projects.  The candidate configurations then do
    not depend on the verdicts -- q_{k+1} = _step(q_k, q_target, eps) -- so the whole chain towards
    the target is generated first and validated in one batch per constraint (plus one for the
    intervals); the tree receives the nodes before the first failing step, exactly the nodes the
    step-by-step loop would have added."""
    node = tree.nearest_neighbor(q_target)
    chain = [node.q]
    while not np.array_equal(q_target, chain[-1]):
        q_prev = chain[-1]
        q = _step(q_prev, q_target, eps)
        if np.linalg.norm(q - q_prev) < equality_threshold:
            break
        if np.linalg.norm(q_target - q) > np.linalg.norm(q_target - q_prev):
            break
        chain.append(q)
    if len(chain) == 1:
        return chain[0]
    Q = np.stack(chain)
    ok = np.ones(len(chain) - 1, dtype=bool)
    for c in constraints:
        idx = np.flatnonzero(ok)
        if len(idx) == 0:
            break
        ok[idx] = np.asarray(c.valid_configs(Q[1:][idx]), dtype=bool)
    if collision_interval_check is not None and ok.any():
        step_dist, cc = collision_interval_check
        n_ok = len(ok) if ok.all() else int(np.argmin(ok))  # only the steps before the first failure matter
        ok[:n_ok] &= np.asarray(cc.valid_intervals(Q[:-1][:n_ok], Q[1:][:n_ok], step_dist), dtype=bool)
    n_add = len(ok) if ok.all() else int(np.argmin(ok))
    for k in range(1, n_add + 1):
        node = Node(chain[k], node)
        tree.add_node(node)
    return chain[n_add]


def _constrained_extend(q_target: np.ndarray, tree: Tree, eps: float, constraints: list[Constraint],
                        collision_interval_check=None, equality_threshold: float = 1e-8) -> np.ndarray:
    """CBiRRT Algorithm 2 (:105-164): grow ``tree`` from its node nearest to ``q_target`` in
    steps of at most ``eps``; returns the configuration reached."""
    if _batch_capable(constraints, collision_interval_check):
        return _constrained_extend_batched(q_target, tree, eps, constraints, collision_interval_check,
                                           equality_threshold)
    node = tree.nearest_neighbor(q_target)
    q_prev = node.q
    q_cur = node.q
    while not np.array_equal(q_target, q_cur):
        q_cur = apply_constraints(q_prev, _step(q_cur, q_target, eps), constraints)
        # stop rules (:151-160): constraint failure | no progress | moved away from the target |
        # colliding interval between the last node and the new configuration
        if q_cur is None:
            return q_prev
        if np.linalg.norm(q_cur - q_prev) < equality_threshold:
            return q_prev
        if np.linalg.norm(q_target - q_cur) > np.linalg.norm(q_target - q_prev):
            return q_prev
        if collision_interval_check is not None and not _valid_collision_interval(
                q_prev, q_cur, *collision_interval_check):
            return q_prev
        node = Node(q_cur, node)
        tree.add_node(node)
        q_prev = q_cur
    return q_cur


def _combine_paths(start_tree: Tree, start_tree_node: Node, goal_tree: Tree,
                   goal_tree_node: Node) -> list[np.ndarray]:
    """Root(start_tree) ... start_tree_node -> goal_tree_node ... root(goal_tree) (:219-249);
    a shared junction configuration appears once."""
    head = [n.q for n in reversed(start_tree.get_path(start_tree_node))]
    tail = [n.q for n in goal_tree.get_path(goal_tree_node)]
    if np.array_equal(head[-1], tail[0]):
        head = head[:-1]
    return head + tail


def smooth_path(waypoints: list[np.ndarray], constraints: list[Constraint],
                collision_interval_check=None, eps: float = 0.05, num_tries: int = 100,
                seed: int | None = None, sparse: bool = False) -> list[np.ndarray]:
    """CBiRRT Algorithm 3 (:9-87): ``num_tries`` random shortcut attempts."""
    if not waypoints:
        raise ValueError("`waypoints` cannot be empty.")
    if eps <= 0.0:
        raise ValueError("`eps` must be > 0.")
    if num_tries <= 0:
        raise ValueError("`num_tries` must be > 0.")

    path = waypoints
    rng = np.random.default_rng(seed=seed)
    for _ in range(num_tries):
        i = rng.integers(0, len(path) - 1)
        j = rng.integers(i + 1, len(path))
        tree = Tree(Node(path[i]))
        reached = _constrained_extend(path[j], tree, eps, constraints, collision_interval_check)
        if not np.array_equal(reached, path[j]):
            continue
        # projections move configurations arbitrarily: keep the shortcut only if it is shorter
        chain = [n.q for n in tree.get_path(tree.nearest_neighbor(reached))]  # path[j] ... path[i]
        if path_length(chain) < path_length(path[i:j + 1]):
            if sparse:
                path = path[:i + 1] + path[j:]
            else:
                chain.reverse()
                path = path[:i] + chain[:-1] + path[j:]
    return path


def smooth_paths(paths: list[list[np.ndarray]], collision, step_dist: float, *, rounds: int = 16, candidates: int = 64,
                 seed: int = 0, min_saving: float = 0.0, return_info: bool = False):
    """Shortcut many paths at once on the GPU: the batched counterpart of ``smooth_path(..., sparse=True)``.

    The paths advance in lockstep.  Every round each path proposes up to ``candidates`` (1..64) shortcuts between
    waypoints it still holds -- all pairs once they are few enough, seeded random pairs otherwise --, the proposals of
    ALL paths that would shorten their path by more than ``min_saving`` are validated by one edge launch of
    ``collision`` (a :class:`mjpl_amd.CollisionConstraint`; end point and interior waypoints ``step_dist`` apart), and
    each path takes its valid ones greedily, largest saving first, skipping any that overlaps one already taken.  A path
    is done when no single shortcut is both valid and shorter, or after ``rounds`` rounds.  ``include/mjpl_hip.h``
    (``mjpl_shortcut_paths``) states the algorithm; the result depends on ``seed``, never on how the batch is chunked.

    Returns a list of waypoint lists: a subset of each path's own full-``nq`` arrays (sparse output, first and last
    waypoint always kept).  With ``return_info`` also a list of dicts, one per path: ``status`` ("converged", "rounds"
    or "nonfinite": a path holding NaN / inf comes back whole), ``length``, ``proposed`` (edges validated) and
    ``accepted`` (shortcuts taken).

    Only the collision constraint is consulted.  A straight segment between two configurations inside the joint box
    stays inside it, so a ``JointLimitConstraint`` the waypoints obey needs no check.  Constraints that project
    (``PoseConstraint``) and dense output (``sparse=False``) remain with :func:`smooth_path`.

    Raises ``ValueError`` for an empty path, a path of fewer than 2 waypoints, a waypoint that is not a full-``nq``
    configuration, or a bad parameter.
    """
    from .. import engine as _engine
    nq = collision.model.nq
    desc = _engine.Engine.shortcut_desc(step_dist, rounds, candidates, seed, min_saving)  # (ValueError for a bad parameter)
    del desc
    paths = list(paths)
    rows, wp_off = [], [0]
    for b, path in enumerate(paths):
        if path is None or len(path) == 0:
            raise ValueError(f"path {b} is empty")
        if len(path) < 2:
            raise ValueError(f"path {b} has {len(path)} waypoint: at least 2 are needed")
        P = np.asarray(path, dtype=np.float64)
        if P.ndim != 2 or P.shape[1] != nq:
            raise ValueError(f"path {b}: waypoints must be full configurations of {nq} entries, got {P.shape}")
        rows.append(P)
        wp_off.append(wp_off[-1] + len(P))
    if not paths:
        return ([], []) if return_info else []
    collision._ensure_full()
    keep, _, length, status, proposed, accepted = collision.engine.shortcut_paths(
        np.concatenate(rows), np.asarray(wp_off, dtype=np.int64), step_dist, rounds=rounds, candidates=candidates, seed=seed,
        min_saving=min_saving)
    out = [[q for q, k in zip(path, keep[wp_off[b]:wp_off[b + 1]]) if k] for b, path in enumerate(paths)]
    if not return_info:
        return out
    names = {_engine.SHORTCUT_CONVERGED: "converged", _engine.SHORTCUT_ROUNDS: "rounds", _engine.SHORTCUT_NONFINITE: "nonfinite"}
    info = [dict(status=names[int(status[b])], length=float(length[b]), proposed=int(proposed[b]), accepted=int(accepted[b]))
            for b in range(len(paths))]
    return out, info


def plan_paths(q_inits, q_goals, collision, step_dist: float, *, epsilon: float, rounds: int = 32, candidates: int = 16,
               nodes: int = 1024, seed: int = 0, lo=None, hi=None, return_info: bool = False):
    """Plan many start/goal pairs at once on the GPU: a bidirectional RRT whose problems take their rounds in lockstep.

    This is the planner for many independent, mostly easy queries -- pick/place pairs, the edges of a roadmap, a set of
    IK goals to rank; :class:`DeviceBiRRT` stays the one for a single hard query.  A pair whose straight edge is valid
    is solved at once.  Otherwise each problem grows a tree from either end, alternately: every round it proposes up to
    ``candidates`` (1..64) extensions of at most ``epsilon`` towards seeded uniform samples of the box ``[lo, hi]``, and
    one edge that would join the trees where the other tree grew last; the edges of ALL problems are validated by one
    edge launch of ``collision`` (a :class:`mjpl_amd.CollisionConstraint`; waypoints ``step_dist`` apart), and each
    problem takes the join if it is valid, its valid extensions otherwise.  A tree holds at most ``nodes`` (2..65536)
    configurations.  ``include/mjpl_hip.h`` (``mjpl_plan_paths``) states the algorithm; the result depends on ``seed``
    and on a problem's index in the call, never on how the batch is chunked.

    ``q_inits`` and ``q_goals`` are full-``nq`` configurations.  ``lo`` and ``hi`` default to the model's joint ranges;
    a joint with ``lo == hi`` stays put (both ends must hold it there).

    Returns, per problem, the path as a list of ``nq`` arrays -- the first and last are the caller's own objects -- or
    ``None`` for a problem that was not solved.  With ``return_info`` also a list of dicts, one per problem: ``status``
    ("solved", "rounds", "nonfinite", "invalid_end" or "nodes"), ``rounds_used``, ``edges`` (edges validated, the
    direct one included) and ``nodes`` (the sizes of the two trees).  The paths are unsmoothed; :func:`smooth_paths`
    takes them as they are (drop the ``None`` entries first).

    Raises ``ValueError`` for lists of different lengths, a configuration that is not a full-``nq`` one, a finite end
    outside ``[lo, hi]``, or a bad parameter.
    """
    from .. import engine as _engine
    model = collision.model
    nq = model.nq
    _engine.Engine.plan_desc(step_dist, epsilon, rounds, candidates, nodes, seed)  # (ValueError for a bad parameter)
    q_inits, q_goals = list(q_inits), list(q_goals)
    if len(q_inits) != len(q_goals):
        raise ValueError(f"{len(q_inits)} q_inits but {len(q_goals)} q_goals")
    lo = np.asarray(model.jnt_range[:, 0] if lo is None else lo, dtype=np.float64)
    hi = np.asarray(model.jnt_range[:, 1] if hi is None else hi, dtype=np.float64)
    if lo.shape != (nq,) or hi.shape != (nq,):
        raise ValueError(f"lo and hi must have {nq} entries, got {lo.shape} and {hi.shape}")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (lo > hi).any():
        raise ValueError("lo and hi must be finite, with lo <= hi")
    if not q_inits:
        return ([], []) if return_info else []
    QI, QG = np.asarray(q_inits, dtype=np.float64), np.asarray(q_goals, dtype=np.float64)
    if QI.shape != (len(q_inits), nq) or QG.shape != QI.shape:
        raise ValueError(f"q_inits and q_goals must be full configurations of {nq} entries, got {QI.shape} and {QG.shape}")
    for name, Q in (("q_inits", QI), ("q_goals", QG)):
        out = np.flatnonzero(((Q < lo) | (Q > hi)).any(axis=1))  # (NaN compares false: the library reports it)
        if len(out):
            raise ValueError(f"{name}[{out[0]}] lies outside [lo, hi]")
    collision._ensure_full()
    P, n_out, status, rounds_used, edges, tree_nodes = collision.engine.plan_paths(
        QI, QG, lo, hi, step_dist, epsilon, rounds=rounds, candidates=candidates, nodes=nodes, seed=seed)
    paths = []
    for b in range(len(q_inits)):
        if status[b] != _engine.PLAN_SOLVED:
            paths.append(None)
            continue
        paths.append([q_inits[b]] + [P[b, k].copy() for k in range(1, n_out[b] - 1)] + [q_goals[b]])
    if not return_info:
        return paths
    names = {_engine.PLAN_SOLVED: "solved", _engine.PLAN_ROUNDS: "rounds", _engine.PLAN_NONFINITE: "nonfinite",
             _engine.PLAN_INVALID_END: "invalid_end", _engine.PLAN_NODES: "nodes"}
    info = [dict(status=names[int(status[b])], rounds_used=int(rounds_used[b]), edges=int(edges[b]),
                 nodes=(int(tree_nodes[b, 0]), int(tree_nodes[b, 1]))) for b in range(len(q_inits))]
    return paths, info


def plan_paths_constrained(q_inits, q_goals, collision, pose, step_dist: float, *, epsilon: float, rounds: int = 64,
                           candidates: int = 16, nodes: int = 1024, chain: int = 8, max_rows: int = 256, seed: int = 0,
                           lo=None, hi=None, return_info: bool = False, extend: int = 1):
    """:func:`plan_paths` under a projecting constraint: many start/goal pairs at once on the GPU, every waypoint on
    the manifold of ``pose`` (a :class:`mjpl_amd.PoseConstraint` made with ``engine=collision.engine``).

    This is the reference's CBiRRT taken in lockstep.  Every tree edge is ONE step of at most ``epsilon`` projected by
    ``pose.apply`` (and kept only if it moved, came no farther from its target and stayed within ``2 * pose.q_step`` of
    the node it left), so there is no straight connect edge of any length -- its interior would leave the manifold.
    Instead each round a problem builds a *bridge*: a chain of up to ``chain`` (1..32) projected steps from the growing
    tree towards the closest node the other tree gained, closed by one straight edge of at most ``epsilon``; beside it, up
    to ``candidates`` extensions towards seeded uniform samples.  An extension is a chain of up to ``extend`` (1..32)
    projected steps from the nearest node, each from the one before it, cut at the first step that is refused: what the
    reference's ``_constrained_extend`` does until it is stopped, taken inside one round and cut at ``extend``.  With the
    default of 1 a tree's frontier moves by at most ``epsilon`` a round, which solves only pairs that are already
    close on the manifold (DESIGN.md 5.18 has the measurements).  Links, closing edge and extensions of ALL
    problems are validated by one edge launch of ``collision`` per round (waypoints ``step_dist`` apart; the interior of
    a step is sampled for collision only, as in the reference).  ``include/mjpl_hip.h``
    (``mjpl_plan_paths_constrained``) states the algorithm.

    Choose ``epsilon < 2 * pose.q_step``: at ``epsilon == 2 * pose.q_step`` the projection's "farther than 2 q_step
    from where it started" rule turns on roundings, and even a free straight line fails at random.

    Returns what :func:`plan_paths` returns: per problem the path as a list of ``nq`` arrays, or ``None``.  A path has
    at most ``max_rows`` waypoints; a longer one is reported, not cut: with ``return_info`` the status strings are those
    of :func:`plan_paths` and ``"long"``.  Both ends must satisfy ``pose`` (``"invalid_end"`` otherwise).
    :func:`smooth_paths` is unconstrained and would leave the manifold: hand the paths to
    ``generate_constrained_trajectories`` as they are.

    Raises ``ValueError`` if ``pose.engine is not collision.engine``, and for everything :func:`plan_paths` raises it for.
    """
    from .. import engine as _engine
    model = collision.model
    nq = model.nq
    if getattr(pose, "engine", None) is not collision.engine:
        raise ValueError("pose and collision must share one engine: PoseConstraint(..., engine=collision.engine)")
    _engine.Engine.cplan_desc(step_dist, epsilon, rounds, candidates, nodes, chain, max_rows, seed)  # (ValueError for a bad parameter)
    _engine.Engine._cplan_extend(extend)
    q_inits, q_goals = list(q_inits), list(q_goals)
    if len(q_inits) != len(q_goals):
        raise ValueError(f"{len(q_inits)} q_inits but {len(q_goals)} q_goals")
    lo = np.asarray(model.jnt_range[:, 0] if lo is None else lo, dtype=np.float64)
    hi = np.asarray(model.jnt_range[:, 1] if hi is None else hi, dtype=np.float64)
    if lo.shape != (nq,) or hi.shape != (nq,):
        raise ValueError(f"lo and hi must have {nq} entries, got {lo.shape} and {hi.shape}")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (lo > hi).any():
        raise ValueError("lo and hi must be finite, with lo <= hi")
    if not q_inits:
        return ([], []) if return_info else []
    QI, QG = np.asarray(q_inits, dtype=np.float64), np.asarray(q_goals, dtype=np.float64)
    if QI.shape != (len(q_inits), nq) or QG.shape != QI.shape:
        raise ValueError(f"q_inits and q_goals must be full configurations of {nq} entries, got {QI.shape} and {QG.shape}")
    for name, Q in (("q_inits", QI), ("q_goals", QG)):
        out = np.flatnonzero(((Q < lo) | (Q > hi)).any(axis=1))  # (NaN compares false: the library reports it)
        if len(out):
            raise ValueError(f"{name}[{out[0]}] lies outside [lo, hi]")
    collision._ensure_full()
    P, n_out, status, rounds_used, edges, tree_nodes = collision.engine.plan_paths_constrained(
        pose, QI, QG, lo, hi, step_dist, epsilon, rounds=rounds, candidates=candidates, nodes=nodes, chain=chain, max_rows=max_rows,
        seed=seed, extend=extend)
    paths = []
    for b in range(len(q_inits)):
        if status[b] != _engine.PLAN_SOLVED:
            paths.append(None)
            continue
        paths.append([q_inits[b]] + [P[b, k].copy() for k in range(1, n_out[b] - 1)] + [q_goals[b]])
    if not return_info:
        return paths
    names = {_engine.PLAN_SOLVED: "solved", _engine.PLAN_ROUNDS: "rounds", _engine.PLAN_NONFINITE: "nonfinite",
             _engine.PLAN_INVALID_END: "invalid_end", _engine.PLAN_NODES: "nodes", _engine.PLAN_LONG: "long"}
    info = [dict(status=names[int(status[b])], rounds_used=int(rounds_used[b]), edges=int(edges[b]),
                 nodes=(int(tree_nodes[b, 0]), int(tree_nodes[b, 1]))) for b in range(len(q_inits))]
    return paths, info
