"""Multi-query planning: a roadmap whose edges are validated once on the GPU and then answer many queries."""
import numpy as np

from .. import engine as _engine


class Roadmap:
    """A probabilistic roadmap over full-``nq`` configurations: build once per scene, query many times.

    :func:`plan_paths` validates its edges again at every call.  A ``Roadmap`` pays for edge validation once --
    :meth:`build` joins every collision-free node to its ``k`` (1..32) nearest nodes within ``radius`` wherever
    ``collision`` (a :class:`mjpl_amd.CollisionConstraint`) finds the straight edge valid with waypoints ``step_dist``
    apart -- and then answers a batch of start/goal pairs with one edge launch (the direct edges and the ends'
    attachments to the graph) and a shortest-path search.  ``include/mjpl_hip.h`` (``mjpl_roadmap_build``,
    ``mjpl_roadmap_query``) states both algorithms; every result is deterministic.

    The graph lives in this object's arrays, not in the engine: ``nodes`` [N, nq], ``node_valid`` uint8 [N],
    ``row_off`` int32 [N + 1], ``adj`` int32 and ``weights`` float64 [2 N k] -- a symmetric CSR adjacency whose rows
    ascend by node index.  It is valid for the scene it was built in.

    Only the collision constraint is consulted, edges are sampled (not certified), nodes cannot be added to a built
    roadmap, and the neighbour search is quadratic in the number of nodes.
    """

    def __init__(self, collision, step_dist: float, radius: float, k: int = 8):
        _engine.Engine.roadmap_desc(radius, step_dist, k)  # (ValueError for a bad parameter)
        self.collision, self.step_dist, self.radius, self.k = collision, float(step_dist), float(radius), int(k)
        nq = collision.model.nq
        self.nodes = np.zeros((0, nq), np.float64)
        self.node_valid, self.row_off = np.zeros(0, np.uint8), np.zeros(1, np.int32)
        self.adj, self.weights = np.zeros(0, np.int32), np.zeros(0, np.float64)

    def build(self, nodes) -> "Roadmap":
        """Build the roadmap over ``nodes`` ([N, nq]; rows in collision or holding NaN / inf stay, as invalid nodes)."""
        nq = self.collision.model.nq
        Q = np.asarray(nodes, dtype=np.float64)
        Q = np.ascontiguousarray(Q.reshape(0, nq) if Q.size == 0 else Q)
        if Q.ndim != 2 or Q.shape[1] != nq:
            raise ValueError(f"nodes must be full configurations of {nq} entries, got {Q.shape}")
        if len(Q) > _engine.ROADMAP_MAX_NODES:
            raise ValueError(f"at most {_engine.ROADMAP_MAX_NODES} nodes, got {len(Q)}")
        self.collision._ensure_full()
        self.node_valid, self.row_off, self.adj, self.weights = self.collision.engine.roadmap_build(Q, self.radius, self.step_dist, self.k)
        self.nodes = Q.copy()
        return self

    def build_uniform(self, n: int, lo=None, hi=None, seed: int = 0) -> "Roadmap":
        """Build over the first ``n`` collision-free configurations of a seeded uniform stream in ``[lo, hi]`` (the
        model's joint ranges by default)."""
        model = self.collision.model
        n = int(n)
        lo = np.asarray(model.jnt_range[:, 0] if lo is None else lo, dtype=np.float64)
        hi = np.asarray(model.jnt_range[:, 1] if hi is None else hi, dtype=np.float64)
        if lo.shape != (model.nq,) or hi.shape != (model.nq,):
            raise ValueError(f"lo and hi must have {model.nq} entries, got {lo.shape} and {hi.shape}")
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()) or (lo > hi).any():
            raise ValueError("lo and hi must be finite, with lo <= hi")
        if not 0 <= n <= _engine.ROADMAP_MAX_NODES:
            raise ValueError(f"n must be 0..{_engine.ROADMAP_MAX_NODES}, got {n}")
        rng = np.random.default_rng(seed)
        kept, have = [], 0
        for _ in range(64):  # (draws of 2 n: a scene where fewer than one sample in 128 is free is not sampled uniformly)
            if have >= n:
                break
            cand = rng.uniform(lo, hi, size=(max(2 * n, 64), model.nq))
            free = cand[self.collision.valid_configs(cand)]
            kept.append(free)
            have += len(free)
        if have < n:
            raise ValueError(f"only {have} of {n} collision-free samples found in [lo, hi]")
        return self.build(np.concatenate(kept)[:n] if kept else np.zeros((0, model.nq)))

    def edges(self):
        """(pairs int32 [E, 2] with i < j, ascending; lengths float64 [E]) of the valid edges."""
        m = int(self.row_off[-1])
        src = np.repeat(np.arange(len(self.nodes), dtype=np.int32), np.diff(self.row_off))
        dst = self.adj[:m]
        up = src < dst
        return np.stack([src[up], dst[up]], axis=1), self.weights[:m][up].copy()

    def components(self) -> np.ndarray:
        """int64 [N]: the lowest node index of every node's connected component, -1 for an invalid row."""
        N = len(self.nodes)
        label = np.where(self.node_valid.astype(bool), np.arange(N), -1).astype(np.int64)
        pairs, _ = self.edges()
        changed = True
        while changed:  # (labels only fall; pointer jumping makes this a few passes)
            low = label.copy()
            np.minimum.at(low, pairs[:, 0], label[pairs[:, 1]])
            np.minimum.at(low, pairs[:, 1], label[pairs[:, 0]])
            ok = low >= 0
            low[ok] = low[low[ok]]
            changed = not np.array_equal(low, label)
            label = low
        return label

    def _ends(self, q_inits, q_goals):
        nq = self.collision.model.nq
        q_inits, q_goals = list(q_inits), list(q_goals)
        if len(q_inits) != len(q_goals):
            raise ValueError(f"{len(q_inits)} q_inits but {len(q_goals)} q_goals")
        QI = np.asarray(q_inits, dtype=np.float64).reshape(len(q_inits), -1) if q_inits else np.zeros((0, nq))
        QG = np.asarray(q_goals, dtype=np.float64).reshape(len(q_goals), -1) if q_goals else np.zeros((0, nq))
        if QI.shape != (len(q_inits), nq) or QG.shape != QI.shape:
            raise ValueError(f"q_inits and q_goals must be full configurations of {nq} entries, got {QI.shape} and {QG.shape}")
        return q_inits, q_goals, QI, QG

    def query_status(self, q_inits, q_goals, connections: int = 8, max_rows: int = 256):
        """The raw arrays of a query: (P float64 [B, max_rows, nq], n_out int32 [B], status int32 [B] -- the
        ``engine.ROADMAP_*`` values --, cost float64 [B])."""
        _engine.Engine.roadmap_query_desc(self.radius, self.step_dist, connections, max_rows)  # (ValueError for a bad parameter)
        _, _, QI, QG = self._ends(q_inits, q_goals)
        self.collision._ensure_full()
        return self.collision.engine.roadmap_query(self.nodes, self.node_valid, self.row_off, self.adj, self.weights, QI, QG, self.radius,
                                                   self.step_dist, connections, max_rows)

    def query(self, q_inits, q_goals, connections: int = 8, max_rows: int = 256):
        """Per problem the shortest path through the roadmap as a list of ``nq`` arrays -- the first and last are the
        caller's own objects -- or ``None`` where there is none: an end that is in collision or holds NaN / inf, ends
        that attach to different components (or to no node within ``radius``), or a path of more than ``max_rows``
        waypoints.  A pair whose straight edge is valid gets that edge.  Each end is attached to its ``connections``
        (1..32) nearest nodes.  The list is what :func:`plan_paths` returns, so :func:`smooth_paths` and
        ``generate_trajectories`` take it as it is (drop the ``None`` entries first)."""
        q_inits, q_goals = list(q_inits), list(q_goals)
        P, n_out, status, _ = self.query_status(q_inits, q_goals, connections, max_rows)
        return [[q_inits[b]] + [P[b, r].copy() for r in range(1, n_out[b] - 1)] + [q_goals[b]] if status[b] == _engine.ROADMAP_SOLVED else None
                for b in range(len(q_inits))]
