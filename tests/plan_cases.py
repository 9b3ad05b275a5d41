"""Inputs and invariant checks shared by tests/test_plan_host.py and tests/test_gpu_plan.py."""
import numpy as np

import plan_reference as ref
from mjpl_amd import scenes

# scenes.two_dof_ball(): ball r = 0.1, wall x in [0.5, 0.7], |y| <= 0.5.  In order: across the wall; free space (the
# direct edge); across; a start inside the wall; across, corner to corner; across, close to the wall on both sides.
BALL_PROBLEMS = (((0.0, 0.0), (1.2, 0.0)), ((0.0, 0.0), (-1.0, 1.0)), ((0.2, -0.3), (1.0, 0.3)), ((0.6, 0.0), (1.2, 0.0)),
                 ((-1.5, -1.5), (1.5, 1.5)), ((0.3, 0.55), (0.9, -0.55)))
BALL_LO, BALL_HI = np.array([-2.0, -2.0]), np.array([2.0, 2.0])
BALL_STEP = 0.02


def ball_ends():
    return np.array([p[0] for p in BALL_PROBLEMS], float), np.array([p[1] for p in BALL_PROBLEMS], float)


def franka_planning():
    """(model, planning columns, base configuration, lo, hi) of the headline scene."""
    model = scenes.franka_p(obstacles=True)
    qidx = scenes.planning_index(model, scenes.FRANKA_ARM_JOINTS)
    return model, qidx, model.keyframe("home").qpos.copy(), model.jnt_range[qidx, 0].copy(), model.jnt_range[qidx, 1].copy()


def random_ends(lo, hi, valid_configs, B, seed, repeats=(5,)):
    """B seeded pairs of valid configurations uniform in [lo, hi] (valid_configs: [N, d] -> bool [N]); the problems in
    `repeats` get q_goal = q_init.  -> (QI, QG) float64 [B, d]."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    Q = np.zeros((2 * B, len(lo)))
    need = np.ones(2 * B, bool)
    while need.any():
        idx = np.flatnonzero(need)
        cand = rng.uniform(lo, hi, size=(len(idx), len(lo)))
        ok = np.asarray(valid_configs(cand), dtype=bool)
        Q[idx[ok]] = cand[ok]
        need[idx[ok]] = False
    QI, QG = Q[:B].copy(), Q[B:].copy()
    for b in repeats:
        QG[b] = QI[b]
    return QI, QG


def check_invariants(QI, QG, res, valid_edges, epsilon, rounds):
    """What every result of the algorithm obeys, whatever the verdict."""
    for b in range(len(QI)):
        n = int(res["n_out"][b])
        if res["status"][b] != ref.SOLVED:
            assert n == 0 and not res["P"][b].any(), b
            continue
        assert 2 <= n <= rounds + 2, b
        assert res["rounds_used"][b] <= rounds
        P = res["P"][b, :n]
        assert P[0].tobytes() == QI[b].tobytes() and P[-1].tobytes() == QG[b].tobytes(), b
        assert not res["P"][b, n:].any()
        assert np.asarray(valid_edges(P[:-1], P[1:]), dtype=bool).all(), b
        # every segment but the junction's is an extension: at most epsilon long, up to the roundings of step()
        j = int(res["junction"][b])
        seg = np.sqrt(ref.d2(P[:-1], P[1:]))
        other = np.delete(seg, j)
        assert (other <= epsilon * (1.0 + 2.0 ** -50)).all(), (b, other.max() / epsilon - 1.0)


def check_rounds_prefix(QI, QG, lo, hi, valid_configs, valid_edges, long_run, R1, **params):
    """The state after rounds = R1 is the state of the longer run after R1 rounds."""
    short = ref.plan_paths(QI, QG, lo, hi, valid_configs, valid_edges, rounds=R1, **params)
    for b in range(len(QI)):
        ls, lr = int(long_run["status"][b]), int(long_run["rounds_used"][b])
        settled = ls in (ref.NONFINITE, ref.INVALID_END) or (ls == ref.SOLVED and lr <= R1) or (ls == ref.NODES and lr < R1)
        if settled:
            assert short["status"][b] == ls and short["rounds_used"][b] == lr and short["edges"][b] == long_run["edges"][b], b
            n = int(short["n_out"][b])
            assert n == long_run["n_out"][b] and short["P"][b, :n].tobytes() == long_run["P"][b, :n].tobytes(), b
            continue
        assert short["status"][b] == ref.ROUNDS and short["rounds_used"][b] == R1, b
        for k in range(4):  # the short run's trees are what the long run's were then: nodes are only ever appended
            mine, theirs = short["trees"][b][k], long_run["trees"][b][k]
            assert len(mine) <= len(theirs), b
            assert np.asarray(mine).tobytes() == np.asarray(theirs[:len(mine)]).tobytes(), (b, k)
