"""Inputs and invariant checks shared by tests/test_cplan_host.py and tests/test_gpu_cplan.py."""
import numpy as np

import cplan_reference as ref
from plan_cases import BALL_HI, BALL_LO, franka_planning  # noqa: F401  (the sampling box and the headline scene)

# scenes.two_dof_ball(): ball r = 0.1, wall x in [0.5, 0.7], |y| <= 0.5; the site's y is held in [0.3, 0.9].  In order:
# the straight line is blocked and the path goes over the wall inside the band; a free straight line; across, corner to
# corner of the band; a start inside the wall; across, from far away; across, close to the wall; a start outside the band.
BALL_PROBLEMS = (((0.0, 0.35), (1.2, 0.35)), ((0.0, 0.7), (1.2, 0.7)), ((0.2, 0.3), (1.0, 0.9)), ((0.6, 0.35), (1.2, 0.35)),
                 ((-1.5, 0.4), (1.5, 0.4)), ((0.3, 0.55), (0.9, 0.45)), ((0.0, 0.0), (1.2, 0.35)))
BALL_STATUS = (ref.SOLVED, ref.SOLVED, ref.SOLVED, ref.INVALID_END, ref.SOLVED, ref.SOLVED, ref.INVALID_END)
BALL_BAND, BALL_TOL, BALL_QSTEP = (0.3, 0.9), 1e-3, 0.1
BALL_STEP = 0.02
# epsilon < 2 q_step: at epsilon = 2 q_step the projection's "farther than 2 q_step from q_old" rule turns on roundings
BALL_PARAMS = dict(epsilon=0.1, chain=8, candidates=16, nodes=1024)
BALL_SEEDS = (0, 0x9E3779B97F4A7C15)


def ball_ends():
    return np.array([p[0] for p in BALL_PROBLEMS], float), np.array([p[1] for p in BALL_PROBLEMS], float)


def check_invariants(QI, QG, res, valid_edges, pose_valid, epsilon, q_step, max_rows):
    """What every result of the algorithm obeys, whatever the verdicts."""
    bound = max(epsilon, 2.0 * q_step) * (1.0 + 2.0 ** -50)
    for b in range(len(QI)):
        n = int(res["n_out"][b])
        if res["status"][b] != ref.SOLVED:
            assert n == 0 and not res["P"][b].any(), b
            continue
        assert 2 <= n <= max_rows, b
        P = res["P"][b, :n]
        assert P[0].tobytes() == QI[b].tobytes() and P[-1].tobytes() == QG[b].tobytes(), b
        assert not res["P"][b, n:].any()
        assert np.asarray(pose_valid(P), dtype=bool).all(), b
        fwd = np.asarray(res["forward"][b], dtype=bool)
        assert len(fwd) == n - 1, b
        QA = np.where(fwd[:, None], P[:-1], P[1:])
        QB = np.where(fwd[:, None], P[1:], P[:-1])
        assert np.asarray(valid_edges(QA, QB), dtype=bool).all(), b
        seg = np.sqrt(ref.d2(P[:-1], P[1:]))
        assert (seg <= bound).all(), (b, seg.max())


def check_rounds_prefix(QI, QG, lo, hi, verdicts, long_run, R1, **params):
    """The state after rounds = R1 is the state of the longer run after R1 rounds (verdicts: the four callables, in the
    order of cplan_reference.plan_paths_constrained)."""
    short = ref.plan_paths_constrained(QI, QG, lo, hi, *verdicts, rounds=R1, **params)
    for b in range(len(QI)):
        ls, lr = int(long_run["status"][b]), int(long_run["rounds_used"][b])
        settled = (ls in (ref.NONFINITE, ref.INVALID_END) or (ls in (ref.SOLVED, ref.LONG) and lr <= R1) or
                   (ls == ref.NODES and lr < R1))
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
