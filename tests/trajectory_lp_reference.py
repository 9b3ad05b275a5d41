"""An independent reference for the profile of mjpl_topp_profile (include/mjpl_hip.h, steps 1 - 6): the constraints of
step 4 handed to a linear-programming solver as inequalities, with no closed form anywhere.  It shares no code with
tests/trajectory_reference.py: the spline's derivatives come from scipy.interpolate.CubicSpline, K_i is the LP "maximise
x over (u, x)", x_{i+1} the LP "maximise u at x = x_i".  A constraint pair missing from the statement's closed form is
not missing here.  Slow (two LPs per grid point) and accurate to the solver's tolerances, not to rounding.
"""
import numpy as np
from scipy.interpolate import CubicSpline
from scipy.optimize import linprog

_OPTIONS = dict(primal_feasibility_tolerance=1e-10, dual_feasibility_tolerance=1e-10, presolve=False)


def _interval_rows(a0, b0, a1, b1, twoD, vmin, vmax, amin, amax, K_next):
    """A z <= h over z = (u, x): the constraints of interval i as header step 4 lists them."""
    A, h = [], []
    for j in range(len(a0)):
        if a0[j] != 0:  # x_i <= (v* / a)^2
            v = (vmax[j] if a0[j] > 0 else vmin[j]) / a0[j]
            A.append([0.0, 1.0]); h.append(v * v)
        # amin <= a u + b x <= amax at the left end; at the right end with x_{i+1} = x + 2D u written out
        for cu, cx in ((a0[j], b0[j]), (a1[j] + twoD * b1[j], b1[j])):
            A.append([cu, cx]); h.append(amax[j])
            A.append([-cu, -cx]); h.append(-amin[j])
    A.append([-twoD, -1.0]); h.append(0.0)     # 0 <= x + 2D u
    A.append([twoD, 1.0]); h.append(K_next)    # x + 2D u <= K_{i+1}
    return np.array(A), np.array(h)


def lp_profile(W, limits, G):
    """-> (K [N+1], x [N+1]) of the path through W under limits = (vmin, vmax, amin, amax) at G intervals per segment."""
    W = np.asarray(W, np.float64)
    vmin, vmax, amin, amax = (np.asarray(v, np.float64) for v in limits)
    n = W.shape[0]
    N = (n - 1) * G
    s = np.arange(N + 1) / N
    spline = CubicSpline(np.linspace(0.0, 1.0, n), W, bc_type="natural")
    a, b = spline(s, 1), spline(s, 2)
    twoD = 2.0 / N
    rows = [None] * N
    K = np.zeros(N + 1)
    for i in range(N - 1, -1, -1):
        A, h = _interval_rows(a[i], b[i], a[i + 1], b[i + 1], twoD, vmin, vmax, amin, amax, K[i + 1])
        rows[i] = (A, h)
        res = linprog([0.0, -1.0], A_ub=A, b_ub=h, bounds=[(None, None), (0.0, None)], method="highs", options=_OPTIONS)
        K[i] = max(res.x[1], 0.0) if res.status == 0 else 0.0  # (infeasible: no x_i reaches the end)
    x = np.zeros(N + 1)
    for i in range(N):
        A, h = rows[i]
        # x fixed at x_i: the rows become bounds on u alone
        res = linprog([-1.0], A_ub=A[:, :1], b_ub=h - A[:, 1] * x[i], bounds=[(None, None)], method="highs", options=_OPTIONS)
        if res.status != 0:
            raise RuntimeError(f"forward LP of interval {i}: {res.message}")
        x[i + 1] = min(max(x[i] + twoD * res.x[0], 0.0), K[i + 1])
    return K, x
