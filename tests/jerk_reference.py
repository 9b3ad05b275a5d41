"""The NumPy statement of mjpl_jerk_profile / mjpl_jerk_sample (include/mjpl_hip.h): a jerk-limited
parameterisation of ONE path by junction-speed lookahead, one IEEE operation per line of arithmetic, in the order the
kernels of mjpl_amd/csrc/mjpl_jerk.h use.  `dtype` selects the arithmetic (np.float64 is what the kernels compute;
np.longdouble is what the precision guard of tests/test_jerk_host.py compares it with).

The path is the natural cubic spline of tests/trajectory_reference.py.  Over a grid of N = (n-1) G intervals of width
D = 1/N the path speed sdot is v_i at junction i with sddot = 0 there; inside interval i it ramps from v_i up to a peak
vp_i, cruises for tc_i and ramps down to v_{i+1}, every ramp a jerk-limited S-curve under the interval's own scalar
limits (V_i, A_i, J_i) on (sdot, |sddot|, |sdddot|).  Those are chosen from the exact maxima of |q'|, |q''|, |q'''|
over the interval so that every column keeps its velocity, acceleration and jerk limit at every instant.
"""
import numpy as np

from trajectory_reference import sample_count, spline_eval, spline_second_derivatives

OK, STALLED, NONFINITE = 0, 1, 2  # MJPL_TOPP_*
ROUNDS, LANES = 10, 64
_quiet = dict(divide="ignore", invalid="ignore", over="ignore")


def cbrt(x):
    """The cube root of a scalar x > 0 as the kernels compute it: the seed 2^ceil(e / 3) for x = m 2^e (0.5 <= m < 1),
    at most twice the root, and eight Newton steps from above.  0, inf and NaN are returned as they are."""
    dtype = type(x)
    if not (x > 0) or not (x < np.inf):
        return x
    _, e = np.frexp(x)
    e = int(e)
    y = np.ldexp(dtype(1), (e + 2) // 3 if e > 0 else -((-e) // 3))
    for _ in range(8):
        y = (dtype(2) * y + x / (y * y)) / dtype(3)
    return y


def interval_bounds(W, M, G, i):
    """(p1, p2, p3) [d]: the maxima of |q'|, |q''| and |q'''| of every column over grid interval i."""
    dtype = W.dtype.type
    n = W.shape[0]
    k = min(i // G, n - 2)
    B0, B1 = dtype(i - k * G) / dtype(G), dtype(i + 1 - k * G) / dtype(G)
    _, a0, b0 = spline_eval(W, M, k, B0)
    _, a1, b1 = spline_eval(W, M, k, B1)
    p1 = np.maximum(np.abs(a0), np.abs(a1))
    with np.errstate(**_quiet):
        inside = b0 * b1 < 0  # q'' changes sign: q' has its vertex inside
        Bv = B0 + (b0 / (b0 - b1)) * (B1 - B0)
        for j in np.nonzero(inside)[0]:
            _, av, _ = spline_eval(W[:, j:j + 1], M[:, j:j + 1], k, Bv[j])
            p1[j] = max(p1[j], abs(av[0]))
    p2 = np.maximum(np.abs(b0), np.abs(b1))
    p3 = np.abs(M[k + 1] - M[k]) * dtype(n - 1)
    return p1, p2, p3


def interval_limits(p1, p2, p3, vlim, alim, jlim):
    """(V, A, J) of one interval.  A term with a zero denominator is +inf."""
    dtype = p1.dtype.type
    inf = dtype(np.inf)
    with np.errstate(**_quiet):
        V = np.min(np.where(p1 != 0, vlim / p1, inf))
        V = min(V, np.min(np.where(p2 != 0, np.sqrt(alim / (dtype(2) * p2)), inf)))
        V = min(V, min(cbrt(jlim[j] / (dtype(3) * p3[j])) if p3[j] != 0 else inf for j in range(len(p3))))
        if not V < inf:
            return V, inf, inf
        A = np.min(np.where(p1 != 0, (alim - p2 * (V * V)) / p1, inf))
        A = min(A, np.min(np.where(p2 != 0, jlim / ((dtype(9) * p2) * V), inf)))
        J = np.min(np.where(p1 != 0, ((jlim - p3 * ((V * V) * V)) - ((dtype(3) * p2) * V) * A) / p1, inf))
    return V, A, J


def ramp_time(dv, A, J):
    """The duration of a speed change dv >= 0 with zero acceleration at both ends (dv a scalar or an array)."""
    dtype = type(A)
    with np.errstate(**_quiet):
        return np.where(dv >= (A * A) / J, dv / A + A / J, dtype(2) * np.sqrt(dv / J))


def ramp_length(va, vb, A, J):
    """The length of the ramp between the speeds va <= vb."""
    dtype = type(A)
    return ((va + vb) * dtype(0.5)) * ramp_time(vb - va, A, J)


def ramp_phases(dv, A, J):
    """(tj, ta): the ramp is tj of jerk +-J, ta of constant acceleration, tj of jerk -+J."""
    dtype = type(A)
    with np.errstate(**_quiet):
        if dv >= (A * A) / J:
            tj = A / J
            return tj, dv / A - tj
        return np.sqrt(dv / J), dtype(0)


def section_search(f, lo, hi, h):
    """The largest feasible argument of the monotone f in [lo, hi] (f(lo) <= h): ten rounds of 64 candidates."""
    dtype = type(h)
    if f(hi) <= h:
        return hi
    frac = (np.arange(LANES) + 1).astype(dtype) / dtype(LANES)
    for _ in range(ROUNDS):
        c = lo + (hi - lo) * frac
        ok = f(c) <= h
        m = LANES if ok.all() else int(np.argmin(ok))  # the leading feasible candidates
        lo, hi = (c[m - 1] if m > 0 else lo), (c[m] if m < LANES else hi)
    return lo


def profile(W, vlim, alim, jlim, G, dtype=np.float64):
    """-> dict(M [n][d], lim [N+1][3] (V, A, J; last row 0), v [N+1], vp, tc [N+1] (last 0), t [N+1] (last: the
    duration), status).  The search of the junction speeds runs over the speed itself, v_{i+1} + Delta, so that the
    interval profile below finds the very ramp the sweep admitted (the same operations on the same operands)."""
    W = np.asarray(W, dtype)
    vlim, alim, jlim = (np.asarray(v, dtype) for v in (vlim, alim, jlim))
    n, d = W.shape
    N = (n - 1) * G
    nan = np.full(N + 1, np.nan, dtype)
    failed = dict(M=np.full((n, d), np.nan, dtype), lim=np.full((N + 1, 3), np.nan, dtype), v=nan, vp=nan.copy(),
                  tc=nan.copy(), t=nan.copy(), status=NONFINITE)
    if not np.all(np.isfinite(W.astype(np.float64))):
        return failed
    M = spline_second_derivatives(W, dtype)
    D = dtype(1) / dtype(N)
    zero, inf = dtype(0), dtype(np.inf)
    lim = np.zeros((N + 1, 3), dtype)
    for i in range(N):
        lim[i] = interval_limits(*interval_bounds(W, M, G, i), vlim, alim, jlim)
    if not np.all(np.isfinite(M)) or np.any(np.isnan(lim)):
        return failed
    V, A, J = lim[:, 0], lim[:, 1], lim[:, 2]
    v, vp, tc, t = (np.zeros(N + 1, dtype) for _ in range(4))
    if np.any(np.isinf(V[:N])):  # the path does not move there: it takes for ever
        tc[:N] = inf
        t[1:] = inf
        return dict(M=M, lim=lim, v=v, vp=vp, tc=tc, t=t, status=STALLED)
    # junction speeds: backward, then forward
    for i in range(N - 1, -1, -1):
        c = zero if i == 0 else min(V[i - 1], V[i])
        v[i] = c if c <= v[i + 1] else section_search(lambda x: ramp_length(v[i + 1], x, A[i], J[i]), v[i + 1], c, D)
    for i in range(N):
        if v[i + 1] > v[i]:
            v[i + 1] = section_search(lambda x: ramp_length(v[i], x, A[i], J[i]), v[i], v[i + 1], D)
    # interval profiles
    dur = np.zeros(N, dtype)
    with np.errstate(**_quiet):
        for i in range(N):
            both = lambda x: ramp_length(v[i], x, A[i], J[i]) + ramp_length(v[i + 1], x, A[i], J[i])
            vp[i] = section_search(both, max(v[i], v[i + 1]), V[i], D)
            tc[i] = max((D - both(vp[i])) / vp[i], zero)
            dur[i] = (ramp_time(vp[i] - v[i], A[i], J[i]) + tc[i]) + ramp_time(vp[i] - v[i + 1], A[i], J[i])
        for i in range(N):
            t[i + 1] = t[i] + dur[i]
    if not all(np.all(np.isfinite(a)) for a in (v, vp, tc, t)):
        return failed
    return dict(M=M, lim=lim, v=v, vp=vp, tc=tc, t=t, status=OK)


def interval_phases(prof, i):
    """[(duration, jerk)] * 7 of interval i: the ramp up, the cruise, the ramp down."""
    v, vp, tc, A, J = prof["v"], prof["vp"][i], prof["tc"][i], prof["lim"][i, 1], prof["lim"][i, 2]
    zero = type(A)(0)
    uj, ua = ramp_phases(vp - v[i], A, J)
    dj, da = ramp_phases(vp - v[i + 1], A, J)
    return [(uj, J), (ua, zero), (uj, -J), (tc, zero), (dj, -J), (da, zero), (dj, J)]


def advance(state, h, jk):
    """(s, sdot, sddot) after the time h of constant path jerk jk."""
    s, sd, sdd = state
    dtype = type(h)
    h2 = h * h
    return (s + ((sd * h + (dtype(0.5) * sdd) * h2) + (jk * (h2 * h)) / dtype(6)), sd + (sdd * h + (dtype(0.5) * jk) * h2),
            sdd + jk * h)


def interval_state(prof, i, tau):
    """(s, sdot, sddot, sdddot) local to interval i at the time tau after its start (s is clamped to [0, D])."""
    dtype = prof["t"].dtype.type
    tau = dtype(tau)
    N = len(prof["v"]) - 1
    D = dtype(1) / dtype(N)
    zero = dtype(0)
    state, jk, inside = (zero, prof["v"][i], zero), zero, False
    if not tau >= prof["t"][i + 1] - prof["t"][i]:
        for h, j in interval_phases(prof, i):
            if tau < h:
                state, jk, inside = advance(state, tau, j), j, True
                break
            state, tau = advance(state, h, j), tau - h
    if not inside:
        state, jk = (D, prof["v"][i + 1], zero), zero
    return min(max(state[0], zero), D), state[1], state[2], jk


def sample(W, prof, dt, dtype=np.float64):
    """-> pos, vel, acc [m][d] at t_k = min(k dt, T), k = 1 .. m."""
    W = np.asarray(W, dtype)
    M, t = prof["M"], prof["t"]
    N = len(t) - 1
    n, d = W.shape
    T = t[N]
    m = sample_count(T, dt)
    pos, vel, acc = (np.zeros((m, d), dtype) for _ in range(3))
    for k in range(1, m + 1):
        tk = min(dtype(k) * dtype(dt), T)
        i = min(max(int(np.searchsorted(t, tk, side="right")) - 1, 0), N - 1)
        sl, sd, sdd, _ = interval_state(prof, i, tk - t[i])
        s = dtype(i) / dtype(N) + sl
        z = min(max(s, dtype(0)), dtype(1)) * dtype(n - 1)
        seg = min(int(np.floor(z)), n - 2)
        q, q1, q2 = spline_eval(W, M, seg, z - dtype(seg))
        pos[k - 1], vel[k - 1], acc[k - 1] = q, q1 * sd, q2 * (sd * sd) + q1 * sdd
    return pos, vel, acc


def joint_derivatives(W, prof, i, tau):
    """(vel, acc, jerk) [d] of every column at the time tau into interval i, the jerk analytic:
    q''' sdot^3 + 3 q'' sdot sddot + q' sdddot."""
    dtype = W.dtype.type
    n = W.shape[0]
    N = len(prof["v"]) - 1
    sl, sd, sdd, sddd = interval_state(prof, i, tau)
    z = min(max(dtype(i) / dtype(N) + sl, dtype(0)), dtype(1)) * dtype(n - 1)
    seg = min(int(np.floor(z)), n - 2)
    _, q1, q2 = spline_eval(W, prof["M"], seg, z - dtype(seg))
    q3 = (prof["M"][seg + 1] - prof["M"][seg]) * dtype(n - 1)
    return q1 * sd, q2 * (sd * sd) + q1 * sdd, (q3 * ((sd * sd) * sd) + (dtype(3) * q2) * (sd * sdd)) + q1 * sddd


# ---- the cases the tests share

def random_case(rng, d, n, still_column=False, repeat=False):
    """Waypoints (uniform for n <= 3, a random walk beyond) and limit magnitudes."""
    if n > 3:
        steps = rng.uniform(0.05, 0.5, (n - 1, d)) * rng.choice([-1.0, 1.0], (n - 1, d))
        W = np.vstack([np.zeros((1, d)), np.cumsum(steps, axis=0)]) + rng.uniform(-1, 1, d)
    else:
        W = rng.uniform(-1, 1, (n, d))
    if still_column and d > 1:
        W[:, d - 1] = W[0, d - 1]
    if repeat:
        W[n // 2] = W[n // 2 - 1]
    return W, rng.uniform(0.5, 2, d), rng.uniform(1, 4, d), rng.uniform(5, 20, d)


PARITY_DIMS = (1, 3, 7, 16)
PARITY_LENGTHS = (2, 3, 17)
PARITY_GRIDS = (1, 2, 4)


def parity_cases():
    """[(name, W, vlim, alim, jlim, G)]: every d x n of the lists above, the grid going round 1, 2, 4; one case whose
    limits come from asymmetric minima (the class's rule min(max, -min)), one with a column that never moves and one
    with a repeated waypoint -- drawn from default_rng(31) in this order."""
    rng = np.random.default_rng(31)
    cases = []
    for a, d in enumerate(PARITY_DIMS):
        for b, n in enumerate(PARITY_LENGTHS):
            G = PARITY_GRIDS[(a + b) % 3]
            cases.append((f"d{d}-n{n}-G{G}", *random_case(rng, d, n), G))
    W, vlim, alim, jlim = random_case(rng, 4, 17)
    cases.append(("asymmetric", W, np.minimum(vlim, 0.6 * vlim), np.minimum(alim, 0.45 * alim), jlim, 2))
    cases.append(("still-column", *random_case(rng, 3, 17, still_column=True), 2))
    cases.append(("repeat", *random_case(rng, 3, 9, repeat=True), 4))
    return cases


EDGE_SHAPES = (("N63", 7, 10, 7), ("N64", 3, 9, 8), ("N65", 3, 14, 5), ("N129", 16, 44, 3))  # (name, d, n, G)


def edge_cases():
    """[(name, W, vlim, alim, jlim, G)]: N % 64 in {63, 0, 1} around the sweeps' blocks of 64, from default_rng(37)."""
    rng = np.random.default_rng(37)
    return [(name, *random_case(rng, d, n), G) for name, d, n, G in EDGE_SHAPES]


_profiles = {}


def shared_profile(kind, k, dtype=np.float64):
    """profile() of parity_cases()[k] (kind "parity") or edge_cases()[k] ("edge"), computed once per process and shared
    (do not write into it)."""
    if (kind, k, dtype) not in _profiles:
        _, W, vlim, alim, jlim, G = (parity_cases() if kind == "parity" else edge_cases())[k]
        _profiles[(kind, k, dtype)] = profile(W, vlim, alim, jlim, G, dtype)
    return _profiles[(kind, k, dtype)]
