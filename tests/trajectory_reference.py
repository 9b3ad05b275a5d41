"""The NumPy statement of mjpl_topp_profile / mjpl_topp_sample (include/mjpl_hip.h): time-optimal
parameterisation of ONE path under velocity and acceleration limits, one IEEE operation per line of arithmetic, in the
order the kernels of mjpl_amd/csrc/mjpl_topp.h use.  `dtype` selects the arithmetic (np.float64 is what the kernels
compute; np.longdouble is what the conditioning guard of tests/test_trajectory_host.py compares it with).

The path is the natural cubic spline through the waypoints at uniform knots k / (n-1).  Over a grid of N = (n-1) G
intervals of width D = 1/N the unknowns are x_i = sdot^2 at the grid points and u_i = sddot on interval i, with
x_{i+1} = x_i + 2 D u_i.  Every constraint of interval i is a line in (u, x): per row (a column's acceleration at the
left or at the right end of the interval) a lower line u >= p + rho x and an upper line u <= P + rho x, and the two
reachability lines 0 <= x + 2 D u <= K_{i+1}.  K_i, the largest x_i from which the end is reachable, is the least
intersection of a lower with an upper line (backward sweep); the forward sweep takes the largest u at every point.
"""
import numpy as np

OK, STALLED, NONFINITE = 0, 1, 2  # MJPL_TOPP_*


def thomas_cprime(n, dtype=np.float64):
    """c'[k] of the Thomas recurrence of the system M[k-1] + 4 M[k] + M[k+1] = rhs[k] (k = 1 .. n-2)."""
    cp = np.zeros(max(n, 2), dtype)
    for k in range(1, n - 1):
        cp[k] = dtype(1) / (dtype(4) - cp[k - 1])
    return cp


def spline_second_derivatives(W, dtype=np.float64):
    """M[n][d]: the knot second derivatives of the natural cubic spline through W at the knots k / (n-1)."""
    W = np.asarray(W, dtype)
    n, d = W.shape
    M = np.zeros((n, d), dtype)
    if n == 2:
        return M
    cp = thomas_cprime(n, dtype)
    scale = dtype(6 * (n - 1) * (n - 1))  # 6 / h^2, exact
    for k in range(1, n - 1):
        rhs = ((W[k + 1] - W[k]) - (W[k] - W[k - 1])) * scale
        M[k] = (rhs - M[k - 1]) / (dtype(4) - cp[k - 1])
    for k in range(n - 3, 0, -1):
        M[k] = M[k] - cp[k] * M[k + 1]
    return M


def spline_eval(W, M, k, B):
    """(q, q', q'') on segment k at the local coordinate B in [0, 1] (s = (k + B) / (n-1))."""
    dtype = W.dtype.type
    r = dtype(W.shape[0] - 1)
    A = dtype(1) - B
    W0, W1, M0, M1 = W[k], W[k + 1], M[k], M[k + 1]
    q = (A * W0 + B * W1) + ((A * A * A - A) * M0 + (B * B * B - B) * M1) / (dtype(6) * r * r)
    q1 = (W1 - W0) * r + ((dtype(3) * B * B - dtype(1)) * M1 - (dtype(3) * A * A - dtype(1)) * M0) / (dtype(6) * r)
    q2 = A * M0 + B * M1
    return q, q1, q2


def spline_at(W, M, s):
    """(q, q', q'') at the path coordinate s, clamped to [0, 1]."""
    dtype = W.dtype.type
    n = W.shape[0]
    z = min(max(dtype(s), dtype(0)), dtype(1)) * dtype(n - 1)
    k = min(int(np.floor(z)), n - 2)
    return spline_eval(W, M, k, z - dtype(k))


def grid_derivatives(W, M, G):
    """a[N+1][d] = q'(s_i), b[N+1][d] = q''(s_i) at the grid points s_i = i / N, N = (n-1) G."""
    dtype = W.dtype.type
    n, d = W.shape
    N = (n - 1) * G
    a, b = np.zeros((N + 1, d), dtype), np.zeros((N + 1, d), dtype)
    for i in range(N + 1):
        k = min(i // G, n - 2)
        _, a[i], b[i] = spline_eval(W, M, k, dtype(i - k * G) / dtype(G))
    return a, b


def interval_lines(a0, b0, a1, b1, twoD, vmin, vmax, amin, amax):
    """The K-independent part of interval i: per row (2d of them: columns at the left end, then at the right end)
    the upper line (P, rho), the K-dependent quotient's operands (pp, g) -- the lower line u >= p + rho x meets the
    reachability line u <= (K - x) / 2D at x = (K - pp) g, pp = 2D p, g = 1 / (1 + 2D rho) -- and xs, the least of
    the velocity cap, the caps of rows without u, the intersections of the rows' lower and upper lines and the
    intersections of the upper lines with the reachability line u >= -x / 2D."""
    dtype = a0.dtype.type
    inf = dtype(np.inf)
    c = np.concatenate([a0, a1 + twoD * b1])
    bb = np.concatenate([b0, b1])
    lo, hi = np.concatenate([amin, amin]), np.concatenate([amax, amax])
    alive = c != 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = np.where(alive, np.where(c > 0, lo, hi) / c, -inf)
        P = np.where(alive, np.where(c > 0, hi, lo) / c, inf)
        rho = np.where(alive, -(bb / c), dtype(0))
        xs = inf
        # velocity: x <= (v* / a)^2 per moving column
        v = np.where(a0 > 0, vmax, vmin) / a0
        xs = min(xs, np.min(np.where(a0 != 0, v * v, inf)))
        # a row without u: b x <= amax (or >= amin)
        flat = ~alive & (bb != 0)
        xs = min(xs, np.min(np.where(flat, np.where(bb > 0, hi, lo) / bb, inf)))
        # lower line of row k against upper line of row l
        D = rho[:, None] - rho[None, :]
        ok = alive[:, None] & alive[None, :] & (D > 0)
        xs = min(xs, np.min(np.where(ok, (P[None, :] - p[:, None]) / D, inf)))
        # upper line of a row against u >= -x / 2D
        inv = dtype(1) / twoD
        e = -inv - rho
        xs = min(xs, np.min(np.where(alive & (e > 0), P / e, inf)))
        den = dtype(1) + twoD * rho
        live = alive & (den > 0)
        pp = np.where(live, p * twoD, -inf)
        g = np.where(live, dtype(1) / den, dtype(1))
    return P, rho, pp, g, xs


def profile(W, vmin, vmax, amin, amax, G, dtype=np.float64):
    """-> dict(M [n][d], x [N+1], u [N+1] (last 0), t [N+1] (last: the duration), K [N+1], a, b [N+1][d], status)."""
    W = np.asarray(W, dtype)
    vmin, vmax, amin, amax = (np.asarray(v, dtype) for v in (vmin, vmax, amin, amax))
    n, d = W.shape
    N = (n - 1) * G
    if not np.all(np.isfinite(W.astype(np.float64))):
        nan = np.full(N + 1, np.nan, dtype)
        return dict(M=np.full((n, d), np.nan, dtype), x=nan, u=nan.copy(), t=nan.copy(), K=nan.copy(), a=None, b=None,
                    status=NONFINITE)
    M = spline_second_derivatives(W, dtype)
    a, b = grid_derivatives(W, M, G)
    twoD = dtype(2) * (dtype(1) / dtype(N))
    lines = [interval_lines(a[i], b[i], a[i + 1], b[i + 1], twoD, vmin, vmax, amin, amax) for i in range(N)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        K = np.zeros(N + 1, dtype)
        for i in range(N - 1, -1, -1):
            P, rho, pp, g, xs = lines[i]
            K[i] = max(dtype(0), min(xs, np.min((K[i + 1] - pp) * g)))
        x = np.zeros(N + 1, dtype)
        for i in range(N):
            P, rho, pp, g, xs = lines[i]
            xn = x[i] + twoD * np.min(P + rho * x[i])
            x[i + 1] = min(max(xn, dtype(0)), K[i + 1])
        u = np.zeros(N + 1, dtype)
        u[:N] = (x[1:] - x[:-1]) / twoD
        t = np.zeros(N + 1, dtype)
        r = np.sqrt(x)
        for i in range(N):
            t[i + 1] = t[i] + twoD / (r[i] + r[i + 1])
    if np.any((x[:-1] == 0) & (x[1:] == 0)):
        status = STALLED
    elif not (np.all(np.isfinite(x)) and np.all(np.isfinite(u)) and np.all(np.isfinite(t)) and np.all(np.isfinite(M))):
        status = NONFINITE
    else:
        status = OK
    return dict(M=M, x=x, u=u, t=t, K=K, a=a, b=b, status=status)


def sample_count(T, dt):
    """Samples at dt, 2 dt, ... and a last one at T itself; a tail shorter than 1e-8 is dropped (float64 always)."""
    return max(int(np.ceil((np.float64(T) - 1e-8) / np.float64(dt))), 0)


def sample(W, prof, dt, dtype=np.float64):
    """-> pos, vel, acc [m][d] at t_k = min(k dt, T), k = 1 .. m."""
    W = np.asarray(W, dtype)
    M, x, u, t = prof["M"], prof["x"], prof["u"], prof["t"]
    N = len(x) - 1
    T = t[N]
    m = sample_count(T, dt)
    d = W.shape[1]
    pos, vel, acc = (np.zeros((m, d), dtype) for _ in range(3))
    for k in range(1, m + 1):
        tk = min(dtype(k) * dtype(dt), T)
        i = min(max(int(np.searchsorted(t, tk, side="right")) - 1, 0), N - 1)
        tau = tk - t[i]
        r = np.sqrt(x[i])
        sd = r + u[i] * tau
        s = dtype(i) / dtype(N) + (r * tau + dtype(0.5) * u[i] * tau * tau)
        q, q1, q2 = spline_at(W, M, s)
        pos[k - 1], vel[k - 1], acc[k - 1] = q, q1 * sd, q2 * (sd * sd) + q1 * u[i]
    return pos, vel, acc


def random_case(rng, d, n, walk=False, still_column=False):
    """Waypoints and symmetric limits as the parity cases draw them."""
    if walk:
        steps = rng.uniform(0.05, 0.5, (n - 1, d)) * rng.choice([-1.0, 1.0], (n - 1, d))
        W = np.vstack([np.zeros((1, d)), np.cumsum(steps, axis=0)]) + rng.uniform(-1, 1, d)
    else:
        W = rng.uniform(-1, 1, (n, d))
    if still_column and d > 1:
        W[:, d - 1] = W[0, d - 1]
    vmax, amax = rng.uniform(0.5, 2, d), rng.uniform(0.5, 3, d)
    return W, -vmax, vmax, -amax, amax


PARITY_GRID = 8
PARITY_DIMS = (1, 3, 4, 7, 16)  # (the pair count (2d + 1)^2 crosses 64 between 3 and 4)
PARITY_LENGTHS = (2, 3, 17, 64)


def parity_cases():
    """[(name, W, vmin, vmax, amin, amax)]: every d x n of the lists above (uniform waypoints for n <= 3, random walks
    beyond), one case with asymmetric limits and one with a column that never moves -- drawn from default_rng(11) in
    this order, so a case is the same wherever it is used.  test_trajectory_host.py guards their conditioning."""
    rng = np.random.default_rng(11)
    cases = []
    for d in PARITY_DIMS:
        for n in PARITY_LENGTHS:
            cases.append((f"d{d}-n{n}", *random_case(rng, d, n, walk=n >= 17)))
    W, vmin, vmax, amin, amax = random_case(rng, 4, 17, walk=True)
    cases.append(("asymmetric", W, -0.6 * vmax, vmax, -0.45 * amax, amax))
    cases.append(("still-column", *random_case(rng, 3, 17, walk=True, still_column=True)))
    return cases


_profiles = {}


def parity_profile(k, dtype=np.float64):
    """profile() of parity case k at PARITY_GRID, computed once per process and shared (do not write into it)."""
    if (k, dtype) not in _profiles:
        _, W, vmin, vmax, amin, amax = parity_cases()[k]
        _profiles[(k, dtype)] = profile(W, vmin, vmax, amin, amax, PARITY_GRID, dtype)
    return _profiles[(k, dtype)]


EDGE_SHAPES = (  # (name, d, n, G): N = (n-1) G
    ("N63", 7, 10, 7), ("N64", 7, 9, 8), ("N65", 7, 14, 5), ("N129", 16, 44, 3), ("G2", 4, 17, 2), ("G64", 3, 5, 64),
    ("d16-still-0-15", 16, 17, 8), ("d16-one-moving", 16, 17, 8))


def edge_cases():
    """[(name, W, vmin, vmax, amin, amax, G)]: what parity_cases() leaves out.  N % 64 in {63, 0, 1} around the forward
    sweep's blocks of 64 (N63, N64, N65, N129), grids that are no power of two (7, 5, 3: i / G is not exact) and the
    ends of the range tried (2, 64), still columns at d = 16 (rows 0, 15, 16 and 31 dead; one live column) -- random
    walks drawn from default_rng(23) in this order -- and three fixed paths with v = +-1, a = +-2 at G = 8: a column
    that reverses (q' = 0 exactly at the middle knot, q'' = -12 there: a row without u), the same beside a column that
    does not, and a repeated waypoint.  test_trajectory_host.py guards their conditioning like the parity cases'."""
    rng = np.random.default_rng(23)
    cases = []
    for name, d, n, G in EDGE_SHAPES:
        W, vmin, vmax, amin, amax = random_case(rng, d, n, walk=True)
        if name == "d16-still-0-15":
            W[:, [0, 15]] = W[0, [0, 15]]
        if name == "d16-one-moving":
            W[:, 1:] = W[0, 1:]
        cases.append((name, W, vmin, vmax, amin, amax, G))
    for name, W in (("reversal-1d", [[0.0], [1.0], [0.0]]), ("reversal-2d", [[0.0, 0.0], [1.0, 0.5], [0.0, 1.0]]),
                    ("repeat", [[0.0], [0.8], [0.8], [0.0]])):
        W = np.array(W)
        one = np.ones(W.shape[1])
        cases.append((name, W, -one, one, -2 * one, 2 * one, PARITY_GRID))
    return cases


def stalled_case():
    """(W, vmin, vmax, amin, amax, G) of a path the statement gives STALLED: at this scale every K underflows to 0, so x
    is all zero and t is inf from the first interval on (at 1e160 x would be subnormal instead, which no test wants)."""
    W = np.array([[0.0], [1.0], [0.3]]) * 1e170
    one = np.ones(1)
    return W, -one, one, -2 * one, 2 * one, PARITY_GRID


def edge_profile(k, dtype=np.float64):
    """profile() of edge case k at its own grid, computed once per process and shared (do not write into it)."""
    if ("edge", k, dtype) not in _profiles:
        _, W, vmin, vmax, amin, amax, G = edge_cases()[k]
        _profiles[("edge", k, dtype)] = profile(W, vmin, vmax, amin, amax, G, dtype)
    return _profiles[("edge", k, dtype)]
