"""The references of the differential splicing tests (lsq_as.hip) at sequencing depth: Fisher's exact test and the Poisson
likelihood-ratio statistic in Python's decimal at 50 digits, the Wilcoxon checkers, and the table and row lists of
tests/test_as_reference_host.py and tests/test_as_precision_gpu.py.  No GPU, no library call: the standard library and NumPy.

fisher_ref    the hypergeometric pmf relative to its mode as running products of the exact integer ratios
              (m-t)(k-t) / ((t+1)(n-k+t+1)), no logarithm anywhere; walked outward on both sides until a term is below
              10^-340 of the mode's -- past the kernel's exp(-746) floor, so a p-value near 1e-300 keeps all its terms;
              R's rule p = sum over d(t) <= d(x) (1 + 1e-7) of d(t) / sum of d(t) on those numbers.  With it the gap:
              the smallest |d(t)/d(x) - (1 + 1e-7)| over all terms.  A table is admissible for a comparison only where the
              gap exceeds MIN_GAP: otherwise a last-bit difference decides whether a term counts.
lrt_ref       Newton's method on the Poisson log-likelihood in decimal (ln and exp are correctly rounded at the context's
              precision) for the kernel's designs, y = round(count) + 1, offset ln(round(total) + 1), until the step is
              below 10^-40; stat = 2 |l_full - l_reduced|.
wilcox_check  wilcox.test's rule with the exact counts in Python integers (moved here from test_as_gpu.py unchanged).
"""
import functools
import math
from decimal import Decimal, getcontext, localcontext
from fractions import Fraction

import numpy as np

PREC = 50
REL = Decimal(1) + Decimal(1) / Decimal(10 ** 7)      # fisher.test's relErr
CUT = Decimal(10) ** -340                             # a walk ends where a term is below this (the mode's term is 1)
MIN_GAP = 1e-10
MAX_CELL = 2 ** 40                                    # lsq_as.hip AS_MAX_CELL


# ---- Fisher -------------------------------------------------------------------------------------------------------------

def hyper_mode(m, n, k):
    """The kernel's starting point: floor((k+1)(m+1)/(m+n+2)) clipped to the support (an argmax of the pmf)."""
    lo, hi = max(0, k - n), min(k, m)
    return min(max(((k + 1) * (m + 1)) // (m + n + 2), lo), hi)


def _walk_side(m, n, k, mode, end):
    """d(t)/d(mode) for t = mode +- 1, +- 2, ... towards `end`, and for every i the sum of the terms from i on."""
    side, d, t = [], Decimal(1), mode
    if end > mode:
        while t < end:
            d = d * Decimal((m - t) * (k - t)) / Decimal((t + 1) * (n - k + t + 1))
            if d < CUT:
                break
            side.append(d)
            t += 1
    else:
        while t > end:
            d = d * Decimal(t * (n - k + t)) / Decimal((m - t + 1) * (k - t + 1))
            if d < CUT:
                break
            side.append(d)
            t -= 1
    tail, s = [Decimal(0)] * (len(side) + 1), Decimal(0)
    for i in range(len(side) - 1, -1, -1):
        s += side[i]
        tail[i] = s
    return side, tail


@functools.lru_cache(maxsize=2)
def _hyper_walk(m, n, k):
    """Both sides of the pmf of (m, n, k); tables that share their margins share the walk."""
    lo, hi = max(0, k - n), min(k, m)
    mode = hyper_mode(m, n, k)
    with localcontext() as ctx:
        ctx.prec = PREC
        return mode, _walk_side(m, n, k, mode, hi), _walk_side(m, n, k, mode, lo)


def _first_le(side, thr):
    """The first index of the non-increasing `side` whose term is <= thr."""
    a, b = 0, len(side)
    while a < b:
        h = (a + b) // 2
        if side[h] <= thr:
            b = h
        else:
            a = h + 1
    return a


def fisher_ref(A, B, C, D):
    """(p, gap) of the two-sided test on the table, fisher.test's rule at 50 digits; p as a float.

    The pmf falls monotonically on each side of the mode, so the terms counted are two tails, found by bisection, and the
    smallest |d(t)/d(x) - REL| over all terms lies at a term next to where a side crosses the threshold or at the mode:
    those are the terms looked at.  An x beyond the walked window has d(x) < CUT of the mode's: p = 0.0, gap inf."""
    A, B, C, D = int(A), int(B), int(C), int(D)
    m, n, k, x = A + B, C + D, A + C, A
    if max(0, k - n) == min(k, m):
        return 1.0, math.inf
    mode, (up, tail_up), (dn, tail_dn) = _hyper_walk(m, n, k)
    j = abs(x - mode)
    side_x = up if x > mode else dn
    if j > len(side_x):
        return 0.0, math.inf
    with localcontext() as ctx:
        ctx.prec = PREC
        dx = Decimal(1) if j == 0 else side_x[j - 1]
        thr = dx * REL
        num, near = Decimal(1) if 1 <= thr else Decimal(0), [Decimal(1)]
        for side, tail in ((up, tail_up), (dn, tail_dn)):
            i = _first_le(side, thr)
            num += tail[i]
            near += side[max(i - 1, 0):i + 1]
        gap = min(abs(d / dx - REL) for d in near)
        p = num / (Decimal(1) + tail_up[0] + tail_dn[0])
    return float(p), float(gap)


def fisher_ref_all_terms(A, B, C, D):
    """fisher_ref without the monotonicity argument: every term compared and counted one by one (small tables only)."""
    m, n, k, x = A + B, C + D, A + C, A
    if max(0, k - n) == min(k, m):
        return 1.0, math.inf
    mode, (up, _), (dn, _) = _hyper_walk(m, n, k)
    with localcontext() as ctx:
        ctx.prec = PREC
        d = dn[::-1] + [Decimal(1)] + up
        dx = d[len(dn) + x - mode]
        p = sum(v for v in d if v <= dx * REL) / sum(d)
        return float(p), float(min(abs(v / dx - REL) for v in d))


def fisher_ref_flat_top(A, B, C, D, window=256):
    """(p, gap) for a table whose x lies within `window` of the mode, from the 2 * window + 1 terms around the mode only.

    The terms outside the window are no larger than the window's two end terms.  Where both end terms are <= d(x) REL,
    every term outside is counted, so 1 - p is the sum of the window's terms above the threshold over the total.  At cells of
    2^40 the variance is 2^38 and d(t)/d(x) - 1 <= (64^2 - 0)/2^39 = 7.5e-9 for x within 64 of the mode: no term is above
    the threshold, the excluded sum is empty and p = 1 needs no total.  An excluded sum that is not empty would need the
    total (1 / pmf(mode)), which a walk of 4e7 terms or a log-gamma series would give: not needed by the tables here, so
    this raises instead of approximating."""
    A, B, C, D = int(A), int(B), int(C), int(D)
    m, n, k, x = A + B, C + D, A + C, A
    lo, hi = max(0, k - n), min(k, m)
    mode = hyper_mode(m, n, k)
    assert abs(x - mode) <= window and hi - mode > window and mode - lo > window
    with localcontext() as ctx:
        ctx.prec = PREC
        up = _walk_side(m, n, k, mode, mode + window)[0]
        dn = _walk_side(m, n, k, mode, mode - window)[0]
        d = dn[::-1] + [Decimal(1)] + up
        assert all(a <= b for a, b in zip(dn[1:], dn)) and all(a <= b for a, b in zip(up[1:], up)) and up[0] <= 1 and dn[0] <= 1
        dx = d[window + x - mode]
        thr = dx * REL
        assert up[-1] <= thr and dn[-1] <= thr
        if any(v > thr for v in d):
            raise NotImplementedError("a term above the threshold: the total would be needed")
        return 1.0, float(min(abs(v / dx - REL) for v in d))


def _sigma(m, n, k):
    N = m + n
    return math.sqrt(k * (m / N) * (n / N) * (N - k) / (N - 1))


def _tables_at(m, n, k, offsets):
    """Tables with the margins (m, n, k) and x = mode + offset."""
    mode = hyper_mode(m, n, k)
    out = []
    for off in offsets:
        x = mode + off
        t = (x, m - x, k - x, n - k + x)
        assert min(t) >= 0, (m, n, k, off)
        out.append(t)
    return out


# Null-ish tables at depth: balanced margins of cell scale c (a few units apart, so that no two margins are equal), and
# x = mode + round(z sigma).  z = +-36 is exp(-648) = 1e-281 of the mode's term at large c, well inside the kernel's
# exp(-746) floor (z = 38.6); z = +-39, +-40 lie beyond it.
DEPTH_SCALES = (10 ** 3, 10 ** 5, 10 ** 6, 10 ** 7, 10 ** 8)
DEPTH_Z = (0, 0.5, -0.5, 1, -1, 2.5, -2.5, 5, -5, 10, -10, 20, -20, 30, -30, 36, -36)
FLOOR_Z = (39, -39, 40, -40)


def _depth_margins(c):
    return 2 * c + 3, 2 * c - 4, 2 * c + 5


def fisher_depth_tables(c, zs=DEPTH_Z):
    m, n, k = _depth_margins(c)
    s = _sigma(m, n, k)
    return _tables_at(m, n, k, [round(z * s) for z in zs])


def fisher_deep_table():
    """The one table at cells of 10^9 (its reference walks 1.2e6 terms)."""
    return fisher_depth_tables(10 ** 9, (-2.5,))[0]


def fisher_skewed_tables():
    """c = 10^6: m : n = 1 : 1000 with k about m (mean 999, sigma 32), and k = 50 against m, n of 10^6 (51 terms)."""
    m, n, k = 10 ** 6, 10 ** 9 + 7, 10 ** 6 + 3
    s = _sigma(m, n, k)
    out = _tables_at(m, n, k, [round(z * s) for z in (0, 1, -1, 2.5, -2.5, 5, -5, 10, -10, 20, -20, 30)])
    m, n, k = 10 ** 6 + 11, 10 ** 6 - 2, 50
    return out + _tables_at(m, n, k, [o - hyper_mode(m, n, k) for o in (0, 1, 10, 24, 25, 26, 40, 49, 50)])


# Chunk edges: the kernel walks 64 terms a step.  Cells of a few hundred, so that the exact rule (math.comb) is the reference.
CHUNK_DIST = (1, 63, 64, 65, 127, 128, 129)
CHUNK_SPAN = (63, 64, 65, 128)


def fisher_chunk_x_tables():
    """|x - mode| exactly each of CHUNK_DIST, on both sides of the mode (mode 303 in a support of 6 .. 601)."""
    return _tables_at(601, 597, 603, [s * d for d in CHUNK_DIST for s in (1, -1)])


def _span_margins(d, upper):
    """Margins with lo = 0 and cells of a few hundred whose mode lies exactly d below hi (upper: k = n = d + 140, the first m
    that does it) or exactly d above lo (k = m = d + 140, the first n), and more than two chunks from the other end."""
    k = d + 140
    for v in range(k, 2000):
        m, n = (v, k) if upper else (k, v)
        mode = hyper_mode(m, n, k)
        if (k - mode == d and mode > 130) if upper else (mode == d and k - mode > 130):
            return m, n, k
    raise LookupError(d)


def fisher_chunk_span_tables():
    """hi - mode, then mode - lo, exactly each of CHUNK_SPAN; x at lo, beside and at the mode, and at hi."""
    out = []
    for d in CHUNK_SPAN:
        for upper in (True, False):
            m, n, k = _span_margins(d, upper)
            lo, hi, mode = max(0, k - n), min(k, m), hyper_mode(m, n, k)
            out += _tables_at(m, n, k, [lo - mode, -1, 0, 1, hi - mode])
    return out


# The declared limit of 2^40 a cell; small supports or small variances, so the reference is instant.
_L = MAX_CELL
LIMIT_TABLES = ((1000, _L, 1300, _L - 5), (_L, _L, 3, 5), (_L, 0, _L, 64))
LIMIT_P = (4.29e-10, 0.7266, 1.08e-19)                # the reference's p to the digits given, held in the host test
# x within 64 of the mode of a table whose every cell is about 2^40 (sigma = 2^19): fisher_ref_flat_top
LIMIT_FLAT_TABLES = ((_L, _L, _L, _L), (_L, _L - 1, _L, _L), (_L - 50, _L, _L, _L - 50))


# ---- LRT ----------------------------------------------------------------------------------------------------------------

def _solve(H, g):
    """H x = g for a small dense system in Decimal: Gaussian elimination with partial pivoting."""
    p = len(g)
    M = [list(H[i]) + [g[i]] for i in range(p)]
    for c in range(p):
        piv = max(range(c, p), key=lambda r: abs(M[r][c]))
        M[c], M[piv] = M[piv], M[c]
        for r in range(c + 1, p):
            f = M[r][c] / M[c][c]
            for q in range(c, p + 1):
                M[r][q] -= f * M[c][q]
    x = [Decimal(0)] * p
    for r in range(p - 1, -1, -1):
        x[r] = (M[r][p] - sum(M[r][q] * x[q] for q in range(r + 1, p))) / M[r][r]
    return x


def lrt_designs(n1, n2):
    """The kernel's full and reduced designs as rows of integers: (1, tissue, rep) against (1, rep); (1, tissue) against
    (1) when n1 = n2 = 1, where rep is aliased with the intercept."""
    tissue = [1] * n1 + [2] * n2
    rep = list(range(1, n1 + 1)) + list(range(1, n2 + 1))
    if n1 == 1 and n2 == 1:
        return [[1, t] for t in tissue], [[1] for _ in tissue]
    return [[1, t, r] for t, r in zip(tissue, rep)], [[1, r] for r in rep]


def _poisson_loglik(X, y, o):
    """max over beta of sum(y eta - exp(eta)), eta = X beta + o: Newton's method from glm.fit's start (one weighted
    least-squares step from mu = y + 0.1), a step halved while it lowers the log-likelihood, until Newton's step is below 10^-40."""
    n, p = len(y), len(X[0])

    def normal(w, v):
        H = [[sum(w[j] * X[j][a] * X[j][b] for j in range(n)) for b in range(p)] for a in range(p)]
        return H, [sum(v[j] * X[j][a] for j in range(n)) for a in range(p)]

    def at(beta):
        eta = [sum(X[j][a] * beta[a] for a in range(p)) + o[j] for j in range(n)]
        mu = [e.exp() for e in eta]
        return mu, sum(y[j] * eta[j] - mu[j] for j in range(n))

    mu = [v + Decimal("0.1") for v in y]
    z = [mu[j].ln() - o[j] + (y[j] - mu[j]) / mu[j] for j in range(n)]
    beta = _solve(*normal(mu, [mu[j] * z[j] for j in range(n)]))
    mu, ll = at(beta)
    tiny = Decimal(10) ** -40
    for _ in range(100):
        step = _solve(*normal(mu, [y[j] - mu[j] for j in range(n)]))
        size = max(abs(s) for s in step)
        slack = abs(ll) * Decimal(10) ** (5 - getcontext().prec)      # a fall within the rounding of ll itself is none
        while True:
            cand = [beta[a] + step[a] for a in range(p)]
            mu_c, ll_c = at(cand)
            if ll_c >= ll - slack:
                break
            step = [s / 2 for s in step]
        beta, mu, ll = cand, mu_c, ll_c
        if size < tiny:
            return ll
    raise ArithmeticError("Newton's method did not converge")


def lrt_ref_row(count, total, n1, n2, prec=PREC):
    """The statistic of one row as a Decimal."""
    with localcontext() as ctx:
        ctx.prec = prec
        y = [Decimal(int(np.rint(c)) + 1) for c in count]
        o = [Decimal(int(np.rint(t)) + 1).ln() for t in total]
        Xf, Xr = lrt_designs(n1, n2)
        return 2 * abs(_poisson_loglik(Xf, y, o) - _poisson_loglik(Xr, y, o))


def lrt_ref(count, total, n1, n2):
    """The statistics of the rows of count / total ([row][sample]) as float64."""
    return np.array([float(lrt_ref_row(c, t, n1, n2)) for c, t in zip(count, total)])


LRT_DESIGNS = ((1, 1), (2, 2), (8, 8), (1, 2), (2, 1), (1, 3), (3, 1))
LRT_BANDS = (("1e4", 1e4), ("1e6", 1e6), ("1e8", 1e8), ("1e10", 1e10), ("2^40", float(2 ** 40)))
LRT_NULL_PER_BAND = 8


@functools.lru_cache(maxsize=None)
def lrt_depth_rows(n1, n2):
    """(count, total, band) of a design's rows.  Per depth band LRT_NULL_PER_BAND null-ish rows -- one fraction f a row,
    count = round(f total + N(0, 1) sqrt(f total)), so the statistic is chi-square-like -- and two rows with a twofold
    change between the conditions; then a row of zero counts under totals of 2^40, a row of counts above its totals and a
    row with one sample's total 0 beside totals of 10^8 (band "edge").  Totals lie within a factor of two of the band's
    depth, at 2^40 within a factor of two below it."""
    rng = np.random.default_rng(1000 + 10 * n1 + n2)
    n = n1 + n2
    count, total, band = [], [], []
    for name, T in LRT_BANDS:
        for i in range(LRT_NULL_PER_BAND + 2):
            t = np.rint(T * rng.uniform(0.5, 1.0 if T == 2 ** 40 else 2.0, size=n))
            f = np.full(n, rng.uniform(0.05, 0.5))
            if i >= LRT_NULL_PER_BAND:
                f[n1:] *= 0.5 if i == LRT_NULL_PER_BAND else 2.0
            count.append(np.rint(f * t + rng.normal(size=n) * np.sqrt(f * t)))
            total.append(t)
            band.append(name)
    count.append(np.zeros(n)); total.append(np.full(n, float(2 ** 40)))
    t = np.rint(1e4 * rng.uniform(0.5, 2.0, size=n))
    count.append(np.rint(t * rng.uniform(3.0, 6.0, size=n))); total.append(t)
    t = np.rint(1e8 * rng.uniform(0.5, 2.0, size=n))
    c = np.rint(0.2 * t)
    t[0] = c[0] = 0.0
    count.append(c); total.append(t)
    band += ["edge"] * 3
    count, total = np.array(count), np.array(total)
    count.setflags(write=False)
    total.setflags(write=False)
    return count, total, tuple(band)


@functools.lru_cache(maxsize=None)
def lrt_depth_ref(n1, n2):
    count, total, _ = lrt_depth_rows(n1, n2)
    ref = lrt_ref(count, total, n1, n2)
    ref.setflags(write=False)
    return ref


# ---- Wilcoxon -----------------------------------------------------------------------------------------------------------

def r_mean(v):
    s = 0.0
    for a in v:
        s += a
    s /= len(v)
    if math.isfinite(s):
        t = 0.0
        for a in v:
            t += a - s
        s += t / len(v)
    return s


_wcounts = {}


def wilcox_counts(nx, ny):
    """cwilcox's counts in Python integers: f(w; a, b) = f(w - b; a - 1, b) + f(w; a, b - 1)."""
    if (nx, ny) not in _wcounts:
        W = nx * ny + 1
        F = [np.array([1] + [0] * (W - 1), dtype=object) for _ in range(nx + 1)]
        for b in range(1, ny + 1):
            for a in range(1, nx + 1):
                F[a][b:] = F[a][b:] + F[a - 1][:W - b]
        _wcounts[(nx, ny)] = [int(v) for v in F[nx]]
    return _wcounts[(nx, ny)]


def wilcox_check(row, n1):
    x = [v for v in row[:n1] if math.isfinite(v)]
    y = [v for v in row[n1:] if math.isfinite(v)]
    diff = math.nan if any(math.isnan(v) for v in row) else r_mean(list(row[:n1])) - r_mean(list(row[n1:]))
    if not x or not y:
        return diff, math.nan
    nx, ny = len(x), len(y)
    W = sum((a > b) + 0.5 * (a == b) for a in x for b in y)
    allv = x + y
    cnt = {}
    for v in allv:
        cnt[v] = cnt.get(v, 0) + 1
    ties = sum(t ** 3 - t for t in cnt.values())
    if nx < 50 and ny < 50 and ties == 0:
        f = wilcox_counts(nx, ny)
        W = int(W)
        P = Fraction(sum(f[W:]) if W > nx * ny / 2 else sum(f[:W + 1]), math.comb(nx + ny, nx))
        return diff, min(1.0, 2 * float(P))
    z = W - nx * ny / 2
    N = nx + ny
    sigma = math.sqrt((nx * ny / 12) * ((N + 1) - ties / (N * (N - 1))))
    if sigma == 0:
        return diff, math.nan
    z = (z - math.copysign(0.5, z) * (z != 0)) / sigma
    return diff, min(math.erfc(-z / math.sqrt(2)), math.erfc(z / math.sqrt(2)))
