"""Reference for `test_as betabin`: the beta-binomial model with one dispersion per row, written from its definition in
mpmath at 50 digits, the fit with a certificate of its maximum, and the seeded rows that the host and the GPU tests share.

Per sample y ~ BetaBinomial(n, a, b), a = mu (1 - rho)/rho, b = (1 - mu)(1 - rho)/rho, the binomial coefficient dropped:

    l(mu, rho) = sum_{i<y} ln(mu (1-rho) + i rho) + sum_{i<n-y} ln((1-mu)(1-rho) + i rho) - sum_{i<n} ln((1-rho) + i rho)

`loglik` is these three sums literally; `loglik_gamma` the same number through loggamma (rho > 0: lnB(a+y, b+n-y) - lnB(a, b);
rho = 0: the binomial y ln mu + (n-y) ln(1-mu), 0 ln 0 = 0), which is what makes rows of 10^5 reads a sample affordable.

The fit maximises over mu in [0, 1] (one per condition in the full model, one in the reduced) and rho in [0, RHO_MAX].  It locates
the maximum in double precision (SciPy's gammaln / digamma; a grid in rho, the concave inner problem in mu by Newton's method),
polishes it at 50 digits by Newton's method on the analytic gradient, and returns it with a certificate (`certify`):
  * every free coordinate's 50-digit derivative g and curvature c satisfy c < 0 and g^2/|c| < 1e-9;
  * every coordinate on a boundary (mu = 0, mu = 1, rho = 0, rho = RHO_MAX) has its derivative pointing out of the domain;
  * the double-precision profile over the rho grid has exactly one local maximum (rises and falls below GRID_NOISE, the noise of
    gammaln differences at these depths, do not count).
A row without a certificate is not a test row: `reference_rows` draws again until it has one.

`reference_rows` takes about a minute, so its result is kept in tests/golden/betabin/rows.json (`python tests/betabin_ref.py write`
rewrites it; `write-deep` the rows of DEEP_BANDS in deep_rows.json): the rows and, as 50-digit strings, the two maxima of each.  `golden_rows` reads it back; the numbers the tests compare
against (l_full, l_reduced, stat) are computed from the stored points on reading, and tests/test_betabin_reference_host.py
certifies every stored point afresh -- a certificate depends on the point, not on how it was found."""
import functools
import json
import math
import os

import mpmath as mp
import numpy as np
from scipy import optimize, special

DPS = 50
RHO_MAX_F = 0.999
MAX_CELL = 2.0 ** 40
GRID = np.concatenate([[0.0], np.logspace(-6.0, math.log10(RHO_MAX_F), 41)])
GRID[-1] = RHO_MAX_F
GRID_NOISE = 1e-6


def grid_noise(groups):
    """What the double-precision profile of these samples may be off by: gammaln is good to a few ulp of values as large as
    n ln(n + 1/rho), 1/rho up to 1e6 on GRID -- 1e-6 at the depths of BANDS, 5e-6 at 1e7 reads a sample, about 1 at 2^40, where a
    double cannot say more about l (which is itself 1e13 there)."""
    n = [nj for _, ns in groups for nj in ns]
    return max(GRID_NOISE, 2e-15 * sum(n) * math.log(max(n) + 1e6))
CERT_BOUND = 1e-9


def _rho_max():
    return mp.mpf(RHO_MAX_F)          # the double itself: the device's domain ends there too


# ---- the rules on a row ---------------------------------------------------------------------------------------------------

def prepare(count, total, n1, n2):
    """(y, n) as lists of ints after rounding half to even, or None where the row gets NA in every output."""
    c, t = np.rint(np.asarray(count, dtype=np.float64)), np.rint(np.asarray(total, dtype=np.float64))
    ok = lambda v: bool(np.all((v >= 0) & (v <= MAX_CELL)))         # NaN and the infinities fail the comparison
    if len(c) != n1 + n2 or len(t) != n1 + n2 or not ok(c) or not ok(t) or bool(np.any(c > t)):
        return None
    i1, i2 = int((t[:n1] > 0).sum()), int((t[n1:] > 0).sum())
    if i1 == 0 or i2 == 0 or i1 + i2 < 3:
        return None
    return [int(v) for v in c], [int(v) for v in t]


# ---- the log-likelihood ------------------------------------------------------------------------------------------------------

def _ln(v):
    return mp.ninf if v == 0 else mp.log(v)


def loglik(y, n, mu, rho):
    """The three sums, term by term, at DPS digits.  y, n: whole numbers per sample; one mu and one rho for all of them."""
    with mp.workdps(DPS):
        mu, rho = mp.mpf(mu), mp.mpf(rho)
        s = mp.mpf(0)
        for yj, nj in zip(y, n):
            for i in range(yj):
                s += _ln(mu * (1 - rho) + i * rho)
            for i in range(nj - yj):
                s += _ln((1 - mu) * (1 - rho) + i * rho)
            for i in range(nj):
                s -= _ln((1 - rho) + i * rho)
        return s


def _lg_diff(x, k):
    """loggamma(x + k) - loggamma(x) = sum_{i<k} ln(x + i); 0 for k = 0 whatever x is, -inf for x = 0 < k."""
    if k == 0:
        return mp.mpf(0)
    if x == 0:
        return mp.ninf
    return mp.loggamma(x + k) - mp.loggamma(x)


def loglik_gamma(y, n, mu, rho):
    """The same number through loggamma; the k ln rho of the three sums cancel (y + (n - y) - n = 0).  The loggammas themselves
    are as large as x ln x with x up to 1/rho + n, so they are taken with 20 digits to spare: the sum is good to DPS digits down
    to rho = 1e-12 at any depth the tool takes."""
    with mp.workdps(DPS + 20):
        mu, rho = mp.mpf(mu), mp.mpf(rho)
        s = mp.mpf(0)
        if rho == 0:
            for yj, nj in zip(y, n):
                if yj:
                    s += yj * _ln(mu)
                if nj - yj:
                    s += (nj - yj) * _ln(1 - mu)
            return s
        t = (1 - rho) / rho
        for yj, nj in zip(y, n):
            s += _lg_diff(mu * t, yj) + _lg_diff((1 - mu) * t, nj - yj) - _lg_diff(t, nj)
        return s


def loglik_full(y, n, n1, mu1, mu2, rho):
    """l of the full model at a given point: condition 1 (the first n1 samples) at mu1, condition 2 at mu2."""
    with mp.workdps(DPS):
        return loglik_gamma(y[:n1], n[:n1], mu1, rho) + loglik_gamma(y[n1:], n[n1:], mu2, rho)


# ---- derivatives at 50 digits ---------------------------------------------------------------------------------------------------

def _psi(order, x):
    """digamma (order 0) or trigamma (order 1); arguments below 40 are lifted there by the recurrence first, which mpmath's own
    trigamma does far more slowly"""
    lift = mp.mpf(0)
    if x < 40:
        for i in range(int(mp.ceil(40 - x))):
            lift += -1 / (x + i) if order == 0 else 1 / (x + i) ** 2
        x = x + int(mp.ceil(40 - x))
    return mp.psi(order, x) + lift


def _psi_diff(order, x, k):
    """psi_order(x + k) - psi_order(x); 0 for k = 0 whatever x is"""
    if k == 0:
        return mp.mpf(0)
    return _psi(order, x + k) - _psi(order, x)


def _group_derivs(y, n, mu, t):
    """Of l summed over one group's samples, in (mu, t), t = (1 - rho)/rho > 0: l_mu, l_t, l_mumu, l_tt, l_mut."""
    A, B = mu * t, (1 - mu) * t
    dA = dB = dT = tA = tB = tT = mp.mpf(0)
    for yj, nj in zip(y, n):
        dA += _psi_diff(0, A, yj); tA += _psi_diff(1, A, yj)
        dB += _psi_diff(0, B, nj - yj); tB += _psi_diff(1, B, nj - yj)
        dT += _psi_diff(0, t, nj); tT += _psi_diff(1, t, nj)
    return (t * (dA - dB), mu * dA + (1 - mu) * dB - dT, t * t * (tA + tB), mu * mu * tA + (1 - mu) ** 2 * tB - tT,
            (dA - dB) + t * (mu * tA - (1 - mu) * tB))


def _rho_slope_at_zero(y, n, mu):
    """dl/drho at rho = 0 of one group, from the three sums: d/drho ln(c (1-rho) + i rho) = (i - c)/c there."""
    s = mp.mpf(0)
    for yj, nj in zip(y, n):
        m = nj - yj
        if yj:
            s += (mp.mpf(yj) * (yj - 1) / 2 - yj * mu) / mu
        if m:
            s += (mp.mpf(m) * (m - 1) / 2 - m * (1 - mu)) / (1 - mu)
        s -= mp.mpf(nj) * (nj - 1) / 2 - nj
    return s


def _mu_status(y, n):
    sy, sm = sum(y), sum(n) - sum(y)
    return "zero" if sy == 0 else ("one" if sm == 0 else "free")


def certify(groups, mus, rho, grid_maxima=1):
    """The certificate of a maximum of sum over groups of l(mu_g, rho): groups = [(y, n), ...], one mu each.  True / False and the
    largest g^2/|c| over the free coordinates."""
    with mp.workdps(DPS):
        rho = mp.mpf(rho)
        mus = [mp.mpf(m) for m in mus]
        worst = mp.mpf(0)
        if grid_maxima != 1 or not (0 <= rho <= _rho_max()):
            return False, worst
        for (y, n), mu in zip(groups, mus):
            st = _mu_status(y, n)
            if (st == "zero" and mu != 0) or (st == "one" and mu != 1) or (st == "free" and not 0 < mu < 1):
                return False, worst
        if rho == 0:
            slope = mp.mpf(0)
            for (y, n), mu in zip(groups, mus):
                sy, sm = sum(y), sum(n) - sum(y)
                if _mu_status(y, n) == "free":       # binomial in mu: g = sy/mu - sm/(1-mu), c = -sy/mu^2 - sm/(1-mu)^2
                    g, c = sy / mu - sm / (1 - mu), -sy / mu ** 2 - sm / (1 - mu) ** 2
                    worst = max(worst, g * g / abs(c))
                # on a mu boundary the binomial's derivative points outward by its sign: -sm at mu = 0, +sy at mu = 1
                slope += _rho_slope_at_zero(y, n, mu)
            return bool(slope <= 0 and worst < CERT_BOUND), worst
        t = (1 - rho) / rho
        t1, t2 = -1 / rho ** 2, 2 / rho ** 3            # dt/drho, d2t/drho2
        l_t = l_tt = mp.mpf(0)
        for (y, n), mu in zip(groups, mus):
            g_mu, g_t, c_mu, c_t, _ = _group_derivs(y, n, mu, t)
            l_t += g_t; l_tt += c_t
            st = _mu_status(y, n)
            if st == "free":
                if not c_mu < 0:
                    return False, worst
                worst = max(worst, g_mu * g_mu / abs(c_mu))
            elif (st == "zero" and g_mu > 0) or (st == "one" and g_mu < 0):
                return False, worst
        g_rho, c_rho = l_t * t1, l_tt * t1 * t1 + l_t * t2
        if rho == _rho_max():
            return bool(g_rho >= 0 and worst < CERT_BOUND), worst
        if g_rho == 0 and c_rho == 0:                    # every group on a mu boundary: l does not depend on rho
            return bool(worst < CERT_BOUND), worst
        if not c_rho < 0:
            return False, worst
        worst = max(worst, g_rho * g_rho / abs(c_rho))
        return bool(worst < CERT_BOUND), worst


# ---- locating the maximum in double precision -----------------------------------------------------------------------------------------

def _solve_mu_double(y, m, t):
    """argmax over mu of one group at each t of an array (t = (1 - rho)/rho): safeguarded Newton on the concave l"""
    sy, sm = y.sum(), m.sum()
    if sy == 0 or sm == 0:
        return np.full(t.shape, 0.0 if sy == 0 else 1.0)
    mu = np.full(t.shape, sy / (sy + sm))
    lo, hi = np.zeros(t.shape), np.ones(t.shape)
    with np.errstate(all="ignore"):
        for _ in range(80):
            a, b = (mu * t)[:, None], ((1 - mu) * t)[:, None]
            g = (special.digamma(a + y) - special.digamma(a)).sum(1) - (special.digamma(b + m) - special.digamma(b)).sum(1)
            h = (special.polygamma(1, a) - special.polygamma(1, a + y)).sum(1) + (special.polygamma(1, b) - special.polygamma(1, b + m)).sum(1)
            lo = np.where(g > 0, mu, lo)
            hi = np.where(g < 0, mu, hi)
            nxt = mu + g / (t * h)
            nxt = np.where((nxt > lo) & (nxt < hi), nxt, 0.5 * (lo + hi))
            nxt = np.where(g == 0, mu, nxt)
            done = np.abs(nxt - mu) <= 1e-13 * np.minimum(nxt, 1 - nxt)
            mu = nxt
            if done.all():
                break
    return mu


def _lg_diff_double(x, k):
    with np.errstate(all="ignore"):
        return np.where(k > 0, special.gammaln(x + k) - special.gammaln(x), 0.0)


def _profile_double(groups, rhos):
    """max over the mu of l at each rho of an array, and the mu: (values [R], mus [G][R])"""
    rhos = np.asarray(rhos, dtype=np.float64)
    val, mus = np.zeros(rhos.shape), []
    pos = rhos > 0
    t = (1 - rhos[pos]) / rhos[pos]
    for y, n in groups:
        y, n = np.asarray(y, dtype=np.float64), np.asarray(n, dtype=np.float64)
        m = n - y
        mu = np.empty(rhos.shape)
        sy, sm = y.sum(), m.sum()
        mu0 = sy / (sy + sm)
        mu[~pos] = mu0
        val[~pos] += (sy * math.log(mu0) if sy else 0.0) + (sm * math.log1p(-mu0) if sm else 0.0)
        if pos.any():
            mp_ = _solve_mu_double(y, m, t)
            mu[pos] = mp_
            a, b = (mp_ * t)[:, None], ((1 - mp_) * t)[:, None]
            val[pos] += (_lg_diff_double(a, y) + _lg_diff_double(b, m) - _lg_diff_double(t[:, None], n)).sum(1)
        mus.append(mu)
    return val, mus


def count_maxima(f, tol):
    """local maxima of a sequence, the ends included; a rise or fall of at most tol does not count"""
    peaks, rising, ext = 0, True, f[0]
    for v in f[1:]:
        if rising:
            if v > ext:
                ext = v
            elif v < ext - tol:
                peaks, rising, ext = peaks + 1, False, v
        else:
            if v < ext:
                ext = v
            elif v > ext + tol:
                rising, ext = True, v
    return peaks + (1 if rising else 0)


# ---- polishing at 50 digits ----------------------------------------------------------------------------------------------------------

def _newton_mu_at(y, n, mu, t):
    """argmax over mu of one free group at a fixed t, from a start close to it"""
    for _ in range(60):
        g, _, c, _, _ = _group_derivs(y, n, mu, t)
        step = -g / c
        mu += step
        if not 0 < mu < 1:
            return None
        if abs(step) < mp.mpf(10) ** (-(DPS - 8)) * min(mu, 1 - mu):
            return mu
    return None


def _polish_interior(groups, mus, rho):
    """Newton on (the free mu, t) from the double-precision optimum"""
    free = [i for i, (y, n) in enumerate(groups) if _mu_status(y, n) == "free"]
    mus = list(mus)
    t = (1 - rho) / rho
    for _ in range(60):
        k = len(free)
        H, g = mp.zeros(k + 1, k + 1), mp.zeros(k + 1, 1)
        for i, (y, n) in enumerate(groups):
            g_mu, g_t, c_mu, c_t, c_mt = _group_derivs(y, n, mus[i], t)
            g[k] += g_t; H[k, k] += c_t
            if i in free:
                q = free.index(i)
                g[q] = g_mu; H[q, q] = c_mu; H[q, k] = c_mt; H[k, q] = c_mt
        if k == 0 and H[0, 0] == 0:
            return None
        try:
            step = mp.lu_solve(H, -g)
        except ZeroDivisionError:
            return None
        for q, i in enumerate(free):
            mus[i] += step[q]
            if not 0 < mus[i] < 1:
                return None
        t += step[k]
        if not t > 0:
            return None
        if max(abs(s) for s in step) < mp.mpf(10) ** (-(DPS - 10)) * min([t] + [min(mus[i], 1 - mus[i]) for i in free]):
            rho = 1 / (1 + t)
            return (mus, rho) if 0 < rho < _rho_max() else None
    return None


def fit_model(groups):
    """The maximum over (one mu per group, one rho) of the summed l, with its certificate.
    Returns dict(l, mus, rho, cert, worst, maxima) -- l, mus, rho as mpf."""
    val, mug = _profile_double(groups, GRID)
    maxima = count_maxima(val, grid_noise(groups))
    ib = int(np.argmax(val))
    lo, hi = GRID[max(ib - 1, 0)], GRID[min(ib + 1, len(GRID) - 1)]
    res = optimize.minimize_scalar(lambda r: -_profile_double(groups, [r])[0][0], bounds=(lo, hi), method="bounded",
                                   options={"xatol": 1e-9 * (hi - lo)})
    rho_d = float(res.x) if -res.fun >= val[ib] else float(GRID[ib])
    with mp.workdps(DPS):
        cands = []
        if ib <= 1:              # rho = 0 with the binomial's own maximum in each mu
            mus0 = [mp.mpf(sum(y)) / sum(n) for y, n in groups]
            cands.append((mus0, mp.mpf(0)))
        if ib >= len(GRID) - 2:  # rho = RHO_MAX with each free mu polished there
            t_hi = (1 - _rho_max()) / _rho_max()
            mus_hi = []
            for (y, n), m in zip(groups, mug):
                st = _mu_status(y, n)
                mus_hi.append(mp.mpf(0) if st == "zero" else (mp.mpf(1) if st == "one" else _newton_mu_at(y, n, mp.mpf(float(m[-1])), t_hi)))
            if all(m is not None for m in mus_hi):
                cands.append((mus_hi, _rho_max()))
        if 0 < rho_d < RHO_MAX_F:
            start = [mp.mpf(float(m[0])) for m in _profile_double(groups, [rho_d])[1]]
            pol = _polish_interior(groups, start, mp.mpf(rho_d))
            if pol:
                cands.append(pol)
        best = None
        for mus, rho in cands:
            ok, worst = certify(groups, mus, rho, maxima)
            l = sum((loglik_gamma(y, n, mu, rho) for (y, n), mu in zip(groups, mus)), mp.mpf(0))
            if best is None or (ok, l) > (best["cert"], best["l"]):
                best = dict(l=l, mus=mus, rho=rho, cert=ok, worst=worst, maxima=maxima)
        if best is None:         # nothing to polish: the double-precision optimum as it is, without a certificate
            mus = [mp.mpf(float(m[0])) for m in _profile_double(groups, [rho_d])[1]]
            l = sum((loglik_gamma(y, n, mu, rho_d) for (y, n), mu in zip(groups, mus)), mp.mpf(0))
            best = dict(l=l, mus=mus, rho=mp.mpf(rho_d), cert=False, worst=mp.inf, maxima=maxima)
        return best


def fit(count, total, n1, n2):
    """The reference's answer for one row: None for an NA row, else dict(y, n, stat, p, lf, lr, mu1, mu2, rho, cert, full, reduced)."""
    yn = prepare(count, total, n1, n2)
    if yn is None:
        return None
    y, n = yn
    full = fit_model([(y[:n1], n[:n1]), (y[n1:], n[n1:])])
    red = fit_model([(y, n)])
    with mp.workdps(DPS):
        stat = max(mp.mpf(0), 2 * (full["l"] - red["l"]))
        return dict(y=y, n=n, stat=float(stat), p=float(mp.erfc(mp.sqrt(stat / 2))), lf=full["l"], lr=red["l"],
                    mu1=float(full["mus"][0]), mu2=float(full["mus"][1]), rho=float(full["rho"]),
                    cert=bool(full["cert"] and red["cert"] and full["l"] >= red["l"] - mp.mpf(10) ** -30), full=full, reduced=red)


# ---- the rows of the tests ----------------------------------------------------------------------------------------------------------------

DESIGNS = [(1, 2), (2, 1), (2, 2), (3, 1), (3, 3), (8, 8)]
BANDS = [10, 10 ** 2, 10 ** 3, 10 ** 4, 10 ** 5]
DEEP_BANDS = [10 ** 6, 10 ** 7, 2 ** 40]          # measured; the tests hold the first two
KINDS = ["null_0.01", "null_0.1", "null_0.3", "null_0.1_again", "shift_up", "shift_down", "under", "zeros", "all_or_nothing", "with_empty"]


def _bb_draw(rng, n, mu, rho):
    a, b = mu * (1 - rho) / rho, (1 - mu) * (1 - rho) / rho
    return rng.binomial(n, rng.beta(a, b, size=len(n)))


def draw_row(kind, n1, n2, band, rng):
    """One row of `kind`: (count, total) as float arrays; totals uniform in [band/2, 3 band/2], and no higher than 2^40"""
    N = n1 + n2
    n = rng.integers(max(2, band // 2), min(band + band // 2, 2 ** 40) + 1, size=N)
    cond2 = np.arange(N) >= n1
    if kind.startswith("null"):
        y = _bb_draw(rng, n, rng.uniform(0.2, 0.8), float(kind.split("_")[1]))
    elif kind.startswith("shift"):
        mu1 = rng.uniform(0.3, 0.7)
        mu = np.where(cond2, mu1 + (0.2 if kind == "shift_up" else -0.2), mu1)
        rho = 0.05
        y = rng.binomial(n, rng.beta(mu * (1 - rho) / rho, (1 - mu) * (1 - rho) / rho))
    elif kind == "under":                        # every sample at the same ratio: closer than binomial draws
        y = np.rint(n * rng.uniform(0.3, 0.7)).astype(np.int64)
    elif kind == "zeros":                        # the smaller condition never shows the form
        y = _bb_draw(rng, n, rng.uniform(0.2, 0.8), 0.1)
        y[cond2 if n2 <= n1 else ~cond2] = 0
    elif kind == "all_or_nothing":               # every sample 0 or n, both in each condition of two or more
        pick = np.array([(j if j < n1 else j - n1) % 2 for j in range(N)])
        y = np.where(pick == 0, n, 0)
    elif kind == "with_empty":                   # a sample without reads, where three informative ones remain
        y = _bb_draw(rng, n, rng.uniform(0.2, 0.8), 0.1)
        if N >= 4:
            j = 0 if n1 >= n2 else n1                 # in the larger condition
            n[j], y[j] = 0, 0
    else:
        raise ValueError(kind)
    return y.astype(np.float64), n.astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference_rows(designs=tuple(DESIGNS), bands=tuple(BANDS)):
    """The rows of the fit tests with their reference answers: ten per design and band, one of each kind; each drawn again (up to
    20 times, seeded) until its fit carries a certificate.  A list of dict(design, band, kind, count, total, ref)."""
    rows = []
    for n1, n2 in designs:
        for band in bands:
            for k, kind in enumerate(KINDS):
                for attempt in range(20):
                    rng = np.random.default_rng([n1, n2, band, k, attempt])
                    count, total = draw_row(kind, n1, n2, band, rng)
                    ref = fit(count, total, n1, n2)
                    if ref is not None and ref["cert"] and _kind_holds(kind, ref):
                        break
                else:
                    raise RuntimeError("no certified row of kind %s for %d+%d at %d" % (kind, n1, n2, band))
                rows.append(dict(design=(n1, n2), band=band, kind=kind, count=count, total=total, ref=ref))
    return rows


def _kind_holds(kind, ref):
    """the boundary maxima that three kinds are there to show"""
    if kind == "under":
        return ref["rho"] == 0.0
    if kind == "zeros":
        return ref["mu1"] == 0.0 or ref["mu2"] == 0.0
    if kind == "all_or_nothing":
        return ref["rho"] == RHO_MAX_F
    return True


# ---- the rows on disk -------------------------------------------------------------------------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "betabin", "rows.json")
GOLDEN_DEEP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "betabin", "deep_rows.json")


def write_golden(path=GOLDEN, bands=tuple(BANDS)):
    out = []
    with mp.workdps(DPS):
        for r in reference_rows(bands=bands):
            f, d = r["ref"]["full"], r["ref"]["reduced"]
            out.append(dict(design=list(r["design"]), band=r["band"], kind=r["kind"], count=[int(v) for v in r["count"]], total=[int(v) for v in r["total"]],
                            full=dict(mus=[mp.nstr(m, DPS) for m in f["mus"]], rho=mp.nstr(f["rho"], DPS)),
                            reduced=dict(mus=[mp.nstr(m, DPS) for m in d["mus"]], rho=mp.nstr(d["rho"], DPS))))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in out) + "\n]\n")


def groups_of(y, n, n1, full):
    return [(y[:n1], n[:n1]), (y[n1:], n[n1:])] if full else [(y, n)]


@functools.lru_cache(maxsize=None)
def golden_rows(deep=False):
    """The rows of tests/golden/betabin/rows.json (deep: deep_rows.json, the bands of DEEP_BANDS) as `reference_rows` gives them,
    the answers computed from the stored maxima: dict(design, band, kind, count, total, ref = dict(y, n, stat, p, lf, lr, mu1,
    mu2, rho, full, reduced))."""
    rows = []
    with mp.workdps(DPS):
        for r in json.load(open(GOLDEN_DEEP if deep else GOLDEN)):
            n1, n2 = r["design"]
            count, total = np.array(r["count"], dtype=np.float64), np.array(r["total"], dtype=np.float64)
            y, n = prepare(count, total, n1, n2)
            models = {}
            for name in ("full", "reduced"):
                mus, rho = [mp.mpf(m) for m in r[name]["mus"]], mp.mpf(r[name]["rho"])
                if abs(rho - _rho_max()) < mp.mpf(10) ** -(DPS - 5):       # the double 0.999 has more than DPS decimal digits
                    rho = _rho_max()
                l = sum((loglik_gamma(gy, gn, mu, rho) for (gy, gn), mu in zip(groups_of(y, n, n1, name == "full"), mus)), mp.mpf(0))
                models[name] = dict(mus=mus, rho=rho, l=l)
            stat = max(mp.mpf(0), 2 * (models["full"]["l"] - models["reduced"]["l"]))
            f = models["full"]
            ref = dict(y=y, n=n, stat=float(stat), p=float(mp.erfc(mp.sqrt(stat / 2))), lf=f["l"], lr=models["reduced"]["l"],
                       mu1=float(f["mus"][0]), mu2=float(f["mus"][1]), rho=float(f["rho"]), full=f, reduced=models["reduced"])
            rows.append(dict(design=(n1, n2), band=r["band"], kind=r["kind"], count=count, total=total, ref=ref))
    return rows


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["write"]:
        write_golden()
        print("wrote", GOLDEN)
    if sys.argv[1:] == ["write-deep"]:
        write_golden(GOLDEN_DEEP, tuple(DEEP_BANDS))
        print("wrote", GOLDEN_DEEP)
