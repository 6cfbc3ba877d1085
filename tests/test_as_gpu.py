"""The differential splicing tests on the device (lsq_as_*; test_as) against restatements of the rules in NumPy and
Python's math / fractions: Fisher's exact test, the Poisson LRT, the Wilcoxon rank-sum test, the corrections, and the
executable end to end on count / solve tables of four synthetic samples."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import lesseq_amd as L
from lesseq_amd import diffsplice as ds
from lesseq_amd.junctions import SORT_TILE

from as_ref import lrt_ref, wilcox_check

pytestmark = pytest.mark.gpu

REL = 1 + 1e-7


# ---- checkers ---------------------------------------------------------------------------------------------------------

def fisher_exact(A, B, C, D):
    """R's rule in exact arithmetic (tolerance 1 + 1e-7 as a rational)."""
    m, n, k, x = A + B, C + D, A + C, A
    lo, hi = max(0, k - n), min(k, m)
    d = [math.comb(m, t) * math.comb(n, k - t) for t in range(lo, hi + 1)]
    dx = d[x - lo]
    num = sum(v for v in d if v * 10 ** 7 <= dx * (10 ** 7 + 1))
    return float(Fraction(num, sum(d)))


def _mode(m, n, k):
    lo, hi = max(0, k - n), min(k, m)
    return min(max(((k + 1) * (m + 1)) // (m + n + 2), lo), hi)


def fisher_logratio(A, B, C, D, rel=REL, drop=None):
    """The same rule on log d(t)/d(mode) from cumulative sums of log ratios, over the window where terms are non-zero."""
    A, B, C, D = int(A), int(B), int(C), int(D)
    m, n, k, x = A + B, C + D, A + C, A
    lo, hi = max(0, k - n), min(k, m)
    if lo == hi:
        return 1.0
    N = m + n
    var = k * (m / N) * (n / N) * (N - k) / max(N - 1, 1)
    mode = _mode(m, n, k)
    w = int(40 * math.sqrt(var)) + 64
    a, b = max(lo, mode - w), min(hi, mode + w)
    if not a <= x <= b:
        return 0.0
    t = np.arange(a, b, dtype=np.float64)
    steps = np.log(((m - t) / (t + 1)) * ((k - t) / (n - k + t + 1)))
    Lg = np.concatenate([[0.0], np.cumsum(steps)])
    Lg -= Lg[mode - a]
    e = np.exp(Lg)
    thr = e[x - a] * rel
    keep = e <= thr
    if drop is not None:
        keep[drop - a] = False
    return float(e[keep].sum() / e.sum())


def lrt_check(count, total, n1, n2):
    """Newton's method on the Poisson log-likelihood (batched over rows) until the step is below 1e-12."""
    y = np.rint(count) + 1.0
    o = np.log(np.rint(total) + 1.0)
    n = n1 + n2
    tissue = np.array([1.0] * n1 + [2.0] * n2)
    rep = np.array(list(range(1, n1 + 1)) + list(range(1, n2 + 1)), dtype=np.float64)
    one = np.ones(n)
    if n1 == 1 and n2 == 1:
        Xf, Xr = np.stack([one, tissue], 1), one[:, None]
    else:
        Xf, Xr = np.stack([one, tissue, rep], 1), np.stack([one, rep], 1)

    def fit(X):
        # start: one weighted least-squares step from mu = y + 0.1
        mu = y + 0.1
        z = np.log(mu) - o + (y - mu) / mu
        H = np.einsum("rn,np,nq->rpq", mu, X, X)
        g = np.einsum("rn,np->rp", mu * z, X)
        beta = np.linalg.solve(H, g[..., None])[..., 0]
        for _ in range(200):
            eta = beta @ X.T + o
            mu = np.exp(eta)
            H = np.einsum("rn,np,nq->rpq", mu, X, X)
            g = np.einsum("rn,np->rp", y - mu, X)
            step = np.linalg.solve(H, g[..., None])[..., 0]
            beta = beta + step
            if np.abs(step).max() < 1e-12:
                break
        eta = beta @ X.T + o
        return (y * eta - np.exp(eta)).sum(1)

    stat = 2 * np.abs(fit(Xf) - fit(Xr))
    p = np.array([math.erfc(math.sqrt(s / 2)) for s in stat])
    return stat, p


def adjust_ref(p):
    p = np.asarray(p, dtype=np.float64)
    ok = ~np.isnan(p)
    n = int(ok.sum())
    if n <= 1:
        return p.copy(), p.copy()
    q = p[ok]
    o = np.argsort(q, kind="stable")
    v = (n / np.arange(1, n + 1)) * q[o]
    cm = np.minimum.accumulate(v[::-1])[::-1]
    bh_q = np.empty(n)
    bh_q[o] = np.minimum(1.0, cm)
    bon, bh = p.copy(), p.copy()
    bon[ok] = np.minimum(1.0, n * q)
    bh[ok] = bh_q
    return bon, bh


def close(a, b, rtol, floor=1e-300):
    """a, b equal within rtol, both NaN, or both below `floor`"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if abs(a) < floor and abs(b) < floor:
        return True
    return abs(a - b) <= rtol * max(abs(a), abs(b))


# ---- Fisher -------------------------------------------------------------------------------------------------------------

# Found by a search with the exact rule: a term on the far side of the mode has d(t) / d(x) - 1 = 2.3e-8, between 1e-14 and
# 1e-7, so R's tolerance counts it and SciPy's would not.
TIE_TABLE = (4355, 13661, 830, 2306)


def test_fisher_uses_r_tolerance(gpu_ctx):
    A, B, C, D = TIE_TABLE
    m, n, k, x = A + B, C + D, A + C, A
    mode = _mode(m, n, k)
    dx = math.comb(m, x) * math.comb(n, k - x)
    span = 2 * abs(mode - x) + 100
    far = range(mode + 1, min(min(k, m), mode + span) + 1) if x < mode else range(max(max(0, k - n), mode - span), mode)
    tied = [t for t in far if 0 < (math.comb(m, t) * math.comb(n, k - t) - dx) * 10 ** 7 <= dx]
    assert len(tied) == 1
    t = tied[0]
    assert (math.comb(m, t) * math.comb(n, k - t) - dx) * 10 ** 14 > dx          # not within SciPy's 1e-14
    p = ds.fisher(gpu_ctx, np.array([TIE_TABLE], dtype=np.float64))[0]
    p_r = fisher_logratio(A, B, C, D)
    p_scipy = fisher_logratio(A, B, C, D, drop=t)
    assert close(p, p_r, 1e-9), (p, p_r)
    assert not close(p, p_scipy, 1e-6), (p, p_scipy)


def test_fisher_regimes_and_edges(gpu_ctx):
    rng = np.random.default_rng(1)
    small = rng.integers(0, 21, size=(3000, 4))
    mid = rng.integers(0, 1001, size=(1500, 4))
    big = rng.integers(0, 10 ** 6 + 1, size=(490, 4))
    huge = rng.integers(0, 10 ** 9 + 1, size=(10, 4))
    edges = [[0, 0, 0, 0], [0, 0, 5, 7], [3, 0, 9, 0], [0, 4, 0, 6], [0, 0, 0, 9], [7, 0, 0, 0], [1, 0, 0, 1]]
    edges += [[a, b, b, a] for a in (0, 1, 2, 5, 30, 400) for b in (0, 1, 3, 17, 250)]
    cells = np.concatenate([small, mid, big, huge, np.array(edges)]).astype(np.float64)
    p = ds.fisher(gpu_ctx, cells)
    assert p.shape == (len(cells),)
    bad = []
    for i, c in enumerate(cells.astype(np.int64)):
        if i < 3000 or i >= 5000 or (3000 <= i < 3030):
            ref, rtol = fisher_exact(*map(int, c)), 1e-12
        else:
            ref, rtol = fisher_logratio(*c), 1e-9
        if not close(p[i], ref, rtol):
            bad.append((c.tolist(), p[i], ref))
    assert not bad, bad[:10]
    # symmetric tables tie on both sides of the mode exactly: p = 1 when x is the mode, and the two tails otherwise
    assert (p[-30:][[i * 5 for i in range(6)]] <= 1.0).all()


def test_fisher_na_negative_and_rounding(gpu_ctx):
    cells = np.array([[np.nan, 1, 2, 3], [1, -1, 2, 3], [1, 2, np.inf, 3], [2.5, 1.5, 3.5, 0.4], [2, 2, 4, 0]], dtype=np.float64)
    p = ds.fisher(gpu_ctx, cells)
    assert np.isnan(p[:3]).all()
    assert p[3] == p[4]            # rint: 2.5 -> 2, 1.5 -> 2, 3.5 -> 4, 0.4 -> 0
    assert close(p[4], fisher_exact(2, 2, 4, 0), 1e-12)


# ---- LRT ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n1,n2", [(1, 1), (2, 2), (2, 3), (4, 4), (8, 8)])
def test_lrt_against_newton(gpu_ctx, n1, n2):
    rng = np.random.default_rng(10 * n1 + n2)
    R, n = 2000, n1 + n2
    total = np.exp(rng.uniform(np.log(5), np.log(2e5), size=(R, n))).round()
    frac = np.concatenate([np.repeat(rng.uniform(0.05, 0.95, (R, 1)), n1, 1), np.repeat(rng.uniform(0.05, 0.95, (R, 1)), n2, 1)], 1)
    count = rng.poisson(total * frac).astype(np.float64)
    count[:20] = 0
    total[:20] = 0
    count[20:30] = rng.uniform(0, 50, size=(10, n))              # non-integers: rounded
    count[30, 0] = np.nan
    count[31, n - 1] = np.nan
    total[32, 1 % n] = np.nan
    stat, p = ds.lrt(gpu_ctx, count, total, n1, n2)
    assert np.isnan(stat[30:33]).all() and np.isnan(p[30:33]).all()
    keep = np.ones(R, bool)
    keep[30:33] = False
    rs, rp = lrt_check(count[keep], total[keep], n1, n2)
    gs, gp = stat[keep], p[keep]
    ds_ = np.abs(gs - rs) / np.maximum(1.0, rs)
    assert ds_.max() <= 1e-6, (ds_.argmax(), gs[ds_.argmax()], rs[ds_.argmax()])
    for a, b in zip(gp, rp):
        assert close(a, b, 1e-6), (a, b)
    assert ((gp >= 0) & (gp <= 1)).all()


# ---- Wilcoxon -----------------------------------------------------------------------------------------------------------

def _wilcox_case(gpu_ctx, value, n1, n2):
    diff, p = ds.wilcox(gpu_ctx, value, n1, n2)
    for i, row in enumerate(value):
        rd, rp = wilcox_check(list(row), n1)
        assert (math.isnan(rd) and math.isnan(diff[i])) or rd == diff[i], (i, row, diff[i], rd)
        assert close(p[i], rp, 1e-9), (i, row, p[i], rp)
    return diff, p


def test_wilcox_exact_and_normal(gpu_ctx):
    rng = np.random.default_rng(3)
    _wilcox_case(gpu_ctx, rng.normal(size=(300, 6)), 3, 3)                       # exact, no ties
    tied = rng.integers(0, 4, size=(300, 9)).astype(np.float64)                  # normal path with tie correction
    _wilcox_case(gpu_ctx, tied, 4, 5)
    d, p = _wilcox_case(gpu_ctx, rng.normal(size=(40, 98)) + np.linspace(0, 1, 40)[:, None] * (np.arange(98) < 49), 49, 49)
    assert (p < 1).any()
    _wilcox_case(gpu_ctx, rng.normal(size=(200, 53)), 50, 3)                     # normal path: nx = 50


def test_wilcox_missing_values(gpu_ctx):
    rng = np.random.default_rng(4)
    v = rng.uniform(size=(60, 8))
    v[0, 1] = np.nan
    v[1, 5] = np.inf
    v[2, :4] = np.nan                      # empty condition 1: NA
    v[3, 4:] = [np.inf, -np.inf, np.nan, np.inf]
    v[4, 0] = -np.inf
    v[5] = 1.0                             # all tied: sigma = 0, NA
    diff, p = _wilcox_case(gpu_ctx, v, 4, 4)
    assert math.isnan(p[2]) and math.isnan(p[3]) and math.isnan(p[5])
    assert math.isnan(diff[0]) and diff[1] == -math.inf and diff[4] == -math.inf


# ---- correction ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 4097, 1000003])
def test_adjust_bit_identical(gpu_ctx, n):
    rng = np.random.default_rng(n)
    p = rng.uniform(size=n) ** 3
    if n > 2:
        p[rng.integers(0, n, n // 10)] = np.nan
        p[rng.integers(0, n, n // 50)] = 0.0
        p[rng.integers(0, n, n // 20)] = 1.0
        p[rng.integers(0, n, n // 20)] = p[rng.integers(0, n, n // 20)]          # ties
        p[rng.integers(0, n, n // 100)] = 1e-300
    bon, bh = ds.adjust(gpu_ctx, p)
    rb, rh = adjust_ref(p)
    assert bon.tobytes() == rb.tobytes()
    assert bh.tobytes() == rh.tobytes()
    if n == 2:
        q = np.array([0.5, np.nan])
        assert ds.adjust(gpu_ctx, q)[1].tobytes() == q.tobytes()


# The correction sorts with the shared device sort: a workgroup takes a tile of SORT_TILE records, a wave a quarter of it.
# The counts of valid values sit on both sides of a tile's end, of two tiles' end and of a wave's span; with NaNs between
# them the flag scan (over all values) and the sort's scans (over its digit table) differ in length.
_T = SORT_TILE
ADJUST_EDGE_COUNTS = [_T - 1, _T, _T + 1, 2 * _T + 1, _T // 4 - 1, _T // 4, _T // 4 + 1]


def _adjust_edge_values(kind, n_valid):
    rng = np.random.default_rng(n_valid)
    if kind == "mixed":
        q = rng.uniform(size=n_valid) ** 3
        q[rng.integers(0, n_valid, n_valid // 50)] = 0.0
        q[rng.integers(0, n_valid, n_valid // 20)] = 1.0
        q[rng.integers(0, n_valid, n_valid // 20)] = q[rng.integers(0, n_valid, n_valid // 20)]      # ties
        return q
    if kind == "three":             # a wave's records share three counters of every digit
        return rng.choice(np.array([1e-3, 0.04, 0.7]), size=n_valid)
    return np.full(n_valid, 0.03)   # "equal": one counter takes a wave's whole span


@pytest.mark.parametrize("kind,n_valid,nans",
                         [("mixed", k, nans) for k in ADJUST_EDGE_COUNTS for nans in (False, True)] + [("three", 2 * _T + 1, False), ("equal", 2 * _T + 1, False)])
def test_adjust_at_sort_edges(gpu_ctx, kind, n_valid, nans):
    q = _adjust_edge_values(kind, n_valid)
    if nans:                        # a NaN after every second value
        p = np.full(n_valid + n_valid // 2, np.nan)
        p[np.arange(n_valid) + np.arange(n_valid) // 2] = q
    else:
        p = q
    assert int((~np.isnan(p)).sum()) == n_valid and (len(p) > n_valid) == nans
    bon, bh = ds.adjust(gpu_ctx, p)
    rb, rh = adjust_ref(p)
    assert bon.tobytes() == rb.tobytes()
    assert bh.tobytes() == rh.tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------------

def _parse(text):
    lines = text.rstrip("\n").split("\n")
    head = lines[0].split("\t")
    rows = [ln.split("\t") for ln in lines[1:]]
    ids = [r[0] for r in rows]
    cols = np.array([[math.nan if f == "NA" else float(f) for f in r[1:]] for r in rows]).reshape(len(rows), len(head) - 1)
    return head, ids, cols


def _matrix(path, ids, values):
    with open(path, "w") as f:
        f.write("ID\t" + "\t".join("s%d" % j for j in range(values.shape[1])) + "\n")
        for i, r in zip(ids, values):
            f.write(i + "\t" + "\t".join(repr(float(v)) for v in r) + "\n")


def test_end_to_end_tables_and_matrices(gpu_ctx, tmp_path):
    d = str(tmp_path)
    counts, solves = [], []
    for k in range(4):
        stem = "s%d" % k
        L.synth_write(L.SynthSpec(seed=23, n_events=300, n_reads=20000, first_read=k * 20000), d, stem)
        argv = ["0", stem, "./", "LH_GENE_TXT", os.path.join(d, stem + ".interval"), "UCSC_GENE2ISOFORM",
                os.path.join(d, stem + ".map"), "0", "1000000", "MRF_SINGLE", "SHORT_READ", "100", os.path.join(d, stem + ".mrf")]
        rc, text = L.cli_run("count", argv)
        assert rc == 0
        counts.append(os.path.join(d, "c%d.out" % k))
        open(counts[-1], "w").write(text)
        rc, text = L.cli_run("solve", argv + ["2000000"])
        assert rc == 0
        solves.append(os.path.join(d, "v%d.out" % k))
        open(solves[-1], "w").write(text)

    # Fisher
    rc, text = L.cli_run("test_as", ["fisher", "--tables", "-", counts[0], counts[1]])
    assert rc == 0
    head, ids, cols = _parse(text)
    assert head == ["ID", "rawP", "bonP", "bhP"]
    inp = ds.read_tables("fisher", counts[:2])
    assert ids == inp.ids and len(ids) > 50
    ref = np.array([fisher_exact(*map(int, np.rint(c))) for c in inp.values])
    for a, b in zip(cols[:, 0], ref):
        assert close(a, b, 1e-12)
    rb, rh = adjust_ref(ref)
    assert np.allclose(cols[:, 1], rb, rtol=1e-12) and np.allclose(cols[:, 2], rh, rtol=1e-12)
    out = os.path.join(d, "fisher.txt")
    assert L.cli_run("test_as", ["fisher", "--tables", out, counts[0], counts[1]]) == (0, "")
    assert open(out).read() == text

    # LRT: tables mode and matrix mode byte-identical, values against the checker
    rc, text = L.cli_run("test_as", ["lrt", "--tables", "2", "2", "-"] + counts)
    assert rc == 0
    inp = ds.read_tables("lrt", counts, 2, 2)
    _matrix(os.path.join(d, "one.txt"), inp.ids, inp.values)
    _matrix(os.path.join(d, "all.txt"), inp.ids, inp.totals)
    rc2, text2 = L.cli_run("test_as", ["lrt", os.path.join(d, "one.txt"), os.path.join(d, "all.txt"), "2", "2", "-"])
    assert rc2 == 0 and text2 == text
    head, ids, cols = _parse(text)
    assert head == ["ID", "LRT_statistics", "rawP", "bonP", "bhP"] and ids == inp.ids
    rs, rp = lrt_check(inp.values, inp.totals, 2, 2)
    assert (np.abs(cols[:, 0] - rs) <= 1e-6 * np.maximum(1, rs)).all()
    for a, b in zip(cols[:, 1], rp):
        assert close(a, b, 1e-6)

    # Wilcoxon
    rc, text = L.cli_run("test_as", ["wilcox", "--tables", "2", "2", "-"] + solves)
    assert rc == 0
    inp = ds.read_tables("wilcox", solves, 2, 2)
    _matrix(os.path.join(d, "rel.txt"), inp.ids, inp.values)
    rc2, text2 = L.cli_run("test_as", ["wilcox", os.path.join(d, "rel.txt"), "2", "2", "-"])
    assert rc2 == 0 and text2 == text
    head, ids, cols = _parse(text)
    assert head == ["ID", "Diff", "rawP", "bonP", "bhP"] and ids == inp.ids
    for i, row in enumerate(inp.values):
        rd, rp_ = wilcox_check(list(row), 2)
        assert close(cols[i, 0], rd, 1e-14, floor=1e-15) and close(cols[i, 1], rp_, 1e-9)


# ---- one large case: grid-stride loops, the multi-workgroup sort ----------------------------------------------------------

def test_large_lrt_and_fisher(gpu_ctx):
    rng = np.random.default_rng(99)
    R, n1, n2 = 400000, 8, 8
    total = np.exp(rng.uniform(np.log(5), np.log(1e5), size=(R, n1 + n2))).round()
    count = rng.binomial(total.astype(np.int64), rng.uniform(0.1, 0.9, size=(R, 1))).astype(np.float64)
    stat, p = ds.lrt(gpu_ctx, count, total, n1, n2)
    assert ((p >= 0) & (p <= 1)).all()
    idx = rng.choice(R, 2000, replace=False)
    rs, rp = lrt_check(count[idx], total[idx], n1, n2)
    # The checker's statistic is the difference of two float64 sums of about 10^7, good to some 1e-9; a p-value near 1 moves
    # as dstat / sqrt(2 pi stat), so below 1e-4 that is too coarse for 1e-6 (one row here has 5.2e-10, which the checker
    # returns as 0 and p = 1, where p = 0.99998177).  Those rows take the 50-digit reference.
    for i in np.flatnonzero(rs < 1e-4):
        rs[i] = lrt_ref(count[idx[i]][None], total[idx[i]][None], n1, n2)[0]
        rp[i] = math.erfc(math.sqrt(rs[i] / 2))
    assert (np.abs(stat[idx] - rs) <= 1e-6 * np.maximum(1, rs)).all()
    for a, b in zip(p[idx], rp):
        assert close(a, b, 1e-6)
    bon, bh = ds.adjust(gpu_ctx, p)
    rb, rh = adjust_ref(p)
    assert bon.tobytes() == rb.tobytes() and bh.tobytes() == rh.tobytes()

    T = 200000
    depth = np.minimum(1e7, 10.0 / rng.uniform(1e-6, 1, size=T) ** 1.2).round()
    share = rng.uniform(0.05, 0.95, size=(T, 4))
    cells = np.rint(depth[:, None] * share / share.sum(1, keepdims=True))
    p = ds.fisher(gpu_ctx, cells)
    assert (((p >= 0) & (p <= 1)) | np.isnan(p)).all() and not np.isnan(p).any()
    for i in rng.choice(T, 2000, replace=False):
        assert close(p[i], fisher_logratio(*cells[i]), 1e-9), (cells[i], p[i])
