"""The FP64 kernels of lsq_as.hip against the 50-digit references of tests/as_ref.py, at read depths a real library reaches
and on the null-ish tables and rows where most real events sit: Fisher's long walk at a p-value someone would read, its
64-term chunk edges, the declared limit of 2^40 a cell; the LRT statistic up to totals of 2^40, where each fit's
log-likelihood is 10^10 times the statistic; and the Wilcoxon edges.  tests/test_as_reference_host.py holds the references
and the table lists against what they claim, on the CPU.  Every test prints the error it measured before it asserts."""
import math

import numpy as np
import pytest

import as_ref as R
from lesseq_amd import diffsplice as ds
from test_as_gpu import close, fisher_exact

pytestmark = pytest.mark.gpu

FISHER_RTOL = 1e-9        # the project's (test_as_gpu.py)
LRT_RTOL = 1e-6


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b)) if a != b else 0.0


def _fisher(gpu_ctx, tables):
    return ds.fisher(gpu_ctx, np.array(tables, dtype=np.float64))


def _held_against_ref(label, tables, p):
    """Every table admissible; p within FISHER_RTOL of the reference where that is above 1e-300, and below 1e-290 where
    it is not.  Returns the largest relative error among the p-values above 1e-300."""
    worst, bad = 0.0, []
    for t, g in zip(tables, p):
        ref, gap = R.fisher_ref(*t)
        assert gap > R.MIN_GAP, (t, gap)
        if ref > 1e-300:
            worst = max(worst, _rel(g, ref))
        if not (close(g, ref, FISHER_RTOL) if ref > 1e-300 else 0 <= g < 1e-290):
            bad.append((t, g, ref))
    print("fisher %s: %d tables, largest relative error %.3g" % (label, len(tables), worst))
    assert not bad, bad[:5]
    return worst


# ---- Fisher -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.DEPTH_SCALES)
def test_fisher_nullish_at_depth(gpu_ctx, c):
    """x = mode + round(z sigma) under balanced margins of cell scale c.  The tables at z = +-36 have p = 8e-284 from c = 10^5
    on (exp(-648) of the mode's term; the kernel's floor exp(-746) is z = 38.6) and are held at FISHER_RTOL like the rest;
    the floor itself is probed at z = +-39, +-40, where the reference is below 1e-300 and p < 1e-290 is all that is asked."""
    tables = R.fisher_depth_tables(c) + R.fisher_depth_tables(c, R.FLOOR_Z)
    p = _fisher(gpu_ctx, tables)
    assert ((p >= 0) & (p <= 1)).all()
    _held_against_ref("cells %.0e" % c, tables, p)
    assert (p[-len(R.FLOOR_Z):] < 1e-290).all()


def test_fisher_deep_and_skewed(gpu_ctx):
    """one table at cells of 10^9; m : n = 1 : 1000 with k about m; k = 50 against margins of 10^6 (51 terms)"""
    tables = [R.fisher_deep_table()] + R.fisher_skewed_tables()
    p = _fisher(gpu_ctx, tables)
    _held_against_ref("cells 1e+09", tables[:1], p[:1])
    _held_against_ref("skewed margins at 1e+06", tables[1:], p[1:])


def test_fisher_chunk_edges(gpu_ctx):
    """|x - mode|, hi - mode and mode - lo at 1, 63, 64, 65, 127, 128, 129: where __shfl(L, dist - j0 - 1), the carry from
    lane 63 and the `valid` mask change.  Cells of a few hundred: the exact rule in integers at 1e-12."""
    tables = R.fisher_chunk_x_tables() + R.fisher_chunk_span_tables()
    p = _fisher(gpu_ctx, tables)
    err = [_rel(g, fisher_exact(*t)) for t, g in zip(tables, p)]
    print("fisher chunk edges: %d tables, largest relative error %.3g" % (len(tables), max(err)))
    bad = [(t, g, e) for t, g, e in zip(tables, p, err) if not e <= 1e-12]
    assert not bad, bad[:5]


def test_fisher_at_the_cell_limit(gpu_ctx):
    """Cells of 2^40 (AS_MAX_CELL; the mode's 128-bit correction).  The three flat-top tables (every cell about 2^40, x
    within 64 of the mode, a walk of 2e7 terms a side) have p = 1 by R's rule: as_ref.fisher_ref_flat_top."""
    L = R.MAX_CELL
    tables = list(R.LIMIT_TABLES) + list(R.LIMIT_FLAT_TABLES)
    cells = np.array(tables + [(L + 1, 5, 7, 9), (5, 7, 9, L + 1), (L + 0.4, L, 3, 5)], dtype=np.float64)
    assert cells[-1, 0] > L and cells[-3, 0] == L + 1
    p = ds.fisher(gpu_ctx, cells)
    k = len(R.LIMIT_TABLES)
    _held_against_ref("cells 2^40, small support", tables[:k], p[:k])
    for t, g in zip(tables[k:], p[k:]):
        ref, gap = R.fisher_ref_flat_top(*t)
        assert gap > R.MIN_GAP
        print("fisher cells 2^40, flat top %s: p - 1 = %.3g" % (t, g - ref))
        assert close(g, ref, FISHER_RTOL), (t, g)
    assert math.isnan(p[-3]) and math.isnan(p[-2])          # a cell of 2^40 + 1
    assert p[-1] == p[1]                                    # 2^40 + 0.4 rounds to 2^40


# ---- LRT ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n1,n2", R.LRT_DESIGNS)
def test_lrt_at_depth(gpu_ctx, n1, n2):
    """The statistic within LRT_RTOL max(1, stat) of the 50-digit Newton fit up to totals of 2^40; the p-value against
    erfc(sqrt(stat / 2)) of the kernel's own statistic, which decouples the tail function from the fit."""
    count, total, band = R.lrt_depth_rows(n1, n2)
    ref = R.lrt_depth_ref(n1, n2)
    stat, p = ds.lrt(gpu_ctx, count, total, n1, n2)
    err = np.abs(stat - ref) / np.maximum(1.0, ref)
    for name in dict.fromkeys(band):
        sel = np.array([b == name for b in band])
        null = sel & (ref < 100)
        print("lrt %d+%d totals %s: largest |dstat|/max(1, stat) %.3g (null-ish rows: largest |dstat| %.3g)"
              % (n1, n2, name, err[sel].max(), np.abs(stat - ref)[null].max() if null.any() else math.nan))
    assert not np.isnan(stat).any() and ((p >= 0) & (p <= 1)).all()
    bad = [(band[i], stat[i], ref[i]) for i in np.flatnonzero(~(err <= LRT_RTOL))]
    assert not bad, bad[:5]
    tail = [_rel(a, math.erfc(math.sqrt(s / 2))) for a, s in zip(p, stat) if not (a < 1e-300 and math.erfc(math.sqrt(s / 2)) < 1e-300)]
    print("lrt %d+%d: largest relative error of p against erfc of the kernel's statistic %.3g" % (n1, n2, max(tail)))
    for a, s in zip(p, stat):
        assert close(a, math.erfc(math.sqrt(s / 2)), 1e-12), (a, s)


# ---- Wilcoxon edges -------------------------------------------------------------------------------------------------------

def _wilcox_rows(gpu_ctx, value, n1, n2):
    value = np.array(value, dtype=np.float64)
    diff, p = ds.wilcox(gpu_ctx, value, n1, n2)
    for i, row in enumerate(value):
        rd, rp = R.wilcox_check(list(row), n1)
        assert (math.isnan(rd) and math.isnan(diff[i])) or rd == diff[i], (i, diff[i], rd)
        assert close(p[i], rp, 1e-9), (i, p[i], rp)
    return p


def test_wilcox_exact_centre(gpu_ctx):
    """W = nx ny / 2 with nx ny even: both tails hold more than half, p = 1.  (2, 2), (4, 3) and (6, 6) in one call, the
    smaller groups through NaN."""
    nan = math.nan
    rows = [[1, 4, nan, nan, nan, nan, 2, 3, nan, nan, nan, nan],
            [1, 2, 6, 7, nan, nan, 3, 4, 5, nan, nan, nan],
            [1, 2, 3, 10, 11, 12, 4, 5, 6, 7, 8, 9]]
    p = _wilcox_rows(gpu_ctx, rows, 6, 6)
    assert (p == 1.0).all()


def test_wilcox_many_group_sizes_in_one_call(gpu_ctx):
    """NaN and +-inf entries drop out, so the rows of one call need the exact tables of seven different (nx, ny)"""
    rng = np.random.default_rng(8)
    sizes = [(49, 49), (1, 1), (1, 49), (49, 1), (3, 7), (48, 2), (10, 49)]
    value = rng.normal(size=(len(sizes), 98))
    for row, (nx, ny) in zip(value, sizes):
        row[nx:49] = [(math.nan, math.inf, -math.inf)[j % 3] for j in range(49 - nx)]
        row[49 + ny:] = [(math.inf, math.nan, -math.inf)[j % 3] for j in range(49 - ny)]
    p = _wilcox_rows(gpu_ctx, value, 49, 49)
    assert not np.isnan(p).any() and p[1] == 1.0 and len(set(p)) > 4


def test_wilcox_at_the_exact_limit_and_with_ties(gpu_ctx):
    rng = np.random.default_rng(9)
    value = rng.normal(size=(2, 99)) + 0.4 * (np.arange(99) < 49)
    value[1, 60] = value[1, 3]                                   # 49 x 50: ny = 50 takes the normal path, with and without a tie
    _wilcox_rows(gpu_ctx, value, 49, 50)
    heavy = rng.integers(0, 6, size=(1, 2000)).astype(np.float64) + (np.arange(2000) < 1000) * (rng.uniform(size=2000) < 0.1)
    p = _wilcox_rows(gpu_ctx, heavy, 1000, 1000)                 # 1000 + 1000 values on seven levels
    assert 0 < p[0] < 1
    zero = [[-0.0, 1.0, 2.0, 0.0, 3.0, 4.0], [0.0, 1.0, 2.0, -0.0, 0.5, 4.0]]
    _wilcox_rows(gpu_ctx, zero, 3, 3)                            # -0.0 == 0.0 is a tie: the normal path
