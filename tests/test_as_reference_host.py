"""The 50-digit references of tests/as_ref.py checked before a kernel is held against them: fisher_ref against the exact
rule in integers, lrt_ref against the float64 Newton checker where float64 is still good and against itself at 70
digits, and the Fisher table lists of tests/test_as_precision_gpu.py against what they claim (admissible gaps, the share
of p-values a comparison can see, the tables at the 2^40 limit)."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np
import pytest

import as_ref as R
from test_as_gpu import TIE_TABLE, fisher_exact, lrt_check


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b)) if a != b else 0.0


# ---- fisher_ref against the exact rule ------------------------------------------------------------------------------------

DEGENERATE = [(0, 0, 0, 0), (0, 0, 5, 7), (5, 7, 0, 0),          # a zero row
              (0, 4, 0, 6), (3, 0, 9, 0),                        # a zero column
              (7, 0, 0, 0), (0, 0, 0, 9), (1, 0, 0, 1),          # lo == hi (the first two), and a support of two
              (0, 9, 12, 30), (4, 30, 9, 0),                     # x at lo (lo = 0, lo = k - n > 0 in the second)
              (9, 0, 3, 30), (12, 5, 0, 40),                     # x at hi (hi = m, hi = k)
              (12, 18, 20, 30), (200, 300, 400, 600)]            # x at the mode


def fisher_exact_recurrence(A, B, C, D):
    """test_as_gpu.fisher_exact with the integers d(t) = C(m, t) C(n, k - t) from their recurrence (every division exact)
    instead of two math.comb a term: the same integers, the same rule, and TIE_TABLE in 0.1 s instead of 40."""
    m, n, k, x = A + B, C + D, A + C, A
    lo, hi = max(0, k - n), min(k, m)
    d = [math.comb(m, lo) * math.comb(n, k - lo)]
    for t in range(lo, hi):
        d.append(d[-1] * (m - t) * (k - t) // ((t + 1) * (n - k + t + 1)))
    dx = d[x - lo]
    num = sum(v for v in d if v * 10 ** 7 <= dx * (10 ** 7 + 1))
    return float(Fraction(num, sum(d)))


def test_fisher_ref_equals_the_exact_rule():
    rng = np.random.default_rng(5)
    tables = [tuple(map(int, t)) for t in rng.integers(0, 21, size=(300, 4))]
    tables += [tuple(map(int, t)) for t in rng.integers(0, 201, size=(60, 4))]
    tables += [tuple(map(int, t)) for t in rng.integers(0, 1001, size=(8, 4))]          # (the exact rule takes 0.1 s at 1000)
    tables += DEGENERATE
    for A, B, C, D in DEGENERATE[8:10]:
        assert A == max(0, A + C - C - D)
    for A, B, C, D in DEGENERATE[10:12]:
        assert A == min(A + C, A + B)
    for A, B, C, D in DEGENERATE[12:]:
        assert A == R.hyper_mode(A + B, C + D, A + C)
    bad = []
    for t in tables:
        p, gap = R.fisher_ref(*t)
        e = fisher_exact(*t)
        if _rel(p, e) > 1e-15 or fisher_exact_recurrence(*t) != e:
            bad.append((t, p, e))
    assert not bad, bad[:5]
    assert _rel(R.fisher_ref(*TIE_TABLE)[0], fisher_exact_recurrence(*TIE_TABLE)) <= 1e-15


def test_fisher_ref_bisection_equals_the_walk_over_all_terms():
    """p and the gap from the two crossings are those from every term, one by one; TIE_TABLE's gap is its known near-tie"""
    rng = np.random.default_rng(6)
    for t in [tuple(map(int, t)) for t in rng.integers(0, 301, size=(200, 4))] + DEGENERATE + [TIE_TABLE]:
        assert R.fisher_ref(*t) == R.fisher_ref_all_terms(*t), t
    gap = R.fisher_ref(*TIE_TABLE)[1]
    assert abs(gap - (1e-7 - 2.3e-8)) < 1e-9          # d(t)/d(x) - 1 = 2.3e-8 (test_as_gpu.py)


def test_fisher_ref_window_is_past_the_kernels_floor():
    """a term at exp(-746) of the mode's is still inside the walk"""
    assert R.CUT < Decimal(-746).exp()
    t = R.fisher_depth_tables(10 ** 5, (39,))[0]
    p, gap = R.fisher_ref(*t)
    assert p < 1e-300 and gap < math.inf


# ---- the Fisher lists of test_as_precision_gpu.py -------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.DEPTH_SCALES)
def test_depth_tables_are_admissible_and_mostly_above_the_floor(c):
    tables = R.fisher_depth_tables(c)
    assert len(set((A + B, C + D, A + C) for A, B, C, D in tables)) == 1
    A, B, C, D = tables[0]
    assert len({A + B, C + D, A + C, B + D}) == 4                                  # no two margins equal
    ref = [R.fisher_ref(*t) for t in tables]
    assert all(gap > R.MIN_GAP for _, gap in ref)
    assert all(p > 0 for p, _ in ref)
    assert sum(p > 1e-300 for p, _ in ref) >= 0.75 * len(tables)
    assert sum(p > 1e-3 for p, _ in ref) >= 7                                      # z up to 2.5: the p-values someone reads
    # beyond the kernel's floor the reference is below anything a double p-value test can see
    assert all(p < 1e-300 for p, _ in [R.fisher_ref(*t) for t in R.fisher_depth_tables(c, R.FLOOR_Z)])


def test_deep_and_skewed_tables_are_admissible_and_above_the_floor():
    p, gap = R.fisher_ref(*R.fisher_deep_table())
    assert gap > R.MIN_GAP and 1e-3 < p < 0.1
    assert min(R.fisher_deep_table()) > 0.99e9
    ref = [R.fisher_ref(*t) for t in R.fisher_skewed_tables()]
    assert all(gap > R.MIN_GAP and p > 1e-300 for p, gap in ref)
    assert sum(p > 1e-3 for p, _ in ref) >= 8
    A, B, C, D = R.fisher_skewed_tables()[0]
    assert 999 < (C + D) / (A + B) < 1001 and abs((A + C) - (A + B)) < 10          # m : n = 1 : 1000, k about m
    A, B, C, D = R.fisher_skewed_tables()[-1]
    assert A + C == 50 and min(A + B, C + D) > 0.99e6


def test_chunk_edge_tables_hit_their_edges():
    dist = []
    for A, B, C, D in R.fisher_chunk_x_tables():
        assert 100 <= max(A, B, C, D) <= 1000
        dist.append(A - R.hyper_mode(A + B, C + D, A + C))
    assert sorted(dist) == sorted([s * d for d in R.CHUNK_DIST for s in (1, -1)])
    up, down = set(), set()
    for A, B, C, D in R.fisher_chunk_span_tables():
        m, n, k = A + B, C + D, A + C
        lo, hi, mode = max(0, k - n), min(k, m), R.hyper_mode(m, n, k)
        assert lo <= A <= hi and max(A, B, C, D) <= 1000
        assert (hi - mode in R.CHUNK_SPAN) != (mode - lo in R.CHUNK_SPAN)
        if hi - mode in R.CHUNK_SPAN:
            up.add(hi - mode)
        else:
            down.add(mode - lo)
    assert up == set(R.CHUNK_SPAN) and down == set(R.CHUNK_SPAN)
    for t in R.fisher_chunk_x_tables() + R.fisher_chunk_span_tables():
        p, gap = R.fisher_ref(*t)
        assert gap > R.MIN_GAP and _rel(p, fisher_exact(*t)) <= 1e-15


def test_limit_tables():
    for t, want in zip(R.LIMIT_TABLES, R.LIMIT_P):
        assert max(t) == R.MAX_CELL
        p, gap = R.fisher_ref(*t)
        assert gap > R.MIN_GAP and _rel(p, want) < 5e-3, (t, p)
    for t in R.LIMIT_FLAT_TABLES:
        assert max(t) == R.MAX_CELL and min(t) >= R.MAX_CELL - 50
        A, B, C, D = t
        assert abs(A - R.hyper_mode(A + B, C + D, A + C)) <= 64
        p, gap = R.fisher_ref_flat_top(*t)
        assert p == 1.0 and gap > R.MIN_GAP
    assert {abs(A - R.hyper_mode(A + B, C + D, A + C)) for A, B, C, D in R.LIMIT_FLAT_TABLES} >= {0, 25}


def test_flat_top_reference_agrees_with_the_full_walk():
    """where both can be had: cells of 10^8 (variance 2.5e7, so d(t)/d(x) - 1 < 1e-7 for x within 2 of the mode)"""
    base = R.fisher_depth_tables(10 ** 8, (0,))[0]
    for off in (0, 2, -1):
        t = (base[0] + off, base[1] - off, base[2] - off, base[3] + off)
        assert R.fisher_ref_flat_top(*t, window=64)[0] == R.fisher_ref(*t)[0] == 1.0
    with pytest.raises(NotImplementedError):
        R.fisher_ref_flat_top(base[0] + 20, base[1] - 20, base[2] - 20, base[3] + 20, window=64)


def test_mode_rule_is_the_argmax_of_the_reference_pmf():
    """the rule that the kernel's 128-bit correction implements, at the 2^40 limit: both neighbours of the mode are
    no larger than it (the pmf is unimodal)"""
    for A, B, C, D in R.LIMIT_TABLES + R.LIMIT_FLAT_TABLES + tuple(R.fisher_depth_tables(10 ** 8, (0,))):
        m, n, k = A + B, C + D, A + C
        lo, hi, mode = max(0, k - n), min(k, m), R.hyper_mode(m, n, k)
        with localcontext() as ctx:
            ctx.prec = R.PREC
            for end in (min(hi, mode + 1), max(lo, mode - 1)):
                side = R._walk_side(m, n, k, mode, end)[0]
                assert len(side) == abs(end - mode) and all(d <= 1 for d in side), (A, B, C, D)


# ---- lrt_ref ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n1,n2", R.LRT_DESIGNS)
def test_lrt_ref_agrees_with_float64_newton_at_shallow_depth(n1, n2):
    rng = np.random.default_rng(100 * n1 + n2)
    rows, n = 24, n1 + n2
    total = np.exp(rng.uniform(np.log(5), np.log(1e4), size=(rows, n))).round()
    frac = np.concatenate([np.repeat(rng.uniform(0.05, 0.95, (rows, 1)), n1, 1), np.repeat(rng.uniform(0.05, 0.95, (rows, 1)), n2, 1)], 1)
    frac[:8] = frac[:8, :1]                                                        # null rows
    count = rng.poisson(total * frac).astype(np.float64)
    count[0], total[0] = 0, 0
    count[1] = rng.uniform(0, 50, size=n)                                          # non-integers: rounded
    ref = R.lrt_ref(count, total, n1, n2)
    chk, _ = lrt_check(count, total, n1, n2)
    err = np.abs(ref - chk) / np.maximum(1.0, ref)
    assert err.max() <= 1e-8, (err.argmax(), ref[err.argmax()], chk[err.argmax()])
    assert (ref[8:] > 20).any() and (ref[2:8] < 20).all()


def test_lrt_ref_is_invariant_to_its_precision():
    count, total, band = R.lrt_depth_rows(8, 8)
    ref = R.lrt_depth_ref(8, 8)
    i = next(i for i, b in enumerate(band) if b == "2^40" and 0.1 < ref[i] < 10)
    assert total[i].min() > 2 ** 39
    a, b = R.lrt_ref_row(count[i], total[i], 8, 8, prec=50), R.lrt_ref_row(count[i], total[i], 8, 8, prec=70)
    assert float(a) == ref[i]
    assert abs(a - b) < Decimal("1e-30"), (a, b)


def test_lrt_depth_rows_are_what_they_claim():
    for n1, n2 in R.LRT_DESIGNS:
        count, total, band = R.lrt_depth_rows(n1, n2)
        assert count.shape == total.shape == (len(band), n1 + n2) and 40 <= len(band) <= 60
        for name, T in R.LRT_BANDS:
            t = total[[b == name for b in band]]
            assert len(t) == R.LRT_NULL_PER_BAND + 2 and t.min() >= 0.5 * T - 1 and t.max() <= min(2 * T, 2.0 ** 40)
        e = band.index("edge")
        assert (count[e] == 0).all() and (total[e] == 2.0 ** 40).all()
        assert (count[e + 1] > total[e + 1]).all()
        assert total[e + 2][0] == 0 and total[e + 2][1:].min() >= 0.5e8
