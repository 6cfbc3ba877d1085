"""Differential splicing tests of the pipeline's step 4 (bin/Test_AS.r): Fisher's exact test, the Poisson log-linear model
with its likelihood-ratio test, the Wilcoxon rank-sum test and the Bonferroni / BH corrections, on the device
(include/lesseq_hip.h, lsq_as_*).  NumPy arrays in and out; NaN stands for R's NA.  The readers of the script's
matrices and of count / solve tables, and R's number formatting, are host-only."""
import ctypes as C

import numpy as np

from ._lib import lib, check, vp, cs, P

_dp = P(C.c_double)


def _f64(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.reshape(-1, cols) if cols else a.reshape(-1)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def fisher(ctx, cells):
    """Two-sided Fisher exact test per 2x2 table; cells [n, 4] = A B C D (Test_AS.r:34-47).  Returns p [n]."""
    c = _f64(cells, 4)
    p = np.empty(len(c))
    check(lib.lsq_as_fisher(ctx.h, len(c), _ptr(c), _ptr(p)))
    return p


def lrt(ctx, count, total, n1, n2):
    """Poisson log-linear model + likelihood-ratio test per row; count, total [n, n1+n2] (Test_AS.r:89-131).
    Returns (stat, p)."""
    a, b = _f64(count, n1 + n2), _f64(total, n1 + n2)
    if a.shape != b.shape:
        raise ValueError("count and total differ in shape: %s, %s" % (a.shape, b.shape))
    stat, p = np.empty(len(a)), np.empty(len(a))
    check(lib.lsq_as_lrt(ctx.h, len(a), n1, n2, _ptr(a), _ptr(b), _ptr(stat), _ptr(p)))
    return stat, p


def betabin(ctx, count, total, n1, n2):
    """Beta-binomial model with one dispersion per row + likelihood-ratio test; count, total [n, n1+n2], n1+n2 >= 3
    (DESIGN 4.6).  Returns (mu1, mu2, rho, stat, p): the full model's fit, the statistic and its chi-square p."""
    a, b = _f64(count, n1 + n2), _f64(total, n1 + n2)
    if a.shape != b.shape:
        raise ValueError("count and total differ in shape: %s, %s" % (a.shape, b.shape))
    out = [np.empty(len(a)) for _ in range(5)]
    check(lib.lsq_as_betabin(ctx.h, len(a), n1, n2, _ptr(a), _ptr(b), *[_ptr(o) for o in out]))
    return tuple(out)


def bb_loglik(ctx, y, n, mu, rho):
    """The beta-binomial log-likelihood alone (a developer entry: lsq_debug_as_bb_loglik): y, n [rows, samples]; mu, rho [rows].
    Returns per row the sum over its samples."""
    y, n = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(n, dtype=np.float64)
    if y.ndim != 2 or y.shape != n.shape:
        raise ValueError("y and n must be [rows, samples] of one shape: %s, %s" % (y.shape, n.shape))
    mu, rho = _f64(mu), _f64(rho)
    if len(mu) != len(y) or len(rho) != len(y):
        raise ValueError("one mu and one rho per row")
    out = np.empty(len(y))
    check(lib.lsq_debug_as_bb_loglik(ctx.h, len(y), y.shape[1], _ptr(y), _ptr(n), _ptr(mu), _ptr(rho), _ptr(out)))
    return out


def wilcox(ctx, value, n1, n2):
    """Mean difference and Wilcoxon rank-sum test per row; value [n, n1+n2] (Test_AS.r:162-175).  Returns (diff, p)."""
    v = _f64(value, n1 + n2)
    diff, p = np.empty(len(v)), np.empty(len(v))
    check(lib.lsq_as_wilcox(ctx.h, len(v), n1, n2, _ptr(v), _ptr(diff), _ptr(p)))
    return diff, p


def adjust(ctx, p):
    """p.adjust(p, "bonferroni") and p.adjust(p, "BH").  Returns (bonferroni, bh)."""
    q = _f64(p)
    bon, bh = np.empty(len(q)), np.empty(len(q))
    check(lib.lsq_as_adjust(ctx.h, len(q), _ptr(q), _ptr(bon), _ptr(bh)))
    return bon, bh


def format_number(v):
    """R's as.character of a double (15 significant digits; NaN as NA)."""
    buf = C.create_string_buffer(64)
    check(lib.lsq_as_format_number(float(v), buf, len(buf)))
    return buf.value.decode()


class Input:
    """The checked input of one test: ids [n], values [n, columns] (cells for Fisher), totals (LRT) or None,
    left_out (tables mode, Fisher: events without exactly two forms)."""

    def __init__(self, h):
        try:
            n, cols = lib.lsq_as_input_rows(h), lib.lsq_as_input_columns(h)
            self.ids = [lib.lsq_as_input_id(h, i).decode() for i in range(n)]

            def arr(ptr):
                return np.ctypeslib.as_array(ptr, shape=(n, cols)).copy() if ptr and n else (np.empty((0, cols)) if n == 0 else None)
            self.values = arr(lib.lsq_as_input_values(h))
            self.totals = arr(lib.lsq_as_input_totals(h))
            self.left_out = lib.lsq_as_input_left_out(h)
        finally:
            lib.lsq_as_input_free(h)


def _read(fn, test, paths, n1, n2):
    enc = [p.encode() if isinstance(p, str) else p for p in paths]
    arr = (cs * max(1, len(enc)))(*enc)
    h = vp()
    check(fn(test.encode(), len(enc), arr, n1, n2, C.byref(h)))
    return Input(h)


def read_matrix(test, paths, n1=1, n2=1):
    """The script's own input files (a header, then ID + values per line): fisher [count_matrix], lrt and betabin
    [count_one, count_all], wilcox [value_matrix]."""
    return _read(lib.lsq_as_read_matrix, test, paths, n1, n2)


def read_tables(test, paths, n1=1, n2=1):
    """This project's count tables (fisher: two, lrt and betabin: n1+n2) or solve tables (wilcox: n1+n2), one per sample."""
    return _read(lib.lsq_as_read_tables, test, paths, n1, n2)
