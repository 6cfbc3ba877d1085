"""`test_as betabin` on the device (lsq_as_betabin, lsq_debug_as_bb_loglik) against the 50-digit reference of
tests/betabin_ref.py: the log-likelihood alone, the fit on the certified rows of tests/golden/betabin/rows.json, the NA rules and
launch shapes, and the executable.  tests/test_betabin_reference_host.py certifies those rows' maxima, on the CPU."""
import math
import os

import mpmath as mp
import numpy as np
import pytest

import lesseq_amd as L
from lesseq_amd import diffsplice as ds

import betabin_ref as R

pytestmark = pytest.mark.gpu

LOGLIK_ATOL = 2.5e-7        # what a log-likelihood may be off by for stat = 2 (l_f - l_r) to meet LRT_RTOL at stat <= 1
LRT_RTOL = 1e-6             # the project's bound on a likelihood-ratio statistic: |d stat| <= LRT_RTOL max(1, stat)


# ---- (1) the building block -------------------------------------------------------------------------------------------------------------

RHOS = [0.0, 1e-12, 1e-8, 1e-4, 0.1, 0.5, 0.999]
MUS = [0.0, 1e-9, 0.3, 1 - 1e-9, 1.0]
# bb_logsum takes min(k, 8 - floor(x)) terms directly and the rest by Stirling's series: k = 8 | 9 is where the series first gets
# a term at x < 1, k = 7 | 8 at 1 <= x < 2; x = c/rho crosses 8 between the rho of RHOS
SIZES = [1, 2, 7, 8, 9, 10, 10 ** 3, 10 ** 6]


def _loglik_cases():
    cases = []
    for n in SIZES:
        for y in sorted({0, 1, n - 1, n}):
            for rho in RHOS:
                for mu in MUS:
                    cases.append((y, n, mu, rho))
    return cases


def test_loglik_against_loggamma(gpu_ctx):
    cases = _loglik_cases()
    y, n, mu, rho = (np.array(v, dtype=np.float64) for v in zip(*cases))
    got = ds.bb_loglik(gpu_ctx, y[:, None], n[:, None], mu, rho)
    worst = {r: 0.0 for r in RHOS}
    minus_inf = 0
    for (yj, nj, m, r), g in zip(cases, got):
        ref = R.loglik_gamma([yj], [nj], m, r)
        if ref == mp.ninf:                       # mu = 0 with y > 0, mu = 1 with y < n
            assert g == -math.inf, (yj, nj, m, r, g)
            minus_inf += 1
            continue
        assert math.isfinite(g), (yj, nj, m, r, g)
        worst[r] = max(worst[r], abs(float(mp.mpf(float(g)) - ref)))
    for r in RHOS:
        print("bb_loglik, rho = %-6g largest |error| %.2e" % (r, worst[r]))
    assert minus_inf == sum(1 for yj, nj, m, r in cases if (m == 0.0 and yj > 0) or (m == 1.0 and yj < nj))
    assert max(worst.values()) <= LOGLIK_ATOL, worst


def test_loglik_sums_over_the_samples_of_a_row(gpu_ctx):
    rng = np.random.default_rng(5)
    n = rng.integers(0, 62500, size=(40, 16))               # sum n <= 10^6 a row; some samples shallow, one empty
    n[:, 3] = 0
    n[:, 5] = rng.integers(1, 12, size=40)
    y = rng.binomial(n, rng.uniform(0.05, 0.95, size=(40, 1)))
    mu = rng.uniform(0.01, 0.99, size=40)
    rho = np.array(RHOS + [3e-7, 0.02, 0.9])[np.arange(40) % 10]
    got = ds.bb_loglik(gpu_ctx, y, n, mu, rho)
    err = [abs(float(mp.mpf(float(g)) - R.loglik_gamma([int(v) for v in yr], [int(v) for v in nr], m, r))) for g, yr, nr, m, r in zip(got, y, n, mu, rho)]
    print("bb_loglik over 16 samples, sum n <= 1e6: largest |error| %.2e" % max(err))
    assert max(err) <= LOGLIK_ATOL
    assert ds.bb_loglik(gpu_ctx, np.empty((0, 3)), np.empty((0, 3)), [], []).shape == (0,)


# ---- (2) the fit ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fitted(gpu_ctx):
    """the device's answer for every golden row, one call per design"""
    out = {}
    for design in R.DESIGNS:
        rows = [r for r in R.golden_rows() if r["design"] == design]
        res = ds.betabin(gpu_ctx, np.array([r["count"] for r in rows]), np.array([r["total"] for r in rows]), *design)
        out[design] = (rows, np.array(res))
    return out


@pytest.mark.parametrize("design", R.DESIGNS, ids=lambda d: "%d+%d" % d)
def test_fit_against_the_certified_maxima(fitted, design):
    rows, (mu1, mu2, rho, stat, p) = fitted[design]
    assert len(rows) == len(R.BANDS) * len(R.KINDS)
    worst_stat, worst_l = {b: 0.0 for b in R.BANDS}, {b: 0.0 for b in R.BANDS}
    bad = []
    for i, r in enumerate(rows):
        ref = r["ref"]
        scale = max(1.0, ref["stat"])
        assert 0 <= mu1[i] <= 1 and 0 <= mu2[i] <= 1 and 0 <= rho[i] <= R.RHO_MAX_F and stat[i] >= 0, (r["band"], r["kind"])
        d_stat = abs(stat[i] - ref["stat"]) / scale
        # the reference's l_full at the device's point against the reference's maximum: the estimates, without a fight over
        # directions in which l is flat
        d_l = float(ref["lf"] - R.loglik_full(ref["y"], ref["n"], design[0], float(mu1[i]), float(mu2[i]), float(rho[i]))) / scale
        d_p = abs(p[i] - math.erfc(math.sqrt(stat[i] / 2)))
        worst_stat[r["band"]] = max(worst_stat[r["band"]], d_stat)
        worst_l[r["band"]] = max(worst_l[r["band"]], abs(d_l))
        if not (d_stat <= LRT_RTOL and abs(d_l) <= LOGLIK_ATOL and d_p <= 1e-12 * p[i]):
            bad.append((r["band"], r["kind"], stat[i], ref["stat"], d_stat, d_l, d_p, (mu1[i], mu2[i], rho[i]), (ref["mu1"], ref["mu2"], ref["rho"])))
    for b in R.BANDS:
        print("betabin %d+%d, totals %-6d |d stat|/max(1, stat) %.2e   (l_max - l(device's point))/max(1, stat) %.2e" % (design + (b, worst_stat[b], worst_l[b])))
    assert not bad, bad[:5]


PINNED_DEPTH = 10 ** 7       # the deepest band of R.DEEP_BANDS at which the statistic met LRT_RTOL when it was measured


def test_fit_at_depth(gpu_ctx):
    """Per-sample totals of 1e6, 1e7 and 2^40: measured, printed, and held up to PINNED_DEPTH.  l itself grows with the depth (1e13
    at 2^40), and stat is a difference of two of them in doubles: measured on an MI355X 3.3e-8, 3.0e-7 and 9.4e-2."""
    worst = {b: [0.0, 0.0] for b in R.DEEP_BANDS}
    bad = []
    for design in R.DESIGNS:
        rows = [r for r in R.golden_rows(True) if r["design"] == design]
        mu1, mu2, rho, stat, p = ds.betabin(gpu_ctx, np.array([r["count"] for r in rows]), np.array([r["total"] for r in rows]), *design)
        for i, r in enumerate(rows):
            ref = r["ref"]
            scale = max(1.0, ref["stat"])
            d_stat = abs(stat[i] - ref["stat"]) / scale
            d_l = abs(float(ref["lf"] - R.loglik_full(ref["y"], ref["n"], design[0], float(mu1[i]), float(mu2[i]), float(rho[i])))) / scale
            w = worst[r["band"]]
            w[0], w[1] = max(w[0], d_stat), max(w[1], d_l)
            if r["band"] <= PINNED_DEPTH and not (d_stat <= LRT_RTOL and d_l <= LOGLIK_ATOL and abs(p[i] - math.erfc(math.sqrt(stat[i] / 2))) <= 1e-12 * p[i]):
                bad.append((design, r["band"], r["kind"], stat[i], ref["stat"], d_stat, d_l))
    for b in R.DEEP_BANDS:
        print("betabin, totals %-14d |d stat|/max(1, stat) %.2e   (l_max - l(device's point))/max(1, stat) %.2e%s"
              % (b, worst[b][0], worst[b][1], "" if b <= PINNED_DEPTH else "   (not held)"))
    assert not bad, bad[:5]


def test_boundary_maxima_come_back_as_boundaries(fitted):
    """rho = 0 for replicates that agree better than binomial draws, mu = 0 for a condition of zeros, rho = 0.999 for all-or-nothing
    samples: where the reference's maximum lies on the boundary the device returns the boundary itself"""
    for design, (rows, (mu1, mu2, rho, stat, p)) in fitted.items():
        for i, r in enumerate(rows):
            if r["kind"] == "under":
                assert rho[i] == 0.0, (design, r["band"], rho[i])
            if r["kind"] == "all_or_nothing":
                assert rho[i] == R.RHO_MAX_F, (design, r["band"], rho[i])
            if r["kind"] == "zeros":
                assert (mu1[i] if r["ref"]["mu1"] == 0.0 else mu2[i]) == 0.0, (design, r["band"], mu1[i], mu2[i])


# ---- (3) NA rules and shapes ----------------------------------------------------------------------------------------------------------------

def _base_rows(design=(2, 2)):
    rows = [r for r in R.golden_rows() if r["design"] == design]
    return np.array([r["count"] for r in rows]), np.array([r["total"] for r in rows])


def test_na_rules_leave_the_good_rows_alone(gpu_ctx):
    count, total = _base_rows()
    clean = np.array(ds.betabin(gpu_ctx, count, total, 2, 2))
    assert not np.isnan(clean).any()
    c, t = count.copy(), total.copy()
    rules = {}

    def spoil(i, name, cj=None, tj=None, j=0):
        if cj is not None:
            c[i, j] = cj
        if tj is not None:
            t[i, j] = tj
        rules[i] = name
    spoil(1, "NA count", cj=math.nan)
    spoil(4, "NA total", tj=math.nan, j=3)
    spoil(7, "negative count", cj=-1.0, j=2)
    spoil(10, "negative total", tj=-3.0, j=1)
    spoil(13, "infinite total", tj=math.inf)
    spoil(16, "infinite count", cj=math.inf, tj=math.inf, j=3)
    spoil(19, "total above 2^40", tj=2.0 ** 40 + 2)
    spoil(22, "y > n", cj=t[22, 1] + 1, j=1)
    c[25, :2], t[25, :2] = 0, 0
    rules[25] = "condition 1 without an informative sample"
    c[28, 2:], t[28, 2:] = 0, 0
    rules[28] = "condition 2 without an informative sample"
    c[31, [0, 2]], t[31, [0, 2]] = 0, 0
    rules[31] = "two informative samples"
    got = np.array(ds.betabin(gpu_ctx, c, t, 2, 2))
    for i in range(len(c)):
        if i in rules:
            assert np.isnan(got[:, i]).all(), (rules[i], got[:, i])
        else:
            assert got[:, i].tobytes() == clean[:, i].tobytes(), i
    # the edges of the rules: 2^40 itself is a cell, a value that rounds to -0 is 0, y = n is not y > n
    c2, t2 = count[:3].copy(), total[:3].copy()
    t2[0, 0] = 2.0 ** 40
    c2[1, 0] = -0.3
    c2[2, 1] = t2[2, 1]
    assert not np.isnan(np.array(ds.betabin(gpu_ctx, c2, t2, 2, 2))).any()


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
def test_result_is_a_function_of_the_row(gpu_ctx, n_rows):
    count, total = _base_rows((3, 3))
    base = np.array(ds.betabin(gpu_ctx, count, total, 3, 3))
    pick = np.random.default_rng(n_rows).permutation(np.arange(n_rows) % len(count))
    got = np.array(ds.betabin(gpu_ctx, count[pick], total[pick], 3, 3))
    assert got.shape == (5, n_rows)
    assert got.tobytes() == np.ascontiguousarray(base[:, pick]).tobytes()


def test_no_rows_and_argument_errors(gpu_ctx):
    out = ds.betabin(gpu_ctx, np.empty((0, 4)), np.empty((0, 4)), 2, 2)
    assert len(out) == 5 and all(o.shape == (0,) for o in out)
    with pytest.raises(L.LsqError, match="at least 3 samples"):
        ds.betabin(gpu_ctx, np.ones((2, 2)), np.ones((2, 2)), 1, 1)
    with pytest.raises(L.LsqError):
        ds.betabin(gpu_ctx, np.ones((2, 4097)), np.ones((2, 4097)), 4097, 0)


def test_degenerate_rows(gpu_ctx):
    # every y = 0, or every y = n: l = 0 at both maxima whatever rho is
    count = np.array([[0, 0, 0, 0], [5, 9, 3, 7]], dtype=np.float64)
    total = np.array([[5, 9, 3, 7], [5, 9, 3, 7]], dtype=np.float64)
    mu1, mu2, rho, stat, p = ds.betabin(gpu_ctx, count, total, 2, 2)
    assert mu1.tolist() == [0, 1] and mu2.tolist() == [0, 1] and stat.tolist() == [0, 0] and p.tolist() == [1, 1]
    assert ((rho >= 0) & (rho <= R.RHO_MAX_F)).all()


# ---- (4) the command line ---------------------------------------------------------------------------------------------------------------------

def _expected_text(gpu_ctx, ids, count, total, n1, n2):
    mu1, mu2, rho, stat, p = ds.betabin(gpu_ctx, count, total, n1, n2)
    bon, bh = ds.adjust(gpu_ctx, p)
    lines = ["ID\tpsi1\tpsi2\trho\tLRT_statistics\trawP\tbonP\tbhP"]
    for i, name in enumerate(ids):
        lines.append("\t".join([name] + [ds.format_number(v[i]) for v in (mu1, mu2, rho, stat, p, bon, bh)]))
    return "\n".join(lines) + "\n"


def test_command_line_matrix_and_tables(gpu_ctx, tmp_path):
    count, total = _base_rows((2, 1))
    count, total = count[:23].copy(), total[:23].copy()
    count[5, 0] = total[5, 0] + 2                      # an NA row: printed as NA, left out of the corrections
    ids = ["form%d" % i for i in range(len(count))]
    expected = _expected_text(gpu_ctx, ids, count, total, 2, 1)
    assert "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n" in expected

    def matrix(path, values):
        with open(path, "w") as f:
            f.write("ID\ta1\ta2\tb1\n")
            for name, row in zip(ids, values):
                f.write(name + "\t" + "\t".join("%d" % v for v in row) + "\n")
        return str(path)
    one, all_ = matrix(tmp_path / "one.txt", count), matrix(tmp_path / "all.txt", total)
    rc, text = L.cli_run("test_as", ["betabin", one, all_, "2", "1", "-"])
    assert rc == 0 and text == expected
    out = str(tmp_path / "out.txt")
    assert L.cli_run("test_as", ["betabin", one, all_, "2", "1", out]) == (0, "")
    assert open(out).read() == expected

    tables = []
    for s in range(3):                                 # a count table: gene, the event total, the form's ID, its count
        tables.append(str(tmp_path / ("s%d.tab" % s)))
        with open(tables[-1], "w") as f:
            for i, name in enumerate(ids):
                f.write("gene%d\t%d\t%s\t%d\n" % (i // 2, total[i, s], name, count[i, s]))
    rc, text = L.cli_run("test_as", ["betabin", "--tables", "2", "1", "-"] + tables)
    assert rc == 0 and text == expected

    # two samples: status 1 and no table.  (That the message is the usage text is held where standard error can be read:
    # tests/test_betabin_reference_host.py; a GPU test's goes to a log, conftest.py.)
    for argv in (["betabin", one, all_, "1", "1", "-"], ["betabin", "--tables", "1", "1", "-"] + tables[:2]):
        assert L.cli_run("test_as", argv) == (1, "")
