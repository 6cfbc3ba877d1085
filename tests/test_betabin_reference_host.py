"""The reference of `test_as betabin` held against what it claims (tests/betabin_ref.py), without a device: the two forms of the
log-likelihood, its limits and shape, the certificates of every row the GPU tests use (tests/golden/betabin/rows.json), and the
host-side readers' answer to "betabin"."""
import math
import os

import mpmath as mp
import numpy as np
import pytest

import lesseq_amd as L
from lesseq_amd import diffsplice as ds

import betabin_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SMALL = [([3, 0, 5, 2], [7, 4, 5, 9]), ([0, 0], [3, 6]), ([4, 11], [4, 11]), ([1], [1]), ([0], [1]), ([13, 2, 40], [40, 2, 41])]
POINTS = [(0.3, 0.1), (0.5, 0.999), (0.2, 1e-8), (1e-9, 0.5), (1 - 1e-9, 1e-4), (0.7, 1e-12)]


def test_three_sums_equal_the_loggamma_form():
    with mp.workdps(R.DPS):
        for y, n in SMALL:
            for mu, rho in POINTS:
                a, b = R.loglik(y, n, mu, rho), R.loglik_gamma(y, n, mu, rho)
                assert abs(a - b) <= mp.mpf(10) ** -40, (y, n, mu, rho, a, b)
    # the boundary values of mu: finite where the data allow them, -inf where they do not, in both forms
    for rho in (0, 1e-8, 0.3):
        assert abs(R.loglik([0, 0], [3, 6], 0, rho)) <= mp.mpf(10) ** -40 and R.loglik_gamma([0, 0], [3, 6], 0, rho) == 0
        assert abs(R.loglik([4, 11], [4, 11], 1, rho)) <= mp.mpf(10) ** -40 and R.loglik_gamma([4, 11], [4, 11], 1, rho) == 0
        assert R.loglik([1, 0], [3, 6], 0, rho) == R.loglik_gamma([1, 0], [3, 6], 0, rho) == mp.ninf
        assert R.loglik([4, 10], [4, 11], 1, rho) == R.loglik_gamma([4, 10], [4, 11], 1, rho) == mp.ninf


def test_rho_zero_is_the_binomial_and_the_limit_is_continuous():
    with mp.workdps(R.DPS):
        for y, n in SMALL:
            for mu in (0.3, 1e-9, 1 - 1e-9):
                mu_ = mp.mpf(mu)
                binom = sum(yj * mp.log(mu_) + (nj - yj) * mp.log(1 - mu_) for yj, nj in zip(y, n))
                assert abs(R.loglik(y, n, mu, 0) - binom) <= mp.mpf(10) ** -40
                assert abs(R.loglik_gamma(y, n, mu, 0) - binom) <= mp.mpf(10) ** -40
                # l(mu, rho) - l(mu, 0) = O(rho): below 1e-12 at rho = 1e-30 for these rows (slopes up to ~1e13 at mu = 1e-9)
                assert abs(R.loglik_gamma(y, n, mu, mp.mpf(10) ** -30) - binom) <= mp.mpf(10) ** -12


def test_concave_in_mu():
    with mp.workdps(R.DPS):
        h = mp.mpf(10) ** -6
        for y, n in SMALL:
            for rho in (0, 1e-6, 0.05, 0.6, 0.999):
                for mu in (0.01, 0.2, 0.5, 0.93):
                    f = [R.loglik_gamma(y, n, mp.mpf(mu) + k * h, rho) for k in (-1, 0, 1)]
                    assert f[0] - 2 * f[1] + f[2] <= 0, (y, n, rho, mu)


def test_pure_binomial_one_plus_two_by_hand():
    # 2 of 10 against 8 of 20 and 12 of 30: condition 2's samples agree exactly and the three together are closer than binomial
    # draws, so both models end at rho = 0 and the statistic is the binomial G-test's
    ref = R.fit([2, 8, 12], [10, 20, 30], 1, 2)
    assert ref["cert"] and ref["rho"] == 0.0 and ref["reduced"]["rho"] == 0
    assert ref["mu1"] == 0.2 and ref["mu2"] == 0.4 and float(ref["reduced"]["mus"][0]) == 22 / 60
    xl = lambda k, p: k * math.log(p)
    by_hand = 2 * ((xl(2, 0.2) + xl(8, 0.8)) + (xl(20, 0.4) + xl(30, 0.6)) - (xl(22, 22 / 60) + xl(38, 38 / 60)))
    assert abs(ref["stat"] - by_hand) <= 1e-13
    assert abs(ref["p"] - math.erfc(math.sqrt(by_hand / 2))) <= 1e-14


def test_na_rules_of_the_reference():
    good = ([2, 8, 12, 5], [10, 20, 30, 9])
    assert R.prepare(*good, 2, 2) is not None
    for j, (c, t) in enumerate([(math.nan, 10), (3, math.nan), (-1, 10), (3, math.inf), (3, 2.0 ** 40 + 2), (11, 10)]):
        count, total = list(good[0]), list(good[1])
        count[j % 4], total[j % 4] = c, t
        assert R.prepare(count, total, 2, 2) is None, (c, t)
    assert R.prepare([0, 0, 12, 5], [0, 0, 30, 9], 2, 2) is None              # condition 1 has no informative sample
    assert R.prepare([2, 0, 12, 0], [10, 0, 30, 0], 2, 2) is None             # two informative samples
    assert R.prepare([2, 0, 12, 5], [10, 0, 30, 9], 2, 2) is not None         # three
    assert R.prepare([2.5, 7.5, 12, 5], [10.4, 20, 30, 9], 2, 2)[0][:2] == [2, 8]      # half to even
    assert R.prepare([2, 8, 12, 5], [2.0 ** 40, 20, 30, 9], 2, 2) is not None


def test_golden_rows_cover_the_designs_bands_and_kinds():
    rows = R.golden_rows()
    assert len(rows) == len(R.DESIGNS) * len(R.BANDS) * len(R.KINDS)
    seen = {(r["design"], r["band"], r["kind"]) for r in rows}
    assert seen == {(d, b, k) for d in R.DESIGNS for b in R.BANDS for k in R.KINDS}
    for r in rows:
        n1, n2 = r["design"]
        assert r["ref"]["stat"] >= 0 and r["ref"]["lf"] >= r["ref"]["lr"] - mp.mpf(10) ** -30
        lo, hi = max(2, r["band"] // 2), r["band"] + r["band"] // 2
        informative = r["total"] > 0
        assert ((r["total"][informative] >= lo) & (r["total"][informative] <= hi)).all()
        # the maxima on the boundary that three kinds are there to show, and a sample without reads
        assert R._kind_holds(r["kind"], r["ref"]), (r["design"], r["band"], r["kind"])
        if r["kind"] == "with_empty" and n1 + n2 >= 4:
            assert (~informative).sum() == 1
    assert sum(0 < r["ref"]["rho"] < R.RHO_MAX_F for r in rows) >= 100          # and interior ones


@pytest.mark.parametrize("deep", [False, True], ids=["bands", "deep"])
@pytest.mark.parametrize("design", R.DESIGNS, ids=lambda d: "%d+%d" % d)
def test_every_golden_row_carries_a_certificate(design, deep):
    """What keeps the GPU tests from resting on an unproved unimodality: the stored maximum of either model of every row they use
    (rows.json, and deep_rows.json for the deeper totals) is certified here from the point alone -- derivatives at 50 digits,
    boundary signs, one local maximum on the rho grid."""
    n1, n2 = design
    rows = [r for r in R.golden_rows(deep) if r["design"] == design]
    assert len(rows) == len(R.KINDS) * len(R.DEEP_BANDS if deep else R.BANDS)
    assert {r["band"] for r in rows} == set(R.DEEP_BANDS if deep else R.BANDS)
    for r in rows:
        ref = r["ref"]
        assert r["total"].max() <= 2.0 ** 40
        for name in ("full", "reduced"):
            groups = R.groups_of(ref["y"], ref["n"], n1, name == "full")
            maxima = R.count_maxima(R._profile_double(groups, R.GRID)[0], R.grid_noise(groups))
            ok, worst = R.certify(groups, ref[name]["mus"], ref[name]["rho"], maxima)
            assert ok, (design, r["band"], r["kind"], name, maxima, worst)


def test_golden_file_is_what_the_generator_gives():
    fresh = R.reference_rows(designs=((2, 2),), bands=(10, 1000))
    stored = [r for r in R.golden_rows() if r["design"] == (2, 2) and r["band"] in (10, 1000)]
    assert len(fresh) == len(stored) == 2 * len(R.KINDS)
    for a, b in zip(fresh, stored):
        assert a["kind"] == b["kind"] and a["count"].tolist() == b["count"].tolist() and a["total"].tolist() == b["total"].tolist()
        assert a["ref"]["cert"]
        assert abs(a["ref"]["lf"] - b["ref"]["lf"]) <= mp.mpf(10) ** -40 and abs(a["ref"]["lr"] - b["ref"]["lr"]) <= mp.mpf(10) ** -40
        assert (a["ref"]["mu1"], a["ref"]["mu2"], a["ref"]["rho"]) == (b["ref"]["mu1"], b["ref"]["mu2"], b["ref"]["rho"])


def test_count_maxima():
    assert R.count_maxima([0, 1, 2, 1, 0], 0.1) == 1
    assert R.count_maxima([3, 2, 1], 0.1) == 1 and R.count_maxima([1, 2, 3], 0.1) == 1 and R.count_maxima([1, 1, 1], 0.1) == 1
    assert R.count_maxima([0, 2, 1, 3, 0], 0.1) == 2 and R.count_maxima([2, 0, 2], 0.1) == 2
    assert R.count_maxima([0, 2, 1.95, 3, 0], 0.1) == 1          # a dip below the tolerance


# ---- the readers ------------------------------------------------------------------------------------------------------------------------

def _same_input(a, b):
    assert a.ids == b.ids
    assert a.values.tobytes() == b.values.tobytes() and a.totals.tobytes() == b.totals.tobytes()


def test_readers_give_betabin_what_they_give_lrt(tmp_path):
    a = os.path.join(GOLD, "wild_s13", "count.out")
    _same_input(ds.read_tables("betabin", [a, a, a, a], 2, 2), ds.read_tables("lrt", [a, a, a, a], 2, 2))
    m = os.path.join(GOLD, "multi_method", "count.out")
    got = ds.read_tables("betabin", [m, m, m], 1, 2)
    _same_input(got, ds.read_tables("lrt", [m, m, m], 1, 2))
    assert got.totals is not None and got.totals.shape == got.values.shape
    one, all_ = tmp_path / "one.txt", tmp_path / "all.txt"
    one.write_text("ID\ta\tb\tc\nf1\t1\t2\t3\nf2\t5\tNA\t7.5\n")
    all_.write_text("ID\ta\tb\tc\nf1\t10\t20\t30\nf2\t50\t60\tInf\n")
    got = ds.read_matrix("betabin", [str(one), str(all_)], 2, 1)
    _same_input(got, ds.read_matrix("lrt", [str(one), str(all_)], 2, 1))
    assert got.values[0].tolist() == [1, 2, 3] and got.totals[0].tolist() == [10, 20, 30]
    # lrt's checks: a negative count, mismatched IDs
    neg = tmp_path / "neg.txt"
    neg.write_text("ID\ta\tb\tc\nf1\t1\t-2\t3\nf2\t5\t6\t7\n")
    with pytest.raises(L.LsqError, match="negative"):
        ds.read_matrix("betabin", [str(neg), str(all_)], 2, 1)
    other = tmp_path / "other.txt"
    other.write_text("ID\ta\tb\tc\nf1\t10\t20\t30\nf3\t50\t60\t70\n")
    with pytest.raises(L.LsqError, match="f3"):
        ds.read_matrix("betabin", [str(one), str(other)], 2, 1)


def test_betabin_with_two_samples_is_an_argument_error(tmp_path, capfd):
    a = os.path.join(GOLD, "toy", "count.out")
    with pytest.raises(L.LsqError, match="at least 3 samples"):
        ds.read_tables("betabin", [a, a], 1, 1)
    one = tmp_path / "one.txt"
    one.write_text("ID\ta\tb\nf1\t1\t2\n")
    with pytest.raises(L.LsqError, match="at least 3 samples"):
        ds.read_matrix("betabin", [str(one), str(one)], 1, 1)
    assert len(ds.read_matrix("lrt", [str(one), str(one)], 1, 1).ids) == 1            # lrt takes the same files
    # the executable answers with its usage text, before any device is opened
    for argv in (["betabin", str(one), str(one), "1", "1", "-"], ["betabin", "--tables", "1", "1", "-", a, a]):
        rc, text = L.cli_run("test_as", argv)
        err = capfd.readouterr().err
        assert rc == 1 and text == "" and "Usage" in err and "test_as betabin --tables" in err, (rc, err)


def test_unknown_test_message_lists_betabin(tmp_path):
    with pytest.raises(L.LsqError, match="fisher, lrt, wilcox, betabin"):
        ds.read_matrix("median", [str(tmp_path / "x")], 2, 2)
