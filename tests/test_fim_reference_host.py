"""The reference of the direct Fisher information tests (tests/fim_ref.py) held against what it claims, on the CPU: against
the oracle's double-precision restatement of fim.h on the golden inputs, against cases worked out by hand, its one-by-one
start counts against the library's accessible read starts, and the direct set against the conditions its GPU test relies
on.  No device call."""
from fractions import Fraction

import numpy as np
import pytest

import lesseq_amd as L
import oracle_binding as ob
import em_ref as R
import fim_ref as F
from test_oracle_golden import load_case, runs

GOLDEN = ["toy", "events_s1", "events_s2", "multi_method", "wild_s11", "wild_s12", "wild_s13", "quirks"]


def geometry(ev, e):
    """an event of the library as the reference takes it: (segment lengths, [segment indices per isoform])"""
    seg_len = [b - a for a, b in ev.segments(e)]
    return seg_len, [[n for n in range(len(seg_len)) if ev.isoform_mask(e, j) >> n & 1] for j in range(ev.K(e))]


@pytest.mark.parametrize("name", GOLDEN)
def test_exact_reference_agrees_with_the_oracles_restatement(name, tmp_path, monkeypatch):
    """the oracle's own theta and G = 1 / ARS go into the exact reference: matrices within 1e-9 of the matrix's largest entry,
    by_diag within 1e-7 relative (inf where the reference says inf), by_inv within 1e-7 relative where the reference's own
    by_inv bound is below that; EVERY event with at most six isoforms is checked"""
    monkeypatch.setenv("LSQO_FIM", "1")
    c, d = load_case(name, tmp_path)
    monkeypatch.chdir(d)
    eligible = checked = inverses = 0
    for tool, r in runs(c):
        if tool != "solve" or r["exit"] != 0:
            continue
        argv = r["argv"]
        rc, _, exact = ob.run("solve", argv)
        assert rc == 0
        groups = [argv[9 + i * 5: 9 + (i + 1) * 5] for i in range((len(argv) - 9) // 5)]
        ev = L.Events(L.Annotation(argv[4], argv[6], int(argv[7]), int(argv[8]), argv[3], argv[5]),
                      tuple(g[1] for g in groups), tuple(int(g[2]) for g in groups))
        assert len(ev) == len(exact)
        for e, o in enumerate(exact):
            assert ev.gene_name(e) == o["gname"] and ev.K(e) == o["K"]
            if o["K"] > 6:
                assert "fim" not in o
                continue
            eligible += 1
            seg_len, isoforms = geometry(ev, e)
            for m, g in enumerate(groups):
                short = g[1] != "MEDIUM_READ"
                ars = [ev.ars(m, e, j) for j in range(o["K"])]
                f = F.fim(seg_len, isoforms, int(g[2]), short, o["theta"], F.G_of(ars))
                assert [sum(s.values()) for s in f.starts] == ars, (name, o["gname"], m)
                D = o["K"] - 1
                scale = max((abs(x) for row in f.I for x in row), default=Fraction(0))
                for p in range(D):
                    for q in range(D):
                        assert abs(Fraction(o["fim"][m][p][q]) - f.I[p][q]) <= Fraction(1e-9) * scale, (name, o["gname"], m, p, q, o["fim"][m][p][q], float(f.I[p][q]))
                by_diag, by_inv = o["fim_var"][m]
                if f.by_diag == F.INF:
                    assert by_diag == F.INF, (name, o["gname"], m, by_diag)
                else:
                    assert abs(Fraction(by_diag) - f.by_diag) <= Fraction(1e-7) * f.by_diag, (name, o["gname"], m, by_diag, float(f.by_diag))
                if f.det != 0 and f.by_inv_rel_bound() < 1e-7:
                    assert abs(Fraction(by_inv) - f.by_inv) <= Fraction(1e-7) * abs(f.by_inv), (name, o["gname"], m, by_inv, float(f.by_inv))
                    inverses += 1
            checked += 1
    print("%s: %d events with at most six isoforms, %d checked, %d inverses compared" % (name, eligible, checked, inverses))
    assert checked == eligible and eligible >= 1


def test_cases_worked_out_by_hand():
    # K = 1: nothing to estimate -- the empty matrix, both variances 0
    f = F.fim([80], [[0]], 10, True, [1.0], [1.0 / 71])
    assert f.I == [] and f.by_diag == 0 and f.by_inv == 0 and f.det == 1 and f.T == 1 and f.starts == [{1: 71}]
    # K = 2, a cassette exon: segments of 20, 10, 20 bases, isoform 0 all three (50 bases), isoform 1 without the middle one
    # (40 bases), MEDIUM reads of 10: 41 and 31 accessible starts.  Isoform 0's reads: starts 0 .. 10 lie in segment 0 and
    # starts 30 .. 40 in segment 2 -- compatible with both isoforms, 22 starts; starts 11 .. 29 touch the middle segment, 19
    # starts of isoform 0 alone.  Isoform 1's: starts 0 .. 10 and 20 .. 30 both isoforms, 22; starts 11 .. 19 span its junction,
    # 9 of isoform 1 alone.  With theta = (1/2, 1/2), G = (1/41, 1/31), a = G0, b = G1:
    #   both:  d = a - b, s = (a + b) / 2, 22 starts of weight a / 2 and 22 of weight b / 2:  22 (a + b) / 2 * (a - b)^2 * 4 / (a + b)^2
    #   0 alone:  d = a, s = a / 2:   19 * a / 2 * a^2 * 4 / a^2 = 38 a
    #   1 alone:  d = -b, s = b / 2:   9 * b / 2 * 4 = 18 b
    #   I = 44 (a - b)^2 / (a + b) + 38 a + 18 b;  a - b = -10 / 1271, a + b = 72 / 1271:  44 * 100 / (72 * 1271) = 550 / 11439,
    #   38 / 41 + 18 / 31 = 1916 / 1271 = 17244 / 11439;  I = 17794 / 11439 = 14 / 9
    f = F.fim([20, 10, 20], [[0, 1, 2], [0, 2]], 10, False, [0.5, 0.5], [Fraction(1, 41), Fraction(1, 31)])
    assert f.starts == [{3: 22, 1: 19}, {3: 22, 2: 9}] and f.T == 4
    assert f.I == [[Fraction(14, 9)]] and f.A == f.I and f.det == Fraction(14, 9)
    assert f.by_diag == Fraction(9, 14) and f.by_inv == Fraction(9, 7) and f.kappa == 1 and f.S == Fraction(9, 7)
    assert f.matrix_bound(0, 0) == 4 * (4 + 4 + 10) * F.EPS * Fraction(14, 9) and f.by_diag_rel_bound() == (72 + 1 + 2) * F.EPS
    assert f.by_inv_bound() == (72 + 3) * F.EPS * Fraction(9, 7)
    # SHORT reads on the same event: every segment before the last contributes one start more, 43 and 32, and the doubled
    # boundary starts generate the read of the next segment's first base: isoform 0's start 20 (the middle segment alone) and
    # start 30 (the last segment alone, both isoforms) are visited twice, isoform 1's start 20 likewise
    f = F.fim([20, 10, 20], [[0, 1, 2], [0, 2]], 10, True, [0.5, 0.5], [Fraction(1, 43), Fraction(1, 32)])
    assert f.starts == [{3: 23, 1: 20}, {3: 23, 2: 9}]
    assert F.accessible_start_lengths([20, 10, 20], 10, True) == [21, 11, 11] and F.accessible_starts([3, 4], 2, True) == [0, 1, 2, 3, 3, 4, 5]
    # less than a read left: 60 + 3 + 4 bases, reads of 10 -- the first segment is the one, it contributes 60 + 1 - (60 + 10 - 67)
    assert F.accessible_start_lengths([60, 3, 4], 10, False) == [58, 0, 0] == F.accessible_start_lengths([60, 3, 4], 10, True)
    assert F.accessible_start_lengths([4, 6], 10, True) == [1, 0] and F.accessible_start_lengths([5, 3], 10, True) == [0, 0]
    # theta_k = 0: the isoform's starts are not visited (but its G still stands in the differences)
    g = F.fim([20, 10, 20], [[0, 1, 2], [0, 2]], 10, False, [1.0, 0.0], [Fraction(1, 41), Fraction(1, 31)])
    assert g.T == 2 and g.I == [[Fraction(41) * 22 * Fraction(-10, 1271) ** 2 + 19 * Fraction(1, 41)]]
    # one class carries every start: isoform 0 is one segment that every isoform begins with, theta = (1, 0, ..): the matrix is
    # n G_0 (d d^T) / G_0^2 with d_p = G_p - G_K -- rank one, singular exactly for D >= 2, regular for D = 1
    for K in (2, 3, 5):
        seg_len = [50, 30, 75, 41, 18][:K]
        isoforms = [[0]] + [[0, j] for j in range(1, K)]
        G = [Fraction(1, 41 + 30 * j) for j in range(K)]
        f = F.fim(seg_len, isoforms, 10, False, [1.0] + [0.0] * (K - 1), G)
        assert f.starts[0] == {(1 << K) - 1: 41} and f.T == 1
        d = [G[p] - G[K - 1] for p in range(K - 1)]
        assert f.I == [[41 * G[0] * d[p] * d[q] / G[0] ** 2 for q in range(K - 1)] for p in range(K - 1)]
        assert (f.det == 0) == (K > 2) and f.by_diag != F.INF
    # the exact inverse
    det, inv = F._det_and_inverse([[Fraction(0), Fraction(2)], [Fraction(3), Fraction(4)]])
    assert det == -6 and inv == [[Fraction(-2, 3), Fraction(1, 3)], [Fraction(1, 2), Fraction(0)]]
    assert F.error_ratio(1.0, Fraction(1), Fraction(0)) == 0 and F.error_ratio(1.5, Fraction(1), Fraction(1)) == 0.5
    assert F.error_ratio(float("nan"), Fraction(1), Fraction(1)) == F.INF and F.error_ratio(1.5, Fraction(1), Fraction(0)) == F.INF


def direct_events(directory):
    """the direct set compiled by the library, held against the set's own geometry: names in output order, K, segments (from
    the gene's first base), isoforms' segments and accessible read starts of both read files"""
    iv, mp = R.write_annotation(str(directory), "fim", F.direct_genes())
    ev = L.Events(L.Annotation(iv, mp), tuple(t for t, _ in F.READ_FILES), tuple(n for _, n in F.READ_FILES))
    cases = F.direct_set()
    assert len(ev) == len(cases) and L.lib.lsq_events_host_genes(ev.h) == 0
    for e, c in enumerate(cases):
        assert ev.gene_name(e) == c.name and ev.K(e) == c.K, c.name
        segs = ev.segments(e)
        base = segs[0][0] - c.segments[0][0]
        assert [(a - base, b - base) for a, b in segs] == c.segments, c.name
        assert geometry(ev, e) == (c.seg_len, c.isoforms), c.name
        assert [[ev.ars(m, e, j) for j in range(c.K)] for m in range(len(F.READ_FILES))] == c.ars, c.name
    return ev


def reference_thetas():
    """em_ref's theta of every event of the set where its loop ends, and that no event comes near the threshold (no flag)"""
    out = []
    for c in F.direct_set():
        T = R.em_trajectory(c.K, c.ars, c.counts)
        assert not T.near_threshold(), c.name
        out.append(T.theta[T.stop])
    return out


def test_one_by_one_start_counts_sum_to_the_accessible_read_starts(tmp_path):
    ev = direct_events(tmp_path)
    n = 0
    for e, c in enumerate(F.direct_set()):
        for m, (rt, rl) in enumerate(F.READ_FILES):
            f = F.reference_at(c, m, [1.0 / c.K] * c.K)
            for k in range(c.K):
                assert sum(f.starts[k].values()) == ev.ars(m, e, k), (c.name, m, k)
                assert all(cls >> k & 1 and 0 < cls < 1 << c.K for cls in f.starts[k]), (c.name, m, k)      # its own reads fit the isoform
                n += 1
    assert n == 2 * sum(c.K for c in F.direct_set())


def test_direct_set_meets_the_conditions_of_its_gpu_test():
    """at em_ref's theta, which the device's agrees with to 1e-6 (tests/test_em_direct_gpu.py): no flag, every K, both read
    files, every geometry edge, every count pattern doing what it is there for, two thirds of the regular cases strict"""
    cases = F.direct_set()
    thetas = reference_thetas()
    refs = [[F.reference_at(c, m, th) for m in range(len(F.READ_FILES))] for c, th in zip(cases, thetas)]
    got = F.coverage(cases, thetas, refs)
    print(got)
    assert 140 <= got["events"] <= 160
    assert F.READ_FILES[0][0] == "SHORT_READ" and F.READ_FILES[1][0] == "MEDIUM_READ" and F.READ_FILES[0][1] != F.READ_FILES[1][1]
    # the random structures keep to what they are to be: at most 8 segments of 1 .. 60 bases
    for c in cases:
        if c.structure.startswith("random"):
            assert c.K >= 4 and len(c.seg_len) <= 8 and all(1 <= l <= 60 for l in c.seg_len) and len({tuple(i) for i in c.isoforms}) == c.K
    assert np.isfinite([x for th in thetas for x in th]).all()
