"""The reference of the direct EM tests (tests/em_ref.py) checked on the CPU: against the oracle's per-read EM, against
the conditions its case sets have to meet, and the acceptance rule against made-up kernel results.  No device call."""
import math

import numpy as np
import pytest

import lesseq_amd as L
import oracle_binding as ob
import em_ref as R


def rows_of(K, ars, counts):
    """one read file's class counts expanded to the per-read rows of the oracle: G_j where the class holds j, else 0"""
    g = [0.0 if a == 0 else 1.0 / a for a in ars]
    rows = []
    for c in range(1, 1 << K):
        rows += [[g[j] if c >> j & 1 else 0.0 for j in range(K)]] * int(counts[c - 1])
    return rows


def small_cases():
    """K = 2 .. 6, one read file, up to a few hundred rows: random sparse counts, every class once, lone classes"""
    rng = np.random.default_rng(7)
    out = []
    for K, lengths in enumerate(R.GENERAL_STRUCTURES[1:], 2):
        ars = [x - 99 for x in lengths]
        nc = (1 << K) - 1
        for trial in range(6):
            cnt = [int(rng.integers(1, 40)) if rng.random() < (0.6 if K < 5 else 0.15) else 0 for _ in range(nc)]
            cnt[nc - 1] += 1
            out.append((K, ars, cnt))
        out.append((K, ars, [1] * nc))
        out.append((K, ars, [5 if c + 1 == 1 << (K - 1) else 0 for c in range(nc)]))
    for _, sname, ars, tr in R.lean_cases():
        if 0 < sum(tr) <= 400 and sname != "ars0" and not (sname == "ars1" and tr[1] == 0 and tr[2] > 0):       # (see the degenerate rows)
            out.append((2, list(ars), list(tr)))
    return out


def test_decimal_reference_agrees_with_the_oracles_per_read_em():
    cases = small_cases()
    assert len(cases) > 80 and {c[0] for c in cases} == {2, 3, 4, 5, 6}
    n_exact = 0
    for K, ars, cnt in cases:
        rows = rows_of(K, ars, cnt)
        assert 0 < len(rows) <= 800
        theta, ll, it = ob.em_rows(K, rows)
        T = R.em_trajectory(K, [ars], [cnt])
        if not T.near_threshold():
            assert it == T.stop, (K, ars, cnt, it, T.stop)
            n_exact += 1
        if it < len(T.theta):
            for a, b in zip(theta, T.theta[it]):
                assert abs(a - b) <= 1e-9, (K, ars, cnt, a, b)
            assert abs(ll - T.ll[it]) <= 1e-9 * max(abs(ll), 1.0) or ll == T.ll[it], (K, ars, cnt, ll, T.ll[it])
    assert n_exact >= 0.9 * len(cases)


def test_degenerate_rows_follow_the_oracle_and_ieee():
    # no reads
    T = R.em_trajectory(3, [[10, 20, 30]], [[0] * 7])
    assert T.stop == 0 and T.theta[0] == [1 / 3] * 3 and T.ll[0] == 0.0
    # K == 1: theta 1, no iteration, the log-likelihood of theta = 1
    T = R.em_trajectory(1, [[201], [251]], [[7], [2]])
    assert T.stop == 0 and T.theta[0] == [1.0] and abs(T.ll[0] - (7 * math.log(1 / 201) + 2 * math.log(1 / 251))) < 1e-12
    # reads in a class whose isoforms all have G = 0: -inf, no number, one iteration -- as the oracle's loop does it
    T = R.em_trajectory(2, [[0, 101]], [[3, 5, 9]])
    assert T.stop == 1 and T.ll[0] == -math.inf and T.ll[1] == -math.inf and T.crit[1] != T.crit[1]
    theta, ll, it = ob.em_rows(2, rows_of(2, [0, 101], [3, 5, 9]))
    assert it == 1 and ll == -math.inf and np.allclose(theta, T.theta[1], rtol=0, atol=1e-15)
    th, ll, it = R.em_float64(2, [[0, 101]], [[3, 5, 9]])
    assert it == 1 and ll == -math.inf
    # an isoform without accessible starts beside one with them, no read on it alone: an ordinary event
    T = R.em_trajectory(2, [[0, 101]], [[0, 5, 9]])
    assert T.stop >= 1 and math.isfinite(T.ll[T.stop]) and T.theta[T.stop] == [0.0, 1.0]
    # a log-likelihood of exactly zero (ARS 1, every read on that isoform): x / 0 goes on, 0 / 0 ends the loop
    T = R.em_trajectory(2, [[1, 51]], [[5, 0, 0]])
    theta, ll, it = ob.em_rows(2, rows_of(2, [1, 51], [5, 0, 0]))
    assert T.stop == it == 2 and T.ll[2] == ll == 0.0 and T.crit[1] == math.inf and T.crit[2] != T.crit[2]
    # ... and where theta only APPROACHES (1, 0) -- reads on both isoforms beside those on the ARS-1 isoform alone -- the test value
    # tends to 1 / kappa - 1, far above 1e-6, in exact arithmetic: the loop ends only because float64 runs out of digits,
    # at an iteration that rounding decides (the oracle's per-read sums: one earlier than the rule of em_ref.py here)
    T = R.em_trajectory(2, [[1, 51]], [[3, 0, 50]])
    theta, ll, it = ob.em_rows(2, rows_of(2, [1, 51], [3, 0, 50]))
    assert T.rounding_stop and abs(T.stop - it) <= 1 and T.ll[T.stop] == ll == 0.0, (T.stop, it, ll)
    assert all(c > 1.0 for c in T.crit[2:T.stop - 1])                       # nowhere near 1e-6 before the digits run out
    assert not R.em_trajectory(2, [[201, 81]], [[3, 0, 50]]).rounding_stop


SETS = ["lean", "general1", "general2", "general3", "general8"]


def the_set(name):
    if name == "lean":
        return R.lean_kac(), R.lean_trajectories()
    M = int(name[len("general"):])
    return R.general_kac(M), R.general_trajectories(M)


@pytest.mark.parametrize("name", SETS)
def test_case_sets_keep_clear_of_the_threshold(name):
    """at most 10 % of a set's events come within W of the threshold at any iteration: the exact-iteration rule bites on the rest"""
    kac, tr = the_set(name)
    near = sum(T.near_threshold() for T in tr)
    print("%s: %d of %d events within %g of the threshold" % (name, near, len(tr), R.W))
    assert near <= 0.10 * len(tr)
    assert R.W == 1e-9


def test_lean_set_holds_what_the_path_tests_need():
    cases, tr = R.lean_cases(), R.lean_trajectories()
    assert len(cases) == 6 * 64
    stops = [T.stop for T in tr]
    assert sum(1 for s in stops if 0 < s < 6) >= 50           # done inside the head, and under every cap but 1
    assert sum(1 for s in stops if 7 <= s <= 31) >= 20        # past the head and the cap of 6, below the split of a learnt placement
    assert sum(1 for s in stops if s > 48) >= 10              # past the cap of 48; four lanes an event under a learnt placement
    # the closed form's linear branch: G0 == G1, reads on both isoforms alone, still running after the head's six iterations
    assert any(c[1] == "equal" and c[3][0] >= 1 and c[3][1] >= 1 and T.stop > 6 for c, T in zip(cases, tr))
    # a fixed point on the boundary: reads on one isoform alone and on both, none on the other alone, G0, G1 < 1
    edge = [T for c, T in zip(cases, tr) if c[1] in ("unequal", "equal", "differ1", "ratio100") and T.stop > 6 and c[3][2] > 0 and (c[3][0] == 0) != (c[3][1] == 0)]
    assert sum(1 for T in edge if min(T.theta[T.stop]) < 0.05) >= 4         # (attracting where b G_other / G_own < 1; the others end inside)
    # G == 1 beside reads on one isoform alone: the tail kernel's exclusion
    assert any(c[1] == "ars1" and T.stop > 6 for c, T in zip(cases, tr))
    # the triples the issue names
    have = {c[3] for c in cases}
    for t in [(0, 0, 0), (1, 1, 10), (1, 1, 10 ** 3), (1, 1, 10 ** 6), (1, 1, 10 ** 9), (1, 10 ** 9, 0), (10 ** 9, 1, 10 ** 9),
              (2 ** 31 - 1, 0, 0), (2 ** 31 + 1, 0, 0), (2 ** 32 - 1, 0, 0), (2 ** 32 + 1, 0, 0), (2 ** 40, 0, 0)]:
        assert t in have, t


def test_structures_have_the_ars_they_are_meant_to_have(tmp_path):
    iv, mp = R.write_annotation(str(tmp_path), "lean", R.lean_genes())
    ev = L.Events(L.Annotation(iv, mp), ("SHORT_READ",), (R.LEAN_READ_LENGTH,))
    cases = R.lean_cases()
    assert len(ev) == len(cases)
    for e, (gname, sname, ars, _) in enumerate(cases):
        assert ev.gene_name(e) == gname and ev.K(e) == 2
        assert (ev.ars(0, e, 0), ev.ars(0, e, 1)) == ars, gname
    a = R.LEAN_ARS
    assert a["equal"][0] == a["equal"][1] and abs(a["differ1"][0] - a["differ1"][1]) == 1 and a["ratio100"][0] >= 100 * a["ratio100"][1]
    assert a["ars1"][0] == 1 and a["ars0"][0] == 0 and a["unequal"][0] != a["unequal"][1]
    for M in (1, 2, 3, 8):
        iv, mp = R.write_annotation(str(tmp_path), "g%d" % M, R.general_genes(M))
        ev = L.Events(L.Annotation(iv, mp), ("SHORT_READ",) * M, R.GENERAL_READ_LENGTHS[:M])
        for e, (gname, K, lengths, ars, counts) in enumerate(R.general_cases(M)):
            assert ev.gene_name(e) == gname and ev.K(e) == K and ev.N(e) <= 32
            assert [[ev.ars(m, e, j) for j in range(K)] for m in range(M)] == ars, gname
        assert L.lib.lsq_events_host_genes(ev.h) == 0


def test_float64_em_stays_within_the_measured_deviation():
    """the sharp bound's source: the plain float64 EM against the decimal reference over all case sets, at equal iteration
    counts; and the two agree on the iteration count wherever the trajectory keeps clear of the threshold"""
    dth = dll = 0.0
    for name in SETS:
        kac, tr = the_set(name)
        for (K, ars, cnt), T in zip(kac, tr):
            th, ll, it = R.em_float64(K, ars, cnt)
            if not T.near_threshold():
                assert it == T.stop, (name, K, ars, cnt, it, T.stop)
            if T.stop == 0:
                continue
            th, ll, it = R.em_float64(K, ars, cnt, T.stop)
            dth = max(dth, max(abs(float(a) - float(b)) for a, b in zip(th, T.theta_dec[T.stop])))
            w = T.ll[T.stop]
            if math.isfinite(w) and w != 0:
                dll = max(dll, abs(ll - w) / abs(w))
            else:
                assert ll == w or (ll != ll and w != w), (name, K, ars, cnt, ll, w)
    print("largest deviation of the float64 EM: theta %.3g absolute, log-likelihood %.3g relative" % (dth, dll))
    assert dth <= R.MEASURED_THETA_DEV and dll <= R.MEASURED_LL_DEV
    assert dth >= R.MEASURED_THETA_DEV / 4 and dll >= R.MEASURED_LL_DEV / 4          # the constants are the measurement, not a guess far above it
    assert R.SHARP_THETA_ABS == min(1000 * R.MEASURED_THETA_DEV, R.REL_TOL) and R.SHARP_LL_REL == min(1000 * R.MEASURED_LL_DEV, R.REL_TOL)


def test_acceptance_rule():
    kac = (2, [[151, 152]], [[30, 50, 100000]])          # comes within W of the threshold at its stop (lean set, differ1)
    T = R.em_trajectory(*kac)
    assert T.near_threshold() and T.stop > 48
    s = T.stop
    ok = lambda t, flags, theta=None, ll=None: R.accept(T, T.theta[t] if theta is None else theta, T.ll[t] if ll is None else ll, t, flags)
    assert ok(s, 0) is None and ok(s, 1) is None
    assert ok(s - 1, 0) is not None and ok(s + 1, 0, theta=T.theta[s], ll=T.ll[s]) is not None              # unflagged: the reference's iteration, nothing else
    assert ok(s - 3, 1) is not None                                           # flagged, but stopped where the test value is far above
    assert ok(s, 2) is not None and ok(s, 4) is not None and ok(s, 5) is not None and ok(s, 3) is not None
    th = list(T.theta[s]); th[0] += 1e-10
    assert ok(s, 0, theta=th) is not None                                     # inside REL_TOL, outside the sharp bound
    assert R.accept(T, th, T.ll[s], s, 0, sharp=False) is None
    assert ok(s, 0, ll=T.ll[s] * (1 + 3e-6)) is not None
    far = R.em_trajectory(2, [[201, 81]], [[3, 5, 2000]])                     # keeps clear of the threshold
    assert not far.near_threshold()
    assert R.accept(far, far.theta[far.stop], far.ll[far.stop], far.stop, 1) is not None      # a flag nothing justifies
    assert R.accept(far, far.theta[far.stop], far.ll[far.stop], far.stop, 0) is None
    nan_t = R.em_trajectory(2, [[0, 101]], [[3, 5, 9]])
    assert R.accept(nan_t, nan_t.theta[1], -math.inf, 1, 0) is None and R.accept(nan_t, nan_t.theta[1], -1.0, 1, 0) is not None


def test_the_probe_is_exported_and_the_abi_version_stays():
    assert hasattr(L.lib, "lsq_debug_last_em_launch") and hasattr(L.Context, "em_launch")
    assert L.lib.lsq_abi_version() == 2
    import os
    dev = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lesseq_hip_dev.h")).read()
    assert "int lsq_debug_last_em_launch(lsq_ctx *c, unsigned out[8]);" in dev
