"""The EM kernels of lsq_em.hip tested directly: class counts chosen by hand go in through lsq_results_set_counts, no
read is involved, and every form of the solve is held against the 40-digit reference of tests/em_ref.py by its
acceptance rule -- after lsq_debug_last_em_launch has said that this form is the one that ran.
Need an MI355X: python -m pytest tests -m gpu."""
import numpy as np
import pytest

import lesseq_amd as L
import em_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("theta", "logll", "iters", "flags")
# The lean set's places: an event with an isoform of ARS 1 (G = 1) is placed with the general kernel, whose loop has the
# reference's own quotients (lsq_em.hip em_quad_body); the five other structures, 64 events each, are the lean group.
LEAN_PLACES, UNIT_G_PLACES = 320, 64


def compile_events(directory, stem, genes, read_lengths, first=0, end=2 ** 62):
    iv, mp = R.write_annotation(str(directory), stem, genes)
    return L.Events(L.Annotation(iv, mp, first, end), ("SHORT_READ",) * len(read_lengths), tuple(read_lengths))


def counts_array(ev, per_event):
    """per_event[e][m][class - 1] -> uint64 [n_methods, n_classes] in output order, and matched bases to go with them"""
    off = ev.class_offsets()
    cnt = np.zeros((ev.n_methods, off[-1]), np.uint64)
    for e, rows in enumerate(per_event):
        for m, row in enumerate(rows):
            assert len(row) == off[e + 1] - off[e]
            cnt[m, off[e]:off[e + 1]] = np.array([int(x) for x in row], np.uint64)
    return cnt, cnt * np.uint64(36)


def context(ev, options=None, band=None):
    ctx = L.Context(0)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    if band is not None:
        ctx.set_em_guard_band(band)
    ctx.upload_events(ev)
    return ctx


def solution(ctx):
    return tuple(x.copy() for x in ctx.solution())


def same_bits(a, b, what):
    for x, y, name in zip(a, b, NAMES):
        if not np.array_equal(x, y, equal_nan=True):
            bad = np.flatnonzero(~((x == y) | ((x != x) & (y != y))))
            raise AssertionError("%s: %s differs at %d places, first %d: %r against %r" % (what, name, len(bad), bad[0], x[bad[0]], y[bad[0]]))


def check_reference(ev, tr, sol, what, only=None):
    """every event's (theta, ll, iters, flags) by the acceptance rule of em_ref.accept (only: a mask of the events to look
    at); returns the number of flagged events"""
    theta, ll, iters, flags = sol
    assert len(tr) == len(ev) == len(ll)
    bad, io, n_flagged = [], 0, 0
    for e, T in enumerate(tr):
        K = ev.K(e)
        assert K == T.K
        if only is None or only[e]:
            why = R.accept(T, theta[io:io + K], ll[e], iters[e], flags[e])
            if why:
                bad.append("%s: %s" % (ev.gene_name(e), why))
            n_flagged += int(flags[e]) & 1
        io += K
    print("%s: %d events, %d flagged, %d refused" % (what, len(tr), n_flagged, len(bad)))
    assert not bad, "%s: %d of %d events refused:\n  %s" % (what, len(bad), len(tr), "\n  ".join(bad[:12]))
    return n_flagged


# ------------------------------------------------------------------------------------------------------- the lean set

@pytest.fixture(scope="module")
def lean(tmp_path_factory):
    """events, counts and reference of the lean set, and its solve four lanes an event (em_regroup = 0): what the other
    forms are held against bit for bit"""
    d = tmp_path_factory.mktemp("lean")
    cases = R.lean_cases()
    ev = compile_events(d, "lean", R.lean_genes(), (R.LEAN_READ_LENGTH,))
    assert len(ev) == len(cases) == 384
    # the structures are what they are meant to be, by the library's own ARS
    for e, (gname, sname, ars, _) in enumerate(cases):
        assert ev.gene_name(e) == gname and ev.K(e) == 2 and (ev.ars(0, e, 0), ev.ars(0, e, 1)) == ars, gname
    a = {s: (ev.ars(0, 64 * i, 0), ev.ars(0, 64 * i, 1)) for i, (s, _, _) in enumerate(R.LEAN_STRUCTURES)}
    assert a["unequal"][0] != a["unequal"][1] and min(a["unequal"]) > 1
    assert a["equal"][0] == a["equal"][1] > 1
    assert abs(a["differ1"][0] - a["differ1"][1]) == 1
    assert a["ratio100"][0] >= 100 * a["ratio100"][1] > 0
    assert a["ars1"][0] == 1 and a["ars1"][1] > 1
    assert a["ars0"][0] == 0 and a["ars0"][1] > 1
    cnt, bases = counts_array(ev, [[list(tr)] for _, _, _, tr in cases])
    ctx = context(ev, {"em_regroup": 0})
    ctx.set_counts(cnt, bases)              # no count() before it: the counts come from outside
    ctx.solve()
    probe = ctx.em_launch()
    sol = solution(ctx)
    got_cnt, got_bases = ctx.counts()
    finalized = ctx.solve_finalize()
    ctx.close()
    tr = R.lean_trajectories()
    # the events whose loop ends on a log-likelihood of exactly 0 (em_ref.py): test_lean_stops_decided_by_rounding holds them
    # against the reference, every other test holds every form's numbers for them against the four-lane form's, bit for bit
    rounding = np.array([T.rounding_stop for T in tr])
    assert 0 < rounding.sum() <= 24 and all(c[1] == "ars1" for c, r in zip(cases, rounding) if r)
    assert sum(1 in c[2] for c in cases) == UNIT_G_PLACES and len(cases) - UNIT_G_PLACES == LEAN_PLACES
    return dict(d=d, ev=ev, cases=cases, cnt=cnt, bases=bases, tr=tr, four_lane=sol, probe=probe, rounding=rounding, plain=~rounding,
                got_counts=(got_cnt.copy(), got_bases.copy()), finalized=finalized)


def test_lean_four_lane(lean):
    p = lean["probe"]
    assert p["lean_form"] == "four_lane" and p["lean_places"] == LEAN_PLACES and p["split"] == LEAN_PLACES and p["general_places"] == UNIT_G_PLACES, p
    assert not p["learnt_placement"] and not p["placement_learnt_after"], p
    n = check_reference(lean["ev"], lean["tr"], lean["four_lane"], "four lanes an event", lean["plain"])
    assert n <= sum(T.near_threshold() for T in lean["tr"])


def test_lean_stops_decided_by_rounding(lean):
    """The events of the lean set whose loop ends on a log-likelihood of exactly 0: an isoform with ARS 1 (G = 1) that takes
    every read.  Where theta reaches (1, 0) in one step -- reads on that isoform alone, 9 events -- any arithmetic agrees with the
    reference.  Where it only approaches it -- reads on both isoforms, none on the other alone, 11 events -- the test value stays
    far above 1e-6 in exact arithmetic and the loop ends at the iteration at which theta rounds to (1, 0): theta's last bit
    decides.  The register forms of the EM, whose 1/s and 1/n are reciprocals and not divisions, held theta_0 at
    1 - 2^-53 .. 1 - 3 * 2^-53 for another iteration or two (measured on an MI355X, every lean form alike: (0, 0, 7) 12
    iterations against the reference's 11, (0, 0, 1000) 13 against 11, (3, 0, 5000) and (0, 0, 2^40) 12 against 11,
    (787384, 0, 4) 5 against 4, and (2382, 0, 4186) a log-likelihood of -2.19e-12 against 0), with no flag set.  Events with an
    isoform of G = 1 are therefore placed with the general kernel and take its loop with the reference's own operations (IEEE
    division, the library's logarithm); this test holds them to the reference's iteration, exactly."""
    check_reference(lean["ev"], lean["tr"], lean["four_lane"], "stops decided by rounding", lean["rounding"])


def test_set_counts_round_trip_and_nothing_replayed(lean):
    """counts() returns what set_counts took; solve_finalize() replays nothing after it (flagged events keep the kernel's numbers)"""
    assert np.array_equal(lean["got_counts"][0], lean["cnt"]) and np.array_equal(lean["got_counts"][1], lean["bases"])
    assert lean["got_counts"][0].dtype == np.uint64 and int(lean["cnt"].max()) == 2 ** 40
    assert lean["finalized"] == 0
    assert not (lean["four_lane"][3] & 4).any()


def test_lean_flat_behind_a_learnt_placement(lean):
    """em_flat_min_events = 0, solved twice: the second solve runs the slow events four lanes an event and the fast ones one lane
    an event, in the order learnt from the first -- the same numbers bit for bit"""
    ctx = context(lean["ev"], {"em_flat_min_events": 0})
    ctx.set_counts(lean["cnt"], lean["bases"])
    ctx.solve()
    p = ctx.em_launch()
    assert p["lean_form"] == "four_lane" and not p["learnt_placement"] and p["placement_learnt_after"] and p["split"] == LEAN_PLACES, p
    same_bits(lean["four_lane"], solution(ctx), "first solve")
    ctx.solve()
    p = ctx.em_launch()
    assert p["lean_form"] == "four_lane_flat3" and p["learnt_placement"] and p["lean_places"] == LEAN_PLACES and p["general_places"] == UNIT_G_PLACES, p
    assert 0 < p["split"] < LEAN_PLACES and p["split"] % 64 == 0, p          # events on both sides (the learnt order has no holes before its end)
    sol = solution(ctx)
    ctx.close()
    same_bits(lean["four_lane"], sol, "one lane an event behind a learnt placement")
    check_reference(lean["ev"], lean["tr"], sol, "four lanes + one lane an event", lean["plain"])


def test_lean_flat_with_a_placement_learnt_on_other_counts(lean):
    """the placement learnt on the same events with every triple rotated, then the counts proper; and one learnt on counts
    that make every event fast, so that EVERY event of the set, the slowest too, is solved one lane an event"""
    ev, cases = lean["ev"], lean["cases"]
    rotated, _ = counts_array(ev, [[[tr[1], tr[2], tr[0]]] for _, _, _, tr in cases])
    quick, _ = counts_array(ev, [[[5, 0, 0]] for _ in cases])
    for what, first, all_flat in (("rotated", rotated, False), ("quick", quick, True)):
        ctx = context(ev, {"em_flat_min_events": 0})
        ctx.set_counts(first, first)
        ctx.solve()
        assert ctx.em_launch()["placement_learnt_after"]
        if all_flat:
            assert int(ctx.solution()[2].max()) < 4        # nothing slow: the learnt split is place 0
        ctx.set_counts(lean["cnt"], lean["bases"])
        ctx.solve()
        p = ctx.em_launch()
        assert p["lean_form"] == "four_lane_flat3" and p["learnt_placement"] and p["lean_places"] == LEAN_PLACES and p["general_places"] == UNIT_G_PLACES, (what, p)
        if all_flat:
            assert p["split"] == 0, p
        sol = solution(ctx)
        ctx.close()
        same_bits(lean["four_lane"], sol, "placement learnt on %s counts" % what)


def test_lean_closed_form(lean):
    """em_closed_form = 1: six ordinary iterations, then the closed form of the EM map in the tail kernel"""
    ctx = context(lean["ev"], {"em_closed_form": 1})
    ctx.set_counts(lean["cnt"], lean["bases"])
    sols = []
    for k in range(2):                       # twice: the tail's list is cleared between the solves
        ctx.solve()
        p = ctx.em_launch()
        assert p["lean_form"] == "head_tail" and p["lean_places"] == LEAN_PLACES and p["general_places"] == UNIT_G_PLACES and not p["learnt_placement"], p
        sols.append(solution(ctx))
    assert ctx.solve_finalize() == 0
    ctx.close()
    same_bits(sols[0], sols[1], "closed form, second solve")
    check_reference(lean["ev"], lean["tr"], sols[0], "head + closed form", lean["plain"])
    rounding = np.flatnonzero(lean["rounding"])          # (G = 1: the tail kernel's ordinary iteration, the four-lane form's arithmetic)
    for x, y, name in zip(lean["four_lane"][1:], sols[0][1:], NAMES[1:]):
        assert np.array_equal(x[rounding], y[rounding], equal_nan=True), name
    # what the head finishes is the four-lane form's arithmetic: bit for bit
    head = np.flatnonzero(lean["four_lane"][2] <= 6)
    assert len(head) > 200
    for x, y, name in zip(lean["four_lane"][1:], sols[0][1:], NAMES[1:]):
        assert np.array_equal(x[head], y[head], equal_nan=True), name


@pytest.mark.parametrize("cap", [1, 6, 48])
def test_lean_capped_four_lane_and_tail(lean, cap):
    """em_quad_cap with em_regroup = 0: the four-lane kernel hands what still runs after `cap` iterations to the tail kernel"""
    ctx = context(lean["ev"], {"em_regroup": 0, "em_quad_cap": cap})
    ctx.set_counts(lean["cnt"], lean["bases"])
    sols = []
    for k in range(2):                       # twice: the tail's list is cleared between the solves
        ctx.solve()
        p = ctx.em_launch()
        assert p["lean_form"] == "four_lane_capped_tail" and p["quad_cap"] == cap and p["lean_places"] == LEAN_PLACES and p["split"] == LEAN_PLACES and p["general_places"] == UNIT_G_PLACES, p
        sols.append(solution(ctx))
    ctx.close()
    same_bits(sols[0], sols[1], "cap %d, second solve" % cap)
    assert (lean["four_lane"][2] > cap).sum() >= 10          # the tail had work
    check_reference(lean["ev"], lean["tr"], sols[0], "cap %d + tail" % cap, lean["plain"])
    rounding = np.flatnonzero(lean["rounding"])
    for x, y, name in zip(lean["four_lane"][1:], sols[0][1:], NAMES[1:]):
        assert np.array_equal(x[rounding], y[rounding], equal_nan=True), name
    below = np.flatnonzero(lean["four_lane"][2] < cap)
    for x, y, name in zip(lean["four_lane"][1:], sols[0][1:], NAMES[1:]):
        assert np.array_equal(x[below], y[below], equal_nan=True), name


@pytest.mark.parametrize("n", [1, 15, 16, 17, 64, 65])
def test_lean_wave_and_workgroup_edges(lean, n):
    """the first n genes alone (Annotation(..., 0, n)), four lanes an event (16 a wave) and one lane an event (64 a workgroup)"""
    iv, mp = str(lean["d"] / "lean.interval"), str(lean["d"] / "lean.map")
    ev = L.Events(L.Annotation(iv, mp, 0, n), ("SHORT_READ",), (R.LEAN_READ_LENGTH,))
    assert len(ev) == n and [ev.gene_name(e) for e in range(n)] == [c[0] for c in lean["cases"][:n]]
    cnt, bases = counts_array(ev, [[list(tr)] for _, _, _, tr in lean["cases"][:n]])
    places = (n + 15) // 16 * 16
    want = (lean["four_lane"][0][:2 * n], lean["four_lane"][1][:n], lean["four_lane"][2][:n], lean["four_lane"][3][:n])
    ctx = context(ev, {"em_regroup": 0})
    ctx.set_counts(cnt, bases)
    ctx.solve()
    p = ctx.em_launch()
    assert p["lean_form"] == "four_lane" and p["lean_places"] == places and p["general_places"] == 0, p
    sol = solution(ctx)
    ctx.close()
    same_bits(want, sol, "four lanes an event, %d genes" % n)
    check_reference(ev, lean["tr"][:n], sol, "four lanes an event, %d genes" % n, lean["plain"][:n])
    # one lane an event for every event: a placement learnt on counts that make all of them fast
    ctx = context(ev, {"em_flat_min_events": 0})
    quick, _ = counts_array(ev, [[[5, 0, 0]]] * n)
    ctx.set_counts(quick, quick)
    ctx.solve()
    ctx.set_counts(cnt, bases)
    ctx.solve()
    p = ctx.em_launch()
    assert p["lean_form"] == "four_lane_flat3" and p["learnt_placement"] and p["split"] == 0 and p["lean_places"] == places, p
    sol = solution(ctx)
    ctx.close()
    same_bits(want, sol, "one lane an event, %d genes" % n)


def test_guard_band_of_one_flags_every_looping_event_and_replays_none(lean):
    """guard band 1.0: every event whose test value comes below 1 + 1e-6 at some iteration is flagged (bit 0) -- that is every
    event that loops to a test value that is a number -- and, the counts being set from outside, none is replayed (bit 2)"""
    ctx = context(lean["ev"], {"em_regroup": 0}, band=1.0)
    ctx.set_counts(lean["cnt"], lean["bases"])
    ctx.solve()
    assert ctx.em_launch()["lean_form"] == "four_lane"
    theta, ll, iters, flags = solution(ctx)
    assert ctx.solve_finalize() == 0
    again = solution(ctx)
    ctx.close()
    same_bits((theta, ll, iters, flags), again, "after solve_finalize")
    same_bits(lean["four_lane"][:3], (theta, ll, iters), "guard band 1.0")
    want = np.array([1 if any(c == c and abs(c - R.THRESHOLD) < 1.0 for c in T.crit[1:T.stop + 1]) else 0 for T in lean["tr"]], np.uint8)
    assert want.sum() > 300
    looping = np.array([T.stop >= 1 and T.crit[T.stop] == T.crit[T.stop] for T in lean["tr"]])
    assert (want[looping] == 1).all()
    plain = lean["plain"]                   # (the others: test_lean_stops_decided_by_rounding)
    assert np.array_equal(flags[plain], want[plain]), np.flatnonzero((flags != want) & plain)[:10]
    assert not (flags & 6).any()


# ---------------------------------------------------------------------------------------------------- the general set

def general_events(tmp, M):
    cases = R.general_cases(M)
    ev = compile_events(tmp, "general%d" % M, R.general_genes(M), R.GENERAL_READ_LENGTHS[:M])
    assert len(ev) == len(cases) == 48
    for e, (gname, K, lengths, ars, counts) in enumerate(cases):
        assert ev.gene_name(e) == gname and ev.K(e) == K and ev.N(e) <= 32
        assert [[ev.ars(m, e, j) for j in range(K)] for m in range(M)] == ars, gname     # G differs per read file
        if M > 1:
            assert ars[0] != ars[1]
    assert L.lib.lsq_events_host_genes(ev.h) == 0
    return ev, cases


def lean_group(cases, M):
    """the events of the lean group: at most two isoforms and four (method, class) pairs"""
    return [K <= 2 and M * ((1 << K) - 1) <= 4 for _, K, _, _, _ in cases]


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_general_set(tmp_path, M):
    """K = 1 .. 6 with M read files of different read lengths: the register-cached loop (K = 3, M = 1; K = 2, M = 2), the loop
    that reads memory (K = 2, M = 3; K = 3, M = 2; K = 4 .. 6; K = 6, M = 8: 504 pairs), K = 1; the lean group four lanes an
    event first, then one lane an event behind the placement learnt (M = 2, 3: its K = 1 events, four slots an event)"""
    ev, cases = general_events(tmp_path, M)
    tr = R.general_trajectories(M)
    cnt, bases = counts_array(ev, [c[4] for c in cases])
    small = lean_group(cases, M)
    n_lean, n_general = (sum(small) + 15) // 16 * 16, (len(cases) - sum(small) + 15) // 16 * 16
    assert n_general > 0 and (n_lean > 0) == (M <= 4)
    ctx = context(ev, {"em_flat_min_events": 0})
    ctx.set_counts(cnt, bases)
    ctx.solve()
    p = ctx.em_launch()
    assert p["lean_form"] == ("four_lane" if n_lean else "none") and p["lean_places"] == n_lean and p["general_places"] == n_general, p
    assert not p["learnt_placement"] and p["placement_learnt_after"] == bool(n_lean), p
    first = solution(ctx)
    got_cnt, got_bases = ctx.counts()
    assert np.array_equal(got_cnt, cnt) and np.array_equal(got_bases, bases)
    ctx.solve()
    p = ctx.em_launch()
    want_form = "none" if not n_lean else "four_lane_flat3" if M == 1 else "four_lane_flat4"
    assert p["lean_form"] == want_form and p["lean_places"] == n_lean and p["general_places"] == n_general and p["learnt_placement"] == bool(n_lean), p
    if M in (2, 3):
        assert p["split"] == 0, p           # K = 1 events take no iteration: all of them one lane an event
    second = solution(ctx)
    assert ctx.solve_finalize() == 0
    ctx.close()
    check_reference(ev, tr, first, "general set, %d read files" % M)
    same_bits(first, second, "general set, %d read files, second solve" % M)


def test_general_set_placements(tmp_path):
    """lsq_debug_set_em_order on the set with one read file: waves uniform in K, every wave of the general kernel mixing
    register-cached and uncached events, and holes -- an event's numbers do not depend on the events it shares a wave with"""
    import ctypes as C
    M = 1
    ev, cases = general_events(tmp_path, M)
    tr = R.general_trajectories(M)
    cnt, bases = counts_array(ev, [c[4] for c in cases])
    ctx = context(ev)
    dev2out = ctx.device_order()
    assert sorted(dev2out.tolist()) == list(range(len(cases)))
    K_of = {d: cases[o][1] for d, o in enumerate(dev2out.tolist())}
    by_K = {K: [d for d in sorted(K_of) if K_of[d] == K] for K in range(1, 7)}
    assert all(len(v) == 8 for v in by_K.values())
    HOLE = 0xFFFFFFFF

    def pad(v):
        return list(v) + [HOLE] * (-len(v) % 16)

    lean_ev = by_K[1] + by_K[2]
    uniform = (pad(lean_ev), sum((pad(by_K[K]) for K in (3, 4, 5, 6)), []))
    # every wave of the general kernel: two K = 3 events (register-cached) among six of K = 4 .. 6, in alternating places
    rest = [d for trio in zip(by_K[4], by_K[5], by_K[6]) for d in trio]
    mixed_waves = []
    for w in range(4):
        wave = rest[6 * w:6 * w + 3] + by_K[3][2 * w:2 * w + 1] + rest[6 * w + 3:6 * w + 6] + by_K[3][2 * w + 1:2 * w + 2]
        mixed_waves += pad(wave)
    mixed = (pad(lean_ev[::-1]), mixed_waves)
    rng = np.random.default_rng(11)
    holes_lean = rng.permutation(np.array(lean_ev + [HOLE] * 16, np.int64)).tolist()
    holes_gen = rng.permutation(np.array(sum((by_K[K] for K in (3, 4, 5, 6)), []) + [HOLE] * 32, np.int64)).tolist()
    holes = (holes_lean, holes_gen)
    ctx.set_counts(cnt, bases)
    ctx.solve()
    p = ctx.em_launch()
    assert p["lean_form"] == "four_lane" and p["lean_places"] == 16 and p["general_places"] == 32, p
    base = solution(ctx)
    check_reference(ev, tr, base, "general set, the library's own placement")
    L.lib.lsq_debug_set_em_order.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint]
    L.lib.lsq_debug_set_em_order.restype = C.c_int
    for what, (small, general) in (("uniform in K", uniform), ("mixed waves", mixed), ("holes", holes)):
        order = np.array(small + general, np.uint32)
        assert len(small) % 16 == 0 and len(order) % 16 == 0
        assert sorted(int(x) for x in order if x != HOLE) == list(range(len(cases)))
        assert L.lib.lsq_debug_set_em_order(ctx.h, order.ctypes.data, len(small), len(order)) == 0
        ctx.solve()
        p = ctx.em_launch()
        assert p["lean_form"] == "four_lane" and p["lean_places"] == len(small) and p["general_places"] == len(general) and not p["learnt_placement"], (what, p)
        sol = solution(ctx)
        check_reference(ev, tr, sol, "general set, placement: " + what)
        same_bits(base, sol, "placement: " + what)
    ctx.close()


def test_counts_from_outside_and_a_host_evaluated_gene(tmp_path):
    """a gene with seven isoforms is evaluated on the host, from its reads: lsq_solve on counts set from outside says so"""
    genes = [("H0_two", [300, 180]), ("H1_seven", [300, 200, 150, 400, 120, 333, 222])]
    ev = compile_events(tmp_path, "host", genes, (100,))
    assert [ev.K(e) for e in range(len(ev))] == [2, 7] and L.lib.lsq_events_host_genes(ev.h) >= 1
    ctx = context(ev)
    cnt, bases = counts_array(ev, [[[3, 4, 5]], [[1] * 127]])
    ctx.set_counts(cnt, bases)
    with pytest.raises(L.LsqError) as ei:
        ctx.solve()
    assert ei.value.status == -6, ei.value         # LSQ_E_UNSUPPORTED
    ctx.close()
