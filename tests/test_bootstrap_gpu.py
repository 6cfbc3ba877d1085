"""The read bootstrap on the device: a replicate's counts against the Python reference of tests/bootstrap_ref.py,
its EM against lsq_solve on those counts and against the 40-digit reference of tests/em_ref.py, the store, the chunks, the
summaries, what the call leaves alone, its errors and the executable's `#boot` lines.
Need an MI355X: python -m pytest tests -m gpu."""
import os

import numpy as np
import pytest

import lesseq_amd as L
import bootstrap_ref as B
import em_ref as R
from test_em_direct_gpu import compile_events, counts_array, context, solution, same_bits
from test_oracle_golden import load_case, runs

pytestmark = pytest.mark.gpu

SEED = 20250301
NB = 8
CAP = 200000                   # reads of an event of the case sets, by rescaling
T = L.lib.lsq_bootstrap_tile()
KEYS = ("mean", "sd", "q025", "q500", "q975")


def capped(row_lists):
    """counts[m][c] of one event with at most CAP reads in all: scaled down, a class with reads keeps at least one"""
    n = sum(int(x) for row in row_lists for x in row)
    if n <= CAP:
        return [[int(x) for x in row] for row in row_lists]
    k = sum(int(x) != 0 for row in row_lists for x in row)
    out = [[0 if int(x) == 0 else 1 + int(x) * (CAP - k) // n for x in row] for row in row_lists]
    assert sum(x for row in out for x in row) <= CAP
    return out


def reference_counts(ev, cnt, seed, b, only=None):
    off = ev.class_offsets()
    if only is None:
        return B.resample(off, cnt, seed, b)
    out = np.zeros_like(cnt)
    for e in only:
        a, z = int(off[e]), int(off[e + 1])
        for m in range(cnt.shape[0]):
            cls = B.draws(cnt[m, a:z], seed, m, e, b)
            if len(cls):
                out[m, a:z] = np.bincount(cls - 1, minlength=z - a).astype(np.uint64)
    return out


# the lean set (384 events, K = 2, one read file) and five events around the tile size, the last one deep
TILE_EVENTS = [("T0_below", (T - 1, 0, 0)), ("T1_tile", (T // 2, 0, T // 2)), ("T2_above", (1, T - 1, 1)), ("T3_three", (T, T, T + 1)), ("T4_deep", (400000, 1, 600002))]


@pytest.fixture(scope="module")
def lean(tmp_path_factory):
    d = tmp_path_factory.mktemp("boot_lean")
    cases = R.lean_cases()
    genes = R.lean_genes() + [(name, [300, 180]) for name, _ in TILE_EVENTS]
    ev = compile_events(d, "lean", genes, (R.LEAN_READ_LENGTH,))
    assert len(ev) == 384 + len(TILE_EVENTS) and [ev.gene_name(384 + i) for i in range(len(TILE_EVENTS))] == [n for n, _ in TILE_EVENTS]
    per_event = [capped([list(tr)]) for _, _, _, tr in cases] + [[list(tr)] for _, tr in TILE_EVENTS]
    assert [sum(p[0]) for p in per_event[384:]] == [T - 1, T, T + 1, 3 * T + 1, 1000003]
    assert CAP - 3 <= max(sum(p[0]) for p in per_event[:384]) <= CAP and any(sum(p[0]) == 0 for p in per_event)
    for p, (_, _, _, tr) in zip(per_event, cases):
        assert [x == 0 for x in p[0]] == [x == 0 for x in tr]               # the zeros stay
    cnt, bases = counts_array(ev, per_event)
    ctx = context(ev)
    ctx.set_counts(cnt, bases)
    ctx.solve()
    ars = [list(c[2]) for c in cases] + [[ev.ars(0, 384 + i, 0), ev.ars(0, 384 + i, 1)] for i in range(len(TILE_EVENTS))]
    yield dict(d=d, ev=ev, cnt=cnt, bases=bases, ctx=ctx, ars=ars)
    ctx.close()


@pytest.fixture(scope="module")
def general(tmp_path_factory):
    d = tmp_path_factory.mktemp("boot_general")
    cases = R.general_cases(2)
    ev = compile_events(d, "general2", R.general_genes(2), R.GENERAL_READ_LENGTHS[:2])
    assert len(ev) == 48 and max(ev.K(e) for e in range(48)) == 6
    per_event = [capped(c[4]) for c in cases]
    cnt, bases = counts_array(ev, per_event)
    ctx = context(ev)
    ctx.set_counts(cnt, bases)
    ctx.solve()
    yield dict(d=d, ev=ev, cnt=cnt, bases=bases, ctx=ctx)
    ctx.close()


@pytest.fixture(scope="module")
def lean_replicates(lean):
    """replicates 0 .. NB - 1 of the lean set, each on its own"""
    return [tuple(x.copy() for x in lean["ctx"].bootstrap_replicate(SEED, b)) for b in range(NB)]


@pytest.fixture(scope="module")
def general_replicates(general):
    return [tuple(x.copy() for x in general["ctx"].bootstrap_replicate(SEED, b)) for b in range(NB)]


# ------------------------------------------------------------------------------------------------------------- counts

@pytest.mark.parametrize("b", [0, 7])
def test_lean_counts_are_the_reference(lean, lean_replicates, b):
    """every event of the lean set, the events of T - 1, T, T + 1 and 3 T + 1 draws among them"""
    got = lean_replicates[b][0]
    want = reference_counts(lean["ev"], lean["cnt"], SEED, b, only=range(384 + 4))
    off = lean["ev"].class_offsets()
    z = int(off[384 + 4])
    bad = np.flatnonzero((got[:, :z] != want[:, :z]).any(axis=0))
    assert not len(bad), (b, bad[:10], got[0, bad[:10]], want[0, bad[:10]])


def test_every_replicate_keeps_the_totals(lean, lean_replicates, general, general_replicates):
    for S, reps in ((lean, lean_replicates), (general, general_replicates)):
        off = np.array(S["ev"].class_offsets(), np.int64)
        total = np.add.reduceat(S["cnt"], off[:-1], axis=1)
        for b, rep in enumerate(reps):
            assert np.array_equal(np.add.reduceat(rep[0], off[:-1], axis=1), total), b
            assert not rep[0][S["cnt"] == 0].any()
        assert not np.array_equal(reps[0][0], reps[1][0])


def test_deep_event_spreads_over_many_tiles(lean, lean_replicates):
    """1 000 003 draws of one event (245 tiles), replicates 0 and 1"""
    e = 384 + 4
    off = lean["ev"].class_offsets()
    a, z = int(off[e]), int(off[e + 1])
    for b in (0, 1):
        want = reference_counts(lean["ev"], lean["cnt"], SEED, b, only=[e])
        assert np.array_equal(lean_replicates[b][0][:, a:z], want[:, a:z]), (b, lean_replicates[b][0][:, a:z], want[:, a:z])


@pytest.mark.parametrize("b", [0, 7])
def test_general_counts_are_the_reference(general, general_replicates, b):
    """K up to 6 (63 classes), two read files"""
    want = reference_counts(general["ev"], general["cnt"], SEED, b)
    assert np.array_equal(general_replicates[b][0], want)


def test_host_call_agrees_with_the_device(general, general_replicates):
    got = L.bootstrap_resample_host(general["ev"].class_offsets(), general["cnt"], SEED, 3)
    assert np.array_equal(got, general_replicates[3][0])


# -------------------------------------------------------------------------------------------------------------- solve

@pytest.mark.parametrize("which", ["lean", "general"])
def test_replicates_solve_as_lsq_solve_does(which, lean, lean_replicates, general, general_replicates):
    """replicate b's (theta, ll, iters, flags) are those of a second context given its counts and solved with em_regroup = 0"""
    S, reps = (lean, lean_replicates) if which == "lean" else (general, general_replicates)
    other = context(S["ev"], {"em_regroup": 0})
    for b, rep in enumerate(reps):
        other.set_counts(rep[0], S["bases"])
        other.solve()
        p = other.em_launch()
        assert p["lean_form"] == "four_lane" and p["general_places"] > 0 and not p["learnt_placement"], p
        same_bits(solution(other), rep[1:], "%s set, replicate %d" % (which, b))
    other.close()


@pytest.mark.parametrize("b", [0, 7])
def test_lean_replicates_against_the_40_digit_reference(lean, lean_replicates, b):
    """em_ref.accept on the replicate's own counts, no new tolerance; events whose loop ends on a log-likelihood of exactly 0
    are held to the reference's iteration exactly, by the same rule"""
    ev, off = lean["ev"], lean["ev"].class_offsets()
    cnt, theta, ll, iters, flags = lean_replicates[b]
    bad, n_rounding = [], 0
    for e in range(len(ev)):
        row = [int(x) for x in cnt[0, int(off[e]):int(off[e + 1])]]
        Tr = R.em_trajectory(2, [lean["ars"][e]], [row])
        n_rounding += Tr.rounding_stop
        why = R.accept(Tr, theta[2 * e:2 * e + 2], ll[e], iters[e], flags[e])
        if why:
            bad.append("%s %r: %s" % (ev.gene_name(e), row, why))
    print("replicate %d: %d events, %d flagged, %d stops decided by rounding, %d refused" % (b, len(ev), int((flags & 1).sum()), n_rounding, len(bad)))
    assert not bad, "\n  ".join(bad[:12])


# ---------------------------------------------------------------------------------------------------- store and chunks

@pytest.fixture(scope="module")
def lean_boot(lean):
    ctx = lean["ctx"]
    s = {k: v.copy() for k, v in ctx.bootstrap(NB, SEED).items()}
    return s, ctx.bootstrap_theta().copy()


def same_summaries(a, b, what):
    for k in ("n_ok",) + KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def test_store_rows_are_the_replicates(lean_boot, lean_replicates):
    _, store = lean_boot
    assert store.shape == (NB, 2 * (384 + len(TILE_EVENTS)))
    for b in range(NB):
        assert np.array_equal(store[b], lean_replicates[b][1], equal_nan=True), b


@pytest.mark.parametrize("which", ["lean", "general"])
def test_chunks_never_change_a_result(which, lean, general):
    S = lean if which == "lean" else general
    got = []
    for chunk in (1, 3, 0):
        ctx = context(S["ev"], {"bootstrap_chunk": chunk})
        ctx.set_counts(S["cnt"], S["bases"])
        ctx.solve()
        got.append(({k: v.copy() for k, v in ctx.bootstrap(NB, SEED).items()}, ctx.bootstrap_theta().copy()))
        ctx.close()
    for s, store in got[1:]:
        assert np.array_equal(store, got[0][1], equal_nan=True)
        same_summaries(s, got[0][0], which)


# ---------------------------------------------------------------------------------------------------------- summaries

def check_summaries(s, store):
    finite = np.isfinite(store)
    eps = 2.0 ** -52
    for i in range(store.shape[1]):
        v = store[finite[:, i], i]
        assert s["n_ok"][i] == len(v), i
        if not len(v):
            assert all(np.isnan(s[k][i]) for k in KEYS), i
            continue
        for k, p in (("q025", 0.025), ("q500", 0.5), ("q975", 0.975)):
            want = np.quantile(v, p)
            assert abs(s[k][i] - want) <= 4 * eps * abs(want), (i, k, s[k][i], want)           # 4 ulp: one interpolation
        bound = 4096 * 2.0 ** -53
        assert abs(s["mean"][i] - v.mean()) <= bound, (i, s["mean"][i], v.mean())
        if len(v) < 2:
            assert np.isnan(s["sd"][i]), i
        else:
            want = v.std(ddof=1)
            assert abs(s["sd"][i] - want) <= bound + 1e-9 * want, (i, s["sd"][i], want)


def test_summaries_are_numpys_on_the_store(lean_boot):
    s, store = lean_boot
    assert np.isfinite(store).all()
    check_summaries(s, store)
    assert (s["sd"] > 0).any() and (s["q025"] <= s["q500"]).all() and (s["q500"] <= s["q975"]).all()


def test_an_event_without_reads(lean, lean_boot):
    """what the EM gives for empty counts, in every replicate identically: theta 1/K"""
    s, store = lean_boot
    off = np.array(lean["ev"].class_offsets(), np.int64)
    empty = np.flatnonzero(np.add.reduceat(lean["cnt"], off[:-1], axis=1)[0] == 0)
    assert len(empty) >= 6
    point = lean["ctx"].solution()[0]
    for e in empty:
        for i in (2 * e, 2 * e + 1):
            assert (store[:, i] == point[i]).all() and point[i] == 0.5
            assert s["n_ok"][i] == NB and s["mean"][i] == 0.5 and s["sd"][i] == 0 and s["q025"][i] == s["q500"][i] == s["q975"][i] == 0.5


def test_summaries_of_the_general_set_and_one_replicate(general):
    ctx = general["ctx"]
    s = ctx.bootstrap(NB, SEED)
    check_summaries(s, ctx.bootstrap_theta())
    s = {k: v.copy() for k, v in ctx.bootstrap(1, SEED).items()}
    store = ctx.bootstrap_theta()
    assert store.shape[0] == 1 and (s["n_ok"] == 1).all() and np.isnan(s["sd"]).all()
    for k in ("mean", "q025", "q500", "q975"):
        assert np.array_equal(s[k], store[0]), k
    assert np.array_equal(store[0], ctx.bootstrap_replicate(SEED, 0)[1])


def test_many_replicates(general):
    """B = 4096: the whole LDS sort, in five chunks"""
    ctx = context(general["ev"], {"bootstrap_chunk": 1000})
    small = np.minimum(general["cnt"], np.uint64(50))
    ctx.set_counts(small, small)
    ctx.solve()
    s = ctx.bootstrap(4096, 1)
    check_summaries(s, ctx.bootstrap_theta())
    ctx.close()


# ---------------------------------------------------------------------------------------------------------- isolation

def test_bootstrap_leaves_the_point_estimate_alone(general):
    ctx = context(general["ev"])
    ctx.set_counts(general["cnt"], general["bases"])
    ctx.solve()
    before = (solution(ctx), tuple(x.copy() for x in ctx.counts()), ctx.em_launch())
    ctx.bootstrap(NB, SEED)
    ctx.bootstrap_replicate(SEED, 5)
    after = (solution(ctx), tuple(x.copy() for x in ctx.counts()), ctx.em_launch())
    same_bits(before[0], after[0], "solution() after bootstrap()")
    assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
    assert before[2] == after[2]
    ctx.solve()
    same_bits(before[0], solution(ctx), "solve() after bootstrap()")
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- errors

def test_errors(general):
    ctx = context(general["ev"])
    for call in (lambda: ctx.bootstrap(NB, 0), lambda: ctx.bootstrap_replicate(0, 0)):
        with pytest.raises(L.LsqError) as ei:
            call()
        assert ei.value.status == -8                # before any count
    ctx.set_counts(general["cnt"], general["bases"])
    with pytest.raises(L.LsqError) as ei:
        ctx.bootstrap(NB, 0)
    assert ei.value.status == -8                    # counts, no solve
    with pytest.raises(L.LsqError) as ei:
        ctx.bootstrap_theta()
    assert ei.value.status == -8
    ctx.solve()
    for n in (0, 4097):
        with pytest.raises(L.LsqError) as ei:
            ctx.bootstrap(n, 0)
        assert ei.value.status == -1
    with pytest.raises(L.LsqError) as ei:
        ctx.set_option("bootstrap_chunk", 4097)
    assert ei.value.status == -1
    ctx.bootstrap(2, 0)
    ctx.close()


def test_a_host_evaluated_gene_has_no_replicates(tmp_path):
    """a gene of seven isoforms is evaluated on the host: n_ok 0 and no number for its rows, the others as without it"""
    genes = [("H0_two", [300, 180]), ("H1_seven", [300, 200, 150, 400, 120, 333, 222]), ("H2_three", [260, 410, 333])]
    lines = ["AlignmentBlocks\n"]
    rng = np.random.default_rng(5)
    for g, (_, lengths) in enumerate(genes):
        for j, length in enumerate(lengths):
            start = 1000 + (g * 8 + j) * 2000
            for _ in range(20 + 7 * j):
                s = start + int(rng.integers(1, length - 100 + 1))
                lines.append("chr1:+:%d:%d:1:100\n" % (s + 1, s + 100))
    mrf = tmp_path / "host.mrf"
    mrf.write_text("".join(lines))
    ev = compile_events(tmp_path, "host", genes, (100,))
    assert [ev.K(e) for e in range(3)] == [2, 7, 3] and L.lib.lsq_events_host_genes(ev.h) == 1
    ctx = context(ev)
    ctx.upload_reads_mrf(0, str(mrf))
    ctx.count(); ctx.solve()
    cnt, bases = [x.copy() for x in ctx.counts()]
    assert cnt[0, :3].sum() > 0 and cnt[0, 130:].sum() > 0
    s = {k: v.copy() for k, v in ctx.bootstrap(NB, SEED).items()}
    store = ctx.bootstrap_theta().copy()
    rep = ctx.bootstrap_replicate(SEED, 2)
    ctx.close()
    host = slice(2, 9)
    assert (s["n_ok"][host] == 0).all() and all(np.isnan(s[k][host]).all() for k in KEYS) and np.isnan(store[:, host]).all()
    assert np.isnan(rep[1][host]).all() and not rep[0][0, 3:3 + 127].any()
    # the two other events: what a context without the gene gives for their counts, event numbers and all
    off = ev.class_offsets()
    want = reference_counts(ev, cnt, SEED, 2, only=[0, 2])
    assert np.array_equal(rep[0][0, :3], want[0, :3]) and np.array_equal(rep[0][0, int(off[2]):], want[0, int(off[2]):])
    dev = np.r_[0:2, 9:12]
    assert (s["n_ok"][dev] == NB).all() and np.isfinite(store[:, dev]).all()
    check_summaries({k: v[dev] for k, v in s.items()}, store[:, dev])


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_boot(lines):
    rows = []
    for line in lines:
        t = line.split("\t")
        assert t[0] == "#boot" and len(t) == 9, line
        rows.append((t[1], t[2], int(t[3])) + tuple(float("nan") if x == "NA" else float(x) for x in t[4:]))
    return rows


def test_solve_bootstrap_lines(tmp_path, monkeypatch):
    c, d = load_case("toy", tmp_path)
    monkeypatch.chdir(d)
    r = [x for t, x in runs(c) if t == "solve" and x["exit"] == 0][0]
    golden = open(os.path.join(d, r["stdout"])).read()
    rc, text = L.cli_run("solve", r["argv"] + ["--bootstrap", "8", "--seed", "3"])
    assert rc == 0 and text.startswith(golden)                 # the table, byte for byte
    rows = parse_boot(text[len(golden):].split("\n")[:-1])
    # the same inputs through the binding
    a = r["argv"]
    ev = L.Events(L.Annotation(a[4], a[6], int(a[7]), int(a[8])), (a[10],), (int(a[11]),))
    ctx = context(ev)
    ctx.upload_reads_mrf(0, a[12])
    ctx.count(); ctx.solve()
    s = ctx.bootstrap(8, 3)
    ctx.close()
    assert len(rows) == ev.total_isoforms == len(golden.split("\n")) - 1
    i = 0
    for e in range(len(ev)):
        for j in range(ev.K(e)):
            assert rows[i][0] == ev.gene_name(e) and rows[i][1] == golden.split("\n")[i].split("\t")[2]
            assert rows[i][2] == s["n_ok"][i] == 8
            for q, k in enumerate(KEYS):
                assert R.same_number(rows[i][3 + q], float(s[k][i])), (rows[i], k, s[k][i])
            i += 1
    assert any(row[4] > 0 for row in rows)                      # some spread at this depth
    # seed 0 unless given; --fim goes first
    rc0, text0 = L.cli_run("solve", a + ["--bootstrap", "8"])
    rc1, text1 = L.cli_run("solve", a + ["--bootstrap", "8", "--seed", "0"])
    assert rc0 == rc1 == 0 and text0 == text1 and text0 != text
    rc, both = L.cli_run("solve", a + ["--fim", "--bootstrap", "8"])
    rc2, fim = L.cli_run("solve", a + ["--fim"])
    assert rc == rc2 == 0 and fim.startswith(golden) and both == fim + text0[len(golden):]
    kinds = [line.split("\t")[0] for line in both[len(golden):].split("\n")[:-1]]
    assert kinds == ["#fim"] * kinds.count("#fim") + ["#boot"] * len(rows) and kinds.count("#fim") == len(ev)
    for bad in (["--bootstrap", "x"], ["--bootstrap", "0"], ["--bootstrap", "4097"], ["--bootstrap"], ["--bootstrap", "8", "--seed", "y"],
                ["--bootstrap", "8", "--seed"], ["--bootstrap", "8", "--fim"]):
        rc, out = L.cli_run("solve", a + bad)
        assert rc == 1 and out == "", bad
