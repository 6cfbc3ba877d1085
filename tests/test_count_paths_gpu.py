"""The count kernel's three streaming loops, verdict by verdict (csrc/lsq_count.hip: stream_pool_wide, stream_pool1_compact,
stream_pool2_compact).

A read is settled by a verdict of a streaming loop, by the general walk over parked reads, by the exception pass or by the
recount; the last three are complete counters on their own, so a test of their sum cannot see which verdicts its input reaches
nor whether a loop parks what it is said to settle.  Here the developer library (liblesseq_hip_dev.so) runs in child processes
of its own (count_paths_child.py) with its path counters on (LSQ_ABLATE 256: lsq_debug_counters) and, in a second count, with
the parked reads dropped instead of walked (288: the loops alone), on files whose reads a plain model of cells and verdicts
(count_cells_ref.py) picks: one file per verdict and kernel.  All figures are exact integers, held against the oracle, the
release library (this process) and the model's parked counts.

What the model found while the files were made (kept as the files' expectations):
  * a two-block record is S or dropped from a start cell only as a lane's FIRST record; behind a first record that crosses no
    junction it is parked -- the records' order inside a group of the pool is not defined (an atomic cursor places them), so
    such files hold the parked count of the layout: per group its records behind the lane leaders (park_bounds);
  * an EMPTY cell cannot hold the first base of a loaded read in a job without shards: the loader keeps a read only when every
    block lies inside a covered region, the union of the exons of the job's events, which is the union of their segments.
    `nobody` and `drop` are reached through start cells here;
  * the loader merges a read's blocks in file order (interval_list::add_interval): touching blocks listed in ascending order
    become ONE block.  The "touching blocks" of the threshold test are listed so, and none of them reaches the exception list
    (its files show 0 entries here); the files of this module list touching blocks second block first, which keeps them apart."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lesseq_amd as L
import oracle_binding as ob
import count_cells_ref as cr
import count_paths_inputs as ci

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "lesseq_amd", "_build", "liblesseq_hip_dev.so")
CHILD = os.path.join(ROOT, "tests", "count_paths_child.py")
CHILD_TIMEOUT = 120
OPTIONS = {"wide": {"compact_pools": 0}, "compact4": {"reads_per_look": 4}, "compact8": {"reads_per_look": 8}}
FULL, ALONE = 256, 288          # LSQ_ABLATE: counters; counters + parked reads dropped
ZERO = ("S_weak", "drop", "nothing", "nobody", "gone")
SETTLED = ("A", "L", "J", "Jb", "same", "far_only")
REASONS = ("park1_no_cell", "park1_one_owner", "park1_two_owner", "park2_no_owner", "park2_one_owner", "park2_follower_plain", "park2_follower_past")
REASON_NAME = {5: "park1_no_cell", 6: "park1_one_owner", 7: "park1_two_owner", 8: "park2_no_owner", 9: "park2_one_owner",
               13: "park2_follower_plain", 14: "park2_follower_past"}
# three events that overlap in span-start order; the bases [3101, 3200) lie in a segment of each
XYZ = [("X", "+", [[(3000, 3200), (3400, 3450)], [(3000, 3200)]]), ("Y", "+", [[(3050, 3250), (3500, 3550)], [(3050, 3250)]]),
       ("Z", "-", [[(3100, 3300), (3600, 3650)], [(3100, 3300)]])]


class File:
    def __init__(self, name, ann, reads, R=100, grids=(None,), verdict=None, mrf=None, forward=False, strands=None):
        self.name, self.ann, self.reads, self.R, self.grids, self.verdict, self.mrf = name, ann, reads, R, list(grids), verdict, mrf
        self.strands = strands
        self.forward = forward          # touching blocks listed in ascending order (the loader merges them), as the threshold test does


class World:
    """the annotations, their models, and per kernel the files and what came of them"""

    def __init__(self, d):
        self.d = str(d)
        self.ann = {}
        for stem, genes in (("abc", ci.ABC), ("g5", ci.ABC + ci.DE), ("xyz", XYZ)):
            iv, mp = ci.write_annotation(self.d, stem, genes)
            ev = L.Events(L.Annotation(iv, mp), ("SHORT_READ",), (100,))
            (b, M, idx), = ci.models_of(ev)
            self.ann[stem] = dict(interval=iv, map=mp, M=M, cov=ev.covered(ci.CHROM))
        spec = L.SynthSpec(seed=23, n_events=40, n_reads=6000, read_length=100, n_chrom=1)
        L.synth_write(spec, self.d, "syn", write_mrf=True)
        # (one- and two-block reads only: pool n stays empty)
        with open(os.path.join(self.d, "syn.mrf")) as f:
            lines = f.read().split("\n")
        self.syn_mrf = os.path.join(self.d, "syn12.mrf")
        with open(self.syn_mrf, "w") as f:
            f.write("\n".join(ln for ln in lines if ln.count(",") <= 1))
        self.ann["syn"] = dict(interval=os.path.join(self.d, "syn.interval"), map=os.path.join(self.d, "syn.map"), M=None, cov=None)
        g5 = self.ann["g5"]
        self.cases = ci.case_files(g5["M"], g5["cov"])
        self.runs = {}
        self.failed = None

    def files(self, kernel):
        thr = ci.threshold_reads()
        st = [x for _, x in ci.threshold_reads(with_strands=True)]
        out = [File("thr40", "abc", thr, R=40, forward=True, strands=st), File("thr100", "abc", thr, forward=True, strands=st), File("seeded", "syn", None, mrf=self.syn_mrf)]
        for v in ci.verdict_names(kernel):
            out.append(File("case_" + v, "g5", self.cases.get((v, kernel), []), verdict=v))
        # span-start ties (a two-block read from an event's first base to its last) and touching blocks in a one-owner cell under
        # one span only: each a pair for the exception pass
        ties = [(1000, 1100, 1400, 1500), (2000, 2100, 2600, 2700), (1450, 1520, 2050, 2130), (1470, 1490, 2160, 2200), (1040, 1180, 1225, 1250)]
        touch = [(a, y, y, w) for a in range(2301, 2340, 2) for y in (a + 1, a + 9, 2350) for w in (y + 1, y + 5, 2360) if a < y < w <= 2360]
        out.append(File("exceptions", "g5", ties * 8 + touch))
        n1 = cr.PER_LOOK[kernel][0]
        park = [(a, b) for b in range(1501, 1601) for a in range(1401, 1450)][:4000]
        out.append(File("ring", "g5", park, grids=(1, 3)))
        out.append(File("multilook", "xyz", [(a, a + ln) for a in range(3100, 3200) for ln in (1, 40, 100) if a + ln <= 3300], grids=(1, 3)))
        for n in (1, 64 * n1 - 1, 64 * n1, 64 * n1 + 1, 4 * 64 * n1 - 1, 4 * 64 * n1 + 1):
            rds = [(1401 + (q // 2) % 49, 1500 - (q // 98) % 40) if q % 2 == 0 else (1401 + (q // 2) % 49, 1501 + (q // 98) % 90) for q in range(n)]
            out.append(File("edge_%d" % n, "g5", rds, grids=(1, 3)))
        return out

    def run(self, kernel):
        """one child for the kernel's files; the release library's tables here; the oracle's"""
        if kernel in self.runs:
            return self.runs[kernel]
        if self.failed:
            # (a child that ended abnormally may have faulted the device: nothing more is started on it from here)
            pytest.fail("the child of %s ended abnormally in an earlier test; no further child is started" % self.failed)
        files = self.files(kernel)
        man = {"options": OPTIONS[kernel], "files": []}
        for f in files:
            a = self.ann[f.ann]
            if f.mrf is None:
                f.mrf = os.path.join(self.d, "%s_%s.mrf" % (kernel, f.name))
                with open(f.mrf, "w") as h:
                    h.write(ci.mrf_text(f.reads, f.forward, f.strands))
            man["files"].append({"name": f.name, "interval": a["interval"], "map": a["map"], "mrf": f.mrf, "R": f.R, "grids": f.grids, "modes": [FULL, ALONE]})
        mp, op = os.path.join(self.d, kernel + "_manifest.json"), os.path.join(self.d, kernel + "_out.json")
        with open(mp, "w") as h:
            json.dump(man, h)
        env = dict(os.environ, LSQ_LIB=DEV_LIB, LSQ_NO_TORCH="1")
        env.pop("LSQ_OPTIONS", None)
        try:
            p = subprocess.run([sys.executable, CHILD, mp, op], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            self.failed = kernel
            pytest.fail("the child of %s ran past %d s: %s" % (kernel, CHILD_TIMEOUT, (e.stderr or b"")[-2000:]))
        if p.returncode != 0:
            self.failed = kernel
            pytest.fail("the child of %s ended with status %d: %s" % (kernel, p.returncode, p.stderr[-2000:]))
        with open(op) as h:
            dev = json.load(h)
        out = {}
        for f in files:
            a = self.ann[f.ann]
            ev = L.Events(L.Annotation(a["interval"], a["map"]), ("SHORT_READ",), (f.R,))
            ctx = L.Context(0)
            for k, v in OPTIONS[kernel].items():
                ctx.set_option(k, v)
            ctx.upload_events(ev)
            ctx.upload_reads(0, L.Reads.from_mrf(f.mrf, ev))
            ctx.count()
            cnt, bases = ctx.counts()
            rel = dict(cnt=cnt[0].copy(), bases=bases[0].copy(), recounted=ctx.count_status()[1][0])
            ctx.close()
            argv = ["0", "t", "./", "LH_GENE_TXT", a["interval"], "UCSC_GENE2ISOFORM", a["map"], "0", "100000", "MRF_SINGLE", "SHORT_READ", str(f.R), f.mrf]
            rc, _, exact = ob.run("count", argv)
            assert rc == 0
            oracle = np.array([x for g in exact for x in [g["supports"][0], g["bases"][0]] + g["iso_count"]], np.int64)
            out[f.name] = dict(file=f, dev=dev[f.name], rel=rel, oracle=oracle, ev=ev, genes=[g["gname"] for g in exact])
        self.runs[kernel] = out
        return out


def table(ev, cnt, bases):
    """per gene: support, matched bases, reads per isoform -- the rows the oracle gives"""
    cnt, bases = np.asarray(cnt, np.int64), np.asarray(bases, np.int64)
    off = ev.class_offsets()
    out = []
    for i in range(len(ev)):
        K = ev.K(i)
        cl = cnt[off[i]:off[i + 1]]
        out += [int(cl.sum()), int(bases[off[i]:off[i + 1]].sum())] + [int(sum(cl[c - 1] for c in range(1, 1 << K) if c >> j & 1)) for j in range(K)]
    return np.array(out, np.int64)


def rows_of(ev, genes):
    """the positions of the genes' rows in a table()"""
    pos, out = 0, []
    for i in range(len(ev)):
        n = 2 + ev.K(i)
        if ev.gene_name(i) in genes:
            out += list(range(pos, pos + n))
        pos += n
    return out


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    if not os.path.exists(DEV_LIB):
        pytest.fail("%s is missing: `make -C lesseq_amd/csrc` builds it beside the library" % DEV_LIB)
    return World(tmp_path_factory.mktemp("paths"))


def invariants(kernel, name, r, report=None):
    """I1 .. I4 on one file; returns per grid the (full, alone) results"""
    f, ev, oracle = r["file"], r["ev"], r["oracle"]
    assert r["rel"]["recounted"] == 0, (kernel, name)
    out = []
    for grid in f.grids:
        full, alone = r["dev"]["%s/%d" % (grid, FULL)], r["dev"]["%s/%d" % (grid, ALONE)]
        what = (kernel, name, grid)
        for x in (full, alone):
            # the kernel that was asked for ran, on one- and two-block records only, and the recount stayed out of it
            assert x["compact"] == (kernel != "wide") and x["reads_per_look"] == cr.PER_LOOK[kernel][0], what
            assert x["pool"][2] == 0 and x["recounted"] == 0, what
        d, da = full["dbg"], alone["dbg"]
        tf, ta = table(ev, full["cnt"], full["bases"]), table(ev, alone["cnt"], alone["bases"])
        print("%s %s grid %s: reads %d, parked1 %d, parked2 %d, %s, walk lanes %d, exceptions %d" % (
            kernel, name, grid, sum(full["pool"]), d["parked1"], d["parked2"], {k: d[k] for k in REASONS if d[k]}, d["walk_lanes"], d["exceptions"]))
        # I1
        assert np.array_equal(np.asarray(full["cnt"], np.uint64), r["rel"]["cnt"]) and np.array_equal(np.asarray(full["bases"], np.uint64), r["rel"]["bases"]), what
        assert np.array_equal(tf, oracle), what
        # I2
        assert (ta <= oracle).all(), what
        assert alone["exceptions"] == 0 and da["walk_steps"] == 0 and da["walk_lanes"] == 0, what
        # I3
        if da["parked1"] + da["parked2"] == 0:
            assert np.array_equal(ta, oracle), what
        # I4 (what is parked does not depend on what becomes of it)
        for x in (d, da):
            assert x["parked1"] == x["park1_no_cell"] + x["park1_one_owner"] + x["park1_two_owner"], what
            two = x["park2_no_owner"] + x["park2_one_owner"] + x["park2_follower_plain"] + x["park2_follower_past"]
            assert x["parked2"] == two if kernel != "wide" else x["parked2"] >= two, what
        assert all(d[k] == da[k] for k in ("parked1", "parked2") + REASONS), what
        assert d["walk_lanes"] >= d["parked1"] + d["parked2"], what
        out.append((full, alone, tf, ta))
    return out


def model_counts(world, kernel, r, full):
    """the parked counts the model gives for the file's loaded reads, held against the counters"""
    f = r["file"]
    a = world.ann[f.ann]
    reads = [rd for rd in (ci.loaded(a["cov"], rd, f.forward) for rd in f.reads) if rd is not None]
    assert full["pool"][0] == sum(1 for rd in reads if len(rd) == 2) and full["pool"][1] == sum(1 for rd in reads if len(rd) == 4), (kernel, f.name, "reads loaded")
    b = cr.park_bounds(a["M"], reads, kernel)
    d = full["dbg"]
    assert d["parked1"] == b["parked1"], (kernel, f.name, d, b)
    assert {k: d[REASON_NAME[k]] for k in (5, 6, 7)} == b["reasons1"], (kernel, f.name, d, b)
    assert b["parked2"][0] <= d["parked2"] <= b["parked2"][1], (kernel, f.name, d, b)
    if b["reasons2"] is not None and kernel != "wide":
        assert {k: d[REASON_NAME[k]] for k in (8, 9, 13, 14)} == b["reasons2"], (kernel, f.name, d, b)
    return reads, b


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_invariants_on_the_threshold_file_and_a_seeded_file(world, kernel):
    """I1 .. I4 on the reads of test_reads_on_every_threshold_of_the_streaming_loops_vs_oracle (R 40 and 100) and on a seeded
    synthetic file; on the threshold files the model's parked counts too.  Prints the share of the reads each kernel settled in
    its loops and the parked counts by reason."""
    run = world.run(kernel)
    for name in ("thr40", "thr100", "seeded"):
        (full, alone, tf, ta), = invariants(kernel, name, run[name])
        n = sum(full["pool"])
        assert n > 3000
        print("%s %s: %.4f of %d reads settled in the loops" % (kernel, name, 1.0 - (full["dbg"]["parked1"] + full["dbg"]["parked2"]) / n, n))
        if name != "seeded":
            model_counts(world, kernel, run[name], full)


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_the_case_files_are_complete(world, kernel):
    """every verdict of the model has a case file for every kernel that has the verdict, of at least 300 reads that lie on at
    least three boundary positions, each read with that verdict; across them every reason counter is reached"""
    M = world.ann["g5"]["M"]
    names = ci.verdict_names(kernel)
    assert set(ci.required_tags(kernel)) == set(names)
    assert set(names) == {v for v in cr.VERDICTS1 + cr.VERDICTS2 if v != "by_place" and (kernel != "wide" or v not in cr.COMPACT_ONLY)}
    for v in names:
        reads = world.cases.get((v, kernel), [])
        assert len(reads) >= 300, (kernel, v, len(reads), "no reads reach this verdict: a promised verdict without a case file")
        # on, one before, one behind the threshold that governs the verdict (the side that is another verdict's lies in that
        # verdict's file), and the 98 % rule on and beside equality: required_tags says which, tags() finds them
        have = {}
        for rd in reads:
            for name, off in ci.tags(M, rd):
                have.setdefault(name, set()).add(off)
        for name, offs in ci.required_tags(kernel)[v].items():
            assert offs <= have.get(name, set()), (kernel, v, name, "wanted", sorted(offs), "held", sorted(have.get(name, set())))
        for rd in reads:
            got = cr.verdict1(M, rd, kernel)[0] if len(rd) == 2 else cr.verdict2(M, rd, kernel, "lead")[0]
            assert got == ("J" if v == "same" else v), (kernel, v, rd, got)
    run = world.run(kernel)
    seen = {k: 0 for k in REASONS}
    for v in names:
        for k in REASONS:
            seen[k] += run["case_" + v]["dev"]["None/%d" % FULL]["dbg"][k]
    want = REASONS if kernel != "wide" else REASONS[:5]          # (the wide loop has no counters for its second records)
    assert all(seen[k] > 0 for k in want), (kernel, seen)


def case_params():
    return [(k, v) for k in cr.KERNELS for v in ci.verdict_names(k)]


@pytest.mark.parametrize("kernel,verdict", case_params())
def test_one_verdict_of_one_kernel(world, kernel, verdict):
    """the file of one verdict through one kernel: the invariants, the model's parked counts, and what the verdict says of the
    loops-alone table"""
    r = world.run(kernel)["case_" + verdict]
    (full, alone, tf, ta), = invariants(kernel, "case_" + verdict, r)
    reads, b = model_counts(world, kernel, r, full)
    d, n, oracle = full["dbg"], len(reads), r["oracle"]
    parked = d["parked1"] + d["parked2"]
    if verdict in SETTLED:
        assert parked == 0 and np.array_equal(ta, oracle) and oracle.sum() > 0
    elif verdict in ZERO and b["by_place"] == 0:
        assert parked == 0 and not ta.any() and not oracle.any()
    elif verdict in ZERO:
        # (drop from a start cell: a lane's later records are parked; whoever settles them, they count for nobody)
        assert not ta.any() and not oracle.any() and parked == b["parked2"][0] == b["parked2"][1]
    elif verdict in ("park_past", "park_nocell", "park"):
        assert parked == n and not ta.any()
        if verdict != "park" and verdict != "park_nocell":
            assert oracle.sum() > 0
    elif verdict == "split":
        M = world.ann["g5"]["M"]
        far = {M.events[M.cell(rd[0])["far"][0]].name for rd in reads}
        near = {M.events[M.cell(rd[0])["near"][0]].name for rd in reads}
        assert not far & near
        rows = rows_of(r["ev"], far)
        assert d["park1_two_owner"] == n == parked
        assert np.array_equal(ta[rows], oracle[rows]) and ta[rows][0] > 0 and ta.sum() == ta[rows].sum()
    elif verdict == "S_add":
        # settled as a lane's first record, parked behind one: the layout's count of each; every settled read counts once
        assert parked == b["parked2"][0] == b["parked2"][1]
        pos, total = 0, 0
        for i in range(len(r["ev"])):
            total += int(ta[pos])
            pos += 2 + r["ev"].K(i)
        assert total == n - parked == b["looks"], (total, n, parked, b)
    else:
        raise AssertionError("no expectation for " + verdict)


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_touching_blocks_and_span_start_ties_reach_the_exception_list(world, kernel):
    """... parked, looked at by the walk, and handed on: as many entries as there are (read, event) pairs with the read's first
    base inside the event's span and either touching blocks or a read from the span's first base to its last"""
    r = world.run(kernel)["exceptions"]
    (full, alone, tf, ta), = invariants(kernel, "exceptions", r)
    reads, b = model_counts(world, kernel, r, full)
    M = world.ann["g5"]["M"]
    pairs = 0
    for a, y, z, w in reads:
        over = [e for e in M.events if e.gs <= a <= e.ge]
        tie = [e for e in over if a == e.gs and w == e.ge]
        if z == y:
            assert len(over) == 1 and not tie
            pairs += 1
        else:
            assert len(tie) == 1
            pairs += 1
    assert full["dbg"]["parked2"] == len(reads) and full["exceptions"] == pairs == full["dbg"]["exceptions"]
    assert not ta.any()


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_the_ring_wraps_and_parked_reads_take_several_looks(world, kernel):
    """about 4 000 parked reads of one bucket through one and three workgroups: every wave's ring passes its capacity (256
    entries) several times; each read carries its one event: as many walk lanes as reads.  And reads in a stretch that three
    overlapping events own: parked without an event, three looks each."""
    run = world.run(kernel)
    for full, alone, tf, ta in invariants(kernel, "ring", run["ring"]):
        reads, b = model_counts(world, kernel, run["ring"], full)
        d = full["dbg"]
        assert len(reads) == 4000 == d["parked1"] == d["park1_one_owner"] == d["walk_lanes"] and not ta.any() and tf.sum() > 0
    M = world.ann["xyz"]["M"]
    for full, alone, tf, ta in invariants(kernel, "multilook", run["multilook"]):
        reads, b = model_counts(world, kernel, run["multilook"], full)
        d = full["dbg"]
        looks = sum(cr.looks_of_walk(M, rd[0]) for rd in reads)
        assert len(reads) >= 280 and looks == 3 * len(reads)
        assert d["parked1"] == d["park1_no_cell"] == len(reads) and d["walk_lanes"] == looks and tf.sum() > 0


@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_the_edges_of_a_workgroups_range(world, kernel):
    """1, 64 NR - 1, 64 NR, 64 NR + 1 and 4 x 64 NR -+ 1 reads (NR: what a lane takes per look) through one and three workgroups,
    settled and parked reads in turn: the tables, and exactly every other read parked"""
    run = world.run(kernel)
    n1 = cr.PER_LOOK[kernel][0]
    for n in (1, 64 * n1 - 1, 64 * n1, 64 * n1 + 1, 4 * 64 * n1 - 1, 4 * 64 * n1 + 1):
        r = run["edge_%d" % n]
        for full, alone, tf, ta in invariants(kernel, "edge_%d" % n, r):
            reads, b = model_counts(world, kernel, r, full)
            d = full["dbg"]
            assert len(reads) == n and d["parked1"] == n // 2 == d["park1_one_owner"] == d["walk_lanes"]
            assert int(ta[rows_of(r["ev"], {"A"})][0]) == n - n // 2
