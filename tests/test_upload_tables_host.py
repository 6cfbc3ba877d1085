"""The tables lsq_events_upload copies to the device (csrc/lsq_upload_tables.cpp), each held against its definition on the host:
Events.upload_tables() runs the same functions the upload does, without a context.  The loader's tables on every case of
route_ref.py; the EM placement on gene sets of a few events, one per rule, against lists worked out by hand.  No GPU.
(tests/test_route_gpu.py reads the uploaded records back: that the device holds these tables is proved there.)"""
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
import route_ref as rr
from golden_inputs import interval_line

PAD = 0xFFFFFFFF
WAVE_PLACES = 16              # 64 lanes / 4 lanes an event


# ------------------------------------------------------------------------------------------------------- what the events say
def device_order(ev):
    """output index of every device event: the buckets in order, each bucket's events in its own order; and per bucket
    (kind, first device event, events)"""
    dev2out, buckets = [], []
    for b in range(ev.num_buckets):
        kind, events = ev.bucket_events(b)
        buckets.append((kind, len(dev2out), events))
        dev2out += events
    return dev2out, buckets


def table_id(ev, job, chrom, t):
    cid = ev.chrom_id(chrom)
    return -1 if cid < 0 else (2 * cid + t if job.stranded else cid)


class Tables:
    def __init__(self, case, ev, shard):
        self.name = case.name + ("" if shard is None else " shard %d+%d" % shard)
        self.case, self.ev, self.job = case, ev, rr.Job(ev, case.chroms, shard=shard)
        self.t = ev.upload_tables()
        self.shift, self.n_tab = (int(x) for x in self.t["route_shift"])
        self.dev2out, self.buckets = device_order(ev)
        # per bucket: table id, first base, largest span end -- from its events' chromosome, strand and spans
        self.bucket_tab, self.bucket_lo, self.bucket_hi = [], [], []
        for _, _, events in self.buckets:
            c, st = self.job.ev[events[0]][:2]
            self.bucket_tab.append(table_id(ev, self.job, c, int(st == "-") if self.job.stranded else 0))
            self.bucket_lo.append(min(self.job.ev[i][2] for i in events))
            self.bucket_hi.append(max(self.job.ev[i][3] for i in events))

    def tables_of_case(self):
        """(chromosome, transcript strand, table id) of every chromosome name of the case that has a table id"""
        for c in self.case.chroms:
            for t in ((0, 1) if self.job.stranded else (0,)):
                tid = table_id(self.ev, self.job, c, t)
                if 0 <= tid < self.n_tab:
                    yield c, t, tid

    def planned_spans(self, chrom, t):
        return sorted(self.job.ev[i][2:4] for i in self.job.planned
                      if self.job.ev[i][0] == chrom and (not self.job.stranded or self.job.ev[i][1] == "+-"[t]))


@pytest.fixture(scope="module")
def route_tables(tmp_path_factory):
    out = []
    for case in rr.all_cases():
        iv, mp, _ = case.write(str(tmp_path_factory.mktemp(case.name)))
        for shard in ((None, (0, 5), (5, 5)) if case.name == "shard" else (None,)):
            ev = L.Events(L.Annotation(iv, mp), ("SHORT_READ",), (50,), library=case.library)
            if shard is not None:
                ev.set_shard(*shard)
            out.append(Tables(case, ev, shard))
    assert [T.name for T in out] == ["bins", "wide4", "wide5", "merge", "limits", "stranded", "shard", "shard shard 0+5", "shard shard 5+5"]
    return out


def closed_union(intervals):
    """sorted closed integer intervals, merged where they overlap or touch"""
    out = []
    for s, e in sorted(intervals):
        if out and s <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


# ------------------------------------------------------------------------------------------------------- the loader's tables
def test_covered_records_are_the_events_regions(route_tables):
    for T in route_tables:
        chrom, cov = T.t["route_chrom"], T.t["cov"]
        assert len(chrom) == max(T.n_tab, 1) and (chrom[:, 7] == 0).all(), T.name
        seen = 0
        for c, t, tid in T.tables_of_case():
            c0, c1 = int(chrom[tid, 3]), int(chrom[tid, 4])
            assert [tuple(int(v) for v in r) for r in cov[c0:c1]] == T.job.regions(c, t), (T.name, c, t)
            seen += c1 - c0
        assert seen == len(cov) and seen > 0, T.name          # (every record belongs to a table of the case; no dummy needed)


def test_locator_shift_base_and_bins_are_route_refs(route_tables):
    for T in route_tables:
        assert T.shift == rr.shift_of(T.job, T.case.chroms), T.name
        chrom = T.t["route_chrom"]
        with_records = 0
        for c, t, tid in T.tables_of_case():
            if not T.job.regions(c, t) and not T.planned_spans(c, t):
                assert int(chrom[tid, 1]) == 0, (T.name, c, t)
                continue
            base, nb = rr.locator_of(T.job, c, t, shift=T.shift)
            assert (int(chrom[tid, 2]), int(chrom[tid, 1])) == (base, nb), (T.name, c, t)
            with_records += 1
        assert with_records >= 2, T.name
    by_name = {T.name: T for T in route_tables}
    assert by_name["wide4"].shift == 10 and by_name["wide5"].shift == 11
    assert len(by_name["wide4"].t["loc"]) == 4191412 + 2


def test_locator_entries_are_lower_bounds_of_each_bins_first_base(route_tables):
    for T in route_tables:
        chrom, cov, clu, loc = T.t["route_chrom"], T.t["cov"], T.t["clu"], T.t["loc"]
        at_a_start = 0
        n_entries = 0
        for tid in range(T.n_tab):
            first, nb, base, c0, c1, u0, u1 = (int(v) for v in chrom[tid, :7])
            assert first == n_entries, (T.name, tid)
            if nb == 0:
                continue
            x = base + (np.arange(nb + 1, dtype=np.int64) << T.shift)          # the first base of every bin, and of the one behind the last
            cov_s, clu_s = cov[c0:c1, 0].astype(np.int64), clu[u0:u1, 0].astype(np.int64)
            assert (np.diff(cov_s) > 0).all() and (np.diff(clu_s) > 0).all(), (T.name, tid)
            want = np.stack([c0 + np.searchsorted(cov_s, x, "left"), u0 + np.searchsorted(clu_s, x, "left")], axis=1)
            got = loc[first:first + nb + 1]
            assert np.array_equal(got, want), (T.name, tid, np.nonzero((got != want).any(axis=1))[0][:5])
            at_a_start += int(np.isin(x, cov_s).sum() + np.isin(x, clu_s).sum())
            n_entries += nb + 1
        assert len(loc) == n_entries + 2 and (loc[n_entries:] == 0).all(), T.name          # (an entry is read as a pair with its successor)
        if T.name in ("bins", "wide4", "wide5"):
            assert at_a_start >= 2, T.name          # (a start ON a bin's first base: lower bound, not upper)


def test_cluster_records_are_cut_at_the_bucket_cuts(route_tables):
    for T in route_tables:
        chrom, clu = T.t["route_chrom"], T.t["clu"]
        seen = 0
        for c, t, tid in T.tables_of_case():
            u0, u1 = int(chrom[tid, 5]), int(chrom[tid, 6])
            recs = [tuple(int(v) for v in r) for r in clu[u0:u1]]
            seen += len(recs)
            mine = [b for b in range(len(T.buckets)) if T.bucket_tab[b] == tid]
            spans = T.planned_spans(c, t)
            if not mine:
                assert not recs and not spans, (T.name, c, t)
                continue
            assert mine == list(range(mine[0], mine[-1] + 1)), (T.name, c, t)
            cuts = [T.bucket_lo[b] for b in mine]
            assert cuts == sorted(cuts) and len(set(cuts)) == len(cuts), (T.name, c, t)
            for s, e, b, lo in recs:
                assert s <= e and not any(s < cut <= e for cut in cuts), (T.name, c, t, "a record crosses a cut", (s, e))
                want_b = mine[0] + max(q for q in range(len(cuts)) if cuts[q] <= s)          # (a record left of the first cut: max() of nothing)
                assert (b, lo) == (want_b, T.bucket_lo[want_b]), (T.name, c, t, (s, e, b, lo), want_b)
                assert e <= T.bucket_hi[b], (T.name, c, t, "end beyond the bucket's hi", (s, e, b))
            # (a span is closed at its end: a read whose first base is gene_end is still a candidate)
            assert closed_union((s, e) for s, e, _, _ in recs) == closed_union(spans), (T.name, c, t)
            assert min(s for s, _, _, _ in recs) >= cuts[0], (T.name, c, t)
        assert seen == len(clu) and seen > 0, T.name
    # the cuts that matter: a case with more than one bucket on a chromosome, and the slices of the shard
    assert any(sum(1 for b in T.bucket_tab if b == T.bucket_tab[0]) > 1 for T in route_tables)


def test_group_bases_are_prefix_sums(route_tables):
    for T in route_tables:
        B = T.ev.num_buckets
        bin_base, cell_base, jgroup_base = (T.t[k].astype(np.int64) for k in ("bin_base", "cell_base", "jgroup_base"))
        assert len(bin_base) == len(cell_base) == len(jgroup_base) == B + 1, T.name
        bins = T.t["bucket_bins"].astype(np.int64)          # the buckets' own bins and junction-group bases, as compiled
        jg_base = T.t["jg_base"].astype(np.int64)
        assert len(bins) == B and (bins >= 1).all() and len(jg_base) == B + 1 and jg_base[0] == 0 and (np.diff(jg_base) >= 0).all(), T.name
        assert bin_base.tolist() == [0] + np.cumsum(bins).tolist(), T.name
        cells = [len(T.ev.bucket_cells(b)) if T.buckets[b][0] == 1 else 0 for b in range(B)]
        assert cell_base.tolist() == [0] + np.cumsum([n + 1 for n in cells]).tolist(), T.name          # (its cells and one group more)
        assert jgroup_base.tolist() == (jg_base + np.array([0] + np.cumsum([n + 1 for n in cells]).tolist())).tolist(), T.name
        assert T.t["group_totals"].tolist() == [bin_base[-1], cell_base[-1], jgroup_base[-1]], T.name
    # (cases with cells, with junction groups, and with buckets of more than one bin: each sum has something to add up)
    assert any(sum(len(T.ev.bucket_cells(b)) for b in range(T.ev.num_buckets)) > 0 and T.t["jg_base"][-1] > 0 and (T.t["bucket_bins"] > 1).any() for T in route_tables)


def test_pack_lists_and_weights(route_tables):
    for T in route_tables:
        ev, d2o = T.ev, T.dev2out
        assert sorted(d2o) == list(T.job.planned), T.name
        K = [ev.K(o) for o in d2o]
        cls_base = [0] + np.cumsum([(1 << k) - 1 for k in K]).tolist()
        iso_base = [0] + np.cumsum(K).tolist()
        by_output = sorted(range(len(d2o)), key=lambda d: d2o[d])
        assert T.t["pack_ev"].tolist() == by_output, T.name
        assert T.t["pack_cls"].tolist() == [cls_base[d] + k for d in by_output for k in range((1 << K[d]) - 1)], T.name          # 2^K - 1 slots an event
        assert T.t["pack_iso"].tolist() == [iso_base[d] + j for d in by_output for j in range(K[d])], T.name
        assert sorted(T.t["pack_cls"].tolist()) == list(range(cls_base[-1])) and sorted(T.t["pack_iso"].tolist()) == list(range(iso_base[-1])), T.name
        want = [0.0] * iso_base[-1]
        for d, o in enumerate(d2o):
            for j in range(K[d]):
                a = ev.ars(0, o, j)
                want[iso_base[d] + j] = 1.0 / a if a > 0 else 0.0
        assert T.t["G"].tolist() == want, T.name
        names = b"".join(ev.gene_name(o).encode() for o in d2o)
        assert T.t["gene_names"].tobytes() == names, T.name
        assert T.t["gene_name_off"].tolist() == [0] + np.cumsum([len(ev.gene_name(o)) for o in d2o]).tolist(), T.name


# ------------------------------------------------------------------------------------------------------- the EM placement
def placement_genes():
    """one chromosome, ascending: K = 1; K = 2; K = 3; K = 2 with an isoform of exactly one read length (one accessible start);
    seven isoforms (beyond the kernels' limit of six: a host bucket)"""
    g = [("e1_k1", "chrE", "+", [[(1000, 1200)]]),
         ("e2_k2", "chrE", "+", [[(3000, 3100), (3200, 3300)], [(3000, 3100)]]),
         ("e3_k3", "chrE", "+", [[(5000, 5100), (5200, 5300), (5400, 5500)], [(5000, 5100), (5400, 5500)], [(5000, 5100)]]),
         ("e4_unit", "chrE", "+", [[(7000, 7050), (7100, 7200)], [(7000, 7050)]])]
    exons = [(9000 + 200 * k, 9100 + 200 * k) for k in range(8)]
    g.append(("e5_host", "chrE", "+", [[exons[0], exons[k + 1]] for k in range(7)]))
    return g


@pytest.fixture(scope="module")
def placement_files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("placement"))
    iv, mp = os.path.join(d, "p.interval"), os.path.join(d, "p.map")
    with open(iv, "w") as f, open(mp, "w") as g:
        for gene, chrom, strand, isoforms in placement_genes():
            for k, exons in enumerate(isoforms):
                f.write(interval_line("%s.%d" % (gene, k), chrom, strand, exons))
                g.write("%s\t%s.%d\n" % (gene, gene, k))
    return iv, mp


def placement_of(placement_files, n_files):
    ev = L.Events(L.Annotation(*placement_files), ("SHORT_READ",) * n_files, (50,) * n_files)
    dev2out, buckets = device_order(ev)
    # the premises of the lists below: device order is the order on the chromosome, the K are as built, e4 has an isoform
    # with one accessible start in every read file and no other event has, e5 sits in a host bucket
    assert [ev.gene_name(o) for o in dev2out] == ["e1_k1", "e2_k2", "e3_k3", "e4_unit", "e5_host"]
    assert [ev.K(o) for o in dev2out] == [1, 2, 3, 2, 7]
    unit = [any(ev.ars(m, o, j) == 1 for m in range(n_files) for j in range(ev.K(o))) for o in dev2out[:4]]
    assert unit == [False, False, False, True]
    assert [kind for kind, _, events in buckets for _ in events] == [1, 1, 1, 1, 2]
    t = ev.upload_tables("em_order", "em_places")
    return t["em_order"].tolist(), t["em_places"].tolist()


def test_em_placement_one_read_file(placement_files):
    order, (small_places, places) = placement_of(placement_files, 1)
    # lean: K <= 2, one (read file, class) pair a lane (1 and 3 pairs for 4 lanes), no isoform with one accessible start
    assert order[:16] == [0, 1] + [PAD] * 14
    assert order[16:] == [2, 3] + [PAD] * 14          # the others; the host bucket's event has no place
    assert (small_places, places) == (16, 32) and small_places % WAVE_PLACES == 0 and places % WAVE_PLACES == 0


def test_em_placement_two_read_files(placement_files):
    order, (small_places, places) = placement_of(placement_files, 2)
    assert order[:16] == [0] + [PAD] * 15             # K = 2 takes 2 x 3 pairs: more than four lanes
    assert order[16:] == [1, 2, 3] + [PAD] * 13
    assert (small_places, places) == (16, 32)


def test_em_placement_on_the_route_cases(route_tables):
    """lean events first, both groups padded to whole waves, every planned event once (no case has a host bucket)"""
    for T in route_tables:
        order = T.t["em_order"].tolist()
        small_places, places = T.t["em_places"].tolist()
        assert len(order) == places and small_places % WAVE_PLACES == 0 and places % WAVE_PLACES == 0, T.name
        lean = [d for d in order[:small_places] if d != PAD]
        rest = [d for d in order[small_places:] if d != PAD]
        assert sorted(lean + rest) == list(range(len(T.dev2out))) and all(kind != 2 for kind, _, _ in T.buckets), T.name
        is_lean = lambda d: T.ev.K(T.dev2out[d]) <= 2 and not any(T.ev.ars(0, T.dev2out[d], j) == 1 for j in range(T.ev.K(T.dev2out[d])))
        assert lean == [d for d in range(len(T.dev2out)) if is_lean(d)] and rest == [d for d in range(len(T.dev2out)) if not is_lean(d)], T.name
        assert order[len(lean):small_places] == [PAD] * (small_places - len(lean)) and small_places - len(lean) < WAVE_PLACES, T.name


# ------------------------------------------------------------------------------------------------------- events made by hand
def test_a_cluster_left_of_the_first_cut_gets_no_record(tmp_path):
    """tools/upload_tables_check.cpp, built against the library under test and run: every table of the bins case's events with
    one read file and with two, then the loader's tables of events made by hand whose first cluster begins left of the first
    bucket cut and whose second lies across it -- the planner makes neither, so no compiled events reach that rule"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir, lib_name = os.path.split(os.path.abspath(L._lib.LIB_PATH))
    exe = str(tmp_path / "upload_tables_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", "-o", exe, os.path.join(root, "tools", "upload_tables_check.cpp"),
                    "-L" + lib_dir, "-l:" + lib_name, "-Wl,-rpath," + lib_dir], check=True, timeout=120)
    iv, mp, _ = rr.bins_case().write(str(tmp_path))
    p = subprocess.run([exe, iv, mp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and p.stdout.decode().endswith("upload_tables_check: ok\n"), (p.returncode, p.stdout[-500:], p.stderr[-500:])
