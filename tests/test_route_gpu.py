"""The loader's routing pass (csrc/lsq_route.hpp), read by read: what every front end leaves in the pools -- Context.pool_reads()
-- against the plain reference of tests/route_ref.py, for every line of every case file, with compact and with wide pools, and
the front ends against each other.  The comparison is exact.  Context.locator() proves that a case reaches the grid it is built
for.  Need an MI355X: python -m pytest tests/test_route_gpu.py -m gpu."""
import pytest

import lesseq_amd as L
import route_ref as rr
from bam_writer import sam_to_bam
from test_junctions_host import sam_of

pytestmark = pytest.mark.gpu

E_RANGE = -5


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """per case: the files on disk, and the reference of a text computed once per (library, shard)"""
    out = {}
    for case in rr.all_cases():
        d = tmp_path_factory.mktemp(case.name)
        iv, mp, paths = case.write(str(d))
        out[case.name] = {"case": case, "iv": iv, "mp": mp, "paths": paths, "d": d, "ref": {}}
    return out


def events_of(c, library=None, shard=None):
    ev = L.Events(L.Annotation(c["iv"], c["mp"]), ("SHORT_READ",), (50,), library=library or c["case"].library)
    if shard is not None:
        ev.set_shard(*shard)
    return ev


def reference(c, ev, stem, text=None, shard=None):
    key = (stem, ev.library, shard)
    if key not in c["ref"]:
        job = rr.Job(ev, c["case"].chroms, shard=shard)
        reads, tally = rr.route(job, c["case"].texts[stem] if text is None else text)
        c["ref"][key] = (job, reads, tally, rr.outcomes(job, reads, tally))
    return c["ref"][key]


def context(ev, compact):
    ctx = L.Context(0)
    ctx.set_option("compact_pools", compact)
    ctx.want_compact = bool(compact)
    ctx.upload_events(ev)
    return ctx


def checked(ctx, ev, ref, how, upload):
    """one front end's pools against the reference: -> {bucket: sorted reads}.  The pools have the format the context was asked
    for (every case file is built to stay in compact records), and a stranded job's library report is the reference's tallies."""
    job, reads, tally, _ = ref
    upload()
    compact = ctx.pool_format(0)[0]
    assert compact == ctx.want_compact, (how, compact)
    if job.stranded:
        assert ctx.library_report(0) == (tally["made_plus"], tally["made_minus"], tally["no_strand"], tally["kept_plus"], tally["kept_minus"]), how
    pooled = ctx.pool_reads(0)
    got = rr.check_pools(job, reads, pooled, lambda sid: (L.lib.lsq_events_strand_name(ev.h, sid) or b"?").decode(), compact, what=how)
    assert ctx.retained(0) == len(reads), (how, ctx.retained(0), len(reads))
    assert ctx.pooled(0) == len(pooled), (how, ctx.pooled(0), len(pooled))
    return got, compact


def mrf_front_ends(ctx, ev, ref, path, monkeypatch, what):
    """the raw kernel, the tile kernel plus list, the byte-walking kernel: each against the reference, and all three alike"""
    got = {}
    got["raw"], compact = checked(ctx, ev, ref, what + " raw", lambda: ctx.upload_reads(0, L.Reads.from_mrf(path, ev)))
    got["tile"], _ = checked(ctx, ev, ref, what + " tile", lambda: ctx.upload_reads_mrf(0, path))
    paths = ctx.parse_paths()
    assert not paths["whole_file_byte_walking"], what
    with monkeypatch.context() as m:
        m.setenv("LSQ_MRF_SLOW", "1")
        got["slow"], _ = checked(ctx, ev, ref, what + " slow", lambda: ctx.upload_reads_mrf(0, path))
        assert ctx.parse_paths()["whole_file_byte_walking"], what
    assert got["raw"] == got["tile"] == got["slow"], what
    return got["raw"], compact, paths


def sam_expressible(text):
    """the lines of an MRF text a SAM record can say: one chromosome, positive coordinates, blocks ascending with a gap, as
    sam_of's reads"""
    out = []
    for _, blocks in rr.parse_mrf(text):
        if len(set(b[0] for b in blocks)) == 1 and blocks[0][2] >= 0 and all(b[2] < b[3] for b in blocks) and all(x[3] < y[2] for x, y in zip(blocks, blocks[1:])):
            out.append((blocks[0][0], blocks[0][1] == "-", [(b[2], b[3]) for b in blocks]))
    return out


def sam_bam_front_ends(c, ctx, ev, stem, what):
    """the case's SAM-expressible lines through the SAM and the BAM kernels, against the reference on sam_to_mrf of the text"""
    sam = sam_of(sam_expressible(c["case"].texts[stem])).encode()
    assert sam.count(b"\n") > 200, what
    ref = reference(c, ev, stem + ".sam", text=L.sam_to_mrf(sam).decode())
    assert ref[3]["one"] >= 1 and ref[3]["two"] >= 1 and ref[3]["dropped"] >= 1, (what, ref[3])
    ps, pb = str(c["d"] / (stem + ".sam")), str(c["d"] / (stem + ".bam"))
    with open(ps, "wb") as f:
        f.write(sam)
    with open(pb, "wb") as f:
        f.write(sam_to_bam(sam))
    a, _ = checked(ctx, ev, ref, what + " sam", lambda: ctx.upload_reads_sam(0, ps))
    b, _ = checked(ctx, ev, ref, what + " bam", lambda: ctx.upload_reads_bam(0, pb))
    assert a == b, what


@pytest.mark.parametrize("compact", [1, 0])
def test_bins(cases, compact, monkeypatch):
    """shift 10; bins of few and of many starts (both branches of route_covered and route_cluster), blocks on every region's and
    every bin's edges, before bin 0 and behind the last bin, negative coordinates, first bases around every span's ends"""
    c = cases["bins"]
    ev = events_of(c)
    ref = reference(c, ev, "r")
    job = ref[0]
    rr.assert_contains(c["case"], "r", ref[3])
    ctx = context(ev, compact)
    loc = ctx.locator()
    assert loc["shift"] == 10
    for name in ("chrA", "chrB", "chrC", "chrD"):
        base, nb = rr.locator_of(job, name)
        got = loc["tables"][ev.chrom_id(name)]
        assert got == (base, nb), (name, got, base, nb)
    assert loc["tables"][ev.chrom_id("chrA")][0] == min(s for s, _ in job.regions("chrA", 0))
    cov = rr.starts_per_bin([s for s, _ in job.regions("chrA", 0)], *rr.locator_of(job, "chrA"))
    spans = rr.starts_per_bin([job.ev[i][2] for i in job.planned if job.ev[i][0] == "chrA"], *rr.locator_of(job, "chrA"))
    assert set(cov) >= {0, 1, 3, 4, 5} and max(cov) >= 9 and max(spans) >= 5
    mrf_front_ends(ctx, ev, ref, c["paths"]["r"], monkeypatch, "bins")
    sam_bam_front_ends(c, ctx, ev, "r", "bins")
    ctx.close()


@pytest.mark.parametrize("compact", [1, 0])
def test_wide(cases, compact, monkeypatch):
    """four chromosomes of 2^30 bases stay under the grid's cap at shift 10, five go to shift 11: the same reads, on the edges of
    bins of either width, come out the same"""
    lines = {}
    for name, shift in (("wide4", 10), ("wide5", 11)):
        c = cases[name]
        ev = events_of(c)
        ref = reference(c, ev, "r")
        job = ref[0]
        rr.assert_contains(c["case"], "r", ref[3])
        ctx = context(ev, compact)
        loc = ctx.locator()
        assert loc["shift"] == shift == rr.shift_of(job, c["case"].chroms)
        for q in range(int(name[4:])):
            base, nb = rr.locator_of(job, "chrW%d" % q, shift=shift)
            assert loc["tables"][ev.chrom_id("chrW%d" % q)] == (base, nb) and base == 0 and nb == (1073000380 >> shift) + 1, (name, q)
        got, _, paths = mrf_front_ends(ctx, ev, ref, c["paths"]["r"], monkeypatch, name)
        assert paths["lines_to_shared_splitter"] >= 1, paths          # the ten-digit coordinates: the tile kernel hands those lines on
        sam_bam_front_ends(c, ctx, ev, "r", name)
        ctx.close()
        lines[name] = sorted(x[:3] for v in got.values() for x in v)
    assert lines["wide4"] == lines["wide5"] and len(lines["wide4"]) > 300       # what the reads come to does not depend on the grid


@pytest.mark.parametrize("compact", [1, 0])
@pytest.mark.parametrize("stem", ["fixed", "seed1", "seed2", "seed3"])
def test_merge(cases, stem, compact, monkeypatch):
    """one long exon keeps every block: orderings of overlapping, nested, equal, touching, disjoint, empty and inverted blocks,
    reads that shrink, reads of up to 16 blocks, a last kept block of another chromosome or strand"""
    c = cases["merge"]
    ev = events_of(c)
    ref = reference(c, ev, stem)
    rr.assert_contains(c["case"], stem, ref[3])
    if stem == "fixed":
        assert sorted(set(len(r.blocks) for r in ref[1].values()))[-1] == 16 and {3, 5, 9, 16} <= set(len(r.blocks) for r in ref[1].values())
    ctx = context(ev, compact)
    mrf_front_ends(ctx, ev, ref, c["paths"][stem], monkeypatch, "merge " + stem)
    ctx.close()


@pytest.mark.parametrize("compact", [1, 0])
def test_limits(cases, compact, monkeypatch):
    """the first and last representable bases; 2^18 - 1 merged bases are pooled, 2^18 are refused by every front end, and the
    context loads a good file afterwards; a many-block list that is sized again gives the same pools"""
    c = cases["limits"]
    ev = events_of(c)
    ref = reference(c, ev, "good")
    rr.assert_contains(c["case"], "good", ref[3])
    ctx = context(ev, compact)
    assert ctx.locator()["shift"] == 10
    loc = ctx.locator()["tables"]
    assert loc[ev.chrom_id("chrP")] == rr.locator_of(ref[0], "chrP") and loc[ev.chrom_id("chrQ")] == rr.locator_of(ref[0], "chrQ")
    want, is_compact, _ = mrf_front_ends(ctx, ev, ref, c["paths"]["good"], monkeypatch, "limits")
    assert is_compact == bool(compact) and ref[3]["long_block"] >= 2          # (check_pools: in compact pools those sit in "many")
    lines = {x[0]: x for v in want.values() for x in v}
    assert sum(e - s for s, e in lines[16][2]) == rr.BIG - 1 == sum(e - s for s, e in lines[17][2]) and len(lines[17][2]) == 3
    assert lines[1][2] == ((rr.LIM - 21, rr.LIM - 1),) and lines[7][2] == ((-rr.LIM + 1, -rr.LIM + 21),) and 3 not in lines and 9 not in lines
    for stem in ("big1", "big3"):
        for how in ("raw", "tile", "slow"):
            with monkeypatch.context() as m:
                if how == "slow":
                    m.setenv("LSQ_MRF_SLOW", "1")
                with pytest.raises(L.LsqError) as ei:
                    if how == "raw":
                        ctx.upload_reads(0, L.Reads.from_mrf(c["paths"][stem], ev))
                    else:
                        ctx.upload_reads_mrf(0, c["paths"][stem])
                assert ei.value.status == E_RANGE, (stem, how)
            again, _ = checked(ctx, ev, ref, "limits after %s %s" % (stem, how), lambda: ctx.upload_reads_mrf(0, c["paths"]["good"]))
            assert again == want, (stem, how)
    with monkeypatch.context() as m:
        m.setenv("LSQ_NB_LIST", "8")              # fewer places than the file has many-block reads: the list is sized again
        assert ref[3]["many"] > 8
        again, _, _ = mrf_front_ends(ctx, ev, ref, c["paths"]["good"], monkeypatch, "limits, short list")
        assert again == want
    ctx.close()


@pytest.mark.parametrize("compact", [1, 0])
@pytest.mark.parametrize("library", ["forward", "reverse"])
def test_stranded(cases, library, compact, monkeypatch):
    """a plus and a minus gene overlap with different exons: every block is filtered against the regions of the read's transcript
    strand, which the first block's strand column gives"""
    c = cases["stranded"]
    ev = events_of(c, library=library)
    ref = reference(c, ev, "r")
    job, reads, tally, o = ref
    for k in ("no_strand", "dropped", "unrouted", "one", "two", "many"):
        assert o[k] >= 1, (k, o)
    assert tally["kept_plus"] >= 1 and tally["kept_minus"] >= 1 and job.regions("chrS", 0) != job.regions("chrS", 1)
    ctx = context(ev, compact)
    mrf_front_ends(ctx, ev, ref, c["paths"]["r"], monkeypatch, "stranded " + library)       # (the library report too, per front end)
    ctx.close()


@pytest.mark.parametrize("compact", [1, 0])
def test_shard(cases, compact, monkeypatch):
    """two slices of a job whose genes interleave: a read in the spans of the other slice's events only is in no pool, and the
    slices' pooled reads together are the unsharded job's"""
    c = cases["shard"]
    flat = lambda got: set(x[:3] for v in got.values() for x in v)
    ev = events_of(c)
    ref = reference(c, ev, "r")
    rr.assert_contains(c["case"], "r", ref[3])
    ctx = context(ev, compact)
    whole, _, _ = mrf_front_ends(ctx, ev, ref, c["paths"]["r"], monkeypatch, "shard, whole")
    ctx.close()
    parts = []
    for q, shard in enumerate(((0, 5), (5, 5))):
        ev = events_of(c, shard=shard)
        ref = reference(c, ev, "r", shard=shard)
        rr.assert_contains(c["case"], "r", ref[3], rr.WANT_SLICE + (("closed_only",) if q == 0 else ()))
        ctx = context(ev, compact)
        got, _, _ = mrf_front_ends(ctx, ev, ref, c["paths"]["r"], monkeypatch, "shard %d" % q)
        ctx.close()
        parts.append(flat(got))
        unrouted = set(line for line, r in ref[1].items() if not r.may)
        assert unrouted and not unrouted & set(x[0] for x in parts[-1])
    assert parts[0] | parts[1] == flat(whole) and parts[0] != parts[1]
