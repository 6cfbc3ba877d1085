"""Splice-site usage and read-through per junction on the device (lsq_ss_device: lsq_readfile.hip, lsq_junc.hip, lsq_sites.hip): the
through count at the smallest shapes at which each part can go wrong, against the definition as tests/sites_ref.py restates it
and against lsq_ss_host.  All values are integers: the device table equals both exactly, in rows, report and text.  Need an
MI355X: python -m pytest tests -m gpu."""
import os
import subprocess

import pytest

import lesseq_amd as L
import bam_writer
import junction_ref as J
import sites_ref as S
from lesseq_amd.sites import LDS_SLOTS
from test_junctions_host import sam_of, BIN, LSQ_E_PARSE
from test_sites_host import index_of, format_reads, BIG
from test_sam_gpu import CHILD_TIMEOUT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same(got, rows, report):
    assert got.rows() == rows
    assert got.report == report
    assert got.text() == S.text(rows)
    assert got.text(ratios=True) == S.text(rows, ratios=True)


def check_case(ctx, d, stem, iso, lines, min_overhang=1, key=None, header="AlignmentBlocks\n"):
    """the device table and the host table against the reference's (key: computed once a session); returns (rows, report, paths)"""
    interval, mrf, paths = S.write_case(str(d), stem, iso, lines, header)
    rows, report = S.table_once(key, interval, mrf, min_overhang) if key else S.table(interval, mrf, min_overhang)
    ix = index_of(paths)
    dev = ix.device(ctx, "MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(dev, rows, report)
    host = ix.host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(host, rows, report)
    assert dev.text(1, True, True) == host.text(1, True, True)
    assert set(dev.times) == set(L.sites.PHASES) and all(v >= 0 for v in dev.times.values())
    return rows, report, paths


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None):
    argv = [os.path.join(BIN, "sites")] + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads]
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=CHILD_TIMEOUT)


# ----------------------------------------------------------------------------- boundary arithmetic, rows, walk length

@pytest.mark.parametrize("min_overhang", [0, 1, 2, 10, 50, BIG])
def test_boundary_arithmetic(gpu_ctx, tmp_path, min_overhang):
    iso, lines = S.boundary_case()
    rows, report, _ = check_case(gpu_ctx, tmp_path, "edge", iso, lines, min_overhang, key="edge")
    by = {r[:3]: r for r in rows}
    assert len(rows) == 5 and report["boundaries"] == 10
    if min_overhang == BIG:
        assert report["through"] == 0
    if min_overhang in (0, 1):
        assert by[("chr2", 1000, 2000)][6] == 7 + 3 * 11
    if min_overhang == 50:
        assert by[("chr2", 1000, 2000)][6] == 7 and by[("chr2", 1000, 2000)][8] == 7


def test_the_table_worked_out_by_hand(gpu_ctx, tmp_path):
    iso, lines, rows, report = S.rows_case()
    got = check_case(gpu_ctx, tmp_path, "rows", iso, lines)
    assert got[0] == rows and got[1] == report
    assert rows[0][5] == rows[1][5] == rows[2][5] == 6 and (rows[0][7], rows[1][7], rows[2][7]) == (3, 1, 6)      # a shared start: one sum; the ends stay apart
    assert rows[2][7] == rows[3][7] == 6                                                                       # a shared end
    assert rows[6][8] == rows[7][6] == 4                                                                       # the end of one row, the start of another: one count
    assert rows[4][4] == 0 and rows[4][6] > 0 and rows[4][8] > 0 and rows[5][4:] == (0, 0, 0, 0, 0) and rows[1][3] == "."


@pytest.mark.parametrize("min_overhang", [0, 1, 10, 51])
def test_rows_and_walks_on_the_junction_cases(gpu_ctx, tmp_path, min_overhang):
    """junction_ref's annotation and reads, with the walk's reads: a block over all boundaries of the 70-exon gene, the 40-block read,
    a block behind the chromosome's last boundary and one ahead of its first"""
    rows, report, paths = check_case(gpu_ctx, tmp_path, "base", J.annotation_lines(), J.extract_lines() + S.walk_lines(), min_overhang, key="base")
    if min_overhang:
        jn = L.JunctionIndex(L.Annotation(paths["interval"], paths["map"])).device(gpu_ctx, "MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
        assert [r[:5] for r in rows if r[4] > 0] == [r[:5] for r in jn.rows()]
    assert {r[3] for r in rows} == {".", "+", "-", "*"} and report["unsupported"] > 0


# ----------------------------------------------------------------------------- combining and counters

@pytest.mark.parametrize("kind", ["one_boundary", "all_distinct", "run_lengths"])
def test_counter_cases(gpu_ctx, tmp_path, kind):
    iso, lines = S.counter_case(kind)
    rows, report, paths = check_case(gpu_ctx, tmp_path, kind, iso, lines, key=kind)
    if kind == "one_boundary":      # every lane the same id
        assert rows == [("chr1", 200, 300, "+", 0, 0, 70000, 0, 0)]
    if kind == "all_distinct":
        assert report["boundaries"] == 70000 == report["through"]
    # the same file shuffled, and the same call twice
    interval, mrf, other = S.write_case(str(tmp_path), kind + "_shuffled", iso, S.shuffled(lines))
    ix = index_of(other)
    a, b = ix.device(gpu_ctx, "MRF_SINGLE", other["mrf"]), ix.device(gpu_ctx, "MRF_SINGLE", other["mrf"])
    same(a, rows, report)
    same(b, rows, report)


@pytest.mark.parametrize("grid", [None, 1])
@pytest.mark.parametrize("n", [LDS_SLOTS - 1, LDS_SLOTS, LDS_SLOTS + 1])
def test_as_many_boundaries_as_a_workgroup_has_slots(gpu_ctx, tmp_path, monkeypatch, n, grid):
    """one workgroup (grid 1) meets every id: the last that finds a slot in LDS, the first that goes to the global counter"""
    if grid:
        monkeypatch.setenv("LSQ_SS_GRID", str(grid))
    iso, lines = S.counter_case("slots", n)
    rows, report, _ = check_case(gpu_ctx, tmp_path, "slots", iso, lines, key="slots%d" % n)
    assert report["boundaries"] == n and report["through"] == 3 * n and all(r[6] == 3 == r[8] for r in rows)


@pytest.mark.parametrize("grid", [1, 3])
def test_the_count_strides_over_the_reads(gpu_ctx, tmp_path, monkeypatch, grid):
    """fewer workgroups than the file needs: every workgroup takes several stretches of reads (a 100 M-read file's shape)"""
    monkeypatch.setenv("LSQ_SS_GRID", str(grid))
    lines = J.extract_lines() + S.walk_lines()
    check_case(gpu_ctx, tmp_path, "stride", J.annotation_lines(), lines * 40 + S.shuffled(S.rows_case()[1] * 20) + lines, key="stride")


# ----------------------------------------------------------------------------- degenerate files

def test_degenerate_files(gpu_ctx, tmp_path):
    iso = J.annotation_lines()
    n_introns = len(J.introns("".join(iso)))
    for stem, lines, header in (("unspliced", [J.mrf_line("chr1", "+", [(150, 250)])] * 300, "AlignmentBlocks\n"), ("header_only", [], "AlignmentBlocks\n"), ("nothing", [], "")):
        rows, report, _ = check_case(gpu_ctx, tmp_path, stem, iso, lines, header=header)
        assert len(rows) == n_introns == report["unsupported"] and report["through"] == len(lines) and all(r[4] == 0 for r in rows)
    mono = [J.interval_line("m.a", "chr1", "+", [(0, 1000)])]
    rows, report, _ = check_case(gpu_ctx, tmp_path, "mono", mono, J.extract_lines())
    assert rows and {r[3] for r in rows} == {"."} and report["unsupported"] == 0
    rows, report, _ = check_case(gpu_ctx, tmp_path, "mono_unspliced", mono, [J.mrf_line("chr1", "+", [(150, 250)])] * 300)
    assert rows == [] and report == dict(zip(S.REPORT, (300, 300, 0, 0, 0, 0, 0, 0)))


# ----------------------------------------------------------------------------- formats and options

@pytest.fixture(scope="module")
def formats(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ssgpu"))
    reads = format_reads()
    interval, mrf, paths = S.write_case(d, "fmt", J.annotation_lines(), [J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads])
    sam = sam_of(reads).encode()
    paths["sam"] = os.path.join(d, "fmt.sam")
    open(paths["sam"], "wb").write(sam)
    for layout in ("htslib", "cut997", "cut61", "stored"):
        paths[layout] = os.path.join(d, "fmt_%s.bam" % layout)
        open(paths[layout], "wb").write(bam_writer.sam_to_bam(sam, layout))
    rows, report = S.table_once("fmt", interval, mrf)
    return paths, reads, rows, report, interval, d


def test_one_table_from_mrf_sam_and_bam(gpu_ctx, formats):
    paths, _, rows, report, _, _ = formats
    ix = index_of(paths)
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), rows, report)
    same(ix.device(gpu_ctx, "SAM_SINGLE", paths["sam"]), rows, report)
    for layout in ("htslib", "cut997", "cut61", "stored"):
        same(ix.device(gpu_ctx, "BAM_SINGLE", paths[layout]), rows, report)
    for fmt in ("UCSC_GFF", "MRF_PAIRED"):
        with pytest.raises(L.LsqError) as e:
            ix.device(gpu_ctx, fmt, paths["mrf"])
        assert e.value.status == -3 and str(e.value).endswith("Unknown file format error: " + fmt)


def test_the_contexts_filters_are_respected(formats):
    paths, reads, rows, _, interval, d = formats
    last = len(reads) - 1
    at = [i for i, r in enumerate(rows) if r[:3] == ("chr1", 3100, 3200)][0]
    assert rows[at][6] == 1
    want = list(rows)
    want[at] = rows[at][:6] + (0,) + rows[at][7:]
    ix = index_of(paths)
    for name, kw, option, value in (("mapq", dict(mapq={last: 3}), "sam_min_mapq", 4), ("flag", dict(flags={last: 0x400}), "sam_skip_flags", 0x904 | 0x400)):
        sam = sam_of(reads, **kw).encode()
        path = os.path.join(d, name + ".sam")
        open(path, "wb").write(sam)
        bam = os.path.join(d, name + ".bam")
        open(bam, "wb").write(bam_writer.sam_to_bam(sam))
        ctx = L.Context(0)
        assert ix.device(ctx, "SAM_SINGLE", path).rows() == rows
        ctx.set_option(option, value)
        assert ix.device(ctx, "SAM_SINGLE", path).rows() == want
        assert ix.device(ctx, "BAM_SINGLE", bam).rows() == want
        assert ix.host("SAM_SINGLE", path, **{"min_mapq" if name == "mapq" else "skip_flags": value}).rows() == want
        ctx.close()


def test_bam_verify_on_a_damaged_file(formats):
    paths, _, rows, report, _, d = formats
    data = bytearray(open(paths["htslib"], "rb").read())
    data[-28 - 8] ^= 1           # the stored CRC32 of the last block ahead of the end-of-file marker
    bad = os.path.join(d, "bad_crc.bam")
    open(bad, "wb").write(bytes(data))
    ix = index_of(paths)
    ctx = L.Context(0)
    same(ix.device(ctx, "BAM_SINGLE", bad), rows, report)        # unverified: the blocks inflate as before
    ctx.set_option("bam_verify", 1)
    same(ix.device(ctx, "BAM_SINGLE", paths["htslib"]), rows, report)
    with pytest.raises(L.LsqError) as e:
        ix.device(ctx, "BAM_SINGLE", bad)
    assert e.value.status == -3 and "CRC32 mismatch" in str(e.value)
    ctx.close()
    p = tool(paths, bad, "BAM_SINGLE", env={"LSQ_BAM_VERIFY": "1"})
    assert p.returncode == 1 and p.stdout == "" and "CRC32 mismatch" in p.stderr


def test_malformed_lines_give_counts_status_and_message(gpu_ctx, formats, tmp_path):
    paths, _, rows, report, _, _ = formats
    good = J.mrf_line("chr1", "+", [(150, 200), (300, 350)])
    bad = "chr1:+:15x:200:1:50"
    path = str(tmp_path / "bad.mrf")
    open(path, "w").write("AlignmentBlocks\n" + good * 400 + bad + "\n" + good * 3)
    ix = index_of(paths)
    with pytest.raises(L.LsqError) as host:
        ix.host("MRF_SINGLE", path)
    with pytest.raises(L.LsqError) as e:
        ix.device(gpu_ctx, "MRF_SINGLE", path)
    assert e.value.status == LSQ_E_PARSE and str(e.value).endswith(": #401:" + bad) and str(e.value) == str(host.value)
    p = tool(paths, path)
    assert p.returncode == 1 and p.stdout == "" and "#401:" + bad in p.stderr
    sam = "@HD\tVN:1.6\n" + "q\t0\tchr1\t101\t60\t50M10N50M\t*\t0\t0\t*\t*\n" * 7 + "q\t0\tchr1\t101\t60\t50Q\t*\t0\t0\t*\t*\n"
    spath = str(tmp_path / "bad.sam")
    open(spath, "w").write(sam)
    with pytest.raises(L.LsqError) as host:
        ix.host("SAM_SINGLE", spath)
    with pytest.raises(L.LsqError) as e:
        ix.device(gpu_ctx, "SAM_SINGLE", spath)
    assert e.value.status == LSQ_E_PARSE and str(e.value) == str(host.value)
    # the context is as good as before
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), rows, report)


# ----------------------------------------------------------------------------- context

def test_a_context_with_events_and_counted_reads_is_left_as_it_was(formats):
    from test_sam_gpu import count_table
    paths, _, rows, report, _, _ = formats
    d = os.path.join(GOLD, "toy")
    ix = index_of(paths)
    fresh = L.Context(0)
    same(ix.device(fresh, "MRF_SINGLE", paths["mrf"]), rows, report)       # a context without events
    fresh.close()
    ev = L.Events(L.Annotation(os.path.join(d, "toy.interval"), os.path.join(d, "toy.map"), 0, 10), ("SHORT_READ",), (50,))
    ctx = L.Context(0)
    ctx.upload_events(ev)
    ctx.upload_reads_mrf(0, os.path.join(d, "toy.mrf"))
    before = count_table(ctx, ev)
    assert before == open(os.path.join(d, "count.out")).read()
    same(ix.device(ctx, "MRF_SINGLE", paths["mrf"]), rows, report)
    same(ix.device(ctx, "SAM_SINGLE", paths["sam"]), rows, report)
    assert count_table(ctx, ev) == before
    ctx.upload_reads_mrf(0, os.path.join(d, "toy.mrf"))                     # the events' dictionaries still serve an upload
    assert count_table(ctx, ev) == before
    ctx.close()


# ----------------------------------------------------------------------------- executable

def test_the_executable(formats, tmp_path):
    paths, _, rows, _, interval, _ = formats
    ix = index_of(paths)
    ctx = L.Context(0)
    table = ix.device(ctx, "MRF_SINGLE", paths["mrf"])
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == table.text() == S.text(rows), p.stderr
    assert "boundary(ies)" in p.stderr
    h = tool(paths, paths["mrf"], opts=["--host"])
    assert h.returncode == 0 and h.stdout == p.stdout
    for opts, want in ((["--min-reads", "3"], table.text(3)), (["--novel"], table.text(0, True)), (["--min-reads", "2", "--novel"], table.text(2, True)),
                       (["--ratios"], table.text(ratios=True)), (["--ratios", "--min-reads", "1"], table.text(1, False, True))):
        p = tool(paths, paths["mrf"], opts=opts)
        assert p.returncode == 0 and p.stdout == want and want != table.text()
        h = tool(paths, paths["mrf"], opts=["--host"] + opts)
        assert h.returncode == 0 and h.stdout == want
    want = ix.device(ctx, "MRF_SINGLE", paths["mrf"], min_overhang=30).text()
    p = tool(paths, paths["sam"], "SAM_SINGLE", opts=["--min-overhang", "30"])
    assert p.returncode == 0 and p.stdout == want == S.text(S.table(interval, open(paths["mrf"]).read(), 30)[0]) and want != table.text()
    p = tool(paths, paths["mrf"], opts=["--min-overhang", "0"])
    assert p.returncode == 0 and p.stdout == ix.device(ctx, "MRF_SINGLE", paths["mrf"], min_overhang=0).text()
    p = tool(paths, paths["mrf"], opts=["--nonsense"])
    assert p.returncode == 1 and p.stdout == "" and "Usage:\nsites " in p.stderr
    out = str(tmp_path / "out.tab")
    p = subprocess.run([os.path.join(BIN, "sites"), "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "BAM_SINGLE", paths["cut61"], out],
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == table.text()
    ctx.close()
