"""Splice junctions on the device (lsq_jn_device: lsq_readfile.hip, lsq_junc.hip, lsq_sort.hpp): every phase at the smallest shapes
at which it can go wrong, against the definition as tests/junction_ref.py restates it and against lsq_jn_host.  All values are
integers: the device table equals both exactly.  Need an MI355X: python -m pytest tests -m gpu."""
import os
import subprocess

import pytest

import lesseq_amd as L
import bam_writer
import junction_ref as J
from lesseq_amd.junctions import SORT_TILE
from test_junctions_host import index_of, sam_of, spliced_reads, BIN, LSQ_E_PARSE
from test_sam_gpu import CHILD_TIMEOUT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same(got, rows, report):
    assert got.rows() == rows
    assert got.report == report
    assert got.text() == J.text(rows)


def check_case(ctx, d, stem, iso, lines, min_overhang=1, want=None):
    """the device table and the host table against the reference's; returns (rows, report, paths)"""
    interval, mrf, paths = J.write_case(str(d), stem, iso, lines)
    rows, report = want or J.table(interval, mrf, min_overhang)
    ix = index_of(paths)
    dev = ix.device(ctx, "MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(dev, rows, report)
    same(ix.host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang), rows, report)
    assert set(dev.times) == set(L.junctions.PHASES) and all(v >= 0 for v in dev.times.values())
    return rows, report, paths


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None):
    argv = [os.path.join(BIN, "junctions")] + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads]
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=CHILD_TIMEOUT)


# ----------------------------------------------------------------------------- extract, annotate

@pytest.mark.parametrize("min_overhang", [1, 9, 10, 11, 50, 51])
def test_extract_and_annotate_cases(gpu_ctx, tmp_path, min_overhang):
    rows, report, _ = check_case(gpu_ctx, tmp_path, "base", J.annotation_lines(), J.extract_lines(), min_overhang)
    if min_overhang == 1:
        assert {r[3] for r in rows} == {".", "+", "-", "*"} and report["no_chromosome"] == 5 and report["dropped_overhang"] == 1
        assert ("chr1", -400, -300, "+", 1, 1, 0, 50) in rows and ("chr3", 120500, 120700, "+", 1, 1, 0, 50) in rows      # the intron table's first and last entry
        assert sum(1 for r in rows if r[0] == "chr3") == 39 + 1 + 1                                              # the 40-block read's junctions, one each of two more reads
    if min_overhang == 51:
        assert rows == [] or all(r[7] >= 51 for r in rows)


@pytest.mark.parametrize("grid", [1, 3])
def test_extract_strides_over_the_reads(gpu_ctx, tmp_path, monkeypatch, grid):
    """fewer workgroups than the file needs: every workgroup takes several stretches of reads (a 100 M-read file's shape)"""
    monkeypatch.setenv("LSQ_JN_EXTRACT_GRID", str(grid))
    lines = J.extract_lines()
    check_case(gpu_ctx, tmp_path, "stride", J.annotation_lines(), lines * 40 + J.reduce_case("max_position")[1] + lines)


def test_files_without_a_junction(gpu_ctx, tmp_path):
    iso = J.annotation_lines()
    for stem, lines, header in (("unspliced", [J.mrf_line("chr1", "+", [(150, 200)])] * 300, "AlignmentBlocks\n"), ("header_only", [], "AlignmentBlocks\n"), ("nothing", [], "")):
        interval, mrf, paths = J.write_case(str(tmp_path), stem, iso, lines, header)
        got = index_of(paths).device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
        assert len(got) == 0 and got.text() == ""
        assert got.report == {"reads": len(lines), "blocks": len(lines), "occurrences": 0, "dropped_overhang": 0, "no_chromosome": 0}


def test_an_annotation_without_any_intron(gpu_ctx, tmp_path):
    rows, _, _ = check_case(gpu_ctx, tmp_path, "mono", [J.interval_line("m.a", "chr1", "+", [(0, 1000)])], J.extract_lines())
    assert rows and {r[3] for r in rows} == {"."}


# ----------------------------------------------------------------------------- sort

SORT_COUNTS = sorted({0, 1, 2, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131073, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1})
_sort_want = {}


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("n_occ", SORT_COUNTS)
def test_sort_at_every_count(gpu_ctx, tmp_path, n_occ, shuffled):
    iso, lines = J.sort_case(n_occ, shuffled)
    if n_occ not in _sort_want:       # (the table does not depend on the file's order: one reference per count)
        _sort_want[n_occ] = J.table("".join(iso), "AlignmentBlocks\n" + "".join(lines))
    rows, report, _ = check_case(gpu_ctx, tmp_path, "sort", iso, lines, want=_sort_want[n_occ])
    assert report["occurrences"] == n_occ == sum(r[4] for r in rows) and len(rows) == n_occ
    if n_occ >= 63:
        # keys that differ in one field only: the chromosome's low and high byte, bit 0 and bit 30 of start and of end
        names = [r[:3] for r in rows]
        for key in (("c000", 200, 300), ("c255", 200, 300), ("c256", 200, 300), ("c300", 200, 300), ("c000", 201, 300), ("c000", 200, 301), ("c000", -200, 300),
                    ("c000", -200, -100), ("c000", -201, -100), ("c000", -200, -99), ("c000", 200 + (1 << 29), 300 + (1 << 29))):
            assert key in names


# ----------------------------------------------------------------------------- reduce

@pytest.mark.parametrize("kind", ["one_junction", "all_distinct", "run_lengths", "tile_edge", "max_position"])
def test_reduce_cases(gpu_ctx, tmp_path, kind):
    iso, lines = J.reduce_case(kind)
    rows, report, paths = check_case(gpu_ctx, tmp_path, kind, iso, lines)
    if kind == "one_junction":
        assert len(rows) == 1 and rows[0][4] == 70000 and 0 < rows[0][5] < 70000 and 0 < rows[0][6] < 70000 and rows[0][5] + rows[0][6] < 70000
    if kind == "all_distinct":
        assert len(rows) == 70000 and all(r[4] == 1 for r in rows)
    if kind == "run_lengths":
        assert [r[4] for r in rows[:10]] == [1, 2, 63, 64, 65, 1, 2, 63, 64, 65]
    if kind == "tile_edge":
        assert [r[4] for r in rows] == [SORT_TILE - 1, 70]
    if kind == "max_position":
        assert [r[7] for r in rows] == [900, 900, 900]
    if kind == "one_junction":      # the same from run to run
        ix = index_of(paths)
        a, b = ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
        assert a.rows() == b.rows() == rows


# ----------------------------------------------------------------------------- formats and options

@pytest.fixture(scope="module")
def formats(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jngpu"))
    reads = spliced_reads()
    interval, mrf, paths = J.write_case(d, "fmt", J.annotation_lines(), [J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads])
    sam = sam_of(reads).encode()
    paths["sam"] = os.path.join(d, "fmt.sam")
    open(paths["sam"], "wb").write(sam)
    for layout in ("htslib", "cut997", "cut61", "stored"):
        paths[layout] = os.path.join(d, "fmt_%s.bam" % layout)
        open(paths[layout], "wb").write(bam_writer.sam_to_bam(sam, layout))
    rows, report = J.table(interval, mrf)
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
    lone = ("chr1", 3100, 3200, "+", 1, 1, 0, 50)
    assert lone in rows
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
        want = [r for r in rows if r != lone]
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
    paths, _, _, _, _, _ = formats
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
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), formats[2], formats[3])


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
    assert p.returncode == 0 and p.stdout == table.text() == J.text(rows), p.stderr
    assert "junction(s)" in p.stderr
    h = tool(paths, paths["mrf"], opts=["--host"])
    assert h.returncode == 0 and h.stdout == p.stdout
    for opts, want in ((["--min-reads", "3"], table.text(3)), (["--novel"], table.text(0, True)), (["--min-reads", "2", "--novel"], table.text(2, True))):
        p = tool(paths, paths["mrf"], opts=opts)
        assert p.returncode == 0 and p.stdout == want and want != table.text()
    want = ix.device(ctx, "MRF_SINGLE", paths["mrf"], min_overhang=30).text()
    p = tool(paths, paths["sam"], "SAM_SINGLE", opts=["--min-overhang", "30"])
    assert p.returncode == 0 and p.stdout == want == J.text(J.table(interval, open(paths["mrf"]).read(), 30)[0]) and want != table.text()
    out = str(tmp_path / "out.tab")
    p = subprocess.run([os.path.join(BIN, "junctions"), "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "BAM_SINGLE", paths["cut61"], out],
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == table.text()
    ctx.close()
