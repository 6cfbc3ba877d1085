"""Intron retention on the device (lsq_ir_device: lsq_readfile.hip, lsq_sites.hip, lsq_cov.hip, lsq_retention.hip): the selection at
the smallest shapes at which each part can go wrong, against the definition as tests/retention_ref.py restates it and against
lsq_ir_host.  All values are integers: the device table equals both exactly, in rows, report and text.  Need an MI355X: python -m
pytest tests -m gpu."""
import os
import subprocess

import pytest

import lesseq_amd as L
import bam_writer
import coverage_ref as V
import junction_ref as J
import retention_ref as R
from test_junctions_host import sam_of, BIN, LSQ_E_PARSE
from test_retention_host import index_of
from test_sites_host import format_reads
from test_sam_gpu import CHILD_TIMEOUT

pytestmark = pytest.mark.gpu


def same(got, rows, report):
    assert got.rows() == rows
    assert got.report == report
    assert got.text() == R.text(rows)
    assert got.text(ratios=True) == R.text(rows, ratios=True)


def check_case(ctx, d, stem, iso, lines, min_overhang=1, key=None):
    """the device table and the host table against the reference's (key: computed once a session); returns (rows, report, paths)"""
    interval, mrf, paths = R.write_case(str(d), stem, iso, lines)
    rows, report = R.table_once(key, interval, mrf, min_overhang) if key else R.table(interval, mrf, min_overhang)
    ix = index_of(paths)
    dev = ix.device(ctx, "MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(dev, rows, report)
    host = ix.host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(host, rows, report)
    assert dev.text(True) == host.text(True)
    assert set(dev.times) == set(L.retention.PHASES) and all(v >= 0 for v in dev.times.values())
    return rows, report, paths


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None):
    argv = [os.path.join(BIN, "retention")] + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads]
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=CHILD_TIMEOUT)


# ----------------------------------------------------------------------------- the table by hand, geometry, ranks

def test_the_table_worked_out_by_hand(gpu_ctx, tmp_path):
    iso, lines, rows, report = R.rows_case()
    got = check_case(gpu_ctx, tmp_path, "rows", iso, lines)
    assert got[0] == rows and got[1] == report
    ix = index_of(got[2])
    assert ix.device(gpu_ctx, "MRF_SINGLE", got[2]["mrf"]).text(ratios=True) == R.RATIO_TEXT


def test_a_piece_against_the_rows_in_every_way(gpu_ctx, tmp_path):
    """a row that begins before the piece and ends inside it, one that begins inside and ends behind, one over the whole intron and
    beyond, row edges on the piece's edges, gaps at the ends and in the middle, two and three pieces, no clean base, a nested intron,
    an untouched one, exons that abut the intron's ends from inside"""
    iso, lines = R.geometry_case()
    rows, report, _ = check_case(gpu_ctx, tmp_path, "geometry", iso, lines, key="geometry_case")
    by = {r[1:3]: r[9:] for r in rows}
    assert by[(1100, 1200)] == (100, 50, 50, 0, 0, 1) and by[(2100, 2200)] == (100, 50, 50, 0, 0, 1) and by[(3100, 3200)] == (100, 100, 100, 1, 1, 1)
    assert by[(4100, 4200)] == (100, 100, 150, 1, 1, 2) and by[(5100, 5200)] == (100, 60, 70, 0, 1, 1)
    assert by[(8100, 8200)] == (0, 0, 0, 0, 0, 0) and by[(10100, 10200)] == (100, 0, 0, 0, 0, 0) and report["no_clean"] == 1 and report["pieces"] == 17
    assert by[(6100, 6400)][0] == 250 and by[(7100, 7500)][0] == 300 and by[(9100, 9900)][0] == 600 and by[(9300, 9400)][0] == 100


def test_every_rank(gpu_ctx, tmp_path):
    """n = 1 .. 9 under a staircase 1 .. n, ties at the rank, a rank among the zeros, all bases at one depth, a largest depth of 1"""
    iso, lines = R.rank_case()
    rows, _, _ = check_case(gpu_ctx, tmp_path, "ranks", iso, lines, key="ranks")
    by = {r[1]: r[9:] for r in rows}
    for n in range(1, 10):
        assert by[1000 * n] == (n, n, n * (n + 1) // 2, (n + 3) // 4, (2 * n + 3) // 4, (3 * n + 3) // 4)
    for start, want in R.RANK_ROWS.items():
        assert by[start] == want


# ----------------------------------------------------------------------------- strides, depth range, grid

def test_rows_around_the_waves_width(gpu_ctx, tmp_path):
    """63, 64, 65, 127, 128 and 129 depth rows inside one intron: a lane's last round with one row, with none"""
    iso, lines = R.stride_case()
    rows, _, _ = check_case(gpu_ctx, tmp_path, "stride", iso, lines, key="stride_case")
    assert [r[10] for r in rows] == [63, 64, 65, 127, 128, 129] and all(r[12:] == (0, 0, 2) for r in rows)


def test_a_depth_above_16_bits_and_a_sum_above_32(gpu_ctx, tmp_path):
    iso, lines = R.deep_case()
    rows, report, _ = check_case(gpu_ctx, tmp_path, "deep", iso, lines, key="deep_case")
    assert rows == [("chr1", 200, 100200, "+", 0, 0, 0, 0, 0, 100000, 100000, 7000000000, 70000, 70000, 70000)] and report["depth_rows"] == 1


def test_a_largest_depth_of_one(gpu_ctx, tmp_path):
    """the bisection's shortest run: [0, 1]"""
    iso = [J.interval_line("g.a", "chr1", "+", [(100, 200), (300, 400)])]
    rows, _, _ = check_case(gpu_ctx, tmp_path, "one", iso, [J.mrf_line("chr1", "+", [(230, 290)])])
    assert rows == [("chr1", 200, 300, "+", 0, 0, 0, 0, 0, 100, 60, 60, 0, 1, 1)]


@pytest.mark.parametrize("grid", [1, 3, None])
def test_the_selection_strides_over_70000_introns(gpu_ctx, tmp_path, monkeypatch, grid):
    """fewer workgroups than the introns need: every wave takes several rounds"""
    if grid:
        monkeypatch.setenv("LSQ_IR_GRID", str(grid))
    iso, lines = R.grid_case()
    rows, report, _ = check_case(gpu_ctx, tmp_path, "grid", iso, lines, key="grid_case")
    assert len(rows) == 70000 == report["pieces"] and len({r[12:] for r in rows}) > 4


# ----------------------------------------------------------------------------- chromosomes, stability

def test_chromosomes(gpu_ctx, tmp_path):
    """the dictionary's order against the names'; neighbours in the dictionary whose rows and introns meet at one coordinate; a
    chromosome without reads; reads on a chromosome the annotation does not name; negative coordinates and an intron across 0"""
    iso, lines = R.chromosome_case()
    rows, report, paths = check_case(gpu_ctx, tmp_path, "chroms", iso, lines, key="chromosome_case")
    assert [r[0] for r in rows] == ["chr1", "chr1", "chr10", "chr2", "chr9", "chrA", "chrB"] and index_of(paths).chrom_names() == ["chr2", "chr10", "chr1", "chrA", "chrB", "chr9"]
    by = {(r[0], r[1], r[2]): r[9:] for r in rows}
    assert by[("chrB", 500, 600)] == (100, 60, 60, 0, 1, 1) and by[("chr9", 200, 300)] == (100, 0, 0, 0, 0, 0) and by[("chr1", -300, 100)][:3] == (400, 50, 65)
    assert report["no_chromosome"] == 1 and report["depth_rows"] > 8


@pytest.mark.parametrize("case", ["geometry_case", "stride_case", "grid_case"])
def test_a_shuffled_file_and_a_second_call_give_the_same_table(gpu_ctx, tmp_path, case):
    iso, lines = getattr(R, case)()
    interval, mrf, paths = R.write_case(str(tmp_path), case, iso, lines)
    rows, report = R.table_once(case, interval, mrf)
    _, _, other = R.write_case(str(tmp_path), case + "_shuffled", iso, R.shuffled(lines))
    ix = index_of(other)
    a, b = ix.device(gpu_ctx, "MRF_SINGLE", other["mrf"]), ix.device(gpu_ctx, "MRF_SINGLE", other["mrf"])
    same(a, rows, report)
    same(b, rows, report)
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), rows, report)


def test_degenerate_files(gpu_ctx, tmp_path):
    iso = R.rows_case()[0]
    for stem, lines, header in (("header_only", [], "AlignmentBlocks\n"), ("nothing", [], ""), ("no_counted_block", [J.mrf_line("chrU", "+", [(100, 200)])], "AlignmentBlocks\n")):
        interval, mrf, paths = J.write_case(str(tmp_path), stem, iso, lines, header)
        rows, report = R.table(interval, mrf)
        ix = index_of(paths)
        same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), rows, report)
        same(ix.host("MRF_SINGLE", paths["mrf"]), rows, report)
        assert len(rows) == 4 and report["depth_rows"] == 0 and all(r[10:] == (0, 0, 0, 0, 0) for r in rows)
    mono = [J.interval_line("m.a", "chr1", "+", [(0, 1000)])]
    interval, mrf, paths = J.write_case(str(tmp_path), "mono", mono, R.rows_case()[1])
    got = index_of(paths).device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    assert got.rows() == [] and got.text() == "" and got.report == R.table(interval, mrf)[1]


# ----------------------------------------------------------------------------- formats and processes

@pytest.fixture(scope="module")
def formats(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("irgpu"))
    reads = format_reads()
    interval, mrf, paths = R.write_case(d, "fmt", J.annotation_lines(), [J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads])
    sam = sam_of(reads).encode()
    paths["sam"] = os.path.join(d, "fmt.sam")
    open(paths["sam"], "wb").write(sam)
    for layout in ("htslib", "cut61"):
        paths[layout] = os.path.join(d, "fmt_%s.bam" % layout)
        open(paths[layout], "wb").write(bam_writer.sam_to_bam(sam, layout))
    rows, report = R.table_once("fmt", interval, mrf)
    return paths, reads, rows, report, interval, d


def test_one_table_from_mrf_sam_and_bam(gpu_ctx, formats):
    paths, _, rows, report, _, _ = formats
    ix = index_of(paths)
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), rows, report)
    same(ix.device(gpu_ctx, "SAM_SINGLE", paths["sam"]), rows, report)
    for layout in ("htslib", "cut61"):
        same(ix.device(gpu_ctx, "BAM_SINGLE", paths[layout]), rows, report)
    for fmt in ("UCSC_GFF", "MRF_PAIRED"):
        with pytest.raises(L.LsqError) as e:
            ix.device(gpu_ctx, fmt, paths["mrf"])
        assert e.value.status == -3 and str(e.value).endswith("Unknown file format error: " + fmt)


@pytest.mark.parametrize("min_overhang", [0, 10, 51])
def test_min_overhang_is_sites(gpu_ctx, formats, min_overhang):
    paths, _, at_one, _, interval, _ = formats
    rows, report = R.table_once("fmt", interval, open(paths["mrf"]).read(), min_overhang)
    same(index_of(paths).device(gpu_ctx, "MRF_SINGLE", paths["mrf"], min_overhang=min_overhang), rows, report)
    assert [r[9:] for r in rows] == [r[9:] for r in at_one]


def test_the_contexts_filters_are_respected(formats):
    paths, reads, rows, _, interval, d = formats
    last = len(reads) - 1                   # the only block through 3100: (3080, 3120), twenty bases of the intron (3100, 3200)
    want = R.table(interval, "AlignmentBlocks\n" + "".join(J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads[:-1]))[0]
    assert want != rows
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
        ctx.close()
    p = tool(paths, os.path.join(d, "mapq.sam"), "SAM_SINGLE", env={"LSQ_SAM_MIN_MAPQ": "4"})
    assert p.returncode == 0 and p.stdout == R.text(want)


def test_the_executable(formats, tmp_path):
    paths, _, rows, _, interval, _ = formats
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == R.text(rows), p.stderr
    assert "depth row(s)" in p.stderr
    h = tool(paths, paths["mrf"], opts=["--host"])
    assert h.returncode == 0 and h.stdout == p.stdout
    p = tool(paths, paths["sam"], "SAM_SINGLE", opts=["--ratios"])
    h = tool(paths, paths["sam"], "SAM_SINGLE", opts=["--host", "--ratios"])
    assert p.returncode == 0 and p.stdout == h.stdout == R.text(rows, ratios=True) and "NA" in p.stdout
    want = R.text(R.table_once("fmt", interval, open(paths["mrf"]).read(), 10)[0])
    p = tool(paths, paths["htslib"], "BAM_SINGLE", opts=["--min-overhang", "10"])
    assert p.returncode == 0 and p.stdout == want != R.text(rows)
    p = tool(paths, paths["mrf"], opts=["--nonsense"])
    assert p.returncode == 1 and p.stdout == "" and "Usage:\nretention " in p.stderr
    out = str(tmp_path / "out.tab")
    p = subprocess.run([os.path.join(BIN, "retention"), "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "BAM_SINGLE", paths["cut61"], out],
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == R.text(rows)


def test_malformed_records_give_counts_status_and_message(gpu_ctx, formats, tmp_path):
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
    p = tool(paths, spath, "SAM_SINGLE")
    assert p.returncode == 1 and p.stdout == ""
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), rows, report)      # the context is as good as before


# ----------------------------------------------------------------------------- cross-checks against what exists

def test_columns_1_to_9_are_the_sites_tables(gpu_ctx, formats):
    paths, _, rows, report, _, _ = formats
    sites = L.SiteIndex(L.Annotation(paths["interval"], paths["map"])).device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    got = index_of(paths).device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    assert [r[:9] for r in got.rows()] == [r for r in sites.rows() if r[3] != "."] and len(got) < len(sites)
    assert {k: got.report[k] for k in L.sites.REPORT} == sites.report


@pytest.mark.parametrize("case", ["geometry_case", "chromosome_case"])
def test_covered_and_depth_sum_are_coverages_region_sums_over_the_pieces(gpu_ctx, tmp_path, case):
    iso, lines = getattr(R, case)()
    interval, mrf, paths = R.write_case(str(tmp_path), case, iso, lines)
    got = index_of(paths).device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    piece_lines, of_row = R.pieces_annotation(interval)
    _, _, ppaths = R.write_case(str(tmp_path), case + "_pieces", piece_lines, lines)
    cov = L.CoverageIndex(L.Annotation(ppaths["interval"], ppaths["map"])).device(gpu_ctx, "MRF_SINGLE", ppaths["mrf"])
    regions = cov.regions()
    assert len(of_row) == len(got) and sum(len(m) for m in of_row) == got.report["pieces"] == len(regions)
    for row, mine in zip(got.rows(), of_row):
        assert row[9] == sum(regions[k][3] for k in mine) and row[10] == sum(regions[k][4] for k in mine) and row[11] == sum(regions[k][5] for k in mine)
    assert any(len(m) == 3 for m in of_row) or case != "geometry_case"


def test_coverage_is_what_it_was_before_and_after_a_retention_call(gpu_ctx, tmp_path):
    interval, mrf, paths = V.write_case(str(tmp_path), "cov", V.definition_annotation(), V.definition_lines())
    rows, regions, report = V.table(interval, mrf)
    cov = L.CoverageIndex(L.Annotation(paths["interval"], paths["map"]))

    def check():
        got = cov.device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
        assert got.rows() == rows and got.regions() == regions and got.report == report
        assert got.text() == V.text(rows) and got.regions_text() == V.regions_text(regions)
        assert set(got.times) == set(L.coverage.PHASES)
    check()
    iso, lines = R.geometry_case()
    _, _, other = R.write_case(str(tmp_path), "ir", iso, lines)
    index_of(other).device(gpu_ctx, "MRF_SINGLE", other["mrf"])
    index_of(paths).device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    check()
