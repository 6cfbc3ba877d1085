"""Per-base read depth on the device (lsq_cov_device: lsq_readfile.hip, lsq_cov.hip, lsq_sort.hpp, lsq_scan.hpp): every phase at the
smallest shapes at which it can go wrong, against the definition as tests/coverage_ref.py restates it and against lsq_cov_host.
All values are integers: the device tables equal both exactly.  Need an MI355X: python -m pytest tests -m gpu."""
import os
import subprocess

import pytest

import lesseq_amd as L
import bam_writer
import coverage_ref as V
from lesseq_amd.coverage import SORT_TILE
from test_coverage_host import index_of, same, tool as host_tool, BIN, LSQ_E_PARSE
from test_junctions_host import sam_of, spliced_reads
from test_sam_gpu import CHILD_TIMEOUT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def check_case(ctx, d, stem, iso, lines, strand=None, min_depth=1, want=None, header="AlignmentBlocks\n"):
    """the device tables and the host tables against the reference's (conservation included: `same`); returns (want, paths)"""
    interval, mrf, paths = V.write_case(str(d), stem, iso, lines, header)
    want = want or V.table(interval, mrf, strand, min_depth)
    ix = index_of(paths)
    dev = ix.device(ctx, "MRF_SINGLE", paths["mrf"], strand=strand, min_depth=min_depth)
    same(dev, want)
    same(ix.host("MRF_SINGLE", paths["mrf"], strand=strand, min_depth=min_depth), want)
    assert set(dev.times) == set(L.coverage.PHASES) and all(v >= 0 for v in dev.times.values())
    return want, paths


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None):
    return host_tool(paths, reads, fmt, opts, env, host=False, timeout=CHILD_TIMEOUT)


# ----------------------------------------------------------------------------- the definition

@pytest.mark.parametrize("strand", [None, "+", "-"])
def test_definition_cases(gpu_ctx, tmp_path, strand):
    (rows, regions, report), _ = check_case(gpu_ctx, tmp_path, "base", V.definition_annotation(), V.definition_lines(), strand)
    if strand is None:
        for r in (("chr1", 200, 340, 1), ("chr1", 1000, 1100, 1), ("chr1", 2000, 2050, 5), ("chr1", 4040, 4060, 2), ("chr1", -450, -400, 2), ("chr1", -20, 30, 1),
                  ("chrA", 450, 500, 2), ("chrB", 500, 520, 2)):
            assert r in rows
        assert [r[0] for r in rows if r[0] != "chr1"] == ["chr10"] * 3 + ["chr2"] * 5 + ["chrA"] * 2 + ["chrB"] * 2      # chr10 ahead of chr2: names, not indices
        assert report["no_chromosome"] == 3 and report["empty"] == 2
    else:
        assert report["other_strand"] > 5 and report["counted"] > 5


def test_files_without_a_counted_block(gpu_ctx, tmp_path):
    iso = V.definition_annotation()
    for stem, lines, header in (("header_only", [], "AlignmentBlocks\n"), ("nothing", [], ""), ("none_counted", [V.mrf_line("chrU", "+", [(1, 9)])] * 300, "AlignmentBlocks\n"),
                                ("wrong_strand", [V.mrf_line("chr1", "+", [(1, 9)])] * 300, "AlignmentBlocks\n")):
        (rows, regions, report), _ = check_case(gpu_ctx, tmp_path, stem, iso, lines, strand="-", header=header)
        assert rows == [] and report["reads"] == len(lines) and report["counted"] == 0 and len(regions) == 7 and all(r[4:] == (0, 0) for r in regions)


# ----------------------------------------------------------------------------- extract, sort

COUNTS = sorted({0, 1, 2, 31, 32, 33, 127, 128, 129, SORT_TILE // 2 - 1, SORT_TILE // 2, SORT_TILE // 2 + 1, 32767, 32768, 32769, 65537})
_count_want = {}


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("b", COUNTS)
def test_every_count_of_blocks(gpu_ctx, tmp_path, b, shuffled):
    """2 b records around a wave, a workgroup, the sort's tile and 2^16"""
    iso, lines = V.count_case(b, shuffled)
    if b not in _count_want:          # (the tables do not depend on the file's order: one reference per count)
        _count_want[b] = V.table("".join(iso), "AlignmentBlocks\n" + "".join(lines))
    (rows, _, report), _ = check_case(gpu_ctx, tmp_path, "count", iso, lines, want=_count_want[b])
    assert report["counted"] == b and report["no_chromosome"] == 1 and report["empty"] == 1 and (rows != []) == (b > 0)


@pytest.mark.parametrize("grid", [1, 3])
def test_extract_strides_over_the_reads(gpu_ctx, tmp_path, monkeypatch, grid):
    """fewer workgroups than the file needs: every workgroup takes several stretches of reads (a 100 M-read file's shape)"""
    monkeypatch.setenv("LSQ_COV_EXTRACT_GRID", str(grid))
    iso, lines = V.count_case(5000, True)
    (_, _, report), _ = check_case(gpu_ctx, tmp_path, "stride", iso, lines, strand="+")
    assert report["reads"] > 4 * 3 * 256 and report["other_strand"] > 1000


# ----------------------------------------------------------------------------- reduce, scan, emit

@pytest.mark.parametrize("kind", ["identical", "disjoint", "chain", "staircase", "run_lengths", "tile_edge"])
def test_shape_cases(gpu_ctx, tmp_path, kind):
    iso, lines = V.shape_case(kind, SORT_TILE)
    (rows, regions, report), paths = check_case(gpu_ctx, tmp_path, kind, iso, lines)
    if kind == "identical":
        assert rows == [("chr1", 1000, 1100, 70000)]
    if kind == "disjoint":
        assert len(rows) == 70000 and all(r[3] == 1 for r in rows)
    if kind == "chain":
        assert rows == [("chr1", 0, 15 * 70000, 1)]
    if kind == "staircase":
        assert [r[3] for r in rows] == list(range(1, 301)) + list(range(300, 0, -1))
    if kind == "run_lengths":
        assert [r[3] for r in rows[:10]] == [1, 2, 63, 64, 65, 1, 2, 63, 64, 65]
    if kind == "tile_edge":
        assert rows == [("chr1", 100, 150, SORT_TILE), ("chr1", 150, 200, SORT_TILE + 70), ("chr1", 200, 300, 70)]
    if kind == "identical":         # the same from run to run
        ix = index_of(paths)
        a, b = ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
        assert a.rows() == b.rows() == rows and a.regions() == b.regions() == regions


# ----------------------------------------------------------------------------- regions

@pytest.mark.parametrize("min_depth", [1, 2, 4])
def test_regions(gpu_ctx, tmp_path, min_depth):
    iso, lines = V.regions_case()
    (rows, regions, _), _ = check_case(gpu_ctx, tmp_path, "regions", iso, lines, min_depth=min_depth)
    assert len(regions) > 4096 and len(rows) == 4
    if min_depth == 2:
        assert regions[:4] == [("inside.a", "chr1", "+", 30, 30, 60), ("on_edges.a", "chr1", "+", 50, 50, 150), ("all_rows.a", "chr1", "-", 150, 100, 300),
                               ("across_gap.a", "chr1", "+", 270, 20, 160)]
        assert regions[7] == ("union.a", "chr1", "+", 160, 100, 290) and regions[9][3:] == (0, 0, 0)
    if min_depth == 4:                # above the largest depth
        assert all(r[4] == 0 for r in regions) and any(r[5] for r in regions)


def test_a_depth_sum_past_32_bits(gpu_ctx, tmp_path):
    iso, lines = V.deep_case()
    (rows, regions, report), _ = check_case(gpu_ctx, tmp_path, "deep", iso, lines)
    assert rows == [("chr1", 0, 100000, 70000)] and regions[0][5] == 7000000000 == report["bases"] and regions[1][4:] == (50000, 3500000000)


# ----------------------------------------------------------------------------- formats and options

@pytest.fixture(scope="module")
def formats(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("covgpu"))
    reads = spliced_reads()
    iso = V.definition_annotation() + [V.interval_line("junc.a", "chr1", "+", [(150, 200), (300, 350), (500, 530)])]
    interval, mrf, paths = V.write_case(d, "fmt", iso, [V.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads])
    sam = sam_of(reads, mapq={0: 3, 7: 3}).encode()
    paths["sam"] = os.path.join(d, "fmt.sam")
    open(paths["sam"], "wb").write(sam)
    for layout in ("htslib", "cut61"):
        paths[layout] = os.path.join(d, "fmt_%s.bam" % layout)
        open(paths[layout], "wb").write(bam_writer.sam_to_bam(sam, layout))
    fewer = V.table(interval, L.sam_to_mrf(sam, min_mapq=4).decode())
    return paths, V.table(interval, mrf), fewer, interval, mrf


def test_one_table_from_mrf_sam_and_bam(gpu_ctx, formats):
    paths, want, fewer, interval, mrf = formats
    ix = index_of(paths)
    for fmt, key in (("MRF_SINGLE", "mrf"), ("SAM_SINGLE", "sam"), ("BAM_SINGLE", "htslib"), ("BAM_SINGLE", "cut61")):
        same(ix.device(gpu_ctx, fmt, paths[key]), want)
        same(ix.host(fmt, paths[key]), want)
    minus = V.table(interval, mrf, "-")
    same(ix.device(gpu_ctx, "BAM_SINGLE", paths["cut61"], strand="-"), minus)
    assert fewer != want and fewer[2]["reads"] == want[2]["reads"] - 2
    ctx = L.Context(0)
    ctx.set_option("sam_min_mapq", 4)
    for fmt, key in (("SAM_SINGLE", "sam"), ("BAM_SINGLE", "htslib")):
        same(ix.device(ctx, fmt, paths[key]), fewer)
        same(ix.host(fmt, paths[key], min_mapq=4), fewer)
        p = tool(paths, paths[key], fmt, env={"LSQ_SAM_MIN_MAPQ": "4"})
        assert p.returncode == 0 and p.stdout == V.text(fewer[0]), p.stderr
    ctx.close()
    for fmt in ("UCSC_GFF", "MRF_PAIRED"):
        with pytest.raises(L.LsqError) as e:
            ix.device(gpu_ctx, fmt, paths["mrf"])
        assert e.value.status == -3 and str(e.value).endswith("Unknown file format error: " + fmt)


# ----------------------------------------------------------------------------- context

def test_a_context_with_events_and_counted_reads_is_left_as_it_was(formats):
    from test_sam_gpu import count_table
    paths, want, _, _, _ = formats
    d = os.path.join(GOLD, "toy")
    ix = index_of(paths)
    ev = L.Events(L.Annotation(os.path.join(d, "toy.interval"), os.path.join(d, "toy.map"), 0, 10), ("SHORT_READ",), (50,))
    ctx = L.Context(0)
    ctx.upload_events(ev)
    ctx.upload_reads_mrf(0, os.path.join(d, "toy.mrf"))
    before = count_table(ctx, ev)
    assert before == open(os.path.join(d, "count.out")).read()
    a = ix.device(ctx, "MRF_SINGLE", paths["mrf"])
    same(a, want)
    assert count_table(ctx, ev) == before
    b = ix.device(ctx, "SAM_SINGLE", paths["sam"])
    assert a.rows() == b.rows() and a.regions() == b.regions()       # two calls, the same tables
    ctx.upload_reads_mrf(0, os.path.join(d, "toy.mrf"))                # the events' dictionaries still serve an upload
    assert count_table(ctx, ev) == before
    ctx.close()


# ----------------------------------------------------------------------------- executable

def test_the_executable(formats, tmp_path):
    paths, want, _, interval, mrf = formats
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == V.text(want[0]), p.stderr
    assert "solve's total_read_bases" in p.stderr and "%d base(s)" % want[2]["bases"] in p.stderr
    h = host_tool(paths, paths["mrf"])
    assert h.returncode == 0 and h.stdout == p.stdout
    regions, hregions = str(tmp_path / "dev.tsv"), str(tmp_path / "host.tsv")
    two = V.table(interval, mrf, "+", 2)
    p = tool(paths, paths["sam"], "SAM_SINGLE", opts=["--strand", "+", "--min-depth", "2", "--regions", regions])
    h = host_tool(paths, paths["sam"], "SAM_SINGLE", opts=["--strand", "+", "--min-depth", "2", "--regions", hregions])
    assert p.returncode == 0 and h.returncode == 0 and p.stdout == h.stdout == V.text(two[0], 2) and p.stdout not in ("", V.text(want[0]))
    assert open(regions).read() == open(hregions).read() == V.regions_text(two[1])
    out = str(tmp_path / "out.bedgraph")
    p = subprocess.run([os.path.join(BIN, "coverage"), "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "BAM_SINGLE", paths["cut61"], out],
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == V.text(want[0])


def test_a_malformed_record_gives_counts_status_and_message(gpu_ctx, formats, tmp_path):
    paths, want, _, _, _ = formats
    ix = index_of(paths)
    sam = "@HD\tVN:1.6\n" + "q\t0\tchr1\t101\t60\t50M10N50M\t*\t0\t0\t*\t*\n" * 7 + "q\t0\tchr1\t101\t60\t50Q\t*\t0\t0\t*\t*\n"
    spath = str(tmp_path / "bad.sam")
    open(spath, "w").write(sam)
    with pytest.raises(L.LsqError) as host:
        ix.host("SAM_SINGLE", spath)
    with pytest.raises(L.LsqError) as e:
        ix.device(gpu_ctx, "SAM_SINGLE", spath)
    assert e.value.status == LSQ_E_PARSE and str(e.value) == str(host.value)
    regions = str(tmp_path / "never.tsv")
    p = tool(paths, spath, "SAM_SINGLE", opts=["--regions", regions])
    assert p.returncode == 1 and p.stdout == "" and "#9:q\t0\tchr1\t101\t60\t50Q" in p.stderr and "Lexical_cast error" in p.stderr and not os.path.exists(regions)
    h = host_tool(paths, spath, "SAM_SINGLE")

    def said(err):
        return [ln.split("] ", 1)[-1] for ln in err.split("\n") if "#9:q" in ln or "Lexical_cast" in ln]
    assert h.returncode == 1 and h.stdout == "" and said(h.stderr) == said(p.stderr) and len(said(p.stderr)) == 2
    # the context is as good as before
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), want)
