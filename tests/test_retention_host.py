"""Intron retention without a GPU (include/lesseq_hip.h, lsq_ir_*): the reference against a table worked out by hand, lsq_ir_host and
`retention --host` against the definition as tests/retention_ref.py restates it."""
import os
import subprocess

import pytest

import lesseq_amd as L
import bam_writer
import junction_ref as J
import retention_ref as R
from test_junctions_host import log_messages, sam_of, BIN, LSQ_E_PARSE
from test_sites_host import format_reads

HERE = os.path.dirname(os.path.abspath(__file__))
USAGE = "Usage:\nretention [--host] [--ratios] [--min-overhang N] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]"


def index_of(paths):
    return L.RetentionIndex(L.Annotation(paths["interval"], paths["map"]))


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None):
    argv = [os.path.join(BIN, "retention"), "--host"] + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads]
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})))


def same(got, rows, report):
    assert got.rows() == rows
    assert got.report == report
    assert got.text() == R.text(rows)
    assert got.text(ratios=True) == R.text(rows, ratios=True)


# ----------------------------------------------------------------------------- the definition

def test_the_table_worked_out_by_hand(tmp_path):
    iso, lines, rows, report = R.rows_case()
    interval, mrf, paths = R.write_case(str(tmp_path), "rows", iso, lines)
    assert R.table(interval, mrf) == (rows, report)
    assert R.text(rows, ratios=True) == R.RATIO_TEXT and "".join(ln.rsplit("\t", 3)[0] + "\n" for ln in R.RATIO_TEXT.splitlines()) == R.text(rows)
    ix = index_of(paths)
    assert ix.num_introns == 4 and ix.chrom_names() == ["chr1"]
    got = ix.host("MRF_SINGLE", paths["mrf"])
    same(got, rows, report)
    assert got.text(ratios=True) == R.RATIO_TEXT
    assert got.times == dict.fromkeys(L.retention.PHASES, 0.0)
    p = tool(paths, paths["mrf"], opts=["--ratios"])
    assert p.returncode == 0 and p.stdout == R.RATIO_TEXT
    line = ("retention: 11 read(s), 14 block(s), 3 occurrence(s) of junctions; 0 block pair(s) below the overhang, 0 with a block on no chromosome of the annotation; "
            "9 boundary(ies), 7 block(s) through one, 3 sites row(s) without a spliced read; 4 intron(s), 1 without a clean base, 4 piece(s); "
            "14 depth row(s), 1176 base(s) in the counted blocks")
    assert log_messages(p.stderr) == [("WARNING", line)]


def test_ranks_by_hand(tmp_path):
    """n = 1 .. 9 under a staircase 1 .. n: column q is the value (q n + 3) div 4 itself; ties, zeros, one depth, largest depth 1"""
    iso, lines = R.rank_case()
    interval, mrf, paths = R.write_case(str(tmp_path), "ranks", iso, lines)
    rows, report = R.table_once("ranks", interval, mrf)
    by = {r[1]: r[9:] for r in rows}
    for n in range(1, 10):
        assert by[1000 * n] == (n, n, n * (n + 1) // 2, (n + 3) // 4, (2 * n + 3) // 4, (3 * n + 3) // 4)
    assert {(q * n + 3) // 4 for n in range(1, 10) for q in (1, 2, 3)} == set(range(1, 8))
    for start, want in R.RANK_ROWS.items():
        assert by[start] == want
    same(index_of(paths).host("MRF_SINGLE", paths["mrf"]), rows, report)


@pytest.mark.parametrize("case", ["geometry_case", "stride_case", "chromosome_case", "deep_case", "grid_case"])
def test_the_host_path_against_the_reference(tmp_path, case):
    iso, lines = getattr(R, case)()
    interval, mrf, paths = R.write_case(str(tmp_path), case, iso, lines)
    rows, report = R.table_once(case, interval, mrf)
    ix = index_of(paths)
    same(ix.host("MRF_SINGLE", paths["mrf"]), rows, report)
    if case == "geometry_case":
        by = {r[1:3]: r[9:] for r in rows}
        assert by[(1100, 1200)] == (100, 50, 50, 0, 0, 1) and by[(2100, 2200)] == (100, 50, 50, 0, 0, 1) and by[(3100, 3200)] == (100, 100, 100, 1, 1, 1)
        assert by[(4100, 4200)] == (100, 100, 150, 1, 1, 2) and by[(5100, 5200)] == (100, 60, 70, 0, 1, 1)
        assert by[(6100, 6400)][0] == 250 and by[(7100, 7500)][0] == 300 and by[(8100, 8200)] == (0, 0, 0, 0, 0, 0) and by[(10100, 10200)] == (100, 0, 0, 0, 0, 0)
        assert by[(9100, 9900)][0] == 600 and by[(9300, 9400)][0] == 100 and by[(11100, 11200)][0] == 40
        assert report["no_clean"] == 1 and report["pieces"] == 1 * 5 + 2 + 3 + 1 + 0 + 3 + 1 + 1 + 1
    if case == "stride_case":
        assert [r[10] for r in rows] == [63, 64, 65, 127, 128, 129] and all(r[12:] == (0, 0, 2) for r in rows)      # a third of the rows each at depth 1, 2, 3; rank 3n/4 falls among the twos
    if case == "chromosome_case":
        assert [r[0] for r in rows] == ["chr1", "chr1", "chr10", "chr2", "chr9", "chrA", "chrB"] and ix.chrom_names() == ["chr2", "chr10", "chr1", "chrA", "chrB", "chr9"]
        by = {(r[0], r[1], r[2]): r[9:] for r in rows}
        assert by[("chrB", 500, 600)] == (100, 60, 60, 0, 1, 1) and by[("chr9", 200, 300)] == (100, 0, 0, 0, 0, 0) and by[("chr1", -300, 100)][:3] == (400, 50, 65)
    if case == "deep_case":
        assert rows == [("chr1", 200, 100200, "+", 0, 0, 0, 0, 0, 100000, 100000, 7000000000, 70000, 70000, 70000)]
    if case == "grid_case":
        assert len(rows) == 70000 and report["no_clean"] == 0 and report["pieces"] == 70000 and len({r[12:] for r in rows}) > 4
        for n_threads in (1, 5):
            same(ix.host_reads(ix.parse_host("MRF_SINGLE", paths["mrf"]), n_threads=n_threads), rows, report)


@pytest.mark.parametrize("min_overhang", [0, 1, 10, 51])
def test_min_overhang_is_sites_and_leaves_the_depth_alone(tmp_path, min_overhang):
    lines = [J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in format_reads()]      # first blocks of 1 .. 50 bases, second ones of 10 .. 49
    interval, mrf, paths = R.write_case(str(tmp_path), "fmt", J.annotation_lines(), lines)
    rows, report = R.table_once("fmt", interval, mrf, min_overhang)
    at_one = R.table_once("fmt", interval, mrf, 1)[0]
    ix = index_of(paths)
    got = ix.host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(got, rows, report)
    sites = L.SiteIndex(L.Annotation(paths["interval"], paths["map"])).host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    assert [r[:9] for r in rows] == [r for r in sites.rows() if r[3] != "."] and {k: got.report[k] for k in L.sites.REPORT} == sites.report
    assert [r[9:] for r in rows] == [r[9:] for r in at_one] and ([r[:9] for r in rows] != [r[:9] for r in at_one]) == (min_overhang > 1)
    p = tool(paths, paths["mrf"], opts=["--min-overhang", str(min_overhang)])
    assert p.returncode == 0 and p.stdout == R.text(rows)


def test_degenerate_files(tmp_path):
    iso = J.annotation_lines()
    for stem, lines, header in (("unspliced", [J.mrf_line("chr1", "+", [(150, 250)])] * 5, "AlignmentBlocks\n"), ("header_only", [], "AlignmentBlocks\n"), ("nothing", [], "")):
        interval, mrf, paths = R.write_case(str(tmp_path), stem, iso, lines, header)
        rows, report = R.table(interval, mrf)
        same(index_of(paths).host("MRF_SINGLE", paths["mrf"]), rows, report)
        assert len(rows) == report["introns"] > 0 and report["depth_rows"] == (1 if lines else 0)
        p = tool(paths, paths["mrf"])
        assert p.returncode == 0 and p.stdout == R.text(rows)
    mono = [J.interval_line("m.a", "chr1", "+", [(0, 1000)])]
    interval, mrf, paths = R.write_case(str(tmp_path), "mono", mono, J.extract_lines())
    got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
    assert got.rows() == [] and got.text() == "" and got.report["introns"] == 0 and got.report["occurrences"] > 0      # novel junctions make no row


# ----------------------------------------------------------------------------- formats

@pytest.fixture(scope="module")
def three_formats(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ir3"))
    reads = format_reads()
    interval, mrf, paths = R.write_case(d, "fmt", J.annotation_lines(), [J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads])
    sam = sam_of(reads).encode()
    paths["sam"] = os.path.join(d, "fmt.sam")
    open(paths["sam"], "wb").write(sam)
    paths["bam"] = os.path.join(d, "fmt.bam")
    open(paths["bam"], "wb").write(bam_writer.sam_to_bam(sam, "cut61"))
    return interval, mrf, paths, reads


def test_one_table_from_mrf_sam_and_bam(three_formats):
    interval, mrf, paths, _ = three_formats
    rows, report = R.table_once("fmt", interval, mrf)
    ix = index_of(paths)
    same(ix.host("MRF_SINGLE", paths["mrf"]), rows, report)
    same(ix.host("SAM_SINGLE", paths["sam"]), rows, report)
    same(ix.host("BAM_SINGLE", paths["bam"]), rows, report)
    p = tool(paths, paths["bam"], "BAM_SINGLE", opts=["--ratios"])
    assert p.returncode == 0 and p.stdout == R.text(rows, ratios=True) and "NA" in p.stdout
    assert report["through"] > 10 and any(r[11] > 0 for r in rows)


def test_the_environments_filters_are_respected(three_formats, tmp_path):
    interval, mrf, paths, reads = three_formats
    rows, _ = R.table_once("fmt", interval, mrf)
    last = len(reads) - 1                   # the only block through 3100: (3080, 3120), twenty bases of the intron (3100, 3200)
    at = [i for i, r in enumerate(rows) if r[:3] == ("chr1", 3100, 3200)][0]
    assert rows[at][6] == 1 and rows[at][10] == 20
    want = R.table(interval, "AlignmentBlocks\n" + "".join(J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads[:-1]))[0]
    assert want[at][6] == 0 and want[at][10] == 0
    ix = index_of(paths)
    for name, kw, env in (("mapq", dict(mapq={last: 3}), {"LSQ_SAM_MIN_MAPQ": "4"}), ("flag", dict(flags={last: 0x400}), {"LSQ_SAM_SKIP_FLAGS": str(0x904 | 0x400)})):
        path = str(tmp_path / (name + ".sam"))
        open(path, "wb").write(sam_of(reads, **kw).encode())
        opts = dict(min_mapq=4) if name == "mapq" else dict(skip_flags=0x904 | 0x400)
        assert ix.host("SAM_SINGLE", path).rows() == rows
        assert ix.host("SAM_SINGLE", path, **opts).rows() == want
        p = tool(paths, path, "SAM_SINGLE", env=env)
        assert p.returncode == 0 and p.stdout == R.text(want)


def test_name_keyed_lines_count_as_blocks(tmp_path):
    """UCSC_GFF: the lines of one name are one read's blocks; two overlapping lines of one name both count in the depth"""
    iso, _, _, _ = R.rows_case()
    interval, _, paths = R.write_case(str(tmp_path), "gff", iso, [])
    reads = [("n1", "chr1", "+", [(150, 200), (300, 350)]), ("n2", "chr1", "+", [(180, 320), (190, 330)]), ("n3", "chr1", "+", [(1050, 1250)])]
    lines = ["track name=x\n", "browser position chr1\n"]
    for n, c, s, bl in reads:
        for a, b in bl:
            lines.append("%s\tsrc\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (c, a + 1, b, s, n))
    path = str(tmp_path / "reads.gff")
    open(path, "w").write("".join(lines))
    mrf = "AlignmentBlocks\n" + "".join(J.mrf_line(c, s, bl) for _, c, s, bl in reads)
    rows, report = R.table(interval, mrf)
    same(index_of(paths).host("UCSC_GFF", path), rows, report)
    assert rows[0] == ("chr1", 200, 300, "+", 1, 1, 2, 1, 2, 100, 100, 200, 2, 2, 2)
    p = tool(paths, path, "UCSC_GFF")
    assert p.returncode == 0 and p.stdout == R.text(rows)


# ----------------------------------------------------------------------------- options, errors

def test_the_output_path_and_bad_options(three_formats, tmp_path):
    interval, mrf, paths, _ = three_formats
    rows, _ = R.table_once("fmt", interval, mrf)
    out = str(tmp_path / "t.tab")
    argv = [os.path.join(BIN, "retention"), "--host", "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"]]
    p = subprocess.run(argv + [out], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == R.text(rows)
    p = subprocess.run(argv + ["-"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == R.text(rows)
    for bad in [["--nonsense"], ["--ratio"], ["--min-reads", "1"], ["--novel"]] + [["--min-overhang"] + v for v in ([], ["-1"], ["4294967296"], ["1x"])]:
        p = tool(paths, paths["mrf"], opts=bad)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], bad
    for args in (argv[2:] + ["--min-overhang"], argv[2:7], argv[2:] + ["-", "-"]):
        p = subprocess.run(argv[:2] + args, capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], args


def test_a_malformed_line_gives_counts_status_and_message(three_formats, tmp_path):
    _, _, paths, _ = three_formats
    good = J.mrf_line("chr1", "+", [(150, 200), (300, 350)])
    bad = "chr1:+:15x:200:1:50"
    path = str(tmp_path / "bad.mrf")
    open(path, "w").write("AlignmentBlocks\n" + good * 40 + bad + "\n" + good * 3)
    ix = index_of(paths)
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_SINGLE", path)
    assert e.value.status == LSQ_E_PARSE and str(e.value).endswith(": #41:" + bad)
    p = tool(paths, path)
    assert p.returncode == 1 and p.stdout == "" and "#41:" + bad in p.stderr and "Lexical_cast error" in p.stderr
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_PAIRED", path)
    assert e.value.status == -3 and str(e.value).endswith("Unknown file format error: MRF_PAIRED")
    p = tool(paths, str(tmp_path / "missing.mrf"))
    assert p.returncode == 1 and p.stdout == ""


def test_new_entry_points_are_exported_and_the_abi_version_stays():
    syms = ("lsq_ir_index_build", "lsq_ir_index_free", "lsq_ir_index_num_chroms", "lsq_ir_index_chrom_name", "lsq_ir_index_num_introns", "lsq_ir_index_dictionaries",
            "lsq_ir_host", "lsq_ir_host_reads", "lsq_ir_device", "lsq_ir_table_free", "lsq_ir_table_rows", "lsq_ir_table_arrays", "lsq_ir_table_report",
            "lsq_ir_table_times", "lsq_ir_format")
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in syms:
        assert hasattr(L.lib, sym), sym
        assert sym + "(" in header, sym
    assert L.lib.lsq_abi_version() == 2 and "#define LSQ_ABI_VERSION 2" in header
    assert os.access(os.path.join(BIN, "retention"), os.X_OK)
    assert L.retention.REPORT == R.REPORT and len(L.retention.REPORT) == 13 and L.retention.PHASES == ("sites", "depth", "index", "select", "copy_back")
    assert L.RetentionIndex is L.retention.RetentionIndex and L.Retention is L.retention.Retention
    rc, _ = L.cli_run("retention", ["retention", "--host"])
    assert rc == 1
