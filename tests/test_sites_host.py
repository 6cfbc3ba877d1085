"""Splice-site usage and read-through per junction without a GPU (include/lesseq_hip.h, lsq_ss_*): lsq_ss_host and `sites --host`
against the definition as tests/sites_ref.py restates it, and against a table worked out by hand."""
import os
import subprocess

import pytest

import lesseq_amd as L
import bam_writer
import junction_ref as J
import sites_ref as S
from test_junctions_host import log_messages, sam_of, spliced_reads, BIN, LSQ_E_PARSE

HERE = os.path.dirname(os.path.abspath(__file__))
USAGE = ("Usage:\nsites [--host] [--ratios] [--min-overhang N] [--min-reads N] [--novel] isoform_format isoforms_path g2i_format g2i_path read_format reads_path "
         "[out_path]")
BIG = 4294967295


def index_of(paths):
    return L.SiteIndex(L.Annotation(paths["interval"], paths["map"]))


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None):
    argv = [os.path.join(BIN, "sites"), "--host"] + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads]
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})))


def same(got, rows, report):
    assert got.rows() == rows
    assert got.report == report
    assert got.text() == S.text(rows)
    assert got.text(ratios=True) == S.text(rows, ratios=True)


def format_reads():
    """(reads for sam_of, the last one alone runs through its boundary): spliced reads, unspliced ones across annotated splice sites"""
    reads = spliced_reads()
    reads += [("chr1", k % 2 == 1, [(180 + k, 320 + k)]) for k in range(7)] + [("chr2", False, [(190, 310)])] * 3 + [("chrU", False, [(190, 310)])]
    reads.append(("chr1", False, [(3080, 3120)]))      # the only block through 3100
    return reads


# ----------------------------------------------------------------------------- the definition

def test_the_table_worked_out_by_hand(tmp_path):
    iso, lines, rows, report = S.rows_case()
    interval, mrf, paths = S.write_case(str(tmp_path), "rows", iso, lines)
    assert S.table(interval, mrf) == (rows, report)
    ix = index_of(paths)
    assert ix.num_introns == 7 and ix.chrom_names() == ["chr1"]
    got = ix.host("MRF_SINGLE", paths["mrf"])
    same(got, rows, report)
    assert got.text().split("\n")[0] == "chr1\t201\t300\t+\t3\t6\t5\t3\t5"
    ratio_lines = got.text(ratios=True).split("\n")
    assert ratio_lines[0] == "chr1\t201\t300\t+\t3\t6\t5\t3\t5\t0.500000\t1.000000\t0.545455\t0.375000"
    assert ratio_lines[4] == "chr1\t1101\t1200\t+\t0\t0\t4\t0\t3\tNA\tNA\t0.000000\t0.000000"
    assert ratio_lines[5] == "chr1\t2101\t2200\t+\t0\t0\t0\t0\t0\tNA\tNA\tNA\tNA"
    assert got.times == dict.fromkeys(L.sites.PHASES, 0.0)
    p = tool(paths, paths["mrf"], opts=["--ratios"])
    assert p.returncode == 0 and p.stdout == S.text(rows, ratios=True)
    line = ("sites: 32 read(s), 47 block(s), 15 occurrence(s) of junctions; 0 block pair(s) below the overhang, 0 with a block on no chromosome of the annotation; "
            "8 row(s), 2 without a spliced read; 12 boundary(ies), 26 block(s) through one")
    assert log_messages(p.stderr) == [("WARNING", line)]


@pytest.mark.parametrize("min_overhang", [0, 1, 2, 10, 50, BIG])
def test_boundary_arithmetic(tmp_path, min_overhang):
    iso, lines = S.boundary_case()
    interval, mrf, paths = S.write_case(str(tmp_path), "edge", iso, lines)
    rows, report = S.table_once("edge", interval, mrf, min_overhang)
    same(index_of(paths).host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang), rows, report)
    by = {r[:3]: r for r in rows}
    assert ("chr1", -S.LIM + 1, -S.LIM + 500) in by and ("chr1", S.LIM - 500, S.LIM - 1) in by and len(rows) == 5 and report["boundaries"] == 10
    if min_overhang == BIG:
        assert report["through"] == 0
    elif min_overhang in (0, 1):
        # per m of OVERHANGS seven of the twelve blocks around p count under m itself; under 1 more do.  By hand for p = 1000 on
        # chr2 (no other block reaches it): m = 1: 7 hits; m = 2, 10, 50 under overhang 1: 11 each (all but the empty block)
        assert by[("chr2", 1000, 2000)][6] == 7 + 3 * 11
        assert S.table_once("edge", interval, mrf, 0) == S.table_once("edge", interval, mrf, 1)      # one-block reads: no junction rule to differ in
    elif min_overhang == 50:
        assert by[("chr2", 1000, 2000)][6] == 7 and by[("chr2", 1000, 2000)][8] == 7
    p = tool(paths, paths["mrf"], opts=["--min-overhang", str(min_overhang)])
    assert p.returncode == 0 and p.stdout == S.text(rows)


@pytest.mark.parametrize("min_overhang", [0, 1, 10, 51])
def test_rows_are_the_junction_tables_united_with_the_annotated_introns(tmp_path, min_overhang):
    lines = J.extract_lines() + S.walk_lines()
    interval, mrf, paths = S.write_case(str(tmp_path), "base", J.annotation_lines(), lines)
    rows, report = S.table_once("base", interval, mrf, min_overhang)
    got = index_of(paths).host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(got, rows, report)
    if min_overhang:
        jn = L.JunctionIndex(L.Annotation(paths["interval"], paths["map"])).host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
        assert [r[:5] for r in rows if r[4] > 0] == [r[:5] for r in jn.rows()]
        assert {k: got.report[k] for k in L.junctions.REPORT} == jn.report
    else:
        assert ("chr1", 200, 300, "+", 8) in [r[:5] for r in rows]      # the empty flank block makes an occurrence when nothing is asked of the flanks
    assert len([r for r in rows if r[4] == 0]) == report["unsupported"] > 0 and {r[3] for r in rows} == {".", "+", "-", "*"}
    if min_overhang == 1:
        big = [r for r in rows if r[0] == "chr3"]
        assert min(min(r[6], r[8]) for r in big if r[1] > 100100 and r[2] < 120700) >= 1      # the block over the whole gene runs through every boundary inside it


# ----------------------------------------------------------------------------- counters, threads

@pytest.mark.parametrize("kind", ["one_boundary", "run_lengths", "all_distinct"])
def test_counter_cases_and_threads(tmp_path, kind):
    iso, lines = S.counter_case(kind)
    interval, mrf, paths = S.write_case(str(tmp_path), kind, iso, lines)
    rows, report = S.table_once(kind, interval, mrf)
    ix = index_of(paths)
    for n_threads in (1, 3, 16):
        same(ix.host("MRF_SINGLE", paths["mrf"], n_threads=n_threads), rows, report)
    if kind == "one_boundary":
        assert rows == [("chr1", 200, 300, "+", 0, 0, 70000, 0, 0)]
    if kind == "all_distinct":
        assert report["boundaries"] == 70000 == report["through"] and all(r[6] == 1 == r[8] for r in rows)
        same(ix.host_reads(ix.parse_host("MRF_SINGLE", paths["mrf"]), n_threads=5), rows, report)
    if kind == "run_lengths":
        assert [v for r in rows[:5] for v in (r[6], r[8])] == [1, 2, 63, 64, 65] * 2


# ----------------------------------------------------------------------------- degenerate files

def test_degenerate_files(tmp_path):
    iso = J.annotation_lines()
    n_introns = len(J.introns("".join(iso)))
    for stem, lines, header in (("unspliced", [J.mrf_line("chr1", "+", [(150, 250)])] * 5, "AlignmentBlocks\n"), ("header_only", [], "AlignmentBlocks\n"), ("nothing", [], "")):
        interval, mrf, paths = S.write_case(str(tmp_path), stem, iso, lines, header)
        rows, report = S.table(interval, mrf)
        got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
        same(got, rows, report)
        assert len(rows) == n_introns == report["unsupported"] and report["through"] == (5 if lines else 0)
        p = tool(paths, paths["mrf"])
        assert p.returncode == 0 and p.stdout == S.text(rows)
        p = tool(paths, paths["mrf"], opts=["--min-reads", "1"])
        assert p.returncode == 0 and p.stdout == ""
    mono = [J.interval_line("m.a", "chr1", "+", [(0, 1000)])]
    interval, mrf, paths = S.write_case(str(tmp_path), "mono", mono, J.extract_lines())
    rows, report = S.table(interval, mrf)
    same(index_of(paths).host("MRF_SINGLE", paths["mrf"]), rows, report)
    assert rows and {r[3] for r in rows} == {"."} and report["unsupported"] == 0
    interval, mrf, paths = S.write_case(str(tmp_path), "mono_unspliced", mono, [J.mrf_line("chr1", "+", [(150, 250)])] * 5)
    got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
    same(got, [], dict(zip(S.REPORT, (5, 5, 0, 0, 0, 0, 0, 0))))
    assert got.text() == ""


# ----------------------------------------------------------------------------- formats

@pytest.fixture(scope="module")
def three_formats(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ss3"))
    reads = format_reads()
    interval, mrf, paths = S.write_case(d, "fmt", J.annotation_lines(), [J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads])
    sam = sam_of(reads).encode()
    paths["sam"] = os.path.join(d, "fmt.sam")
    open(paths["sam"], "wb").write(sam)
    for layout in ("htslib", "cut61"):
        paths["bam_" + layout] = os.path.join(d, "fmt_%s.bam" % layout)
        open(paths["bam_" + layout], "wb").write(bam_writer.sam_to_bam(sam, layout))
    return interval, mrf, paths, reads


def test_one_table_from_mrf_sam_and_bam(three_formats):
    interval, mrf, paths, reads = three_formats
    rows, report = S.table_once("fmt", interval, mrf)
    ix = index_of(paths)
    same(ix.host("MRF_SINGLE", paths["mrf"]), rows, report)
    sam = open(paths["sam"], "rb").read()
    assert S.table(interval, L.sam_to_mrf(sam).decode()) == (rows, report)
    same(ix.host("SAM_SINGLE", paths["sam"]), rows, report)
    for layout in ("htslib", "cut61"):
        same(ix.host("BAM_SINGLE", paths["bam_" + layout]), rows, report)
        p = tool(paths, paths["bam_" + layout], "BAM_SINGLE")
        assert p.returncode == 0 and p.stdout == S.text(rows)
    assert report["through"] > 10 and report["occurrences"] > 100


def test_a_filter_that_removes_one_record_changes_that_boundarys_count(three_formats, tmp_path):
    interval, mrf, paths, reads = three_formats
    rows, _ = S.table_once("fmt", interval, mrf)
    ix = index_of(paths)
    last = len(reads) - 1
    at = [i for i, r in enumerate(rows) if r[:3] == ("chr1", 3100, 3200)][0]
    assert rows[at][6] == 1
    want = list(rows)
    want[at] = rows[at][:6] + (0,) + rows[at][7:]
    for name, kw, env in (("mapq", dict(mapq={last: 3}), {"LSQ_SAM_MIN_MAPQ": "4"}), ("flag", dict(flags={last: 0x400}), {"LSQ_SAM_SKIP_FLAGS": str(0x904 | 0x400)})):
        sam = sam_of(reads, **kw).encode()
        path = str(tmp_path / (name + ".sam"))
        open(path, "wb").write(sam)
        opts = dict(min_mapq=4) if name == "mapq" else dict(skip_flags=0x904 | 0x400)
        assert ix.host("SAM_SINGLE", path).rows() == rows                       # the defaults keep the record
        assert ix.host("SAM_SINGLE", path, **opts).rows() == want
        bam = str(tmp_path / (name + ".bam"))
        open(bam, "wb").write(bam_writer.sam_to_bam(sam))
        assert ix.host("BAM_SINGLE", bam, **opts).rows() == want
        p = tool(paths, path, "SAM_SINGLE", env=env)
        assert p.returncode == 0 and p.stdout == S.text(want)


def test_name_keyed_lines_count_as_blocks(tmp_path):
    """UCSC_GFF: the lines of one name are one read's blocks; two overlapping lines of one name both run through a boundary"""
    iso, _, _, _ = S.rows_case()
    interval, _, paths = S.write_case(str(tmp_path), "gff", iso, [])
    reads = [("n1", "chr1", "+", [(150, 200), (300, 350)]), ("n2", "chr1", "+", [(180, 320), (190, 330)]), ("n3", "chr1", "+", [(1050, 1250)])]
    lines = ["track name=x\n", "browser position chr1\n"]
    for n, c, s, bl in reads:
        for a, b in bl:
            lines.append("%s\tsrc\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (c, a + 1, b, s, n))
    path = str(tmp_path / "reads.gff")
    open(path, "w").write("".join(lines))
    mrf = "AlignmentBlocks\n" + "".join(J.mrf_line(c, s, bl) for _, c, s, bl in reads)
    rows, report = S.table(interval, mrf)
    got = index_of(paths).host("UCSC_GFF", path)
    same(got, rows, report)
    assert rows[0] == ("chr1", 200, 300, "+", 1, 1, 2, 1, 2) and report["through"] == 6
    p = tool(paths, path, "UCSC_GFF")
    assert p.returncode == 0 and p.stdout == S.text(rows)


# ----------------------------------------------------------------------------- text, options, errors

def test_formatter_options_and_the_output_path(three_formats, tmp_path):
    interval, mrf, paths, _ = three_formats
    rows, _ = S.table_once("fmt", interval, mrf)
    got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
    for min_reads, novel, ratios in ((0, False, False), (1, False, True), (2, True, False), (0, True, True), (100000, False, False)):
        want = S.text(rows, min_reads, novel, ratios)
        assert got.text(min_reads, novel, ratios) == want
        p = tool(paths, paths["mrf"], opts=["--min-reads", str(min_reads)] + (["--novel"] if novel else []) + (["--ratios"] if ratios else []))
        assert p.returncode == 0 and p.stdout == want
    assert S.text(rows, 1) != S.text(rows) and S.text(rows, 0, True) not in ("", S.text(rows)) and "NA" in S.text(rows, ratios=True)
    out = str(tmp_path / "t.tab")
    argv = [os.path.join(BIN, "sites"), "--host", "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"]]
    p = subprocess.run(argv + [out], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == S.text(rows)
    p = subprocess.run(argv + ["-"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == S.text(rows)


def test_bad_options_give_the_usage_text(three_formats):
    _, _, paths, _ = three_formats
    numbers = [[opt] + v for opt in ("--min-overhang", "--min-reads") for v in ([], ["-1"], ["4294967296"], ["1x"])]
    for bad in [["--nonsense"], ["--ratio"]] + numbers:
        p = tool(paths, paths["mrf"], opts=bad)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], bad
    positional = ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"]]
    for argv in (positional + ["--min-overhang"], positional + ["--min-reads"], positional[:5], positional + ["-", "-"]):
        p = subprocess.run([os.path.join(BIN, "sites"), "--host"] + argv, capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], argv


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
    syms = ("lsq_ss_index_build", "lsq_ss_index_free", "lsq_ss_index_num_chroms", "lsq_ss_index_chrom_name", "lsq_ss_index_num_introns", "lsq_ss_index_dictionaries",
            "lsq_ss_host", "lsq_ss_host_reads", "lsq_ss_device", "lsq_ss_table_free", "lsq_ss_table_rows", "lsq_ss_table_arrays", "lsq_ss_table_report",
            "lsq_ss_table_times", "lsq_ss_format", "lsq_ss_lds_slots")
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in syms:
        assert hasattr(L.lib, sym), sym
        assert sym + "(" in header, sym
    assert L.lib.lsq_abi_version() == 2 and "#define LSQ_ABI_VERSION 2" in header
    assert os.access(os.path.join(BIN, "sites"), os.X_OK)
    assert L.sites.LDS_SLOTS >= 1024 and L.sites.LDS_SLOTS & (L.sites.LDS_SLOTS - 1) == 0
    assert L.sites.REPORT == S.REPORT and L.SiteIndex is L.sites.SiteIndex and L.Sites is L.sites.Sites
    rc, _ = L.cli_run("sites", ["sites", "--host"])
    assert rc == 1
