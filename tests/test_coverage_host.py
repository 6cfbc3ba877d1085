"""Per-base read depth without a GPU (include/lesseq_hip.h, lsq_cov_*): lsq_cov_host and `coverage --host` against the definition as
tests/coverage_ref.py restates it.  All values are integers: the tables equal the reference's exactly."""
import os
import subprocess

import pytest

import lesseq_amd as L
import bam_writer
import coverage_ref as V
from test_junctions_host import sam_of, spliced_reads, log_messages

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "lesseq_amd", "bin")
LSQ_E_PARSE = -4
USAGE = ("Usage:\ncoverage [--host] [--strand +|-] [--min-depth N] [--regions regions_path] isoform_format isoforms_path g2i_format g2i_path read_format reads_path "
         "[out_path]")


def index_of(paths):
    return L.CoverageIndex(L.Annotation(paths["interval"], paths["map"]))


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None, host=True, timeout=None):
    argv = [os.path.join(BIN, "coverage")] + (["--host"] if host else []) + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads]
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=timeout)


def same(got, want):
    rows, regions, report = want
    assert got.rows() == rows
    assert got.regions() == regions
    assert got.report == report
    assert got.text() == V.text(rows) and got.regions_text() == V.regions_text(regions)
    assert V.conserved(got.rows(), got.report)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cov"))
    return V.write_case(d, "base", V.definition_annotation(), V.definition_lines())


def test_the_reference_states_the_rows_two_ways(base):
    interval, mrf, _ = base
    arrays, _ = V.depth_arrays(interval, mrf)
    assert V.rows_of(arrays) == V.fast_rows_of(arrays)


@pytest.mark.parametrize("strand", [None, "+", "-"])
def test_host_equals_the_reference_on_the_definition_cases(base, strand):
    interval, mrf, paths = base
    want = V.table(interval, mrf, strand)
    rows, regions, report = want
    ix = index_of(paths)
    assert ix.chrom_names() == ["chr2", "chr10", "chr1", "chrA", "chrB", "chr9"] and ix.num_regions == 7
    same(ix.host("MRF_SINGLE", paths["mrf"], strand=strand), want)
    if strand is None:
        # the cases are there, worked out by hand
        assert [r[0] for r in rows if r[0] != "chr1"] == ["chr10"] * 3 + ["chr2"] * 5 + ["chrA"] * 2 + ["chrB"] * 2
        for r in (("chr1", 100, 120, 1), ("chr1", 120, 150, 2), ("chr1", 180, 200, 2), ("chr1", 200, 340, 1),      # nested, overlapping; 260 and 300 are no boundaries
                  ("chr1", 1000, 1100, 1), ("chr1", 1200, 1220, 1), ("chr1", 1220, 1250, 2), ("chr1", 1250, 1300, 1), ("chr1", 2000, 2050, 5),
                  ("chr1", 3000, 3050, 1), ("chr1", 3100, 3150, 1), ("chr1", 4000, 4040, 1), ("chr1", 4040, 4060, 2), ("chr1", 4060, 4100, 1),
                  ("chr1", -500, -450, 1), ("chr1", -450, -400, 2), ("chr1", -400, -380, 1), ("chr1", -20, 30, 1),
                  ("chrA", 400, 450, 1), ("chrA", 450, 500, 2), ("chrB", 500, 520, 2), ("chrB", 520, 600, 1), ("chr1", 5010, 5020, 1), ("chr1", 5110, 5120, 1)):
            assert r in rows, r
        assert report["no_chromosome"] == 3 and report["empty"] == 2 and report["other_strand"] == 0 and report["counted"] == report["blocks"] - 5
        assert ("g9.a", "chr9", "+", 100, 0, 0) in regions and ("gB.a", "chrB", "+", 100, 100, 120) in regions
    else:
        assert report["other_strand"] > 5 and report["counted"] > 5 and report["no_chromosome"] == 3
    p = tool(paths, paths["mrf"], opts=["--strand", strand] if strand else [])
    assert p.returncode == 0 and p.stdout == V.text(rows), p.stderr


def test_min_depth_counts_the_covered_bases_and_filters_the_text(base, tmp_path):
    interval, mrf, paths = base
    ix = index_of(paths)
    for min_depth in (1, 2, 6):
        want = V.table(interval, mrf, None, min_depth)
        got = ix.host("MRF_SINGLE", paths["mrf"], min_depth=min_depth)
        same(got, want)
        assert got.text(min_depth) == V.text(want[0], min_depth)
        out = str(tmp_path / ("r%d.tsv" % min_depth))
        p = tool(paths, paths["mrf"], opts=["--min-depth", str(min_depth), "--regions", out])
        assert p.returncode == 0 and p.stdout == V.text(want[0], min_depth) and open(out).read() == V.regions_text(want[1])
    assert V.text(want[0], 6) == "" and all(r[4] == 0 for r in want[1]) and any(r[5] for r in want[1])
    assert V.text(V.table(interval, mrf)[0], 2) not in ("", V.text(V.table(interval, mrf)[0]))


def test_the_text_formats(base):
    interval, mrf, paths = base
    got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
    lines = got.text().split("\n")
    assert lines[0] == "chr1\t-500\t-450\t1" and lines[-1] == "" and all(len(ln.split("\t")) == 4 for ln in lines[:-1])
    rt = got.regions_text().split("\n")
    assert rt[5] == "gB.a\tchrB\t+\t100\t100\t120\t1.2000" and rt[6] == "g9.a\tchr9\t+\t100\t0\t0\t0.0000"


def test_regions(tmp_path):
    iso, lines = V.regions_case()
    interval, mrf, paths = V.write_case(str(tmp_path), "regions", iso, lines)
    ix = index_of(paths)
    for min_depth in (1, 2, 3, 4):
        want = V.table(interval, mrf, None, min_depth)
        same(ix.host("MRF_SINGLE", paths["mrf"], min_depth=min_depth), want)
    rows, regions, _ = V.table(interval, mrf, None, 2)
    assert rows == [("chr1", 100, 150, 2), ("chr1", 150, 200, 3), ("chr1", 200, 250, 1), ("chr1", 400, 500, 1)]
    assert regions[:11] == [("inside.a", "chr1", "+", 30, 30, 60), ("on_edges.a", "chr1", "+", 50, 50, 150), ("all_rows.a", "chr1", "-", 150, 100, 300),
                            ("across_gap.a", "chr1", "+", 270, 20, 160), ("uncovered.a", "chr1", "+", 100, 0, 0), ("between.a", "chr1", "+", 150, 0, 0),
                            ("no_reads.a", "chr9", "+", 100, 0, 0), ("union.a", "chr1", "+", 160, 100, 290), ("unsorted.a", "chr1", "-", 50, 20, 60),
                            ("no_exon.a", "chr1", "+", 0, 0, 0), ("none_counted.a", "chr1", "+", 0, 0, 0)]
    assert "no_exon.a\tchr1\t+\t0\t0\t0\t0.0000\n" in V.regions_text(regions) and len(regions) > 4096


def test_a_depth_sum_past_32_bits(tmp_path):
    iso, lines = V.deep_case()
    interval, mrf, paths = V.write_case(str(tmp_path), "deep", iso, lines)
    want = V.table(interval, mrf)
    assert want[0] == [("chr1", 0, 100000, 70000)] and want[1][0][5] == 7000000000 and want[1][1][4:] == (50000, 3500000000)
    same(index_of(paths).host("MRF_SINGLE", paths["mrf"], n_threads=4), want)


def test_empty_inputs(tmp_path):
    iso = V.definition_annotation()
    for stem, lines, header in (("header_only", [], "AlignmentBlocks\n"), ("nothing", [], ""), ("none_counted", [V.mrf_line("chrU", "+", [(1, 9)])] * 3, "AlignmentBlocks\n")):
        interval, mrf, paths = V.write_case(str(tmp_path), stem, iso, lines, header)
        got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
        same(got, V.table(interval, mrf))
        assert len(got) == 0 and got.text() == "" and got.report["reads"] == len(lines) and got.report["bases"] == 0 and len(got.regions()) == 7
        p = tool(paths, paths["mrf"])
        assert p.returncode == 0 and p.stdout == ""


def test_one_table_from_mrf_sam_and_bam(tmp_path):
    reads = spliced_reads()
    iso = V.definition_annotation() + [V.interval_line("junc.a", "chr1", "+", [(150, 200), (300, 350), (500, 530)])]
    interval, mrf, paths = V.write_case(str(tmp_path), "fmt", iso, [V.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads])
    sam = sam_of(reads, mapq={0: 3, 7: 3}).encode()
    spath, bpath = str(tmp_path / "fmt.sam"), str(tmp_path / "fmt.bam")
    open(spath, "wb").write(sam)
    open(bpath, "wb").write(bam_writer.sam_to_bam(sam, "cut61"))
    ix = index_of(paths)
    for strand in (None, "-"):
        want = V.table(interval, mrf, strand)
        same(ix.host("MRF_SINGLE", paths["mrf"], strand=strand), want)
        same(ix.host("SAM_SINGLE", spath, strand=strand), want)
        same(ix.host("BAM_SINGLE", bpath, strand=strand), want)
    assert want[2]["other_strand"] > 50 and want[2]["no_chromosome"] >= 100
    # a filter that removes two records
    fewer = V.table(interval, L.sam_to_mrf(sam, min_mapq=4).decode())
    assert fewer[2]["reads"] == len(reads) - 2 and fewer != V.table(interval, mrf)
    same(ix.host("SAM_SINGLE", spath, min_mapq=4), fewer)
    same(ix.host("BAM_SINGLE", bpath, min_mapq=4), fewer)
    for fmt, path in (("SAM_SINGLE", spath), ("BAM_SINGLE", bpath)):
        p = tool(paths, path, fmt, env={"LSQ_SAM_MIN_MAPQ": "4"})
        assert p.returncode == 0 and p.stdout == V.text(fewer[0])
    p = tool(paths, bpath, "BAM_SINGLE", env={"LSQ_BAM_VERIFY": "1"})
    assert p.returncode == 0 and p.stdout == V.text(V.table(interval, mrf)[0])


def test_ucsc_gff_reads_one_line_per_block(base, tmp_path):
    interval, _, paths = base
    reads = [("n1", "chr1", "+", [(150, 200), (300, 350)]), ("n2", "chr1", "-", [(160, 200), (300, 350), (500, 520)]), ("n3", "chr2", "+", [(150, 200)])]
    lines = ["track name=x\n", "browser position chr1\n"]      # (the format has two header lines)
    for n, c, s, bl in reads:
        for a, b in bl:
            lines.append("%s\tsrc\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (c, a + 1, b, s, n))
    path = str(tmp_path / "reads.gff")
    open(path, "w").write("".join(lines))
    mrf = "AlignmentBlocks\n" + "".join(V.mrf_line(c, s, bl) for _, c, s, bl in reads)
    for strand in (None, "+"):
        same(index_of(paths).host("UCSC_GFF", path, strand=strand), V.table(interval, mrf, strand))
    p = tool(paths, path, "UCSC_GFF")
    assert p.returncode == 0 and p.stdout == V.text(V.table(interval, mrf)[0]) != ""


def test_threads_do_not_change_the_tables(tmp_path):
    iso, lines = V.count_case(140001, True)
    interval, mrf, paths = V.write_case(str(tmp_path), "big", iso, lines)
    want = V.table(interval, mrf)
    ix = index_of(paths)
    for n_threads in (1, 3, 16):
        same(ix.host("MRF_SINGLE", paths["mrf"], n_threads=n_threads), want)
    reads = ix.parse_host("MRF_SINGLE", paths["mrf"])
    same(ix.host_reads(reads, n_threads=5), want)
    same(ix.host_reads(reads, strand="-", n_threads=5), V.table(interval, mrf, "-"))
    assert want[2]["counted"] == 140001 and want[2]["reads"] > 1 << 16


def test_the_tool_logs_the_report_and_takes_an_output_path(base, tmp_path):
    interval, mrf, paths = base
    rows, _, report = V.table(interval, mrf)
    out = str(tmp_path / "t.bedgraph")
    argv = [os.path.join(BIN, "coverage"), "--host", "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"]]
    p = subprocess.run(argv + [out], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == V.text(rows)
    assert "%d counted in %d row(s)" % (report["counted"], len(rows)) in p.stderr and "%d base(s) in the counted blocks (solve's total_read_bases)" % report["bases"] in p.stderr
    line = ("coverage: %d read(s), %d block(s), %d counted in %d row(s); %d on no chromosome of the annotation, %d empty or descending, %d of the other strand; "
            "%d base(s) in the counted blocks (solve's total_read_bases)"
            % (report["reads"], report["blocks"], report["counted"], len(rows), report["no_chromosome"], report["empty"], report["other_strand"], report["bases"]))
    assert log_messages(p.stderr) == [("WARNING", line)]
    p = subprocess.run(argv + ["-"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == V.text(rows)
    for bad in (["--strand", "x"], ["--strand"], ["--min-depth", "-1"], ["--min-depth", "4294967296"], ["--min-depth", "1x"], ["--min-depth"], ["--regions"], ["--nonsense"]):
        p = tool(paths, paths["mrf"], opts=bad)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], bad
    # an option that ends the line has no value; five and eight positional arguments
    for bad in (argv[2:] + ["--min-depth"], argv[2:] + ["--regions"], argv[2:] + ["--strand"], argv[2:7], argv[2:] + ["-", "-"]):
        p = subprocess.run(argv[:2] + bad, capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], bad
    # the regions file is written before the output file: an output path that cannot be written leaves the regions behind
    regions, lost = str(tmp_path / "r.tsv"), str(tmp_path / "no_such_directory" / "t.bedgraph")
    p = subprocess.run(argv[:2] + ["--regions", regions] + argv[2:] + [lost], capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr)[-1] == ("ERROR", "cannot write " + lost)
    assert open(regions).read() == V.regions_text(V.table(interval, mrf)[1]) and not os.path.exists(lost)


def test_a_malformed_record_gives_counts_status_and_message(base, tmp_path):
    _, _, paths = base
    good = V.mrf_line("chr1", "+", [(150, 200), (300, 350)])
    bad = "chr1:+:15x:200:1:50"
    path = str(tmp_path / "bad.mrf")
    open(path, "w").write("AlignmentBlocks\n" + good * 40 + bad + "\n" + good * 3)
    ix = index_of(paths)
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_SINGLE", path)
    assert e.value.status == LSQ_E_PARSE and str(e.value).endswith(": #41:" + bad)
    regions = str(tmp_path / "never.tsv")
    p = tool(paths, path, opts=["--regions", regions])
    assert p.returncode == 1 and p.stdout == "" and "#41:" + bad in p.stderr and "Lexical_cast error" in p.stderr and not os.path.exists(regions)
    sam = "@HD\tVN:1.6\n" + "q\t0\tchr1\t101\t60\t50M10N50M\t*\t0\t0\t*\t*\n" * 7 + "q\t0\tchr1\t101\t60\t50Q\t*\t0\t0\t*\t*\n"
    spath = str(tmp_path / "bad.sam")
    open(spath, "w").write(sam)
    with pytest.raises(L.LsqError) as e:
        ix.host("SAM_SINGLE", spath)
    assert e.value.status == LSQ_E_PARSE and ": #9:q\t0\tchr1\t101\t60\t50Q" in str(e.value)
    p = tool(paths, spath, "SAM_SINGLE")
    assert p.returncode == 1 and p.stdout == "" and "#9:q" in p.stderr
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_PAIRED", path)
    assert e.value.status == -3
    with pytest.raises(ValueError):
        ix.host("MRF_SINGLE", paths["mrf"], strand="x")
    p = tool(paths, str(tmp_path / "missing.mrf"))
    assert p.returncode == 1 and p.stdout == ""


def test_new_entry_points_are_exported_and_the_abi_version_stays():
    syms = ("lsq_cov_index_build", "lsq_cov_index_free", "lsq_cov_index_num_chroms", "lsq_cov_index_chrom_name", "lsq_cov_index_num_regions", "lsq_cov_index_dictionaries",
            "lsq_cov_host", "lsq_cov_host_reads", "lsq_cov_device", "lsq_cov_table_free", "lsq_cov_table_rows", "lsq_cov_table_regions", "lsq_cov_table_arrays",
            "lsq_cov_table_region_arrays", "lsq_cov_table_region_name", "lsq_cov_table_region_strand", "lsq_cov_table_report", "lsq_cov_table_times", "lsq_cov_format",
            "lsq_cov_format_regions", "lsq_cov_sort_tile")
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in syms:
        assert hasattr(L.lib, sym), sym
        assert sym + "(" in header, sym
    assert L.lib.lsq_abi_version() == 2 and "#define LSQ_ABI_VERSION 2" in header
    assert os.access(os.path.join(BIN, "coverage"), os.X_OK)
    assert L.coverage.SORT_TILE >= 1024 and L.CoverageIndex is L.coverage.CoverageIndex
    rc, text = L.cli_run("coverage", ["--nonsense"])
    assert rc == 1 and text == ""
