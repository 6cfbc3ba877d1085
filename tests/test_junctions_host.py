"""Splice junctions without a GPU (include/lesseq_hip.h, lsq_jn_*): lsq_jn_host and `junctions --host` against the definition as
tests/junction_ref.py restates it."""
import os
import re
import subprocess

import pytest

import lesseq_amd as L
import bam_writer
import junction_ref as J

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "lesseq_amd", "bin")
LSQ_E_PARSE = -4
USAGE = ("Usage:\njunctions [--host] [--min-overhang N] [--min-reads N] [--novel] isoform_format isoforms_path g2i_format g2i_path read_format reads_path "
         "[out_path]")
LOG_PREFIX = re.compile(r"^\[LOG \d{4}-\d\d-\d\d \d\d:\d\d:\d\d (ERROR|WARNING|INFO|DEBUG)\] ", re.M)


def log_messages(stderr):
    """[(level, text)] of an executable's log: every message behind its "[LOG <date> <time> <level>] ", nothing between them"""
    parts = LOG_PREFIX.split(stderr)
    assert parts[0] == "" and all(t.endswith("\n") for t in parts[2::2]), stderr
    return [(lv, t[:-1]) for lv, t in zip(parts[1::2], parts[2::2])]


def index_of(paths):
    return L.JunctionIndex(L.Annotation(paths["interval"], paths["map"]))


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None):
    argv = [os.path.join(BIN, "junctions"), "--host"] + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads]
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})))


def same(got, rows, report):
    assert got.rows() == rows
    assert got.report == report
    assert got.text() == J.text(rows)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jn"))
    interval, mrf, paths = J.write_case(d, "base", J.annotation_lines(), J.extract_lines())
    return interval, mrf, paths


def test_the_index_holds_the_annotations_chromosomes_and_introns(base):
    interval, _, paths = base
    ix = index_of(paths)
    assert ix.chrom_names() == J.chromosomes(interval) == ["chr1", "chr2", "chrM", "chr3"]
    assert ix.num_introns == len(J.introns(interval))


@pytest.mark.parametrize("min_overhang", [1, 9, 10, 11, 50, 51])
def test_host_equals_the_reference_on_the_extraction_and_annotation_cases(base, min_overhang):
    interval, mrf, paths = base
    rows, report = J.table(interval, mrf, min_overhang)
    got = index_of(paths).host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(got, rows, report)
    if min_overhang == 1:
        # the cases are there: every ann character, a negative start, both ends of the range, pairs of every kind that makes none
        assert {r[3] for r in rows} == {".", "+", "-", "*"}
        assert rows[0][:3] == ("chr1", -(1 << 30) + 30, -(1 << 30) + 50) and ("chr1", (1 << 30) - 50, (1 << 30) - 30) in [r[:3] for r in rows]
        assert report["no_chromosome"] == 5 and report["dropped_overhang"] == 1 and report["reads"] == len(J.extract_lines()) - 1
        assert ("chr1", 200, 300, "+", 7, 4, 2, 50) in rows and ("chr2", 200, 300, "-", 2, 1, 1, 50) in rows
        assert ("chr3", 120500, 120700, "+", 1, 1, 0, 50) in rows and ("chr3", 100100, 120700, ".", 1, 1, 0, 50) in rows
    p = tool(paths, paths["mrf"], opts=["--min-overhang", str(min_overhang)])
    assert p.returncode == 0 and p.stdout == J.text(rows)


def test_the_tool_writes_the_report_to_the_log_and_takes_an_output_path(base, tmp_path):
    interval, mrf, paths = base
    rows, report = J.table(interval, mrf)
    out = str(tmp_path / "t.tab")
    p = subprocess.run([os.path.join(BIN, "junctions"), "--host", "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"], out],
                       capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == J.text(rows)
    assert "%d occurrence(s) of %d junction(s)" % (report["occurrences"], len(rows)) in p.stderr
    line = ("junctions: %d read(s), %d block(s), %d occurrence(s) of %d junction(s); %d block pair(s) below the overhang, %d with a block on no chromosome of the annotation"
            % (report["reads"], report["blocks"], report["occurrences"], len(rows), report["dropped_overhang"], report["no_chromosome"]))
    assert log_messages(p.stderr) == [("WARNING", line)]
    p = subprocess.run([os.path.join(BIN, "junctions"), "--host", "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"], "-"],
                       capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout == J.text(rows)      # "-": standard output
    numbers = [[opt] + v for opt in ("--min-overhang", "--min-reads") for v in ([], ["-1"], ["4294967296"], ["1x"])]
    for bad in [["--min-overhang", "0"], ["--nonsense"]] + numbers:
        p = tool(paths, paths["mrf"], opts=bad)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], bad
    positional = ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"]]
    # a number option that ends the line has no value; five and eight positional arguments
    for argv in (positional + ["--min-overhang"], positional + ["--min-reads"], positional[:5], positional + ["-", "-"]):
        p = subprocess.run([os.path.join(BIN, "junctions"), "--host"] + argv, capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], argv


def test_formatter_options(base):
    interval, mrf, paths = base
    rows, _ = J.table(interval, mrf)
    got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
    for min_reads, novel in ((0, False), (2, False), (0, True), (2, True), (1000, False)):
        want = J.text(rows, min_reads, novel)
        assert got.text(min_reads, novel) == want
        p = tool(paths, paths["mrf"], opts=["--min-reads", str(min_reads)] + (["--novel"] if novel else []))
        assert p.returncode == 0 and p.stdout == want
    assert J.text(rows, 2, True) != J.text(rows, 2, False) != J.text(rows)


def test_empty_inputs(tmp_path):
    iso = J.annotation_lines()
    for stem, lines, header in (("unspliced", [J.mrf_line("chr1", "+", [(150, 200)])] * 5, "AlignmentBlocks\n"), ("header_only", [], "AlignmentBlocks\n"), ("nothing", [], "")):
        interval, mrf, paths = J.write_case(str(tmp_path), stem, iso, lines, header)
        got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
        assert len(got) == 0 and got.text() == "" and got.report["reads"] == len(lines) and got.report["occurrences"] == 0
        p = tool(paths, paths["mrf"])
        assert p.returncode == 0 and p.stdout == ""
    # an annotation without any intron
    interval, mrf, paths = J.write_case(str(tmp_path), "mono", [J.interval_line("m.a", "chr1", "+", [(0, 1000)])], J.extract_lines())
    rows, report = J.table(interval, mrf)
    ix = index_of(paths)
    assert ix.num_introns == 0
    same(ix.host("MRF_SINGLE", paths["mrf"]), rows, report)
    assert rows and {r[3] for r in rows} == {"."}


def sam_of(reads, mapq=None, flags=None):
    """a SAM text of reads [(chrom, minus, [(start, end)] ascending with gaps)]: a CIGAR of M and N"""
    lines = ["@HD\tVN:1.6"]
    for k, (chrom, minus, blocks) in enumerate(reads):
        cigar = ""
        for q, (s, e) in enumerate(blocks):
            if q:
                cigar += "%dN" % (s - blocks[q - 1][1])
            cigar += "%dM" % (e - s)
        flag = (16 if minus else 0) | (flags or {}).get(k, 0)
        lines.append("r%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t*\t*" % (k, flag, chrom, blocks[0][0] + 1, (mapq or {}).get(k, 60), cigar))
    return "\n".join(lines) + "\n"


def spliced_reads():
    reads = []
    for k in range(300):
        s = 150 + k % 50
        reads.append((("chr1", "chr2", "chrU")[k % 3], k % 2 == 1, [(s, 200), (300, 310 + k % 40)] + ([(500, 530)] if k % 5 == 0 else [])))
    reads.append(("chr1", False, [(3050, 3100), (3200, 3250)]))      # the only read of its junction
    return reads


@pytest.fixture(scope="module")
def three_formats(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("jn3"))
    reads = spliced_reads()
    mrf_lines = [J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads]
    interval, mrf, paths = J.write_case(d, "fmt", J.annotation_lines(), mrf_lines)
    sam = sam_of(reads).encode()
    paths["sam"] = os.path.join(d, "fmt.sam")
    open(paths["sam"], "wb").write(sam)
    for layout in ("htslib", "cut61"):
        paths["bam_" + layout] = os.path.join(d, "fmt_%s.bam" % layout)
        open(paths["bam_" + layout], "wb").write(bam_writer.sam_to_bam(sam, layout))
    return interval, mrf, paths, reads


def test_one_table_from_mrf_sam_and_bam(three_formats):
    interval, mrf, paths, reads = three_formats
    rows, report = J.table(interval, mrf)
    ix = index_of(paths)
    same(ix.host("MRF_SINGLE", paths["mrf"]), rows, report)
    sam = open(paths["sam"], "rb").read()
    assert J.table(interval, L.sam_to_mrf(sam).decode()) == (rows, report)
    same(ix.host("SAM_SINGLE", paths["sam"]), rows, report)
    for layout in ("htslib", "cut61"):
        bam = open(paths["bam_" + layout], "rb").read()
        assert J.table(interval, L.bam_to_mrf(bam).decode()) == (rows, report)
        same(ix.host("BAM_SINGLE", paths["bam_" + layout]), rows, report)
        p = tool(paths, paths["bam_" + layout], "BAM_SINGLE")
        assert p.returncode == 0 and p.stdout == J.text(rows)
    assert len(rows) > 10 and report["no_chromosome"] >= 100


def test_a_filter_that_removes_one_record_changes_that_junctions_row(three_formats, tmp_path):
    interval, mrf, paths, reads = three_formats
    rows, _ = J.table(interval, mrf)
    ix = index_of(paths)
    last = len(reads) - 1
    lone = ("chr1", 3100, 3200, "+", 1, 1, 0, 50)
    assert lone in rows
    for name, kw, env in (("mapq", dict(mapq={last: 3}), {"LSQ_SAM_MIN_MAPQ": "4"}), ("flag", dict(flags={last: 0x400}), {"LSQ_SAM_SKIP_FLAGS": str(0x904 | 0x400)})):
        sam = sam_of(reads, **kw).encode()
        path = str(tmp_path / (name + ".sam"))
        open(path, "wb").write(sam)
        opts = dict(min_mapq=4) if name == "mapq" else dict(skip_flags=0x904 | 0x400)
        assert ix.host("SAM_SINGLE", path).rows() == rows                       # the defaults keep the record
        got = ix.host("SAM_SINGLE", path, **opts).rows()
        assert got == [r for r in rows if r != lone]
        want, _ = J.table(interval, L.sam_to_mrf(sam, **opts).decode())
        assert got == want
        bam = str(tmp_path / (name + ".bam"))
        open(bam, "wb").write(bam_writer.sam_to_bam(sam))
        assert ix.host("BAM_SINGLE", bam, **opts).rows() == got
        p = tool(paths, path, "SAM_SINGLE", env=env)
        assert p.returncode == 0 and p.stdout == J.text(got)
    # one occurrence fewer of a junction many reads have: that row's counts alone
    sam = sam_of(reads, mapq={0: 0}).encode()
    path = str(tmp_path / "first.sam")
    open(path, "wb").write(sam)
    got = ix.host("SAM_SINGLE", path, min_mapq=1).rows()
    diff = [(a, b) for a, b in zip(rows, got) if a != b]
    assert len(got) == len(rows) and len(diff) == 2 and all(a[:4] == b[:4] and a[4] - 1 == b[4] and a[5] - 1 == b[5] for a, b in diff)


def test_ucsc_gff_reads_one_line_per_block(base, tmp_path):
    interval, _, paths = base
    reads = [("n1", "chr1", "+", [(150, 200), (300, 350)]), ("n2", "chr1", "-", [(160, 200), (300, 350), (500, 520)]), ("n3", "chr2", "+", [(150, 200)]),
             ("n4", "chr1", "+", [(150, 200), (200, 250)])]
    lines = ["track name=x\n", "browser position chr1\n"]
    blocks = [(n, c, s, b) for n, c, s, bl in reads for b in bl]
    # lines of one name need not be neighbours: n2's last block comes at the end of the file
    blocks = [b for b in blocks if b != ("n2", "chr1", "-", (500, 520))] + [("n2", "chr1", "-", (500, 520))]
    for n, c, s, (a, b) in blocks:
        lines.append("%s\tsrc\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (c, a + 1, b, s, n))
    path = str(tmp_path / "reads.gff")
    open(path, "w").write("".join(lines))
    mrf = "AlignmentBlocks\n" + "".join(J.mrf_line(c, s, bl) for _, c, s, bl in reads)
    rows, report = J.table(interval, mrf)
    got = index_of(paths).host("UCSC_GFF", path)
    same(got, rows, report)
    assert [r[:5] for r in rows] == [("chr1", 200, 300, "+", 2), ("chr1", 350, 500, ".", 1)]
    p = tool(paths, path, "UCSC_GFF")
    assert p.returncode == 0 and p.stdout == J.text(rows)


def test_a_malformed_line_gives_counts_status_and_message(base, tmp_path):
    _, _, paths = base
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
    sam = "@HD\tVN:1.6\n" + "q\t0\tchr1\t101\t60\t50M10N50M\t*\t0\t0\t*\t*\n" * 7 + "q\t0\tchr1\t101\t60\t50Q\t*\t0\t0\t*\t*\n"
    spath = str(tmp_path / "bad.sam")
    open(spath, "w").write(sam)
    with pytest.raises(L.LsqError) as e:
        ix.host("SAM_SINGLE", spath)
    assert e.value.status == LSQ_E_PARSE and ": #9:q\t0\tchr1\t101\t60\t50Q" in str(e.value)
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_PAIRED", path)
    assert e.value.status == -3 and str(e.value).endswith("Unknown file format error: MRF_PAIRED")
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_SINGLE", str(tmp_path / "missing.mrf"))
    assert e.value.status == -2
    p = tool(paths, str(tmp_path / "missing.mrf"))
    assert p.returncode == 1 and p.stdout == ""


def test_threads_do_not_change_the_table(tmp_path):
    iso, lines = J.sort_case(131073, True)
    interval, mrf, paths = J.write_case(str(tmp_path), "big", iso, lines)
    rows, report = J.table(interval, mrf)
    ix = index_of(paths)
    for n_threads in (1, 3, 16):
        same(ix.host("MRF_SINGLE", paths["mrf"], n_threads=n_threads), rows, report)
    reads = ix.parse_host("MRF_SINGLE", paths["mrf"])
    same(ix.host_reads(reads, n_threads=5), rows, report)
    assert [r[0] for r in rows if r[0] in ("c000", "c255", "c256", "c300")][-3:] == ["c255", "c256", "c300"]


def test_new_entry_points_are_exported_and_the_abi_version_stays():
    syms = ("lsq_jn_index_build", "lsq_jn_index_free", "lsq_jn_index_num_chroms", "lsq_jn_index_chrom_name", "lsq_jn_index_num_introns", "lsq_jn_index_dictionaries",
            "lsq_jn_host", "lsq_jn_host_reads", "lsq_jn_device", "lsq_jn_table_free", "lsq_jn_table_rows", "lsq_jn_table_arrays", "lsq_jn_table_report",
            "lsq_jn_table_times", "lsq_jn_format", "lsq_jn_sort_tile")
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in syms:
        assert hasattr(L.lib, sym), sym
        assert sym + "(" in header, sym
    assert L.lib.lsq_abi_version() == 2 and "#define LSQ_ABI_VERSION 2" in header
    assert os.access(os.path.join(BIN, "junctions"), os.X_OK)
    assert L.junctions.SORT_TILE >= 1024
