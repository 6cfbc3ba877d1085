"""Reads per exon bin and per gene without a GPU (include/lesseq_hip.h, lsq_xb_*): lsq_xb_host and `exonbins --host` against the
definition as tests/exonbins_ref.py restates it.  All values are integers: the tables equal the reference's exactly."""
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
import bam_writer
import exonbins_ref as V
from lesseq_amd import diffsplice as ds
from test_junctions_host import sam_of, log_messages

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "lesseq_amd", "bin")
TOY = os.path.join(HERE, "golden", "toy")
LSQ_E_PARSE = -4
USAGE = "Usage:\nexonbins [--host] [--bins prefix] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]"
TOY_TABLE = "RI1\t4\tRI1:1\t3\nRI1\t4\tRI1:2\t1\nRI1\t4\tRI1:3\t2\nSE1\t8\tSE1:1\t5\nSE1\t8\tSE1:2\t3\nSE1\t8\tSE1:3\t3\n"
TOY_REPORT = {"reads": 13, "blocks": 17, "no_chromosome_or_empty": 1, "no_gene": 1, "several_genes": 0, "bin_hits": 17}


def index_of(paths):
    return L.ExonBinIndex(L.Annotation(paths["interval"], paths["map"]))


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None, host=True, timeout=None, out=None):
    argv = ([os.path.join(BIN, "exonbins")] + (["--host"] if host else []) + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads] +
            ([out] if out else []))
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=timeout)


def same(got, want):
    rows, report = want
    assert got.rows() == rows
    assert got.report == report
    assert got.text() == V.text(rows)
    assert int(got.reads.sum()) == report["bin_hits"] and len(got.total) == got.index.num_genes


def toy_paths():
    return {"interval": os.path.join(TOY, "toy.interval"), "map": os.path.join(TOY, "toy.map"), "mrf": os.path.join(TOY, "toy.mrf")}


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("xb"))
    interval, mrf, paths = V.write_case(d, "base", V.definition_annotation(), V.definition_lines())
    return interval, open(paths["map"]).read(), mrf, paths


# ----------------------------------------------------------------------------- the worked example

def test_the_toy_example_byte_for_byte():
    paths = toy_paths()
    texts = [open(paths[k]).read() for k in ("interval", "map", "mrf")]
    want = V.table(*texts)
    assert V.text(want[0]) == TOY_TABLE and want[1] == TOY_REPORT
    ix = index_of(paths)
    assert ix.bins() == [("RI1:1", "chr1", "+", 5000, 5200), ("RI1:2", "chr1", "+", 5200, 5300), ("RI1:3", "chr1", "+", 5300, 5500),
                         ("SE1:1", "chr1", "+", 1000, 1100), ("SE1:2", "chr1", "+", 1200, 1300), ("SE1:3", "chr1", "+", 1500, 1600)]
    got = ix.host("MRF_SINGLE", paths["mrf"])
    same(got, want)
    assert got.text() == TOY_TABLE and got.report == TOY_REPORT
    # gene order: count's, for the same two files
    count_genes = list(dict.fromkeys(ln.split("\t")[0] for ln in open(os.path.join(TOY, "count.out"))))
    assert list(dict.fromkeys(r[0] for r in got.rows())) == count_genes == ix.gene_names()
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == TOY_TABLE
    assert V.report_line(TOY_REPORT, 6, 2) in p.stderr


# ----------------------------------------------------------------------------- bins

def test_bin_construction(base):
    interval, gmap, _, paths = base
    genes = V.genes_of(interval, gmap)
    ix = index_of(paths)
    assert ix.bins() == V.bin_rows(genes)
    assert ix.gene_names() == [g[0] for g in genes] == sorted(ix.gene_names(), key=lambda n: n.encode()) and ix.gene_names()[0] == "Zlast"
    by_gene = {g[0]: g for g in genes}
    # worked out by hand
    assert by_gene["mix"][3] == [(1000, 1050), (1050, 1100), (1100, 1150), (1150, 1200), (1300, 1350), (1350, 1400), (1400, 1500), (1600, 1650), (1700, 1800)]
    assert by_gene["neg"][3] == [(-500, -450), (-450, -400), (-400, -350), (-300, -200), (-20, 30)] and by_gene["neg"][2] == "-"
    assert by_gene["ovB"][3] == [(200, 250), (250, 350), (350, 400), (600, 800)] and by_gene["ovB"][2] == "."
    assert len(by_gene["big"][3]) == 70 and by_gene["big"][3] == V.BIG
    assert by_gene["edge"][3] == [(V.LIM - 100, V.LIM + 50), (V.LIM + 100, V.LIM + 200)]
    # the arrays
    first = ix.gene_first_bin
    assert ix.num_bins == sum(len(g[3]) for g in genes) == len(ix.bin_start) and ix.num_genes == len(genes) and len(first) == len(genes) + 1 and first[-1] == ix.num_bins
    assert ix.bin_start.dtype == np.int64 and ix.bin_start.tolist() == [s for g in genes for s, _ in g[3]] and ix.bin_end.tolist() == [e for g in genes for _, e in g[3]]
    assert ix.bin_gene.tolist() == [k for k, g in enumerate(genes) for _ in g[3]]
    assert [ix.chrom_names()[c] for c in ix.gene_chrom] == [g[1] for g in genes]
    assert ix.chrom_names() == ["chr1", "chr2", "chr3", "chr4"]


def test_host_equals_the_reference_on_the_definition_cases(base):
    interval, gmap, mrf, paths = base
    want = V.table(interval, gmap, mrf)
    rows, report = want
    ix = index_of(paths)
    same(ix.host("MRF_SINGLE", paths["mrf"]), want)
    same(ix.host_reads(ix.parse_host("MRF_SINGLE", paths["mrf"]), n_threads=3), want)
    n = {r[2]: r[3] for r in rows}
    total = {r[0]: r[1] for r in rows}
    # the cases are there, worked out by hand on the reads of chr2 and chr3
    assert [n["ovA:%d" % k] for k in (1, 2)] == [4, 2] and total["ovA"] == 5
    assert [n["ovB:%d" % k] for k in (1, 2, 3, 4)] == [1, 2, 1, 2] and total["ovB"] == 4
    assert total["ovC"] == 2 and total["ovD"] == 3 and n["ovD:2"] == 2 and n["neg:3"] == n["neg:4"] == 0 and n["neg:5"] == 1
    assert n["big:1"] == 1 and n["big:4"] == 2 and n["big:30"] == 2 and total["big"] == 3
    assert n["edge:1"] == 1 and n["edge:2"] == 0 and n["Zlast:1"] == 2
    assert report["no_chromosome_or_empty"] == 6 and report["several_genes"] == 7 and report["reads"] == len(V.definition_lines()) - 1
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == V.text(rows) and V.report_line(report, len(rows), ix.num_genes) in p.stderr


def test_overlapping_genes_and_the_numpy_reference(tmp_path):
    iso, lines = V.overlap_case(3000)
    interval, mrf, paths = V.write_case(str(tmp_path), "overlap", iso, lines)
    gmap = open(paths["map"]).read()
    want = V.table(interval, gmap, mrf)
    assert V.table_of_one_block_reads(interval, gmap, mrf) == want
    same(index_of(paths).host("MRF_SINGLE", paths["mrf"]), want)
    assert want[1]["several_genes"] > 2000 and want[1]["no_gene"] > 10


def test_empty_inputs(base, tmp_path):
    interval, gmap, _, _ = base
    for stem, lines, header in (("header_only", [], "AlignmentBlocks\n"), ("nothing", [], ""), ("none_hit", [V.mrf_line("chrU", "+", [(1, 9)])] * 3, "AlignmentBlocks\n")):
        _, mrf, paths = V.write_case(str(tmp_path), stem, V.definition_annotation(), lines, header)
        want = V.table(interval, gmap, mrf)
        got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
        same(got, want)
        assert len(got) > 90 and not got.reads.any() and not got.total.any() and got.report["reads"] == len(lines) == got.report["no_gene"]
        p = tool(paths, paths["mrf"])
        assert p.returncode == 0 and p.stdout == V.text(want[0]) and len(p.stdout.split("\n")) == len(got) + 1      # every bin is printed, zeros included


def test_a_gene_on_two_chromosomes(tmp_path):
    iso = [V.interval_line("a.1", "chr1", "+", [(100, 200)]), V.interval_line("two.1", "chr1", "+", [(100, 200)]), V.interval_line("two.2", "chr2", "+", [(100, 200)]),
           V.interval_line("zz.1", "chr1", "+", [(100, 200)]), V.interval_line("zz.2", "chr3", "+", [(100, 200)])]
    interval, mrf, paths = V.write_case(str(tmp_path), "two", iso, [V.mrf_line("chr1", "+", [(100, 150)])])
    with pytest.raises(ValueError):
        V.genes_of(interval, open(paths["map"]).read())
    with pytest.raises(L.LsqError) as e:
        index_of(paths)
    assert "gene two " in str(e.value) and "zz" not in str(e.value)
    prefix, out = str(tmp_path / "bins"), str(tmp_path / "out.tab")
    p = tool(paths, paths["mrf"], opts=["--bins", prefix], out=out)
    assert p.returncode == 1 and p.stdout == "" and "gene two " in p.stderr and "zz" not in p.stderr
    assert not os.path.exists(out) and not os.path.exists(prefix + ".interval") and not os.path.exists(prefix + ".map")


# ----------------------------------------------------------------------------- formats, threads

def random_files(d):
    iso, reads = V.random_case()
    interval, mrf, paths = V.write_case(d, "rnd", iso, [V.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads])
    sam = sam_of(reads, mapq={0: 3, 7: 3}).encode()
    paths["sam"], paths["bam"] = os.path.join(d, "rnd.sam"), os.path.join(d, "rnd.bam")
    open(paths["sam"], "wb").write(sam)
    open(paths["bam"], "wb").write(bam_writer.sam_to_bam(sam, "cut61"))
    gmap = open(paths["map"]).read()
    return paths, V.table(interval, gmap, mrf), V.table(interval, gmap, L.sam_to_mrf(sam, min_mapq=4).decode())


def test_one_table_from_mrf_sam_and_bam(tmp_path):
    paths, want, fewer = random_files(str(tmp_path))
    ix = index_of(paths)
    assert 300 <= ix.num_bins <= 500 and ix.num_genes == 40 and want[1]["reads"] == 5000
    assert want[1]["several_genes"] > 100 and want[1]["no_gene"] > 100 and want[1]["no_chromosome_or_empty"] > 100
    for fmt, key in (("MRF_SINGLE", "mrf"), ("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam")):
        same(ix.host(fmt, paths[key]), want)
    assert fewer[1]["reads"] == 4998 and fewer != want
    for fmt, key in (("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam")):
        same(ix.host(fmt, paths[key], min_mapq=4), fewer)
        p = tool(paths, paths[key], fmt, env={"LSQ_SAM_MIN_MAPQ": "4"})
        assert p.returncode == 0 and p.stdout == V.text(fewer[0])
    p = tool(paths, paths["bam"], "BAM_SINGLE", env={"LSQ_BAM_VERIFY": "1"})
    assert p.returncode == 0 and p.stdout == V.text(want[0])


def test_ucsc_gff_reads_one_line_per_block(base, tmp_path):
    interval, gmap, _, paths = base
    reads = [("n1", "chr1", "+", [(1010, 1060), (1310, 1360)]), ("n2", "chr2", "-", [(650, 750), (150, 250)]), ("n3", "chr4", "+", V.BIG[:5])]
    lines = ["track name=x\n", "browser position chr1\n"]      # (the format has two header lines)
    for n, c, s, bl in reads:
        for a, b in bl:
            lines.append("%s\tsrc\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (c, a + 1, b, s, n))
    path = str(tmp_path / "reads.gff")
    open(path, "w").write("".join(lines))
    want = V.table(interval, gmap, "AlignmentBlocks\n" + "".join(V.mrf_line(c, s, bl) for _, c, s, bl in reads))
    same(index_of(paths).host("UCSC_GFF", path), want)
    p = tool(paths, path, "UCSC_GFF")
    assert p.returncode == 0 and p.stdout == V.text(want[0]) and want[1]["bin_hits"] == 13


def test_threads_do_not_change_the_table(tmp_path):
    iso, lines = V.hot_case(True, 70000, 1000)
    interval, mrf, paths = V.write_case(str(tmp_path), "big", iso, lines)
    want = V.table_of_one_block_reads(interval, open(paths["map"]).read(), mrf)
    ix = index_of(paths)
    for n_threads in (1, 3, 16):
        same(ix.host("MRF_SINGLE", paths["mrf"], n_threads=n_threads), want)
    same(ix.host_reads(ix.parse_host("MRF_SINGLE", paths["mrf"]), n_threads=5), want)
    assert want[1]["reads"] > 1 << 16


# ----------------------------------------------------------------------------- the executable's files

def test_the_bins_files_are_an_annotation_coverage_reads(base, tmp_path):
    interval, gmap, mrf, paths = base
    genes = V.genes_of(interval, gmap)
    ix = index_of(paths)
    assert ix.bins_text() == V.bins_texts(genes)
    prefix, out = str(tmp_path / "bins"), str(tmp_path / "t.tab")
    p = tool(paths, paths["mrf"], opts=["--bins", prefix], out=out)
    rows, _ = V.table(interval, gmap, mrf)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == V.text(rows)
    iv, mp = open(prefix + ".interval").read(), open(prefix + ".map").read()
    assert (iv, mp) == V.bins_texts(genes)
    # every line parses: the loader takes the pair, a gene per gene and a line per bin
    a = L.Annotation(prefix + ".interval", prefix + ".map")
    assert L.lib.lsq_annotation_num_genes(a.h) == len(genes) and L.lib.lsq_annotation_num_isoforms_loaded(a.h) == len(rows)
    again = L.ExonBinIndex(a)          # the bins of the bins are the bins
    assert [b[1:] for b in again.bins()] == [b[1:] for b in ix.bins()]
    regions = str(tmp_path / "depth.tsv")
    argv = [os.path.join(BIN, "coverage"), "--host", "--regions", regions, "LH_GENE_TXT", prefix + ".interval", "UCSC_GENE2ISOFORM", prefix + ".map", "MRF_SINGLE", paths["mrf"]]
    c = subprocess.run(argv, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    lines = open(regions).read().splitlines()
    assert [ln.split("\t")[0] for ln in lines] == [r[2] for r in rows]
    depth = {ln.split("\t")[0]: ln.split("\t") for ln in lines}
    assert depth["mix:1"][3] == "50" and int(depth["mix:1"][5]) > 0 and depth["edge:2"][4:6] == ["0", "0"]


def test_two_samples_make_an_lrt_input(base, tmp_path):
    interval, gmap, mrf, paths = base
    a, b = str(tmp_path / "a.tab"), str(tmp_path / "b.tab")
    assert tool(paths, paths["mrf"], out=a).returncode == 0
    _, mrf2, paths2 = V.write_case(str(tmp_path), "second", V.definition_annotation(), V.definition_lines()[::2])
    assert tool(paths2, paths2["mrf"], out=b).returncode == 0
    ra, rb = V.table(interval, gmap, mrf)[0], V.table(interval, gmap, mrf2)[0]
    assert [r[2] for r in ra] == [r[2] for r in rb] and ra != rb                   # the same rows, other counts
    inp = ds.read_tables("lrt", [a, a, b, b], 2, 2)
    assert inp.ids == [r[2] for r in ra] and inp.values.shape == (len(ra), 4) == inp.totals.shape
    assert inp.values.tolist() == [[x[3], x[3], y[3], y[3]] for x, y in zip(ra, rb)]
    assert inp.totals.tolist() == [[x[1], x[1], y[1], y[1]] for x, y in zip(ra, rb)]


def test_the_tool_takes_an_output_path_and_refuses_nonsense(base, tmp_path):
    interval, gmap, mrf, paths = base
    rows, report = V.table(interval, gmap, mrf)
    p = tool(paths, paths["mrf"], out="-")
    assert p.returncode == 0 and p.stdout == V.text(rows)
    assert log_messages(p.stderr) == [("INFO", V.report_line(report, len(rows), index_of(paths).num_genes))]
    for bad in (["--bins"], ["--nonsense"], ["--strand", "+"]):
        p = tool(paths, paths["mrf"], opts=bad)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], bad
    positional = ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"]]
    # --bins at the end of the line has no value; five and eight positional arguments
    for argv in (positional + ["--bins"], positional[:5], positional + ["-", "-"]):
        p = subprocess.run([os.path.join(BIN, "exonbins"), "--host"] + argv, capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], argv
    # everything is formatted before anything is written, and the bins' files come first: a prefix that cannot be written leaves no file
    prefix, out = str(tmp_path / "no_such_directory" / "bins"), str(tmp_path / "t.tab")
    p = tool(paths, paths["mrf"], opts=["--bins", prefix], out=out)
    assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr)[-1] == ("ERROR", "cannot write " + prefix + ".interval")
    assert not os.path.exists(out) and os.listdir(str(tmp_path)) == []


def test_a_malformed_record_gives_counts_status_and_message(base, tmp_path):
    _, _, _, paths = base
    good = V.mrf_line("chr1", "+", [(1010, 1060), (1310, 1360)])
    bad = "chr1:+:15x:200:1:50"
    path = str(tmp_path / "bad.mrf")
    open(path, "w").write("AlignmentBlocks\n" + good * 40 + bad + "\n" + good * 3)
    ix = index_of(paths)
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_SINGLE", path)
    assert e.value.status == LSQ_E_PARSE and str(e.value).endswith(": #41:" + bad)
    prefix, out = str(tmp_path / "never"), str(tmp_path / "never.tab")
    p = tool(paths, path, opts=["--bins", prefix], out=out)
    assert p.returncode == 1 and p.stdout == "" and "#41:" + bad in p.stderr and "Lexical_cast error" in p.stderr
    assert not os.path.exists(prefix + ".interval") and not os.path.exists(prefix + ".map") and not os.path.exists(out)
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_PAIRED", path)
    assert e.value.status == -3
    p = tool(paths, str(tmp_path / "missing.mrf"))
    assert p.returncode == 1 and p.stdout == ""


def test_new_entry_points_are_exported_and_the_abi_version_stays():
    syms = ("lsq_xb_index_build", "lsq_xb_index_free", "lsq_xb_index_num_chroms", "lsq_xb_index_num_genes", "lsq_xb_index_num_bins", "lsq_xb_index_chrom_name",
            "lsq_xb_index_gene_name", "lsq_xb_index_gene_strand", "lsq_xb_index_dictionaries", "lsq_xb_index_arrays", "lsq_xb_host", "lsq_xb_host_reads", "lsq_xb_device",
            "lsq_xb_table_free", "lsq_xb_table_arrays", "lsq_xb_table_report", "lsq_xb_table_times", "lsq_xb_format", "lsq_xb_format_bins")
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in syms:
        assert hasattr(L.lib, sym), sym
        assert sym + "(" in header, sym
    assert L.lib.lsq_abi_version() == 2 and "#define LSQ_ABI_VERSION 2" in header
    assert os.access(os.path.join(BIN, "exonbins"), os.X_OK)
    assert L.ExonBinIndex is L.exonbins.ExonBinIndex and L.ExonBins is L.exonbins.ExonBins
    rc, text = L.cli_run("exonbins", ["--nonsense"])
    assert rc == 1 and text == ""
