"""Junction reads per event form without a GPU (include/lesseq_hip.h, lsq_ps_*): lsq_ps_host and `psi --host` against the
definition as tests/psi_ref.py restates it.  All values are integers, psi is a fixed order of double operations on them: the tables
equal the reference's exactly, as numbers and as text."""
import math
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
import bam_writer
import psi_ref as V
from lesseq_amd import diffsplice as ds
from test_junctions_host import sam_of, log_messages

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "lesseq_amd", "bin")
GOLD = os.path.join(HERE, "golden")
LSQ_E_ARG, LSQ_E_PARSE = -1, -4
USAGE = "Usage:\npsi [--host] [--psi] [--min-overhang N] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]"
TOY_TABLE = "RI1\t1\tRI1.ret\t0\nRI1\t1\tRI1.spl\t1\nSE1\t3\tSE1.inc\t2\nSE1\t3\tSE1.skp\t1\n"
TOY_PSI_TABLE = "RI1\t1\tRI1.ret\t0\t0\tNA\nRI1\t1\tRI1.spl\t1\t1\tNA\nSE1\t3\tSE1.inc\t2\t2\t0.500000\nSE1\t3\tSE1.skp\t1\t1\t0.500000\n"
TOY_REPORT = {"reads": 13, "blocks": 17, "occurrences": 4, "dropped_overhang": 0, "no_chromosome": 0, "informative_occurrences": 4, "counted": 4, "several_events": 0}


def index_of(paths):
    return L.PsiIndex(L.Annotation(paths["interval"], paths["map"]))


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None, host=True, timeout=None, out=None):
    argv = ([os.path.join(BIN, "psi")] + (["--host"] if host else []) + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads] +
            ([out] if out else []))
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=timeout)


def same(got, want):
    rows, report, introns = want
    assert got.rows() == rows
    assert got.report == report
    assert got.index.form_introns.tolist() == introns
    assert got.text() == V.text(rows) and got.text(psi=True) == V.text(rows, introns)
    psi = got.psi()
    assert psi.dtype == np.float64 and [None if math.isnan(p) else p for p in psi.tolist()] == V.psi_of(rows, introns)
    assert len(got.total) == got.index.num_events and len(got) == got.index.num_forms == len(rows)


def toy_paths():
    d = os.path.join(GOLD, "toy")
    return {"interval": os.path.join(d, "toy.interval"), "map": os.path.join(d, "toy.map"), "mrf": os.path.join(d, "toy.mrf"), "count": os.path.join(d, "count.out")}


def s1_paths():
    d = os.path.join(GOLD, "events_s1")
    return {"interval": os.path.join(d, "ev.interval"), "map": os.path.join(d, "ev.map"), "mrf": os.path.join(d, "ev.mrf"), "count": os.path.join(d, "count.out")}


def want_of(paths, min_overhang=1):
    return V.table(*[open(paths[k]).read() for k in ("interval", "map", "mrf")], min_overhang=min_overhang)


def random_files(d):
    iso, reads = V.random_case()
    interval, mrf, paths = V.write_case(d, "rnd", iso, [V.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads])
    sam = sam_of(reads, mapq={0: 3, 7: 3}).encode()
    paths["sam"], paths["bam"] = os.path.join(d, "rnd.sam"), os.path.join(d, "rnd.bam")
    open(paths["sam"], "wb").write(sam)
    open(paths["bam"], "wb").write(bam_writer.sam_to_bam(sam, "cut61"))
    gmap = open(paths["map"]).read()
    return paths, V.table(interval, gmap, mrf), V.table(interval, gmap, L.sam_to_mrf(sam, min_mapq=4).decode())


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ps"))
    interval, mrf, paths = V.write_case(d, "base", V.definition_annotation(), V.definition_lines())
    return interval, open(paths["map"]).read(), mrf, paths


@pytest.fixture(scope="module")
def formats(tmp_path_factory):
    return random_files(str(tmp_path_factory.mktemp("psrnd")))


# ----------------------------------------------------------------------------- the worked examples, the reference itself

def test_the_reference_on_the_toy_example():
    rows, report, introns = want_of(toy_paths())
    assert V.text(rows) == TOY_TABLE and V.text(rows, introns) == TOY_PSI_TABLE and report == TOY_REPORT


def test_the_reference_on_the_hand_worked_definition_cases(base):
    interval, gmap, mrf, _ = base
    rows, report, introns = V.table(interval, gmap, mrf)
    assert rows == V.DEFINITION_ROWS and introns == V.DEFINITION_INTRONS and report == V.DEFINITION_REPORT
    assert [ln.split("\t")[5] for ln in V.text(rows, introns).splitlines()] == V.DEFINITION_PSI
    by_form = {f: d for _, forms in V.events_of(interval, gmap) for f, d in forms}
    # the intron all three forms hold is informative in none; A.1 and A.2 share one; the union of overlapping exons; the range's end
    assert by_form["A.3"] == set() and by_form["A.2"] == {("chr1", 400, 500)} and by_form["A.1"] == {("chr1", 400, 500), ("chr1", 600, 700)}
    assert by_form["UN.a"] == {("chr1", 5200, 5300)} and by_form["UN.b"] == {("chr1", 5100, 5300)} and by_form["ONE.a"] == set()
    assert by_form["OV1.a"] == {("chr1", 2100, 2200)} <= by_form["OV2.a"] and by_form["EDGE.a"] == {("chr1", V.LIM - 200, V.LIM - 150)}


def test_the_toy_example_byte_for_byte():
    paths = toy_paths()
    ix = index_of(paths)
    got = ix.host("MRF_SINGLE", paths["mrf"])
    same(got, want_of(paths))
    assert got.text() == TOY_TABLE and got.text(psi=True) == TOY_PSI_TABLE and got.report == TOY_REPORT
    assert ix.event_names() == ["RI1", "SE1"] and ix.form_names() == ["RI1.ret", "RI1.spl", "SE1.inc", "SE1.skp"]
    assert ix.event_first_form.tolist() == [0, 2, 4] and ix.form_introns.tolist() == [0, 1, 2, 1] and ix.num_introns == 4 and ix.chrom_names() == ["chr1"]
    p = tool(paths, paths["mrf"], opts=["--psi"])
    assert p.returncode == 0 and p.stdout == TOY_PSI_TABLE
    assert log_messages(p.stderr) == [("INFO", V.report_line(TOY_REPORT, 4, 4, 2))]


def test_events_s1_and_the_order_of_counts_table():
    paths = s1_paths()
    want = want_of(paths)
    ix = index_of(paths)
    got = ix.host("MRF_SINGLE", paths["mrf"])
    same(got, want)
    lines = {ln.split("\t")[2]: ln.split("\t") for ln in got.text(psi=True).splitlines()}
    assert lines["15.a"] == ["15", "9", "15.a", "4", "2", "0.285714"] and lines["15.b"] == ["15", "9", "15.b", "5", "1", "0.714286"]
    assert lines["1.a"][1:] == ["0", "1.a", "0", "0", "NA"] and lines["1.b"][1:] == ["0", "1.b", "0", "0", "NA"]
    assert ix.num_events == 40 and want[1]["reads"] == 1500 and want[1]["counted"] > 100
    for q in (toy_paths(), paths):         # events and forms as count prints them
        count = [ln.split("\t") for ln in open(q["count"]).read().splitlines()]
        assert [(r[0], r[2]) for r in index_of(q).host("MRF_SINGLE", q["mrf"]).rows()] == [(c[0], c[2]) for c in count]
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == V.text(want[0])


# ----------------------------------------------------------------------------- the definition

def test_host_equals_the_reference_on_the_definition_cases(base):
    interval, gmap, mrf, paths = base
    want = V.table(interval, gmap, mrf)
    ix = index_of(paths)
    same(ix.host("MRF_SINGLE", paths["mrf"]), want)
    same(ix.host_reads(ix.parse_host("MRF_SINGLE", paths["mrf"]), n_threads=3), want)
    assert ix.event_names() == sorted(ix.event_names(), key=lambda n: n.encode()) and ix.num_introns == 13
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == V.text(want[0]) and V.report_line(want[1], 13, 18, 9) in p.stderr
    p = tool(paths, paths["mrf"], opts=["--psi"])
    assert p.returncode == 0 and p.stdout == V.text(want[0], want[2])
    assert [ln.split("\t")[5] for ln in p.stdout.splitlines()] == V.DEFINITION_PSI


def test_forms_come_in_the_maps_order_not_the_interval_files(tmp_path):
    iso = V.definition_annotation()
    interval, mrf, paths = V.write_case(str(tmp_path), "order", iso[::-1], V.definition_lines())
    gmap = V.map_of(iso)
    open(paths["map"], "w").write(gmap)
    want = V.table(interval, gmap, mrf)
    assert want[0] == V.DEFINITION_ROWS
    same(index_of(paths).host("MRF_SINGLE", paths["mrf"]), want)


def test_a_form_the_map_alone_names_and_an_event_without_forms(base, tmp_path):
    interval, gmap, mrf, paths = base
    # an isoform without a line is the loader's error, as for count and every other tool
    only = dict(paths, map=str(tmp_path / "only.map"))
    open(only["map"], "w").write(gmap + "SE\tSE.ghost\n")
    with pytest.raises(L.LsqError) as e:
        index_of(only)
    assert e.value.status == LSQ_E_ARG and "SE.ghost" in str(e.value)
    p = tool(only, paths["mrf"])
    assert p.returncode == 1 and p.stdout == "" and "SE.ghost" in p.stderr
    # an event the map gives no isoform: no form, no row, and the other events as they were
    worm = str(tmp_path / "worm.map")
    groups = {}
    for ln in gmap.splitlines():
        groups.setdefault(ln.split("\t")[0], []).append(ln.split("\t")[1])
    open(worm, "w").write("".join("%s\t%s\n" % (g, ";".join(f)) for g, f in groups.items()) + "NONE\t;\n")
    ix = L.PsiIndex(L.Annotation(paths["interval"], worm, g2i_format="WORMBASE_GENE2ISOFORMS"))
    got = ix.host("MRF_SINGLE", paths["mrf"])
    assert "NONE" in ix.event_names() and ix.num_events == 10 and got.rows() == V.DEFINITION_ROWS and got.text(psi=True) == V.text(V.DEFINITION_ROWS, V.DEFINITION_INTRONS)


def test_host_equals_the_reference_on_a_random_case(formats):
    paths, want, fewer = formats
    ix = index_of(paths)
    assert ix.num_events == 40 and want[1]["reads"] == 5000 and want[1]["counted"] > 1500 and want[1]["several_events"] > 50
    assert want[1]["no_chromosome"] > 50 and want[1]["occurrences"] > want[1]["informative_occurrences"] > 1500 and 0 in want[2] and max(want[2]) >= 3
    for fmt, key in (("MRF_SINGLE", "mrf"), ("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam")):
        same(ix.host(fmt, paths[key]), want)
    assert fewer[1]["reads"] == 4998 and fewer != want
    for fmt, key in (("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam")):
        same(ix.host(fmt, paths[key], min_mapq=4), fewer)
        p = tool(paths, paths[key], fmt, opts=["--psi"], env={"LSQ_SAM_MIN_MAPQ": "4"})
        assert p.returncode == 0 and p.stdout == V.text(fewer[0], fewer[2])
    p = tool(paths, paths["bam"], "BAM_SINGLE", env={"LSQ_BAM_VERIFY": "1"})
    assert p.returncode == 0 and p.stdout == V.text(want[0])
    texts = [open(paths[k]).read() for k in ("interval", "map", "mrf")]
    assert V.fast_table(*texts) == want and V.fast_table(*texts, min_overhang=30) == V.table(*texts, min_overhang=30)       # the second reference is the first
    for n in (2, 30):
        w = V.table(open(paths["interval"]).read(), open(paths["map"]).read(), open(paths["mrf"]).read(), min_overhang=n)
        same(ix.host("MRF_SINGLE", paths["mrf"], min_overhang=n), w)
        assert w[1]["dropped_overhang"] > 0 and w != want


# ----------------------------------------------------------------------------- the junction rule

@pytest.mark.parametrize("n", [1, 10, 25])
def test_the_junction_rules_edges(tmp_path, n):
    cases = V.rule_lines(n)
    interval, mrf, paths = V.write_case(str(tmp_path), "rule", V.definition_annotation(), [ln for ln, _ in cases])
    gmap = open(paths["map"]).read()
    ix = index_of(paths)
    for m in sorted({1, max(1, n - 1), n, n + 1}):
        want = V.table(interval, gmap, mrf, min_overhang=m)
        same(ix.host("MRF_SINGLE", paths["mrf"], min_overhang=m), want)
        p = tool(paths, paths["mrf"], opts=["--min-overhang", str(m)])
        assert p.returncode == 0 and p.stdout == V.text(want[0])
        if m == n:         # worked out by hand: which of the lines count for SE.skp at overhang n
            skp = {r[2]: r[3] for r in want[0]}["SE.skp"]
            assert skp == sum(counts for _, counts in cases) == 5 and want[1]["no_chromosome"] == 1
            # every line alone
            for ln, counts in cases:
                rows, _, _ = V.table(interval, gmap, "AlignmentBlocks\n" + ln, min_overhang=n)
                assert {r[2]: r[3] for r in rows}["SE.skp"] == int(counts), ln
    if n > 1:
        assert V.table(interval, gmap, mrf, min_overhang=n - 1)[1]["dropped_overhang"] < V.table(interval, gmap, mrf, min_overhang=n)[1]["dropped_overhang"]
    assert max(len(r) for r in V.mrf_reads(mrf)) == 16


def test_min_overhang_zero_is_an_argument_error(base):
    _, _, _, paths = base
    ix = index_of(paths)
    for call in (lambda: ix.host("MRF_SINGLE", paths["mrf"], min_overhang=0), lambda: ix.host_reads(ix.parse_host("MRF_SINGLE", paths["mrf"]), min_overhang=0)):
        with pytest.raises(L.LsqError) as e:
            call()
        assert e.value.status == LSQ_E_ARG and "min_overhang" in str(e.value)
    p = tool(paths, paths["mrf"], opts=["--min-overhang", "0"])
    assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)]


# ----------------------------------------------------------------------------- text, the executable

def test_text_columns_and_na_rules(base, tmp_path):
    interval, gmap, mrf, paths = base
    got = index_of(paths).host("MRF_SINGLE", paths["mrf"])
    four, six = got.text().splitlines(), got.text(psi=True).splitlines()
    assert all(len(ln.split("\t")) == 4 for ln in four) and all(len(ln.split("\t")) == 6 for ln in six) and len(four) == len(six) == 18
    assert [ln.split("\t")[:4] for ln in six] == [ln.split("\t") for ln in four]
    psi = {ln.split("\t")[2]: ln.split("\t")[5] for ln in six}
    # a form without an informative intron makes its whole event NA, reads or none; so does an event without a read
    assert psi["A.1"] == psi["A.2"] == psi["A.3"] == "NA" and psi["OV1.a"] == "NA" and psi["SG.a"] == "NA" and psi["ONE.a"] == "NA"
    unspliced = str(tmp_path / "unspliced.mrf")                                # reads that cross none of these introns
    open(unspliced, "w").write("AlignmentBlocks\n" + V.mrf_line("chr1", "+", [(1000, 1600)]) * 5 + V.mrf_line("chr1", "+", [(3050, 3100), (3200, 3250)]))
    empty = index_of(paths).host("MRF_SINGLE", unspliced)
    assert not empty.reads.any() and set(ln.split("\t")[5] for ln in empty.text(psi=True).splitlines()) == {"NA"} and np.isnan(empty.psi()).all()
    assert len(empty.text().splitlines()) == 18                                # every form is printed, zeros included


def test_the_tool_takes_an_output_path_and_refuses_nonsense(base, tmp_path):
    interval, gmap, mrf, paths = base
    rows, report, introns = V.table(interval, gmap, mrf)
    p = tool(paths, paths["mrf"], out="-")
    assert p.returncode == 0 and p.stdout == V.text(rows)
    assert log_messages(p.stderr) == [("INFO", V.report_line(report, 13, 18, 9))]
    out = str(tmp_path / "t.tab")
    p = tool(paths, paths["mrf"], opts=["--psi"], out=out)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == V.text(rows, introns)
    for bad in (["--min-overhang"], ["--nonsense"], ["--min-overhang", "-3"], ["--min-overhang", "x"], ["--bins", "p"]):
        p = tool(paths, paths["mrf"], opts=bad)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], bad
    positional = ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"]]
    for argv in (positional + ["--min-overhang"], positional[:5], positional + ["-", "-"]):
        p = subprocess.run([os.path.join(BIN, "psi"), "--host"] + argv, capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], argv
    p = tool(paths, paths["mrf"], out=str(tmp_path / "no_such_directory" / "t.tab"))
    assert p.returncode == 1 and p.stdout == ""


def test_a_malformed_record_gives_counts_status_and_message(base, tmp_path):
    _, _, _, paths = base
    good = V.mrf_line("chr1", "+", [(1050, 1100), (1500, 1550)])
    bad = "chr1:+:15x:200:1:50"
    path = str(tmp_path / "bad.mrf")
    open(path, "w").write("AlignmentBlocks\n" + good * 40 + bad + "\n" + good * 3)
    ix = index_of(paths)
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_SINGLE", path)
    assert e.value.status == LSQ_E_PARSE and str(e.value).endswith(": #41:" + bad)
    out = str(tmp_path / "never.tab")
    p = tool(paths, path, out=out)
    assert p.returncode == 1 and p.stdout == "" and "#41:" + bad in p.stderr and "Lexical_cast error" in p.stderr and not os.path.exists(out)
    with pytest.raises(L.LsqError) as e:
        ix.host("MRF_PAIRED", path)
    assert e.value.status == -3
    p = tool(paths, str(tmp_path / "missing.mrf"))
    assert p.returncode == 1 and p.stdout == ""


def test_the_name_keyed_formats_on_the_host(base, tmp_path):
    interval, gmap, _, paths = base
    reads = [("n1", "chr1", "+", [(1050, 1100), (1200, 1300), (1500, 1550)]), ("n2", "chr1", "-", [(2050, 2100), (2200, 2250)]), ("n3", "chr1", "+", [(350, 400), (500, 550)])]
    lines = ["track name=x\n", "browser position chr1\n"]      # (the format has two header lines)
    for n, c, s, bl in reads:
        for a, b in bl:
            lines.append("%s\tsrc\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (c, a + 1, b, s, n))
    path = str(tmp_path / "reads.gff")
    open(path, "w").write("".join(lines))
    want = V.table(interval, gmap, "AlignmentBlocks\n" + "".join(V.mrf_line(c, s, bl) for _, c, s, bl in reads))
    same(index_of(paths).host("UCSC_GFF", path), want)
    p = tool(paths, path, "UCSC_GFF", opts=["--psi"])
    assert p.returncode == 0 and p.stdout == V.text(want[0], want[2]) and want[1]["counted"] == 3 and want[1]["several_events"] == 1


# ----------------------------------------------------------------------------- threads

def test_threads_do_not_change_the_table(tmp_path):
    iso, lines = V.hot_case(True, 200, 300)
    small = V.table("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    assert V.fast_table("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines)) == small and small[1]["counted"] > 300
    iso, lines = V.hot_case(True, 70000, 1000)
    interval, mrf, paths = V.write_case(str(tmp_path), "big", iso, lines)
    want = V.fast_table(interval, V.map_of(iso), mrf)
    ix = index_of(paths)
    for n_threads in (1, 4):
        same(ix.host("MRF_SINGLE", paths["mrf"], n_threads=n_threads), want)
    same(ix.host_reads(ix.parse_host("MRF_SINGLE", paths["mrf"]), n_threads=4), want)
    assert want[1]["reads"] > 1 << 16 and {r[2]: r[3] for r in want[0]}["h2.skp"] == 70000


# ----------------------------------------------------------------------------- two samples

def test_two_samples_make_a_fisher_input(base, tmp_path):
    interval, gmap, mrf, paths = base
    a, b = str(tmp_path / "a.tab"), str(tmp_path / "b.tab")
    assert tool(paths, paths["mrf"], out=a).returncode == 0
    _, mrf2, paths2 = V.write_case(str(tmp_path), "second", V.definition_annotation(), V.definition_lines()[::2])
    assert tool(paths2, paths2["mrf"], out=b).returncode == 0
    ra, rb = V.table(interval, gmap, mrf)[0], V.table(interval, gmap, mrf2)[0]
    assert [r[2] for r in ra] == [r[2] for r in rb] and ra != rb                   # the same rows, other counts
    inp = ds.read_tables("fisher", [a, b])
    two = [(x, y) for x, y in zip(ra, rb) if sum(r[0] == x[0] for r in ra) == 2]
    assert inp.ids == [x[2] for x, _ in two][1::2] == ["C2.skp", "EDGE.b", "OV1.b", "OV2.b", "SE.skp", "SG.b", "UN.b"]
    assert inp.values.tolist() == [[two[k][0][3], two[k][1][3], two[k + 1][0][3], two[k + 1][1][3]] for k in range(0, len(two), 2)]
    lrt = ds.read_tables("lrt", [a, a, b, b], 2, 2)
    assert lrt.ids == [r[2] for r in ra] and lrt.totals.tolist() == [[x[1], x[1], y[1], y[1]] for x, y in zip(ra, rb)]


def test_new_entry_points_are_exported_and_the_abi_version_stays():
    syms = ("lsq_ps_index_build", "lsq_ps_index_free", "lsq_ps_index_num_chroms", "lsq_ps_index_num_events", "lsq_ps_index_num_forms", "lsq_ps_index_num_introns",
            "lsq_ps_index_chrom_name", "lsq_ps_index_event_name", "lsq_ps_index_form_name", "lsq_ps_index_dictionaries", "lsq_ps_index_arrays", "lsq_ps_host",
            "lsq_ps_host_reads", "lsq_ps_device", "lsq_ps_table_free", "lsq_ps_table_arrays", "lsq_ps_table_report", "lsq_ps_table_times", "lsq_ps_table_psi", "lsq_ps_format")
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in syms:
        assert hasattr(L.lib, sym), sym
        assert sym + "(" in header, sym
    assert L.lib.lsq_abi_version() == 2 and "#define LSQ_ABI_VERSION 2" in header
    assert os.access(os.path.join(BIN, "psi"), os.X_OK)
    assert L.PsiIndex is L.psi.PsiIndex and L.Psi is L.psi.Psi and L.psi.REPORT == V.REPORT and len(L.psi.REPORT) == 8
    rc, text = L.cli_run("psi", ["--nonsense"])
    assert rc == 1 and text == ""
