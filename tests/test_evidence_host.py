"""Junction and exon-body reads per event form without a GPU (include/lesseq_hip.h, lsq_fe_*): lsq_fe_host and `evidence --host`
against the definition as tests/evidence_ref.py restates it.  All values are integers, psi is a fixed order of double operations on
them: the tables equal the reference's exactly, as numbers and as text."""
import math
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
import bam_writer
import evidence_ref as E
import psi_ref as V
from lesseq_amd import diffsplice as ds
from test_junctions_host import sam_of, log_messages

HERE = os.path.dirname(os.path.abspath(__file__))
BIN = os.path.join(os.path.dirname(HERE), "lesseq_amd", "bin")
GOLD = os.path.join(HERE, "golden")
LSQ_E_ARG, LSQ_E_PARSE = -1, -4
USAGE = "Usage:\nevidence [--host] [--psi --read-length L] [--min-overhang N] [--min-body N] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]"
TOY_TABLE = "RI1\t2\tRI1.ret\t1\nRI1\t2\tRI1.spl\t1\nSE1\t4\tSE1.inc\t3\nSE1\t4\tSE1.skp\t1\n"
TOY_PSI_TABLE = ("RI1\t2\tRI1.ret\t1\t0\t100\t149\t0.247475\nRI1\t2\tRI1.spl\t1\t1\t0\t49\t0.752525\n"
                 "SE1\t4\tSE1.inc\t3\t2\t100\t149\t0.496622\nSE1\t4\tSE1.skp\t1\t1\t0\t49\t0.503378\n")
TOY_REPORT = {"reads": 13, "blocks": 17, "occurrences": 4, "dropped_overhang": 0, "no_chromosome": 0, "informative_occurrences": 4, "skipped_blocks": 1, "body_hits": 4,
              "counted": 6, "several_events": 0, "counted_by_body_alone": 2}
POSITION_OPTIONS = ((50, 1, 1), (50, 10, 10), (30, 10, 25), (400, 1, 1))       # (read length, min_overhang, min_body)


def index_of(paths):
    return L.EvidenceIndex(L.Annotation(paths["interval"], paths["map"]))


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None, host=True, timeout=None, out=None):
    argv = ([os.path.join(BIN, "evidence")] + (["--host"] if host else []) + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads] +
            ([out] if out else []))
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=timeout)


def same(got, want, pos=None, read_length=50):
    """the table against the reference's (rows, report, introns, body); with `pos`, the reference's positions under read_length and
    the options the table was made with, the eight columns and psi too"""
    rows, report, introns, body = want
    assert got.rows() == rows
    assert got.report == report
    assert got.index.form_introns.tolist() == introns and got.index.form_body.tolist() == body
    assert got.text() == E.text(rows)
    assert len(got.total) == got.index.num_events and len(got) == got.index.num_forms == len(rows)
    if pos is not None:
        assert got.text(psi=True, read_length=read_length) == E.text(rows, introns, body, pos)
        psi = got.psi(read_length)
        assert psi.dtype == np.float64 and [None if math.isnan(p) else p for p in psi.tolist()] == E.psi_of(rows, pos)


def toy_paths():
    d = os.path.join(GOLD, "toy")
    return {"interval": os.path.join(d, "toy.interval"), "map": os.path.join(d, "toy.map"), "mrf": os.path.join(d, "toy.mrf"), "count": os.path.join(d, "count.out")}


def texts_of(paths):
    return [open(paths[k]).read() for k in ("interval", "map", "mrf")]


def want_of(paths, min_overhang=1, min_body=1):
    return E.table(*texts_of(paths), min_overhang=min_overhang, min_body=min_body)


def random_files(d):
    iso, reads = V.random_case()
    rng = np.random.RandomState(7)
    # psi's reads are cut from exon chains; a third of them moved by a few bases, so that blocks straddle the regions' edges
    moved = []
    for c, minus, blocks in reads:
        if rng.rand() < 0.33:
            k = int(rng.randint(-70, 70))
            blocks = [(s + k, e + k) for s, e in blocks]
        moved.append((c, minus, blocks))
    interval, mrf, paths = V.write_case(d, "rnd", iso, [V.mrf_line(c, "-" if minus else "+", b) for c, minus, b in moved])
    sam = sam_of(moved, mapq={0: 3, 7: 3}).encode()
    paths["sam"], paths["bam"] = os.path.join(d, "rnd.sam"), os.path.join(d, "rnd.bam")
    open(paths["sam"], "wb").write(sam)
    open(paths["bam"], "wb").write(bam_writer.sam_to_bam(sam, "cut61"))
    gmap = open(paths["map"]).read()
    return paths, E.table(interval, gmap, mrf), E.table(interval, gmap, L.sam_to_mrf(sam, min_mapq=4).decode()), E.positions(interval, gmap, 50)


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fe"))
    interval, mrf, paths = E.write_case(d, "base", E.definition_annotation(), E.definition_lines())
    return interval, open(paths["map"]).read(), mrf, paths


@pytest.fixture(scope="module")
def formats(tmp_path_factory):
    return random_files(str(tmp_path_factory.mktemp("fernd")))


# ----------------------------------------------------------------------------- the worked examples, the reference itself

def test_the_reference_on_the_toy_example():
    paths = toy_paths()
    rows, report, introns, body = want_of(paths)
    pos = E.positions(*texts_of(paths)[:2], 50)
    assert E.text(rows) == TOY_TABLE and E.text(rows, introns, body, pos) == TOY_PSI_TABLE and report == TOY_REPORT and pos == [149, 49, 149, 49]


def test_the_reference_on_the_hand_worked_definition_cases(base):
    interval, gmap, mrf, _ = base
    rows, report, introns, body = E.table(interval, gmap, mrf)
    assert rows == E.DEFINITION_ROWS and introns == E.DEFINITION_INTRONS and body == E.DEFINITION_BODY and report == E.DEFINITION_REPORT
    regions = {f[0]: f[4] for _, forms in E.events_of(interval, gmap) for f in forms}
    assert regions["A.1"] == [] and regions["A.2"] == [(600, 700)] and regions["A.3"] == [(400, 500), (600, 700)]          # a region two of three forms share
    assert regions["OW1.a"] == regions["OW2.a"] == [(6100, 6300)] and regions["ONE.a"] == [] and regions["SG.a"] == [] and regions["SG.b"] == [(4100, 4200)]
    assert regions["EDGE.a"] == [] and regions["EDGE.b"] == [(E.LIM - 200, E.LIM - 150)] and regions["EZ.b"] == [(E.LIM - 400, E.LIM)]
    assert E.fast_table(interval, gmap, mrf) == (rows, report, introns, body)                   # the second reference is the first
    # every one of psi's own definition reads counts for the forms psi counts it for, and more
    psi_rows = {r[2]: r[3] for r in V.DEFINITION_ROWS}
    assert all(r[3] >= psi_rows[r[2]] for r in rows if r[2] in psi_rows)


def test_the_toy_example_byte_for_byte():
    paths = toy_paths()
    ix = index_of(paths)
    got = ix.host("MRF_SINGLE", paths["mrf"])
    same(got, want_of(paths), E.positions(*texts_of(paths)[:2], 50))
    assert got.text() == TOY_TABLE and got.text(psi=True, read_length=50) == TOY_PSI_TABLE and got.report == TOY_REPORT
    assert ix.event_names() == ["RI1", "SE1"] and ix.form_names() == ["RI1.ret", "RI1.spl", "SE1.inc", "SE1.skp"]
    assert ix.event_first_form.tolist() == [0, 2, 4] and ix.form_introns.tolist() == [0, 1, 2, 1] and ix.form_body.tolist() == [100, 0, 100, 0]
    assert ix.num_introns == 4 and ix.num_regions == 2 and ix.chrom_names() == ["chr1"] and ix.positions(50).tolist() == [149, 49, 149, 49]
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == TOY_TABLE
    p = tool(paths, paths["mrf"], opts=["--psi", "--read-length", "50"])
    assert p.returncode == 0 and p.stdout == TOY_PSI_TABLE
    assert log_messages(p.stderr) == [("INFO", E.report_line(TOY_REPORT, 4, 2, 4, 2))]
    # psi on the same files: the retained intron is NA there, and the read inside the skipped exon is not counted
    both = L.PsiIndex(L.Annotation(paths["interval"], paths["map"])).host("MRF_SINGLE", paths["mrf"]).text(psi=True).splitlines()
    assert both[0].endswith("NA") and both[2].split("\t")[3] == "2"
    for q in (paths,):          # events and forms as count prints them
        count = [ln.split("\t") for ln in open(q["count"]).read().splitlines()]
        assert [(r[0], r[2]) for r in got.rows()] == [(c[0], c[2]) for c in count]


# ----------------------------------------------------------------------------- the definition

def test_host_equals_the_reference_on_the_definition_cases(base):
    interval, gmap, mrf, paths = base
    want = E.table(interval, gmap, mrf)
    pos = E.positions(interval, gmap, 50)
    ix = index_of(paths)
    same(ix.host("MRF_SINGLE", paths["mrf"]), want, pos)
    same(ix.host_reads(ix.parse_host("MRF_SINGLE", paths["mrf"]), n_threads=3), want, pos)
    assert ix.event_names() == sorted(ix.event_names(), key=lambda n: n.encode()) and ix.num_introns == 14 and ix.num_regions == 13
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == E.text(want[0]) and E.report_line(want[1], 14, 13, 24, 12) in p.stderr
    p = tool(paths, paths["mrf"], opts=["--psi", "--read-length", "50"])
    assert p.returncode == 0 and p.stdout == E.text(*want[:1], want[2], want[3], pos)
    psi = {ln.split("\t")[2]: ln.split("\t")[7] for ln in p.stdout.splitlines()}
    # SG: the long form counts, the short one is a subset of it and has no position; the one-form event; A.1 without a region still has its introns
    assert psi["SG.a"] == psi["SG.b"] == "NA" and psi["ONE.a"] == "NA" and psi["A.1"] != "NA" and psi["OV1.a"] != "NA" and psi["EZ.b"] == "NA"
    assert {r[2]: r[3] for r in want[0]}["SG.b"] == 1


@pytest.mark.parametrize("min_body", [1, 10])
def test_the_body_rules_edges(tmp_path, min_body):
    cases = E.edge_lines(min_body)
    interval, mrf, paths = E.write_case(str(tmp_path), "edge", E.definition_annotation(), [ln for ln, _ in cases])
    gmap = open(paths["map"]).read()
    ix = index_of(paths)
    for m in sorted({1, max(1, min_body - 1), min_body, min_body + 1}):
        want = E.table(interval, gmap, mrf, min_body=m)
        same(ix.host("MRF_SINGLE", paths["mrf"], min_body=m), want)
        p = tool(paths, paths["mrf"], opts=["--min-body", str(m)])
        assert p.returncode == 0 and p.stdout == E.text(want[0])
        if m == min_body:       # worked out by hand: which of the lines count for SE.inc at this min_body
            assert {r[2]: r[3] for r in want[0]}["SE.inc"] == sum(counts for _, counts in cases) == 6
            for ln, counts in cases:         # every line alone
                rows = E.table(interval, gmap, "AlignmentBlocks\n" + ln, min_body=m)[0]
                assert {r[2]: r[3] for r in rows}["SE.inc"] == int(counts), ln


def test_a_region_shorter_than_min_body_and_min_body_beyond_every_block(base):
    interval, gmap, mrf, paths = base
    ix = index_of(paths)
    want = E.table(interval, gmap, mrf, min_body=60)
    same(ix.host("MRF_SINGLE", paths["mrf"], min_body=60), want, E.positions(interval, gmap, 100, min_body=60), read_length=100)
    n = {r[2]: r[3] for r in want[0]}
    # OV2.a's and EDGE.b's regions hold 50 bases: only OV2.a's junction read is left; the 60-base read inside OV1.b's region still counts
    assert n["OV2.a"] == 1 and n["EDGE.b"] == 0 and n["OV1.b"] == 1 and n["EZ.b"] == 0 and n["A.3"] == 1
    # nothing can hit: the table is psi's
    top = (1 << 31) - 1
    got = ix.host("MRF_SINGLE", paths["mrf"], min_body=top)
    same(got, E.table(interval, gmap, mrf, min_body=top))
    assert got.report["body_hits"] == 0 and got.report["counted_by_body_alone"] == 0


def test_with_no_body_hit_possible_the_counts_are_psis(formats):
    paths = formats[0]
    got = index_of(paths).host("MRF_SINGLE", paths["mrf"], min_body=(1 << 31) - 1)
    psi = L.PsiIndex(L.Annotation(paths["interval"], paths["map"])).host("MRF_SINGLE", paths["mrf"])
    assert (got.reads == psi.reads).all() and (got.total == psi.total).all() and psi.reads.sum() > 1000
    assert [got.report[k] for k in E.REPORT[:6]] == [psi.report[k] for k in V.REPORT[:6]]
    assert got.report["counted"] == psi.report["counted"] and got.report["several_events"] == psi.report["several_events"]
    assert got.report["counted_by_body_alone"] == 0 and got.report["body_hits"] == 0


def test_forms_come_in_the_maps_order_not_the_interval_files(tmp_path):
    iso = E.definition_annotation()
    interval, mrf, paths = E.write_case(str(tmp_path), "order", iso[::-1], E.definition_lines())
    gmap = V.map_of(iso)
    open(paths["map"], "w").write(gmap)
    want = E.table(interval, gmap, mrf)
    assert want[0] == E.DEFINITION_ROWS
    same(index_of(paths).host("MRF_SINGLE", paths["mrf"]), want)


# ----------------------------------------------------------------------------- positions

@pytest.mark.parametrize("options", POSITION_OPTIONS, ids=["L%d_o%d_b%d" % o for o in POSITION_OPTIONS])
def test_the_closed_form_of_positions_equals_the_enumeration(base, formats, options):
    interval, gmap, _, paths = base
    pos = E.positions(interval, gmap, *options)
    assert index_of(paths).positions(*options).tolist() == pos
    rnd = formats[0]
    texts = texts_of(rnd)
    want = E.positions(texts[0], texts[1], *options)
    assert index_of(rnd).positions(*options).tolist() == want
    if options == (50, 10, 10):        # SE.inc: both introns and the region, one window; ONE.a: nothing informative
        by = dict(zip([r[2] for r in E.DEFINITION_ROWS], pos))
        assert by["SE.inc"] == 131 and by["SE.skp"] == 31 and by["ONE.a"] == 0 and by["SG.a"] == 0
    if options[0] == 400:              # forms shorter than the read
        assert 0 in want and pos[3] == 0


def test_positions_where_an_exon_is_shorter_than_the_overhang(tmp_path):
    iso = [E.interval_line("P.a", "chr1", "+", [(100, 200), (300, 305), (400, 500)]), E.interval_line("P.b", "chr1", "+", [(100, 200), (400, 500)])]
    interval, _, paths = E.write_case(str(tmp_path), "short", iso, [])
    gmap = open(paths["map"]).read()
    ix = index_of(paths)
    for options in POSITION_OPTIONS + ((50, 6, 6), (50, 5, 5)):
        assert ix.positions(*options).tolist() == E.positions(interval, gmap, *options), options
    # by hand, L 50: at overhang 6 the 5-base exon carries no junction and no body hit (P.a: nothing); at 5 both introns and the region do
    assert ix.positions(50, 6, 6).tolist() == [0, 39] and ix.positions(50, 5, 5).tolist() == [46, 41]


# ----------------------------------------------------------------------------- formats, options

def test_host_equals_the_reference_on_a_random_case(formats):
    paths, want, fewer, pos = formats
    ix = index_of(paths)
    assert ix.num_events == 40 and want[1]["reads"] == 5000 and want[1]["counted"] > 2000 and want[1]["several_events"] > 50 and want[1]["counted_by_body_alone"] > 300
    assert want[1]["skipped_blocks"] > 50 and want[1]["body_hits"] > 1000 and want[1]["informative_occurrences"] > 1000 and 0 in want[3] and ix.num_regions > 40
    for fmt, key in (("MRF_SINGLE", "mrf"), ("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam")):
        same(ix.host(fmt, paths[key]), want, pos)
    assert fewer[1]["reads"] == 4998 and fewer != want
    for fmt, key in (("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam")):
        same(ix.host(fmt, paths[key], min_mapq=4), fewer)
        p = tool(paths, paths[key], fmt, opts=["--psi", "--read-length", "50"], env={"LSQ_SAM_MIN_MAPQ": "4"})
        assert p.returncode == 0 and p.stdout == E.text(fewer[0], fewer[2], fewer[3], pos)
    p = tool(paths, paths["bam"], "BAM_SINGLE", env={"LSQ_BAM_VERIFY": "1"})
    assert p.returncode == 0 and p.stdout == E.text(want[0])
    texts = texts_of(paths)
    assert E.fast_table(*texts) == want and E.fast_table(*texts, min_overhang=30, min_body=25) == E.table(*texts, min_overhang=30, min_body=25)
    for mo, mb in ((2, 2), (30, 1), (1, 40), (10, 25)):
        w = E.table(*texts, min_overhang=mo, min_body=mb)
        same(ix.host("MRF_SINGLE", paths["mrf"], min_overhang=mo, min_body=mb), w)
        assert w != want
    p = tool(paths, paths["sam"], "SAM_SINGLE", opts=["--psi", "--read-length", "30", "--min-overhang", "10", "--min-body", "25"])
    w = E.table(*texts, min_overhang=10, min_body=25)
    assert p.returncode == 0 and p.stdout == E.text(w[0], w[2], w[3], E.positions(texts[0], texts[1], 30, 10, 25))
    assert E.report_line(w[1], ix.num_introns, ix.num_regions, ix.num_forms, ix.num_events, 10, 25) in p.stderr


def test_bad_options_are_argument_errors_and_the_usage_text(base, tmp_path):
    interval, gmap, mrf, paths = base
    ix = index_of(paths)
    reads = ix.parse_host("MRF_SINGLE", paths["mrf"])
    for call, word in ((lambda: ix.host("MRF_SINGLE", paths["mrf"], min_overhang=0), "min_overhang"), (lambda: ix.host("MRF_SINGLE", paths["mrf"], min_body=0), "min_body"),
                       (lambda: ix.host_reads(reads, min_body=0), "min_body"), (lambda: ix.host_reads(reads, min_overhang=0), "min_overhang"),
                       (lambda: ix.positions(0), "read_length"), (lambda: ix.positions(1 << 18), "read_length"), (lambda: ix.positions(50, 0, 1), "min_overhang"),
                       (lambda: ix.positions(50, 1, 0), "min_body"), (lambda: ix.host_reads(reads).psi(0), "read_length"),
                       (lambda: ix.host_reads(reads).text(psi=True, read_length=1 << 18), "read_length")):
        with pytest.raises(L.LsqError) as e:
            call()
        assert e.value.status == LSQ_E_ARG and word in str(e.value)
    assert ix.positions((1 << 18) - 1).tolist() == [0] * 24
    rows, report = E.table(interval, gmap, mrf)[:2]
    p = tool(paths, paths["mrf"], out="-")
    assert p.returncode == 0 and p.stdout == E.text(rows)
    assert log_messages(p.stderr) == [("INFO", E.report_line(report, 14, 13, 24, 12))]
    for bad in (["--psi"], ["--psi", "--read-length"], ["--psi", "--read-length", "0"], ["--psi", "--read-length", str(1 << 18)], ["--read-length", "x"], ["--min-body", "0"],
                ["--min-body"], ["--min-body", "-3"], ["--min-overhang", "0"], ["--min-overhang", "x"], ["--nonsense"], ["--bins", "p"]):
        p = tool(paths, paths["mrf"], opts=bad)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], bad
    positional = ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "MRF_SINGLE", paths["mrf"]]
    for argv in (positional + ["--min-body"], positional[:5], positional + ["-", "-"]):
        p = subprocess.run([os.path.join(BIN, "evidence"), "--host"] + argv, capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], argv
    out = str(tmp_path / "t.tab")
    p = tool(paths, paths["mrf"], out=out)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == E.text(rows)
    p = tool(paths, paths["mrf"], out=str(tmp_path / "no_such_directory" / "t.tab"))
    assert p.returncode == 1 and p.stdout == ""


def test_a_malformed_record_gives_counts_status_and_message(base, tmp_path):
    _, _, _, paths = base
    good = E.mrf_line("chr1", "+", [(1220, 1260)])
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
    reads = [("n1", "chr1", "+", [(1050, 1100), (1200, 1300), (1500, 1550)]), ("n2", "chr1", "-", [(2120, 2180)]), ("n3", "chr1", "+", [(610, 620), (630, 640)]),
             ("n4", "chr1", "+", [(6150, 6250)])]
    lines = ["track name=x\n", "browser position chr1\n"]      # (the format has two header lines)
    for n, c, s, bl in reads:
        for a, b in bl:
            lines.append("%s\tsrc\texon\t%d\t%d\t.\t%s\t.\t%s\n" % (c, a + 1, b, s, n))
    path = str(tmp_path / "reads.gff")
    open(path, "w").write("".join(lines))
    want = E.table(interval, gmap, "AlignmentBlocks\n" + "".join(E.mrf_line(c, s, bl) for _, c, s, bl in reads))
    same(index_of(paths).host("UCSC_GFF", path), want)
    p = tool(paths, path, "UCSC_GFF")
    assert p.returncode == 0 and p.stdout == E.text(want[0]) and want[1]["counted"] == 4 and want[1]["several_events"] == 1 and want[1]["counted_by_body_alone"] == 3


# ----------------------------------------------------------------------------- threads

def test_threads_do_not_change_the_table(tmp_path):
    iso, lines = E.hot_case(True, 200, 300)
    texts = ("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    small = E.table(*texts)
    assert E.fast_table(*texts) == small and small[1]["counted"] > 300
    iso, lines = E.hot_case(True, 70000, 1000)
    interval, mrf, paths = E.write_case(str(tmp_path), "big", iso, lines)
    want = E.fast_table(interval, V.map_of(iso), mrf)
    ix = index_of(paths)
    for n_threads in (1, 4):
        same(ix.host("MRF_SINGLE", paths["mrf"], n_threads=n_threads), want)
    same(ix.host_reads(ix.parse_host("MRF_SINGLE", paths["mrf"]), n_threads=4), want)
    assert want[1]["reads"] > 1 << 16 and {r[2]: r[3] for r in want[0]}["h2.ret"] == 70000


# ----------------------------------------------------------------------------- two samples

def test_two_samples_make_a_fisher_input_with_both_rows_of_a_retained_intron(tmp_path):
    iso, lines = E.hot_case(True, 300, 600)
    tables, rows = [], []
    for k in range(2):
        interval, mrf, paths = E.write_case(str(tmp_path), "s%d" % k, iso, [ln for j, ln in enumerate(lines) if (j * 7 + 3 * k) % 4 != 1])
        tables.append(str(tmp_path / ("s%d.tab" % k)))
        assert tool(paths, paths["mrf"], out=tables[-1]).returncode == 0
        rows.append(E.table(interval, open(paths["map"]).read(), mrf)[0])
        assert open(tables[-1]).read() == E.text(rows[-1])
    a, b = rows
    inp = ds.read_tables("fisher", tables)
    assert inp.ids == ["h%d.spl" % g for g in range(6)]
    assert inp.values.tolist() == [[a[k][3], b[k][3], a[k + 1][3], b[k + 1][3]] for k in range(0, 12, 2)]
    # a retained-intron event now has a non-zero row for both forms, in both samples
    assert all(min(v) > 0 for g, v in enumerate(inp.values.tolist()) if g != 2) and a != b
    lrt = ds.read_tables("lrt", tables * 2, 2, 2)
    assert lrt.ids == [r[2] for r in a]


def test_new_entry_points_are_exported_and_the_abi_version_stays():
    syms = ("lsq_fe_index_build", "lsq_fe_index_free", "lsq_fe_index_num_chroms", "lsq_fe_index_num_events", "lsq_fe_index_num_forms", "lsq_fe_index_num_introns",
            "lsq_fe_index_num_regions", "lsq_fe_index_chrom_name", "lsq_fe_index_event_name", "lsq_fe_index_form_name", "lsq_fe_index_dictionaries", "lsq_fe_index_arrays",
            "lsq_fe_index_positions", "lsq_fe_host", "lsq_fe_host_reads", "lsq_fe_device", "lsq_fe_table_free", "lsq_fe_table_arrays", "lsq_fe_table_report",
            "lsq_fe_table_times", "lsq_fe_table_psi", "lsq_fe_format")
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in syms:
        assert hasattr(L.lib, sym), sym
        assert sym + "(" in header, sym
    assert L.lib.lsq_abi_version() == 2 and "#define LSQ_ABI_VERSION 2" in header
    assert os.access(os.path.join(BIN, "evidence"), os.X_OK)
    assert L.EvidenceIndex is L.evidence.EvidenceIndex and L.Evidence is L.evidence.Evidence and L.evidence.REPORT == E.REPORT and len(L.evidence.REPORT) == 11
    assert L.evidence.PHASES == ("index_upload", "count", "copy_back")
    rc, text = L.cli_run("evidence", ["--nonsense"])
    assert rc == 1 and text == ""
