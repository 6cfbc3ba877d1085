"""parseGencode on the device: every fixture of tests/golden/gtf/ (what the reference's own binaries printed) through
cli_run and as a process, byte for byte and, for the "PROBLEM:" cases, stream for stream; the rules where the reference
has no answer ('#' and empty lines, short lines); generated GTFs against the restatement in gtf_ref.py (200 000 shuffled
lines, a line ending on, before and behind every edge the kernels know, a 70 KB line, a 5 000-exon transcript); the
getters against the formatted text; events --gtf against events --annotation, and count on its output against the oracle."""
import os
import random
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
from lesseq_amd import gencode
from lesseq_amd import localevents as le
import golden_inputs as gi
import gtf_ref as R
import localev_ref as LR
import oracle_binding as ob

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "gtf")
BIN = os.path.join(ROOT, "lesseq_amd", "bin")

GTF_CASES = sorted(os.path.relpath(d, GOLD) for d, _, fs in os.walk(GOLD) if "in.gtf" in fs)
PARSED = [c for c in GTF_CASES if os.path.exists(os.path.join(GOLD, c, "out.map"))]


def rd(*parts):
    with open(os.path.join(GOLD, *parts), "rb") as f:
        return f.read()


def run_tool(tool, args=(), data=None, **kw):
    p = subprocess.run([os.path.join(BIN, tool)] + list(args), input=data, capture_output=True, timeout=300, **kw)
    return p.returncode, p.stdout, p.stderr


def check_against_restatement(ctx, data):
    """the device result on `data`, as formatted text and through the getters, equals gtf_ref.py; returns the Gtf"""
    rc, want, err = R.parse_gencode(data)
    assert rc == 0, err
    g = gencode.parse_gtf(ctx, data)
    iv, mp = g.format()
    assert iv == want
    assert mp == R.isoform_map(R.cut_f1(want))[1]
    return g


@pytest.mark.parametrize("case", GTF_CASES)
def test_golden_in_process(case, tmp_path):
    path = os.path.join(GOLD, case, "in.gtf")
    rc, text = L.cli_run("parseGencode", [path])
    assert rc == int(rd(case, "status"))
    assert text.encode() == rd(case, "out.interval")


@pytest.mark.parametrize("case", GTF_CASES)
def test_golden_as_a_process(case):
    data = rd(case, "in.gtf")
    want = (int(rd(case, "status")), rd(case, "out.interval"), rd(case, "out.stderr"))
    assert run_tool("parseGencode", data=data) == want                                          # standard input
    assert run_tool("parseGencode", [os.path.join(GOLD, case, "in.gtf")]) == want               # a path
    p = subprocess.run("cat '%s' | '%s'" % (os.path.join(GOLD, case, "in.gtf"), os.path.join(BIN, "parseGencode")), shell=True,
                       capture_output=True, timeout=300)                                       # a pipe from cat
    assert (p.returncode, p.stdout, p.stderr) == want


@pytest.mark.parametrize("case", PARSED)
def test_the_readme_pipeline(case):
    gtf = os.path.join(GOLD, case, "in.gtf")
    p = subprocess.run("cat '%s' | '%s' | cut -f1 | '%s'" % (gtf, os.path.join(BIN, "parseGencode"), os.path.join(BIN, "gencodeIsoformMap")),
                       shell=True, capture_output=True, timeout=300)
    assert (p.returncode, p.stdout, p.stderr) == (0, rd(case, "out.map"), b"")


GOOD = b'chr1\tsrc\texon\t100\t200\t.\t+\t.\tgene_id "G"; transcript_id "T";\n'


def test_comment_and_empty_lines_are_skipped(gpu_ctx):
    data = b"##description: made up\n##provider: nobody\n#\n\n" + GOOD + b"\r\n\n# in the middle\tgene_id A\n" + GOOD.replace(b"100", b"300").replace(b"200", b"400") + b"#last"
    rc, out, err = run_tool("parseGencode", data=data)
    assert (rc, out) == (0, b"G|T\tchr1\t+\t99\t400\t2\t99,299\t200,400\n")
    assert err.count(b"\n") == 1 and b"WARNING] " in err and b"8 line(s) that are empty or begin with '#' were skipped" in err
    assert R.parse_gencode(data) == (0, out, b"")
    g = gencode.parse_gtf(gpu_ctx, data)
    assert g.format()[0] == out and (g.num_transcripts, g.num_genes, g.num_exon_lines) == (1, 1, 2)
    # nothing but comments
    assert run_tool("parseGencode", data=b"##a\n##b\n")[:2] == (0, b"")
    assert run_tool("parseGencode", data=b"") == (0, b"", b"")


@pytest.mark.parametrize("bad,line", [(b"chr1\tsrc\tgene\t7\n", 3), (b"chr1 src exon 100 200 . + . gene_id \"G\"; transcript_id \"T\";\n", 3),
                                      (b"chr1\tsrc\texon\t100\t200\t.\t+\t.\n", 3), (b"x", 3), (b" \n", 3)])
def test_short_lines_are_refused(bad, line):
    data = GOOD + GOOD + bad + (GOOD if bad.endswith(b"\n") else b"")
    want_err = b"PROBLEM: line %d has fewer than nine TAB-separated fields\n" % line
    assert run_tool("parseGencode", data=data) == (1, b"", want_err)
    assert R.parse_gencode(data) == (1, b"", want_err)


def test_first_bad_line_wins_and_library_status(gpu_ctx, tmp_path):
    data = GOOD * 300 + b"chr1\tsrc\tCDS\t1\t2\t.\t+\t.\tgene_id A\n" + GOOD * 300 + b"short\n" + GOOD * 50
    assert run_tool("parseGencode", data=data) == (1, b"", b"PROBLEM: Unexpected token: gene_id A\n")
    with pytest.raises(L.LsqError) as e:
        gencode.parse_gtf(gpu_ctx, data)
    assert e.value.status == -4 and "PROBLEM: Unexpected token: gene_id A" in str(e.value)
    data = GOOD * 300 + b"short\n" + GOOD * 300 + b"chr1\tsrc\tCDS\t1\t2\t.\t+\t.\tgene_id A\n"
    assert run_tool("parseGencode", data=data) == (1, b"", b"PROBLEM: line 301 has fewer than nine TAB-separated fields\n")
    with pytest.raises(L.LsqError) as e:
        gencode.parse_gtf(gpu_ctx, str(tmp_path / "missing.gtf"))
    assert e.value.status == -2
    rc, text = L.cli_run("parseGencode", [str(tmp_path / "missing.gtf")])
    assert rc == 1 and text == ""


# ---- generated inputs ---------------------------------------------------------------------------------------------------

def exon_line(rng, g, t, chrom=None, strand=None, pad=0, feature="exon"):
    s = rng.randrange(1, 10 ** 7)
    attrs = 'gene_id "%s"; transcript_id "%s"; gene_type "protein_coding"; level 2; tag "basic";' % (g, t)
    if pad:
        attrs = 'note "%s"; ' % ("p" * pad) + attrs
    return ("%s\tHAVANA\t%s\t%d\t%d\t.\t%s\t.\t%s\n" % (chrom or "chr%d" % (1 + sum(g.encode()) % 5), feature, s, s + rng.randrange(1, 900), strand or "+-"[len(g) & 1], attrs)).encode()


def test_two_hundred_thousand_shuffled_lines(gpu_ctx):
    rng = random.Random(41)
    lines = []
    for g in range(6000):
        gid = "ENSG%08d.%d" % (rng.randrange(10 ** 8), g % 7)
        chrom, strand = "chr%d" % (1 + g % 23), "+-"[g & 1]
        for t in range(1 + g % 5):
            tid = "ENST%08d" % rng.randrange(10 ** 8)
            lines.append(exon_line(rng, gid, tid, chrom, strand, feature="transcript"))
            for _ in range(rng.randint(1, 20)):
                lines.append(exon_line(rng, gid, tid, chrom, strand, pad=rng.choice([0, 0, 0, 40, 700])))
                if rng.random() < 0.3:
                    lines.append(exon_line(rng, gid, tid, chrom, strand, feature=rng.choice(["CDS", "UTR", "Exon", "exons", "exo"])))
    while len(lines) < 200000:
        lines.append(exon_line(rng, "FILL%d" % rng.randrange(300), "fill.%d" % rng.randrange(900)))
    rng.shuffle(lines)
    data = b"".join(lines)
    assert data.count(b"\n") >= 200000
    g = check_against_restatement(gpu_ctx, data)
    assert g.num_exon_lines == sum(1 for l in lines if l.split(b"\t")[2] == b"exon")
    ms = g.times_ms()
    assert len(ms) == 4 and all(t >= 0 for t in ms) and ms[2] > 0


def text_with_line_ending_at(rng, target, tail_lines=40, final_newline=True):
    """A GTF whose byte `target` is the newline of an exon line (so the next line starts at target + 1), with lines on
    both sides"""
    out, n = [], 0
    probe = exon_line(rng, "EDGE%d" % target, "edge.%d" % target)
    while True:
        l = exon_line(rng, "G%d" % rng.randrange(50), "t%d" % rng.randrange(200))
        if n + len(l) + 220 + len(probe) > target + 1:
            break
        out.append(l)
        n += len(l)
    room = target + 1 - n - len(probe)                    # bytes of one padded line ahead of the probe
    l = exon_line(rng, "PAD", "pad.1", pad=1)
    assert room >= len(l)
    l = l.replace(b'note "p"', b'note "' + b"p" * (1 + room - len(l)) + b'"')
    assert len(l) == room
    out.append(l)
    out.append(probe)
    data = b"".join(out)
    assert len(data) == target + 1 and data[target:target + 1] == b"\n", (len(data), target)
    for _ in range(tail_lines):
        out.append(exon_line(rng, "G%d" % rng.randrange(50), "t%d" % rng.randrange(200), pad=rng.choice([0, 100, 3000])))
    data = b"".join(out)
    return data if final_newline else data[:-1]


# what the kernels know: 64-byte ballot chunks, the 4 096 bytes 256 lanes take per round, the newline scan's tile of
# 7 680 bytes, the LDS window of 7 680 + 2 560 bytes (per tile)
TILE, WINDOW = 7680, 7680 + 2560
EDGES = [640, 4096, TILE, WINDOW, 2 * TILE, TILE + WINDOW, 3 * TILE, 2 * TILE + WINDOW]


@pytest.mark.parametrize("edge", EDGES)
def test_lines_ending_around_every_edge(edge, gpu_ctx):
    rng = random.Random(edge)
    for delta in (-1, 0, 1, -2, 2, -17, 16, 63, -64):
        # `edge` is the first byte of a tile / window / chunk: a line whose newline is byte edge - 1 ends on the edge
        data = text_with_line_ending_at(rng, edge - 1 + delta, final_newline=delta != 2)
        check_against_restatement(gpu_ctx, data)


def test_tile_edge_sweep(gpu_ctx):
    rng = random.Random(5)
    for delta in range(-70, 71):
        check_against_restatement(gpu_ctx, text_with_line_ending_at(rng, TILE - 1 + delta, tail_lines=8))


def test_more_lines_in_a_tile_than_one_round_lists(gpu_ctx):
    """runs of empty and '#' lines, one and two bytes each: thousands of newlines in a 7 680-byte tile, which the kernel lists
    1 024 at a time; the exon lines between and behind them keep their places, and a short line behind them its number"""
    rng = random.Random(9)
    ex = [exon_line(rng, "G%d" % (k % 3), "t%d" % (k % 5)) for k in range(41)]
    data = b"".join(ex[:10]) + b"\n" * 5000 + ex[10] + b"#\n" * 3000 + b"".join(ex[11:40]) + b"\n" * 1024 + ex[40]
    g = check_against_restatement(gpu_ctx, data)
    assert g.num_exon_lines == 41
    bad = data + b"short\n"
    with pytest.raises(L.LsqError) as e:
        gencode.parse_gtf(gpu_ctx, bad)
    assert "PROBLEM: line %d has fewer than nine TAB-separated fields" % bad.count(b"\n") in str(e.value)


def test_long_lines_and_many_exons(gpu_ctx):
    rng = random.Random(77)
    lines = [exon_line(rng, "G%d" % (k % 9), "t%d" % (k % 31)) for k in range(300)]
    long70 = ("chr9\tsrc\texon\t5\t9\t.\t-\t.\t" + " ".join('tag "filler_%05d";' % k for k in range(3900)) + ' gene_id "LONG70"; transcript_id "l.1";\n').encode()
    assert len(long70) > 70000
    ids_first = ('chr9\tsrc\texon\t15\t19\t.\t-\t.\tgene_id "LONG70"; transcript_id "l.1"; ' + " ".join('note "x;y %d";' % k for k in range(6000)) + "\n").encode()
    not_exon = long70.replace(b"\texon\t", b"\tCDS\t")
    lines[100:100] = [long70, not_exon]
    lines[200:200] = [ids_first]
    many = [("chrM\tsrc\texon\t%d\t%d\t.\t+\t.\tgene_id \"MANY\"; transcript_id \"many.1\";\n" % (s, s + rng.randrange(1, 90))).encode()
            for s in rng.sample(range(1, 10 ** 6), 5000)]
    for k, l in enumerate(many):
        lines.insert(rng.randrange(len(lines)), l) if k % 2 else lines.append(l)
    data = b"".join(lines) + long70[:-1]                     # ... and a 70 KB last line without a newline
    g = check_against_restatement(gpu_ctx, data)
    names = [g.name(i) for i in range(len(g))]
    s, e = g.exons(names.index(b"MANY|many.1"))
    assert len(s) == 5000 and list(s) == sorted(s) and list(e) == sorted(e)


def test_getters_agree_with_the_text(gpu_ctx):
    for case in PARSED:
        g = gencode.parse_gtf(gpu_ctx, os.path.join(GOLD, case, "in.gtf"))
        iv, mp = g.format()
        assert iv == rd(case, "out.interval") and mp == rd(case, "out.map")
        want = R.transcripts(rd(case, "in.gtf"))
        assert len(g) == g.num_transcripts == len(want)
        assert g.num_genes == len({n.split(b"|", 1)[0] for n, *_ in want if b"|" in n})
        for i, (name, chrom, strand, starts, ends) in enumerate(want):
            assert (g.name(i), g.chrom(i), g.strand(i)) == (name, chrom, strand)
            s, e = g.exons(i)
            assert s.dtype == np.int32 and list(s) == starts and list(e) == ends
        with pytest.raises(IndexError):
            g.name(len(want))
    # the bytes and the path give the same result
    assert gencode.parse_gtf(gpu_ctx, rd("cuff", "in.gtf")).format() == gencode.parse_gtf(gpu_ctx, os.path.join(GOLD, "cuff", "in.gtf")).format()


# ---- events --gtf ------------------------------------------------------------------------------------------------------

def _events_annotation(iv, mp, out_prefix):
    return L.cli_run("events", ["--annotation", "LH_GENE_TXT", iv, "UCSC_GENE2ISOFORM", mp, out_prefix])


def test_events_gtf_equals_events_annotation_on_the_reference_files(tmp_path, gpu_ctx):
    case = "cuff"
    d = os.path.join(GOLD, case)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    rc1, t1 = _events_annotation(os.path.join(d, "out.interval"), os.path.join(d, "out.map"), str(tmp_path / "a") + "/ev_")
    rc2, t2 = L.cli_run("events", ["--gtf", os.path.join(d, "in.gtf"), str(tmp_path / "b") + "/ev_"])
    assert rc1 == rc2 == 0 and t1 == t2 and t1.count("processing gene") >= 3
    a, b = LR.read_out(str(tmp_path / "a") + "/ev_"), LR.read_out(str(tmp_path / "b") + "/ev_")
    assert a == b and sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b"))
    # the Python entry gives the same graphs
    ga = le.Graphs.from_annotation(os.path.join(d, "out.interval"), os.path.join(d, "out.map"))
    gb = le.Graphs.from_gtf(gpu_ctx, os.path.join(d, "in.gtf"))
    assert ga.names() == gb.names() and [ga.shape(i) for i in range(len(ga))] == [gb.shape(i) for i in range(len(gb))]
    assert [ga.positions(i) for i in range(len(ga))] == [gb.positions(i) for i in range(len(gb))]


def test_events_gtf_refuses_what_events_annotation_refuses(tmp_path):
    """the gencode set holds ids with quotes and blanks, which the gene-list reader of events does not take: both modes say so"""
    d = os.path.join(GOLD, "gencode")
    rc1, t1 = _events_annotation(os.path.join(d, "out.interval"), os.path.join(d, "out.map"), str(tmp_path) + "/a_")
    rc2, t2 = L.cli_run("events", ["--gtf", os.path.join(d, "in.gtf"), str(tmp_path) + "/b_"])
    assert rc1 == rc2 == 1 and t1 == t2 == "" and os.listdir(tmp_path) == []
    p = subprocess.run([os.path.join(BIN, "events"), "--gtf", os.path.join(GOLD, "errors", "unquoted_gene_id", "in.gtf"), str(tmp_path) + "/c_"],
                       capture_output=True, timeout=300)
    assert (p.returncode, p.stdout, p.stderr) == (1, b"", rd("errors", "unquoted_gene_id", "out.stderr")) and os.listdir(tmp_path) == []


def wide_gtf(path):
    """tests/golden/wide/wide.interval (genes past 64 segments and 64 isoforms) written as a GTF"""
    w = os.path.join(HERE, "golden", "wide")
    gene_of = {}
    for ln in open(os.path.join(w, "wide.map")):
        g, t = ln.split()
        gene_of[t] = g
    rows = []
    for ln in open(os.path.join(w, "wide.interval")):
        f = ln.rstrip("\n").split("\t")
        for s, e in zip(f[6].split(","), f[7].split(",")):
            rows.append('%s\twide\texon\t%d\t%s\t.\t%s\t.\tgene_id "%s"; transcript_id "%s";\n' % (f[1], int(s) + 1, e, f[2], gene_of[f[0]], f[0]))
    random.Random(3).shuffle(rows)
    with open(path, "w") as f:
        f.write("##made from wide.interval\n" + "".join(rows))
    return len(rows)


def test_wide_genes_from_gtf_and_count_against_the_oracle(tmp_path):
    gtf = str(tmp_path / "wide.gtf")
    assert wide_gtf(gtf) > 3000
    rc, iv, _ = run_tool("parseGencode", [gtf])
    assert rc == 0 and iv.count(b"\n") == sum(1 for _ in open(os.path.join(HERE, "golden", "wide", "wide.interval")))
    rc, mp, err = run_tool("gencodeIsoformMap", data=R.cut_f1(iv))
    assert rc == 0 and err == b""
    assert (0, iv, b"") == R.parse_gencode(open(gtf, "rb").read())
    (tmp_path / "w.interval").write_bytes(iv)
    (tmp_path / "w.map").write_bytes(mp)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    rc1, t1 = _events_annotation(str(tmp_path / "w.interval"), str(tmp_path / "w.map"), str(tmp_path / "a") + "/ev_")
    p = subprocess.run([os.path.join(BIN, "events"), "--gtf", gtf, str(tmp_path / "b") + "/ev_"], capture_output=True, text=True, timeout=300)
    assert rc1 == 0 and p.returncode == 0 and p.stdout == t1
    a, b = LR.read_out(str(tmp_path / "a") + "/ev_"), LR.read_out(str(tmp_path / "b") + "/ev_")
    assert a == b and "ES.interval" in b
    # count on the events' output, against the oracle, on one toy read file
    ivp, mpp = str(tmp_path / "b" / "ev_ES.interval"), str(tmp_path / "b" / "ev_ES.map")
    forms = []
    for ln in open(ivp):
        f = ln.rstrip("\n").split("\t")
        forms.append((f[1], f[2], list(zip(map(int, f[6].split(",")), map(int, f[7].split(","))))))
    rng = random.Random(9)
    lines = ["AlignmentBlocks\n"]
    for _ in range(4000):
        chrom, strand, exons = forms[rng.randrange(len(forms))]
        n = sum(e - s for s, e in exons)
        if n >= 40:
            lines.append(gi.mrf_line(chrom, strand, gi.transcript_blocks(exons, rng.randrange(0, n - 40 + 1), 40)))
    mrf = str(tmp_path / "toy.mrf")
    open(mrf, "w").writelines(lines)
    argv = ["0", "ES", "./", "LH_GENE_TXT", ivp, "UCSC_GENE2ISOFORM", mpp, "0", "1000000", "MRF_SINGLE", "SHORT_READ", "40", mrf]
    rc, text = L.cli_run("count", argv)
    orc, otext, _ = ob.run("count", argv)
    assert rc == 0 and orc == 0 and text == otext and len(text) > 0
