"""Junction and exon-body reads per event form on the device (lsq_fe_device: lsq_readfile.hip, lsq_evidence.hip): the count kernel at
the smallest shapes at which it can go wrong, against the definition as tests/evidence_ref.py restates it and against lsq_fe_host.
All values are integers, psi is computed on the host from them: the device table equals both exactly, report and text included.
Need an MI355X: python -m pytest tests -m gpu."""
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
import evidence_ref as E
import psi_ref as V
from lesseq_amd import diffsplice as ds
from test_evidence_host import index_of, same, tool as host_tool, toy_paths, texts_of, want_of, random_files, BIN, LSQ_E_PARSE, TOY_TABLE, TOY_PSI_TABLE, TOY_REPORT
from test_sam_gpu import CHILD_TIMEOUT

pytestmark = pytest.mark.gpu


def check_paths(ctx, paths, want, min_overhang=1, min_body=1, pos=None):
    ix = index_of(paths)
    dev = ix.device(ctx, "MRF_SINGLE", paths["mrf"], min_overhang=min_overhang, min_body=min_body)
    same(dev, want, pos)
    host = ix.host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang, min_body=min_body)
    same(host, want, pos)
    assert (dev.reads == host.reads).all() and (dev.total == host.total).all() and dev.report == host.report
    assert dev.text(psi=True, read_length=50) == host.text(psi=True, read_length=50)
    assert set(dev.times) == set(L.evidence.PHASES) and all(v >= 0 for v in dev.times.values())


def check_case(ctx, d, stem, iso, lines, want=None, header="AlignmentBlocks\n", min_overhang=1, min_body=1, fast=False):
    """the device table and the host table against the reference's; returns (want, paths)"""
    interval, mrf, paths = E.write_case(str(d), stem, iso, lines, header)
    want = want or (E.fast_table if fast else E.table)(interval, open(paths["map"]).read(), mrf, min_overhang=min_overhang, min_body=min_body)
    check_paths(ctx, paths, want, min_overhang, min_body)
    return want, paths


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None, out=None):
    return host_tool(paths, reads, fmt, opts, env, host=False, timeout=CHILD_TIMEOUT, out=out)


# ----------------------------------------------------------------------------- the definition

def test_the_toy_example(gpu_ctx):
    paths = toy_paths()
    got = index_of(paths).device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    assert got.text() == TOY_TABLE and got.text(psi=True, read_length=50) == TOY_PSI_TABLE and got.report == TOY_REPORT
    check_paths(gpu_ctx, paths, want_of(paths), pos=E.positions(*texts_of(paths)[:2], 50))


def test_definition_cases(gpu_ctx, tmp_path):
    (rows, report, introns, body), paths = check_case(gpu_ctx, tmp_path, "base", E.definition_annotation(), E.definition_lines())
    assert rows == E.DEFINITION_ROWS and report == E.DEFINITION_REPORT and introns == E.DEFINITION_INTRONS and body == E.DEFINITION_BODY
    # a region shorter than min_body; nothing can hit
    for min_body in (60, (1 << 31) - 1):
        check_paths(gpu_ctx, paths, want_of(paths, min_body=min_body), min_body=min_body)
    check_paths(gpu_ctx, paths, want_of(paths, 10, 25), 10, 25)


@pytest.mark.parametrize("n", [1, 10])
def test_the_body_rules_edges(gpu_ctx, tmp_path, n):
    cases = E.edge_lines(n)
    for m in sorted({1, n, n + 1}):
        (rows, _, _, _), _ = check_case(gpu_ctx, tmp_path, "edge%d" % m, E.definition_annotation(), [ln for ln, _ in cases], min_body=m)
        if m == n:
            assert {r[2]: r[3] for r in rows}["SE.inc"] == sum(c for _, c in cases) == 6


def test_files_without_a_hit(gpu_ctx, tmp_path):
    iso = E.definition_annotation()
    for stem, lines, header in (("header_only", [], "AlignmentBlocks\n"), ("nothing", [], ""), ("unknown", [E.mrf_line("chrU", "+", [(1220, 1260)])] * 300, "AlignmentBlocks\n"),
                                ("common", [E.mrf_line("chr1", "+", [(1020, 1080)])] * 300, "AlignmentBlocks\n")):
        (rows, report, _, _), _ = check_case(gpu_ctx, tmp_path, stem, iso, lines, header=header)
        assert all(r[1] == 0 and r[3] == 0 for r in rows) and len(rows) == 24 and report["reads"] == len(lines) and report["counted"] == 0


# ----------------------------------------------------------------------------- formats

@pytest.fixture(scope="module")
def formats(tmp_path_factory):
    return random_files(str(tmp_path_factory.mktemp("fegpu")))


def test_one_table_from_mrf_sam_and_bam(gpu_ctx, formats):
    paths, want, fewer, pos = formats
    ix = index_of(paths)
    tables = [ix.device(gpu_ctx, fmt, paths[key]) for fmt, key in (("MRF_SINGLE", "mrf"), ("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam"))]
    for t in tables:
        same(t, want, pos)
        assert (t.reads == tables[0].reads).all() and (t.total == tables[0].total).all() and t.report == tables[0].report
    same(ix.host("MRF_SINGLE", paths["mrf"]), want, pos)
    ctx = L.Context(0)
    ctx.set_option("sam_min_mapq", 4)
    ctx.set_option("bam_verify", 1)
    for fmt, key in (("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam")):
        same(ix.device(ctx, fmt, paths[key]), fewer)
        same(ix.host(fmt, paths[key], min_mapq=4), fewer)
    ctx.close()
    for fmt in ("UCSC_GFF", "MRF_PAIRED"):
        with pytest.raises(L.LsqError) as e:
            ix.device(gpu_ctx, fmt, paths["mrf"])
        assert e.value.status == -3 and str(e.value).endswith("Unknown file format error: " + fmt)
    for bad in ({"min_overhang": 0}, {"min_body": 0}):
        with pytest.raises(L.LsqError) as e:
            ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"], **bad)
        assert e.value.status == -1
    a, b = ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"])          # the same from run to run
    assert a.rows() == b.rows() == want[0] and a.report == b.report
    texts = texts_of(paths)
    for mo, mb in ((30, 1), (1, 40), (10, 25)):
        w = E.table(*texts, min_overhang=mo, min_body=mb)
        same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"], min_overhang=mo, min_body=mb), w)


# ----------------------------------------------------------------------------- the grid, the wave

COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 767, 768, 769)
_count_want = {}


@pytest.mark.parametrize("grid", [1, 3, None], ids=["grid1", "grid3", "default"])
@pytest.mark.parametrize("n", COUNTS)
def test_every_count_of_reads(gpu_ctx, tmp_path, monkeypatch, n, grid):
    """reads around a wave, a workgroup and three workgroups; with LSQ_FE_GRID 1 and 3 every workgroup strides"""
    if grid:
        monkeypatch.setenv("LSQ_FE_GRID", str(grid))
    else:
        monkeypatch.delenv("LSQ_FE_GRID", raising=False)
    iso, lines = E.count_case(n, seed=n)
    if n not in _count_want:
        _count_want[n] = E.table("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    (_, report, _, _), _ = check_case(gpu_ctx, tmp_path, "count", iso, lines, want=_count_want[n])
    assert report["reads"] == n


@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "default"])
def test_reads_of_up_to_16_blocks_past_four_workgroups(gpu_ctx, tmp_path, monkeypatch, grid):
    """the lanes of one wave hold between 1 and 16 blocks, every block looks back at all pairs and at the earlier blocks; the long
    form's inner exons are its body, the same reads cross its introns: some form gets both kinds of evidence from one read"""
    if grid:
        monkeypatch.setenv("LSQ_FE_GRID", str(grid))
    iso, lines = V.deep_case()
    (rows, report, _, body), paths = check_case(gpu_ctx, tmp_path, "deep", iso, lines)
    n = {r[2]: r[3] for r in rows}
    assert report["reads"] == 1100 > 4 * 256 and max(len(ln.split(",")) for ln in lines) == 16 and min(len(ln.split(",")) for ln in lines) == 1
    assert body[0] == 1500 and n["D.long"] > 900 and report["informative_occurrences"] > 5 * n["D.long"] and report["body_hits"] > 5 * n["D.long"]
    assert report["several_events"] > 300 and 0 < report["counted_by_body_alone"] < report["counted"]
    # one read, both kinds, one count: D.long's second exon is body, the junction into it is informative
    line = E.mrf_line("chr1", "+", [(1050, 1100), (1300, 1400), (1600, 1650)])
    (one, rep, _, _), _ = check_case(gpu_ctx, tmp_path, "both", iso, [line])
    assert {r[2]: r[3] for r in one}["D.long"] == 1 and rep["informative_occurrences"] == 2 and rep["body_hits"] >= 1 and rep["counted_by_body_alone"] == 0


def test_one_block_over_40_regions_of_40_events(gpu_ctx, tmp_path):
    """a wave with one lane of 40 hits and 63 of none: the cell walk across many cells, and as many rounds of the wave's loop"""
    iso, lines = E.spread_case()
    (rows, report, _, _), _ = check_case(gpu_ctx, tmp_path, "spread", iso, lines)
    assert [r[3] for r in rows] == [5, 0] * 40 and report["body_hits"] == 200 and report["counted"] == 5 == report["several_events"] == report["counted_by_body_alone"]


def test_500_small_regions_nested_in_one_long_region(gpu_ctx, tmp_path):
    """a block inside the long region hits the long one and only those small ones it overlaps"""
    iso, lines = E.nested_case()
    (rows, report, _, body), _ = check_case(gpu_ctx, tmp_path, "nested", iso, lines, fast=True)
    n = {r[2]: r[3] for r in rows}
    assert n["L.ret"] == 700 == report["reads"] and body[0] == 151000 and len(rows) == 1002
    small = sum(v for k, v in n.items() if k.endswith(".inc"))
    assert 0 < small and report["body_hits"] == 700 + small and 100 < report["several_events"] < 700
    # the fast reference is the plain one, on the first reads
    interval, gmap = "".join(iso), V.map_of(iso)
    mrf = "AlignmentBlocks\n" + "".join(lines[:40])
    assert E.fast_table(interval, gmap, mrf) == E.table(interval, gmap, mrf)


_hot_want = {}


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_a_hot_region(gpu_ctx, tmp_path, shuffled):
    """200 000 unspliced reads inside one retained intron beside 1 000 elsewhere: where combining inside the wave can lose or double a hit"""
    iso, lines = E.hot_case(shuffled)
    if "t" not in _hot_want:          # (the table does not depend on the file's order)
        _hot_want["t"] = E.fast_table("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    (rows, report, _, _), _ = check_case(gpu_ctx, tmp_path, "hot", iso, lines, want=_hot_want["t"])
    n = {r[2]: r[3] for r in rows}
    assert n["h2.ret"] == 200000 and n["h2.spl"] == 0 and report["reads"] == 201000


@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "default"])
def test_more_forms_and_events_than_a_workgroup_keeps_counters_for(gpu_ctx, tmp_path, monkeypatch, grid):
    """3000 two-form events: with one workgroup, ids must share a slot of its 2048 form and 1024 event counters, and the others go past them"""
    if grid:
        monkeypatch.setenv("LSQ_FE_GRID", str(grid))
    iso, lines = E.many_case()
    (rows, report, introns, body), _ = check_case(gpu_ctx, tmp_path, "many_ids", iso, lines, fast=True)
    assert len(rows) == 6000 and introns == [2, 1] * 3000 and body == [100, 0] * 3000 and report["several_events"] == 0
    assert [r[3] for r in rows] == [v for g in range(3000) for v in ((1 if g % 7 == 0 else 0), 2)] and [r[1] for r in rows[::2]] == [3 if g % 7 == 0 else 2 for g in range(3000)]
    assert report["counted_by_body_alone"] == report["body_hits"] == len(range(0, 3000, 7))


# ----------------------------------------------------------------------------- context

def test_a_context_with_events_and_counted_reads_is_left_as_it_was(formats):
    from test_sam_gpu import count_table
    paths, want, _, _ = formats
    toy = toy_paths()
    ix = index_of(paths)
    ev = L.Events(L.Annotation(toy["interval"], toy["map"], 0, 10), ("SHORT_READ",), (50,))
    ctx = L.Context(0)
    ctx.upload_events(ev)
    ctx.upload_reads_mrf(0, toy["mrf"])
    before = count_table(ctx, ev)
    assert before == open(toy["count"]).read()
    same(ix.device(ctx, "MRF_SINGLE", paths["mrf"]), want)
    assert count_table(ctx, ev) == before
    ctx.close()


# ----------------------------------------------------------------------------- executable

def test_the_executable(formats, tmp_path):
    paths, want, _, pos = formats
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == E.text(want[0]), p.stderr
    ix = index_of(paths)
    assert E.report_line(want[1], ix.num_introns, ix.num_regions, ix.num_forms, ix.num_events) in p.stderr
    out = str(tmp_path / "out.tab")
    p = tool(paths, paths["bam"], "BAM_SINGLE", opts=["--psi", "--read-length", "50"], out=out)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == E.text(want[0], want[2], want[3], pos)
    texts = texts_of(paths)
    p = tool(paths, paths["sam"], "SAM_SINGLE", opts=["--psi", "--read-length", "30", "--min-overhang", "10", "--min-body", "25"])
    w = E.table(*texts, min_overhang=10, min_body=25)
    assert p.returncode == 0 and p.stdout == E.text(w[0], w[2], w[3], E.positions(texts[0], texts[1], 30, 10, 25)) and w[0] != want[0]
    p = tool(paths, paths["mrf"], opts=["--psi"])
    assert p.returncode == 1 and p.stdout == ""


def test_a_malformed_record_gives_counts_status_and_message(gpu_ctx, formats, tmp_path):
    paths, want, _, _ = formats
    ix = index_of(paths)
    sam = "@HD\tVN:1.6\n" + "q\t0\tchr1\t101\t60\t50M10N50M\t*\t0\t0\t*\t*\n" * 7 + "q\t0\tchr1\t101\t60\t50Q\t*\t0\t0\t*\t*\n"
    spath = str(tmp_path / "bad.sam")
    open(spath, "w").write(sam)
    with pytest.raises(L.LsqError) as host:
        ix.host("SAM_SINGLE", spath)
    with pytest.raises(L.LsqError) as e:
        ix.device(gpu_ctx, "SAM_SINGLE", spath)
    assert e.value.status == LSQ_E_PARSE and str(e.value) == str(host.value)
    out = str(tmp_path / "never.tab")
    p = tool(paths, spath, "SAM_SINGLE", opts=["--psi", "--read-length", "50"], out=out)
    assert p.returncode == 1 and p.stdout == "" and "#9:q\t0\tchr1\t101\t60\t50Q" in p.stderr and "Lexical_cast error" in p.stderr and not os.path.exists(out)
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), want)         # the context is as good as before


def test_two_samples_through_test_as_fisher(gpu_ctx, tmp_path):
    """the tables of two samples are a differential splicing test of retained introns: for every event the p-value of the 2x2 of
    the reference's counts, retaining form against spliced form"""
    iso, lines = E.hot_case(True, 300, 600)
    tables, wants = [], []
    for k in range(2):
        interval, mrf, paths = E.write_case(str(tmp_path), "s%d" % k, iso, [ln for j, ln in enumerate(lines) if (j * 7 + 3 * k) % 4 != 1])
        wants.append(E.table(interval, open(paths["map"]).read(), mrf)[0])
        tables.append(str(tmp_path / ("s%d.tab" % k)))
        assert tool(paths, paths["mrf"], out=tables[-1]).returncode == 0
        assert open(tables[-1]).read() == E.text(wants[-1])
    p = subprocess.run([os.path.join(BIN, "test_as"), "fisher", "--tables", "-"] + tables, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0, p.stderr
    out = [ln.split("\t") for ln in p.stdout.split("\n")[:-1]]
    assert out[0] == ["ID", "rawP", "bonP", "bhP"]
    a, b = wants
    cells = [[a[r][3], b[r][3], a[r + 1][3], b[r + 1][3]] for r in range(0, 12, 2)]
    assert [ln[0] for ln in out[1:]] == ["h%d.spl" % g for g in range(6)] and all(min(c) > 0 for g, c in enumerate(cells) if g != 2)
    pv = ds.fisher(gpu_ctx, np.array(cells, np.float64))
    assert [float(ln[1]) for ln in out[1:]] == [float("%.15g" % v) for v in pv] and (pv < 1).any()
