"""Junction reads per event form on the device (lsq_ps_device: lsq_readfile.hip, lsq_psi.hip): the count kernel at the smallest
shapes at which it can go wrong, against the definition as tests/psi_ref.py restates it and against lsq_ps_host.  All values are
integers, psi is computed on the host from them: the device table equals both exactly, report and text included.  Need an MI355X:
python -m pytest tests -m gpu."""
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
import psi_ref as V
from lesseq_amd import diffsplice as ds
from test_psi_host import index_of, same, tool as host_tool, toy_paths, s1_paths, want_of, random_files, BIN, LSQ_E_PARSE, TOY_TABLE, TOY_PSI_TABLE, TOY_REPORT
from test_sam_gpu import CHILD_TIMEOUT

pytestmark = pytest.mark.gpu


def check_paths(ctx, paths, want, min_overhang=1):
    ix = index_of(paths)
    dev = ix.device(ctx, "MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(dev, want)
    host = ix.host("MRF_SINGLE", paths["mrf"], min_overhang=min_overhang)
    same(host, want)
    assert (dev.reads == host.reads).all() and (dev.total == host.total).all() and dev.report == host.report and dev.text(psi=True) == host.text(psi=True)
    assert set(dev.times) == set(L.psi.PHASES) and all(v >= 0 for v in dev.times.values())


def check_case(ctx, d, stem, iso, lines, want=None, header="AlignmentBlocks\n", min_overhang=1):
    """the device table and the host table against the reference's; returns (want, paths)"""
    interval, mrf, paths = V.write_case(str(d), stem, iso, lines, header)
    want = want or V.table(interval, open(paths["map"]).read(), mrf, min_overhang=min_overhang)
    check_paths(ctx, paths, want, min_overhang)
    return want, paths


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None, out=None):
    return host_tool(paths, reads, fmt, opts, env, host=False, timeout=CHILD_TIMEOUT, out=out)


# ----------------------------------------------------------------------------- the definition

def test_the_toy_example(gpu_ctx):
    paths = toy_paths()
    got = index_of(paths).device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    assert got.text() == TOY_TABLE and got.text(psi=True) == TOY_PSI_TABLE and got.report == TOY_REPORT
    check_paths(gpu_ctx, paths, want_of(paths))


def test_definition_cases(gpu_ctx, tmp_path):
    (rows, report, introns), _ = check_case(gpu_ctx, tmp_path, "base", V.definition_annotation(), V.definition_lines())
    assert rows == V.DEFINITION_ROWS and report == V.DEFINITION_REPORT and introns == V.DEFINITION_INTRONS


def test_events_s1(gpu_ctx):
    paths = s1_paths()
    want = want_of(paths)
    check_paths(gpu_ctx, paths, want)
    assert {r[2]: r[3] for r in want[0]}["15.b"] == 5


@pytest.mark.parametrize("n", [1, 10])
def test_the_junction_rules_edges(gpu_ctx, tmp_path, n):
    for m in sorted({1, n, n + 1}):
        (rows, report, _), _ = check_case(gpu_ctx, tmp_path, "rule%d" % m, V.definition_annotation(), [ln for ln, _ in V.rule_lines(n)], min_overhang=m)
        if m == n:
            assert {r[2]: r[3] for r in rows}["SE.skp"] == 5 and report["no_chromosome"] == 1


def test_files_without_a_hit(gpu_ctx, tmp_path):
    iso = V.definition_annotation()
    for stem, lines, header in (("header_only", [], "AlignmentBlocks\n"), ("nothing", [], ""), ("unknown", [V.mrf_line("chrU", "+", [(1050, 1100), (1500, 1550)])] * 300, "AlignmentBlocks\n"),
                                ("unspliced", [V.mrf_line("chr1", "+", [(1000, 1600)])] * 300, "AlignmentBlocks\n")):
        (rows, report, _), _ = check_case(gpu_ctx, tmp_path, stem, iso, lines, header=header)
        assert all(r[1] == 0 and r[3] == 0 for r in rows) and len(rows) == 18 and report["reads"] == len(lines) and report["counted"] == 0


# ----------------------------------------------------------------------------- formats

@pytest.fixture(scope="module")
def formats(tmp_path_factory):
    return random_files(str(tmp_path_factory.mktemp("psgpu")))


def test_one_table_from_mrf_sam_and_bam(gpu_ctx, formats):
    paths, want, fewer = formats
    ix = index_of(paths)
    tables = [ix.device(gpu_ctx, fmt, paths[key]) for fmt, key in (("MRF_SINGLE", "mrf"), ("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam"))]
    for t in tables:
        same(t, want)
        assert (t.reads == tables[0].reads).all() and (t.total == tables[0].total).all() and t.report == tables[0].report
    same(ix.host("MRF_SINGLE", paths["mrf"]), want)
    ctx = L.Context(0)
    ctx.set_option("sam_min_mapq", 4)
    for fmt, key in (("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam")):
        same(ix.device(ctx, fmt, paths[key]), fewer)
        same(ix.host(fmt, paths[key], min_mapq=4), fewer)
    ctx.close()
    for fmt in ("UCSC_GFF", "MRF_PAIRED"):
        with pytest.raises(L.LsqError) as e:
            ix.device(gpu_ctx, fmt, paths["mrf"])
        assert e.value.status == -3 and str(e.value).endswith("Unknown file format error: " + fmt)
    with pytest.raises(L.LsqError) as e:
        ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"], min_overhang=0)
    assert e.value.status == -1
    a, b = ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"])          # the same from run to run
    assert a.rows() == b.rows() == want[0] and a.report == b.report


# ----------------------------------------------------------------------------- the grid, the wave

COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 767, 768, 769)
_count_want = {}


@pytest.mark.parametrize("grid", [1, 3, None], ids=["grid1", "grid3", "default"])
@pytest.mark.parametrize("n", COUNTS)
def test_every_count_of_reads(gpu_ctx, tmp_path, monkeypatch, n, grid):
    """reads around a wave, a workgroup and three workgroups; with LSQ_PS_GRID 1 and 3 every workgroup strides"""
    if grid:
        monkeypatch.setenv("LSQ_PS_GRID", str(grid))
    else:
        monkeypatch.delenv("LSQ_PS_GRID", raising=False)
    iso, lines = V.count_case(n, seed=n)
    if n not in _count_want:
        _count_want[n] = V.table("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    (_, report, _), _ = check_case(gpu_ctx, tmp_path, "count", iso, lines, want=_count_want[n])
    assert report["reads"] == n


@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "default"])
def test_reads_of_up_to_16_blocks_past_four_workgroups(gpu_ctx, tmp_path, monkeypatch, grid):
    """the lanes of one wave hold between 0 and 15 pairs, and every pair behind the first looks back at its read's earlier ones"""
    if grid:
        monkeypatch.setenv("LSQ_PS_GRID", str(grid))
    iso, lines = V.deep_case()
    (rows, report, _), _ = check_case(gpu_ctx, tmp_path, "deep", iso, lines)
    n = {r[2]: r[3] for r in rows}
    assert report["reads"] == 1100 > 4 * 256 and max(len(ln.split(",")) for ln in lines) == 16 and min(len(ln.split(",")) for ln in lines) == 1
    assert n["D.odd"] == n["D.ends"] == n["E.b"] == 0 and n["D.long"] > 900 and report["informative_occurrences"] > 5 * n["D.long"] and report["several_events"] > 300


_hot_want = {}


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_a_hot_intron(gpu_ctx, tmp_path, shuffled):
    """200 000 reads on one junction beside 1 000 on others: where combining inside the wave can lose or double a hit"""
    iso, lines = V.hot_case(shuffled)
    if "t" not in _hot_want:          # (the table does not depend on the file's order)
        _hot_want["t"] = V.fast_table("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    (rows, report, _), _ = check_case(gpu_ctx, tmp_path, "hot", iso, lines, want=_hot_want["t"])
    n = {r[2]: r[3] for r in rows}
    assert n["h2.skp"] == 200000 and n["h2.inc"] == 0 and report["reads"] == 201000


@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "default"])
def test_more_forms_and_events_than_a_workgroup_keeps_counters_for(gpu_ctx, tmp_path, monkeypatch, grid):
    """3000 two-form events: with one workgroup, ids must share a slot of its 2048 form and 1024 event counters, and the others go past them"""
    if grid:
        monkeypatch.setenv("LSQ_PS_GRID", str(grid))
    iso, lines = V.many_case()
    want = V.fast_table("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    (rows, report, introns), _ = check_case(gpu_ctx, tmp_path, "many_ids", iso, lines, want=want)
    assert len(rows) == 6000 and introns == [2, 1] * 3000 and report["several_events"] == 0
    assert [r[3] for r in rows] == [v for g in range(3000) for v in ((1 if g % 7 == 0 else 0), 2)] and [r[1] for r in rows[::2]] == [3 if g % 7 == 0 else 2 for g in range(3000)]


# ----------------------------------------------------------------------------- context

def test_a_context_with_events_and_counted_reads_is_left_as_it_was(formats):
    from test_sam_gpu import count_table
    paths, want, _ = formats
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
    paths, want, _ = formats
    p = tool(paths, paths["mrf"])
    assert p.returncode == 0 and p.stdout == V.text(want[0]), p.stderr
    ix = index_of(paths)
    assert V.report_line(want[1], ix.num_introns, ix.num_forms, ix.num_events) in p.stderr
    out = str(tmp_path / "out.tab")
    p = tool(paths, paths["bam"], "BAM_SINGLE", opts=["--psi"], out=out)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == V.text(want[0], want[2])
    p = tool(paths, paths["sam"], "SAM_SINGLE", opts=["--psi", "--min-overhang", "30"])
    w = V.table(open(paths["interval"]).read(), open(paths["map"]).read(), open(paths["mrf"]).read(), min_overhang=30)
    assert p.returncode == 0 and p.stdout == V.text(w[0], w[2]) != V.text(want[0], want[2])


def test_a_malformed_record_gives_counts_status_and_message(gpu_ctx, formats, tmp_path):
    paths, want, _ = formats
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
    p = tool(paths, spath, "SAM_SINGLE", opts=["--psi"], out=out)
    assert p.returncode == 1 and p.stdout == "" and "#9:q\t0\tchr1\t101\t60\t50Q" in p.stderr and "Lexical_cast error" in p.stderr and not os.path.exists(out)
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), want)         # the context is as good as before


def test_two_samples_through_test_as_fisher(gpu_ctx, formats, tmp_path):
    """the tables of two samples are a junction-count differential splicing test: for every two-form event the p-value of the
    2x2 of the reference's counts"""
    paths, want, _ = formats
    lines = open(paths["mrf"]).read().split("\n")[1:-1]
    interval, gmap = open(paths["interval"]).read(), open(paths["map"]).read()
    tables, wants = [], []
    for k in range(2):
        sample = str(tmp_path / ("s%d.mrf" % k))
        open(sample, "w").write("AlignmentBlocks\n" + "".join(ln + "\n" for j, ln in enumerate(lines) if (j * 7 + 3 * k) % 4 != 1))
        wants.append(V.table(interval, gmap, open(sample).read())[0])
        tables.append(str(tmp_path / ("s%d.tab" % k)))
        assert tool(paths, sample, out=tables[-1]).returncode == 0
        assert open(tables[-1]).read() == V.text(wants[-1])
    p = subprocess.run([os.path.join(BIN, "test_as"), "fisher", "--tables", "-"] + tables, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0, p.stderr
    out = [ln.split("\t") for ln in p.stdout.split("\n")[:-1]]
    assert out[0] == ["ID", "rawP", "bonP", "bhP"]
    a, b = wants
    ids, cells = [], []
    for r in range(len(a) - 1):
        if a[r][0] == a[r + 1][0] and sum(x[0] == a[r][0] for x in a) == 2:
            ids.append(a[r + 1][2])
            cells.append([a[r][3], b[r][3], a[r + 1][3], b[r + 1][3]])
    assert [ln[0] for ln in out[1:]] == ids and len(ids) > 10 and np.array(cells).sum() > 1000
    pv = ds.fisher(gpu_ctx, np.array(cells, np.float64))
    assert [float(ln[1]) for ln in out[1:]] == [float("%.15g" % v) for v in pv] and (pv < 1).any()
