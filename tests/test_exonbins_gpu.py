"""Reads per exon bin and per gene on the device (lsq_xb_device: lsq_readfile.hip, lsq_exonbins.hip): the count kernel at the
smallest shapes at which it can go wrong, against the definition as tests/exonbins_ref.py restates it and against lsq_xb_host.
All values are integers: the device table equals both exactly.  Need an MI355X: python -m pytest tests -m gpu."""
import os
import subprocess

import pytest

import lesseq_amd as L
import exonbins_ref as V
from test_exonbins_host import index_of, same, tool as host_tool, toy_paths, random_files, BIN, LSQ_E_PARSE, TOY_TABLE, TOY_REPORT
from test_sam_gpu import CHILD_TIMEOUT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def check_case(ctx, d, stem, iso, lines, want=None, header="AlignmentBlocks\n"):
    """the device table and the host table against the reference's; returns (want, paths)"""
    interval, mrf, paths = V.write_case(str(d), stem, iso, lines, header)
    gmap = open(paths["map"]).read()
    want = want or V.table(interval, gmap, mrf)
    ix = index_of(paths)
    dev = ix.device(ctx, "MRF_SINGLE", paths["mrf"])
    same(dev, want)
    host = ix.host("MRF_SINGLE", paths["mrf"])
    same(host, want)
    assert (dev.reads == host.reads).all() and (dev.total == host.total).all()
    assert set(dev.times) == set(L.exonbins.PHASES) and all(v >= 0 for v in dev.times.values())
    return want, paths


def tool(paths, reads, fmt="MRF_SINGLE", opts=(), env=None, out=None):
    return host_tool(paths, reads, fmt, opts, env, host=False, timeout=CHILD_TIMEOUT, out=out)


# ----------------------------------------------------------------------------- the definition

def test_the_toy_example(gpu_ctx):
    paths = toy_paths()
    got = index_of(paths).device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    assert got.text() == TOY_TABLE and got.report == TOY_REPORT


def test_definition_cases(gpu_ctx, tmp_path):
    (rows, report), _ = check_case(gpu_ctx, tmp_path, "base", V.definition_annotation(), V.definition_lines())
    n = {r[2]: r[3] for r in rows}
    assert [n["ovB:%d" % k] for k in (1, 2, 3, 4)] == [1, 2, 1, 2] and n["big:30"] == 2 and n["edge:1"] == 1 and report["several_genes"] == 7


def test_overlapping_genes(gpu_ctx, tmp_path):
    iso, lines = V.overlap_case(3000)
    (_, report), _ = check_case(gpu_ctx, tmp_path, "overlap", iso, lines)
    assert report["several_genes"] > 2000


def test_files_without_a_hit(gpu_ctx, tmp_path):
    iso = V.definition_annotation()
    for stem, lines, header in (("header_only", [], "AlignmentBlocks\n"), ("nothing", [], ""), ("none_hit", [V.mrf_line("chrU", "+", [(1, 9)])] * 300, "AlignmentBlocks\n"),
                                ("beside", [V.mrf_line("chr1", "+", [(1200, 1300)])] * 300, "AlignmentBlocks\n")):
        (rows, report), _ = check_case(gpu_ctx, tmp_path, stem, iso, lines, header=header)
        assert all(r[1] == 0 and r[3] == 0 for r in rows) and len(rows) > 90 and report["reads"] == len(lines) == report["no_gene"]


# ----------------------------------------------------------------------------- formats

@pytest.fixture(scope="module")
def formats(tmp_path_factory):
    return random_files(str(tmp_path_factory.mktemp("xbgpu")))


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
    ctx.close()
    for fmt in ("UCSC_GFF", "MRF_PAIRED"):
        with pytest.raises(L.LsqError) as e:
            ix.device(gpu_ctx, fmt, paths["mrf"])
        assert e.value.status == -3 and str(e.value).endswith("Unknown file format error: " + fmt)


# ----------------------------------------------------------------------------- the grid, the wave

COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 767, 768, 769)
_count_want = {}


@pytest.mark.parametrize("grid", [1, 3, None], ids=["grid1", "grid3", "default"])
@pytest.mark.parametrize("n", COUNTS)
def test_every_count_of_reads(gpu_ctx, tmp_path, monkeypatch, n, grid):
    """reads around a wave, a workgroup and three workgroups; with LSQ_XB_GRID 1 and 3 every workgroup strides"""
    if grid:
        monkeypatch.setenv("LSQ_XB_GRID", str(grid))
    else:
        monkeypatch.delenv("LSQ_XB_GRID", raising=False)
    iso, lines = V.overlap_case(n, seed=n)
    if n not in _count_want:
        _count_want[n] = V.table("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    (_, report), _ = check_case(gpu_ctx, tmp_path, "count", iso, lines, want=_count_want[n])
    assert report["reads"] == n


@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "default"])
def test_strides_over_reads_of_many_blocks(gpu_ctx, tmp_path, monkeypatch, grid):
    if grid:
        monkeypatch.setenv("LSQ_XB_GRID", str(grid))
    lines = V.definition_lines() * 40
    (_, report), _ = check_case(gpu_ctx, tmp_path, "many", V.definition_annotation(), lines)
    assert report["reads"] == 40 * 37 > 4 * 256


_hot_want = {}


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_a_hot_bin(gpu_ctx, tmp_path, shuffled):
    """200 000 reads inside one bin beside 1 000 spread over the rest: where combining inside the wave can lose or double a hit"""
    iso, lines = V.hot_case(shuffled)
    if "t" not in _hot_want:          # (the table does not depend on the file's order)
        _hot_want["t"] = V.table_of_one_block_reads("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    (rows, report), _ = check_case(gpu_ctx, tmp_path, "hot", iso, lines, want=_hot_want["t"])
    n = {r[2]: r[3] for r in rows}
    assert n["hot:2"] == 200000 and n["hot:1"] == n["hot:3"] == 0 and report["reads"] == 201000


@pytest.mark.parametrize("kind", ["distinct", "alternate"])
def test_a_wave_of_different_bins(gpu_ctx, tmp_path, kind):
    iso, lines = V.wave_case(kind)
    (rows, report), _ = check_case(gpu_ctx, tmp_path, kind, iso, lines)
    n = {r[2]: r[3] for r in rows}
    if kind == "distinct":
        assert [n["w:%d" % (k + 1)] for k in range(64)] == [4] * 17 + [3] * 47 and rows[0][:2] == ("v", 0)
    else:
        assert (n["v:1"], n["v:2"]) == (105, 104) and rows[-1][:2] == ("w", 0)


@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "default"])
def test_more_bins_and_genes_than_a_workgroup_keeps_counters_for(gpu_ctx, tmp_path, monkeypatch, grid):
    """3000 one-bin genes: with one workgroup, ids must share a slot of its 2048 bin and 1024 gene counters, and the others go past them"""
    if grid:
        monkeypatch.setenv("LSQ_XB_GRID", str(grid))
    iso, lines = V.many_case()
    want = V.table_of_one_block_reads("".join(iso), V.map_of(iso), "AlignmentBlocks\n" + "".join(lines))
    (rows, report), _ = check_case(gpu_ctx, tmp_path, "many_ids", iso, lines, want=want)
    assert len(rows) == 3000 and [r[1] for r in rows] == [r[3] for r in rows] == [3 if g % 7 == 0 else 2 for g in range(3000)] and report["no_gene"] == 0


def test_the_same_from_run_to_run(gpu_ctx, formats):
    paths, want, _ = formats
    ix = index_of(paths)
    a, b = ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    assert a.rows() == b.rows() == want[0] and a.report == b.report


# ----------------------------------------------------------------------------- context

def test_a_context_with_events_and_counted_reads_is_left_as_it_was(formats):
    from test_sam_gpu import count_table
    paths, want, _ = formats
    d = os.path.join(GOLD, "toy")
    ix = index_of(paths)
    ev = L.Events(L.Annotation(os.path.join(d, "toy.interval"), os.path.join(d, "toy.map"), 0, 10), ("SHORT_READ",), (50,))
    ctx = L.Context(0)
    ctx.upload_events(ev)
    ctx.upload_reads_mrf(0, os.path.join(d, "toy.mrf"))
    before = count_table(ctx, ev)
    assert before == open(os.path.join(d, "count.out")).read()
    same(ix.device(ctx, "MRF_SINGLE", paths["mrf"]), want)
    assert count_table(ctx, ev) == before
    same(ix.device(ctx, "SAM_SINGLE", paths["sam"]), want)
    ctx.upload_reads_mrf(0, os.path.join(d, "toy.mrf"))                # the events' dictionaries still serve an upload
    assert count_table(ctx, ev) == before
    ctx.close()


# ----------------------------------------------------------------------------- executable

def test_the_executable(formats, tmp_path):
    paths, want, _ = formats
    p = tool(paths, paths["mrf"])
    h = host_tool(paths, paths["mrf"])
    assert p.returncode == 0 and h.returncode == 0 and p.stdout == h.stdout == V.text(want[0]), p.stderr
    ix = index_of(paths)
    assert V.report_line(want[1], ix.num_bins, ix.num_genes) in p.stderr
    prefix, out = str(tmp_path / "bins"), str(tmp_path / "out.tab")
    p = tool(paths, paths["bam"], "BAM_SINGLE", opts=["--bins", prefix], out=out)
    assert p.returncode == 0 and p.stdout == "" and open(out).read() == V.text(want[0])
    assert (open(prefix + ".interval").read(), open(prefix + ".map").read()) == ix.bins_text()


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
    prefix, out = str(tmp_path / "never"), str(tmp_path / "never.tab")
    p = tool(paths, spath, "SAM_SINGLE", opts=["--bins", prefix], out=out)
    assert p.returncode == 1 and p.stdout == "" and "#9:q\t0\tchr1\t101\t60\t50Q" in p.stderr and "Lexical_cast error" in p.stderr
    assert not os.path.exists(out) and not os.path.exists(prefix + ".interval") and not os.path.exists(prefix + ".map")
    # the context is as good as before
    same(ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"]), want)


def test_four_tables_through_test_as_lrt(formats, tmp_path):
    """the tables of four samples are a differential exon usage test: one row per bin"""
    paths, want, _ = formats
    lines = open(paths["mrf"]).read().split("\n")[1:-1]
    tables = []
    for k in range(4):
        sample = str(tmp_path / ("s%d.mrf" % k))
        open(sample, "w").write("AlignmentBlocks\n" + "".join(ln + "\n" for j, ln in enumerate(lines) if (j * 7 + k) % 4 != 1 or k < 2))
        tables.append(str(tmp_path / ("s%d.tab" % k)))
        assert tool(paths, sample, out=tables[-1]).returncode == 0
    p = subprocess.run([os.path.join(BIN, "test_as"), "lrt", "--tables", "2", "2", "-"] + tables, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0, p.stderr
    out = p.stdout.split("\n")
    assert out[0].split("\t")[0] == "ID" and [ln.split("\t")[0] for ln in out[1:-1]] == [r[2] for r in want[0]]
