"""Stranded counting in the read-file tools on the device (lsq_stranded.hip: the stranded forms of the exonbins, psi
and evidence count kernels; lsq_libtype.hip) at the smallest shapes at which they can go wrong, against the split definition as tests/stranded_tools_ref.py
restates it and against the host paths.  All values are integers: tables, reports and library reports equal both exactly.
Need an MI355X: python -m pytest tests -m gpu."""
import random

import pytest

import lesseq_amd as L
import evidence_ref
import test_stranded_tools_host as H
import stranded_inputs as S
import stranded_tools_ref as R
from test_stranded_tools_host import TOOLS, FORMATS, tools, libs, hand_case
from test_sam_gpu import CHILD_TIMEOUT

pytestmark = pytest.mark.gpu

HEADER = S.SAM_HEADER + ["@SQ\tSN:chrD\tLN:100000"]


class CrossRec(S.Rec):
    """a record whose blocks lie on more than one chromosome: an MRF line alone can say that"""

    def __init__(self, flag, blocks):
        super().__init__(blocks[0][0], flag, [(s, e) for _, s, e in blocks], mrf_strand="-" if flag & 16 else "+")
        self.chroms = [c for c, _, _ in blocks]

    def mrf_line(self, strand):
        out, q = [], 1
        for c, (s, e) in zip(self.chroms, self.blocks):
            out.append("%s:%s:%d:%d:%d:%d" % (c, strand, s + 1, e, q, q + e - s - 1))
            q += e - s
        return ",".join(out)


def two_forms(name, chrom, strand, at):
    """a gene of three exons with a form that skips the second: three bins; an informative intron for either form"""
    ex = [(at, at + 100), (at + 300, at + 400), (at + 600, at + 700)]
    return S.Gene(name, chrom, strand, [(name + ".inc", ex), (name + ".skp", [ex[0], ex[2]])])


def shapes_case(seed=5, n=640):
    """An antisense pair of identical coordinates (the same bins and introns in both tables of chrA), a chromosome of plus genes
    alone (its minus table is empty), the last chromosome with a minus gene alone (the highest table id, whose successor is the
    offsets' last entry), a chromosome the annotation lacks; reads of all six flags in turn, so every wave holds both transcript
    strands; in the MRF file alone: reads whose blocks change chromosome, and reads without a transcript strand first, last and in
    the middle of a wave.  More reads than one stride of a grid of one workgroup."""
    genes = [two_forms("ap", "chrA", "+", 1000), two_forms("am", "chrA", "-", 1000), two_forms("aq", "chrA", "+", 3000),
             two_forms("bp1", "chrB", "+", 500), two_forms("bp2", "chrB", "+", 2500), two_forms("dm", "chrD", "-", 1000)]
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        g = genes[rng.randrange(len(genes))]
        _, exons = g.isoforms[rng.randrange(2)]
        nb = rng.choice([1, 2, 2, len(exons)])
        chrom = "chrC" if i % 53 == 17 else g.chrom
        recs.append(S.Rec(chrom, S.FLAGS[i % 6], S.reads_along(rng, exons, nb)))
    cross = [CrossRec(16, [("chrA", 1050, 1090), ("chrD", 1060, 1100), ("chrD", 1300, 1340)]),      # minus: am, then dm and its first intron
             CrossRec(0, [("chrD", 1060, 1100), ("chrA", 1300, 1340), ("chrA", 1600, 1640)]),       # plus: nothing on chrD, ap on chrA
             CrossRec(0, [("chrC", 10, 50), ("chrB", 560, 600), ("chrB", 800, 840)])]
    odd = S.mrf_only_records()
    mrf_recs = odd[:1] + recs[:100] + odd[1:2] + cross[:1] + recs[100:400] + cross[1:] + recs[400:] + odd[2:]
    return genes, recs, mrf_recs


def many_ids_case(tool, n_each=1300, seed=9):
    """more bins (forms) and genes (events) than a workgroup keeps counters of its own for -- 2048 and 1024 -- with the minus
    strand's at the high ids (names sort bytewise); exonbins: one-block reads, psi: reads over a junction"""
    genes = [two_forms("a%04d" % g, "chrA", "+", 1000 * g) for g in range(n_each)] + [two_forms("z%04d" % g, "chrA", "-", 1000 * g + 200000) for g in range(n_each)]
    rng = random.Random(seed)
    recs = []
    for i in range(3000):
        g = genes[rng.randrange(len(genes))]
        at = g.isoforms[0][1][0][0]
        if tool.name == "exonbins":
            s0 = at + rng.choice((20, 320, 620))
            blocks = [(s0, s0 + 40)]
        else:
            blocks = rng.choice(([(at + 60, at + 100), (at + 300, at + 340)], [(at + 60, at + 100), (at + 600, at + 640)], [(at + 360, at + 400), (at + 600, at + 640)]))
        recs.append(S.Rec("chrA", S.FLAGS[i % 6], blocks))
    return genes, recs


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("strshapes"))
    genes, recs, mrf_recs = shapes_case()
    paths = S.write_inputs(d, "shapes", genes, recs, header=HEADER)
    with open(paths["mrf"], "w") as f:
        f.write(S.input_mrf(mrf_recs, len(HEADER)))
    return genes, recs, mrf_recs, paths


_want = {}


def want_of(tool, key, genes, recs, lib, **kw):
    k = (tool.name, key, lib)
    if k not in _want:
        _want[k] = (R.expected(tool.ref, genes, recs, lib, n_comment=len(HEADER), **kw) if lib != "unstranded" else
                    (R.unstranded(tool.ref, genes, recs, n_comment=len(HEADER), **kw), None))
    return _want[k]


def check(tool, ctx, ix, fmt, path, want, lib_report):
    dev = ix.device(ctx, fmt, path)
    tool.same(dev, want)
    assert dev.library_report() == lib_report
    host = ix.host(fmt, path)
    assert (dev.reads == host.reads).all() and (dev.total == host.total).all() and dev.report == host.report and host.library_report() == lib_report
    return dev


@tools
@libs
@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "default"])
def test_the_shapes_at_which_a_stranded_kernel_can_go_wrong(gpu_ctx, shapes, monkeypatch, tool, lib, grid):
    if grid:
        monkeypatch.setenv(tool.grid_env, str(grid))
    else:
        monkeypatch.delenv(tool.grid_env, raising=False)
    genes, recs, mrf_recs, paths = shapes
    want, lib_report = want_of(tool, "shapes_mrf", genes, mrf_recs, lib)
    ix = tool.index(paths, lib)
    assert ix.chrom_names() == ["chrA", "chrB", "chrD"]
    dev = check(tool, gpu_ctx, ix, "MRF_SINGLE", paths["mrf"], want, lib_report)
    rows = {r[2]: r for r in dev.rows()}
    # reads without a strand are tallied and count for nothing; both strands count; the antisense pair differs from the unstranded table
    assert lib_report["no_strand"] == 3 and lib_report["plus_counted"] > 50 and lib_report["minus_counted"] > 50 and dev.report["reads"] == len(mrf_recs) > 2 * 256
    unstranded, _ = want_of(tool, "shapes_mrf", genes, mrf_recs, "unstranded")
    u = {r[2]: r for r in unstranded[0]}
    first = "ap:1" if tool.name == "exonbins" else "ap.inc"
    assert rows[first][1] < u[first][1] and rows[first.replace("ap", "am")][1] < u[first.replace("ap", "am")][1]
    assert rows[first.replace("ap", "dm")][1] > 0 and rows[first.replace("ap", "bp1")][1] > 0


@tools
@libs
def test_one_table_from_mrf_sam_and_bam(gpu_ctx, shapes, tool, lib):
    """the second-mate flags 0x81 / 0x91 land on the strand of their first mate in all three formats; an unstranded index through
    the same context afterwards gives the unstranded table: nothing sticks to the context"""
    genes, recs, _, paths = shapes
    want, lib_report = want_of(tool, "shapes", genes, recs, lib)
    ix = tool.index(paths, lib)
    only_recs = paths["mrf"] + ".recs"
    with open(only_recs, "w") as f:
        f.write(S.input_mrf(recs, len(HEADER)))
    tables = [check(tool, gpu_ctx, ix, fmt, only_recs if key == "mrf" else paths[key], want, lib_report) for fmt, key in FORMATS]
    assert all(t.report == tables[0].report for t in tables) and lib_report["no_strand"] == 0
    mates = [r for r in recs if r.flag & 0x80]
    assert len(mates) > 100 and {r.t(lib) for r in mates} == {0, 1}
    plain, _ = want_of(tool, "shapes", genes, recs, "unstranded")
    for fmt, key in FORMATS[1:]:
        tool.same(tool.index(paths).device(gpu_ctx, fmt, paths[key]), plain)
    check(tool, gpu_ctx, ix, "SAM_SINGLE", paths["sam"], want, lib_report)


@tools
@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "default"])
def test_more_ids_than_a_workgroup_keeps_counters_for(gpu_ctx, tmp_path, monkeypatch, tool, grid):
    """with one workgroup the minus strand's ids, the high ones, find the slots taken and go to the global counters"""
    if grid:
        monkeypatch.setenv(tool.grid_env, str(grid))
    else:
        monkeypatch.delenv(tool.grid_env, raising=False)
    key = "many_" + tool.name
    if key not in _want:
        _want[key] = many_ids_case(tool)
    genes, recs = _want[key]
    paths = S.write_inputs(str(tmp_path), "many", genes, recs, header=HEADER)
    for lib in S.LIBS:
        want, lib_report = want_of(tool, key, genes, recs, lib, table=tool.numpy_table)
        ix = tool.index(paths, lib)
        dev = check(tool, gpu_ctx, ix, "MRF_SINGLE", paths["mrf"], want, lib_report)
        assert len(dev.total) == 2600 and len(dev.reads) > 2048
        assert int((dev.total[:1300] > 0).sum()) > 300 and int((dev.total[1300:] > 0).sum()) > 300


@libs
def test_evidence_counts_a_read_once_for_its_own_strand_and_prints_psi(gpu_ctx, tmp_path, lib):
    """a read that crosses an informative intron of its own strand's event while its second block lies on the body of the
    opposite strand's counts once, for its own strand; the eight columns of --psi --read-length on a stranded table"""
    genes, recs = hand_case()
    paths = S.write_inputs(str(tmp_path), "hand", genes, recs)
    tool = TOOLS[2]
    want, lib_report = R.expected(evidence_ref, genes, recs, lib)
    ix = tool.index(paths, lib)
    dev = ix.device(gpu_ctx, "MRF_SINGLE", paths["mrf"])
    interval, gmap = R.annotation_texts(genes)
    tool.helpers.same(dev, want, pos=evidence_ref.positions(interval, gmap, 50), read_length=50)
    assert dev.library_report() == lib_report and dev.text(psi=True, read_length=50) == ix.host("MRF_SINGLE", paths["mrf"]).text(psi=True, read_length=50)
    rows = {r[2]: r for r in dev.rows()}
    assert rows["M.a"][3] == 1 and rows["P.a"][3] == 1 and dev.report["several_events"] == 0


@tools
def test_the_executable_on_the_device(shapes, tool):
    genes, recs, mrf_recs, paths = shapes
    for lib, fmt, key, case, reads in (("forward", "MRF_SINGLE", "mrf", "shapes_mrf", mrf_recs), ("reverse", "BAM_SINGLE", "bam", "shapes", recs)):
        want, lib_report = want_of(tool, case, genes, reads, lib)
        p = tool.run(paths, paths[key], fmt, opts=["--library", lib], host=False, timeout=CHILD_TIMEOUT)
        h = tool.run(paths, paths[key], fmt, env={"LSQ_LIBRARY": lib})
        assert p.returncode == 0 and h.returncode == 0, p.stderr
        assert p.stdout == h.stdout == tool.ref.text(want[0])
        assert tool.log_line(lib, lib_report) in p.stderr and tool.log_line(lib, lib_report) in h.stderr
    plain = tool.run(paths, paths["mrf"], host=False, timeout=CHILD_TIMEOUT)
    assert plain.returncode == 0 and plain.stdout == tool.ref.text(want_of(tool, "shapes_mrf", genes, mrf_recs, "unstranded")[0][0]) and "library" not in plain.stderr


# ----------------------------------------------------------------------------- libtype

@pytest.mark.parametrize("grid", [1, None], ids=["grid1", "default"])
def test_libtype_equals_the_brute_force_reference_and_the_host_path(gpu_ctx, shapes, monkeypatch, grid):
    """the shapes case: both strands in every wave, a one-strand chromosome, the last chromosome's minus table, reads that change
    chromosome, a chromosome the annotation lacks, reads without a strand first, last and inside a wave; three formats"""
    if grid:
        monkeypatch.setenv("LSQ_LT_GRID", str(grid))
    else:
        monkeypatch.delenv("LSQ_LT_GRID", raising=False)
    genes, recs, mrf_recs, paths = shapes
    ix = H.libtype_index(paths)
    for fmt, key in FORMATS:
        want = R.libtype(genes, mrf_recs if key == "mrf" else recs)
        dev = ix.device(gpu_ctx, fmt, paths[key])
        H.libtype_same(dev, want)
        host = ix.host(fmt, paths[key])
        assert dev.counts == host.counts and dev.text() == host.text()
        assert set(dev.times) == set(L.libtype.PHASES) and all(v >= 0 for v in dev.times.values())
        assert want["reads"] > 2 * 256 and want["no_strand"] == (3 if key == "mrf" else 0) and min(want["sense"], want["antisense"], want["ambiguous"], want["no_gene"]) > 10
    # an unstranded index of another tool through the same context afterwards: nothing sticks to the context
    plain, _ = want_of(TOOLS[0], "shapes", genes, recs, "unstranded")
    TOOLS[0].same(TOOLS[0].index(paths).device(gpu_ctx, "SAM_SINGLE", paths["sam"]), plain)


def test_libtype_a_file_with_no_read_and_one_whose_reads_are_all_ambiguous(gpu_ctx, tmp_path):
    genes, _ = hand_case()
    both = [S.Rec("chrA", S.FLAGS[i % 6], [(110 + i % 40, 160 + i % 40)]) for i in range(300)]      # M and P share every exon
    for tag, recs in (("none", []), ("both", both)):
        paths = S.write_inputs(str(tmp_path), tag, genes, recs)
        want = R.libtype(genes, recs)
        ix = H.libtype_index(paths)
        for fmt, key in FORMATS:
            dev = ix.device(gpu_ctx, fmt, paths[key])
            H.libtype_same(dev, want)
            H.libtype_same(ix.host(fmt, paths[key]), want)
            assert dev.forward_fraction is None and dev.library == "undetermined" and dev.counts["ambiguous"] == len(recs) == dev.counts["reads"]


def test_libtype_verdicts_on_the_device(gpu_ctx, tmp_path):
    for n_sense, n_anti, flip, verdict in ((120, 0, False, "forward"), (120, 0, True, "reverse"), (99, 0, False, "undetermined"), (90, 10, False, "forward"), (60, 40, False, "unstranded")):
        genes, recs = H.sense_case(n_sense, n_anti, flip)
        paths = S.write_inputs(str(tmp_path), "v", genes, recs)
        dev = H.libtype_index(paths).device(gpu_ctx, "BAM_SINGLE", paths["bam"])
        H.libtype_same(dev, R.libtype(genes, recs))
        assert dev.library == verdict


def test_the_libtype_executable_on_the_device(shapes):
    genes, recs, mrf_recs, paths = shapes
    p = H.libtype_tool(paths, paths["mrf"], host=False, timeout=CHILD_TIMEOUT)
    h = H.libtype_tool(paths, paths["mrf"])
    assert p.returncode == 0 and h.returncode == 0, p.stderr
    assert p.stdout == h.stdout == R.libtype_text(R.libtype(genes, mrf_recs)) and p.stderr.count("libtype:") == 1
