"""Intron clusters on the GPU (include/lesseq_hip.h, lsq_cl_device): on every case the device table equals the definition
(tests/clusters_ref.py) and the host table exactly -- arrays, count matrix, report and both texts.  The cases are
tests/clusters_cases.py's, handed in through add_rows unless the test names read files."""
import os
import subprocess

import pytest

import lesseq_amd as L
import bam_writer
import junction_ref as J
import clusters_cases as K
from test_junctions_host import sam_of, BIN
from test_sam_gpu import CHILD_TIMEOUT

pytestmark = pytest.mark.gpu

CASES = dict(K.small_cases(), **K.large_cases())
ROUNDS_CAP = 64        # of the chain of 2^15 + 1 rows: label propagation without jumping needs about 2^15


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("clgpu"))
    interval, paths = K.write_annotation(d)
    ctx = L.Context(0)
    yield d, interval, paths, L.JunctionIndex(L.Annotation(paths["interval"], paths["map"])), ctx
    ctx.close()


_references = {}


def reference(interval, name):
    if name not in _references:
        _references[name] = K.reference(interval, *CASES[name])
    return _references[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_reference_and_the_host(setup, name):
    _, interval, _, ix, ctx = setup
    samples, opts = CASES[name]
    pool = K.pool_of(ix, samples)
    got = pool.device(ctx, **opts)
    want = reference(interval, name)
    K.same(got, want)
    K.same_tables(got, pool.host(**opts))
    assert (got.rounds > 0) == (want.report["kept_rows"] > 0)
    if name == "worked_example":
        assert got.cluster.tolist() == [1, 2, 2, 1, 0, 3, 0, 3, 0]           # numbered along chromosome names: chr10 before chr2, whose index is 0
        assert got.text().split("\n")[:2] == ["clu_1\tchr10\t101\t900\t.\t5\t1", "clu_1\tchr10\t301\t900\t.\t4\t2"]      # by cluster, not by coordinate
    if name == "staircase":
        print("staircase: %d rows, %d rounds" % (len(got), got.rounds))
        assert got.report["clusters"] == 1 and got.report["printed_rows"] == (1 << 15) + 1 and (got.cluster == 1).all()
        assert 2 <= got.rounds <= ROUNDS_CAP
    if name == "staircase_broken":
        assert got.report["clusters"] == 2 and got.report["long_rows"] == 1 and got.rounds <= ROUNDS_CAP
        assert [int((got.cluster == q).sum()) for q in (0, 1, 2)] == [1, 1 << 14, 1 << 14] and got.cluster[0] == 1 and got.cluster[-1] == 2
    if name.startswith("pairs_"):
        n = int(name[6:])
        assert got.report["introns"] == n and got.report["clusters"] == n // 2 and got.report["singletons"] == n % 2
    if name == "empty_pool":
        assert len(got) == 0 and got.text() == "" and got.n_samples == 0 and got.counts.shape == (0, 0)


def test_the_samples_in_another_order(setup):
    _, interval, _, ix, ctx = setup
    samples, opts = CASES["random"]
    first = K.pool_of(ix, samples).device(ctx, **opts)
    order = [2, 0, 3, 1]
    other = K.pool_of(ix, [samples[k] for k in order]).device(ctx, **opts)
    assert other.text() == first.text() == reference(interval, "random").text
    assert [other.sample_text(q) for q in range(4)] == [first.sample_text(k) for k in order]
    assert (other.counts == first.counts[:, order]).all() and (other.cluster == first.cluster).all()


@pytest.mark.parametrize("name", ["random", "staircase"])
def test_two_runs_in_one_context_give_identical_arrays(setup, name):
    _, _, _, ix, ctx = setup
    samples, opts = CASES[name]
    pool = K.pool_of(ix, samples)
    a, b = pool.device(ctx, **opts), pool.device(ctx, **opts)
    K.same_tables(a, b)
    assert max(a.rounds, b.rounds) <= ROUNDS_CAP       # (a stale read may cost a round, never a result: the rounds themselves may differ)


def test_times_has_the_named_phases(setup):
    _, _, _, ix, ctx = setup
    samples, opts = CASES["random"]
    got = K.pool_of(ix, samples).device(ctx, **opts)
    assert tuple(got.times) == ("upload", "sort", "reduce", "filter", "links", "components", "totals", "copy_back") == L.clusters.PHASES
    assert all(v >= 0 for v in got.times.values()) and sum(got.times.values()) > 0
    empty = L.ClusterPool(ix).device(ctx)
    assert empty.times == dict.fromkeys(L.clusters.PHASES, 0.0) and empty.rounds == 0


# ----------------------------------------------------------------------------- through read files

def spliced(chrom, a, b, n, minus=False):
    """n reads of two blocks of 50 bases around the intron [a, b)"""
    return [(chrom, minus, [(a - 50, a), (b, b + 50)])] * n


def file_reads():
    one = spliced("chr10", 200, 400, 6) + spliced("chr10", 200, 500, 5) + spliced("chr10", 300, 900, 4, True) + spliced("chr2", 100, 900, 3) + [("chr1", False, [(10, 90)])]
    two = spliced("chr10", 200, 400, 2) + spliced("chr10", 100, 900, 7) + spliced("chr10", 300, 900, 1) + spliced("chr2", 100, 900, 9, True) + spliced("chr2", 100, 950, 8)
    return one, two


@pytest.fixture(scope="module")
def read_files(setup):
    d, interval, paths, ix, ctx = setup
    files, samples = {}, []
    for stem, reads in zip(("one", "two"), file_reads()):
        mrf = "AlignmentBlocks\n" + "".join(J.mrf_line(c, "-" if minus else "+", b) for c, minus, b in reads)
        files[stem] = os.path.join(d, stem + ".mrf")
        open(files[stem], "w").write(mrf)
        rows, _ = J.table(interval, mrf)
        samples.append([(K.NAMES.index(r[0]), r[1], r[2], r[4]) for r in rows])
    sam = sam_of(file_reads()[1]).encode()
    files["two_sam"] = os.path.join(d, "two.sam")
    open(files["two_sam"], "wb").write(sam)
    files["two_bam"] = os.path.join(d, "two.bam")
    open(files["two_bam"], "wb").write(bam_writer.sam_to_bam(sam))
    return files, samples


def test_tables_from_the_junctions_device_path(setup, read_files):
    _, interval, _, ix, ctx = setup
    files, samples = read_files
    opts = dict(min_cluster_reads=10)
    want = K.reference(interval, samples, opts)
    assert want.report["clusters"] == 3 and want.report["singletons"] == 0 and want.report["pooled_rows"] == 9
    for second in (("MRF_SINGLE", files["two"]), ("SAM_SINGLE", files["two_sam"]), ("BAM_SINGLE", files["two_bam"])):
        pool = L.ClusterPool(ix)
        pool.add(ix.device(ctx, "MRF_SINGLE", files["one"]))
        pool.add(ix.device(ctx, *second))
        got = pool.device(ctx, **opts)
        K.same(got, want)
        K.same_tables(got, pool.host(**opts))


def test_the_executable_writes_the_files(setup, read_files, tmp_path):
    _, interval, paths, ix, ctx = setup
    files, samples = read_files
    want = K.reference(interval, samples, dict(min_cluster_reads=10))
    head = [os.path.join(BIN, "clusters"), "--min-cluster-reads", "10", "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"]]
    for fmt, second in (("MRF_SINGLE", files["two"]), ("BAM_SINGLE", files["two_bam"])):
        prefix = str(tmp_path / fmt)
        first = files["one"]
        if fmt == "BAM_SINGLE":
            first = str(tmp_path / "one.bam")
            open(first, "wb").write(bam_writer.sam_to_bam(sam_of(file_reads()[0]).encode()))
        p = subprocess.run(head + [fmt, prefix, first, second], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        assert p.returncode == 0 and p.stdout == "", p.stderr
        assert open(prefix + ".clusters.tab").read() == want.text
        assert [open(prefix + ".%d.tab" % k).read() for k in (1, 2)] == want.sample_texts
        assert "clusters: 2 sample(s), 9 pooled row(s), 6 distinct intron(s); " in p.stderr
    p = subprocess.run(head + ["MRF_SINGLE", "-", files["one"], files["two"]], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0 and p.stdout == want.text
