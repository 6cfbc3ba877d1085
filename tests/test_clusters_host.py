"""Intron clusters without a GPU (include/lesseq_hip.h, lsq_cl_*): the definition as tests/clusters_ref.py restates it against
tables worked out by hand, lsq_cl_host against it on every case the GPU tests use, the reader of `junctions` text, and
`clusters --host` with read files and with --tables."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
from lesseq_amd._lib import lib, vp, cs
import junction_ref as J
import clusters_ref as R
import clusters_cases as K
from test_junctions_host import log_messages, BIN

HERE = os.path.dirname(os.path.abspath(__file__))
TOY = os.path.join(HERE, "golden", "toy")
LSQ_E_ARG, LSQ_E_IO, LSQ_E_PARSE, LSQ_E_RANGE = -1, -2, -4, -5
USAGE = ("Usage:\nclusters [--host] [--min-overhang N] [--min-reads N] [--max-intron L] [--min-cluster-reads N] isoform_format isoforms_path g2i_format g2i_path "
         "read_format out_prefix reads_path_1 [reads_path_2 ...]\n"
         "clusters [--host] [--min-reads N] [--max-intron L] [--min-cluster-reads N] --tables isoform_format isoforms_path g2i_format g2i_path "
         "out_prefix junctions_path_1 [junctions_path_2 ...]")
EXAMPLE_1 = ("clu_1\t7\tchr10:101:900\t5\nclu_1\t7\tchr10:301:900\t2\nclu_2\t4\tchr10:201:400\t3\nclu_2\t4\tchr10:201:500\t1\n"
             "clu_3\t20\tchr10:3001:4000\t10\nclu_3\t20\tchr10:3501:4000\t10\n")
TOY_TABLE = "clu_1\t3\tchr1:1101:1200\t1\nclu_1\t3\tchr1:1101:1500\t1\nclu_1\t3\tchr1:1301:1500\t1\n"
CASES = dict(K.small_cases(), **K.large_cases())


@pytest.fixture(scope="module")
def annotation(tmp_path_factory):
    interval, paths = K.write_annotation(str(tmp_path_factory.mktemp("cl")))
    return interval, paths, L.JunctionIndex(L.Annotation(paths["interval"], paths["map"]))


def toy_argv(*opts):
    return [os.path.join(BIN, "clusters"), "--host"] + list(opts) + ["LH_GENE_TXT", os.path.join(TOY, "toy.interval"), "UCSC_GENE2ISOFORM", os.path.join(TOY, "toy.map")]


def run(argv):
    return subprocess.run(argv, capture_output=True, text=True)


# ----------------------------------------------------------------------------- the definition

def test_the_reference_gives_the_worked_example(annotation):
    interval, _, _ = annotation
    samples, opts = K.worked_example()
    want = K.reference(interval, samples, opts)
    assert want.sample_texts[0] == EXAMPLE_1
    assert [ln.split("\t")[1] for ln in want.sample_texts[1].split("\n")[:-1]] == ["2", "2", "5", "5", "20", "20"]
    assert [ln.split("\t")[3] for ln in want.sample_texts[1].split("\n")[:-1]] == ["0", "2", "4", "1", "10", "10"]
    assert [ln.split("\t")[2] for ln in want.sample_texts[1].split("\n")[:-1]] == [ln.split("\t")[2] for ln in want.sample_texts[0].split("\n")[:-1]]
    by = {r[:3]: r for r in want.rows}
    assert by[("chr10", 3000, 200000)][6:] == (0, R.LONG_ROW) and by[("chr10", 1000, 2000)][6:] == (0, R.SINGLETON) and by[("chr2", 100, 900)][6:] == (0, R.SINGLETON)
    assert [r[0] for r in want.rows] == ["chr10"] * 8 + ["chr2"]                        # names, not indices: chr2 is index 0
    assert by[("chr10", 200, 400)][3] == "+" and by[("chr10", 3000, 4000)][3] == "-" and by[("chr2", 100, 900)][3] == "+"
    assert want.text.split("\n")[0] == "clu_1\tchr10\t101\t900\t.\t5\t1"
    assert want.report == dict(zip(R.REPORT, (2, 17, 9, 1, 0, 8, 5, 2, 0, 3, 6)))


def test_the_reference_on_cases_worked_out_by_hand(annotation):
    interval, _, _ = annotation
    cases = K.small_cases()

    def statuses(name):
        return [(r[1], r[2], r[6], r[7]) for r in K.reference(interval, *cases[name]).rows]
    assert statuses("shared_start_only") == [(100, 200, 1, 0), (100, 300, 1, 0), (400, 500, 0, 3)]
    assert statuses("shared_end_only") == [(100, 300, 1, 0), (200, 300, 1, 0), (400, 500, 0, 3)]
    assert statuses("start_equals_end") == [(100, 200, 0, 3), (200, 300, 0, 3)]
    assert [r[0:1] + r[6:] for r in K.reference(interval, *cases["two_chromosomes"]).rows] == [("chr1", 0, 3), ("chr10", 0, 3), ("chr2", 1, 0), ("chr2", 1, 0)]
    assert statuses("bridge_kept") == [(100, 200, 1, 0), (100, 250, 1, 0), (100, 500, 1, 0), (400, 500, 1, 0), (450, 500, 1, 0)]
    assert statuses("bridge_weak") == [(100, 200, 1, 0), (100, 250, 1, 0), (100, 500, 0, 1), (400, 500, 2, 0), (450, 500, 2, 0)]
    assert statuses("three_samples") == [(100, 200, 1, 0), (100, 300, 0, 1), (150, 200, 1, 0)]
    assert statuses("max_intron_zero") == [(50, 1100, 1, 0), (100, 1100, 1, 0), (100, 1101, 1, 0), (100, 500000, 1, 0)]
    assert statuses("length_exactly_l") == [(50, 1100, 0, 2), (100, 1100, 0, 3), (100, 1101, 0, 2), (100, 500000, 0, 2)]
    assert statuses("long_and_weak") == [(50, 1100, 0, 2), (100, 1100, 0, 1), (100, 1101, 0, 2), (100, 500000, 0, 2)]       # both long and weak: long
    assert statuses("cluster_total") == [(100, 200, 1, 0), (100, 300, 1, 0), (1000, 1200, 0, 4), (1100, 1200, 0, 4)]          # 30 printed, 29 not
    dup = K.reference(interval, *cases["duplicate_rows"])
    assert dup.counts == [[8, 0], [4, 4]] and [r[4:6] for r in dup.rows] == [(8, 1), (8, 2)] and dup.report["pooled_rows"] == 6
    assert K.reference(interval, *cases["zero_reads"]).rows[0][4:] == (0, 0, 0, 1)
    empty = K.reference(interval, *cases["empty_pool"])
    assert empty.rows == [] and empty.text == "" and empty.sample_texts == [] and set(empty.report.values()) == {0}
    chain = K.reference(interval, *CASES["staircase"])
    assert chain.report["clusters"] == 1 and chain.report["printed_rows"] == (1 << 15) + 1
    broken = K.reference(interval, *CASES["staircase_broken"])
    assert (broken.report["clusters"], broken.report["long_rows"], broken.report["printed_rows"]) == (2, 1, 1 << 15)
    sizes = {}
    for r in K.reference(interval, *CASES["random"]).rows:
        if r[6]:
            sizes[r[6]] = sizes.get(r[6], 0) + 1
    assert len(set(sizes.values())) >= 8 and max(sizes.values()) >= 20


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_equals_the_reference(annotation, name):
    interval, _, ix = annotation
    samples, opts = CASES[name]
    pool = K.pool_of(ix, samples)
    assert pool.num_samples == len(samples) and pool.num_rows == sum(len(s) for s in samples)
    got = pool.host(**opts)
    K.same(got, K.reference(interval, samples, opts))
    assert got.rounds == 0 and got.times == dict.fromkeys(L.clusters.PHASES, 0.0)
    if name in ("random", "pairs_%d" % (3 * K.SORT_TILE + 1)):
        for n_threads in (1, 3, 16):
            K.same_tables(pool.host(n_threads=n_threads, **opts), got)


def test_the_worked_example_from_the_library(annotation):
    _, _, ix = annotation
    samples, opts = K.worked_example()
    got = K.pool_of(ix, samples).host(**opts)
    assert got.sample_text(0) == EXAMPLE_1 and got.cluster.tolist() == [1, 2, 2, 1, 0, 3, 0, 3, 0] and got.status.tolist() == [0, 0, 0, 0, 3, 0, 2, 0, 3]
    with pytest.raises(L.LsqError) as e:
        got.sample_text(2)
    assert e.value.status == LSQ_E_ARG


def test_a_pool_solved_again_and_samples_in_another_order(annotation):
    interval, _, ix = annotation
    samples, opts = CASES["random"]
    pool = K.pool_of(ix, samples)
    first = pool.host(**opts)
    K.same_tables(pool.host(**opts), first)
    loose = dict(opts, min_reads=1, min_cluster_reads=1)
    K.same(pool.host(**loose), K.reference(interval, samples, loose))
    order = [2, 0, 3, 1]
    other = K.pool_of(ix, [samples[k] for k in order]).host(**opts)
    assert other.text() == first.text() and [other.sample_text(q) for q in range(4)] == [first.sample_text(k) for k in order]


# ----------------------------------------------------------------------------- rows handed in, limits

def test_rows_that_are_refused_leave_the_pool_as_it_was(annotation):
    _, _, ix = annotation
    pool = L.ClusterPool(ix)
    pool.add_rows([K.CHR1], [100], [200], [5])
    for rows, status in ((([3], [100], [200], [1]), LSQ_E_ARG), (([0, 0], [100, 300], [200, 300], [1, 1]), LSQ_E_ARG), (([0], [300], [200], [1]), LSQ_E_ARG),
                         (([0], [-(1 << 30)], [200], [1]), LSQ_E_RANGE), (([0], [100], [1 << 30], [1]), LSQ_E_RANGE),
                         (([0, 0], [100, 100], [200, 300], [0xFFFFFFFF, 1]), LSQ_E_RANGE)):
        with pytest.raises(L.LsqError) as e:
            pool.add_rows(*rows)
        assert e.value.status == status, rows
    assert (pool.num_samples, pool.num_rows) == (1, 1)
    pool.add_rows([0], [-(1 << 30) + 1], [(1 << 30) - 1], [0xFFFFFFFF])
    got = pool.host(max_intron=0)
    assert got.rows()[1] == ("chr2", -(1 << 30) + 1, (1 << 30) - 1, ".", 0xFFFFFFFF, 1, 0, 3)
    with pytest.raises(ValueError):
        pool.add_rows([0], [1, 2], [3], [4])


def test_sums_beyond_32_bits_are_kept(annotation):
    _, _, ix = annotation
    pool = L.ClusterPool(ix)
    for _ in range(3):
        pool.add_rows([K.CHR1, K.CHR1], [100, 100], [200, 300], [0xFFFFFFF0, 5])
    got = pool.host()
    assert got.reads.tolist() == [3 * 0xFFFFFFF0, 15] and got.counts.tolist() == [[0xFFFFFFF0] * 3, [5] * 3]
    assert got.sample_text(1).split("\n")[0] == "clu_1\t%d\tchr1:101:200\t%d" % (0xFFFFFFF5, 0xFFFFFFF0)


# ----------------------------------------------------------------------------- the text reader

@pytest.fixture(scope="module")
def junction_files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cljn"))
    interval, mrf, paths = J.write_case(d, "base", J.annotation_lines(), J.extract_lines())
    ix = L.JunctionIndex(L.Annotation(paths["interval"], paths["map"]))
    jt = ix.host("MRF_SINGLE", paths["mrf"])
    paths["tab"] = os.path.join(d, "base.tab")
    open(paths["tab"], "w").write(jt.text())
    return paths, ix, jt


def test_junctions_text_read_back_equals_the_table(junction_files):
    paths, ix, jt = junction_files
    assert len(jt) > 10 and jt.start.min() < 0
    a, b = L.ClusterPool(ix), L.ClusterPool(ix)
    a.add(jt)
    b.add_text(paths["tab"])
    assert a.num_rows == b.num_rows == len(jt)
    for opts in (dict(), dict(max_intron=0, min_cluster_reads=1)):
        K.same_tables(a.host(**opts), b.host(**opts))
    got = b.host(max_intron=0, min_cluster_reads=1)
    assert [r[:5] for r in got.rows()] == [r[:5] for r in jt.rows()]              # ann from the index, as junctions gives it
    assert got.report["clusters"] >= 1
    other = L.JunctionIndex(L.Annotation(os.path.join(TOY, "toy.interval"), os.path.join(TOY, "toy.map")))
    with pytest.raises(L.LsqError) as e:
        L.ClusterPool(other).add(jt)
    assert e.value.status == LSQ_E_ARG


def test_the_readers_failures_name_file_and_line(junction_files, tmp_path):
    paths, ix, jt = junction_files
    good = "chr1\t201\t300\t+\t7\t4\t2\t50"
    bad_lines = ["chrU\t201\t300\t.\t7\t4\t2\t50", "chr1\t201\t300\t+\t7\t4\t2", "chr1\t201\t300\t+\t7\t4\t2\t50\t1", "chr1\t2x1\t300\t+\t7\t4\t2\t50",
                 "chr1\t201\t300\t+\t-7\t4\t2\t50", "chr1\t201\t300\t?\t7\t4\t2\t50", "chr1\t201\t300\t++\t7\t4\t2\t50", "chr1\t301\t300\t+\t7\t4\t2\t50",
                 "chr1\t201\t300\t+\t4294967296\t4\t2\t50", "chr1\t201\t300\t+\t7\t\t2\t50", ""]
    pool = L.ClusterPool(ix)
    for k, bad in enumerate(bad_lines):
        path = str(tmp_path / ("bad%d.tab" % k))
        open(path, "w").write((good + "\n") * 4 + bad + "\n" + good + "\n")
        with pytest.raises(L.LsqError) as e:
            pool.add_text(path)
        assert e.value.status == LSQ_E_PARSE and str(e.value).endswith("%s: #5:%s" % (path, bad)), bad
    with pytest.raises(L.LsqError) as e:
        pool.add_text(str(tmp_path / "missing.tab"))
    assert e.value.status == LSQ_E_IO
    assert pool.num_samples == 0
    path = str(tmp_path / "ok.tab")
    open(path, "w").write((good + "\n") * 2 + "chr1\t300\t300\t.\t1\t0\t0\t9")       # one base, no newline at the end
    pool.add_text(path)
    open(path, "w").write("")
    pool.add_text(path)
    assert (pool.num_samples, pool.num_rows) == (2, 3) and pool.host(min_cluster_reads=1).counts.tolist() == [[14, 0], [1, 0]]


# ----------------------------------------------------------------------------- the executable

def test_the_tool_on_the_toy_files(tmp_path):
    prefix = str(tmp_path / "toy")
    mrf = os.path.join(TOY, "toy.mrf")
    p = run(toy_argv("--min-cluster-reads", "1") + ["MRF_SINGLE", prefix, mrf])
    assert p.returncode == 0 and p.stdout == ""
    assert open(prefix + ".1.tab").read() == TOY_TABLE
    assert open(prefix + ".clusters.tab").read() == "clu_1\tchr1\t1101\t1200\t+\t1\t1\nclu_1\tchr1\t1101\t1500\t+\t1\t1\nclu_1\tchr1\t1301\t1500\t+\t1\t1\n"
    assert sorted(os.listdir(str(tmp_path))) == ["toy.1.tab", "toy.clusters.tab"]
    line = "clusters: 1 sample(s), 4 pooled row(s), 4 distinct intron(s); 0 long, 0 weak, 4 kept; 2 component(s), 1 singleton(s), 0 weak cluster(s); 1 cluster(s) of 3 row(s) printed"
    assert log_messages(p.stderr) == [("WARNING", line)]
    # the same file three times: three samples with the same rows; "-": the cluster table alone, on standard output
    p = run(toy_argv("--min-cluster-reads", "9") + ["MRF_SINGLE", "-", mrf, mrf, mrf])
    assert p.returncode == 0 and p.stdout == "clu_1\tchr1\t1101\t1200\t+\t3\t3\nclu_1\tchr1\t1101\t1500\t+\t3\t3\nclu_1\tchr1\t1301\t1500\t+\t3\t3\n"
    p = run(toy_argv("--min-cluster-reads", "10") + ["MRF_SINGLE", "-", mrf, mrf, mrf])
    assert p.returncode == 0 and p.stdout == ""
    p = run(toy_argv() + ["MRF_SINGLE", prefix + "_default", mrf])                                  # 3 reads against the default of 30
    assert p.returncode == 0 and open(prefix + "_default.1.tab").read() == "" == open(prefix + "_default.clusters.tab").read()
    rc, text = L.cli_run("clusters", toy_argv("--min-cluster-reads", "1")[1:] + ["MRF_SINGLE", "-", mrf])
    assert rc == 0 and text.count("\n") == 3


def test_tables_gives_what_the_read_files_give(tmp_path):
    mrf = os.path.join(TOY, "toy.mrf")
    tab = str(tmp_path / "toy.junctions.tab")
    argv = [os.path.join(BIN, "junctions"), "--host", "LH_GENE_TXT", os.path.join(TOY, "toy.interval"), "UCSC_GENE2ISOFORM", os.path.join(TOY, "toy.map"), "MRF_SINGLE", mrf, tab]
    assert run(argv).returncode == 0
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert run(toy_argv("--min-cluster-reads", "1") + ["MRF_SINGLE", a, mrf, mrf]).returncode == 0
    assert run(toy_argv("--min-cluster-reads", "1", "--tables") + [b, tab, tab]).returncode == 0
    for name in (".clusters.tab", ".1.tab", ".2.tab"):
        assert open(a + name).read() == open(b + name).read() != ""
    assert open(b + ".2.tab").read() == TOY_TABLE
    p = run(toy_argv("--min-reads", "3", "--max-intron", "399", "--min-cluster-reads", "1", "--tables") + ["-", tab, tab])       # 1101-1500 is 400 long
    assert p.returncode == 0 and p.stdout == "" and "; 1 long, 3 weak, 0 kept; " in p.stderr
    p = run(toy_argv("--min-reads", "2", "--max-intron", "400", "--min-cluster-reads", "7", "--tables") + ["-", tab, tab])
    assert p.returncode == 0 and p.stdout == "" and "; 0 long, 0 weak, 4 kept; 2 component(s), 1 singleton(s), 1 weak cluster(s); " in p.stderr


def test_all_files_or_none(tmp_path):
    mrf = os.path.join(TOY, "toy.mrf")
    bad_line = "chr1:+:15x:200:1:50"
    bad = str(tmp_path / "bad.mrf")
    open(bad, "w").write(open(mrf).read() + bad_line + "\n")
    prefix = str(tmp_path / "out")
    p = run(toy_argv("--min-cluster-reads", "1") + ["MRF_SINGLE", prefix, mrf, bad])
    assert p.returncode == 1 and p.stdout == ""
    errors = [t for lv, t in log_messages(p.stderr) if lv == "ERROR"]
    assert errors[0].startswith(bad + ": ") and errors[0].endswith(bad_line) and "Lexical_cast error" in errors[1]
    assert sorted(os.listdir(str(tmp_path))) == ["bad.mrf"]
    tab = str(tmp_path / "bad.tab")
    open(tab, "w").write("chr1\t1101\t1200\t+\t1\t1\t0\t25\nchr1\t1101\n")
    good = str(tmp_path / "good.tab")
    open(good, "w").write("chr1\t1101\t1200\t+\t1\t1\t0\t25\n")
    p = run(toy_argv("--tables") + [prefix, good, tab])
    assert p.returncode == 1 and p.stdout == "" and (tab + ": #2:chr1\t1101") in p.stderr
    p = run(toy_argv("--tables") + [prefix, good, str(tmp_path / "missing.tab")])
    assert p.returncode == 1 and p.stdout == ""
    assert sorted(os.listdir(str(tmp_path))) == ["bad.mrf", "bad.tab", "good.tab"]
    p = run(toy_argv("--tables") + [str(tmp_path / "no_such_dir" / "out"), good])
    assert p.returncode == 1 and p.stdout == ""


def test_bad_options_give_the_usage_text(tmp_path):
    mrf = os.path.join(TOY, "toy.mrf")
    tail = ["MRF_SINGLE", str(tmp_path / "o"), mrf]
    numbers = [[opt] + v for opt in ("--min-overhang", "--min-reads", "--max-intron", "--min-cluster-reads") for v in ([], ["-1"], ["4294967296"], ["1x"])]
    for bad in [["--nonsense"], ["--table"], ["--min-overhang", "0"], ["--max-intron", "2147483648"]] + numbers:
        p = run(toy_argv(*bad) + tail)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], bad
    for argv in (toy_argv() + tail[:2], toy_argv() + tail[:1], toy_argv("--tables") + tail[1:2], toy_argv("--tables", "--min-overhang", "2") + tail[1:], toy_argv() + tail + ["--min-reads"]):
        p = run(argv)
        assert p.returncode == 1 and p.stdout == "" and log_messages(p.stderr) == [("ERROR", USAGE)], argv
    assert os.listdir(str(tmp_path)) == []


# ----------------------------------------------------------------------------- downstream

def read_tables(test, paths, n1, n2):
    h = vp()
    arr = (cs * len(paths))(*[p.encode() for p in paths])
    L.check(lib.lsq_as_read_tables(test.encode(), len(paths), arr, n1, n2, C.byref(h)))
    try:
        n, cols = lib.lsq_as_input_rows(h), lib.lsq_as_input_columns(h)
        ids = [lib.lsq_as_input_id(h, i).decode() for i in range(n)]
        values = np.ctypeslib.as_array(lib.lsq_as_input_values(h), (n, cols)).copy()
        totals = np.ctypeslib.as_array(lib.lsq_as_input_totals(h), (n, cols)).copy()
    finally:
        lib.lsq_as_input_free(h)
    return ids, values, totals


def test_test_as_reads_the_sample_tables_as_they_are(tmp_path):
    """what `test_as lrt --tables 1 1` and `test_as betabin --tables 2 1` read of the tables `clusters --host` wrote"""
    mrf = os.path.join(TOY, "toy.mrf")
    prefix = str(tmp_path / "s")
    assert run(toy_argv("--min-cluster-reads", "1") + ["MRF_SINGLE", prefix, mrf, mrf, mrf]).returncode == 0
    tables = [prefix + ".%d.tab" % k for k in (1, 2, 3)]
    ids, values, totals = read_tables("lrt", tables[:2], 1, 1)
    assert ids == ["chr1:1101:1200", "chr1:1101:1500", "chr1:1301:1500"] and values.tolist() == [[1, 1]] * 3 and totals.tolist() == [[3, 3]] * 3
    ids, values, totals = read_tables("betabin", tables, 2, 1)
    assert len(ids) == 3 and values.tolist() == [[1, 1, 1]] * 3 and totals.tolist() == [[3, 3, 3]] * 3


def test_new_entry_points_are_exported_and_the_abi_version_stays():
    syms = ("lsq_cl_pool_create", "lsq_cl_pool_free", "lsq_cl_pool_samples", "lsq_cl_pool_rows", "lsq_cl_pool_add_table", "lsq_cl_pool_add_rows", "lsq_cl_pool_add_text",
            "lsq_cl_host", "lsq_cl_device", "lsq_cl_table_free", "lsq_cl_table_rows", "lsq_cl_table_samples", "lsq_cl_table_chrom_name", "lsq_cl_table_rounds",
            "lsq_cl_table_arrays", "lsq_cl_table_counts", "lsq_cl_table_report", "lsq_cl_table_times", "lsq_cl_format", "lsq_cl_format_sample")
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in syms:
        assert hasattr(L.lib, sym), sym
        assert sym + "(" in header, sym
    assert L.lib.lsq_abi_version() == 2 and "#define LSQ_ABI_VERSION 2" in header
    assert os.access(os.path.join(BIN, "clusters"), os.X_OK)
    assert L.clusters.REPORT == R.REPORT and L.ClusterPool is L.clusters.ClusterPool and L.Clusters is L.clusters.Clusters
    rc, _ = L.cli_run("clusters", ["--host"])
    assert rc == 1
