"""Stranded counting in the read-file tools without a GPU (lsq_xb_index_build_library, lsq_ps_index_build_library,
lsq_fe_index_build_library, `exonbins|psi|evidence --host --library`): the host paths against the split definition as tests/stranded_tools_ref.py restates it from the
tools' own brute-force references.  All values are integers: tables, reports and library reports equal the reference's exactly."""
import os
import subprocess

import pytest

import lesseq_amd as L
import exonbins_ref
import psi_ref
import evidence_ref
import stranded_inputs as S
import stranded_tools_ref as R
import test_exonbins_host as xb_host
import test_psi_host as ps_host
import test_evidence_host as fe_host
from test_junctions_host import log_messages

HERE = os.path.dirname(os.path.abspath(__file__))
LSQ_E_UNSUPPORTED, LSQ_E_STATE = -6, -8
FORMATS = (("MRF_SINGLE", "mrf"), ("SAM_SINGLE", "sam"), ("BAM_SINGLE", "bam"))


class Tool:
    def __init__(self, name, ref, index_class, helpers, grid_env, numpy_table):
        self.name, self.ref, self.index_class, self.helpers, self.grid_env, self.numpy_table = name, ref, index_class, helpers, grid_env, numpy_table

    def index(self, paths, library=None):
        a = L.Annotation(paths["interval"], paths["map"])
        return self.index_class(a) if library is None else self.index_class(a, library)

    def same(self, got, want):
        self.helpers.same(got, want)

    def run(self, paths, reads, fmt="MRF_SINGLE", opts=(), env=None, host=True, timeout=None):
        return self.helpers.tool(paths, reads, fmt, opts, env, host=host, timeout=timeout)

    def log_line(self, lib, rep):
        return "%s: %s library: %d reads of the + strand, %d retained; %d of the - strand, %d retained; %d without a strand" % (
            self.name, lib, rep["plus"], rep["plus_counted"], rep["minus"], rep["minus_counted"], rep["no_strand"])

    def __repr__(self):
        return self.name


TOOLS = [Tool("exonbins", exonbins_ref, L.ExonBinIndex, xb_host, "LSQ_XB_GRID", exonbins_ref.table_of_one_block_reads),
         Tool("psi", psi_ref, L.PsiIndex, ps_host, "LSQ_PS_GRID", psi_ref.fast_table),
         Tool("evidence", evidence_ref, L.EvidenceIndex, fe_host, "LSQ_FE_GRID", evidence_ref.fast_table)]
tools = pytest.mark.parametrize("tool", TOOLS, ids=repr)
libs = pytest.mark.parametrize("lib", S.LIBS)


# ----------------------------------------------------------------------------- the references, by hand

def hand_case():
    """two genes of identical coordinates on opposite strands, a plus gene alone on its chromosome, a read of every kind"""
    ex = [(100, 200), (300, 400)]
    genes = [S.Gene("M", "chrA", "-", [("M.a", ex), ("M.b", ex[:1])]), S.Gene("P", "chrA", "+", [("P.a", ex), ("P.b", ex[:1])]),
             S.Gene("Q", "chrB", "+", [("Q.a", [(100, 200), (250, 300)]), ("Q.b", [(100, 200)])])]
    recs = [S.Rec("chrA", 0, [(110, 150)]),                    # forward: plus
            S.Rec("chrA", 16, [(110, 150)]),                   # forward: minus
            S.Rec("chrA", 0x91, [(310, 350)]),                 # the second mate of a plus fragment
            S.Rec("chrA", 0x81, [(150, 200), (300, 350)]),     # the second mate of a minus fragment, over the intron
            S.Rec("chrB", 16, [(120, 200), (250, 280)]),       # forward: minus, where no minus gene lies
            S.Rec("chrC", 0, [(1, 50)]),                       # a chromosome the annotation lacks
            S.Rec("chrA", 0, [(110, 150)], mrf_strand=".")]    # no transcript strand
    return genes, recs


def hand_case_through_the_host_path(tool, tmp_path):
    """the host path gives what the reference gives on the hand case: the values asserted by hand below are the library's too"""
    genes, recs = hand_case()
    paths = S.write_inputs(str(tmp_path), "hand", genes, recs)
    for lib in S.LIBS:
        want, lib_report = R.expected(tool.ref, genes, recs, lib)
        got = tool.index(paths, lib).host("MRF_SINGLE", paths["mrf"])
        tool.same(got, want)
        assert got.library_report() == lib_report


def test_the_exonbins_reference_on_a_case_worked_out_by_hand(tmp_path):
    genes, recs = hand_case()
    hand_case_through_the_host_path(TOOLS[0], tmp_path)
    (rows, report), lib = R.expected(exonbins_ref, genes, recs, "forward")
    assert rows == [("M", 2, "M:1", 2), ("M", 2, "M:2", 1), ("P", 2, "P:1", 1), ("P", 2, "P:2", 1), ("Q", 0, "Q:1", 0), ("Q", 0, "Q:2", 0)]
    assert report == {"reads": 7, "blocks": 9, "no_chromosome_or_empty": 1, "no_gene": 2, "several_genes": 0, "bin_hits": 5}
    assert lib == {"plus": 3, "minus": 3, "no_strand": 1, "plus_counted": 2, "minus_counted": 2}
    (rows, report), lib = R.expected(exonbins_ref, genes, recs, "reverse")
    assert rows == [("M", 2, "M:1", 1), ("M", 2, "M:2", 1), ("P", 2, "P:1", 2), ("P", 2, "P:2", 1), ("Q", 1, "Q:1", 1), ("Q", 1, "Q:2", 1)]
    assert report == {"reads": 7, "blocks": 9, "no_chromosome_or_empty": 1, "no_gene": 1, "several_genes": 0, "bin_hits": 7}
    assert lib == {"plus": 3, "minus": 3, "no_strand": 1, "plus_counted": 3, "minus_counted": 2}
    # unstranded, the antisense pair shares every read
    rows, report = R.unstranded(exonbins_ref, genes, recs)
    assert rows[:4] == [("M", 5, "M:1", 4), ("M", 5, "M:2", 2), ("P", 5, "P:1", 4), ("P", 5, "P:2", 2)] and report["several_genes"] == 5


def test_the_psi_reference_on_a_case_worked_out_by_hand(tmp_path):
    genes, recs = hand_case()
    hand_case_through_the_host_path(TOOLS[1], tmp_path)
    # one read crosses the intron 200-300 of M.a / P.a (a minus fragment's second mate), one the intron 200-250 of Q.a (a minus record)
    (rows, report, introns), lib = R.expected(psi_ref, genes, recs, "forward")
    assert rows == [("M", 1, "M.a", 1), ("M", 1, "M.b", 0), ("P", 0, "P.a", 0), ("P", 0, "P.b", 0), ("Q", 0, "Q.a", 0), ("Q", 0, "Q.b", 0)]
    assert introns == [1, 0, 1, 0, 1, 0]
    assert report == {"reads": 7, "blocks": 9, "occurrences": 2, "dropped_overhang": 0, "no_chromosome": 0, "informative_occurrences": 1, "counted": 1, "several_events": 0}
    assert lib == {"plus": 3, "minus": 3, "no_strand": 1, "plus_counted": 0, "minus_counted": 1}
    (rows, report, _), lib = R.expected(psi_ref, genes, recs, "reverse")
    assert rows == [("M", 0, "M.a", 0), ("M", 0, "M.b", 0), ("P", 1, "P.a", 1), ("P", 1, "P.b", 0), ("Q", 1, "Q.a", 1), ("Q", 1, "Q.b", 0)]
    assert report["informative_occurrences"] == 2 and report["counted"] == 2 and report["occurrences"] == 2
    assert lib == {"plus": 3, "minus": 3, "no_strand": 1, "plus_counted": 2, "minus_counted": 0}
    rows, report, _ = R.unstranded(psi_ref, genes, recs)
    assert rows[0] == ("M", 1, "M.a", 1) and rows[2] == ("P", 1, "P.a", 1) and report["several_events"] == 1


def test_the_evidence_reference_on_a_case_worked_out_by_hand(tmp_path):
    genes, recs = hand_case()
    hand_case_through_the_host_path(TOOLS[2], tmp_path)
    # M.a / P.a: the intron 200-300 and the body 300-400; Q.a: the intron 200-250 and the body 250-300; the .b forms hold neither.
    # The minus fragment's second mate crosses M.a's intron and its second block lies on P.a's body too: forward it counts once, for M
    (rows, report, introns, body), lib = R.expected(evidence_ref, genes, recs, "forward")
    assert rows == [("M", 1, "M.a", 1), ("M", 1, "M.b", 0), ("P", 1, "P.a", 1), ("P", 1, "P.b", 0), ("Q", 0, "Q.a", 0), ("Q", 0, "Q.b", 0)]
    assert introns == [1, 0, 1, 0, 1, 0] and body == [100, 0, 100, 0, 50, 0]
    assert report == {"reads": 7, "blocks": 9, "occurrences": 2, "dropped_overhang": 0, "no_chromosome": 0, "informative_occurrences": 1, "skipped_blocks": 1, "body_hits": 2,
                      "counted": 2, "several_events": 0, "counted_by_body_alone": 1}
    assert lib == {"plus": 3, "minus": 3, "no_strand": 1, "plus_counted": 1, "minus_counted": 1}
    (rows, report, _, _), lib = R.expected(evidence_ref, genes, recs, "reverse")
    assert rows == [("M", 1, "M.a", 1), ("M", 1, "M.b", 0), ("P", 1, "P.a", 1), ("P", 1, "P.b", 0), ("Q", 1, "Q.a", 1), ("Q", 1, "Q.b", 0)]
    assert (report["informative_occurrences"], report["body_hits"], report["counted"], report["several_events"], report["counted_by_body_alone"]) == (2, 3, 3, 0, 1)
    assert lib == {"plus": 3, "minus": 3, "no_strand": 1, "plus_counted": 2, "minus_counted": 1}
    rows, report, _, _ = R.unstranded(evidence_ref, genes, recs)
    assert rows[0] == ("M", 2, "M.a", 2) and rows[2] == ("P", 2, "P.a", 2) and report["several_events"] == 2 and report["body_hits"] == 5


def test_evidence_counts_a_read_once_for_its_own_strand_and_prints_psi(tmp_path):
    """the hand-worked case through the host path; --psi --read-length on a stranded table"""
    genes, recs = hand_case()
    paths = S.write_inputs(str(tmp_path), "hand", genes, recs)
    tool = TOOLS[2]
    for lib in S.LIBS:
        want, lib_report = R.expected(evidence_ref, genes, recs, lib)
        got = tool.index(paths, lib).host("MRF_SINGLE", paths["mrf"])
        interval, gmap = R.annotation_texts(genes)
        tool.helpers.same(got, want, pos=evidence_ref.positions(interval, gmap, 50), read_length=50)
        assert got.library_report() == lib_report
        p = tool.run(paths, paths["mrf"], opts=["--library", lib, "--psi", "--read-length", "50"])
        assert p.returncode == 0 and p.stdout == got.text(psi=True, read_length=50) and tool.log_line(lib, lib_report) in p.stderr


# ----------------------------------------------------------------------------- the host paths

@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """the small case of the stranded-library tests: its files, with the records only an MRF file can hold in the MRF file alone --
    first, in the middle and last"""
    d = str(tmp_path_factory.mktemp("strtools"))
    genes, recs = S.small_records()
    odd = S.mrf_only_records()
    with_odd = odd[:1] + recs[:150] + odd[1:2] + recs[150:] + odd[2:]
    paths = S.write_inputs(d, "small", genes, recs)
    with open(paths["mrf"], "w") as f:
        f.write(S.input_mrf(with_odd))
    return genes, recs, with_odd, paths


_want = {}


def want_of(tool, genes, recs, lib, key):
    """the reference's (table, library report) of a case, computed once"""
    k = (tool.name, lib, key)
    if k not in _want:
        _want[k] = R.expected(tool.ref, genes, recs, lib) if lib != "unstranded" else (R.unstranded(tool.ref, genes, recs), None)
    return _want[k]


@tools
@libs
def test_host_paths_equal_the_split_definition(small, tool, lib):
    genes, recs, with_odd, paths = small
    ix = tool.index(paths, lib)
    assert ix.library == lib and ix.chrom_names() == ["chrA", "chrB"]
    for fmt, key in FORMATS:
        want, lib_report = want_of(tool, genes, with_odd if key == "mrf" else recs, lib, key == "mrf")
        got = ix.host(fmt, paths[key])
        tool.same(got, want)
        assert got.library_report() == lib_report and lib_report["no_strand"] == (3 if key == "mrf" else 0)
        again = ix.host_reads(ix.parse_host(fmt, paths[key]), n_threads=3)
        tool.same(again, want)
        assert again.library_report() == lib_report


@tools
def test_explicit_unstranded_equals_the_default(small, tool):
    genes, recs, with_odd, paths = small
    default, named = tool.index(paths), tool.index(paths, "unstranded")
    assert default.library == named.library == "unstranded"
    want, _ = want_of(tool, genes, with_odd, "unstranded", True)
    a, b = default.host("MRF_SINGLE", paths["mrf"]), named.host("MRF_SINGLE", paths["mrf"])
    tool.same(a, want)
    assert a.text() == b.text() and a.report == b.report
    for t in (a, b):
        with pytest.raises(L.LsqError) as e:
            t.library_report()
        assert e.value.status == LSQ_E_STATE and "unstranded" in str(e.value)
    with pytest.raises(ValueError):
        tool.index(paths, "sideways")


@tools
def test_the_stranded_tables_are_no_accident(small, tool):
    """the antisense pair g01 / g02 tells the three library types apart, and both strands keep reads"""
    genes, recs, with_odd, paths = small
    tables = {lib: want_of(tool, genes, with_odd, lib, True) for lib in ("unstranded",) + S.LIBS}
    pair = {lib: [r for r in t[0][0] if r[0] in ("g01", "g02")] for lib, t in tables.items()}
    assert len(pair["unstranded"]) >= 4
    assert pair["forward"] != pair["unstranded"] and pair["reverse"] != pair["unstranded"] and pair["forward"] != pair["reverse"]
    assert tables["forward"][0][0] != tables["reverse"][0][0]
    for lib in S.LIBS:
        rep = tables[lib][1]
        assert rep["plus_counted"] > 10 and rep["minus_counted"] > 10 and rep["plus"] > rep["plus_counted"] and rep["minus"] > rep["minus_counted"]
        got = tool.index(paths, lib).host("MRF_SINGLE", paths["mrf"])
        assert [r for r in got.rows() if r[0] in ("g01", "g02")] == pair[lib]


@tools
def test_a_gene_of_two_strands_has_no_place_in_a_stranded_index(tmp_path, tool):
    genes = S.small_genes()
    genes.insert(2, S.Gene("g02x", "chrA", {"g02x.a": "+", "g02x.b": "-"}, [("g02x.a", [(3000, 3100), (3200, 3300)]), ("g02x.b", [(3000, 3100), (3250, 3300)])]))
    genes.append(S.Gene("g09", "chrB", ".", [("g09.a", [(5000, 5100)])]))
    paths = S.write_inputs(str(tmp_path), "mixed", genes, S.small_records()[1][:20])
    for lib in S.LIBS:
        with pytest.raises(L.LsqError) as e:
            tool.index(paths, lib)
        assert e.value.status == LSQ_E_UNSUPPORTED and " g02x " in str(e.value) and "g09" not in str(e.value) and "2 such" in str(e.value)
    ix = tool.index(paths)
    assert len(ix.host("MRF_SINGLE", paths["mrf"]).rows()) > 0
    p = tool.run(paths, paths["mrf"], opts=["--library", "forward"])
    assert p.returncode == 1 and p.stdout == "" and " g02x " in p.stderr
    assert tool.run(paths, paths["mrf"]).returncode == 0


# ----------------------------------------------------------------------------- the executables

@tools
def test_the_executable_takes_the_option_and_the_environment(small, tool):
    genes, recs, with_odd, paths = small
    default = tool.run(paths, paths["mrf"])
    assert default.returncode == 0 and "library" not in default.stderr
    for lib in S.LIBS:
        want, lib_report = want_of(tool, genes, with_odd, lib, True)
        text = tool.ref.text(want[0])
        by_option = tool.run(paths, paths["mrf"], opts=["--library", lib])
        by_env = tool.run(paths, paths["mrf"], env={"LSQ_LIBRARY": lib})
        for p in (by_option, by_env):
            assert p.returncode == 0 and p.stdout == text, p.stderr
            assert log_messages(p.stderr)[-1] == ("INFO", tool.log_line(lib, lib_report))
        assert text != default.stdout
        want, lib_report = want_of(tool, genes, recs, lib, False)
        for fmt, key in FORMATS[1:]:
            p = tool.run(paths, paths[key], fmt, opts=["--library", lib])
            assert p.returncode == 0 and p.stdout == tool.ref.text(want[0]) and tool.log_line(lib, lib_report) in p.stderr
    # unstranded by name, and the option ahead of the environment
    for opts, env in ((["--library", "unstranded"], None), ([], {"LSQ_LIBRARY": "unstranded"}), (["--library", "unstranded"], {"LSQ_LIBRARY": "reverse"})):
        p = tool.run(paths, paths["mrf"], opts=opts, env=env)
        assert p.returncode == 0 and p.stdout == default.stdout and p.stderr.count("\n") == default.stderr.count("\n")
    for opts, env in ((["--library", "sideways"], None), ([], {"LSQ_LIBRARY": "sideways"}), (["--library", "Forward"], None), (["--library"], None)):
        p = tool.run(paths, paths["mrf"], opts=opts, env=env)
        assert p.returncode == 1 and p.stdout == "" and "ERROR" in p.stderr, (opts, env)


def test_new_entry_points_are_exported():
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for prefix in ("lsq_xb", "lsq_ps", "lsq_fe"):
        for sym in (prefix + "_index_build_library", prefix + "_index_library", prefix + "_table_library_report"):
            assert hasattr(L.lib, sym), sym
            assert sym + "(" in header, sym
    assert L.lib.lsq_abi_version() == 2


# ----------------------------------------------------------------------------- libtype

BIN = os.path.join(os.path.dirname(HERE), "lesseq_amd", "bin")


def libtype_index(paths):
    return L.LibTypeIndex(L.Annotation(paths["interval"], paths["map"]))


def libtype_tool(paths, reads, fmt="MRF_SINGLE", env=None, host=True, timeout=None, opts=()):
    argv = [os.path.join(BIN, "libtype")] + (["--host"] if host else []) + list(opts) + ["LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], fmt, reads]
    return subprocess.run(argv, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=timeout)


def libtype_same(got, want):
    assert {k: got.counts[k] for k in R.LIBTYPE_KEYS} == want
    f, lib = R.libtype_verdict(want)
    assert got.forward_fraction == f and got.library == lib and got.text() == R.libtype_text(want)


def sense_case(n_sense, n_antisense, flip=False):
    """a plus and a minus gene apart; reads on either, n_sense on their gene's strand and n_antisense against it (flip: every
    flag's 0x10 the other way), single-end and both mates in turn; a read on no gene and one on a chromosome the annotation lacks"""
    genes = [S.Gene("P", "chrA", "+", [("P.a", [(1000, 1100), (1300, 1400)])]), S.Gene("M", "chrA", "-", [("M.a", [(5000, 5100), (5300, 5400)])])]
    recs = []
    for i in range(n_sense + n_antisense):
        minus_gene = i % 2 == 1
        want_minus = (minus_gene != (i >= n_sense)) != flip      # the strand the fragment's first mate must lie on
        mate = (0, 0x40, 0x80)[i % 3]
        flag = (0x1 | mate if mate else 0) | (16 if want_minus != (mate == 0x80) else 0)
        at = 5000 if minus_gene else 1000
        recs.append(S.Rec("chrA", flag, [(at + 60, at + 100), (at + 300, at + 330)] if i % 4 == 0 else [(at + 10, at + 50)]))
        assert recs[-1].r_minus == want_minus
    recs += [S.Rec("chrA", 0, [(9000, 9040)]), S.Rec("chrC", 16, [(1010, 1050)])]
    return genes, recs


def test_the_libtype_reference_on_the_hand_case_and_the_host_path(tmp_path):
    genes, recs = hand_case()
    want = R.libtype(genes, recs)
    # M and P share every exon: a read on chrA is on both; Q is plus alone; chrC is no chromosome of the annotation; one read has no strand
    assert want == {"reads": 7, "no_strand": 1, "plus_none": 1, "plus_plus": 0, "plus_minus": 0, "plus_both": 2, "minus_none": 0, "minus_plus": 1, "minus_minus": 0,
                    "minus_both": 2, "sense": 0, "antisense": 1, "ambiguous": 4, "no_gene": 1, "unplaced_genes": 0}
    assert R.libtype_verdict(want) == (0.0, "undetermined")
    paths = S.write_inputs(str(tmp_path), "hand", genes, recs)
    ix = libtype_index(paths)
    libtype_same(ix.host("MRF_SINGLE", paths["mrf"]), want)
    assert ix.num_intervals == 6 and ix.unplaced_genes == 0 and ix.chrom_names() == ["chrA", "chrB"]


@pytest.mark.parametrize("flip,verdict,fraction", [(False, "forward", 1.0), (True, "reverse", 0.0)])
def test_libtype_all_reads_sense_and_all_flipped(tmp_path, flip, verdict, fraction):
    genes, recs = sense_case(120, 0, flip)
    want = R.libtype(genes, recs)
    assert (want["sense"], want["antisense"]) == ((0, 120) if flip else (120, 0)) and want["no_gene"] == 2
    paths = S.write_inputs(str(tmp_path), "sense", genes, recs)
    ix = libtype_index(paths)
    for fmt, key in FORMATS:
        got = ix.host(fmt, paths[key])
        libtype_same(got, want)
        assert got.library == verdict and got.forward_fraction == fraction
        libtype_same(ix.host_reads(ix.parse_host(fmt, paths[key]), n_threads=3), want)
    p = libtype_tool(paths, paths["bam"], "BAM_SINGLE")
    assert p.returncode == 0 and p.stdout == R.libtype_text(want) and p.stdout.endswith("forward_fraction\t%.6f\nlibrary\t%s\n" % (fraction, verdict))
    assert log_messages(p.stderr)[-1][0] == "INFO" and log_messages(p.stderr)[-1][1].endswith(": " + verdict)


@pytest.mark.parametrize("n_sense,n_anti,verdict", [(99, 0, "undetermined"), (90, 10, "forward"), (89, 11, "undetermined"), (10, 90, "reverse"), (11, 89, "undetermined"),
                                                   (40, 60, "unstranded"), (60, 40, "unstranded"), (39, 61, "undetermined"), (61, 39, "undetermined"), (0, 0, "undetermined")])
def test_libtype_thresholds_are_inclusive(tmp_path, n_sense, n_anti, verdict):
    genes, recs = sense_case(n_sense, n_anti)
    want = R.libtype(genes, recs)
    assert (want["sense"], want["antisense"]) == (n_sense, n_anti) and R.libtype_verdict(want)[1] == verdict
    paths = S.write_inputs(str(tmp_path), "edge", genes, recs)
    got = libtype_index(paths).host("SAM_SINGLE", paths["sam"])
    libtype_same(got, want)
    assert got.library == verdict and got.forward_fraction == (n_sense / (n_sense + n_anti) if n_sense + n_anti else None)
    p = libtype_tool(paths, paths["sam"], "SAM_SINGLE")
    assert p.returncode == 0 and p.stdout == R.libtype_text(want)      # exit status 0 whatever the verdict
    if not n_sense + n_anti:
        assert "forward_fraction\tNA\n" in p.stdout


def test_libtype_on_the_small_case_genes_without_a_strand_and_the_filters(small, tmp_path):
    genes, recs, with_odd, paths = small
    ix = libtype_index(paths)
    for fmt, key in FORMATS:
        want = R.libtype(genes, with_odd if key == "mrf" else recs)
        libtype_same(ix.host(fmt, paths[key]), want)
        assert want["no_strand"] == (3 if key == "mrf" else 0) and want["sense"] > 50 and want["antisense"] > 50 and want["ambiguous"] > 10
        p = libtype_tool(paths, paths[key], fmt)
        assert p.returncode == 0 and p.stdout == R.libtype_text(want)
    # genes without a strand of their own are left out and counted: no error here
    more = genes + [S.Gene("g02x", "chrA", {"g02x.a": "+", "g02x.b": "-"}, [("g02x.a", [(3000, 3100)]), ("g02x.b", [(3000, 3100)])]), S.Gene("g09", "chrB", ".", [("g09.a", [(5000, 5100)])])]
    paths2 = S.write_inputs(str(tmp_path), "mixed", more, recs)
    want = R.libtype(more, recs)
    assert want["unplaced_genes"] == 2
    libtype_same(libtype_index(paths2).host("SAM_SINGLE", paths2["sam"]), want)
    # LSQ_SAM_SKIP_FLAGS as for count: with 0x10 skipped only plus records are left
    fewer = R.libtype(genes, [r for r in recs if not r.flag & 0x10])
    p = libtype_tool(paths, paths["sam"], "SAM_SINGLE", env={"LSQ_SAM_SKIP_FLAGS": "0x914"})
    assert p.returncode == 0 and p.stdout == R.libtype_text(fewer) and fewer["reads"] < len(recs)
    p = libtype_tool(paths, paths["bam"], "BAM_SINGLE", env={"LSQ_BAM_VERIFY": "1"})
    assert p.returncode == 0 and p.stdout == R.libtype_text(R.libtype(genes, recs))


def test_libtype_a_malformed_record_and_bad_options(small, tmp_path):
    _, _, _, paths = small
    bad = str(tmp_path / "bad.mrf")
    open(bad, "w").write("AlignmentBlocks\nchrA:+:1001:1050:1:50\nchrA:+:15x:200:1:50\n")
    with pytest.raises(L.LsqError) as e:
        libtype_index(paths).host("MRF_SINGLE", bad)
    assert e.value.status == -4 and str(e.value).endswith("#2:chrA:+:15x:200:1:50")
    p = libtype_tool(paths, bad)
    assert p.returncode == 1 and p.stdout == "" and "#2:chrA:+:15x:200:1:50" in p.stderr
    for opts in (["--nonsense"], ["--library", "forward"]):
        p = libtype_tool(paths, paths["mrf"], opts=opts)
        assert p.returncode == 1 and p.stdout == "" and "Usage:\nlibtype [--host]" in p.stderr
    assert L.LibTypeIndex is L.libtype.LibTypeIndex and os.access(os.path.join(BIN, "libtype"), os.X_OK)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lesseq_hip.h")).read()
    for sym in ("lsq_lt_index_build", "lsq_lt_index_free", "lsq_lt_host", "lsq_lt_host_reads", "lsq_lt_device", "lsq_lt_table_free", "lsq_lt_table_counts", "lsq_lt_table_verdict", "lsq_lt_format"):
        assert hasattr(L.lib, sym) and sym + "(" in header, sym


# ----------------------------------------------------------------------------- the toy example of README

def test_the_toy_example_whose_genes_and_reads_are_all_plus():
    """README: --library forward prints the unstranded tables, --library reverse the same rows with every count 0; libtype says forward"""
    for tool in TOOLS:
        paths = tool.helpers.toy_paths()
        plain = tool.run(paths, paths["mrf"])
        forward = tool.run(paths, paths["mrf"], opts=["--library", "forward"])
        reverse = tool.run(paths, paths["mrf"], opts=["--library", "reverse"])
        assert plain.returncode == forward.returncode == reverse.returncode == 0
        assert forward.stdout == plain.stdout == tool.helpers.TOY_TABLE
        rows = [ln.split("\t") for ln in plain.stdout.splitlines()]
        assert reverse.stdout == "".join("%s\t0\t%s\t0\n" % (r[0], r[2]) for r in rows)
        assert "13 reads of the + strand" in forward.stderr and "13 of the - strand, 0 retained" in reverse.stderr
    paths = TOOLS[0].helpers.toy_paths()
    got = libtype_index(paths).host("MRF_SINGLE", paths["mrf"])
    assert got.counts["reads"] == 13 and got.counts["sense"] == 12 and got.counts["antisense"] == 0 and got.counts["plus_none"] == 1
    assert got.forward_fraction == 1.0 and got.library == "undetermined"      # twelve informative reads decide nothing
