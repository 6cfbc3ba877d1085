"""Stranded libraries on the host: the transcript-strand rule through the converters, the stranded compile
(covered regions per strand, genes that cannot be placed), the host parsers under stranded events, the new entry points.
No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
import stranded_inputs as si
from bam_writer import sam_to_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lesseq_amd", "bin")
LSQ_E_UNSUPPORTED = -6
LSQ_E_STATE = -8


def events(iv, mp, library="unstranded", R=50):
    return L.Events(L.Annotation(iv, mp, 0, 10 ** 9), ("SHORT_READ",), (R,), library=library)


# ---- the rule, as a truth table through the converters ---------------------------------------------------------------
ALL_FLAGS = [a | b | c | d for a in (0, 0x10) for b in (0, 0x1) for c in (0, 0x40) for d in (0, 0x80)]


def strand_columns(mrf_text):
    return [ln.split(":")[1] for ln in mrf_text.splitlines()[1:] if not ln.startswith("#")]


@pytest.mark.parametrize("tool", ["sam2mrf", "bam2mrf"])
def test_transcript_strand_truth_table_through_the_converters(tool, tmp_path):
    assert len(ALL_FLAGS) == 16
    recs = [si.Rec("chrA", fl, [(100 + 10 * k, 140 + 10 * k)]) for k, fl in enumerate(ALL_FLAGS)]
    text = si.sam_text(recs).encode()
    path = str(tmp_path / ("in.sam" if tool == "sam2mrf" else "in.bam"))
    with open(path, "wb") as f:
        f.write(text if tool == "sam2mrf" else sam_to_bam(text))
    plain = subprocess.run([os.path.join(BIN, tool), path], capture_output=True, text=True, timeout=60)
    assert plain.returncode == 0
    assert strand_columns(plain.stdout) == ["-" if fl & 0x10 else "+" for fl in ALL_FLAGS]      # without the option: the alignment strand, as before
    for lib in si.LIBS:
        p = subprocess.run([os.path.join(BIN, tool), "--library", lib, path], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        want = []
        for fl in ALL_FLAGS:
            s, mate2 = bool(fl & 0x10), bool(fl & 0x1) and bool(fl & 0x80)
            want.append("-" if (s ^ (lib == "reverse") ^ mate2) else "+")
        assert strand_columns(p.stdout) == want, lib
        assert [si.transcript_minus(lib, fl & 0x10, fl) for fl in ALL_FLAGS] == [int(w == "-") for w in want]
        # everything but the strand column is the plain conversion
        assert [ln.split(":")[2:] for ln in p.stdout.splitlines()] == [ln.split(":")[2:] for ln in plain.stdout.splitlines()]
    bad = subprocess.run([os.path.join(BIN, tool), "--library", "sideways", path], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 1 and bad.stdout == ""


# ---- the stranded compile ---------------------------------------------------------------------------------------------
def test_covered_regions_per_strand_equal_the_split_compiles(tmp_path):
    genes = si.small_genes()
    iv, mp = si.write_annotation(str(tmp_path), "all", genes)
    un = events(iv, mp)
    assert un.library == "unstranded"
    # the abutting exons are one covered region of the chromosome ...
    assert any(s <= 5080 and 5120 <= e for s, e in un.covered("chrA"))
    for lib in si.LIBS:
        ev = events(iv, mp, lib)
        assert ev.library == lib and len(ev) == len(un)
        for minus, strand in enumerate("+-"):
            sub = [g for g in genes if g.strand == strand]
            siv, smp = si.write_annotation(str(tmp_path), "sub" + str(minus), sub)
            split = events(siv, smp)
            for chrom in ("chrA", "chrB"):
                assert ev.covered(chrom, minus) == split.covered(chrom), (lib, strand, chrom)
            # ... and of neither strand
            assert not any(s <= 5080 and 5120 <= e for s, e in ev.covered("chrA", minus))
        assert ev.covered("chrB", 1) == [] and ev.covered("chrC", 0) == []
        # events of opposite strands share no bucket: at least a bucket per (chromosome, strand) that has genes
        assert ev.num_buckets >= 3


@pytest.mark.parametrize("kind", ["mixed", "dot"])
def test_a_gene_without_a_strand_of_its_own_is_unsupported_in_a_stranded_compile(kind, tmp_path):
    genes = si.small_genes()
    if kind == "mixed":
        bad = si.Gene("g035", "chrA", {"g035.a": "+", "g035.b": "-"}, [("g035.a", [(30000, 30100)]), ("g035.b", [(30000, 30100), (30200, 30300)])])
    else:
        bad = si.Gene("g035", "chrA", ".", [("g035.a", [(30000, 30100)]), ("g035.b", [(30000, 30100), (30200, 30300)])])
    also = si.Gene("g09", "chrB", "?", [("g09.a", [(40000, 40100)])])
    iv, mp = si.write_annotation(str(tmp_path), kind, genes + [bad, also])
    for lib in si.LIBS:
        with pytest.raises(L.LsqError) as e:
            events(iv, mp, lib)
        assert e.value.status == LSQ_E_UNSUPPORTED
        assert "g035" in str(e.value) and "2 such gene" in str(e.value) and "g09" not in str(e.value)      # the first, and how many
    un = events(iv, mp)
    assert len(un) == len(genes) + 2 and un.library == "unstranded"
    assert len(events(iv, mp, "unstranded")) == len(genes) + 2


def test_unknown_library_name_is_refused(tmp_path):
    iv, mp = si.write_annotation(str(tmp_path), "a", si.small_genes())
    with pytest.raises(ValueError):
        events(iv, mp, "sideways")
    assert [L.lib.lsq_library_from_name(n) for n in (b"unstranded", b"forward", b"reverse", b"Forward", b"")] == [0, 1, 2, -1, -1]


# ---- the host parsers under stranded events ------------------------------------------------------------------------------
def strand_strings(ev, ids):
    return [L.lib.lsq_events_strand_name(ev.h, int(i)).decode() for i in ids]


def test_sam_and_bam_host_parsers_carry_the_first_mates_strand_under_stranded_events(tmp_path):
    """MRF knows no mates: under stranded events the SAM and BAM parsers write the strand of the fragment's first mate, so that
    their arrays are those of the MRF file `sam2mrf --library forward` writes -- and lsq_reads_upload derives t from them"""
    genes, recs = si.small_records(n=120)
    paths = si.write_inputs(str(tmp_path), "p", genes, recs)
    un = events(paths["interval"], paths["map"])
    plain = L.Reads.from_sam(paths["sam"], un)
    assert strand_strings(un, plain.arrays()[5]) == ["-" if r.flag & 0x10 else "+" for r in recs for _ in r.blocks]      # unstranded events: as before
    for lib in si.LIBS:
        ev = events(paths["interval"], paths["map"], lib)
        from_mrf = L.Reads.from_mrf(paths["mrf"], ev)
        for other in (L.Reads.from_sam(paths["sam"], ev), L.Reads.from_bam(paths["bam"], ev)):
            x, y = from_mrf.arrays(), other.arrays()
            assert len(from_mrf) == len(other) == len(recs)
            for k in range(5):
                assert np.array_equal(x[k], y[k]), k
            assert strand_strings(ev, x[5]) == strand_strings(ev, y[5]) == ["-" if r.r_minus else "+" for r in recs for _ in r.blocks]


def bed_lines(recs):
    out = ["track name=reads"]
    for k, r in enumerate(recs):
        s, e = r.blocks[0][0], r.blocks[-1][1]
        st = r.mrf_strand if r.mrf_strand is not None else "-" if r.r_minus else "+"
        out.append("%s\t%d\t%d\tr%04d\t0\t%s\t%d\t%d\t0\t%d\t%s\t%s" % (r.chrom, s, e, k, st, s, e, len(r.blocks), "".join("%d," % (b - a) for a, b in r.blocks),
                                                                    "".join("%d," % (a - s) for a, _ in r.blocks)))
    return "".join(ln + "\n" for ln in out)


def test_name_keyed_host_parser_filters_by_transcript_strand(tmp_path):
    """UCSC_BED lines are accepted or dropped by their whole span on the host: under stranded events against the covered regions
    of the line's transcript strand -- the lines the two split parses accept, and no line without a strand"""
    genes, recs = si.small_records(n=150)
    recs = [r for r in recs if len(r.blocks) == 1] + si.mrf_only_records()
    d = str(tmp_path)
    iv, mp = si.write_annotation(d, "all", genes)
    path = os.path.join(d, "all.bed")
    with open(path, "w") as f:
        f.write(bed_lines(recs))
    un = L.Reads.from_mrf(path, events(iv, mp), read_format="UCSC_BED")
    for lib in si.LIBS:
        ev = events(iv, mp, lib)
        got = L.Reads.from_mrf(path, ev, read_format="UCSC_BED")
        want = []
        for minus, strand in enumerate("+-"):
            siv, smp = si.write_annotation(d, "sub%d" % minus, [g for g in genes if g.strand == strand])
            sub = [r for r in recs if r.t(lib) == minus]
            spath = os.path.join(d, "sub%d.bed" % minus)
            with open(spath, "w") as f:
                f.write(bed_lines(sub))
            a = L.Reads.from_mrf(spath, events(siv, smp), read_format="UCSC_BED").arrays()
            want += sorted(zip(a[2].tolist(), a[3].tolist()))
        a = got.arrays()
        assert sorted(zip(a[2].tolist(), a[3].tolist())) == sorted(want), lib
        assert 0 < len(got) < len(un)
        assert (5080, 5120) in zip(un.arrays()[2].tolist(), un.arrays()[3].tolist()) and (5080, 5120) not in zip(a[2].tolist(), a[3].tolist())


def test_a_name_on_both_strands_is_a_read_per_strand_under_stranded_events(tmp_path):
    """the name-keyed formats merge the lines of a name into one read; lsq_reads_upload routes a read by one strand, so in a stranded
    job such a name is two reads, as it is in the two split jobs"""
    genes = si.small_genes()
    d = str(tmp_path)
    iv, mp = si.write_annotation(d, "all", genes)
    # (inside [1100, 1200): covered by the plus gene g01 and by the minus gene g02, so every line passes either strand's filter)
    recs = [si.Rec("chrA", 0, [(1110, 1150)]), si.Rec("chrA", 16, [(1130, 1170)]), si.Rec("chrA", 0, [(1120, 1160)])]
    text = bed_lines(recs).replace("r0001", "r0000").replace("r0002", "r0000")        # one name: two lines on +, one on -
    path = os.path.join(d, "one.bed")
    with open(path, "w") as f:
        f.write(text)
    un = L.Reads.from_mrf(path, events(iv, mp), read_format="UCSC_BED")
    assert len(un) == 1 and un.num_blocks == 3
    for lib in si.LIBS:
        ev = events(iv, mp, lib)
        got = L.Reads.from_mrf(path, ev, read_format="UCSC_BED")
        a = got.arrays()
        assert len(got) == 2 and got.num_blocks == 3
        per_read = [sorted(zip(a[2][a[0][r]:a[0][r + 1]].tolist(), strand_strings(ev, a[5][a[0][r]:a[0][r + 1]]))) for r in range(2)]
        assert sorted(per_read) == sorted([[(1110, "+"), (1120, "+")], [(1130, "-")]])


def test_the_read_sharded_driver_refuses_a_stranded_job(monkeypatch):
    """dist.run_read_sharded: as for read files that are not MRF_SINGLE, before anything is opened (main falls back to event shards)"""
    import lesseq_amd.dist as ld
    argv = ["0", "x", "./", "LH_GENE_TXT", "none.interval", "UCSC_GENE2ISOFORM", "none.map", "0", "10", "MRF_SINGLE", "SHORT_READ", "50", "none.mrf"]
    monkeypatch.setenv("LSQ_LIBRARY", "reverse")
    with pytest.raises(ValueError, match="unstranded jobs only"):
        ld.run_read_sharded("count", argv, 0, 1)


# ---- the surface ---------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_and_the_abi_version_stays():
    for name in ("lsq_events_compile_library", "lsq_events_library", "lsq_library_from_name", "lsq_last_library_report"):
        assert hasattr(L.lib, name), name
    assert L.lib.lsq_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "lesseq_hip.h")).read()
    for name in ("lsq_events_compile_library", "lsq_events_library", "lsq_last_library_report", "LSQ_LIBRARY_FORWARD", "LSQ_LIBRARY_REVERSE"):
        assert name in header
    assert "#define LSQ_ABI_VERSION 2" in header


@pytest.mark.parametrize("tool", ["count", "solve"])
def test_an_unknown_LSQ_LIBRARY_is_a_usage_error(tool, tmp_path):
    """decided before anything is opened: exit status 1, nothing on standard output"""
    argv = ["0", "x", "./", "LH_GENE_TXT", "none.interval", "UCSC_GENE2ISOFORM", "none.map", "0", "10", "MRF_SINGLE", "SHORT_READ", "50", "none.mrf"]
    p = subprocess.run([os.path.join(BIN, tool)] + argv + (["1000"] if tool == "solve" else []), capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, LSQ_LIBRARY="sideways"), cwd=str(tmp_path))
    assert p.returncode == 1 and p.stdout == "" and "LSQ_LIBRARY" in p.stderr
