"""Stranded libraries on the device: every routing kernel's stranded form -- MRF fast and byte-walking, SAM tile and
listed-lines, BAM, parsed blocks from the host -- against the oracle on the split inputs (tests/stranded_inputs.py), the library
report against counts made in Python, both sides of the ROUTE_CHROM_LDS limit, shards, the executables under LSQ_LIBRARY, and the
unchanged default.  Need an MI355X: python -m pytest tests -m gpu."""
import os
import random
import subprocess

import numpy as np
import pytest

import lesseq_amd as L
import oracle_binding as ob
import stranded_inputs as si
from bam_writer import bam_stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lesseq_amd", "bin")
R = 50
TEXT_TILE = 7680          # bytes of text a workgroup of the tile kernels takes (lsq_text.hpp)
CHILD_TIMEOUT = 300


def events(paths, library):
    return L.Events(L.Annotation(paths["interval"], paths["map"], 0, 10 ** 9), ("SHORT_READ",), (R,), library=library)


def count_table(ctx, ev):
    ctx.count()
    return L.format_count(ev, ctx.counts()[0])


def run_job(paths, library, how, expect_table, expect_report):
    """one read file through `how` into a fresh context of a stranded job: its count table and its library report"""
    ev = events(paths, library)
    ctx = L.Context(0)
    try:
        ctx.upload_events(ev)
        if how == "mrf":
            ctx.upload_reads_mrf(0, paths["mrf"])
        elif how == "sam":
            ctx.upload_reads_sam(0, paths["sam"])
        elif how == "bam":
            ctx.upload_reads_bam(0, paths["bam"])
        elif how == "host_mrf":
            ctx.upload_reads(0, L.Reads.from_mrf(paths["mrf"], ev))
        elif how == "host_sam":
            ctx.upload_reads(0, L.Reads.from_sam(paths["sam"], ev))
        elif how == "host_bam":
            ctx.upload_reads(0, L.Reads.from_bam(paths["bam"], ev))
        else:
            raise AssertionError(how)
        report = ctx.library_report(0)
        retained = ctx.retained(0)
        table = count_table(ctx, ev)
        extra = {"sam_paths": ctx.sam_paths(), "host_genes": L.lib.lsq_events_host_genes(ev.h)}
    finally:
        ctx.close()
    assert report == tuple(expect_report), (library, how, report, expect_report)
    assert retained == expect_report[3] + expect_report[4]
    assert table == expect_table, (library, how)
    return extra


# ---- the small case ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("stranded_small"))
    genes, recs = si.small_records()
    mrf_recs = recs + si.mrf_only_records()       # (at the end: every other record keeps the line number it has in the SAM file)
    paths = si.write_inputs(d, "small", genes, mrf_recs)
    case = {"d": d, "genes": genes, "recs": recs, "mrf_recs": mrf_recs, "paths": paths}
    case["unstranded"], un_retained, _ = si.unstranded(d, "small", genes, recs)
    for lib in si.LIBS:
        table, retained = si.expected(d, "small", genes, recs, lib)
        table_mrf, retained_mrf = si.expected(d, "small_m", genes, mrf_recs, lib)
        assert table_mrf == table and retained_mrf == retained        # records without a strand make no read
        case[lib] = {"table": table, "report": si.report_of(recs, lib, retained), "report_mrf": si.report_of(mrf_recs, lib, retained)}
        # the case cannot pass vacuously: a gene of each strand whose row differs from the unstranded job's ...
        differing = {a.split("\t")[0] for a, b in zip(case["unstranded"].splitlines(), table.splitlines()) if a != b}
        strand_of = {g.name: g.strand for g in genes}
        assert {strand_of[g] for g in differing} == {"+", "-"}, differing
        # ... and the read inside the union of the abutting exons only is retained unstranded and dropped stranded
        blank = [si.Rec("chrC", 0, [(1, 2)]) if r is si.UNION_ONLY else r for r in recs]
        _, retained_blank = si.expected(d, "small_b", genes, blank, lib)
        _, un_blank, _ = si.unstranded(d, "small_b", genes, blank)
        assert un_retained - un_blank == 1 and retained_blank == retained
        assert case[lib]["report_mrf"][2] == 3 and case[lib]["report"][2] == 0
    assert sum(len(r.blocks) == 4 for r in recs) >= 5 and sum(len(r.blocks) == 2 for r in recs) >= 20
    assert {r.flag for r in recs} >= set(si.FLAGS)
    return case


@pytest.mark.parametrize("how", ["mrf", "mrf_slow", "sam", "sam_slow", "bam", "host_mrf", "host_sam", "host_bam"])
@pytest.mark.parametrize("library", si.LIBS)
def test_small_case_equals_the_oracle_on_the_split_inputs(small, library, how, monkeypatch):
    exp = small[library]
    if how.endswith("_slow"):
        monkeypatch.setenv("LSQ_MRF_SLOW" if how == "mrf_slow" else "LSQ_SAM_SLOW", "1")       # the byte-walking kernels over the whole file
    base = how.replace("_slow", "")
    extra = run_job(small["paths"], library, base, exp["table"], exp["report_mrf"] if base.endswith("mrf") else exp["report"])
    assert extra["host_genes"] == 1          # the gene of 7 isoforms: a bucket the host evaluates sees stranded reads
    if how == "sam_slow":
        assert extra["sam_paths"]["whole_file_byte_walking"]


@pytest.mark.parametrize("tool", ["count", "solve"])
@pytest.mark.parametrize("library", si.LIBS)
def test_small_case_through_the_executables_with_LSQ_LIBRARY(small, library, tool):
    exp_table, _ = si.expected(small["d"], "small_x", small["genes"], small["recs"], library, tool=tool)
    for fmt in ("SAM_SINGLE", "MRF_SINGLE"):
        argv = si.argv_of(small["paths"], fmt, R, solve=tool == "solve")
        p = subprocess.run([os.path.join(BIN, tool)] + ["2"] + argv[1:], capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=dict(os.environ, LSQ_LIBRARY=library))
        assert p.returncode == 0, p.stderr
        if tool == "count":
            assert p.stdout == exp_table, (library, fmt)
        else:
            assert ob.solve_text_close(p.stdout, exp_table), (library, fmt, p.stdout, exp_table)
        rep = small[library]["report" if fmt == "SAM_SINGLE" else "report_mrf"]
        assert "%s library: %d reads of the + strand, %d retained; %d of the - strand, %d retained; %d without a strand" % (library, rep[0], rep[3], rep[1], rep[4], rep[2]) in p.stderr


def test_small_case_in_process_and_under_two_gpus(small, monkeypatch):
    """lsq_cli_run reads LSQ_LIBRARY too; and so does the job over several slices (LSQ_GPUS=2 on one device, blocks through the host)"""
    argv = si.argv_of(small["paths"], "BAM_SINGLE", R)
    monkeypatch.setenv("LSQ_LIBRARY", "reverse")
    rc, text = L.cli_run("count", argv)
    assert rc == 0 and text == small["reverse"]["table"]
    monkeypatch.setenv("LSQ_GPUS", "2")
    monkeypatch.setenv("LSQ_DEVICES", "0,0")
    monkeypatch.setenv("LSQ_GATHER", "host")
    rc, text = L.cli_run("count", si.argv_of(small["paths"], "MRF_SINGLE", R))
    assert rc == 0 and text == small["reverse"]["table"]


@pytest.mark.parametrize("library", ["forward", "unstranded"])
def test_LSQ_SHARD_reads_falls_back_to_event_shards_in_a_stranded_job(library, tmp_path):
    """an annotation without a gene the host evaluates (such a gene forces event shards by itself) and MRF_SINGLE reads: unstranded, the
    two slices share the reads; stranded, the job says that it is sharded by events instead, and prints the stranded table"""
    d = str(tmp_path)
    genes, recs = si.small_records()
    keep = [g for g in genes if len(g.isoforms) <= 5]
    assert len(keep) == len(genes) - 1
    paths = si.write_inputs(d, "f", keep, recs)
    if library == "unstranded":
        table, _, _ = si.unstranded(d, "f", keep, recs)
    else:
        table, _ = si.expected(d, "f", keep, recs, library)
    env = dict(os.environ, LSQ_GPUS="2", LSQ_DEVICES="0,0", LSQ_GATHER="host", LSQ_SHARD="reads", LSQ_LIBRARY=library)
    p = subprocess.run([os.path.join(BIN, "count")] + ["2"] + si.argv_of(paths, "MRF_SINGLE", R)[1:], capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
    assert p.returncode == 0, p.stderr
    assert p.stdout == table
    said = "LSQ_SHARD=reads: a stranded job (LSQ_LIBRARY=forward) is sharded by events instead" in p.stderr
    shared_reads = "(over 2 GPUs)" in p.stderr              # the read-sharded job's closing line
    assert (said, shared_reads) == ((True, False) if library == "forward" else (False, True)), p.stderr


def test_unstranded_default_is_unchanged(small, monkeypatch):
    """LSQ_LIBRARY=unstranded, and the explicit unstranded compile, print byte for byte what the plain run prints"""
    paths = small["paths"]
    argv = si.argv_of(paths, "SAM_SINGLE", R)
    monkeypatch.delenv("LSQ_LIBRARY", raising=False)
    rc, plain = L.cli_run("count", argv)
    assert rc == 0 and plain == small["unstranded"]
    monkeypatch.setenv("LSQ_LIBRARY", "unstranded")
    rc, text = L.cli_run("count", argv)
    assert rc == 0 and text == plain
    rc, solve_text = L.cli_run("solve", argv + ["1000000"])
    monkeypatch.delenv("LSQ_LIBRARY")
    rc2, solve_plain = L.cli_run("solve", argv + ["1000000"])
    assert rc == rc2 == 0 and solve_text == solve_plain
    tables = []
    for ev in (L.Events(L.Annotation(paths["interval"], paths["map"], 0, 10 ** 9), ("SHORT_READ",), (R,)), events(paths, "unstranded")):
        ctx = L.Context(0)
        ctx.upload_events(ev)
        ctx.upload_reads_sam(0, paths["sam"])
        with pytest.raises(L.LsqError):
            ctx.library_report(0)          # no report without a library
        tables.append(count_table(ctx, ev))
        ctx.close()
    assert tables[0] == tables[1] == plain


def test_two_event_shards_of_a_stranded_job_give_the_one_shard_counts(small):
    paths = small["paths"]
    ev = events(paths, "forward")
    ctx = L.Context(0)
    ctx.upload_events(ev)
    ctx.upload_reads_bam(0, paths["bam"])
    ctx.count()
    full = ctx.counts()[0].copy()
    assert L.format_count(ev, full) == small["forward"]["table"]
    total = np.zeros_like(full)
    for first, count in ev.shard_bounds(2):
        assert count > 0
        ev.set_shard(first, count)
        ctx.upload_events(ev)
        ctx.upload_reads_bam(0, paths["bam"])
        assert ctx.library_report(0) == tuple(small["forward"]["report"])       # the load-time filter is that of the whole job
        ctx.count()
        total += ctx.counts()[0]
    ctx.close()
    assert np.array_equal(total, full)
    assert L.format_count(ev, total) == small["forward"]["table"]


def test_name_keyed_reads_of_a_stranded_solve(tmp_path, monkeypatch):
    """UCSC_BED through `solve`: the host parser filters and groups by name, lsq_reads_upload routes the parsed blocks; a name whose lines
    lie on both strands is a read per strand.  Expected: the oracle's solve on the split annotation and the split BED lines"""
    from test_stranded_host import bed_lines
    d = str(tmp_path)
    genes, recs = si.small_records()
    recs = [r for r in recs if len(r.blocks) <= 2] + si.mrf_only_records()
    lines = bed_lines(recs).splitlines()
    both = [k for k, r in enumerate(recs) if r.chrom == "chrA" and len(r.blocks) == 1 and 1100 <= r.blocks[0][0] and r.blocks[0][1] <= 1200]
    assert len({recs[k].r_minus for k in both}) == 2
    for k in both:                                           # one name for the reads in the stretch both g01 (+) and g02 (-) cover
        f = lines[k + 1].split("\t")
        f[3] = "shared"
        lines[k + 1] = "\t".join(f)
    iv, mp = si.write_annotation(d, "all", genes)
    path = os.path.join(d, "all.bed")
    with open(path, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    for lib in si.LIBS:
        tables = []
        for minus, strand in enumerate("+-"):
            siv, smp = si.write_annotation(d, "sub%d" % minus, [g for g in genes if g.strand == strand])
            spath = os.path.join(d, "sub%d.bed" % minus)
            with open(spath, "w") as f:
                f.write("".join(ln + "\n" for k, ln in enumerate(lines) if k == 0 or recs[k - 1].t(lib) == minus))
            rc, text, _ = ob.run("solve", ["0", "x", "./", "LH_GENE_TXT", siv, "UCSC_GENE2ISOFORM", smp, "0", "1000000", "UCSC_BED", "SHORT_READ", str(R), spath, "1000000"])
            assert rc == 0
            tables.append(text)
        monkeypatch.setenv("LSQ_LIBRARY", lib)
        rc, text = L.cli_run("solve", ["0", "x", "./", "LH_GENE_TXT", iv, "UCSC_GENE2ISOFORM", mp, "0", "1000000", "UCSC_BED", "SHORT_READ", str(R), path, "1000000"])
        assert rc == 0
        assert ob.solve_text_close(text, si.merge_tables(tables)), (lib, text, si.merge_tables(tables))


# ---- tile and block boundaries -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boundaries(tmp_path_factory):
    """some 3 000 records: about 25 tiles of SAM text, a BAM of BGZF blocks of 997 bytes (records straddle them); a few heads longer than
    the tile kernel's window go to the listed-lines kernel"""
    d = str(tmp_path_factory.mktemp("stranded_bounds"))
    genes, recs = si.small_records(seed=5, n=3000)
    header = si.SAM_HEADER
    lines = [r.sam_line(k).replace("q%d\t" % k, "read_with_a_name_of_some_length_%06d\t" % k, 1) for k, r in enumerate(recs)]
    for k in range(7, len(lines), 500):
        lines[k] = "L" * 300 + lines[k]                      # a head of more than 256 bytes
    text = ("".join(h + "\n" for h in header) + "".join(ln + "\n" for ln in lines)).encode()
    iv, mp = si.write_annotation(d, "b", genes)
    paths = {"interval": iv, "map": mp, "sam": os.path.join(d, "b.sam"), "bam": os.path.join(d, "b.bam"), "mrf": os.path.join(d, "b.mrf")}
    with open(paths["sam"], "wb") as f:
        f.write(text)
    with open(paths["bam"], "wb") as f:
        f.write(si.sam_to_bam(text, "cut997"))
    with open(paths["mrf"], "w") as f:
        f.write(si.input_mrf(recs, len(header)))
    # mate-2 and minus-strand records sit on tile boundaries
    pos, crossing = sum(len(h) + 1 for h in header), []
    for r, ln in zip(recs, lines):
        if pos // TEXT_TILE != (pos + len(ln)) // TEXT_TILE:
            crossing.append(r.flag)
        pos += len(ln) + 1
    assert 20 <= len(text) // TEXT_TILE <= 40
    assert any(f & 0x80 for f in crossing) and any(f & 0x10 for f in crossing), crossing
    # ... and on the boundaries of the BAM's BGZF blocks: the inflated stream is cut every 997 bytes, records or not
    head, records = bam_stream(text)
    pos, straddling = len(head), []
    for r, raw in zip(recs, records):
        if pos // 997 != (pos + len(raw) - 1) // 997:
            straddling.append(r.flag)
        pos += len(raw)
    assert sum(1 for f in straddling if f & 0x80) >= 10 and sum(1 for f in straddling if f & 0x10) >= 10, len(straddling)
    case = {"paths": paths}
    for lib in si.LIBS:
        table, retained = si.expected(d, "b", genes, recs, lib)
        case[lib] = {"table": table, "report": si.report_of(recs, lib, retained)}
    return case


@pytest.mark.parametrize("how", ["sam", "bam", "mrf"])
@pytest.mark.parametrize("library", si.LIBS)
def test_records_across_tile_and_block_boundaries(boundaries, library, how):
    extra = run_job(boundaries["paths"], library, how, boundaries[library]["table"], boundaries[library]["report"])
    if how == "sam":
        # both SAM kernels ran: the tile kernel, and the listed-lines kernel for the long heads
        assert extra["sam_paths"]["lines_to_fall_back_kernel"] >= 6 and not extra["sam_paths"]["whole_file_byte_walking"]


# ---- more (chromosome, strand) records than the routing kernels stage in LDS -------------------------------------------------
def many_chromosomes(n_chrom):
    """40 genes, one each on alternating strands; gene i on chromosome i % n_chrom, at coordinates of its own"""
    rng = random.Random(3)
    genes, recs = [], []
    for i in range(40):
        chrom, base = "c%02d" % (i % n_chrom), 10000 * (i + 1)
        ex = [(base, base + 200), (base + 400, base + 600), (base + 800, base + 1000)]
        genes.append(si.Gene("g%02d" % i, chrom, "+-"[i % 2], [("g%02d.a" % i, ex), ("g%02d.b" % i, [ex[0], ex[2]])]))
        for _ in range(12):
            recs.append(si.Rec(chrom, rng.choice(si.FLAGS), si.reads_along(rng, rng.choice(genes[-1].isoforms)[1], rng.choice([1, 2]))))
    header = ["@HD\tVN:1.6"] + ["@SQ\tSN:c%02d\tLN:1000000" % c for c in range(n_chrom)]
    return genes, recs, header


@pytest.mark.parametrize("library,how", [("forward", "mrf"), ("forward", "sam"), ("forward", "bam"), ("forward", "host_sam"), ("reverse", "sam"), ("reverse", "mrf")])
def test_forty_chromosomes_exceed_the_records_staged_in_lds(library, how, tmp_path):
    """80 (chromosome, strand) records: read from global memory; the same genes on 3 chromosomes (6 records, staged in LDS) print the same table"""
    tables = []
    for n_chrom in (40, 3):
        genes, recs, header = many_chromosomes(n_chrom)
        d = str(tmp_path / ("n%d" % n_chrom))
        os.makedirs(d)
        paths = si.write_inputs(d, "m", genes, recs, header=header)
        table, retained = si.expected(d, "m", genes, recs, library, n_comment=len(header))
        assert len(table.splitlines()) == 80 and min(retained) > 50
        run_job(paths, library, how, table, si.report_of(recs, library, retained))
        tables.append(table)
    assert tables[0] == tables[1]
