"""BAM_SINGLE on the device: the inflate kernel against zlib, the record-start passes and the BAM routing kernels
(lsq_bam_device.hpp) against the host parser and the device SAM parse of the same lines, and count / solve from BAM files against
the reference's stdout on the equivalent MRF (tests/golden/sam; each in.sam is rewritten as BAM at run time by tests/bam_writer.py).
Need an MI355X: python -m pytest tests -m gpu.  Every case directory is run; none is skipped."""
import os
import subprocess

import pytest

import lesseq_amd as L
import bam_writer as bw
from test_sam_host import BIN, SAM_CASES, load, read, same_reads
from test_sam_gpu import context_for, check_run, option_env, count_table, CHILD_TIMEOUT
from test_bam_host import payload_file, corrupt_case, accepted_incomplete_codes, raw_block

pytestmark = pytest.mark.gpu

DEVICE_LAYOUTS = ("htslib", "cut997", "cut61", "flush")


def write_case(name, layout, tmp_path):
    """the case's in.sam ('\\n'-terminated lines) and its BAM in the layout, in tmp_path"""
    c, d = load(name)
    sam = bw.terminated(read(os.path.join(d, "in.sam")))
    bam_path, sam_path = str(tmp_path / ("in.%s.bam" % layout)), str(tmp_path / "in.lines.sam")
    with open(bam_path, "wb") as f:
        f.write(bw.sam_to_bam(sam, layout))
    with open(sam_path, "wb") as f:
        f.write(sam)
    return c, d, bam_path, sam_path


def test_every_case_directory_is_run():
    assert SAM_CASES == ["basic", "cigar", "filters", "multi", "names"]


@pytest.mark.parametrize("layout", bw.LAYOUTS)
def test_inflate_kernel_equals_zlib(layout):
    """staging and the inflate kernel alone: the payload in every layout, and the hand-written block of distance 32 768"""
    data, want = payload_file(layout)
    ctx = L.Context(0)
    assert ctx.bgzf_inflate(data) == want
    ctx.close()


def test_inflate_kernel_accepts_the_incomplete_codes_zlib_accepts():
    ctx = L.Context(0)
    for name, raw, want in accepted_incomplete_codes():
        assert ctx.bgzf_inflate(raw_block(raw, len(want)) + bw.EOF_BLOCK) == want, name
    ctx.close()


@pytest.mark.parametrize("layout", DEVICE_LAYOUTS)
@pytest.mark.parametrize("name", SAM_CASES)
def test_device_parser_equals_host_parser_and_device_sam(name, layout, tmp_path):
    c, d, bam, sam = write_case(name, layout, tmp_path)
    for cv in c["conversions"]:
        ev, ctx = context_for(d)
        ctx.set_option("sam_skip_flags", cv["skip_flags"])
        ctx.set_option("sam_min_mapq", cv["min_mapq"])
        dev = ctx.parse_bam_device(bam)
        paths = ctx.bam_paths()
        # a layout that cuts the stream regardless of records must take the repair pass; one that respects them must not
        assert paths["blocks"] >= 2 and (paths["blocks_repaired"] > 0) == layout.startswith("cut"), paths
        same_reads(ev, L.Reads.from_bam(bam, ev, cv["skip_flags"], cv["min_mapq"]), dev)
        same_reads(ev, ctx.parse_sam_device(sam), dev)
        same_reads(ev, L.Reads.from_mrf(os.path.join(d, cv["mrf"]), ev), dev)
        ctx.close()


def bam_argv(r, bam):
    assert r["argv"].count("SAM_SINGLE") == 1 and r["argv"].count("in.sam") == 1
    return [bam if a == "in.sam" else "BAM_SINGLE" if a == "SAM_SINGLE" else a for a in r["argv"]]


@pytest.mark.parametrize("layout", ("htslib", "cut61"))
@pytest.mark.parametrize("name", SAM_CASES)
def test_count_and_solve_from_bam_match_the_reference(name, layout, tmp_path, monkeypatch):
    """in-process: count byte for byte, solve within solve_text_close, exit statuses equal, every run of the case -- the read file
    swapped for its BAM (multi: one BAM and one MRF file in one run); the non-default filters through the environment variables"""
    c, d, bam, _ = write_case(name, layout, tmp_path)
    monkeypatch.chdir(d)
    n = 0
    for r in c["runs"]:
        for k in ("LSQ_SAM_SKIP_FLAGS", "LSQ_SAM_MIN_MAPQ"):
            monkeypatch.delenv(k, raising=False)
        for k, v in option_env(r).items():
            monkeypatch.setenv(k, v)
        rc, text = L.cli_run(r["tool"], bam_argv(r, bam))
        check_run(name, r, rc, text, d)
        n += 1
    assert n == len(c["runs"]) and n >= 2


@pytest.mark.parametrize("name", SAM_CASES)
def test_executables_from_bam_match_the_reference(name, tmp_path):
    """once as child processes of the executables (the second thread stages the BAM file beside the annotation load)"""
    c, d, bam, _ = write_case(name, "htslib", tmp_path)
    for r in c["runs"]:
        p = subprocess.run([os.path.join(BIN, r["tool"])] + bam_argv(r, bam), cwd=d, capture_output=True, text=True, env=dict(os.environ, **option_env(r)), timeout=CHILD_TIMEOUT)
        check_run(name, r, p.returncode, p.stdout, d)


@pytest.mark.parametrize("name", ["l_read_name_zero-htslib", "l_read_name_zero-cut61", "record_past_the_end-cut61", "block_type_3", "output_under_isize", "output_over_isize",
                                  "bad_gzip_magic_at_the_start", "bad_bam_magic", "bsize_past_eof"])
def test_error_files_give_the_host_parsers_status_and_message(name, tmp_path):
    """a malformed record, an invalid deflate block, a wrong ISIZE -- each clean in the CPU sanitizer program (test_bam_host) -- and
    the files the host side rejects before any launch: the device chain reports what the host parser reports"""
    _, data, status, msg = corrupt_case(name)
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as f:
        f.write(data)
    _, d = load("basic")
    ev, ctx = context_for(d)
    with pytest.raises(L.LsqError) as host:
        L.Reads.from_bam(path, ev)
    assert host.value.status == status and str(host.value).endswith(": " + msg)
    with pytest.raises(L.LsqError) as e:
        ctx.parse_bam_device(path)
    assert (e.value.status, str(e.value)) == (host.value.status, str(host.value))
    with pytest.raises(L.LsqError) as e:
        ctx.upload_reads_bam(0, path)
    assert (e.value.status, str(e.value)) == (host.value.status, str(host.value))
    ctx.close()


def test_filter_options_through_set_option_give_the_filters_goldens(tmp_path):
    c, d, bam, _ = write_case("filters", "cut997", tmp_path)
    seen = 0
    for r in c["runs"]:
        if r["tool"] != "count":
            continue
        ev, ctx = context_for(d)
        for k, v in r["options"].items():
            ctx.set_option(k, v)
        ctx.upload_reads_bam(0, bam)
        assert count_table(ctx, ev) == open(os.path.join(d, r["stdout"])).read(), r["options"]
        ctx.close()
        seen += 1
    assert seen == 3


def test_ingest_reports_the_bam_passes_by_name(tmp_path):
    """the chain of a BAM file: three passes of its own, then the six every read file shares; an MRF ingest afterwards reports
    its own seven again; pools equal to those of the host parser's arrays"""
    c, d, bam, _ = write_case("basic", "cut61", tmp_path)
    R = int(c["runs"][0]["argv"][11])
    ev, ctx = context_for(d, R)
    ctx.upload_reads(0, L.Reads.from_bam(bam, ev))
    want = (count_table(ctx, ev), ctx.retained(0), ctx.pooled_blocks(0))
    ctx.upload_reads_bam(0, bam)
    st = ctx.ingest_stages()
    assert [s["stage"] for s in st] == ["bgzf_inflate", "bam_record_starts", "bam_route", "partition_count", "partition_scatter", "group_classify", "group_offsets", "group_place"]
    assert all(s["ms"] > 0 for s in st) and st[0]["bytes"] >= os.path.getsize(bam)
    assert ctx.bam_paths()["blocks_repaired"] > 0
    assert (count_table(ctx, ev), ctx.retained(0), ctx.pooled_blocks(0)) == want
    ctx.upload_reads_mrf(0, os.path.join(d, "in.mrf"))
    assert [s["stage"] for s in ctx.ingest_stages()][:2] == ["newline_count", "route"] and len(ctx.ingest_stages()) == 7
    assert (count_table(ctx, ev), ctx.retained(0), ctx.pooled_blocks(0)) == want
    ctx.close()


def test_two_slices_print_the_reference_table(tmp_path):
    """LSQ_SHARD=reads takes MRF_SINGLE files only: a BAM job is sharded by events instead and prints the same table"""
    c, d, bam, _ = write_case("basic", "htslib", tmp_path)
    env = dict(os.environ, LSQ_GPUS="2", LSQ_DEVICES="0,0", LSQ_GATHER="host", LSQ_SHARD="reads")
    r = c["runs"][0]
    p = subprocess.run([os.path.join(BIN, r["tool"])] + bam_argv(r, bam), cwd=d, capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0, p.stderr
    check_run("basic", r, p.returncode, p.stdout, d)
