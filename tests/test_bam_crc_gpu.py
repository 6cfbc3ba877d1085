"""BAM_SINGLE verified on the device: the CRC-32 pass of the chain (lsq_bgzf_crc_kernel, a wave a BGZF block) against zlib.crc32 on
hand-built files -- every ISIZE at which a lane's slice, its head and its tail change shape, blocks at odd offsets of the stream,
more blocks than a workgroup's waves -- the option "bam_verify" through the parser, the ingest and the executables, the damaged
files of tests/test_bam_crc_host.py with the host's status and message, and the whole-file check (lsq_bam_check, bamcheck).
Need an MI355X: python -m pytest tests -m gpu."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import lesseq_amd as L
import bam_writer as bw
from test_sam_host import BIN, load, same_reads
from test_sam_gpu import context_for, count_table, CHILD_TIMEOUT
from test_bam_host import payload_file, blocks_of, good_bam_parts
from test_bam_gpu import write_case, bam_argv
from test_bam_crc_host import CRC_NAMES, crc_case

pytestmark = pytest.mark.gpu

ISIZES = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097, 65535, 65536)
SHARED_STAGES = ["partition_count", "partition_scatter", "group_classify", "group_offsets", "group_place"]


def deflated_block(payload, level):
    """a BGZF block around the raw deflate stream zlib makes of the payload; the stored sum is left 0: the kernel's own is asked for"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    bsize = 18 + len(data) + 8
    assert bsize <= 65536, (len(payload), level)
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + data + struct.pack("<II", 0, len(payload))


def sums_of(ctx, payloads, level):
    got = ctx.bgzf_crc32(b"".join(deflated_block(p, level) for p in payloads) + bw.EOF_BLOCK)
    assert got[-1] == 0 and len(got) == len(payloads) + 1          # (the end-of-file block: no bytes)
    return got[:-1]


@pytest.fixture(scope="module")
def ctx0():
    ctx = L.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("kind", ["zeros", "ones", "random"])
def test_crc_kernel_equals_zlib_at_every_slice_shape(kind, ctx0):
    """the sizes in order and once more in reverse: behind the 1-byte block every block begins at an odd offset of the stream.
    A BGZF block holds at most 65 536 bytes with its 26 of header and trailer, and bytes drawn from all 256 values do not deflate:
    the random payloads of 65 535 and 65 536 bytes are drawn from 0..127 (7 bits a byte under their Huffman code), the shorter
    ones from all values."""
    rng = np.random.default_rng(17)
    sizes = ISIZES + ISIZES[::-1]
    if kind == "random":
        payloads = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) if n < 65000 else bytes(rng.integers(0, 128, n, dtype=np.uint8)) for n in sizes]
    else:
        payloads = [(b"\0" if kind == "zeros" else b"\xff") * n for n in sizes]
    assert [len(p) for p in payloads] == list(sizes)
    want = [zlib.crc32(p) for p in payloads]
    assert sums_of(ctx0, payloads, 6) == want


@pytest.mark.parametrize("layout", bw.LAYOUTS)
def test_crc_kernel_equals_zlib_on_the_payload(layout, ctx0):
    data, _ = payload_file(layout)
    want = [zlib.crc32(zlib.decompress(data[o:o + n], 31)) for o, n in blocks_of(data)]
    assert len(want) >= 4 and ctx0.bgzf_crc32(data) == want


def test_crc_kernel_loops_over_more_blocks_than_a_workgroup_holds(ctx0):
    payloads = [bytes([k & 0xff]) for k in range(300)]
    assert sums_of(ctx0, payloads, 6) == [zlib.crc32(p) for p in payloads]


def test_the_option_takes_zero_and_one(ctx0):
    for v in (0, 1, 0):
        ctx0.set_option("bam_verify", v)
    for v in (2, -1, 0.5):
        with pytest.raises(L.LsqError) as e:
            ctx0.set_option("bam_verify", v)
        assert e.value.status == -1


@pytest.mark.parametrize("layout", ("htslib", "cut61"))
@pytest.mark.parametrize("name", ("basic", "cigar"))
def test_verified_device_parse_and_ingest_equal_the_unverified_ones(name, layout, tmp_path):
    c, d, bam, _ = write_case(name, layout, tmp_path)
    ev, ctx = context_for(d)
    plain = ctx.parse_bam_device(bam)
    ctx.upload_reads_bam(0, bam)
    names = [s["stage"] for s in ctx.ingest_stages()]
    assert names == ["bgzf_inflate", "bam_record_starts", "bam_route"] + SHARED_STAGES
    table = count_table(ctx, ev)
    ctx.set_option("bam_verify", 1)
    assert len(plain) > 50
    same_reads(ev, plain, ctx.parse_bam_device(bam))
    ctx.upload_reads_bam(0, bam)
    st = ctx.ingest_stages()
    assert [s["stage"] for s in st] == ["bgzf_inflate", "bgzf_crc32", "bam_record_starts", "bam_route"] + SHARED_STAGES
    assert all(s["ms"] > 0 for s in st) and st[1]["bytes"] >= ctx.bam_paths()["blocks"]
    assert count_table(ctx, ev) == table
    ctx.set_option("bam_verify", 0)
    ctx.upload_reads_bam(0, bam)
    assert [s["stage"] for s in ctx.ingest_stages()] == names
    ctx.close()


@pytest.mark.parametrize("name", CRC_NAMES)
def test_damaged_files_give_the_host_parsers_status_and_message(name, tmp_path):
    (_, data, accepted, _, _), _ = crc_case(name)
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as f:
        f.write(data)
    d = good_bam_parts()[3]
    ev, ctx = context_for(d)
    with pytest.raises(L.LsqError) as host:
        L.Reads.from_bam(path, ev, verify=True)
    if accepted:        # the option off: the device takes the file as the host parser does
        same_reads(ev, L.Reads.from_bam(path, ev), ctx.parse_bam_device(path))
    ctx.set_option("bam_verify", 1)
    with pytest.raises(L.LsqError) as e:
        ctx.parse_bam_device(path)
    assert (e.value.status, str(e.value)) == (host.value.status, str(host.value))
    with pytest.raises(L.LsqError) as e:
        ctx.upload_reads_bam(0, path)
    assert (e.value.status, str(e.value)) == (host.value.status, str(host.value))
    ctx.close()
    ctx = L.Context(0)          # no events, the option left off: the check always verifies
    with pytest.raises(L.LsqError) as e:
        ctx.bam_check(path)
    assert (e.value.status, str(e.value)) == (host.value.status, str(host.value))
    ctx.close()


@pytest.mark.parametrize("name,layout", [("basic", "htslib"), ("cigar", "cut61"), ("filters", "cut997"), ("names", "flush")])
def test_device_check_equals_the_host_check(name, layout, tmp_path, ctx0):
    _, _, bam, _ = write_case(name, layout, tmp_path)
    want = L.bam_check_host(bam)
    got = ctx0.bam_check(bam)
    assert want["records"] > 50 and want["reads"] > 20 and want["blocks"] >= 2
    assert (got["blocks_repaired"] > 0) == layout.startswith("cut")
    assert {k: v for k, v in got.items() if k != "blocks_repaired"} == {k: v for k, v in want.items() if k != "blocks_repaired"}


def test_device_check_names_the_first_malformed_record(tmp_path, ctx0):
    from test_bam_host import corrupt_case
    _, data, status, msg = corrupt_case("l_read_name_zero-cut61")
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as f:
        f.write(data)
    for check in (ctx0.bam_check, L.bam_check_host):
        with pytest.raises(L.LsqError) as e:
            check(path)
        assert e.value.status == status and str(e.value).endswith(": " + msg)


def test_executables_verify_when_asked(tmp_path):
    """count as a child process with LSQ_BAM_VERIFY=1: the golden table from a good file, exit status 1 and the message from the
    file with a flipped bit -- which the same run without the variable takes; bamcheck on both"""
    c, d, bam, _ = write_case("basic", "htslib", tmp_path)
    r = next(r for r in c["runs"] if r["tool"] == "count" and not r["options"])
    env = dict(os.environ, LSQ_BAM_VERIFY="1")
    p = subprocess.run([os.path.join(BIN, "count")] + bam_argv(r, bam), cwd=d, capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0 and p.stdout == open(os.path.join(d, r["stdout"])).read(), p.stderr
    (_, data, _, _, msg), _ = crc_case("payload_bit")
    bad = str(tmp_path / "bad.bam")
    with open(bad, "wb") as f:
        f.write(data)
    p = subprocess.run([os.path.join(BIN, "count")] + bam_argv(r, bad), cwd=d, capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    assert p.returncode == 1 and p.stdout == "" and msg in p.stderr
    p = subprocess.run([os.path.join(BIN, "count")] + bam_argv(r, bad), cwd=d, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 0 and p.stdout != ""
    p = subprocess.run([os.path.join(BIN, "bamcheck"), bam], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    want = L.bam_check_host(bam)
    assert p.returncode == 0 and [ln.split("\t") for ln in p.stdout.split("\n")[:-1]] == [[k, str(v)] for k, v in want.items()], p.stderr
    p = subprocess.run([os.path.join(BIN, "bamcheck"), bad], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert p.returncode == 1 and p.stdout == "" and msg in p.stderr


def mixed_bam(d, n=300, bad=None, payload=300):
    """(header lines, BGZF bytes) of n records on the basic case's first reference -- reads of one, two and three blocks, unmapped
    and secondary records among them -- in payload blocks of 300 bytes, which cut most records in two; bad: that record's
    l_read_name set to zero"""
    sam = bw.terminated(read_file(os.path.join(d, "in.sam")))
    head_text, refs, _ = bw.parse_sam(sam)
    recs = []
    for k in range(n):
        flag = 4 if k % 7 == 0 else 0x100 if k % 11 == 0 else 16 if k % 2 else 0
        cigar = "30M200N20M" if k % 3 == 0 else "10M50N20M60N20M" if k % 5 == 0 else "50M"
        recs.append("r%d\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t*\t*\n" % (k, flag, refs[0][0], 1000 + 10 * k, cigar))
    head, rs = bw.bam_stream((head_text + "".join(recs)).encode("latin-1"))
    if bad is not None:
        body = bytearray(rs[bad][4:])
        body[8] = 0
        rs[bad] = struct.pack("<I", len(body)) + bytes(body)
    stream = head + b"".join(rs)
    return head_text.count("\n"), bw.bgzf_file([stream[i:i + payload] for i in range(0, len(stream), payload)] or [b""])


def read_file(path):
    with open(path, "rb") as f:
        return f.read()


def test_check_and_parse_are_one_walk(tmp_path, ctx0):
    """lsq_bam_check's record walk is the first pass of lsq_mrf_parse_device: the same counts on a file of filtered records,
    multi-block reads and records that straddle the BGZF blocks; the same first malformed record, by status and message, from
    the check, the parse and the ingest; nothing and no error from a file that is its header alone"""
    _, d = load("basic")
    ev, ctx = context_for(d)
    h, data = mixed_bam(d)
    path = str(tmp_path / "mixed.bam")
    with open(path, "wb") as f:
        f.write(data)
    rep = ctx0.bam_check(path)
    dev = ctx.parse_bam_device(path)
    assert rep["records"] == 300 and rep["blocks_repaired"] > 0 and ctx.bam_paths()["blocks_repaired"] > 0
    assert 150 < rep["reads"] < 300 and rep["read_blocks"] > rep["reads"]
    assert (rep["reads"], rep["read_blocks"]) == (len(dev), dev.num_blocks)
    same_reads(ev, L.Reads.from_bam(path, ev), dev)
    ctx.upload_reads_bam(0, path)
    # one malformed record, late in the file
    _, data = mixed_bam(d, bad=200)
    bad = str(tmp_path / "bad.bam")
    with open(bad, "wb") as f:
        f.write(data)
    seen = []
    for run in (lambda: ctx0.bam_check(bad), lambda: ctx.parse_bam_device(bad), lambda: ctx.upload_reads_bam(0, bad)):
        with pytest.raises(L.LsqError) as e:
            run()
        seen.append((e.value.status, str(e.value)))
    assert seen[0] == seen[1] == seen[2] and seen[0][0] == -4 and ("#%d:<BAM record at byte " % (h + 201)) in seen[0][1], seen
    # the header alone
    _, data = mixed_bam(d, n=0)
    empty = str(tmp_path / "empty.bam")
    with open(empty, "wb") as f:
        f.write(data)
    rep = ctx0.bam_check(empty)
    assert (rep["records"], rep["reads"], rep["read_blocks"]) == (0, 0, 0)
    dev = ctx.parse_bam_device(empty)
    assert (len(dev), dev.num_blocks) == (0, 0)
    ctx.upload_reads_bam(0, empty)
    assert ctx.retained(0) == 0
    ctx.close()
