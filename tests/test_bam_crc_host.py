"""BAM_SINGLE verified on the host (CPU only): the shared CRC-32 header (lsq_crc32.hpp) against zlib.crc32 as a program of its own
under the address and undefined-behaviour sanitizers (tools/bam_crc_check.cpp); the checked parser and converter
(lsq_bam_parse_checked, lsq_bam_to_mrf_checked, bam2mrf --verify) on good files and on files with a flipped bit, a flipped stored
sum or no end-of-file marker -- each accepted without verification, which is what the feature adds; bamcheck --host.  The
reference for every checksum is zlib, never the code under test.  tests/test_bam_crc_gpu.py runs the same files on the device."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import lesseq_amd as L
import bam_writer as bw
from test_sam_host import BIN, SAM_CASES, load, read, same_reads, events_of
from test_bam_host import ROOT, LSQ_E_FORMAT, FORMAT_TAIL, blocks_of, good_bam_parts, corrupt_case

CRC_LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 65535, 65536)
VERIFY_LAYOUTS = ("htslib", "cut61", "stored", "isize0", "extra")


# ---- the header against zlib -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def crc_program(tmp_path_factory):
    """tools/bam_crc_check.cpp built with the address and undefined-behaviour sanitizers: runs on the CPU, as a program of its own"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("bamcrc") / "bam_crc_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "lesseq_amd", "csrc"),
                    os.path.join(ROOT, "tools", "bam_crc_check.cpp"), "-o", exe], check=True)
    return exe


def crc_contents(n, seed=3):
    return {"zeros": bytes(n), "ones": b"\xff" * n, "random": bytes(np.random.default_rng(seed + n).integers(0, 256, n, dtype=np.uint8))}


def test_combine_and_xpow8_equal_zlib(crc_program, tmp_path):
    """whole, sliced in 64 and joined by crc32_combine, and folded as the kernel folds (mulmod by xpow8 of the bytes behind a slice)"""
    paths, want = [], []
    for n in CRC_LENGTHS:
        for kind, data in crc_contents(n).items():
            p = tmp_path / ("%s.%d" % (kind, n))
            p.write_bytes(data)
            paths.append(str(p))
            want.append("%d %08x %08x %08x" % ((n,) + (zlib.crc32(data),) * 3))
    p = subprocess.run([crc_program] + paths, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    assert p.stdout.split("\n")[:-1] == want


# ---- good files ------------------------------------------------------------------------------------------------------------
def stored_sums(data):
    return [struct.unpack_from("<I", data, o + n - 8)[0] for o, n in blocks_of(data)]


def payload_sums(data):
    return [zlib.crc32(zlib.decompress(data[o:o + n], 31)) for o, n in blocks_of(data)]


@pytest.mark.parametrize("layout", VERIFY_LAYOUTS)
@pytest.mark.parametrize("name", SAM_CASES)
def test_verified_parse_equals_the_unverified_one(name, layout, tmp_path):
    c, d = load(name)
    bam = bw.sam_to_bam(bw.terminated(read(os.path.join(d, "in.sam"))), layout)
    assert stored_sums(bam) == payload_sums(bam) and bam.endswith(bw.EOF_BLOCK)        # (the writer writes true sums)
    path = str(tmp_path / "in.bam")
    with open(path, "wb") as f:
        f.write(bam)
    ev = events_of(d)
    for cv in c["conversions"]:
        assert L.bam_to_mrf(bam, cv["skip_flags"], cv["min_mapq"], verify=True) == L.bam_to_mrf(bam, cv["skip_flags"], cv["min_mapq"])
        plain = L.Reads.from_bam(path, ev, cv["skip_flags"], cv["min_mapq"])
        assert len(plain) > 50
        for n_threads in (0, 1):
            same_reads(ev, plain, L.Reads.from_bam(path, ev, cv["skip_flags"], cv["min_mapq"], n_threads=n_threads, verify=True))


# ---- damaged files ---------------------------------------------------------------------------------------------------------
def crc_message(stored, computed, off):
    return "CRC32 mismatch (stored 0x%08x, computed 0x%08x) in the BGZF block at file offset %d%s" % (stored, computed, off, FORMAT_TAIL)


def plain_read_index(recs, lo, hi):
    """a record of recs[lo:hi] that makes a read under the default filters and whose CIGAR is one long match"""
    for k in range(lo, hi):
        ref, pos, l_name, _, _, n_cigar, flag = struct.unpack_from("<iiBBHHH", recs[k], 4)
        if ref >= 0 and pos > 8 and not flag & 0x904 and n_cigar == 1 and struct.unpack_from("<I", recs[k], 36 + l_name)[0] & 15 == 0:
            return k
    raise AssertionError("no plain read")


def crc_cases():
    """(name, BGZF bytes, accepted without verification, its reads differ from the good file's, message with verification):
    the damage the block chain, the decoder and the record rules all let pass.  The stream of tests/golden/sam/basic in three
    stored blocks, the damage in the second; returned with the undamaged file."""
    head, recs, _, _ = good_bam_parts()
    stream = head + b"".join(recs)
    cuts = [len(head) + sum(len(r) for r in recs[:k]) for k in (30, 60)]        # (blocks begin with a record)
    parts = [stream[:cuts[0]], stream[cuts[0]:cuts[1]], stream[cuts[1]:]]
    blocks = [bw.bgzf_block(p, level=0) for p in parts]
    off = [0, len(blocks[0]), len(blocks[0]) + len(blocks[1])]
    good = b"".join(blocks) + bw.EOF_BLOCK
    sums = [zlib.crc32(p) for p in parts]
    assert stored_sums(good)[:3] == sums
    # a plain read of the second block, the low bits of its pos: still a well-formed record, at another place
    k = plain_read_index(recs, 30, 60)
    at = sum(len(r) for r in recs[30:k]) + 8                   # (block_size, refID, then pos)
    body = blocks[1].index(parts[1][:64])
    assert blocks[1][body:body + len(parts[1])] == parts[1]    # (a stored deflate block: the payload as it is)
    flipped = bytearray(parts[1])
    flipped[at] ^= 2
    payload_bit = bytearray(good)
    payload_bit[off[1] + body + at] ^= 2
    stored_bit = bytearray(good)
    stored_bit[off[2] - 8 + 2] ^= 0x10
    two = bytearray(payload_bit)
    two[len(good) - len(bw.EOF_BLOCK) - 8] ^= 1
    # many blocks, so that the host parser runs several threads: the stored sums of blocks 5 and 6 changed
    many = bytearray(bw.bgzf_bytes(stream, "cut997"))
    chain = blocks_of(bytes(many))
    assert len(chain) >= 17
    for j in (5, 6):
        many[chain[j][0] + chain[j][1] - 8] ^= 0x80
    many_sums = payload_sums(bw.bgzf_bytes(stream, "cut997"))
    # a deflate error behind a block whose sum differs: the deflate error speaks
    _, inflate_bad, _, inflate_msg = corrupt_case("block_type_3")
    inflate_and_crc = bytearray(inflate_bad)
    first_len = blocks_of(inflate_bad)[0][1]
    inflate_and_crc[first_len - 8] ^= 1
    noeof = bw.sam_to_bam(bw.terminated(read(os.path.join(good_bam_parts()[3], "in.sam"))), "noeof")
    return [
        ("payload_bit", bytes(payload_bit), True, True, crc_message(sums[1], zlib.crc32(bytes(flipped)), off[1])),
        ("stored_sum_bit", bytes(stored_bit), True, False, crc_message(sums[1] ^ 0x100000, sums[1], off[1])),
        ("two_bad_blocks", bytes(two), True, True, crc_message(sums[1], zlib.crc32(bytes(flipped)), off[1])),
        ("two_bad_blocks_of_many", bytes(many), True, False, crc_message(many_sums[5] ^ 0x80, many_sums[5], chain[5][0])),
        ("deflate_error_and_bad_sum", bytes(inflate_and_crc), False, False, inflate_msg),
        ("no_eof_marker", noeof, True, False, "no end-of-file marker in the BGZF block at file offset %d%s" % (len(noeof), FORMAT_TAIL)),
        ("cut_at_a_block_boundary", good[:-len(bw.EOF_BLOCK)], True, False, "no end-of-file marker in the BGZF block at file offset %d%s" % (len(good) - len(bw.EOF_BLOCK), FORMAT_TAIL)),
    ], good


CRC_NAMES = ["payload_bit", "stored_sum_bit", "two_bad_blocks", "two_bad_blocks_of_many", "deflate_error_and_bad_sum", "no_eof_marker", "cut_at_a_block_boundary"]
CRC_CASES = None


def crc_case(name):
    global CRC_CASES
    if CRC_CASES is None:
        CRC_CASES = crc_cases()
    return next(c for c in CRC_CASES[0] if c[0] == name), CRC_CASES[1]


def test_the_damaged_set_is_complete():
    crc_case("payload_bit")
    assert [c[0] for c in CRC_CASES[0]] == CRC_NAMES


@pytest.mark.parametrize("name", CRC_NAMES)
def test_damaged_files_pass_unverified_and_are_refused_verified(name, tmp_path):
    (_, data, accepted, changed, msg), good = crc_case(name)
    d = good_bam_parts()[3]
    ev = events_of(d)
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as f:
        f.write(data)
    if accepted:
        # what the feature adds: today these run through, the flipped pos bit into other numbers than the good file's
        text = L.bam_to_mrf(data)
        assert (text != L.bam_to_mrf(good)) == changed
        assert len(L.Reads.from_bam(path, ev)) > 50
        p = subprocess.run([os.path.join(BIN, "bam2mrf"), path], capture_output=True)
        assert p.returncode == 0 and p.stdout == text
    with pytest.raises(L.LsqError) as e:
        L.bam_to_mrf(data, verify=True)
    assert e.value.status == LSQ_E_FORMAT and str(e.value).endswith(": " + msg), str(e.value)
    for n_threads in (1, 0, 4):
        with pytest.raises(L.LsqError) as e:
            L.Reads.from_bam(path, ev, n_threads=n_threads, verify=True)
        assert e.value.status == LSQ_E_FORMAT and str(e.value).endswith(": " + msg), str(e.value)
    with pytest.raises(L.LsqError) as e:
        L.bam_check_host(path)
    assert e.value.status == LSQ_E_FORMAT and str(e.value).endswith(": " + msg), str(e.value)
    p = subprocess.run([os.path.join(BIN, "bam2mrf"), "--verify", path], capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and msg in p.stderr and "Lexical_cast error" not in p.stderr
    p = subprocess.run([os.path.join(BIN, "bamcheck"), "--host", path], capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and msg in p.stderr


# ---- bamcheck --------------------------------------------------------------------------------------------------------------
def report_of(bam):
    """what a check of a good file reports, from the converter's text and the block chain read in Python"""
    lines = L.bam_to_mrf(bam).split(b"\n")[1:-1]
    h = bw_header_lines(bam)
    rec = lines[h:]
    assert lines[:h] == [b"#"] * h
    chain = blocks_of(bam)
    return {"file_bytes": len(bam), "blocks": len(chain), "inflated_bytes": sum(struct.unpack_from("<I", bam, o + n - 4)[0] for o, n in chain), "header_lines": h,
            "references": bw_references(bam), "records": len(rec), "reads": sum(1 for ln in rec if ln != b"#"), "read_blocks": sum(ln.count(b",") + 1 for ln in rec if ln != b"#")}


def inflated(bam):
    return b"".join(zlib.decompress(bam[o:o + n], 31) for o, n in blocks_of(bam))


def bw_header_lines(bam):
    s = inflated(bam)
    text = s[8:8 + struct.unpack_from("<I", s, 4)[0]]
    return text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)


def bw_references(bam):
    s = inflated(bam)
    return struct.unpack_from("<I", s, 8 + struct.unpack_from("<I", s, 4)[0])[0]


@pytest.mark.parametrize("name,layout", [("basic", "htslib"), ("cigar", "cut61"), ("filters", "isize0"), ("names", "stored")])
def test_bamcheck_host_reports_the_file(name, layout, tmp_path):
    _, d = load(name)
    bam = bw.sam_to_bam(bw.terminated(read(os.path.join(d, "in.sam"))), layout)
    path = str(tmp_path / "in.bam")
    with open(path, "wb") as f:
        f.write(bam)
    want = dict(report_of(bam), blocks_repaired=0)
    assert want["records"] > 50 and want["reads"] > 20 and want["read_blocks"] >= want["reads"] and want["blocks"] >= 2
    assert L.bam_check_host(path) == want and L.bam_check_host(path, n_threads=1) == want
    p = subprocess.run([os.path.join(BIN, "bamcheck"), "--host", path], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    assert [ln.split("\t") for ln in p.stdout.split("\n")[:-1]] == [[k, str(want[k])] for k in ("file_bytes", "blocks", "inflated_bytes", "header_lines", "references", "records",
                                                                                                  "reads", "read_blocks", "blocks_repaired")]
    p = subprocess.run([os.path.join(BIN, "bamcheck"), "--host", str(tmp_path / "none.bam")], capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and "cannot open reads file" in p.stderr
    p = subprocess.run([os.path.join(BIN, "bamcheck"), "--host"], capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and "Usage" in p.stderr


def test_new_entry_points_are_exported():
    public = ("lsq_bam_parse_checked", "lsq_bam_to_mrf_checked", "lsq_bam_check", "lsq_bam_check_host")
    for sym in public + ("lsq_debug_bgzf_crc32",):
        assert hasattr(L.lib, sym), sym
    header = open(os.path.join(ROOT, "include", "lesseq_hip.h")).read()
    for sym in public:
        assert sym + "(" in header
    assert "lsq_bam_report;" in header and "bam_verify" in header
    assert "lsq_debug_bgzf_crc32(" in open(os.path.join(ROOT, "include", "lesseq_hip_dev.h")).read()
    assert L.lib.lsq_abi_version() == 2
    with pytest.raises(L.LsqError) as e:
        L.bam_check_host(os.path.join(ROOT, "no", "such.bam"))
    assert e.value.status == -2
