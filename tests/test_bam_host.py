"""BAM_SINGLE on the host (CPU only): the shared DEFLATE decoder against zlib, the converter (lsq_bam_to_mrf, bam2mrf) and the host
parser (lsq_bam_parse) against their SAM counterparts on the fixtures of tests/golden/sam -- each in.sam rewritten as BAM at run
time (tests/bam_writer.py) in every BGZF layout, so the reference pins BAM through SAM -- every corrupt input's status and message,
and the shared headers as a program of their own under the address and undefined-behaviour sanitizers (tools/bam_decode_check.cpp)."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import lesseq_amd as L
import bam_writer as bw
from test_sam_host import GOLD, BIN, SAM_CASES, load, read, same_reads, events_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LSQ_E_FORMAT, LSQ_E_PARSE = -3, -4
FORMAT_TAIL = ": Unknown file format error: BAM_SINGLE"


# ---- streams ---------------------------------------------------------------------------------------------------------------
class Bits:
    """a DEFLATE bit stream written by hand: fields least significant bit first, Huffman codes most significant bit first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        self.put(int(format(v, "0%db" % n)[::-1], 2), n)

    def fixed_symbol(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xc0 + s - 280, 8)

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc & 0xff]) if self.n else b"")


def long_distance_stream():
    """one fixed-code block zlib itself never writes: 32 768 literals, then a match of length 258 at distance 32 768 (zlib stops at
    32 506) and one at distance 1.  Returns (deflate bytes, the bytes they mean)."""
    rng = np.random.default_rng(5)
    lit = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    b = Bits()
    b.put(1, 1)
    b.put(1, 2)
    for v in lit:
        b.fixed_symbol(v)
    b.fixed_symbol(285)          # length 258
    b.code(29, 5)                # distance 24 577 + 13 extra bits
    b.put(32768 - 24577, 13)
    b.fixed_symbol(285)
    b.code(0, 5)                 # distance 1
    b.fixed_symbol(256)
    raw = b.bytes()
    want = zlib.decompressobj(-15).decompress(raw)
    assert len(want) == 32768 + 516 and want[32768:32768 + 258] == lit[:258] and want[-258:] == want[-259:-258] * 258
    return raw, want


def raw_block(deflate, isize, crc=0):
    """a BGZF block around deflate bytes given as they are"""
    bsize = 18 + len(deflate) + 8
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + deflate + struct.pack("<II", crc, isize)


def payload():
    """~200 KB that zlib's compressor turns into every kind of code: bytes of geometric frequencies (code lengths up to the
    longest), text-like repeats at every distance, runs (distance 1, length 258), incompressible bytes"""
    rng = np.random.default_rng(11)
    geo = bytes(np.minimum(rng.geometric(0.08, 70000) - 1, 255).astype(np.uint8))
    words = [bytes(rng.integers(97, 123, int(n), dtype=np.uint8)) for n in rng.integers(3, 40, 400)]
    text = b" ".join(words[int(i)] for i in rng.integers(0, 400, 4000))
    runs = b"".join(bytes([int(v)]) * int(n) for v, n in zip(rng.integers(0, 256, 40), rng.integers(1, 3000, 40)))
    noise = bytes(rng.integers(0, 256, 20000, dtype=np.uint8))
    far = noise[:300]            # the same bytes again about 32 500 bytes later: a match near the window's edge
    p = geo + text + runs + noise + bytes(12200) + far + geo[:5000]
    assert 190000 < len(p) < 260000
    return p


PAYLOAD = payload()


def payload_file(layout):
    """(BGZF bytes, the stream they inflate to): the payload in the layout's blocks, then the hand-written block"""
    raw, want = long_distance_stream()
    body = bw.bgzf_file(bw.split_stream(PAYLOAD, layout), layout)
    eof = b"" if layout == "noeof" else bw.EOF_BLOCK
    if eof:
        body = body[:-len(eof)]
    return body + raw_block(raw, len(want), zlib.crc32(want)) + eof, PAYLOAD + want


def as_bam_header_text(stream):
    """a BAM whose header text is `stream` (NULs and all): the decoder's bytes decide l_text, n_ref and where the records begin"""
    return b"BAM\x01" + struct.pack("<I", len(stream)) + stream + struct.pack("<I", 0)


# ---- the decoder against zlib ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def check_program(tmp_path_factory):
    """tools/bam_decode_check.cpp built with the address and undefined-behaviour sanitizers: runs on the CPU, as a program of its own"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("bamcheck") / "bam_decode_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", os.path.join(ROOT, "lesseq_amd", "csrc"),
                    os.path.join(ROOT, "tools", "bam_decode_check.cpp"), "-o", exe], check=True)
    return exe


def run_check(exe, args):
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (args, p.returncode, p.stdout, p.stderr[-2000:])
    return p.stdout.rstrip("\n")


def test_payload_reaches_the_decoders_corners():
    """what zlib makes of the payload: dynamic blocks with 15-bit codes, length 258, distance 1, distances near the window"""
    d = zlib.compressobj(9, zlib.DEFLATED, -15)
    assert len(d.compress(PAYLOAD) + d.flush()) < 0.8 * len(PAYLOAD)
    assert any(bytes([v]) * 258 in PAYLOAD for v in range(256))
    raw, want = long_distance_stream()
    assert zlib.decompressobj(-15).decompress(raw) == want


@pytest.mark.parametrize("layout", bw.LAYOUTS)
def test_decoder_equals_zlib_on_the_payload(layout, tmp_path, check_program):
    """the shared decoder's host build: byte for byte in the sanitizer program; through lsq_bam_to_mrf as the header text of a BAM"""
    data, want = payload_file(layout)
    ref = b"".join(zlib.decompress(data[o:o + n], 31) for o, n in blocks_of(data))
    assert ref == want
    (tmp_path / "p.bgzf").write_bytes(data)
    (tmp_path / "p.raw").write_bytes(want)
    assert run_check(check_program, ["inflate", str(tmp_path / "p.bgzf"), str(tmp_path / "p.raw")]) == "ok %d" % len(want)
    stream = as_bam_header_text(want)
    text = want[:want.index(b"\0")] if b"\0" in want else want
    h = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    for lay in (layout, "cut997"):
        assert L.bam_to_mrf(bw.bgzf_bytes(stream, lay)) == b"AlignmentBlocks\n" + b"#\n" * h


@pytest.mark.parametrize("name", ["single_one_bit_distance_code", "distance_code_without_lengths"])
def test_incomplete_codes_that_zlib_accepts_are_accepted(name, tmp_path, check_program):
    """a single one-bit distance code, and a distance code without lengths in a block of literals"""
    _, raw, want = next(c for c in accepted_incomplete_codes() if c[0] == name)
    (tmp_path / "p.bgzf").write_bytes(raw_block(raw, len(want), zlib.crc32(want)) + bw.EOF_BLOCK)
    (tmp_path / "p.raw").write_bytes(want)
    assert run_check(check_program, ["inflate", str(tmp_path / "p.bgzf"), str(tmp_path / "p.raw")]) == "ok %d" % len(want)
    # ... and through the library, as a block behind a BAM header: the block inflates (no format error), and its few bytes are
    # then a record that runs past the end of the stream
    stream = as_bam_header_text(b"@CO\tx\n")
    with pytest.raises(L.LsqError) as e:
        L.bam_to_mrf(bw.bgzf_block(stream) + raw_block(raw, len(want)) + bw.EOF_BLOCK)
    assert e.value.status == LSQ_E_PARSE and str(e.value).endswith(": #2:<BAM record at byte %d of the inflated stream>" % len(stream))


def blocks_of(data):
    out, o = [], 0
    while o < len(data):
        n = struct.unpack_from("<H", data, o + 16)[0] + 1 if data[o + 12:o + 14] == b"BC" else None
        if n is None:           # an extra subfield ahead of BC
            xlen = struct.unpack_from("<H", data, o + 10)[0]
            x = o + 12
            while data[x:x + 2] != b"BC":
                x += 4 + struct.unpack_from("<H", data, x + 2)[0]
            assert x < o + 12 + xlen
            n = struct.unpack_from("<H", data, x + 4)[0] + 1
        out.append((o, n))
        o += n
    return out


# ---- the five cases in every layout ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", bw.LAYOUTS)
@pytest.mark.parametrize("name", SAM_CASES)
def test_bam_means_its_sam_equivalent(name, layout, tmp_path):
    """bam_to_mrf equals sam_to_mrf of the same lines byte for byte; Reads.from_bam equals Reads.from_sam -- with the filters
    case's non-default options; bam2mrf from a file and from standard input"""
    c, d = load(name)
    sam = bw.terminated(read(os.path.join(d, "in.sam")))
    bam = bw.sam_to_bam(sam, layout)
    path, sam_path = str(tmp_path / "in.bam"), str(tmp_path / "in.sam")
    with open(path, "wb") as f:
        f.write(bam)
    with open(sam_path, "wb") as f:
        f.write(sam)
    for cv in c["conversions"]:
        want = L.sam_to_mrf(sam, cv["skip_flags"], cv["min_mapq"])
        assert want == read(os.path.join(d, cv["mrf"]))
        assert L.bam_to_mrf(bam, cv["skip_flags"], cv["min_mapq"]) == want, cv
        ev = events_of(d)
        a = L.Reads.from_bam(path, ev, cv["skip_flags"], cv["min_mapq"])
        assert len(a) > 50
        same_reads(ev, L.Reads.from_sam(sam_path, ev, cv["skip_flags"], cv["min_mapq"]), a)
        same_reads(ev, a, L.Reads.from_bam(path, ev, cv["skip_flags"], cv["min_mapq"], n_threads=1))
    if layout in ("htslib", "cut61"):
        cv = c["conversions"][-1]
        opts = ["--skip-flags", str(cv["skip_flags"]), "--min-mapq", str(cv["min_mapq"])]
        want = read(os.path.join(d, cv["mrf"]))
        p = subprocess.run([os.path.join(BIN, "bam2mrf")] + opts + [path], capture_output=True)
        assert p.returncode == 0 and p.stdout == want, p.stderr
        p = subprocess.run([os.path.join(BIN, "bam2mrf")] + opts, input=bam, capture_output=True)
        assert p.returncode == 0 and p.stdout == want, p.stderr
    ev = events_of(d)
    same_reads(ev, L.Reads.from_mrf(path, ev, read_format="BAM_SINGLE"), L.Reads.from_mrf(os.path.join(d, "in.mrf"), ev))


def test_layouts_are_what_they_claim():
    c, d = load("basic")
    sam = bw.terminated(read(os.path.join(d, "in.sam")))
    head, recs = bw.bam_stream(sam)
    stream = head + b"".join(recs)
    sizes = {}
    for layout in bw.LAYOUTS:
        data = bw.sam_to_bam(sam, layout)
        blocks = blocks_of(data)
        assert b"".join(zlib.decompress(data[o:o + n], 31) for o, n in blocks) == stream, layout
        assert data.endswith(bw.EOF_BLOCK) == (layout != "noeof")
        sizes[layout] = [struct.unpack_from("<I", data, o + n - 4)[0] for o, n in blocks]
    assert min(len(r) for r in recs) > 2 * 61 and set(sizes["cut61"][:-2]) == {61} and set(sizes["cut997"][:-2]) == {997}
    assert 0 in sizes["isize0"][1:-1] and 0 not in sizes["htslib"][:-1]
    # htslib: every block begins with a record (or the header)
    starts, at = {len(head)}, len(head)
    for r in recs:
        at += len(r)
        starts.add(at)
    off = 0
    for n in sizes["htslib"]:
        assert off == 0 or off in starts
        off += n


# ---- corrupt inputs --------------------------------------------------------------------------------------------------------
def good_bam_parts():
    c, d = load("basic")
    sam = bw.terminated(read(os.path.join(d, "in.sam")))
    head, recs = bw.bam_stream(sam)
    text, _, _ = bw.parse_sam(sam)
    return head, recs, text.count("\n"), d


def dynamic_block(lit, dist, n_lit, n_dist, body, pad=8):
    """a dynamic block written by hand: code lengths lit / dist ({symbol: length}) over n_lit / n_dist codes, every length sent
    as itself through a code length code of sixteen 4-bit codes; body(bits, lit_code, dist_code) writes the symbols"""
    b = Bits()
    b.put(1, 1); b.put(2, 2); b.put(n_lit - 257, 5); b.put(n_dist - 1, 5); b.put(19 - 4, 4)
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        b.put(4 if sym < 16 else 0, 3)
    for s in range(n_lit):
        b.code(lit.get(s, 0), 4)
    for s in range(n_dist):
        b.code(dist.get(s, 0), 4)

    def canonical(lengths):
        codes, code = {}, 0
        for ln in range(1, 16):
            for s in sorted(k for k, v in lengths.items() if v == ln):
                codes[s] = (code, ln)
                code += 1
            code <<= 1
        return codes
    if body:
        body(b, canonical(lit), canonical(dist))
    return b.bytes() + bytes(pad)


def accepted_incomplete_codes():
    """(name, deflate bytes, what they mean): the two incomplete codes zlib lets pass, and the decoder with it"""
    def one_distance(b, lc, dc):          # a, then length 3 at the only distance code there is, end
        b.code(*lc[97]); b.code(*lc[257]); b.code(*dc[0]); b.code(*lc[256])

    def literals_only(b, lc, dc):
        b.code(*lc[97]); b.code(*lc[97]); b.code(*lc[256])
    out = [("single_one_bit_distance_code", dynamic_block({97: 1, 256: 2, 257: 2}, {0: 1}, 258, 1, one_distance, pad=0), b"aaaa"),
           ("distance_code_without_lengths", dynamic_block({97: 1, 256: 1}, {}, 257, 1, literals_only, pad=0), b"aa")]
    for name, raw, want in out:
        assert zlib.decompressobj(-15).decompress(raw) == want, name
    return out


def zlib_rejects(deflate):
    d = zlib.decompressobj(-15)
    try:
        d.decompress(deflate)
    except zlib.error:
        return True
    return not d.eof


def deflate_cases():
    """(name, BGZF bytes, message) of every way a block's bytes can be wrong; the bad block is the second of three"""
    head, recs, _, _ = good_bam_parts()
    stream = head + b"".join(recs)
    a, b, c = stream[:5000], stream[5000:9000], stream[9000:]
    first, last = bw.bgzf_block(a), bw.bgzf_block(c) + bw.EOF_BLOCK
    off = len(first)
    good = bw.bgzf_block(b)
    cdata = good[18:-8]

    def with_isize(n):
        return good[:-4] + struct.pack("<I", n)

    dyn = Bits()                 # a dynamic block whose code length code is over-subscribed: four codes of one bit
    dyn.put(1, 1); dyn.put(2, 2); dyn.put(0, 5); dyn.put(0, 5); dyn.put(0, 4)
    for _ in range(4):
        dyn.put(1, 3)
    inc = Bits()                 # ... and incomplete: a single code of two bits
    inc.put(1, 1); inc.put(2, 2); inc.put(0, 5); inc.put(0, 5); inc.put(0, 4)
    inc.put(2, 3)
    for _ in range(3):
        inc.put(0, 3)
    early = Bits()               # a fixed block that begins with a match: nothing to copy from
    early.put(1, 1); early.put(1, 2); early.fixed_symbol(257); early.code(0, 5); early.fixed_symbol(256)
    def use_empty_distance_code(bits, lc, dc):
        bits.code(*lc[97]); bits.code(*lc[257])

    cases = [
        ("over_subscribed_literal_code", raw_block(dynamic_block({0: 1, 1: 1, 256: 1}, {0: 1, 1: 1}, 257, 2, None), len(b)), "an over-subscribed code"),
        ("incomplete_literal_code", raw_block(dynamic_block({0: 2, 256: 2}, {0: 1, 1: 1}, 257, 2, None), len(b)), "an incomplete code"),
        ("over_subscribed_distance_code", raw_block(dynamic_block({0: 1, 256: 1}, {0: 1, 1: 1, 2: 1}, 257, 3, None), len(b)), "an over-subscribed code"),
        ("incomplete_distance_code", raw_block(dynamic_block({0: 1, 256: 1}, {0: 2, 1: 2}, 257, 2, None), len(b)), "an incomplete code"),
        ("match_through_an_empty_distance_code", raw_block(dynamic_block({97: 1, 256: 2, 257: 2}, {}, 258, 1, use_empty_distance_code), len(b)), "an invalid symbol"),
        ("truncated_stream", raw_block(cdata[:len(cdata) // 2], len(b)), "the deflate stream is cut short"),
        ("block_type_3", raw_block(b"\x07\x00", len(b)), "deflate block type 3"),
        ("len_nlen_mismatch", raw_block(b"\x01\x05\x00\x05\x00hello", len(b)), "a stored block's LEN and NLEN do not match"),
        ("over_subscribed_code", raw_block(dyn.bytes() + bytes(8), len(b)), "an over-subscribed code"),
        ("incomplete_code", raw_block(inc.bytes() + bytes(8), len(b)), "an incomplete code"),
        ("distance_before_the_start", raw_block(early.bytes(), len(b)), "a distance before the start of the output"),
        ("output_over_isize", with_isize(len(b) - 1), "more bytes than ISIZE"),
        ("output_under_isize", with_isize(len(b) + 1), "fewer bytes than ISIZE"),
    ]
    for name, blk, _ in cases[:11]:
        assert zlib_rejects(blk[18:-8]), name
    return [(name, first + blk + last, "invalid deflate stream (%s) in the BGZF block at file offset %d%s" % (what, off, FORMAT_TAIL)) for name, blk, what in cases]


def file_cases():
    head, recs, _, _ = good_bam_parts()
    stream = head + b"".join(recs)
    first, second = bw.bgzf_block(stream[:5000]), bw.bgzf_block(stream[5000:])
    good = first + second + bw.EOF_BLOCK
    off = len(first)
    no_bc = second[:12] + b"XY" + second[14:]
    return [
        ("bsize_past_eof", good[:off + len(second) - 9], "BSIZE past the end of the file in the BGZF block at file offset %d%s" % (off, FORMAT_TAIL)),
        ("missing_bc", first + no_bc + bw.EOF_BLOCK, "no BC subfield in the BGZF block at file offset %d%s" % (off, FORMAT_TAIL)),
        ("bad_gzip_magic", first + b"\x1f\x8c" + second[2:], "bad gzip magic in the BGZF block at file offset %d%s" % (off, FORMAT_TAIL)),
        ("bad_gzip_magic_at_the_start", b"@HD\tVN:1.6\n" * 4, "bad gzip magic in the BGZF block at file offset 0" + FORMAT_TAIL),
        ("bad_bam_magic", bw.bgzf_bytes(b"BAX\x01" + stream[4:]), "bad BAM magic in the BGZF block at file offset 0" + FORMAT_TAIL),
        ("empty_file", b"", "no BAM magic in the BGZF block at file offset 0" + FORMAT_TAIL),
    ]


def record_cases():
    """(name, BGZF bytes, message): every record malformation, the bad record late in the file, a second bad one behind it"""
    head, recs, h, d = good_bam_parts()
    n_ref = len(bw.parse_sam(bw.terminated(read(os.path.join(d, "in.sam"))))[1])

    def plain_read(r):       # mapped, primary, its CIGAR one long match: a record in which every field at fault is looked at
        ref, _, l_name, _, _, n_cigar, flag = struct.unpack_from("<iiBBHHH", r, 4)
        return ref >= 0 and not flag & 0x904 and n_cigar == 1 and struct.unpack_from("<I", r, 36 + l_name)[0] & 15 == 0 and struct.unpack_from("<I", r, 36 + l_name)[0] >> 4 >= 40
    k = max(i for i in range(len(recs) - 5) if plain_read(recs[i]))
    assert k > len(recs) // 2

    def mutate(r, what):
        body = bytearray(r[4:])
        if what == "block_size_below_32":
            return struct.pack("<I", 31) + bytes(body)
        if what == "l_read_name_zero":
            body[8] = 0
        elif what == "name_and_cigar_beyond_block_size":
            struct.pack_into("<H", body, 12, 60000)
        elif what == "ref_id_at_n_ref":
            struct.pack_into("<i", body, 0, n_ref)
        elif what == "ref_id_below_minus_one":
            struct.pack_into("<i", body, 0, -2)
        elif what == "cigar_op_code_nine":
            body[32 + body[8]] = (body[32 + body[8]] & 0xf0) | 9
        elif what == "pos_below_minus_one":
            struct.pack_into("<i", body, 4, -2)
        elif what == "pos_two_to_the_31":
            struct.pack_into("<i", body, 4, 2 ** 31 - 1)
        elif what == "reference_end_beyond_two_to_the_31":
            struct.pack_into("<i", body, 4, 2 ** 31 - 30)
        return struct.pack("<I", len(body)) + bytes(body)

    kinds = ["block_size_below_32", "l_read_name_zero", "name_and_cigar_beyond_block_size", "ref_id_at_n_ref", "ref_id_below_minus_one", "cigar_op_code_nine",
             "pos_below_minus_one", "pos_two_to_the_31", "reference_end_beyond_two_to_the_31"]
    out = []
    at = len(head) + sum(len(r) for r in recs[:k])
    for what in kinds:
        # (a record that makes a read, so that the field at fault is looked at)
        rs = list(recs)
        rs[k] = mutate(recs[k], what)
        if what != "block_size_below_32":
            rs[k + 3] = mutate(recs[k + 3], "l_read_name_zero")
        out.append((what, head + b"".join(rs), "#%d:<BAM record at byte %d of the inflated stream>" % (h + k + 1, at)))
    whole = head + b"".join(recs)
    last = len(head) + sum(len(r) for r in recs[:-1])
    out.append(("record_past_the_end", whole[:-5], "#%d:<BAM record at byte %d of the inflated stream>" % (h + len(recs), last)))
    out.append(("block_size_field_past_the_end", whole + b"\x40\x00", "#%d:<BAM record at byte %d of the inflated stream>" % (h + len(recs) + 1, len(whole))))
    return [(name, stream, msg) for name, stream, msg in out]


DEFLATE_CASES, FILE_CASES, RECORD_CASES = None, None, None


def all_corrupt_cases():
    global DEFLATE_CASES, FILE_CASES, RECORD_CASES
    if DEFLATE_CASES is None:
        DEFLATE_CASES, FILE_CASES, RECORD_CASES = deflate_cases(), file_cases(), record_cases()
    cases = [(n, data, LSQ_E_FORMAT, msg) for n, data, msg in DEFLATE_CASES + FILE_CASES]
    for layout in ("htslib", "cut61"):
        cases += [("%s-%s" % (n, layout), bw.bgzf_bytes(stream, layout), LSQ_E_PARSE, msg) for n, stream, msg in RECORD_CASES]
    return cases


CORRUPT_NAMES = (["over_subscribed_literal_code", "incomplete_literal_code", "over_subscribed_distance_code", "incomplete_distance_code",
                  "match_through_an_empty_distance_code", "truncated_stream", "block_type_3", "len_nlen_mismatch", "over_subscribed_code", "incomplete_code", "distance_before_the_start", "output_over_isize",
                  "output_under_isize", "bsize_past_eof", "missing_bc", "bad_gzip_magic", "bad_gzip_magic_at_the_start", "bad_bam_magic", "empty_file"] +
                 ["%s-%s" % (n, lay) for lay in ("htslib", "cut61") for n in
                  ("block_size_below_32", "l_read_name_zero", "name_and_cigar_beyond_block_size", "ref_id_at_n_ref", "ref_id_below_minus_one", "cigar_op_code_nine",
                   "pos_below_minus_one", "pos_two_to_the_31", "reference_end_beyond_two_to_the_31", "record_past_the_end", "block_size_field_past_the_end")])


def corrupt_case(name):
    return next(c for c in all_corrupt_cases() if c[0] == name)


def test_the_corrupt_set_is_complete():
    assert [c[0] for c in all_corrupt_cases()] == CORRUPT_NAMES


@pytest.mark.parametrize("name", CORRUPT_NAMES)
def test_corrupt_inputs_give_their_status_and_message(name, tmp_path, check_program):
    """converter, host parser (one thread and several), executable and the sanitizer program: the documented status and message"""
    _, data, status, msg = corrupt_case(name)
    _, _, _, d = good_bam_parts()
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as f:
        f.write(data)
    ev = events_of(d)
    with pytest.raises(L.LsqError) as e:
        L.bam_to_mrf(data)
    assert e.value.status == status and str(e.value).endswith(": " + msg), str(e.value)
    for n_threads in (1, 0):
        with pytest.raises(L.LsqError) as e:
            L.Reads.from_bam(path, ev, n_threads=n_threads)
        assert e.value.status == status and str(e.value).endswith(": " + msg), str(e.value)
    p = subprocess.run([os.path.join(BIN, "bam2mrf"), path], capture_output=True, text=True)
    assert p.returncode == 1 and p.stdout == "" and msg in p.stderr and ("Lexical_cast error" in p.stderr) == (status == LSQ_E_PARSE)
    assert run_check(check_program, ["mrf", path]) == "%d %s" % (status, msg)


def test_good_streams_are_clean_in_the_sanitizer_program(tmp_path, check_program):
    for name in SAM_CASES:
        c, d = load(name)
        sam = bw.terminated(read(os.path.join(d, "in.sam")))
        for layout in ("htslib", "cut61", "flush", "stored"):
            path = str(tmp_path / "g.bam")
            with open(path, "wb") as f:
                f.write(bw.sam_to_bam(sam, layout))
            for cv in c["conversions"]:
                mrf = read(os.path.join(d, cv["mrf"])).split(b"\n")[1:-1]
                n_head = bw.parse_sam(sam)[0].count("\n")
                reads = sum(1 for ln in mrf if ln != b"#")
                blocks = sum(ln.count(b",") + 1 for ln in mrf if ln != b"#")
                assert run_check(check_program, ["mrf", path, str(cv["skip_flags"]), str(cv["min_mapq"])]) == "ok %d %d %d" % (len(mrf) - n_head, reads, blocks)


def test_header_shapes(tmp_path):
    """a header text without a final newline counts its last line; a text with NUL padding ends at the NUL; a header that spans
    many blocks; no records at all"""
    head, recs, _, d = good_bam_parts()
    ev = events_of(d)
    refs = head[8 + struct.unpack_from("<I", head, 4)[0]:]
    for text, h in ((b"@HD\tVN:1.6\n@CO\tx", 2), (b"@HD\tVN:1.6\n\0\0\0", 1), (b"", 0), (b"@CO\t" + b"y" * 200000 + b"\n", 1)):
        stream = b"BAM\x01" + struct.pack("<I", len(text)) + text + refs
        got = L.bam_to_mrf(bw.bgzf_bytes(stream + b"".join(recs[:40]), "cut997")).split(b"\n")
        assert got[:1 + h] == [b"AlignmentBlocks"] + [b"#"] * h and len(got) == 1 + h + 40 + 1
        assert L.bam_to_mrf(bw.bgzf_bytes(stream)) == b"AlignmentBlocks\n" + b"#\n" * h
        path = str(tmp_path / "h.bam")
        with open(path, "wb") as f:
            f.write(bw.bgzf_bytes(stream + b"".join(recs[:40])))
        r = L.Reads.from_bam(path, ev)
        if len(r):
            assert int(r.arrays()[1][0]) > h


def test_new_entry_points_are_exported():
    for sym in ("lsq_bam_parse", "lsq_bam_to_mrf", "lsq_last_bam_paths", "lsq_last_ingest_stage_count", "lsq_debug_bgzf_inflate"):
        assert hasattr(L.lib, sym), sym
    header = open(os.path.join(ROOT, "include", "lesseq_hip.h")).read()
    for sym in ("lsq_bam_parse", "lsq_bam_to_mrf", "lsq_last_bam_paths", "lsq_last_ingest_stage_count"):
        assert sym + "(" in header
    assert L.lib.lsq_abi_version() == 2
    with pytest.raises(L.LsqError) as e:
        L.Reads.from_bam(os.path.join(ROOT, "no", "such.bam"), events_of(os.path.join(GOLD, "basic")))
    assert e.value.status == -2
