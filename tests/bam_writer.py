"""A BAM writer for the tests, pure Python (struct, zlib): the '\\n'-terminated lines of a well-formed SAM text as a BAM file,
in a chosen BGZF layout.  Not a test.

What the text loses on the way, none of which BAM_SINGLE reads: a QNAME beyond BAM's 254 bytes is cut, optional fields are
dropped.  References come from the @SQ lines, then any other RNAME in order of appearance.  A last line without '\\n' is not
a record, as in SAM.  The '@' lines ahead of the first record are the header text, and '@' lines come first -- but for comment
lines ("@CO") behind a record, which tests/golden/sam/names holds: in SAM_SINGLE such a line makes no read and takes a read
number, a BAM file has no place for it, and it is written as a record that does the same (unmapped, no reference, no CIGAR).
Any other '@' line behind a record is refused."""
import struct
import zlib

MAX_PAYLOAD = 0xff00        # what htslib puts into one BGZF block at most
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# every layout the tests run: how the inflated stream is cut into blocks, and how each block is deflated
LAYOUTS = ("htslib", "cut997", "cut61", "stored", "fixed", "flush", "isize0", "extra", "noeof")


def bgzf_block(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, extra=b""):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush_at is None:
        data = c.compress(payload) + c.flush()
    else:       # several deflate blocks, an empty stored one among them
        data = c.compress(payload[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(payload[flush_at:]) + c.flush()
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(data) + 8
    assert bsize <= 65536 and len(payload) <= 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + extra + b"BC" + struct.pack("<HH", 2, bsize - 1) + data +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def bgzf_file(chunks, layout="htslib"):
    """the chunks of an inflated stream, a BGZF block each, deflated as the layout says"""
    out = []
    for k, ch in enumerate(chunks):
        if layout == "stored":
            out.append(bgzf_block(ch, level=0))
        elif layout == "fixed":
            out.append(bgzf_block(ch, strategy=zlib.Z_FIXED))
        elif layout == "flush":
            out.append(bgzf_block(ch, flush_at=len(ch) // 2))
        elif layout == "extra":
            out.append(bgzf_block(ch, extra=b"XY" + struct.pack("<H", 3) + b"abc"))
        else:
            out.append(bgzf_block(ch))
        if layout == "isize0" and k == len(chunks) // 2:
            out.append(bgzf_block(b""))
    if layout != "noeof":
        out.append(EOF_BLOCK)
    return b"".join(out)


def split_stream(stream, layout):
    """a raw byte stream in the layout's blocks (no records to respect)"""
    n = {"cut997": 997, "cut61": 61}.get(layout, MAX_PAYLOAD)
    return [stream[i:i + n] for i in range(0, len(stream), n)] or [b""]


def bgzf_bytes(stream, layout="htslib"):
    return bgzf_file(split_stream(stream, layout), layout)


def reg2bin(beg, end):
    if end > 1 << 29:            # beyond what the binning index covers
        return 0
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


CIGAR_OPS = "MIDNSHP=X"
SEQ_CODES = "=ACMGRSVTWYHKDBN"


def record(fields, ref_ids):
    f = list(fields) + ["*", "0", "0", "*", "*"][max(len(fields) - 6, 0):]      # (fields 7-11 a short line leaves out)
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    name = qname.encode("latin-1")[:254] + b"\0"
    ops = []
    if cigar != "*":
        num = ""
        for ch in cigar:
            if ch.isdigit():
                num += ch
            else:
                assert num and int(num) < (1 << 28), cigar
                ops.append(int(num) << 4 | CIGAR_OPS.index(ch))
                num = ""
        assert not num, cigar
    assert len(ops) <= 65535
    ref = -1 if rname == "*" else ref_ids[rname]
    pos0 = int(pos) - 1
    ref_len = sum(v >> 4 for v in ops if CIGAR_OPS[v & 15] in "MDN=X")
    l_seq = 0 if seq == "*" else len(seq)
    packed = bytearray((l_seq + 1) // 2)
    for i in range(l_seq):
        code = SEQ_CODES.find(seq[i].upper())
        packed[i // 2] |= (15 if code < 0 else code) << (4 if i % 2 == 0 else 0)
    q = b"\xff" * l_seq if qual == "*" or len(qual) != l_seq else bytes(max(ord(c) - 33, 0) & 0xff for c in qual)
    nref = -1 if rnext == "*" else ref if rnext == "=" else ref_ids.get(rnext, -1)
    body = struct.pack("<iiBBHHHiiii", ref, pos0, len(name), int(mapq), reg2bin(max(pos0, 0), max(pos0, 0) + max(ref_len, 1)), len(ops), int(flag), l_seq,
                       nref, int(pnext) - 1, int(tlen)) + name + struct.pack("<%dI" % len(ops), *ops) + bytes(packed) + q
    return struct.pack("<I", len(body)) + body


def parse_sam(sam_bytes):
    """(header text, reference names and lengths, the records' fields) of the '\\n'-terminated lines of a SAM text"""
    lines = sam_bytes.decode("latin-1").split("\n")[:-1]
    n_head = 0
    while n_head < len(lines) and lines[n_head].startswith("@"):
        n_head += 1
    refs = []
    for ln in lines[:n_head]:
        if ln.startswith("@SQ\t"):
            tags = dict(t.split(":", 1) for t in ln.split("\t")[1:] if ":" in t)
            if "SN" in tags and tags["SN"] not in [r[0] for r in refs]:
                refs.append((tags["SN"], int(tags.get("LN", "0"))))
    assert not any(ln.startswith("@") and not ln.startswith("@CO\t") for ln in lines[n_head:]), "header lines come first"
    recs = [["late_comment_line", "4", "*", "0", "0", "*"] if ln.startswith("@CO\t") else ln.split("\t") for ln in lines[n_head:]]
    for f in recs:
        assert len(f) >= 6, f
        if f[2] != "*" and f[2] not in [r[0] for r in refs]:
            refs.append((f[2], 0))
    return "".join(ln + "\n" for ln in lines[:n_head]), refs, recs


def bam_stream(sam_bytes):
    """(the BAM header's bytes, the records' bytes) of a SAM text"""
    text, refs, recs = parse_sam(sam_bytes)
    t = text.encode("latin-1")
    head = b"BAM\x01" + struct.pack("<I", len(t)) + t + struct.pack("<I", len(refs))
    for name, ln in refs:
        nm = name.encode("latin-1") + b"\0"
        head += struct.pack("<I", len(nm)) + nm + struct.pack("<I", ln)
    ids = {name: i for i, (name, _) in enumerate(refs)}
    return head, [record(f, ids) for f in recs]


def sam_to_bam(sam_bytes, layout="htslib"):
    head, recs = bam_stream(sam_bytes)
    if layout in ("cut997", "cut61"):
        return bgzf_bytes(head + b"".join(recs), layout)
    # htslib: the header in blocks of its own; a block is flushed before a record that would not fit (a record larger than a
    # block is cut wherever the blocks end)
    chunks = split_stream(head, layout)
    cur = b""
    for r in recs:
        if cur and len(cur) + len(r) > MAX_PAYLOAD:
            chunks.append(cur)
            cur = b""
        cur += r
        while len(cur) > MAX_PAYLOAD:
            chunks.append(cur[:MAX_PAYLOAD])
            cur = cur[MAX_PAYLOAD:]
    if cur:
        chunks.append(cur)
    return bgzf_file(chunks, layout)


def terminated(sam_bytes):
    """the text's '\\n'-terminated lines alone: what the BAM holds"""
    return sam_bytes[:sam_bytes.rfind(b"\n") + 1]
