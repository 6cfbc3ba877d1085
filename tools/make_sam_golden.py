#!/usr/bin/env python3
"""Capture tests/golden/sam/: SAM inputs invented here from fixed seeds, their MRF equivalents made by the pure-Python
converter below (written from the format's definition in DESIGN.md 4.9, independently of lsq_sam_line.hpp), and what the
reference's own prebuilt bin/count and bin/solve print for those MRF files -- standard output, standard error and exit
status, each recorded.  CPU only, run in a build tree that has the reference next to it:

    make -C oracle ref && python tools/make_sam_golden.py

Per case directory: in.sam, in.mrf (further <name>.mrf where a case converts one input several ways), x.interval, x.map,
case.json and the captured outputs.  case.json: "conversions" (sam, mrf, skip_flags, min_mapq) and "runs" -- per run the
tool, `argv` (the SAM_SINGLE command line of this project), `ref_argv` (the MRF_SINGLE one the reference was given),
`options` (sam_skip_flags / sam_min_mapq where not the defaults), exit status, the file holding stdout, and stderr itself.
Nothing of the reference is copied: only what its programs read and wrote.  A case on which the reference ends with a
signal is refused, so a fixture can never record a crash as truth.
"""
import json
import os
import random
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "sam")
REF = os.environ.get("LSQ_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_inputs as gi  # noqa: E402

DEFAULT_SKIP = 0x904
POS_MAX = 2 ** 31 - 1
CIGAR_RE = re.compile(rb"([0-9]+)([MIDNSHP=X])")
UINT_RE = re.compile(rb"[0-9]+")


class Malformed(Exception):
    def __init__(self, k, line):
        Exception.__init__(self, "#%d:%s" % (k, line.decode("latin-1")))
        self.k, self.line = k, line


def _uint(field, limit):
    if not UINT_RE.fullmatch(field):
        return None
    v = int(field)
    return v if v <= limit else None


def convert_line(line, skip_flags, min_mapq):
    """b'#' or the MRF blocks of one SAM line (without its newline); None for a malformed line"""
    if line[:1] == b"@":
        return b"#"
    f = line.split(b"\t")
    if len(f) < 6:
        return None
    flag, mapq = _uint(f[1], 65535), _uint(f[4], 255)
    if flag is None or mapq is None:
        return None
    if flag & skip_flags or mapq < min_mapq:
        return b"#"
    pos = _uint(f[3], POS_MAX)
    if pos is None:
        return None
    rname, cigar = f[2], f[5]
    if cigar == b"*":
        return b"#"
    ops, at = [], 0
    for m in CIGAR_RE.finditer(cigar):
        if m.start() != at or int(m.group(1)) > POS_MAX:
            return None
        ops.append((int(m.group(1)), m.group(2)))
        at = m.end()
    if at != len(cigar) or not ops:
        return None
    if rname == b"*" or pos == 0 or b":" in rname or b"," in rname or rname[:1] == b"#":
        return b"#"
    strand = b"-" if flag & 0x10 else b"+"
    ref, bs, q, qs, qe, blocks = pos, pos, 1, 1, 0, []
    for n, op in ops:
        if op in b"M=XD":
            if n > 0:
                if ref == bs:
                    qs, qe = q, q - 1
                ref += n
                if op != b"D":
                    q += n
                    qe = q - 1
        elif op == b"N":
            if ref > bs:
                blocks.append((bs, ref - 1, qs, qe))
            ref += n
            bs = ref
        elif op in b"IS":
            q += n
        if ref - 1 > POS_MAX:
            return None
    if ref > bs:
        blocks.append((bs, ref - 1, qs, qe))
    if not blocks:
        return b"#"
    return b",".join(b"%s:%s:%d:%d:%d:%d" % (rname, strand, a, b, c, d) for a, b, c, d in blocks)


def sam_to_mrf(data, skip_flags=DEFAULT_SKIP, min_mapq=0):
    out = [b"AlignmentBlocks"]
    lines = data.split(b"\n")[:-1]                 # a last line without a newline is never seen
    for k, line in enumerate(lines, 1):
        r = convert_line(line, skip_flags, min_mapq)
        if r is None:
            raise Malformed(k, line)
        out.append(r)
    return b"\n".join(out) + b"\n"


# ----------------------------------------------------------------------------- inputs

QUAL_CHARS = "!\"#$%&'()*+,-./0123456789:;<=>?@ABCDEFGHIJ"


def seq_qual(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n)), "".join(rng.choice(QUAL_CHARS) for _ in range(n))


def cigar_qlen(cigar):
    return sum(int(n) for n, op in re.findall(r"([0-9]+)([MIDNSHP=X])", cigar) if op in "MIS=X")


WITH_SEQ = True          # SEQ and QUAL of the read's bases (`basic`); "*" elsewhere, which keeps the other fixtures small


def record(rng, qname, flag, rname, pos, mapq, cigar, tags=True, qlen=None):
    n = cigar_qlen(cigar) if qlen is None else qlen
    seq, qual = seq_qual(rng, n) if n and (WITH_SEQ or qlen is not None) else ("*", "*")
    f = [qname, str(flag), rname, str(pos), str(mapq), cigar, "*", "0", "0", seq, qual]
    if tags:
        f += ["NH:i:1", "NM:i:%d" % rng.randrange(3), "XS:A:%s" % rng.choice("+-")]
    return "\t".join(f) + "\n"


def blocks_cigar(rng, blocks, fancy=True):
    """(POS, CIGAR) of 0-based half-open blocks in ascending order; the M runs dressed up without moving a block"""
    parts = []
    for k, (s, e) in enumerate(blocks):
        if k:
            parts.append("%dN" % (s - blocks[k - 1][1]))
        n = e - s
        v = rng.random() if fancy else 1.0
        if v < 0.15 and n > 6:
            a = rng.randrange(1, n - 2)
            b = rng.randrange(1, n - a)
            parts.append("%d=%dX%d=" % (a, b, n - a - b) if n - a - b else "%d=%dX" % (a, b))
        elif v < 0.25 and n > 4:
            a = rng.randrange(1, n - 1)
            parts.append("%dM%dI%dM" % (a, rng.randrange(1, 4), n - a))
        else:
            parts.append("%dM" % n)
    c = "".join(parts)
    if fancy and rng.random() < 0.2:
        c = "%dS" % rng.randrange(1, 9) + c
    if fancy and rng.random() < 0.2:
        c += "%dS" % rng.randrange(1, 9)
    if fancy and rng.random() < 0.05:
        c = "7H" + c + "3H"
    return blocks[0][0] + 1, c


def read_record(rng, k, read, mapq=None, fancy=True, flag_extra=0):
    chrom, strand, blocks = read
    ok = all(blocks[i][0] >= blocks[i - 1][1] for i in range(1, len(blocks)))
    if not ok:
        blocks = blocks[:1]
    pos, cigar = blocks_cigar(rng, blocks, fancy)
    flag = (16 if strand == "-" else 0) | flag_extra
    return record(rng, "q%d" % k, flag, chrom, pos, rng.choice([0, 3, 20, 30, 60, 255]) if mapq is None else mapq, cigar)


HEADER = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:9000000\n@SQ\tSN:chr2\tLN:9000000\n@PG\tID:aligner\tPN:aligner\tCL:aligner --in reads.fq:1,2 #x\n"


def events_annotation(rng, n_events, R, chroms):
    events = gi.gen_events(rng, n_events, R, chroms)
    iv, mp = [], []
    for e in events:
        for k, form in enumerate(e["forms"]):
            iname = "%s.%s" % (e["name"], "ab"[k])
            iv.append(gi.interval_line(iname, e["chrom"], e["strand"], form))
            mp.append("%s\t%s\n" % (e["name"], iname))
    return events, "".join(iv), "".join(mp)


def noise(rng, k, events):
    """a record that the default masks skip: unmapped, secondary or supplementary (the last two on real event coordinates)"""
    v = rng.randrange(3)
    if v == 0:
        return record(rng, "u%d" % k, 4, "*", 0, 0, "*", tags=False, qlen=100)
    e = rng.choice(events)
    a, b = e["forms"][0][0]
    return read_record(rng, k, (e["chrom"], e["strand"], [(a, min(b, a + 100))]), flag_extra=256 if v == 1 else 2048)


def basic():
    rng = random.Random(20261016)
    chroms = ["chr1", "chr2"]
    events, iv, mp = events_annotation(rng, 10, 100, chroms)
    reads = gi.gen_reads(rng, events, 100, 100, chroms)
    out = [HEADER]
    for k, r in enumerate(reads):
        if rng.random() < 0.12:
            out.append(noise(rng, k, events))
        out.append(read_record(rng, k, r))
    out.append(read_record(rng, 99999, reads[0]).rstrip("\n"))          # no newline at the end of the file: never seen
    return {"sam": "".join(out), "interval": iv, "map": mp, "R": 100}


CIGAR_IV = (gi.interval_line("G.a", "chr1", "+", [(1000, 1400), (2000, 2300), (3000, 3400), (4000, 4200)])
            + gi.interval_line("G.b", "chr1", "+", [(1000, 1400), (3000, 3400), (4000, 4200)])
            + gi.interval_line("H.a", "chr2", "-", [(500, 900), (1500, 1700), (2500, 2900)])
            + gi.interval_line("H.b", "chr2", "-", [(500, 900), (2500, 2900)]))
CIGAR_MAP = "G\tG.a\nG\tG.b\nH\tH.a\nH\tH.b\n"


def cigar():
    rng = random.Random(77)
    hand = [
        ("chr1", 0, 1101, "50M"),
        ("chr1", 0, 1101, "20M5D30M"),                     # D inside an exon: one block of 55 bases
        ("chr1", 0, 1381, "15M10D25M"),                    # D across an exon end: the block leaves the exon
        ("chr1", 0, 1396, "5M605D20M"),                    # ... a deletion as long as the intron: still one block
        ("chr1", 0, 1101, "5S45M"), ("chr1", 0, 1101, "45M5S"), ("chr1", 0, 1101, "5S40M5S"),
        ("chr1", 0, 1101, "3I47M"), ("chr1", 0, 1101, "47M3I"), ("chr1", 0, 1101, "2S3I40M3I2S"),
        ("chr1", 0, 1101, "5H50M5H"), ("chr1", 0, 1101, "25M2P25M"), ("chr1", 0, 1101, "4H3S20M1P1I22M4S2H"),
        ("chr1", 0, 1381, "20M600N30M"),                   # one gap
        ("chr1", 0, 1381, "20M600N300M700N20M"),           # two gaps
        ("chr1", 0, 1391, "10M600N300M700N400M600N10M"),   # three gaps: four blocks
        ("chr1", 0, 1381, "20M1600N30M"),                  # the skipping form
        ("chr1", 0, 1101, "20S30I"),                       # no block
        ("chr1", 0, 1101, "10H"), ("chr1", 0, 1101, "0M"), ("chr1", 0, 1101, "5N"), ("chr1", 0, 1101, "5N3S"),
        ("chr1", 0, 1101, "0M50M"), ("chr1", 0, 1101, "25M0N25M"), ("chr1", 0, 1101, "0S50M0D"), ("chr1", 0, 1101, "0N50M0N"),
        ("chr1", 0, 1101, "25M0D0I25M"), ("chr1", 0, 1381, "20M0N600N0N30M"),
        ("chr1", 0, 1101, "20=5X25="), ("chr1", 0, 1101, "10=10X10M10=10X"), ("chr1", 0, 1381, "10=10X600N15X15="),
        ("chr1", 0, 1101, "5D45M"), ("chr1", 0, 1101, "45M5D"), ("chr1", 0, 1381, "20M600N5D25M"), ("chr1", 0, 1101, "7D"),
        ("chr1", 0, 1001, "1M1D" * 150),                   # 300 operations, one block of 300 bases
        ("chr1", 0, 1001, "1M1I" * 150),                   # 300 operations, one block of 150 bases
        ("chr1", 0, 1201, "1=1X1M0N" * 75),                # 300 operations, 75 abutting blocks of 3 bases
        ("chr2", 16, 601, "50M"), ("chr2", 16, 881, "20M600N30M"), ("chr2", 16, 881, "20M600N200M800N30M"),
        ("chr2", 16, 881, "20M1600N30M"), ("chr2", 0, 601, "50M"), ("chr2", 16, 601, "10S20=5X5D20M3I5S"),
        ("chr1", 0, 2147483600, "40M"), ("chr1", 0, 2147483647, "1M"), ("chr1", 0, 1073741800, "50M"),
    ]
    out = [HEADER]
    reads = []
    for form in ([(1000, 1400), (2000, 2300), (3000, 3400), (4000, 4200)], [(1000, 1400), (3000, 3400), (4000, 4200)]):
        tlen = sum(b - a for a, b in form)
        for _ in range(18):
            reads.append(("chr1", "+", gi.transcript_blocks(form, rng.randrange(0, tlen - 50), 50)))
    for form in ([(500, 900), (1500, 1700), (2500, 2900)], [(500, 900), (2500, 2900)]):
        tlen = sum(b - a for a, b in form)
        for _ in range(10):
            reads.append(("chr2", "-", gi.transcript_blocks(form, rng.randrange(0, tlen - 50), 50)))
    rng.shuffle(reads)
    k = 0
    for i, r in enumerate(reads):
        out.append(read_record(rng, i, r))
        if k < len(hand):
            chrom, flag, pos, cg = hand[k]
            out.append(record(rng, "h%d" % k, flag, chrom, pos, 60, cg))
            k += 1
    assert k == len(hand)
    # a record whose QNAME alone is 300 bytes, one longer than 8 KiB whose head is short (a 9 KB tag)
    out.append(record(rng, "n" * 300, 0, "chr1", 1151, 60, "50M"))
    out.append(record(rng, "long_tag", 16, "chr2", 601, 60, "50M").rstrip("\n") + "\tZZ:Z:" + "ab:cd,ef#" * 1000 + "\n")
    for i, r in enumerate(reads[:6]):
        out.append(read_record(rng, 1000 + i, r))
    return {"sam": "".join(out), "interval": CIGAR_IV, "map": CIGAR_MAP, "R": 50}


LONG_CHROM = "scaffold_" + "0123456789" * 3 + "x"          # 40 bytes


def names():
    rng = random.Random(5)
    iv = (gi.interval_line("A.1", "c1", "+", [(200, 300), (400, 500)]) + gi.interval_line("A.2", "c1", "+", [(100, 300), (400, 500)])
          + gi.interval_line("L.1", LONG_CHROM, "-", [(1000, 1200), (1500, 1700)]) + gi.interval_line("L.2", LONG_CHROM, "-", [(1000, 1200), (1300, 1350), (1500, 1700)])
          # genes named like reads: reads that span exactly [5000, 5140) on '+' tie with the gene on (start, end, strand) and the
          # NAME decides, bytewise: "read-<k>" against "read-25" / "read-7"
          + gi.interval_line("R.1", "c2", "+", [(5000, 5040), (5100, 5140)]) + gi.interval_line("R.2", "c2", "+", [(5000, 5040), (5060, 5080), (5100, 5140)])
          + gi.interval_line("S.1", "c2", "+", [(9000, 9040), (9100, 9140)]) + gi.interval_line("S.2", "c2", "+", [(9000, 9040), (9060, 9080), (9100, 9140)]))
    mp = "A\tA.1\nA\tA.2\nL\tL.1\nL\tL.2\nread-25\tR.1\nread-25\tR.2\nread-7\tS.1\nread-7\tS.2\n"
    out = ["@HD\tVN:1.6\n", "@SQ\tSN:c1\tLN:100000\n", "@CO\ta comment with\ttabs:and,marks\n"]
    base = [("c1", "+", [(210, 250)]), ("c1", "+", [(260, 300), (400, 440)]), ("c1", "-", [(110, 150)]), ("c1", "+", [(120, 160)]),
            (LONG_CHROM, "-", [(1010, 1060)]), (LONG_CHROM, "-", [(1180, 1200), (1500, 1530)]), (LONG_CHROM, "-", [(1180, 1200), (1300, 1330)]),
            (LONG_CHROM + "y", "-", [(1010, 1060)]), (LONG_CHROM[:-1], "-", [(1010, 1060)]),
            ("c9", "+", [(210, 250)]), ("chrUn_gl000220", "+", [(210, 250)]), ("C1", "+", [(210, 250)]), ("c1 ", "+", [(210, 250)]),
            ("c1:x", "+", [(210, 250)]), ("HLA-A*01:01", "+", [(210, 250)]), ("c1,c2", "+", [(210, 250)]), (":", "-", [(210, 250)]),
            ("#c1", "+", [(210, 250)]), ("c1#", "+", [(210, 250)]), ("=", "+", [(210, 250)])]
    for i, r in enumerate(base):
        out.append(read_record(rng, i, r, fancy=False))
    i = len(base)
    while len(out) < 90:
        n = len(out) + 1          # this line will be read-<n>
        g0 = 5000 if n % 2 else 9000
        if n % 3 == 0:
            r = ("c2", "+", [(g0, g0 + 40), (g0 + 100, g0 + 140)])
        elif n % 3 == 1:
            r = ("c2", "+", [(g0, g0 + 40), (g0 + 60, g0 + 80), (g0 + 100, g0 + 140)])
        else:
            r = ("c2", "-" if n % 4 == 1 else "+", [(g0, g0 + 40), (g0 + 100, g0 + 140)])
        out.append(read_record(rng, i, r, fancy=False))
        i += 1
        if n in (30, 77):
            out.append("@CO\ta header line in the middle of the file consumes a read number\n")
    return {"sam": "".join(out), "interval": iv, "map": mp, "R": 40}


def filters():
    rng = random.Random(31)
    chroms = ["chr1", "chr2"]
    events, iv, mp = events_annotation(rng, 8, 100, chroms)
    reads = gi.gen_reads(rng, events, 170, 100, chroms)
    out = [HEADER]
    for k, r in enumerate(reads):
        v = rng.random()
        extra = 0
        if v < 0.10:
            extra = 256
        elif v < 0.20:
            extra = 2048
        elif v < 0.28:
            extra = 4                      # flagged unmapped but with coordinates (an aligner's mate-placed record)
        elif v < 0.36:
            extra = 1024 | 1 | 64
        out.append(read_record(rng, k, r, flag_extra=extra))
        if v > 0.93:
            out.append(record(rng, "u%d" % k, 4, "*", 0, 0, "*", tags=False, qlen=100))
    return {"sam": "".join(out), "interval": iv, "map": mp, "R": 100}


def multi():
    rng = random.Random(404)
    chroms = ["chr1", "chr2", "chr3"]
    events, iv, mp = events_annotation(rng, 8, 75, chroms)
    out = [HEADER]
    for k, r in enumerate(gi.gen_reads(rng, events, 100, 75, chroms)):
        out.append(read_record(rng, k, r))
    other = "AlignmentBlocks\n" + "".join(gi.mrf_line(*r) for r in gi.gen_reads(rng, events, 50, 36, chroms))
    return {"sam": "".join(out), "interval": iv, "map": mp, "R": 75, "other_mrf": other}


# ----------------------------------------------------------------------------- capture

def run_ref(tool, argv, cwd):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "oracle", "_ref", "lib"))
    p = subprocess.run([os.path.join(REF, "bin", tool)] + argv, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode < 0 or p.returncode >= 128:
        raise SystemExit("the reference's %s ended with status %d (a signal) in %s: this input cannot be a fixture" % (tool, p.returncode, cwd))
    return p.returncode, p.stdout, p.stderr


def write(path, data):
    with open(path, "wb") as f:
        f.write(data if isinstance(data, bytes) else data.encode("latin-1"))


def capture(name, inp, variants=None, reads=None, extra=None):
    """variants: [(mrf file name, options)] conversions of in.sam, a run of count and solve each; reads: the read files of
    a run as [(format, read type, R, sam-side file, mrf-side file)] (default: in.sam alone)"""
    d = os.path.join(OUT, name)
    os.makedirs(d)
    sam = inp["sam"].encode("latin-1")
    write(os.path.join(d, "in.sam"), sam)
    write(os.path.join(d, "x.interval"), inp["interval"])
    write(os.path.join(d, "x.map"), inp["map"])
    for fn, data in (extra or {}).items():
        write(os.path.join(d, fn), data)
    case = {"name": name, "conversions": [], "runs": []}
    n_lines = sam.count(b"\n")
    for mrf_name, opts in (variants or [("in.mrf", {})]):
        mrf = sam_to_mrf(sam, opts.get("sam_skip_flags", DEFAULT_SKIP), opts.get("sam_min_mapq", 0))
        assert mrf.count(b"\n") == n_lines + 1
        write(os.path.join(d, mrf_name), mrf)
        case["conversions"].append({"sam": "in.sam", "mrf": mrf_name, "skip_flags": opts.get("sam_skip_flags", DEFAULT_SKIP), "min_mapq": opts.get("sam_min_mapq", 0)})
        rf = reads or [("SAM_SINGLE", "SHORT_READ", inp["R"], "in.sam", mrf_name)]
        base = ["0", "x", "./", "LH_GENE_TXT", "x.interval", "UCSC_GENE2ISOFORM", "x.map", "0", "1000000"]
        for tool in ("count", "solve"):
            argv, ref_argv = list(base), list(base)
            for fmt, rt, R, sam_side, mrf_side in rf:
                trb = [str(1000 * R)] if tool == "solve" else []
                argv += [fmt, rt, str(R), sam_side] + trb
                ref_argv += ["MRF_SINGLE", rt, str(R), mrf_side if fmt == "SAM_SINGLE" else sam_side] + trb
            rc, so, se = run_ref(tool, ref_argv, d)
            stem = "%s%s" % (tool, "" if mrf_name == "in.mrf" else "." + mrf_name[:-4])
            write(os.path.join(d, stem + ".out"), so)
            case["runs"].append({"tool": tool, "argv": argv, "ref_argv": ref_argv, "options": opts, "exit": rc, "stdout": stem + ".out", "stderr": se.decode("latin-1")})
            print("%-10s %-5s %-22s exit %d, %5d bytes of stdout, %d SAM lines" % (name, tool, mrf_name, rc, len(so), n_lines))
    with open(os.path.join(d, "case.json"), "w") as f:           # a line per conversion and per run
        f.write('{"name": %s,\n "conversions": [\n  %s],\n "runs": [\n  %s]}\n' % (json.dumps(name), ",\n  ".join(json.dumps(c, sort_keys=True) for c in case["conversions"]),
                                                                                 ",\n  ".join(json.dumps(r, sort_keys=True) for r in case["runs"])))


def main():
    if not os.path.isdir(os.path.join(REF, "bin")):
        raise SystemExit("no reference tree at %s" % REF)
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "lib", "libgsl.so.0")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    global WITH_SEQ
    capture("basic", basic())
    WITH_SEQ = False
    capture("cigar", cigar())
    capture("names", names())
    capture("filters", filters(), variants=[("in.mrf", {}), ("in.skip4.mrf", {"sam_skip_flags": 4}), ("in.mapq30.mrf", {"sam_min_mapq": 30})])
    m = multi()
    capture("multi", m, reads=[("SAM_SINGLE", "MEDIUM_READ", m["R"], "in.sam", "in.mrf"), ("MRF_SINGLE", "SHORT_READ", 36, "other.mrf", "other.mrf")],
            extra={"other.mrf": m["other_mrf"]})


if __name__ == "__main__":
    main()
