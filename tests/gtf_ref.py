"""A restatement of what the reference's prebuilt bin/parseGencode and bin/gencodeIsoformMap do (they ship without
source; the rules were probed black-box and are listed in DESIGN.md 4.8), for inputs that have no reference beside them.
test_gtf_host.py pins this file to the reference: it must reproduce every fixture of tests/golden/gtf/ byte for byte.

Where the reference dies of a segmentation fault there is nothing to restate; the rules of this project apply there:
lines that are empty or begin with '#' are skipped, a line of fewer than nine TAB-separated fields is an input error, and
so is a map-input line without '|' (unless it is the only line, which the reference prints)."""

def lines_of(data):
    """[(1-based number, bytes)]: '\\n' ends a line and takes one '\\r' before it along; the last line needs no newline
    (and keeps its '\\r')."""
    out = []
    pieces = data.split(b"\n")
    last_unterminated = pieces.pop()
    for no, p in enumerate(pieces, 1):
        out.append((no, p[:-1] if p.endswith(b"\r") else p))
    if last_unterminated:
        out.append((len(pieces) + 1, last_unterminated))
    return out


def atoi32(field):
    """C's atoi: blanks, a sign, digits; strtol saturates at the ends of a 64-bit long; the low 32 bits are taken."""
    i = 0
    while i < len(field) and field[i:i + 1] in (b" ", b"\t", b"\n", b"\v", b"\f", b"\r"):
        i += 1
    neg = False
    if i < len(field) and field[i:i + 1] in (b"+", b"-"):
        neg = field[i:i + 1] == b"-"
        i += 1
    v = 0
    while i < len(field) and 48 <= field[i] <= 57:
        v = v * 10 + field[i] - 48
        i += 1
    v = -v if neg else v
    v = max(-2 ** 63, min(2 ** 63 - 1, v))
    return wrap32(v)


def wrap32(v):
    v &= 0xFFFFFFFF
    return v - 2 ** 32 if v >= 2 ** 31 else v


class Problem(Exception):
    pass


def attribute(attrs, key):
    """Field 9 is cut at every ';' (quotes do not protect one).  The first piece that holds `key` anywhere is the item; its
    value runs from behind the item's first '"' to its last '"', or to the item's end when it holds one quote only."""
    for item in attrs.split(b";"):
        if key in item:
            q0 = item.find(b'"')
            if q0 < 0:
                raise Problem(b"PROBLEM: Unexpected token: " + item)
            q1 = item.rfind(b'"')
            return item[q0 + 1:q1] if q1 > q0 else item[q0 + 1:]
    raise Problem(b"PROBLEM: Expected to find attribute: " + key)


def parse_gencode(data):
    """(exit status, standard output, standard error) of `parseGencode` on the GTF bytes"""
    tx = {}          # (gene, transcript) -> [chrom, strand, starts, ends], chrom / strand of the first exon line in file order
    try:
        for no, line in lines_of(data):
            if not line or line.startswith(b"#"):
                continue
            f = line.split(b"\t")
            if len(f) < 9:
                raise Problem(b"PROBLEM: line %d has fewer than nine TAB-separated fields" % no)
            gene = attribute(f[8], b"gene_id")                 # every line is checked, whatever its feature
            transcript = attribute(f[8], b"transcript_id")
            if f[2] != b"exon":
                continue
            t = tx.setdefault((gene, transcript), [f[0], f[6], [], []])
            t[2].append(wrap32(atoi32(f[3]) - 1))
            t[3].append(atoi32(f[4]))
    except Problem as p:
        return 1, b"", p.args[0] + b"\n"
    out = []
    for (gene, transcript) in sorted(tx):                       # two keys, bytewise
        chrom, strand, starts, ends = tx[(gene, transcript)]
        starts.sort()
        ends.sort()                                             # each list on its own
        out.append(b"\t".join([gene + b"|" + transcript, chrom, strand, b"%d" % starts[0], b"%d" % ends[-1], b"%d" % len(starts),
                               b",".join(b"%d" % s for s in starts), b",".join(b"%d" % e for e in ends)]) + b"\n")
    return 0, b"".join(out), b""


def transcripts(data):
    """[(name, chrom, strand, starts, ends)] in output order, from parse_gencode's text"""
    rc, out, _ = parse_gencode(data)
    assert rc == 0
    res = []
    for line in out.split(b"\n")[:-1]:
        f = line.split(b"\t")
        res.append((f[0], f[1], f[2], [int(x) for x in f[6].split(b",")], [int(x) for x in f[7].split(b",")]))
    return res


def isoform_map(data):
    """(exit status, standard output, standard error) of `gencodeIsoformMap` on the name list"""
    lines = [(no, l) for no, l in lines_of(data) if l]
    if len(lines) > 1:
        for no, l in lines:
            if b"|" not in l:
                return 1, b"", b"PROBLEM: line %d has no '|' between gene and transcript id\n" % no
    out, counter, prev = [], 1, None
    for _, l in lines:
        key = l.split(b"|", 1)[0]
        if prev is not None and key != prev:
            counter += 1
        prev = key
        out.append(b"%d\t" % counter + l + b"\n")
    return 0, b"".join(out), b""


def cut_f1(interval):
    return b"".join(l.split(b"\t", 1)[0] + b"\n" for l in interval.split(b"\n")[:-1])
