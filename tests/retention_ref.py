"""The retention table's definition (include/lesseq_hip.h, lsq_ir_*) restated in plain Python from the MRF text and
the interval file themselves -- no parser, no sort and no depth row of the library is involved -- and the hand-built inputs the
retention tests share.  Columns 1-9 are sites_ref's; the depth is coverage_ref.depth_arrays' dense numpy array per chromosome; the
clean mask is painted from every exon of the interval text; an order statistic is np.sort(depth[mask])[k - 1].  The cases keep
their coordinates within a few hundred thousand bases, so the dense arrays stay small."""
import random

import numpy as np

import coverage_ref as V
import junction_ref as J
import sites_ref as S
from junction_ref import LIM, interval_line, mrf_line, write_case  # noqa: F401

REPORT = S.REPORT + ("introns", "no_clean", "pieces", "depth_rows", "bases")


# ----------------------------------------------------------------------------- the definition

def exons_by_chrom(interval_text):
    """{chrom: [(start, end)]}: every exon of every line with end > start, clamped to +-2^30"""
    out = {}
    for chrom, _, exons in J.isoforms(interval_text):
        for s, e in exons:
            s, e = max(s, -LIM), min(e, LIM)
            if e > s:
                out.setdefault(chrom, []).append((s, e))
    return out


def clean_mask(exons, a, b):
    """bool[b - a]: the bases of [a, b) in no exon"""
    mask = np.ones(b - a, bool)
    for s, e in exons:
        if s < b and e > a:
            mask[max(s, a) - a:min(e, b) - a] = False
    return mask


def body_depth(arrays, chrom, a, b):
    """int64[b - a]: the depth over [a, b), 0 where the chromosome has no counted block"""
    full = np.zeros(b - a, np.int64)
    if chrom in arrays:
        lo, depth = arrays[chrom]
        x, y = max(a, lo), min(b, lo + len(depth))
        if y > x:
            full[x - a:y - a] = depth[x - lo:y - lo]
    return full


def pieces_of(mask, a):
    """[(start, end)]: the maximal stretches of clean bases"""
    edge = np.flatnonzero(np.diff(np.concatenate(([0], mask.astype(np.int8), [0]))))
    return [(a + int(s), a + int(e)) for s, e in zip(edge[0::2], edge[1::2])]


def rank(q, n):
    return (q * n + 3) // 4


def table(interval_text, mrf_text, min_overhang=1):
    """(rows, report): rows [(chrom, start, end, ann, reads, left_spliced, left_through, right_spliced, right_through, clean, covered,
    depth_sum, q25, q50, q75)] in table order; report the thirteen numbers"""
    srows, srep = S.table(interval_text, mrf_text, min_overhang)
    arrays, crep = V.depth_arrays(interval_text, mrf_text)
    exons = exons_by_chrom(interval_text)
    near = {}                         # (chrom, 4096-base window) -> the exons that touch it: a mask paints only its neighbours
    for c, ex in exons.items():
        for s, e in ex:
            for w in range(s >> 12, ((e - 1) >> 12) + 1):
                near.setdefault((c, w), []).append((s, e))
    rows, no_clean, n_pieces = [], 0, 0
    for r in srows:
        c, a, b, ann = r[:4]
        if ann == ".":
            continue
        ex = [x for w in range(a >> 12, ((b - 1) >> 12) + 1) for x in near.get((c, w), ())]
        mask = clean_mask(ex, a, b)
        d = np.sort(body_depth(arrays, c, a, b)[mask])
        n = len(d)
        n_pieces += len(pieces_of(mask, a))
        no_clean += n == 0
        q = [int(d[rank(k, n) - 1]) if n else 0 for k in (1, 2, 3)]
        rows.append(tuple(r) + (n, int((d >= 1).sum()), int(d.sum())) + tuple(q))
    depth_rows = len(V.fast_rows_of(arrays))
    report = dict(srep, introns=len(rows), no_clean=int(no_clean), pieces=n_pieces, depth_rows=depth_rows, bases=crep["bases"])
    return rows, report


_tables = {}


def table_once(key, interval_text, mrf_text, min_overhang=1):
    """table() of an input that several tests share (and of a file whose order does not matter), computed once a session"""
    if (key, min_overhang) not in _tables:
        _tables[(key, min_overhang)] = table(interval_text, mrf_text, min_overhang)
    return _tables[(key, min_overhang)]


def text(rows, ratios=False):
    def ratio(a, b):
        return "\tNA" if b == 0 else "\t%.6f" % (a / b)
    out = []
    for c, s, e, a, r, ls, lt, rs, rt, n, cov, dsum, q25, q50, q75 in rows:
        line = "%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % (c, s + 1, e, a, r, ls, lt, rs, rt, n, cov, dsum, q25, q50, q75)
        if ratios:
            line += ratio(dsum, n) + ratio(cov, n) + (ratio(q50, q50 + max(ls, rs)) if n else "\tNA")
        out.append(line + "\n")
    return "".join(out)


def pieces_annotation(interval_text):
    """(isoform lines, [[line index]] per row of the table): an annotation whose lines are the pieces of every intron, for
    coverage's region sums; the rows are those of table() -- the annotation's introns, by chromosome name (bytewise), start, end"""
    exons = exons_by_chrom(interval_text)
    lines, of_row = [], []
    for (c, a, b) in sorted(J.introns(interval_text), key=lambda k: (k[0].encode(), k[1], k[2])):
        if not (a > -LIM and b < LIM):
            continue
        mine = []
        for s, e in pieces_of(clean_mask(exons.get(c, []), a, b), a):
            mine.append(len(lines))
            lines.append(interval_line("p%d" % len(lines), c, "+", [(s, e)]))
        of_row.append(mine)
    return lines, of_row


# ----------------------------------------------------------------------------- inputs

def rows_case():
    """(isoform lines, mrf lines, the table by hand at min_overhang 1, its report).  By hand:
    (200, 300), all clean: depth 1 on [200,230), 2 on [230,235), 4 on [235,238), 2 on [238,240), 1 on [240,260), 2 on [260,270), 1 on
    [270,300): 80 ones, 17 twos, 3 fours, sum 126; ranks 25, 50, 75 all fall among the ones.  Two reads are spliced over it, a
    third from its left site to 260 (a novel junction: no row, one more in left_spliced).
    (1100, 1500) less gB.b's exon [1200,1250): pieces [1100,1200) and [1250,1500), 350 bases; depth 2 on [1100,1200) and [1250,1290),
    3 on [1290,1300), 1 on [1300,1310): 190 zeros, 10 ones, 140 twos, 10 threes; ranks 88 and 175 are zeros, rank 263 is a two.
    (2100, 2200) lies in gC.b's exon: no clean base.  (3100, 3110): ten clean bases, no read."""
    iso = [interval_line("gA.a", "chr1", "+", [(100, 200), (300, 400)]),
           interval_line("gB.a", "chr1", "+", [(1000, 1100), (1500, 1600)]),
           interval_line("gB.b", "chr1", "-", [(1200, 1250)]),
           interval_line("gC.a", "chr1", "+", [(2000, 2100), (2200, 2300)]),
           interval_line("gC.b", "chr1", "+", [(2050, 2250)]),
           interval_line("gD.a", "chr1", "+", [(3000, 3100), (3110, 3200)])]
    m = mrf_line
    R = ([m("chr1", "+", [(150, 200), (300, 350)])] * 2 + [m("chr1", "+", [(150, 240)]), m("chr1", "-", [(230, 330)])] + [m("chr1", "+", [(235, 238)])] * 2 +
         [m("chr1", "+", [(150, 200), (260, 270)])] +
         [m("chr1", "+", [(1050, 1300)])] * 2 + [m("chr1", "-", [(1290, 1310)])] + [m("chr1", "+", [(2050, 2250)])])
    rows = [("chr1", 200, 300, "+", 2, 3, 1, 2, 1, 100, 100, 126, 1, 1, 1),
            ("chr1", 1100, 1500, "+", 0, 0, 2, 0, 0, 350, 160, 320, 0, 0, 2),
            ("chr1", 2100, 2200, "+", 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0),
            ("chr1", 3100, 3110, "+", 0, 0, 0, 0, 0, 10, 0, 0, 0, 0, 0)]
    report = dict(zip(REPORT, (11, 14, 3, 0, 0, 9, 7, 3, 4, 1, 4, 14, 1176)))
    return iso, R, rows, report


RATIO_TEXT = ("chr1\t201\t300\t+\t2\t3\t1\t2\t1\t100\t100\t126\t1\t1\t1\t1.260000\t1.000000\t0.250000\n"
              "chr1\t1101\t1500\t+\t0\t0\t2\t0\t0\t350\t160\t320\t0\t0\t2\t0.914286\t0.457143\tNA\n"
              "chr1\t2101\t2200\t+\t0\t0\t1\t0\t1\t0\t0\t0\t0\t0\t0\tNA\tNA\tNA\n"
              "chr1\t3101\t3110\t+\t0\t0\t0\t0\t0\t10\t0\t0\t0\t0\t0\t0.000000\t0.000000\tNA\n")


def geometry_case():
    """(isoform lines, mrf lines): a piece against the rows in every way -- see the comments"""
    il, m = interval_line, mrf_line

    def gene(name, a, b, strand="+"):
        return il(name, "chr1", strand, [(a - 100, a), (b, b + 100)])
    iso = [gene("ends_inside.a", 1100, 1200), gene("begins_inside.a", 2100, 2200), gene("over_all.a", 3100, 3200), gene("on_edges.a", 4100, 4200),
           gene("gaps.a", 5100, 5200),
           gene("two.a", 6100, 6400), il("two.b", "chr1", "-", [(6200, 6250)]),                                  # another isoform's exon inside: two pieces
           gene("three.a", 7100, 7500), il("three.b", "chr1", "+", [(7200, 7250), (7300, 7350)]),                 # three; three.b's own intron (7250, 7300) is nested in it
           gene("covered.a", 8100, 8200), il("covered.b", "chr1", "+", [(8050, 8250)]),                         # no clean base
           gene("outer.a", 9100, 9900), il("outer.b", "chr1", "+", [(9200, 9300), (9400, 9500)]),                 # (9300, 9400) nested in (9100, 9900)
           gene("untouched.a", 10100, 10200),
           il("abut.a", "chr1", "+", [(11000, 11100), (11200, 11300)]), il("abut.b", "chr1", "+", [(11100, 11150)]),      # an exon that begins where the intron does
           il("abut.c", "chr1", "+", [(11190, 11200)])]                                                          # ... and one that ends where it ends
    R = [m("chr1", "+", [(1050, 1150)]),                                          # a row that begins before the piece and ends inside it
         m("chr1", "+", [(2150, 2250)]),                                          # begins inside, ends behind
         m("chr1", "+", [(3050, 3250)]),                                          # one row over the whole intron and beyond both ends
         m("chr1", "+", [(4100, 4200)]), m("chr1", "-", [(4100, 4150)]),          # row edges on the piece's edges
         m("chr1", "+", [(5110, 5140)]), m("chr1", "+", [(5160, 5190)]), m("chr1", "+", [(5120, 5130)]),      # a gap at either end and in the middle
         m("chr1", "+", [(6150, 6300)]), m("chr1", "+", [(6240, 6260)]),          # rows across the exon between two pieces
         m("chr1", "+", [(7050, 7600)]), m("chr1", "+", [(7050, 7600)]), m("chr1", "+", [(7260, 7290)]), m("chr1", "+", [(7340, 7360)]),
         m("chr1", "+", [(8000, 8300)]),
         m("chr1", "+", [(9350, 9450)]), m("chr1", "+", [(9150, 9250), (9300, 9320)]), m("chr1", "+", [(9890, 9950)]),
         m("chr1", "+", [(11090, 11160)]), m("chr1", "+", [(11180, 11260)]), m("chr1", "+", [(11155, 11156)])]
    return iso, R


def rank_case():
    """(isoform lines, mrf lines): introns of n = 1 .. 9 clean bases under a staircase of depths 1 .. n (every value of (q n + 3) div 4,
    n even and odd); ties at the rank (depths 1 1 2 2 2 2 3 3); a rank among the zeros (2 5 0 0 0 3 7 1: q25 = 0 < q50); all bases
    at one depth; a body whose largest depth is 1"""
    iso, R = [], []

    def intron(name, base, n):
        iso.append(interval_line(name + ".a", "chr1", "+", [(base - 50, base), (base + n, base + n + 50)]))
    for n in range(1, 10):
        base = 1000 * n
        intron("stair%d" % n, base, n)
        R += [mrf_line("chr1", "+", [(base + j, base + n)]) for j in range(n)]
    intron("ties", 20000, 8)
    R += [mrf_line("chr1", "+", [(20000, 20008)]), mrf_line("chr1", "+", [(20002, 20008)]), mrf_line("chr1", "+", [(20006, 20008)])]
    intron("zeros", 21000, 8)
    for at, d in ((0, 2), (1, 5), (5, 3), (6, 7), (7, 1)):
        R += [mrf_line("chr1", "-", [(21000 + at, 21001 + at)])] * d
    intron("flat", 22000, 13)
    R += [mrf_line("chr1", "+", [(21990, 22020)])] * 6
    intron("one", 23000, 40)
    R += [mrf_line("chr1", "+", [(23005, 23031)])]
    return iso, R


RANK_ROWS = {20000: (8, 8, 16, 1, 2, 2), 21000: (8, 5, 18, 0, 1, 3), 22000: (13, 13, 78, 6, 6, 6), 23000: (40, 26, 26, 0, 1, 1)}      # start -> clean, covered, depth_sum, q25, q50, q75


def stride_case(counts=(63, 64, 65, 127, 128, 129)):
    """(isoform lines, mrf lines): introns with exactly `counts` depth rows inside -- one-base blocks a base apart, the row's depth 1 + j % 3"""
    iso, R = [], []
    for g, n in enumerate(counts):
        base = 10000 * (g + 1)
        iso.append(interval_line("s%d.a" % n, "chr1", "+", [(base - 50, base), (base + 2 * n + 5, base + 2 * n + 55)]))
        for j in range(n):
            R += [mrf_line("chr1", "+-"[j & 1], [(base + 2 + 2 * j, base + 3 + 2 * j)])] * (1 + j % 3)
    return iso, R


def deep_case():
    """70 000 identical blocks of 100 000 bases over a clean intron: a depth above 2^16, a depth_sum of 7e9"""
    iso = [interval_line("deep.a", "chr1", "+", [(100, 200), (100200, 100300)])]
    return iso, [mrf_line("chr1", "+", [(200, 100200)])] * 70000


def grid_case(n_chroms=20, genes=35, exons=101, seed=7):
    """(isoform lines, mrf lines): n_chroms * genes * (exons - 1) introns (70 000) of 1 .. 9 bases between exons of 6, some 150
    blocks a chromosome over them"""
    rng = random.Random(seed)
    iso, R = [], []
    for c in range(n_chroms):
        chrom = "c%02d" % c
        for g in range(genes):
            at, ex = 2000 * g + 10, []
            for j in range(exons):
                ex.append((at, at + 6))
                at += 6 + 1 + (j + g + c) % 9
            iso.append(interval_line("%sg%d.a" % (chrom, g), chrom, "+-"[g & 1], ex))
        for _ in range(150):
            s = rng.randrange(0, 2000 * genes)
            R.append(mrf_line(chrom, "+-"[s & 1], [(s, s + 5 + rng.randrange(60))]))
    return iso, R


def chromosome_case():
    """(isoform lines, mrf lines): chr2 ahead of chr10 in the dictionary; chrA and chrB neighbours in it, chrA's last row ending at
    500 where chrB's first intron begins; chr9 without reads; reads on chrU, which the annotation does not name; negative
    coordinates and an intron across 0"""
    il, m = interval_line, mrf_line
    iso = [il("g2.a", "chr2", "+", [(100, 200), (300, 400)]),
           il("g10.a", "chr10", "-", [(100, 200), (300, 400)]),
           il("g1.a", "chr1", "+", [(-600, -500), (-400, -300), (100, 200)]),                 # introns (-500, -400) and (-300, 100)
           il("gA.a", "chrA", "+", [(100, 200), (450, 600)]),
           il("gB.a", "chrB", "+", [(400, 500), (600, 700)]),
           il("g9.a", "chr9", "+", [(100, 200), (300, 400)])]
    R = [m("chr2", "+", [(150, 260)]), m("chr2", "-", [(250, 350)]), m("chr10", "+", [(190, 310)]), m("chr10", "+", [(150, 200), (300, 350)]),
         m("chr1", "+", [(-450, -380)]), m("chr1", "-", [(-20, 30)]), m("chr1", "-", [(-350, -300), (100, 150)]), m("chr1", "+", [(-10, 5)]),
         m("chrA", "+", [(300, 500)]), m("chrA", "-", [(450, 500)]),                            # chrA's last row ends at 500 ...
         m("chrB", "+", [(520, 580)]),                                                        # ... chrB's intron (500, 600) has its own row only
         m("chrU", "+", [(100, 400)]), m("chrU", "+", [(150, 200), (300, 350)])]
    return iso, R


def shuffled(lines, seed=3):
    out = list(lines)
    random.Random(seed).shuffle(out)
    return out
