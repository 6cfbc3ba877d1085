"""The sites table's definition (include/lesseq_hip.h, lsq_ss_*) restated in plain Python from the MRF text and the
interval file themselves -- no parser of the library is involved -- and the hand-built inputs the sites tests share.  The junction
rows, the introns and the chromosome rule are junction_ref's; `through` tests every block against every boundary of its
chromosome (numpy compares all pairs: no search, no walk).  For SAM and BAM inputs the reference runs on L.sam_to_mrf /
L.bam_to_mrf, the formats' defined equivalents."""
import random

import numpy as np

import junction_ref as J
from junction_ref import LIM, interval_line, mrf_line, write_case  # noqa: F401

REPORT = ("reads", "blocks", "occurrences", "dropped_overhang", "no_chromosome", "boundaries", "through", "unsupported")


# ----------------------------------------------------------------------------- the definition

def through_counts(boundaries, blocks, m):
    """{(chrom, p): blocks [s, e) of chrom with s + m <= p <= e - m}; boundaries {chrom: [p]}, blocks {chrom: [(s, e)]}"""
    out = {}
    for chrom, ps in boundaries.items():
        p = np.array(ps, dtype=np.int64)
        n = np.zeros(len(p), dtype=np.int64)
        bl = np.array(blocks.get(chrom, []), dtype=np.int64).reshape(-1, 2)
        step = max(1, 4000000 // max(1, len(p)))
        for at in range(0, len(bl), step):
            s, e = bl[at:at + step, 0:1], bl[at:at + step, 1:2]
            n += ((s + m <= p[None, :]) & (p[None, :] <= e - m)).sum(axis=0)
        for q, v in zip(ps, n):
            out[(chrom, q)] = int(v)
    return out


def table(interval_text, mrf_text, min_overhang=1):
    """(rows, report): rows [(chrom, start, end, ann, reads, left_spliced, left_through, right_spliced, right_through)] in table
    order; report the eight numbers"""
    jrows, report = J.table(interval_text, mrf_text, min_overhang)
    known = set(J.chromosomes(interval_text))
    rows = {(c.encode(), s, e): [a, r] for c, s, e, a, r, _, _, _ in jrows}
    for (c, s, e), a in J.introns(interval_text).items():
        if s > -LIM and e < LIM:
            rows.setdefault((c.encode(), s, e), [a, 0])
    boundaries = {}
    for c, s, e in rows:
        boundaries.setdefault(c, set()).update((s, e))
    boundaries = {c: sorted(v) for c, v in boundaries.items()}
    blocks = {}
    for read in J.mrf_reads(mrf_text):
        for c, _, s, e in read:
            if c in known and e > s and not (s <= -LIM or e >= LIM or s >= LIM or e <= -LIM):
                blocks.setdefault(c.encode(), []).append((s, e))
    thr = through_counts(boundaries, blocks, max(min_overhang, 1))
    as_left, as_right = {}, {}
    for (c, s, e), (_, r) in rows.items():
        as_left[(c, s)] = as_left.get((c, s), 0) + r
        as_right[(c, e)] = as_right.get((c, e), 0) + r
    out = [(c.decode(), s, e, a, r, as_left[(c, s)], thr[(c, s)], as_right[(c, e)], thr[(c, e)]) for (c, s, e), (a, r) in sorted(rows.items())]
    report = dict(report, boundaries=sum(len(v) for v in boundaries.values()), through=sum(thr.values()), unsupported=sum(1 for r in out if r[4] == 0))
    return out, report


_tables = {}


def table_once(key, interval_text, mrf_text, min_overhang=1):
    """table() of an input that several tests share (and of a file whose order does not matter), computed once a session"""
    if (key, min_overhang) not in _tables:
        _tables[(key, min_overhang)] = table(interval_text, mrf_text, min_overhang)
    return _tables[(key, min_overhang)]


def text(rows, min_reads=0, novel_only=False, ratios=False):
    def ratio(a, b):
        return "\tNA" if b == 0 else "\t%.6f" % (a / b)
    out = []
    for c, s, e, a, r, ls, lt, rs, rt in rows:
        if r < min_reads or (novel_only and a != "."):
            continue
        line = "%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d" % (c, s + 1, e, a, r, ls, lt, rs, rt)
        if ratios:
            line += ratio(r, ls) + ratio(r, rs) + ratio(ls, ls + lt) + ratio(rs, rs + rt)
        out.append(line + "\n")
    return "".join(out)


# ----------------------------------------------------------------------------- inputs

OVERHANGS = (1, 2, 10, 50)


def boundary_case():
    """(isoform lines, mrf lines): one-block reads placed around boundaries for every m of OVERHANGS -- s + m == p, p == e - m, each
    off by one base either way, lengths 2m-1, 2m, 2m+1, an empty block, a block on no chromosome, the same on a second chromosome,
    a chromosome with no boundary, negative coordinates, boundaries and blocks at the ends of the coordinate range"""
    iso = [interval_line("a.1", "chr1", "+", [(100, 1000), (2000, 3000)]),
           interval_line("b.1", "chr2", "-", [(100, 1000), (2000, 3000)]),
           interval_line("n.1", "chr1", "+", [(-3000, -2000), (-1000, -500)]),
           interval_line("lo.1", "chr1", "+", [(-LIM - 100, -LIM + 1), (-LIM + 500, -LIM + 600)]),
           interval_line("hi.1", "chr1", "+", [(LIM - 600, LIM - 500), (LIM - 1, LIM + 100)]),
           interval_line("out.1", "chr1", "+", [(-LIM - 900, -LIM - 800), (-LIM + 700, -LIM + 800)]),      # an intron that begins outside the range: no row
           interval_line("mono.1", "chrM", "+", [(10, 500)])]
    m_ = mrf_line
    R = []
    for m in OVERHANGS:
        for chrom, p in (("chr1", 1000), ("chr1", 2000), ("chr2", 1000), ("chr2", 2000), ("chr1", -2000), ("chr1", -1000), ("chr1", -LIM + 500), ("chr1", LIM - 500)):
            for s, e in ((p - m, p + m), (p - m, p + m + 5), (p - m - 5, p + m), (p - m + 1, p + m + 5), (p - m - 1, p + m + 5), (p - m - 5, p + m - 1), (p - m - 5, p + m + 1),
                         (p - m, p + m - 1), (p - m + 1, p + m), (p - m, p + m + 1), (p - m - 1, p + m), (p, p)):
                R.append(m_(chrom, "+", [(s, e)]))
            R.append(m_("chrU", "+", [(p - m - 5, p + m + 5)]))
        # the ends of the range: the outermost blocks that have a chromosome, and one base further, which have none
        R += [m_("chr1", "+", [(-LIM + 1, -LIM + 1 + 2 * m)]), m_("chr1", "+", [(-LIM + 1, -LIM + 501 + m)]), m_("chr1", "+", [(-LIM, -LIM + 501 + m)]),
              m_("chr1", "-", [(LIM - 1 - 2 * m, LIM - 1)]), m_("chr1", "-", [(LIM - 500 - m, LIM - 1)]), m_("chr1", "-", [(LIM - 500 - m, LIM)])]
    R += [m_("chrM", "+", [(10, 400)]), m_("chr1", "+", [(0, 100000)]), m_("chr1", "+", [(-LIM + 1, LIM - 1)])]
    return iso, R


def rows_case():
    """(isoform lines, mrf lines, the table by hand at min_overhang 1, its report)"""
    iso = [interval_line("gA.a", "chr1", "+", [(100, 200), (300, 400), (500, 600)]),
           interval_line("gA.b", "chr1", "+", [(100, 200), (500, 600)]),                  # shares its start with gA.a's first intron, its end with the second
           interval_line("gB.a", "chr1", "+", [(1000, 1100), (1200, 1300)]),              # no spliced read, unspliced ones across both ends
           interval_line("gC.a", "chr1", "+", [(2000, 2100), (2200, 2300)]),              # nothing touches it
           interval_line("gD.a", "chr1", "-", [(3000, 3100), (3200, 3400)]),              # 3200 ends this intron ...
           interval_line("gD.b", "chr1", "-", [(3000, 3200), (3300, 3400)])]              # ... and begins this one
    m = mrf_line
    R = ([m("chr1", "+", [(150, 200), (300, 350)])] * 3 + [m("chr1", "+", [(150, 200), (500, 550)])] * 2 + [m("chr1", "+", [(350, 400), (500, 550)])] * 4 +
         [m("chr1", "+", [(150, 200), (450, 550)])] +                                     # novel; its second block runs through 500
         [m("chr1", "+", [(180, 320)])] * 5 + [m("chr1", "+", [(390, 460)])] * 2 +
         [m("chr1", "+", [(1050, 1150)])] * 3 + [m("chr1", "+", [(1150, 1250)])] * 2 + [m("chr1", "+", [(1050, 1250)])] +
         [m("chr1", "-", [(3050, 3100), (3200, 3250)])] * 2 + [m("chr1", "-", [(3150, 3200), (3300, 3350)])] * 3 + [m("chr1", "-", [(3190, 3210)])] * 4)
    rows = [("chr1", 200, 300, "+", 3, 6, 5, 3, 5),
            ("chr1", 200, 450, ".", 1, 6, 5, 1, 2),
            ("chr1", 200, 500, "+", 2, 6, 5, 6, 1),
            ("chr1", 400, 500, "+", 4, 4, 2, 6, 1),
            ("chr1", 1100, 1200, "+", 0, 0, 4, 0, 3),
            ("chr1", 2100, 2200, "+", 0, 0, 0, 0, 0),
            ("chr1", 3100, 3200, "-", 2, 2, 0, 2, 4),
            ("chr1", 3200, 3300, "-", 3, 3, 4, 3, 0)]
    report = dict(zip(REPORT, (32, 47, 15, 0, 0, 12, 26, 2)))
    return iso, R, rows, report


def walk_lines():
    """reads for the walk over junction_ref.annotation_lines(): one block over all boundaries of the 70-exon gene, one behind the
    chromosome's last boundary, one ahead of its first (the 40-block read is junction_ref.extract_lines()')"""
    return [mrf_line("chr3", "+", [(99000, 125000)]), mrf_line("chr3", "+", [(130000, 130100)]), mrf_line("chr3", "+", [(50, 150)]),
            mrf_line("chr3", "-", [(100050, 100150), (120650, 120750)])]


def many_boundaries(n_chroms, genes=10, exons=101):
    """isoform lines with genes * (exons - 1) introns a chromosome, no boundary shared: 2 * genes * (exons - 1) boundaries each;
    returns (lines, [(chrom, p)] in index order)"""
    iso, where = [], []
    for c in range(n_chroms):
        for g in range(genes):
            base = 1000000 * g
            iso.append(interval_line("c%02dg%d.a" % (c, g), "c%02d" % c, "+-"[g & 1], [(base + 1000 * j, base + 1000 * j + 500) for j in range(exons)]))
            for j in range(exons - 1):
                where += [("c%02d" % c, base + 1000 * j + 500), ("c%02d" % c, base + 1000 * (j + 1))]
    return iso, where


def through_line(chrom, p, k=0):
    return mrf_line(chrom, "+-"[k & 1], [(p - 20 - k % 7, p + 20 + k % 5)])


def counter_case(kind, slots=0):
    """(isoform lines, mrf lines) for the combining add and the counters"""
    if kind == "one_boundary":
        return [interval_line("g1.a", "chr1", "+", [(100, 200), (300, 400)])], [through_line("chr1", 200, k) for k in range(70000)]
    if kind == "all_distinct":              # 35 chromosomes of 2 000 boundaries, each hit once
        iso, where = many_boundaries(35)
        assert len(where) == 70000
        return iso, [through_line(c, p, k) for k, (c, p) in enumerate(where)]
    if kind == "run_lengths":               # runs of 1, 2, 63, 64 and 65 equal ids in file order
        iso, where = many_boundaries(1, genes=1)
        lines = []
        for j, (c, p) in enumerate(where):
            lines += [through_line(c, p, k) for k in range((1, 2, 63, 64, 65)[j % 5])]
        return iso, lines
    if kind == "slots":                     # `slots` distinct boundaries on one chromosome, each hit by three blocks, round after round
        n_introns, odd = (slots - 3) // 2 if slots & 1 else slots // 2, slots & 1
        iso = [interval_line("s%04d.a" % j, "chr1", "+", [(1000 * j, 1000 * j + 300), (1000 * j + 600, 1000 * j + 900)]) for j in range(n_introns)]
        where = [p for j in range(n_introns) for p in (1000 * j + 300, 1000 * j + 600)]
        if odd:                             # two introns with one start: three boundaries
            iso += [interval_line("odd.a", "chr1", "+", [(-5000, -4700), (-4400, -4000)]), interval_line("odd.b", "chr1", "+", [(-5000, -4700), (-4200, -4000)])]
            where += [-4700, -4400, -4200]
        assert len(set(where)) == slots
        return iso, [through_line("chr1", p, k) for k in range(3) for p in where]
    raise ValueError(kind)


def shuffled(lines, seed=3):
    out = list(lines)
    random.Random(seed).shuffle(out)
    return out
