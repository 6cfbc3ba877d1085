"""The coverage tables' definition (include/lesseq_hip.h, lsq_cov_*) restated from the MRF text and the interval file
themselves with one dense numpy depth array per chromosome -- no parser and no sort of the library is involved -- and the
hand-built inputs the coverage tests share.  The dense arrays span a chromosome's counted blocks, so the cases keep those within
a few hundred thousand bases of each other."""
import random

import numpy as np

from golden_inputs import interval_line, mrf_line
from junction_ref import isoforms, chromosomes, mrf_reads, write_case  # noqa: F401  (the texts' fields; no definition)

LIM = 1 << 30
REPORT = ("reads", "blocks", "counted", "no_chromosome", "empty", "other_strand", "bases")


# ----------------------------------------------------------------------------- the definition

def depth_arrays(interval_text, mrf_text, strand=None):
    """({chrom: (lo, depth int64[hi - lo])} over the span of the chromosome's counted blocks, report)"""
    known = set(chromosomes(interval_text))
    reads = mrf_reads(mrf_text)
    rep = dict.fromkeys(REPORT, 0)
    rep["reads"] = len(reads)
    blocks = {}
    for read in reads:
        for c, st, s, e in read:
            rep["blocks"] += 1
            if c not in known or not (-LIM < s < LIM and -LIM < e < LIM):
                rep["no_chromosome"] += 1
            elif e <= s:
                rep["empty"] += 1
            elif strand is not None and st != strand:
                rep["other_strand"] += 1
            else:
                rep["counted"] += 1
                rep["bases"] += e - s
                blocks.setdefault(c, []).append((s, e))
    out = {}
    for c, bl in blocks.items():
        s = np.array([b[0] for b in bl], np.int64)
        e = np.array([b[1] for b in bl], np.int64)
        lo, hi = int(s.min()), int(e.max())
        step = np.zeros(hi - lo + 1, np.int64)       # +1 on a block's first base, -1 behind its last: the running sum is the depth
        np.add.at(step, s - lo, 1)
        np.add.at(step, e - lo, -1)
        out[c] = (lo, np.cumsum(step)[:-1])
    return out, rep


def rows_of(arrays):
    """[(chrom, start, end, depth)]: the maximal stretches of one depth > 0, by chromosome name (bytewise), then start"""
    rows = []
    for c in sorted(arrays, key=lambda n: n.encode()):
        lo, depth = arrays[c]
        x = 0
        while x < len(depth):
            y = x
            while y < len(depth) and depth[y] == depth[x]:
                y += 1
            if depth[x] > 0:
                rows.append((c, lo + x, lo + y, int(depth[x])))
            x = y
    return rows


def fast_rows_of(arrays):
    """the same through numpy (the large cases); test_coverage_host checks the two against each other"""
    rows = []
    for c in sorted(arrays, key=lambda n: n.encode()):
        lo, depth = arrays[c]
        cut = np.flatnonzero(np.diff(depth)) + 1
        starts = np.concatenate(([0], cut))
        ends = np.concatenate((cut, [len(depth)]))
        rows += [(c, lo + int(a), lo + int(b), int(depth[a])) for a, b in zip(starts, ends) if depth[a] > 0]
    return rows


def regions_of(interval_text, arrays, min_depth=1):
    """[(name, chrom, strand, bases, covered, depth_sum)] per isoform line, in file order"""
    out = []
    names = [ln.split()[0] for ln in interval_text.split("\n") if len(ln.split()) >= 8]
    for name, (chrom, strand, exons) in zip(names, isoforms(interval_text)):
        ex = [(s, e) for s, e in exons if e > s]
        bases = covered = depth_sum = 0
        if ex:
            lo, hi = min(s for s, _ in ex), max(e for _, e in ex)
            mask = np.zeros(hi - lo, bool)
            for s, e in ex:
                mask[s - lo:e - lo] = True
            bases = int(mask.sum())
            if chrom in arrays:
                dlo, depth = arrays[chrom]
                full = np.zeros(hi - lo, np.int64)           # the chromosome's depth over the line's span
                a, b = max(lo, dlo), min(hi, dlo + len(depth))
                if b > a:
                    full[a - lo:b - lo] = depth[a - dlo:b - dlo]
                covered = int((full[mask] >= min_depth).sum())
                depth_sum = int(full[mask].sum())
        out.append((name, chrom, strand, bases, covered, depth_sum))
    return out


def table(interval_text, mrf_text, strand=None, min_depth=1):
    """(rows, regions, report)"""
    arrays, rep = depth_arrays(interval_text, mrf_text, strand)
    return fast_rows_of(arrays), regions_of(interval_text, arrays, min_depth), rep


def text(rows, min_depth=0):
    return "".join("%s\t%d\t%d\t%d\n" % r for r in rows if r[3] >= min_depth)


def regions_text(regions):
    return "".join("%s\t%s\t%s\t%d\t%d\t%d\t%.4f\n" % (n, c, s, b, v, d, d / b if b else 0.0) for n, c, s, b, v, d in regions)


def conserved(rows, report):
    """the sum of (end - start) * depth over the rows is the counted blocks' summed length"""
    return sum((e - s) * d for _, s, e, d in rows) == report["bases"]


# ----------------------------------------------------------------------------- inputs

def definition_annotation():
    """chr2 ahead of chr10 (the dictionary's order is not the names'), chrA and chrB neighbours in the dictionary, a chromosome
    without reads"""
    return [interval_line("g2.a", "chr2", "+", [(100, 200), (300, 400)]),
            interval_line("g10.a", "chr10", "-", [(100, 400)]),
            interval_line("g1.a", "chr1", "+", [(100, 350), (1000, 1100), (2000, 2050)]),
            interval_line("g1.b", "chr1", "-", [(-600, -300), (3000, 3150), (4000, 4100)]),
            interval_line("gA.a", "chrA", "+", [(400, 500)]),
            interval_line("gB.a", "chrB", "+", [(500, 600)]),
            interval_line("g9.a", "chr9", "+", [(100, 200)])]


def definition_lines():
    m = mrf_line
    return [m("chr1", "+", [(100, 200)]), m("chr1", "-", [(120, 150)]),          # nested
            m("chr1", "+", [(180, 260)]),                                        # overlapping
            m("chr1", "-", [(260, 300)]), m("chr1", "+", [(300, 340)]),          # abutting at the same depth: no boundary at 300
            m("chr1", "+", [(1000, 1050)]), m("chr1", "+", [(1050, 1100)]),      # an abutting pair alone: one row
            m("chr1", "+", [(1200, 1250)]), m("chr1", "-", [(1250, 1300)]), m("chr1", ".", [(1220, 1250)]),      # abutting, another depth: a boundary
            ] + [m("chr1", "+-"[k % 2], [(2000, 2050)]) for k in range(5)] + [   # the same block five times
            m("chr1", "+", [(3000, 3050), (3100, 3150)]),                        # a spliced read
            m("chr1", "-", [(4000, 4060), (4040, 4100)]),                        # a read whose own blocks overlap
            m("chr1", "+", [(5000, 5000), (5010, 5020)]),                        # an empty block
            m("chr1", "+", [(5100, 5090), (5110, 5120)]),                        # a descending block
            m("chrU", "+", [(100, 200)]),                                        # a chromosome the annotation does not name
            m("chr1", "+", [(LIM - 30, LIM)]), m("chr1", "+", [(-LIM, -LIM + 30)]),      # beyond +-2^30
            m("chr1", "+", [(-500, -400)]), m("chr1", "-", [(-450, -380), (-20, 30)]),   # negative coordinates, and across 0
            m("chrA", "+", [(400, 500)]), m("chrA", "-", [(450, 500)]),          # chrA's last end is chrB's first start
            m("chrB", "+", [(500, 600)]), m("chrB", ".", [(500, 520)]),
            m("chr10", "+", [(100, 180)]), m("chr10", "-", [(150, 400)]),
            m("chr2", "-", [(150, 320)]), m("chr2", ".", [(100, 120), (300, 400)]),
            m("chr1", "+", [(9000, 9010)]).rstrip("\n") + "," + m("chr2", "+", [(9000, 9010)])]      # a read across two chromosomes


def count_case(b, shuffled, seed=3):
    """(isoform lines, mrf lines): b counted blocks over three chromosomes within a few thousand bases, every seventh read with two
    blocks; a few blocks that are not counted ride along; sorted by chromosome and start, or shuffled"""
    iso = [interval_line("k%d.a" % c, "c%d" % c, "+-"[c % 2], [(100, 900), (1500, 3000), (4000, 5200)]) for c in range(3)]
    iso.append(interval_line("k0.b", "c0", "+", [(0, 6000)]))
    blocks = [(i % 3, 100 + i * 37 % 5000, 20 + i % 50) for i in range(b)]
    blocks.sort()
    reads, i = [], 0
    while i < len(blocks):
        n = 2 if len(reads) % 7 == 6 and i + 1 < len(blocks) and blocks[i][0] == blocks[i + 1][0] else 1
        reads.append(blocks[i:i + n])
        i += n
    if shuffled:
        random.Random(seed).shuffle(reads)
    lines = [mrf_line("c%d" % r[0][0], "+-."[(r[0][1] + r[0][2]) % 3], [(s, s + n) for _, s, n in r]) for r in reads]
    return iso, lines + [mrf_line("cU", "+", [(100, 200)]), mrf_line("c1", "+", [(700, 700)])]


def shape_case(kind, tile=4096):
    """(isoform lines, mrf lines) for the reduce, scan and emit phases"""
    iso = [interval_line("s.a", "chr1", "+", [(0, 2000000)])]
    rng = random.Random(13)
    N = 70000

    def one(s, e):
        return mrf_line("chr1", rng.choice("+-."), [(s, e)])
    if kind == "identical":
        lines = [one(1000, 1100) for _ in range(N)]
    elif kind == "disjoint":
        lines = [one(20 * j, 20 * j + 10 + j % 7) for j in range(N)]
    elif kind == "chain":
        lines = [one(15 * j, 15 * j + 15) for j in range(N)]
    elif kind == "staircase":
        lines = [one(i, 300) for i in range(300)] + [one(1000, 1000 + i + 1) for i in range(300)]
    elif kind == "run_lengths":
        lines, j = [], 0
        while len(lines) < 4500:
            for n in (1, 2, 63, 64, 65):
                lines += [one(100 * j, 100 * j + 30 + n) for _ in range(n)]
                j += 1
    elif kind == "tile_edge":
        # sorted records: `tile` begins at 100 fill the sort's first tile to its last place
        lines = [one(100, 200) for _ in range(tile)] + [one(150, 300) for _ in range(70)]
    else:
        raise ValueError(kind)
    if kind != "chain":
        rng.shuffle(lines)
    return iso, lines


def regions_case():
    """(isoform lines, mrf lines): rows [100,150) 2, [150,200) 3, [200,250) 1, a gap, [400,500) 1 on chr1; lines whose exons lie in
    every way against them, a line without exon, and 4 200 more lines"""
    m = mrf_line
    lines = [m("chr1", "+", [(100, 200)]), m("chr1", "-", [(100, 200)]), m("chr1", "+", [(150, 250)]), m("chr1", "+", [(400, 500)])]
    iso = [interval_line("inside.a", "chr1", "+", [(110, 140)]),
           interval_line("on_edges.a", "chr1", "+", [(150, 200)]),
           interval_line("all_rows.a", "chr1", "-", [(100, 250)]),
           interval_line("across_gap.a", "chr1", "+", [(180, 450)]),
           interval_line("uncovered.a", "chr1", "+", [(600, 700)]),
           interval_line("between.a", "chr1", "+", [(250, 400)]),
           interval_line("no_reads.a", "chr9", "+", [(100, 200)]),
           interval_line("union.a", "chr1", "+", [(100, 180), (150, 220), (480, 520)]),
           interval_line("unsorted.a", "chr1", "-", [(440, 460), (90, 120)]),
           interval_line("no_exon.a", "chr1", "+", [(300, 300)]),
           interval_line("none_counted.a", "chr1", "+", [(100, 250)], exon_count=0)]
    rng = random.Random(17)
    for k in range(4200):
        s = rng.randrange(0, 650)
        iso.append(interval_line("m%04d.a" % k, "chr1" if k % 11 else "chr9", "+-"[k % 2], [(s, s + 1 + rng.randrange(120))] + ([(s + 200, s + 230)] if k % 3 == 0 else [])))
    return iso, lines


def deep_case():
    """70 000 blocks of 100 000 bases over one exon: a depth_sum of 7e9, past 32 bits"""
    iso = [interval_line("deep.a", "chr1", "+", [(0, 100000)]), interval_line("deep.b", "chr1", "+", [(50000, 150000)])]
    return iso, [mrf_line("chr1", "+", [(0, 100000)])] * 70000
