"""The junction table's definition (include/lesseq_hip.h, lsq_jn_*) restated in plain Python from the MRF text and
the interval file themselves -- no parser of the library is involved -- and the hand-built inputs the junction tests share.  For
SAM and BAM inputs the reference runs on L.sam_to_mrf / L.bam_to_mrf, the formats' defined equivalents."""
import random

from golden_inputs import interval_line, mrf_line

LIM = 1 << 30


# ----------------------------------------------------------------------------- the definition

def isoforms(interval_text):
    """[(chrom, strand, [(start, end)] the first exonCount exons)] of an LH_GENE_TXT text, every line"""
    out = []
    for line in interval_text.split("\n"):
        t = line.split()
        if len(t) < 8:
            continue
        n = int(t[5])
        starts = [int(x) for x in t[6].split(",") if x]
        ends = [int(x) for x in t[7].split(",") if x]
        out.append((t[1], t[2], list(zip(starts, ends))[:n]))
    return out


def chromosomes(interval_text):
    """the dictionary: distinct chromosome strings, first seen first"""
    names = []
    for chrom, _, _ in isoforms(interval_text):
        if chrom not in names:
            names.append(chrom)
    return names


def introns(interval_text):
    """{(chrom, start, end): ann}"""
    seen = {}
    for chrom, strand, exons in isoforms(interval_text):
        iv = sorted((s, e) for s, e in exons if e > s)
        merged = []
        for s, e in iv:
            if merged and s <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], e)
            else:
                merged.append([s, e])
        for a, b in zip(merged, merged[1:]):
            seen.setdefault((chrom, a[1], b[0]), set()).add(strand)
    return {k: (next(iter(v)) if len(v) == 1 and next(iter(v)) in ("+", "-") else "*") for k, v in seen.items()}


def mrf_reads(mrf_text):
    """[[(chrom, strand, start0, end)]] per read of an MRF_SINGLE text: the header line skipped, '#' and "AlignmentBlocks" lines no
    read, an unterminated last line never seen"""
    lines = mrf_text.split("\n")[1:-1]
    reads = []
    for ln in lines:
        if ln.startswith("#") or ln == "AlignmentBlocks":
            continue
        blocks = []
        for b in ln.split(","):
            f = b.split(":")
            blocks.append((f[0], f[1], int(f[2]) - 1, int(f[3])))
        reads.append(blocks)
    return reads


def table(interval_text, mrf_text, min_overhang=1):
    """(rows, report): rows [(chrom, start, end, ann, reads, plus, minus, max_overhang)] in table order; report the five numbers"""
    known = set(chromosomes(interval_text))
    ann = introns(interval_text)
    reads = mrf_reads(mrf_text)
    acc = {}
    n_blocks = n_occ = dropped = nochrom = 0

    def chrom_of(b):
        c, _, s, e = b
        if c not in known or s <= -LIM or e >= LIM or s >= LIM or e <= -LIM:
            return None
        return c
    for blocks in reads:
        n_blocks += len(blocks)
        for a, b in zip(blocks, blocks[1:]):
            ca, cb = chrom_of(a), chrom_of(b)
            if ca is None or cb is None:
                nochrom += 1
                continue
            if ca != cb or b[2] <= a[3]:
                continue
            ov = min(a[3] - a[2], b[3] - b[2])
            if ov < min_overhang:
                dropped += 1
                continue
            n_occ += 1
            r = acc.setdefault((ca.encode(), a[3], b[2]), [0, 0, 0, 0])
            r[0] += 1
            r[1] += a[1] == "+"
            r[2] += a[1] == "-"
            r[3] = max(r[3], ov)
    rows = [(k[0].decode(), k[1], k[2], ann.get((k[0].decode(), k[1], k[2]), "."), v[0], v[1], v[2], v[3]) for k, v in sorted(acc.items())]
    return rows, {"reads": len(reads), "blocks": n_blocks, "occurrences": n_occ, "dropped_overhang": dropped, "no_chromosome": nochrom}


def text(rows, min_reads=0, novel_only=False):
    return "".join("%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (c, s + 1, e, a, r, p, m, o) for c, s, e, a, r, p, m, o in rows
                   if r >= min_reads and (not novel_only or a == "."))


# ----------------------------------------------------------------------------- inputs

def write_case(d, stem, isoform_lines, mrf_lines, header="AlignmentBlocks\n"):
    """stem.interval, stem.map (a gene per isoform line unless the line's name holds a '.': then the part before it), stem.mrf;
    returns (interval text, mrf text, paths)"""
    interval = "".join(isoform_lines)
    names = [ln.split("\t")[0] for ln in isoform_lines]
    gmap = "".join("%s\t%s\n" % (n.split(".")[0], n) for n in names)
    mrf = header + "".join(mrf_lines)
    paths = {}
    for ext, body in (("interval", interval), ("map", gmap), ("mrf", mrf)):
        paths[ext] = "%s/%s.%s" % (d, stem, ext)
        with open(paths[ext], "w") as f:
            f.write(body)
    return interval, mrf, paths


def annotation_lines():
    """the annotate cases: touching, overlapping, empty and unsorted exons, one intron on both strands, a strand that is neither,
    the same coordinates on another chromosome, negative coordinates, a gene of 70 exons and 20 isoforms"""
    L = [interval_line("neg.a", "chr1", "+", [(-500, -400), (-300, -200)]),                     # the intron table's first entry
         interval_line("g1.a", "chr1", "+", [(100, 200), (300, 400), (500, 600)]),
         interval_line("g1.b", "chr1", "+", [(100, 200), (500, 600)]),
         interval_line("touch.a", "chr1", "+", [(1000, 1100), (1100, 1200), (1300, 1400)]),
         interval_line("over.a", "chr1", "+", [(2000, 2100), (2050, 2200), (2300, 2400)]),
         interval_line("empty.a", "chr1", "+", [(3000, 3100), (3150, 3150), (3200, 3300)]),
         interval_line("unsorted.a", "chr1", "-", [(4300, 4400), (4000, 4100)]),
         interval_line("both.a", "chr1", "+", [(5000, 5100), (5200, 5300)]),
         interval_line("both.b", "chr1", "-", [(5000, 5100), (5200, 5300)]),
         interval_line("dot.a", "chr1", ".", [(6000, 6100), (6200, 6300)]),
         interval_line("short.a", "chr1", "+", [(7000, 7100), (7200, 7300), (7400, 7500)], exon_count=2),      # the third exon is not the line's
         interval_line("g2.a", "chr2", "-", [(100, 200), (300, 400)]),
         interval_line("mono.a", "chrM", "+", [(10, 500)])]
    exons = [(100000 + 300 * k, 100000 + 300 * k + 100) for k in range(70)]
    for j in range(20):
        L.append(interval_line("big.%02d" % j, "chr3", "+", [x for k, x in enumerate(exons) if k == 0 or k == 69 or (k + j) % 3]))
    return L


def extract_lines():
    """the extract and annotate reads, by what they test; the last line is a spliced read"""
    m = mrf_line
    R = [m("chr1", "+", [(150, 200)]),                                        # one block
         m("chr1", "+", [(150, 200), (300, 350)]),                            # a known junction
         m("chr1", "-", [(160, 200), (300, 330)]),
         m("chr1", ".", [(170, 200), (300, 380)]),
         m("chr1", "+", [(150, 200), (200, 250)]),                            # gap 0
         m("chr1", "+", [(150, 200), (180, 250)]),                            # overlapping
         m("chr1", "+", [(300, 350), (150, 200)]),                            # descending
         m("chr1", "+", [(150, 200), (301, 350)]),                            # off by one base at either end
         m("chr1", "+", [(150, 199), (300, 350)]),
         m("chr1", "+", [(150, 201), (300, 350)]),
         m("chr1", "+", [(150, 200), (299, 350)]),
         m("chr2", "+", [(150, 200), (300, 350)]),                            # the same coordinates on another chromosome
         m("chrM", "+", [(20, 60), (80, 120)]),                               # a chromosome without any intron
         m("chr1", "+", [(150, 200), (500, 550)]),                            # g1.b's intron
         m("chr1", "+", [(150, 200), (300, 400), (500, 550)]),                # three blocks: two junctions
         m("chr1", "+", [(1050, 1100), (1100, 1200), (1300, 1350)]),          # touching exons: one gap, one junction
         m("chr1", "+", [(1150, 1200), (1300, 1350)]),
         m("chr1", "+", [(2150, 2200), (2300, 2350)]),                        # overlapping exons
         m("chr1", "+", [(2050, 2100), (2300, 2350)]),                        # ... the first exon's end is no intron start
         m("chr1", "+", [(3050, 3100), (3200, 3250)]),                        # an empty exon inside the intron
         m("chr1", "+", [(3050, 3100), (3150, 3250)]),
         m("chr1", "-", [(4050, 4100), (4300, 4350)]),                        # unsorted exon list
         m("chr1", "+", [(5050, 5100), (5200, 5250)]),                        # both strands: '*'
         m("chr1", "+", [(6050, 6100), (6200, 6250)]),                        # a strand that is neither: '*'
         m("chr1", "+", [(7050, 7100), (7200, 7250)]),                        # exonCount 2 of 3 listed
         m("chr1", "+", [(7250, 7300), (7400, 7450)]),
         m("chr1", "+", [(-450, -400), (-300, -250)]),                        # a negative start: the intron table's first entry
         m("chr1", "+", [(-50, -10), (20, 60)]),                              # a negative against a positive start
         m("chr1", "+", [(-LIM + 1, -LIM + 30), (-LIM + 50, -LIM + 90)]),     # the coordinate range's ends
         m("chr1", "+", [(LIM - 90, LIM - 50), (LIM - 30, LIM - 1)]),
         m("chr1", "+", [(LIM - 90, LIM - 50), (LIM - 30, LIM)]),             # ... and one past them: no chromosome (second block)
         m("chr1", "+", [(-LIM, -LIM + 30), (-LIM + 50, -LIM + 90)]),         # (first block)
         m("chrU", "+", [(150, 200), (300, 350)]),                            # a chromosome the annotation does not name
         m("chr1", "+", [(150, 200)]).rstrip("\n") + "," + m("chrU", "+", [(300, 350)]),      # second block without a chromosome
         m("chrU", "+", [(150, 200)]).rstrip("\n") + "," + m("chr1", "+", [(300, 350)]),      # first block
         m("chr1", "+", [(150, 200)]).rstrip("\n") + "," + m("chr2", "+", [(300, 350)]),      # a chromosome change inside a read
         m("chr3", "+", [(100000, 100100), (120700, 120750)]),                # the 70-exon gene: first exon to last, no isoform's intron
         m("chr3", "+", [(100000 + 300 * k, 100000 + 300 * k + 100) for k in range(40)]),      # a read of 40 blocks
         m("chr3", "+", [(120700 - 300 + 50, 120700 - 300 + 100), (120700, 120750)]),          # the intron table's last entry
         "#\n",
         m("chr1", "+", [(190, 200), (300, 350)]),                            # overhang 10 ...
         m("chr1", "-", [(150, 200), (300, 309)]),                            # ... 9
         m("chr1", "+", [(150, 200), (300, 311)]),                            # ... 11
         m("chr1", "+", [(200, 200), (300, 350)]),                            # an empty flank block
         m("chr2", "-", [(150, 200), (300, 350)])]                            # a spliced read on the last line
    return R


def sort_case(n_occ, shuffled, seed=5):
    """(isoform lines, mrf lines): n_occ occurrences whose keys differ in one field only -- chromosome indices 0, 255, 256 and 300,
    start and end at bit 0 and at bit 30 (a negative against a positive coordinate flips bit 30 of the biased field) -- then
    distinct junctions up to n_occ; sorted by key or shuffled"""
    iso = [interval_line("c%03d.a" % c, "c%03d" % c, "+", [(100, 200), (300, 400)]) for c in range(301)]
    keys = []
    for c in (0, 255, 256, 300):
        keys.append((c, 200, 300))
    keys += [(0, 201, 300), (0, 200, 301), (0, -200, 300), (0, -200, -100), (0, -201, -100), (0, -200, -99), (0, 200 + (1 << 29), 300 + (1 << 29))]
    k = 0
    while len(keys) < n_occ:
        keys.append((k % 7, 1000 + 3 * (k // 7), 2000 + 5 * (k // 7) + k % 3))
        k += 1
    keys = sorted(keys[:n_occ])
    if shuffled:
        random.Random(seed).shuffle(keys)
    return iso, [mrf_line("c%03d" % c, "+-"[(s + e) & 1], [(s - 40, s), (e, e + 30)]) for c, s, e in keys]


def reduce_case(kind):
    """(isoform lines, mrf lines) for the reduce phase"""
    iso = [interval_line("g1.a", "chr1", "+", [(100, 200), (300, 400)])]
    rng = random.Random(11)

    def occ(j, strand=None, ov=None):
        s = 1000 + 10 * j
        ov = ov or 20
        return mrf_line("chr1", strand or rng.choice("+-."), [(s - ov, s), (s + 500, s + 500 + 1000)])
    if kind == "one_junction":
        lines = [occ(0) for _ in range(70000)]
    elif kind == "all_distinct":
        lines = [occ(j) for j in range(70000)]
    elif kind == "run_lengths":
        lines, j = [], 0
        while len(lines) < 9000:
            for n in (1, 2, 63, 64, 65):
                lines += [occ(j) for _ in range(n)]
                j += 1
    elif kind == "tile_edge":
        # sorted order: junction 0 fills all but the last place of the sort's first tile, junction 1 begins on it
        from lesseq_amd.junctions import SORT_TILE
        lines = [occ(0) for _ in range(SORT_TILE - 1)] + [occ(1) for _ in range(70)]
        rng.shuffle(lines)
    elif kind == "max_position":
        lines = []
        for j, where in enumerate((0, 100, 199)):      # the largest overhang on the first, a middle and the last occurrence of a run
            lines += [occ(j, ov=900 if q == where else 20 + q % 7) for q in range(200)]
    else:
        raise ValueError(kind)
    return iso, lines
