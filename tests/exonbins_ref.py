"""The exon-bin table's definition (include/lesseq_hip.h, lsq_xb_*) restated in plain Python from the interval, map
and MRF texts themselves -- no parser and no lookup structure of the library is involved: every read is tried against every bin of
its chromosome -- and the hand-built inputs the exonbins tests share."""
import random

import numpy as np

from golden_inputs import interval_line, mrf_line
from junction_ref import isoforms, chromosomes, mrf_reads, write_case  # noqa: F401  (the texts' fields; no definition)

LIM = 1 << 30
REPORT = ("reads", "blocks", "no_chromosome_or_empty", "no_gene", "several_genes", "bin_hits")


# ----------------------------------------------------------------------------- the definition

def genes_of(interval_text, map_text):
    """[(gene, chrom, strand, [(start, end)] bins ascending)] in gene order: the loader keeps the genes of the map in bytewise name
    order (the order of count's table); of two isoform lines of one name the later one is the name's"""
    names = [ln.split()[0] for ln in interval_text.split("\n") if len(ln.split()) >= 8]
    by_name = dict(zip(names, isoforms(interval_text)))
    groups = {}
    for ln in map_text.split("\n"):
        t = ln.split()
        if len(t) >= 2:
            groups.setdefault(t[0], []).append(by_name[t[1]])
    out = []
    for gene in sorted(groups, key=lambda n: n.encode()):
        lines = groups[gene]
        chroms = {c for c, _, _ in lines}
        if len(chroms) > 1:
            raise ValueError(gene)
        strands = {s for _, s, _ in lines}
        exons = [(s, e) for _, _, ex in lines for s, e in ex if e > s]
        cuts = sorted({x for se in exons for x in se})
        bins = [(a, b) for a, b in zip(cuts, cuts[1:]) if any(s <= a and b <= e for s, e in exons)]
        out.append((gene, chroms.pop(), strands.pop() if len(strands) == 1 else ".", bins))
    return out


def bin_rows(genes):
    """[(gene:k, chrom, strand, start, end)] in table order"""
    return [("%s:%d" % (g, k + 1), c, st, s, e) for g, c, st, bins in genes for k, (s, e) in enumerate(bins)]


def table(interval_text, map_text, mrf_text):
    """(rows [(gene, total, gene:k, reads)] in table order, report)"""
    known = set(chromosomes(interval_text))
    genes = genes_of(interval_text, map_text)
    reads = mrf_reads(mrf_text)
    n_reads = [[0] * len(bins) for _, _, _, bins in genes]
    total = [0] * len(genes)
    rep = dict.fromkeys(REPORT, 0)
    rep["reads"] = len(reads)
    for read in reads:
        rep["blocks"] += len(read)
        good = []
        for c, _, s, e in read:
            if c not in known or not (-LIM < s < LIM and -LIM < e < LIM) or e <= s:
                rep["no_chromosome_or_empty"] += 1
            else:
                good.append((c, s, e))
        hit_genes = 0
        for g, (_, gc, _, bins) in enumerate(genes):
            hit = [any(c == gc and s < be and e > bs for c, s, e in good) for bs, be in bins]
            for k, h in enumerate(hit):
                n_reads[g][k] += h
            rep["bin_hits"] += sum(hit)
            if any(hit):
                total[g] += 1
                hit_genes += 1
        rep["no_gene"] += hit_genes == 0
        rep["several_genes"] += hit_genes > 1
    rows = [(gene, total[g], "%s:%d" % (gene, k + 1), n_reads[g][k]) for g, (gene, _, _, bins) in enumerate(genes) for k in range(len(bins))]
    return rows, rep


def table_of_one_block_reads(interval_text, map_text, mrf_text):
    """the same for a file whose reads all have one block on a known chromosome: every bin against all reads at once (numpy);
    test_exonbins_host checks it against table()"""
    genes = genes_of(interval_text, map_text)
    reads = mrf_reads(mrf_text)
    assert all(len(r) == 1 for r in reads)
    cid = {c: i for i, c in enumerate(chromosomes(interval_text))}
    c = np.array([cid[r[0][0]] for r in reads], np.int64)
    s = np.array([r[0][2] for r in reads], np.int64)
    e = np.array([r[0][3] for r in reads], np.int64)
    assert (e > s).all()
    rows, n_genes_hit, hits = [], np.zeros(len(reads), np.int64), 0
    for gene, gc, _, bins in genes:
        any_bin = np.zeros(len(reads), bool)
        per_bin = []
        for bs, be in bins:
            h = (c == cid[gc]) & (s < be) & (e > bs)
            per_bin.append(int(h.sum()))
            any_bin |= h
        n_genes_hit += any_bin
        hits += sum(per_bin)
        rows += [(gene, int(any_bin.sum()), "%s:%d" % (gene, k + 1), n) for k, n in enumerate(per_bin)]
    rep = {"reads": len(reads), "blocks": len(reads), "no_chromosome_or_empty": 0, "no_gene": int((n_genes_hit == 0).sum()),
           "several_genes": int((n_genes_hit > 1).sum()), "bin_hits": hits}
    return rows, rep


def map_of(isoform_lines):
    """the map text write_case writes"""
    return "".join("%s\t%s\n" % (ln.split("\t")[0].split(".")[0], ln.split("\t")[0]) for ln in isoform_lines)


def text(rows):
    return "".join("%s\t%d\t%s\t%d\n" % r for r in rows)


def bins_texts(genes):
    """(interval text, map text) of --bins"""
    rows = bin_rows(genes)
    return ("".join("%s\t%s\t%s\t%d\t%d\t1\t%d\t%d\n" % (i, c, st, s, e, s, e) for i, c, st, s, e in rows),
            "".join("%s\t%s\n" % (i.rsplit(":", 1)[0], i) for i, _, _, _, _ in rows))


def report_line(rep, n_bins, n_genes):
    """what the executable logs"""
    return ("exonbins: %d read(s), %d block(s), %d without a chromosome of the annotation or empty; %d bin(s) of %d gene(s): %d read(s) on no gene, "
            "%d on more than one, %d bin hit(s)" % (rep["reads"], rep["blocks"], rep["no_chromosome_or_empty"], n_bins, n_genes, rep["no_gene"], rep["several_genes"], rep["bin_hits"]))


# ----------------------------------------------------------------------------- inputs

BIG = [(100000 + 300 * k, 100000 + 300 * k + 100) for k in range(70)]


def definition_annotation():
    """bin construction: exons that touch, overlap, nest, repeat, come unsorted, an empty exon, an exon beyond exonCount; negative
    coordinates; two genes whose boundaries interleave and the same two on another chromosome; a gene of 70 exons and 20 isoforms"""
    I = interval_line
    L = [I("mix.a", "chr1", "+", [(1000, 1100), (1100, 1200), (1300, 1500)]),                    # touching
         I("mix.b", "chr1", "+", [(1050, 1150), (1350, 1400), (1300, 1500)]),                    # overlapping; nested; a repeat
         I("mix.c", "chr1", "+", [(1700, 1800), (1600, 1650), (1620, 1620), (1900, 1950)], exon_count=3),      # unsorted; empty; the fourth is not the line's
         I("neg.a", "chr1", "-", [(-500, -400), (-300, -200)]),
         I("neg.b", "chr1", "-", [(-450, -350), (-300, -200), (-20, 30)]),
         I("ovA.a", "chr2", "+", [(100, 300), (500, 700)]),                                      # ovA and ovB interleave
         I("ovB.a", "chr2", "-", [(200, 400), (600, 800)]),
         I("ovB.b", "chr2", "+", [(250, 350)]),                                                  # its strands differ: '.'
         I("ovC.a", "chr3", "+", [(100, 300), (500, 700)]),                                      # the same coordinates elsewhere
         I("ovD.a", "chr3", "-", [(200, 400), (600, 800)]),
         I("Zlast.a", "chr1", "+", [(3000, 3100)]),                                              # byte order: 'Z' ahead of every lower-case name
         I("edge.a", "chr1", "+", [(LIM - 100, LIM + 50), (LIM + 100, LIM + 200)])]              # a bin across and a bin beyond the coordinate range
    for j in range(20):
        L.append(I("big.%02d" % j, "chr4", "+", [x for k, x in enumerate(BIG) if k == 0 or k == 69 or (k + j) % 3]))
    return L


def definition_lines():
    m = mrf_line
    R = [m("chr1", "+", [(950, 1000)]),                                       # ends exactly at a bin's start: no hit
         m("chr1", "+", [(1200, 1250)]),                                      # starts exactly at a bin's end: no hit
         m("chr1", "+", [(999, 1001)]),                                       # one base of overlap, either side
         m("chr1", "+", [(1199, 1201)]),
         m("chr1", "-", [(1049, 1051)]),                                      # one base in each of two bins
         m("chr1", "+", [(1010, 1020), (1030, 1040)]),                        # two blocks in one bin: once
         m("chr1", "+", [(1020, 1180)]),                                      # one block over four bins: the gene once
         m("chr1", "+", [(1150, 1350)]),                                      # ... across the gap between two exons
         m("chr1", "+", [(1350, 1450), (1010, 1060), (1040, 1120)]),          # descending, overlapping each other
         m("chr1", "+", [(1040, 1120), (1350, 1450), (1010, 1060), (1350, 1450)]),
         m("chr1", "+", [(1060, 1070), (1010, 1020), (1110, 1120)]),          # the gene's second bin first: the gene once
         m("chr1", "+", [(900, 5000)]),                                       # over mix and Zlast: two genes
         m("chr1", "+", [(1610, 1640)]),                                      # where the empty exon lies
         m("chr1", "+", [(1900, 1950)]),                                      # the exon that is not the line's
         m("chr1", "+", [(1010, 1010)]),                                      # an empty block alone ...
         m("chr1", "+", [(1010, 1010), (1020, 1030)]),                        # ... and ahead of a good one
         m("chr1", "+", [(1030, 1020), (3010, 3020)]),                        # a descending block
         m("chrU", "+", [(1010, 1020)]),                                      # a chromosome the annotation does not name
         m("chrU", "+", [(1010, 1020)]).rstrip("\n") + "," + m("chr1", "+", [(1020, 1030)]),
         m("chr1", "+", [(1020, 1030)]).rstrip("\n") + "," + m("chr2", "+", [(250, 260)]),       # a chromosome change inside a read: three genes
         m("chr2", "+", [(250, 280)]),                                        # two overlapping genes
         m("chr2", "-", [(150, 180)]),                                        # one of them
         m("chr2", "+", [(350, 450), (550, 650)]),
         m("chr2", "+", [(650, 750), (150, 250)]),
         m("chr3", "+", [(250, 280)]),                                        # the same coordinates on another chromosome
         m("chr3", "+", [(750, 790)]),
         m("chr1", "+", [(-460, -440)]),                                      # negative coordinates
         m("chr1", "+", [(-350, -300)]),                                      # ends at a bin's start, begins at another's end
         m("chr1", "+", [(-25, 25)]),
         m("chr1", "+", [(-LIM + 1, -LIM + 30)]),                             # the coordinate range's ends ...
         m("chr1", "+", [(LIM - 50, LIM - 1)]),                               # ... inside: the bin across the range's end
         m("chr1", "+", [(LIM - 50, LIM)]),                                   # ... and one past them: no chromosome
         m("chr4", "+", BIG[3:19]),                                           # a 16-block read
         m("chr4", "+", BIG[20:60][::-1]),                                    # 40 blocks, descending
         m("chr4", "+", [(100000, 121000)]),                                  # one block over all 70 bins
         m("chr4", "+", [(100100, 100300)]),                                  # between two bins
         "#\n",
         m("chr3", "-", [(100, 800)])]                                        # the last line
    return R


def overlap_case(n, seed=3):
    """(isoform lines, mrf lines): three genes whose bins overlap one another on chr1, n one-block reads over them; each of the
    last 64 reads lies in a different stretch"""
    iso = [interval_line("p.a", "chr1", "+", [(100 * k, 100 * k + 60) for k in range(40)]),
           interval_line("q.a", "chr1", "-", [(100 * k + 30, 100 * k + 130) for k in range(0, 40, 2)]),
           interval_line("r.a", "chr1", "+", [(0, 4000)])]
    rng = random.Random(seed)
    lines = []
    for _ in range(n):
        s = rng.randrange(-50, 4100)
        lines.append(mrf_line("chr1", "+", [(s, s + rng.choice((1, 10, 50, 75, 300)))]))
    return iso, lines


def random_case(seed=17, n_genes=40, n_reads=5000):
    """(isoform lines, read tuples [(chrom, minus, blocks)]): about 400 bins in 40 genes on three chromosomes, neighbours overlapping;
    reads of one to five ascending blocks (what a CIGAR can say), a few on no gene or on an unnamed chromosome"""
    rng = random.Random(seed)
    iso, spans = [], []
    for g in range(n_genes):
        chrom = "chr%d" % (1 + g % 3)
        lo = 1000 + 900 * (g // 3) + rng.randrange(200)
        exons, x = [], lo
        for _ in range(rng.randrange(5, 10)):
            w = rng.randrange(30, 150)
            exons.append((x, x + w))
            x += w + rng.randrange(0, 120)
        spans.append((chrom, lo, x))
        for j in range(rng.randrange(1, 4)):
            ex = [(s + rng.choice((0, 0, 10)), e - rng.choice((0, 0, 10))) for s, e in exons if rng.random() < 0.8] or exons[:1]
            iso.append(interval_line("g%02d.%d" % (g, j), chrom, "+-"[g & 1], ex))
    reads = []
    for _ in range(n_reads):
        chrom, lo, hi = spans[rng.randrange(n_genes)]
        if rng.random() < 0.03:
            chrom = "chrU"
        blocks, x = [], rng.randrange(lo - 100, hi + 50)
        for _ in range(rng.choice((1, 1, 1, 2, 2, 3, 5))):
            w = rng.randrange(5, 90)
            blocks.append((x, x + w))
            x += w + rng.randrange(1, 200)
        reads.append((chrom, rng.random() < 0.5, blocks))
    return iso, reads


def hot_case(shuffled, n_hot=200000, n_rest=1000, seed=23):
    """(isoform lines, mrf lines): n_hot one-block reads inside one bin beside n_rest spread over the rest, in coordinate order or shuffled"""
    iso = [interval_line("cold%d.a" % g, "chr1", "+", [(1000 * g + 100 * k, 1000 * g + 100 * k + 70) for k in range(6)]) for g in range(5)]
    iso.insert(2, interval_line("hot.a", "chr1", "+", [(20000, 20100), (20200, 20400), (20500, 20600)]))
    rng = random.Random(seed)
    reads = [(20200 + rng.randrange(150), 50) for _ in range(n_hot)] + [(rng.randrange(-50, 5000), rng.choice((20, 50, 120))) for _ in range(n_rest)]
    if shuffled:
        rng.shuffle(reads)
    else:
        reads.sort()
    return iso, ["chr1:+:%d:%d:1:%d\n" % (s + 1, s + w, w) for s, w in reads]


def wave_case(kind):
    """(isoform lines, mrf lines): 64 reads a wave -- `distinct`: each of a wave's reads in a bin of its own; `alternate`: the reads
    alternate between two bins; three waves and a part of one"""
    iso = [interval_line("w.a", "chr1", "+", [(100 * k, 100 * k + 50) for k in range(64)]), interval_line("v.a", "chr1", "+", [(10000, 10050), (10100, 10150)])]
    if kind == "distinct":
        lines = [mrf_line("chr1", "+", [(100 * (k % 64) + 10, 100 * (k % 64) + 40)]) for k in range(3 * 64 + 17)]
    else:
        lines = [mrf_line("chr1", "+", [(10000 + 100 * (k & 1) + 10, 10000 + 100 * (k & 1) + 40)]) for k in range(3 * 64 + 17)]
    return iso, lines


def many_case(n_genes=3000, seed=29):
    """(isoform lines, mrf lines): more genes, and more bins, than a workgroup of the count kernel keeps counters of its own for:
    one-exon genes 100 bases apart, two reads on every gene and a third on every seventh, shuffled"""
    iso = [interval_line("m%04d.a" % g, "chr1", "+", [(100 * g, 100 * g + 60)]) for g in range(n_genes)]
    rng = random.Random(seed)
    at = [g for g in range(n_genes) for _ in range(3 if g % 7 == 0 else 2)]
    rng.shuffle(at)
    return iso, [mrf_line("chr1", "+", [(100 * g + rng.randrange(50), 100 * g + 70)]) for g in at]
