"""What the loader must make of every line of an MRF text, restated in plain Python, and the inputs of the routing tests.
Not a test module.  No GPU code: the annotation's side comes from the compiled events (Events.covered / span / chrom / strand /
bucket_events, all host calls), the merge from the oracle's interval list.

The definition (the reference's loader, count/count.cpp:279-336, as oracle/lsq_oracle.c restates it), per data line:

  kept blocks   a block (chrom, strand, start - 1, end) is kept if the chromosome has tables, both coordinates lie strictly
                inside (-2^30, 2^30), and contains_interval holds against the covered regions of the chromosome (of the
                chromosome and the read's transcript strand in a stranded job): lower bound of the start among the regions'
                starts; the region there, or the one before it, holds the block.  A block with start >= end is contained
                wherever it lies: it adds no base, and still gives the read its chromosome and strand.
  merge         the kept blocks go through interval_list::add (oracle_binding.merge_intervals) one after the other, in file
                order, whatever their chromosome.  The read's chromosome and strand are the last kept block's.
  retained      a read that kept a block and whose merged list is not empty.  THIS is what Context.retained reports -- and
                what the oracle's n_loaded counts too: the oracle drops a read whose kept blocks are all empty (the
                reference itself reads the first start of an empty list there, which is undefined).  test_route_reference_host
                pins the equality on every case file.
  pooled        p = the first merged base; the planned events are the shard's when one is set.  MUST: every planned event of
                the read's chromosome (and transcript strand, stranded) with gene_start <= p < gene_end is among the events of
                the bucket the read lies in.  MAY: a pooled read has a planned event with gene_start <= p <= gene_end (the
                reference's candidate window, count.cpp:423-432, closed at its end).  No event in the closed window: in no
                pool.  An event in the half-open window: in exactly one pool, once.
  pool          three or more merged blocks: "many".  Wide pools: "one" / "two" / "many" by the number of blocks exactly.
                Compact pools: a one- or two-block read may sit in "many" instead.
  stranded      the transcript strand is that of the first block's strand column ("+" plus, "-" minus), flipped by a reverse
                library; a first block with another string makes no read; the read carries "+" or "-", its transcript strand.
"""
import itertools
import os
import random

import oracle_binding as ob
from golden_inputs import interval_line

LIM = 1 << 30
SHIFT0 = 10                 # the locator's smallest shift
LOC_CAP = 1 << 22           # ... raised until the grid has at most this many entries


# ---------------------------------------------------------------------------------------------------------------- the text
def parse_mrf(text):
    """[(line_no, [(chrom, strand, start - 1, end)])] of the data lines: the first line is the header whatever it says, the
    lines after it count from 1, '#' lines and a repeated header line are no data"""
    out = []
    for k, line in enumerate(text.split("\n")[1:], 1):
        if line == "" and k == text.count("\n"):
            break                                     # (what follows the last newline)
        if line.startswith("#") or line == "AlignmentBlocks":
            continue
        blocks = []
        for item in line.split(","):
            f = item.split(":")
            blocks.append((f[0], f[1], int(f[2]) - 1, int(f[3])))
        out.append((k, blocks))
    return out


def contains_interval(regions, start, end):
    """interval_list::contains_interval over sorted disjoint (start, end) regions"""
    if not start < end:
        return True
    lo = 0
    while lo < len(regions) and regions[lo][0] < start:        # lower bound of `start` among the starts, the slow way
        lo += 1
    for q in (lo, lo - 1):
        if 0 <= q < len(regions) and regions[q][0] <= start and end <= regions[q][1]:
            return True
    return False


# ---------------------------------------------------------------------------------------------------------------- the job
class Job:
    """the annotation's side of a job, read off compiled events once (shard: (first event, events) or None)"""

    def __init__(self, events, chrom_names, shard=None):
        self.library = events.library
        self.stranded = self.library != "unstranded"
        self.n_events = len(events)
        self.ev = [(events.chrom(i), events.strand(i)) + tuple(events.span(i)) for i in range(self.n_events)]
        self.planned = range(self.n_events) if shard is None else range(shard[0], shard[0] + shard[1])
        self.covered = {}
        for c in chrom_names:
            for minus in ((False, True) if self.stranded else (False,)):
                self.covered[(c, int(minus))] = events.covered(c, minus)
        self.has_tables = set(c for (c, _), v in self.covered.items() if v)
        self.buckets = [set(events.bucket_events(b)[1]) for b in range(events.num_buckets)]

    def regions(self, chrom, t):
        return self.covered.get((chrom, t if self.stranded else 0), [])

    def window(self, chrom, t, p, closed):
        """the planned events whose span holds p"""
        return [i for i in self.planned if self.ev[i][0] == chrom and (not self.stranded or self.ev[i][1] == "+-"[t])
                and self.ev[i][2] <= p and (p <= self.ev[i][3] if closed else p < self.ev[i][3])]


class RefRead:
    __slots__ = ("line", "chrom", "strand", "t", "blocks", "n_kept", "n_dropped", "other_chrom", "must", "may")


def route(job, text):
    """-> (reads: {line_no: RefRead} of the retained reads, tally: dict).  RefRead.must / .may: the planned events with the
    first base in their half-open / closed span."""
    reads = {}
    tally = {"lines": 0, "no_strand": 0, "made_plus": 0, "made_minus": 0, "kept_plus": 0, "kept_minus": 0, "dropped": 0, "only_empty": 0}
    for line_no, blocks in parse_mrf(text):
        tally["lines"] += 1
        t = 0
        if job.stranded:
            s0 = blocks[0][1]
            if s0 not in ("+", "-"):
                tally["no_strand"] += 1
                continue
            t = int((s0 == "-") ^ (job.library == "reverse"))
            tally["made_minus" if t else "made_plus"] += 1
        kept = []
        for chrom, strand, start, end in blocks:
            if chrom not in job.has_tables or not (-LIM < start < LIM and -LIM < end < LIM):
                continue
            if contains_interval(job.regions(chrom, t), start, end):
                kept.append((chrom, strand, start, end))
        merged = ob.merge_intervals([(start, end) for _, _, start, end in kept if start < end])      # (one after the other, in file order)
        if not kept or not merged:
            tally["dropped" if not kept else "only_empty"] += 1
            continue
        r = RefRead()
        r.line, r.chrom, r.t = line_no, kept[-1][0], t
        r.strand = "+-"[t] if job.stranded else kept[-1][1]
        r.blocks = tuple((int(s), int(e)) for s, e in merged)
        r.n_kept, r.n_dropped = len(kept), len(blocks) - len(kept)
        r.other_chrom = len(set(b[0] for b in kept)) > 1
        r.must = job.window(r.chrom, t, r.blocks[0][0], closed=False)
        r.may = job.window(r.chrom, t, r.blocks[0][0], closed=True)
        reads[line_no] = r
        if job.stranded:
            tally["kept_minus" if t else "kept_plus"] += 1
    return reads, tally


def outcomes(job, reads, tally):
    """how many reads of a routed text meet each outcome the cases are built for"""
    o = {"dropped": tally["dropped"], "only_empty": tally["only_empty"], "no_strand": tally["no_strand"], "unrouted": 0, "closed_only": 0,
         "one": 0, "two": 0, "many": 0, "long_block": 0, "shrunk": 0, "other_chrom": 0,
         "at_start_m1": 0, "at_start": 0, "at_end_m1": 0, "at_end": 0, "at_end_p1": 0}
    for r in reads.values():
        if not r.may:
            o["unrouted"] += 1
        elif not r.must:
            o["closed_only"] += 1
        if r.must:
            o[("one", "two", "many")[min(len(r.blocks), 3) - 1]] += 1
            o["long_block"] += len(r.blocks) <= 2 and any(e - s >= 1024 for s, e in r.blocks)      # (compact pools: must sit in "many")
        o["shrunk"] += len(r.blocks) < r.n_kept
        o["other_chrom"] += r.other_chrom
        p = r.blocks[0][0]
        for i in job.planned:
            c, st, gs, ge = job.ev[i]
            if c != r.chrom or (job.stranded and st != "+-"[r.t]):
                continue
            for key, x in (("at_start_m1", gs - 1), ("at_start", gs), ("at_end_m1", ge - 1), ("at_end", ge), ("at_end_p1", ge + 1)):
                o[key] += p == x
    return o


def check_pools(job, reads, pooled, strand_name, compact, what=""):
    """the pooled reads of one front end -- Context.pool_reads() -- against the reference: every invariant of the module's
    docstring, read by read.  strand_name: strand id -> string.  Returns {bucket: sorted [(line, strand string, blocks, pool)]}."""
    seen = {}
    per_bucket = {}
    for line, bucket, sid, pool, blocks in pooled:
        assert line not in seen, (what, "line pooled twice", line, seen[line], bucket)
        seen[line] = bucket
        r = reads.get(line)
        assert r is not None, (what, "a read the reference does not retain is pooled", line, bucket, blocks)
        assert blocks == r.blocks, (what, "blocks", line, blocks, r.blocks)
        assert strand_name(sid) == r.strand, (what, "strand", line, strand_name(sid), r.strand)
        assert r.may, (what, "pooled without an event in the closed window", line, blocks)
        assert 0 <= bucket < len(job.buckets) and set(r.must) <= job.buckets[bucket], (what, "bucket", line, bucket, r.must, sorted(job.buckets[bucket]))
        assert any(job.ev[i][0] == r.chrom for i in job.buckets[bucket]), (what, "bucket of another chromosome", line, bucket)
        want = ("one", "two", "many")[min(len(blocks), 3) - 1]
        assert pool == want or (compact and pool == "many"), (what, "pool", line, pool, want)
        if compact and any(e - s >= 1024 for s, e in blocks):          # (a compact record holds blocks shorter than 1 024 bases)
            assert pool == "many", (what, "pool of a long block", line, pool)
        per_bucket.setdefault(bucket, []).append((line, r.strand, blocks, pool))
    for line, r in reads.items():
        if r.must:
            assert line in seen, (what, "a read with an event in the half-open window is in no pool", line, r.blocks, r.must)
    return {b: sorted(v) for b, v in per_bucket.items()}


# ---------------------------------------------------------------------------------------------------------------- the grid
def locator_of(job, chrom, t=0, shift=SHIFT0):
    """(loc_base, loc_nb) of a chromosome table by the construction in lsq_device.hip, from the covered and the span starts
    (a cluster record starts at a span start or at a bucket's first base, which is one)"""
    starts = [s for s, _ in job.regions(chrom, t)] + [job.ev[i][2] for i in job.planned if job.ev[i][0] == chrom and (not job.stranded or job.ev[i][1] == "+-"[t])]
    base = (min(starts) >> shift) << shift
    return base, ((max(starts) - base) >> shift) + 1


def grid_entries(job, chroms, shift):
    n = 0
    for c in chroms:
        for t in ((0, 1) if job.stranded else (0,)):
            starts = [s for s, _ in job.regions(c, t)]
            if starts:
                n += (max(starts) >> shift) - (min(starts) >> shift) + 2
    return n


def shift_of(job, chroms):
    shift = SHIFT0
    while grid_entries(job, chroms, shift) > LOC_CAP and shift < 30:
        shift += 1
    return shift


def starts_per_bin(starts, base, nb, shift=SHIFT0):
    h = [0] * nb
    for s in starts:
        h[(s - base) >> shift] += 1
    return h


# ---------------------------------------------------------------------------------------------------------------- the cases
class Case:
    """name, genes [(gene, chrom, strand, [isoform exons, ...])], chromosome names the reads use, {file stem: MRF text}"""

    def __init__(self, name, genes, chroms, texts, library="unstranded"):
        self.name, self.genes, self.chroms, self.texts, self.library = name, genes, chroms, texts, library

    def write(self, d):
        iv, mp = os.path.join(d, self.name + ".interval"), os.path.join(d, self.name + ".map")
        with open(iv, "w") as f, open(mp, "w") as g:
            for gene, chrom, strand, isoforms in self.genes:
                for k, exons in enumerate(isoforms):
                    f.write(interval_line("%s.%d" % (gene, k), chrom, strand, exons))
                    g.write("%s\t%s.%d\n" % (gene, gene, k))
        paths = {}
        for stem, text in self.texts.items():
            paths[stem] = os.path.join(d, "%s_%s.mrf" % (self.name, stem))
            with open(paths[stem], "w") as f:
                f.write(text)
        return iv, mp, paths

    def argv(self, iv, mp, path, R=50):
        return ["0", "x", "./", "LH_GENE_TXT", iv, "UCSC_GENE2ISOFORM", mp, "0", "1000000", "MRF_SINGLE", "SHORT_READ", str(R), path]


def text_of(reads, strand="+"):
    """reads: lists of (chrom, start, end) or (chrom, start, end, strand) blocks, 0-based half-open (an empty or inverted block is
    written as it is)"""
    lines = ["AlignmentBlocks"]
    for blocks in reads:
        lines.append(",".join("%s:%s:%d:%d:1:1" % (b[0], b[3] if len(b) > 3 else strand, b[1] + 1, b[2]) for b in blocks))
    return "\n".join(lines) + "\n"


def small_gene(name, chrom, s, strand="+"):
    """two exons of 20 bases, 30 apart; the second isoform skips... nothing it could: it ends early"""
    return (name, chrom, strand, [[(s, s + 20), (s + 50, s + 70)], [(s, s + 20)]])


def edge_reads(chrom, regions):
    """per region: blocks that begin at start + d or end at end + d, d in -1, 0, 1, of one base, the region's length and one more"""
    out = []
    for rs, re in regions:
        for d in (-1, 0, 1):
            for ln in (1, re - rs, re - rs + 1):
                out.append([(chrom, rs + d, rs + d + ln)])
                out.append([(chrom, re + d - ln, re + d)])
    return out


def bin_edge_reads(chrom, xs):
    return [[(chrom, x + d, x + d + ln)] for x in xs for d in (-1, 0, 1) for ln in (1, 30)]


def union(exons):
    return ob.merge_intervals(sorted(exons)) if exons else []


def regions_of(genes, chrom, strand=None):
    """the covered regions as the annotation gives them: the union of the chromosome's exons (the tests compare it with
    Events.covered before they build on it)"""
    ex = sorted(set(e for _, c, st, iso in genes if c == chrom and strand in (None, st) for exons in iso for e in exons))
    out = []
    for s, e in ex:
        if out and s <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def bins_case():
    """shift 10.  chrA starts on a multiple of 1024: three bins of genes 100 bases apart (twelve region starts and six gene
    starts a bin), then bins of 0, 1, 3, 4 and 5 region starts; chrB starts off a multiple; chrC has one gene; chrD a gene
    across 0; chrA also holds spans that overlap, for first bases around a span's ends."""
    A0 = 10240
    genes = [small_gene("a%02d" % k, "chrA", A0 + 170 * k) for k in range(18)]           # bins 0-2
    b = lambda k: A0 + 1024 * k
    genes += [small_gene("s1", "chrA", b(5) - 30),                                      # bin 4: one start; bin 5: one ...
              small_gene("s2", "chrA", b(5) + 200),                                     # ... and two: three
              small_gene("s3", "chrA", b(7) + 100), small_gene("s4", "chrA", b(7) + 400),       # bin 7: four
              small_gene("s5", "chrA", b(9) + 100), small_gene("s6", "chrA", b(9) + 400), small_gene("s7", "chrA", b(10) - 30)]       # bin 9: five; bin 10: one
    # spans that overlap: w ends 5 bases into x; y's first exon lies over x's end
    X = b(12) + 300
    genes += [("w", "chrA", "+", [[(X - 65, X - 45), (X - 15, X + 5)], [(X - 65, X - 45)]]), small_gene("x", "chrA", X),
              ("y", "chrA", "+", [[(X + 65, X + 85), (X + 115, X + 135)], [(X + 65, X + 85)]])]
    genes += [small_gene("b%d" % k, "chrB", 5000 + 170 * k) for k in range(4)]
    genes += [small_gene("c0", "chrC", 70000)]
    genes += [("d0", "chrD", "+", [[(-70, -50), (-20, 0), (30, 50)], [(-70, -50), (30, 50)]]), small_gene("d1", "chrD", 400)]
    reads = []
    for c in ("chrA", "chrB", "chrC", "chrD"):
        reg = regions_of(genes, c)
        reads += edge_reads(c, reg)
        reads += [[(c, r1[1] - 5, r1[1]), (c, r2[0], r2[0] + 5)] for r1, r2 in zip(reg, reg[1:])]
        reads += [[(c, r1[0], r1[0] + 5), (c, r2[0], r2[0] + 5), (c, r3[1] - 5, r3[1])] for r1, r2, r3 in zip(reg, reg[1:], reg[2:])]
        starts = [s for s, _ in reg]
        base = (min(starts) >> 10) << 10
        nb = ((max(starts) - base) >> 10) + 1
        reads += bin_edge_reads(c, [base + 1024 * k for k in range(-1, nb + 2)])
    for g, c, _, iso in genes:                                                        # first bases around every span's ends
        gs, ge = min(s for ex in iso for s, _ in ex), max(e for ex in iso for _, e in ex)
        reads += [[(c, p, p + 4)] for p in (gs - 1, gs, ge - 1, ge, ge + 1)]
    reads += [[("chrA", A0, A0 + 20), ("chrC", 70000, 70010)], [("chrB", 5000, 5010), ("chrA", A0 + 50, A0 + 50)]]       # the last kept block's chromosome, where the first base lies in no span
    reads += [[("chrZ", 10240, 10260)], [("chrZ", 100, 130), ("chrZ", 200, 230)], [("chrZ", 10240, 10260), ("chrA", A0, A0 + 20)]]
    reads += [[("chrD", -20, 0)], [("chrD", -1, 0)], [("chrD", -1, 1)], [("chrD", -60, -50), ("chrD", -20, -10)], [("chrD", -5, 0), ("chrD", 30, 35)], [("chrD", -70, -69)]]
    return Case("bins", genes, ("chrA", "chrB", "chrC", "chrD", "chrZ"), {"r": text_of(reads)})


WIDE_MID = 536870912          # 2^29: a multiple of every bin width in reach


def wide_case(n_chrom):
    """per chromosome a gene at 1 000, genes whose first exon starts exactly at 2^29 - 2048, 2^29 and 2^29 + 2048, and one at
    [1 073 000 000, 1 073 000 400): four chromosomes take 4 * 1 047 853 = 4 191 412 grid entries at shift 10, under the cap of
    2^22; five exceed it and go to shift 11.  The reads are the same whatever the chromosomes."""
    genes, reads = [], []
    for q in range(n_chrom):
        c = "chrW%d" % q
        genes.append(small_gene("w%d_lo" % q, c, 1000))
        for m in (-1, 0, 1):
            x = WIDE_MID + 2048 * m
            genes.append(("w%d_m%d" % (q, m + 1), c, "+", [[(x - 50, x - 30), (x, x + 20), (x + 50, x + 70)], [(x - 50, x - 30), (x + 50, x + 70)]]))
        T = 1073000000
        genes.append(("w%d_hi" % q, c, "+", [[(T, T + 20), (T + 50, T + 70), (T + 380, T + 400)], [(T, T + 20), (T + 380, T + 400)]]))
    for q in range(min(n_chrom, 4)):
        c = "chrW%d" % q
        reg = regions_of(genes, c)
        reads += edge_reads(c, reg)
        reads += [[(c, r1[1] - 5, r1[1]), (c, r2[0], r2[0] + 5)] for r1, r2 in zip(reg, reg[1:]) if r2[0] - r1[1] < 1000]
        reads += bin_edge_reads(c, [WIDE_MID + 1024 * k for k in range(-5, 6)] + [0, 1024, 2048, 1073000000 - 576, 1073000000 + 448])
    reads += [[("chrW9", 1000, 1020)], [("chrZ", WIDE_MID, WIDE_MID + 20)]]
    return Case("wide%d" % n_chrom, genes, tuple("chrW%d" % q for q in range(n_chrom)) + ("chrW9", "chrZ"), {"r": text_of(reads)})


MERGE_ALPHABET = {"base": (1110, 1130), "overlap": (1120, 1140), "nested": (1115, 1125), "equal": (1110, 1130), "touch_after": (1130, 1140),
                  "touch_before": (1100, 1110), "disjoint": (1150, 1160), "empty": (1135, 1135), "inverted": (1140, 1130)}


def merge_case():
    """one long exon holds every block: what is left is the merge"""
    genes = [("m", "chrM", "+", [[(1000, 3000)], [(1000, 2000), (2500, 3000)]]), small_gene("n", "chrN", 500)]
    M = lambda *bl: [("chrM", s, e) for s, e in bl]
    fixed = [M(*t) for t in itertools.product(MERGE_ALPHABET.values(), repeat=3)]
    # 2 -> 3 -> 2: a later block bridges two earlier ones
    fixed += [M((1100, 1110), (1120, 1130), (1140, 1150), (1105, 1125)), M((1100, 1110), (1140, 1150), (1120, 1130), (1125, 1145)),
              M((1100, 1110), (1120, 1130), (1140, 1150), (1110, 1120)), M((1100, 1110), (1120, 1130), (1140, 1150), (1110, 1140)),
              M((1100, 1110), (1120, 1130), (1140, 1150), (1090, 1160)), M((1100, 1110), (1120, 1130), (1140, 1150), (1160, 1170), (1105, 1165))]
    dropped = [("chrM", 500, 510), ("chrZ", 1100, 1110), ("chrM", 2990, 3001), ("chrN", 100, 110)]
    for nb in (3, 5, 9, 16):
        for first in (1100, 1101):
            bl = []
            for k in range(nb):
                bl.append(("chrM", first + 30 * k, first + 30 * k + 12))
                if k % 2 == 0:
                    bl.append(dropped[(k // 2) % len(dropped)])
            fixed.append(bl)
            fixed.append(list(reversed(bl)))
    # 16 blocks that shrink to 8, then to 1
    fixed.append(M(*[(1100 + 20 * k, 1110 + 20 * k) for k in range(16)]) + M(*[(1105 + 40 * k, 1125 + 40 * k) for k in range(8)]))
    fixed.append(M(*[(1100 + 20 * k, 1110 + 20 * k) for k in range(16)]) + M((1100, 1410)))
    # the last kept block on another chromosome, or with another strand string
    fixed += [M((1100, 1120)) + [("chrN", 500, 510)], M((1100, 1120), (1200, 1220)) + [("chrN", 505, 505)], [("chrN", 500, 510)] + M((1100, 1120)),
              [("chrM", 1100, 1120, "+"), ("chrM", 1200, 1220, "-")], [("chrM", 1100, 1120, "-"), ("chrM", 1110, 1130, "xyz")], [("chrM", 1100, 1120, "+"), ("chrM", 1105, 1105, ".")],
              M((1100, 1120)) + [("chrN", 100, 110)], M((1100, 1120)) + [("chrZ", 1100, 1100)]]
    # only empty blocks
    fixed += [M((1135, 1135)), M((1135, 1135), (1140, 1130)), M((500, 500), (5000, 4000)), [("chrN", 500, 500)] + M((1100, 1100))]
    texts = {"fixed": text_of(fixed)}
    for seed in (1, 2, 3):
        rng = random.Random(seed)
        rnd = []
        for _ in range(3000):
            w = rng.randrange(1000, 2930)
            rnd.append(M(*[(lambda a, ln: (a, a + ln))(w + rng.randrange(60), rng.choice((0, 1, 1, 2, 3, 5, 8, 13, 21))) for _ in range(rng.randrange(1, 7))]))
        texts["seed%d" % seed] = text_of(rnd)
    return Case("merge", genes, ("chrM", "chrN", "chrZ"), texts)


BIG = 1 << 18          # a read of this many merged bases is refused


def limits_case():
    """the first and last representable bases; reads of 2^18 - 1 merged bases (pooled) and of 2^18 (refused)"""
    genes = [("top", "chrP", "+", [[(LIM - 101, LIM - 81), (LIM - 21, LIM - 1)], [(LIM - 21, LIM - 1)]]),
             ("bot", "chrP", "+", [[(-LIM + 1, -LIM + 21), (-LIM + 81, -LIM + 101)], [(-LIM + 1, -LIM + 21)]]),
             ("long", "chrQ", "+", [[(100000, 400000)], [(100000, 200000), (300000, 400000)]])]
    P = lambda *bl: [("chrP", s, e) for s, e in bl]
    Q = lambda *bl: [("chrQ", s, e) for s, e in bl]
    good = [P((LIM - 21, LIM - 1)), P((LIM - 2, LIM - 1)), P((LIM - 21, LIM)), P((LIM - 1, LIM)), P((LIM - 101, LIM - 81), (LIM - 21, LIM - 1)), P((LIM - 21, LIM - 1), (LIM - 1, LIM)),
            P((-LIM + 1, -LIM + 21)), P((-LIM + 1, -LIM + 2)), P((-LIM, -LIM + 21)), P((-LIM, -LIM + 1)), P((-LIM + 1, -LIM + 21), (-LIM + 81, -LIM + 101)), P((-LIM, -LIM + 1), (-LIM + 1, -LIM + 21)),
            P((LIM - 1, LIM - 1)), P((-LIM, -LIM)), P((LIM, LIM)),
            Q((100000, 100000 + BIG - 1)), Q((100000, 187381), (187382, 274763), (274764, 100002 + BIG - 1)), Q((100000, 100050)), Q((399990, 400000)),
            Q((100000, 101023)), Q((100000, 101024)), Q((100000, 100010), (399990, 400000))]
    assert sum(e - s for _, s, e in good[16]) == BIG - 1
    many = [Q((100000 + 7 * k, 100003 + 7 * k), (100100 + 7 * k, 100103 + 7 * k), (100200 + 7 * k, 100203 + 7 * k)) for k in range(40)]
    # short reads that fit compact records, so that the few long ones (more than 1 in 16 would turn the file to wide records) stay
    # the exception: the file is kept in compact records when they are asked for
    short = [Q((100000 + 11 * k, 100030 + 11 * k)) for k in range(60)] + [Q((150000 + 11 * k, 150020 + 11 * k), (150100 + 11 * k, 150120 + 11 * k)) for k in range(20)]
    short += [P((LIM - 21 + k, LIM - 1)) for k in range(1, 10)] + [P((-LIM + 1, -LIM + 21 - k)) for k in range(1, 10)]
    # a last kept block on another chromosome, where the first base lies in no span
    short += [[("chrQ", 100000, 100050), ("chrP", LIM - 21, LIM - 1)]]
    return Case("limits", genes, ("chrP", "chrQ"), {"good": text_of(good + many + short), "big1": text_of([Q((100000, 100050)), Q((100000, 100000 + BIG))]),
                                                    "big3": text_of([Q((100000, 187381), (187382, 274763), (274764, 100002 + BIG)), Q((100000, 100050))])})


def stranded_case():
    """a plus and a minus gene overlap on chrS with different exons: the covered regions differ per strand; chrT has plus genes
    only.  Strand columns "+", "-", ".", a long string; second blocks whose strand column disagrees with the first."""
    genes = [("p", "chrS", "+", [[(1000, 1100), (1300, 1400), (1600, 1700)], [(1000, 1100), (1600, 1700)]]),
             ("q", "chrS", "-", [[(1050, 1250), (1350, 1500)], [(1050, 1250)]]),
             ("p2", "chrS", "+", [[(1680, 1760), (1800, 1850)], [(1680, 1760)]]),
             ("t", "chrT", "+", [[(200, 300), (400, 500)], [(200, 300)]])]
    long_strand = "s" * 40
    reads = []
    for st in ("+", "-", ".", long_strand):
        for c in ("chrS", "chrT"):
            for strand in ("+", "-"):
                for rd in edge_reads(c, regions_of(genes, c, strand)):
                    reads.append([b + (st,) for b in rd])
        reads += [[("chrS", 1060, 1090, st), ("chrS", 1360, 1390, st)], [("chrS", 1060, 1090, st), ("chrS", 1610, 1640, st)],
                  [("chrS", 1060, 1090, st), ("chrS", 1360, 1390, st), ("chrS", 1610, 1640, st)], [("chrZ", 1060, 1090, st)]]
    for a, b in (("+", "-"), ("-", "+"), ("+", "."), (".", "+"), ("-", long_strand), (long_strand, "-")):
        reads += [[("chrS", 1060, 1090, a), ("chrS", 1360, 1390, b)], [("chrS", 1060, 1090, a), ("chrS", 1070, 1100, b)], [("chrS", 1060, 1090, a), ("chrS", 1200, 1200, b)],
                  [("chrS", 1210, 1240, a), ("chrS", 1360, 1390, b), ("chrS", 1460, 1490, b)], [("chrT", 210, 240, a), ("chrT", 410, 440, b)]]
    reads += [[("chrT", 210, 240, st), ("chrS", 1060, 1090, st)] for st in ("+", "-")]       # both in plus regions: a read of chrS, whose first base (210) lies in no span there
    for p in (999, 1000, 1049, 1050, 1249, 1250, 1251, 1499, 1500, 1501, 1699, 1700, 1701, 1759, 1760, 1849, 1850):
        reads += [[("chrS", p, p + 3, st)] for st in ("+", "-")]
    return Case("stranded", genes, ("chrS", "chrT", "chrZ"), {"r": text_of(reads)}, library="forward")


def shard_case():
    """genes that interleave in output order (names) and in place: the even ones a slice, the odd ones the other"""
    genes = []
    for k in range(8):
        s = 2000 + 120 * k
        genes.append(("g%d%d" % (k % 2, k), "chrH", "+", [[(s, s + 40), (s + 60, s + 100)], [(s, s + 40)]]))       # g0*: k even, sorted first
    genes.append(("g09", "chrI", "+", [[(100, 140), (160, 200)], [(100, 140)]]))
    genes.append(("g19", "chrI", "+", [[(190, 230), (240, 300)], [(240, 300)]]))                                  # its first exon lies over g09's end
    reads = []
    for c in ("chrH", "chrI"):
        reg = regions_of(genes, c)
        reads += edge_reads(c, reg)
        reads += [[(c, r1[1] - 5, r1[1]), (c, r2[0], r2[0] + 5)] for r1, r2 in zip(reg, reg[1:])]
    for g, c, _, iso in genes:
        gs, ge = min(s for ex in iso for s, _ in ex), max(e for ex in iso for _, e in ex)
        reads += [[(c, p, p + 4)] for p in (gs - 1, gs, ge - 1, ge, ge + 1)]
    return Case("shard", genes, ("chrH", "chrI"), {"r": text_of(reads)})


# the outcomes every text is built to contain: asserted (>= 1) from the reference alone wherever the text is used.  "unrouted" -- a
# retained read with no planned event in the closed window -- needs a last kept block on another chromosome (or a shard): the bins,
# merge/fixed, limits and stranded files and the shard's slices hold one; the wide files cannot (their chromosomes carry the same
# genes, so a covered base lies in a span on every one of them), nor can merge's seeded files (one exon).
WANT = {("bins", "r"): ("dropped", "unrouted", "one", "two", "many", "at_start_m1", "at_start", "at_end_m1", "at_end", "at_end_p1"),
        ("wide4", "r"): ("dropped", "one", "two", "at_start", "at_end_m1"), ("wide5", "r"): ("dropped", "one", "two", "at_start", "at_end_m1"),
        ("merge", "fixed"): ("only_empty", "unrouted", "one", "two", "many", "shrunk", "other_chrom"),
        ("merge", "seed1"): ("only_empty", "one", "two", "many", "shrunk"), ("merge", "seed2"): ("only_empty", "one", "two", "many", "shrunk"),
        ("merge", "seed3"): ("only_empty", "one", "two", "many", "shrunk"),
        ("limits", "good"): ("dropped", "only_empty", "unrouted", "one", "two", "many", "long_block"), ("limits", "big1"): ("one",), ("limits", "big3"): ("one", "many"),
        ("stranded", "r"): ("no_strand", "dropped", "unrouted", "one", "two", "many", "shrunk", "at_start", "at_end_m1", "at_end", "at_end_p1"),
        ("shard", "r"): ("dropped", "one", "two", "at_start_m1", "at_start", "at_end_m1", "at_end", "at_end_p1")}
WANT_SLICE = ("unrouted", "one", "two", "at_start", "at_end_m1")        # ... and each slice of the shard case; the first also "closed_only"


def assert_contains(case, stem, o, keys=None):
    for k in (WANT[(case.name, stem)] if keys is None else keys):
        assert o[k] >= 1, (case.name, stem, k, o)


def all_cases():
    return [bins_case(), wide_case(4), wide_case(5), merge_case(), limits_case(), stranded_case(), shard_case()]
