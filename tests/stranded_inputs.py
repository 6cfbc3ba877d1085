"""Inputs and expected tables of the stranded-library tests.  Not a test module.

A stranded job is by definition two unstranded jobs: the plus genes on the reads whose transcript strand is "+", the minus
genes on those whose transcript strand is "-".  So the expected table of a case comes from the oracle (oracle_binding.run,
which restates the unstranded reference) run twice on inputs split here in Python, its rows put back in output order.  The
split read files keep every line's number (a read that is left out becomes a '#' line: read names are "read-<line>") and
carry the transcript strand in the strand column, as `sam2mrf --library` writes it."""
import os
import random

import oracle_binding as ob
from bam_writer import sam_to_bam

LIBS = ("forward", "reverse")


def transcript_minus(lib, minus, flag=0):
    """t = s XOR (library == reverse) XOR mate2, as 0 (plus) / 1 (minus)"""
    mate2 = bool(flag & 0x1) and bool(flag & 0x80)
    return int(bool(minus) ^ (lib == "reverse") ^ mate2)


class Gene:
    def __init__(self, name, chrom, strand, isoforms):
        self.name, self.chrom, self.strand, self.isoforms = name, chrom, strand, isoforms      # isoforms: [(name, [(start, end), ...])]


def write_annotation(d, stem, genes):
    iv, mp = os.path.join(d, stem + ".interval"), os.path.join(d, stem + ".map")
    with open(iv, "w") as f, open(mp, "w") as g:
        for ge in genes:
            for iname, exons in ge.isoforms:
                st = ge.strand if isinstance(ge.strand, str) else ge.strand[iname]
                f.write("%s\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (iname, ge.chrom, st, exons[0][0], exons[-1][1], len(exons),
                                                             ",".join(str(s) for s, _ in exons), ",".join(str(e) for _, e in exons)))
                g.write("%s\t%s\n" % (ge.name, iname))
    return iv, mp


class Rec:
    """one alignment: blocks are 0-based [start, end) on the reference; flag carries the strand and the mate bits"""

    def __init__(self, chrom, flag, blocks, mrf_strand=None):
        self.chrom, self.flag, self.blocks, self.mrf_strand = chrom, flag, blocks, mrf_strand

    @property
    def r_minus(self):      # the strand of the fragment's first mate: what the MRF form of the record carries
        return bool(self.flag & 0x10) ^ (bool(self.flag & 0x1) and bool(self.flag & 0x80))

    def t(self, lib):
        """0 / 1, or None for an MRF record whose strand column is neither + nor -"""
        if self.mrf_strand is not None and self.mrf_strand not in ("+", "-"):
            return None
        return int(self.r_minus ^ (lib == "reverse"))

    def mrf_line(self, strand):
        out, q = [], 1
        for s, e in self.blocks:
            out.append("%s:%s:%d:%d:%d:%d" % (self.chrom, strand, s + 1, e, q, q + e - s - 1))
            q += e - s
        return ",".join(out)

    def sam_line(self, k):
        cig, prev = "", None
        for s, e in self.blocks:
            if prev is not None:
                cig += "%dN" % (s - prev)
            cig += "%dM" % (e - s)
            prev = e
        return "q%d\t%d\t%s\t%d\t30\t%s\t*\t0\t0\t*\t*" % (k, self.flag, self.chrom, self.blocks[0][0] + 1, cig)


SAM_HEADER = ["@HD\tVN:1.6\tSO:unsorted", "@SQ\tSN:chrA\tLN:100000", "@SQ\tSN:chrB\tLN:100000", "@SQ\tSN:chrC\tLN:100000"]


def sam_text(recs, header=SAM_HEADER):
    return "".join(h + "\n" for h in header) + "".join(r.sam_line(k) + "\n" for k, r in enumerate(recs))


def mrf_text(recs, n_comment, strand_of):
    """header, a '#' line per SAM header line (so that a record has the line number it has in the SAM file), a line per record;
    strand_of(rec) -> the strand column, or None for a line that is left out ('#')"""
    out = ["AlignmentBlocks"] + ["#"] * n_comment
    for r in recs:
        st = strand_of(r)
        out.append("#" if st is None else r.mrf_line(st))
    return "".join(ln + "\n" for ln in out)


def input_mrf(recs, n_comment=len(SAM_HEADER)):
    """the MRF input of a job: the strand column holds the first mate's strand (MRF knows no mates), or the record's own string"""
    return mrf_text(recs, n_comment, lambda r: r.mrf_strand if r.mrf_strand is not None else "-" if r.r_minus else "+")


def merge_tables(tables):
    """rows of several tables in output order: by gene name, bytewise; a gene's rows stay together and in order"""
    rows = []
    for t in tables:
        for k, ln in enumerate(t.splitlines()):
            rows.append((ln.split("\t")[0].encode(), len(rows), ln))
    rows.sort(key=lambda x: (x[0], x[1]))
    return "".join(ln + "\n" for _, _, ln in rows)


def expected(d, tag, genes, recs, lib, tool="count", R=50, n_comment=len(SAM_HEADER), total_read_bases="1000000"):
    """(table, reads retained per transcript strand) of the stranded job, from two oracle runs on the split inputs"""
    tables, retained = [], []
    for tbit, strand in enumerate("+-"):
        sub = [g for g in genes if g.strand == strand]
        iv, mp = write_annotation(d, "%s_%s_%d" % (tag, lib, tbit), sub)
        path = os.path.join(d, "%s_%s_%d.mrf" % (tag, lib, tbit))
        with open(path, "w") as f:
            f.write(mrf_text(recs, n_comment, lambda r: strand if r.t(lib) == tbit else None))
        argv = ["0", "x", "./", "LH_GENE_TXT", iv, "UCSC_GENE2ISOFORM", mp, "0", "1000000", "MRF_SINGLE", "SHORT_READ", str(R), path]
        if tool == "solve":
            argv.append(total_read_bases)
        if not sub:
            tables.append(""); retained.append(0)
            continue
        rc, text, _ = ob.run(tool, argv)
        assert rc == 0, (rc, argv)
        tables.append(text)
        retained.append(ob.last_n_loaded[0])
    return merge_tables(tables), retained


def unstranded(d, tag, genes, recs, tool="count", R=50, n_comment=len(SAM_HEADER)):
    iv, mp = write_annotation(d, tag + "_u", genes)
    path = os.path.join(d, tag + "_u.mrf")
    with open(path, "w") as f:
        f.write(input_mrf([r for r in recs], n_comment))
    argv = ["0", "x", "./", "LH_GENE_TXT", iv, "UCSC_GENE2ISOFORM", mp, "0", "1000000", "MRF_SINGLE", "SHORT_READ", str(R), path]
    rc, text, _ = ob.run(tool, argv + (["1000000"] if tool == "solve" else []))
    assert rc == 0
    return text, ob.last_n_loaded[0], argv


def report_of(recs, lib, retained):
    t = [r.t(lib) for r in recs]
    return (t.count(0), t.count(1), t.count(None), retained[0], retained[1])


# ---- the small case --------------------------------------------------------------------------------------------------------
def small_genes():
    host_first, host_last = (8000, 8100), (8800, 8900)
    return [
        # an antisense pair whose exons overlap
        Gene("g01", "chrA", "+", [("g01.a", [(1000, 1200), (1500, 1700), (2000, 2200)]), ("g01.b", [(1000, 1200), (2000, 2200)])]),
        Gene("g02", "chrA", "-", [("g02.a", [(1100, 1300), (1600, 1800)]), ("g02.b", [(1100, 1300), (1700, 1800)])]),
        # a plus exon abutting a minus exon: [5000, 5100) | [5100, 5200)
        Gene("g03", "chrA", "+", [("g03.a", [(5000, 5100), (5300, 5400)]), ("g03.b", [(5000, 5100), (5350, 5400)])]),
        Gene("g04", "chrA", "-", [("g04.a", [(5100, 5200), (5500, 5600)]), ("g04.b", [(5100, 5200), (5550, 5600)])]),
        # beyond the kernels' limits (7 isoforms): a bucket the host evaluates
        Gene("g05", "chrA", "+", [("g05.%d" % i, [host_first, (8200 + 60 * i, 8250 + 60 * i), host_last]) for i in range(7)]),
        # five exons: reads of four blocks
        Gene("g06", "chrA", "-", [("g06.a", [(12000 + 100 * i, 12050 + 100 * i) for i in range(5)]),
                                  ("g06.b", [(12000 + 100 * i, 12050 + 100 * i) for i in (0, 1, 3, 4)])]),
        # a chromosome with genes of one strand only
        Gene("g07", "chrB", "+", [("g07.a", [(100, 300), (500, 700)]), ("g07.b", [(100, 300), (600, 700)])]),
        Gene("g08", "chrB", "+", [("g08.a", [(2000, 2200), (2400, 2600)]), ("g08.b", [(2000, 2200), (2450, 2600)])]),
    ]


FLAGS = (0, 16, 0x41, 0x51, 0x81, 0x91)      # single-end, first mate, second mate: each on either strand

UNION_ONLY = Rec("chrA", 0, [(5080, 5120)])      # inside [5000, 5200), the union of the abutting exons, and inside neither exon


def reads_along(rng, exons, n_blocks, L=40):
    """a read of n_blocks blocks that follows consecutive exons: the tail of the first, whole ones between, the head of the last"""
    if n_blocks == 1:
        s, e = rng.choice(exons)
        a = rng.randrange(s, max(e - L, s) + 1)
        return [(a, min(a + L, e))]
    k = rng.randrange(0, len(exons) - n_blocks + 1)
    run = exons[k:k + n_blocks]
    cut_a, cut_b = rng.randrange(5, 30), rng.randrange(5, 30)
    return [(run[0][1] - cut_a, run[0][1])] + list(run[1:-1]) + [(run[-1][0], run[-1][0] + cut_b)]


def small_records(seed=11, n=300):
    rng = random.Random(seed)
    genes = small_genes()
    recs = [
        # span-start ties: a read whose first base is the first base of an event's span, on either strand
        Rec("chrA", 0, [(1000, 1040)]), Rec("chrA", 16, [(1000, 1040)]), Rec("chrA", 16, [(1100, 1140)]), Rec("chrA", 0x91, [(1100, 1140)]),
        Rec("chrA", 0, [(8000, 8040)]), Rec("chrA", 0x81, [(12000, 12040)]),
        UNION_ONLY, Rec("chrA", 16, [(5080, 5120)]),
        # a chromosome the annotation lacks
        Rec("chrC", 0, [(100, 140)]), Rec("chrC", 16, [(300, 320), (400, 420)]),
    ]
    while len(recs) < n:
        g = rng.choice(genes)
        _, exons = rng.choice(g.isoforms)
        nb = rng.choice([1, 1, 2, 2, 4] if len(exons) >= 4 else [1, 1, 2] if len(exons) >= 2 else [1])
        # mostly the gene's own strand in a forward library, some antisense
        flag = rng.choice(FLAGS)
        recs.append(Rec(g.chrom, flag, reads_along(rng, exons, nb)))
    return genes, recs


def mrf_only_records():
    """records only an MRF file can hold: strand columns that are no strand"""
    return [Rec("chrA", 0, [(1010, 1050)], mrf_strand="."), Rec("chrB", 0, [(120, 160)], mrf_strand="*"), Rec("chrA", 0, [(5010, 5050)], mrf_strand="+-")]


def write_inputs(d, tag, genes, recs, header=SAM_HEADER, bam_layout="htslib"):
    """the job's annotation and its read files: the SAM text, its BAM, the MRF form"""
    iv, mp = write_annotation(d, tag, genes)
    sam = os.path.join(d, tag + ".sam")
    text = sam_text([r for r in recs if r.mrf_strand is None], header).encode()
    with open(sam, "wb") as f:
        f.write(text)
    bam = os.path.join(d, tag + ".bam")
    with open(bam, "wb") as f:
        f.write(sam_to_bam(text, bam_layout))
    mrf = os.path.join(d, tag + ".mrf")
    with open(mrf, "w") as f:
        f.write(input_mrf(recs, len(header)))
    return {"interval": iv, "map": mp, "sam": sam, "bam": bam, "mrf": mrf}


def argv_of(paths, fmt, R=50, solve=False):
    key = {"MRF_SINGLE": "mrf", "SAM_SINGLE": "sam", "BAM_SINGLE": "bam"}[fmt]
    a = ["0", "x", "./", "LH_GENE_TXT", paths["interval"], "UCSC_GENE2ISOFORM", paths["map"], "0", "1000000", fmt, "SHORT_READ", str(R), paths[key]]
    return a + (["1000000"] if solve else [])
