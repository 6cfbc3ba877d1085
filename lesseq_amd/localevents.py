"""Local events of the pipeline's step 2 (bin/Events.r): the eight local-event annotations (ES RI A5SS A3SS MXE AFE ALE
T3) detected on the device from classify's splicing graphs (include/lesseq_hip.h, lsq_le_*).  Loading -- from a
directory of .matrix files plus the gene list, or from an annotation with classify done in memory -- is host-only;
Graphs.from_gtf starts from the GTF itself, which is parsed on the device."""
import ctypes as C

from ._lib import lib, check, vp, _b

TYPES = ("ES", "RI", "A5SS", "A3SS", "MXE", "AFE", "ALE", "T3")


class Record:
    """One .interval line: id, chrom, strand, start, end, exon count, exon starts, exon ends; counter is its .map
    counter (shared by the two forms of an event)."""
    __slots__ = ("counter", "id", "chrom", "strand", "start", "end", "n", "starts", "ends")

    def __init__(self, counter, iv_line):
        f = iv_line.split("\t")
        self.counter = counter
        self.id, self.chrom, self.strand = f[0], f[1], f[2]
        self.start, self.end, self.n = int(f[3]), int(f[4]), int(f[5])
        self.starts = [int(x) for x in f[6].split(",")]
        self.ends = [int(x) for x in f[7].split(",")]

    def __repr__(self):
        return "Record(%s, %s)" % (self.counter, self.id)


class Result:
    """Detected events of a Graphs; keeps the graphs alive (the result formats from them)."""

    def __init__(self, graphs, h):
        self.graphs, self.h = graphs, h

    def __del__(self, _free=lib.lsq_le_result_free):
        if getattr(self, "h", None):
            _free(self.h)
            self.h = None

    def num_events(self, t):
        return lib.lsq_le_num_events(self.h, TYPES.index(t))

    def events(self, t):
        """[(gene index, code)] of type t in the script's order (code: column i, or the block / form)"""
        g, c = C.c_int64(), C.c_int32()
        out = []
        for q in range(self.num_events(t)):
            check(lib.lsq_le_event(self.h, TYPES.index(t), q, C.byref(g), C.byref(c)))
            out.append((g.value, c.value))
        return out

    def text(self, t):
        """(interval text, map text) that Events.r appends for type t"""
        a, b = vp(), vp()
        check(lib.lsq_le_format(self.h, TYPES.index(t), C.byref(a), C.byref(b)))
        try:
            return C.string_at(a).decode(), C.string_at(b).decode()
        finally:
            lib.lsq_free(a)
            lib.lsq_free(b)

    def records(self):
        """{type: [Record, ...]}: two records per event, counters from 1 per type"""
        out = {}
        for t in TYPES:
            iv, mp = self.text(t)
            out[t] = [Record(m.split("\t", 1)[0], line) for line, m in zip(iv.splitlines(), mp.splitlines())]
        return out

    def times_ms(self):
        """HIP-event milliseconds: upload, count kernel + scan, emit kernel, download"""
        ms = (C.c_double * 4)()
        check(lib.lsq_le_result_times(self.h, ms))
        return list(ms)

    def write(self, out_prefix):
        """Append <out_prefix><TYPE>.interval / .map for every type with events (Events.r's append = T)"""
        check(lib.lsq_le_write(self.h, _b(out_prefix)))


class Graphs:
    """The splicing graphs Events.r walks, in its order."""

    def __init__(self, h):
        self.h = h

    def __del__(self, _free=lib.lsq_le_graphs_free):
        if getattr(self, "h", None):
            _free(self.h)
            self.h = None

    @classmethod
    def from_matrices(cls, matrix_prefix, group_file):
        h = vp()
        check(lib.lsq_le_load_matrices(_b(matrix_prefix), _b(group_file), C.byref(h)))
        return cls(h)

    @classmethod
    def from_annotation(cls, isoforms_path, g2i_path, isoform_format="LH_GENE_TXT", g2i_format="UCSC_GENE2ISOFORM"):
        h = vp()
        check(lib.lsq_le_load_annotation(_b(isoform_format), _b(isoforms_path), _b(g2i_format), _b(g2i_path), C.byref(h)))
        return cls(h)

    @classmethod
    def from_gtf(cls, ctx, gtf_path):
        """GTF -> annotation (parsed on the device, lesseq_amd.gencode) -> classify, all in memory: the graphs
        from_annotation makes from the two files parseGencode and gencodeIsoformMap write for the same GTF"""
        h = vp()
        check(lib.lsq_le_load_gtf(ctx.h, _b(gtf_path), C.byref(h)))
        return cls(h)

    def __len__(self):
        return lib.lsq_le_num_genes(self.h)

    def names(self):
        return [lib.lsq_le_gene_name(self.h, i).decode() for i in range(len(self))]

    def shape(self, i):
        n, k = C.c_int(), C.c_int()
        check(lib.lsq_le_gene_shape(self.h, i, C.byref(n), C.byref(k)))
        return n.value, k.value

    def positions(self, i):
        """pos[1..2N] of gene i (the digit runs of its matrix header), as a list"""
        p = C.POINTER(C.c_int32)()
        n = lib.lsq_le_gene_positions(self.h, i, C.byref(p))
        if n < 0:
            raise IndexError(i)
        return [p[j] for j in range(n)]

    def detect(self, ctx):
        h = vp()
        check(lib.lsq_le_detect(ctx.h, self.h, C.byref(h)))
        return Result(self, h)


def detect(ctx, graphs):
    return graphs.detect(ctx)


__all__ = ["TYPES", "Graphs", "Result", "Record", "detect"]
