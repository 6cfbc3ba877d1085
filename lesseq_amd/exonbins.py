"""Reads per exon bin and per gene of a read file (include/lesseq_hip.h, lsq_xb_*): a gene's exons cut at every exon
boundary into disjoint bins, the reads that overlap each bin and each gene -- the count table `test_as lrt --tables` reads.  The
device path parses the file and counts on the GPU; the host path runs from the host parsers and touches no GPU."""
import ctypes as C

import numpy as np

from ._lib import lib, check, vp, u64, u32, i64, P

PHASES = ("index_upload", "count", "copy_back")
REPORT = ("reads", "blocks", "no_chromosome_or_empty", "no_gene", "several_genes", "bin_hits")


def _b(s):
    return s.encode() if isinstance(s, str) else s


class ExonBins:
    """The table of one read file: numpy arrays (copies) `reads` per bin and `total` per gene, `report`, `times` (device ms per
    phase), rows(), text(), bins_text()."""

    def __init__(self, h, index):
        self.h = h
        self.index = index
        nb, ng = index.num_bins, index.num_genes
        reads, total = P(u64)(), P(u64)()
        check(lib.lsq_xb_table_arrays(h, C.byref(reads), C.byref(total)))
        self.reads = np.ctypeslib.as_array(reads, (nb,)).copy() if nb else np.zeros(0, np.uint64)
        self.total = np.ctypeslib.as_array(total, (ng,)).copy() if ng else np.zeros(0, np.uint64)
        rep = (u64 * 6)()
        check(lib.lsq_xb_table_report(h, rep))
        self.report = dict(zip(REPORT, (int(v) for v in rep)))
        ms = (C.c_float * 3)()
        check(lib.lsq_xb_table_times(h, ms))
        self.times = dict(zip(PHASES, (float(v) for v in ms)))

    def __del__(self, _free=lib.lsq_xb_table_free):
        if getattr(self, "h", None):
            _free(self.h)
            self.h = None

    def __len__(self):
        return len(self.reads)

    def rows(self):
        """[(gene, total[gene], gene:k, reads[bin])] in table order"""
        names, first = self.index.gene_names(), self.index.gene_first_bin
        return [(names[g], int(self.total[g]), "%s:%d" % (names[g], b - int(first[g]) + 1), int(self.reads[b]))
                for g in range(len(names)) for b in range(int(first[g]), int(first[g + 1]))]

    def text(self):
        out = vp()
        check(lib.lsq_xb_format(self.h, C.byref(out)))
        try:
            return C.string_at(out).decode()
        finally:
            lib.lsq_free(out)

    def bins_text(self):
        return self.index.bins_text()


class ExonBinIndex:
    """lsq_xb_index_build: the annotation's chromosomes, every gene's bins, the lookup of the bins that overlap a block"""

    def __init__(self, annotation):
        h = vp()
        check(lib.lsq_xb_index_build(annotation.h, C.byref(h)))
        self.h = h
        nb, ng = self.num_bins, self.num_genes
        ptrs = [P(i64)(), P(i64)(), P(u32)(), P(u32)(), P(u32)()]
        check(lib.lsq_xb_index_arrays(h, *[C.byref(p) for p in ptrs]))
        for (k, dt, n), p in zip((("bin_start", np.int64, nb), ("bin_end", np.int64, nb), ("bin_gene", np.uint32, nb), ("gene_first_bin", np.uint32, ng + 1),
                                  ("gene_chrom", np.uint32, ng)), ptrs):
            setattr(self, k, np.ctypeslib.as_array(p, (n,)).copy() if n else np.zeros(0, dt))

    def __del__(self, _free=lib.lsq_xb_index_free):
        if getattr(self, "h", None):
            _free(self.h)
            self.h = None

    @property
    def num_chroms(self):
        return lib.lsq_xb_index_num_chroms(self.h)

    @property
    def num_genes(self):
        return lib.lsq_xb_index_num_genes(self.h)

    @property
    def num_bins(self):
        return lib.lsq_xb_index_num_bins(self.h)

    def chrom_names(self):
        return [lib.lsq_xb_index_chrom_name(self.h, c).decode() for c in range(self.num_chroms)]

    def gene_names(self):
        return [lib.lsq_xb_index_gene_name(self.h, g).decode() for g in range(self.num_genes)]

    def gene_strands(self):
        return [lib.lsq_xb_index_gene_strand(self.h, g).decode() for g in range(self.num_genes)]

    def bins(self):
        """[(gene:k, chromosome name, strand, start, end)] in table order"""
        names, chroms, strands = self.gene_names(), self.chrom_names(), self.gene_strands()
        return [("%s:%d" % (names[g], b - int(self.gene_first_bin[g]) + 1), chroms[self.gene_chrom[g]], strands[g], int(self.bin_start[b]), int(self.bin_end[b]))
                for g in range(len(names)) for b in range(int(self.gene_first_bin[g]), int(self.gene_first_bin[g + 1]))]

    def bins_text(self):
        """(the LH_GENE_TXT text with a line per bin, the gene->isoform text): the bins as an annotation"""
        iv, mp = vp(), vp()
        check(lib.lsq_xb_format_bins(self.h, C.byref(iv), C.byref(mp)))
        try:
            return C.string_at(iv).decode(), C.string_at(mp).decode()
        finally:
            lib.lsq_free(iv)
            lib.lsq_free(mp)

    def host(self, read_format, path, skip_flags=0x904, min_mapq=0, n_threads=0):
        """lsq_xb_host: every read format lsq_reads_parse takes; no GPU touched"""
        t = vp()
        check(lib.lsq_xb_host(self.h, _b(read_format), _b(path), skip_flags, min_mapq, n_threads, C.byref(t)))
        return ExonBins(t, self)

    def parse_host(self, read_format, path, n_threads=0):
        """lsq_reads_parse against the index's dictionaries: an api.Reads for host_reads"""
        from .api import Reads

        class _Dictionaries:
            h = vp(lib.lsq_xb_index_dictionaries(self.h))
        return Reads.from_mrf(path, _Dictionaries, n_threads, read_format)

    def host_reads(self, reads, n_threads=0):
        """lsq_xb_host_reads: from arrays already parsed against this index (parse_host)"""
        t = vp()
        check(lib.lsq_xb_host_reads(self.h, reads.h, n_threads, C.byref(t)))
        return ExonBins(t, self)

    def device(self, ctx, read_format, path):
        """lsq_xb_device: MRF_SINGLE, SAM_SINGLE or BAM_SINGLE under the context's sam_skip_flags / sam_min_mapq / bam_verify"""
        t = vp()
        check(lib.lsq_xb_device(ctx.h, self.h, _b(read_format), _b(path), C.byref(t)))
        return ExonBins(t, self)


__all__ = ["ExonBinIndex", "ExonBins", "PHASES", "REPORT"]
