"""Reads per exon bin and per gene of a read file (include/lesseq_hip.h, lsq_xb_*): a gene's exons cut at every exon
boundary into disjoint bins, the reads that overlap each bin and each gene -- the count table `test_as lrt --tables` reads.  The
device path parses the file and counts on the GPU; the host path runs from the host parsers and touches no GPU."""
import ctypes as C

import numpy as np

from ._lib import lib, check, u64, u32, i64, P, _b, take_text
from ._readtool import Index, Table, copied

PHASES = ("index_upload", "count", "copy_back")
REPORT = ("reads", "blocks", "no_chromosome_or_empty", "no_gene", "several_genes", "bin_hits")


class ExonBins(Table):
    """The table of one read file: numpy arrays (copies) `reads` per bin and `total` per gene, `report`, `times` (device ms per
    phase), rows(), text(), bins_text()."""
    PREFIX = "lsq_xb"

    def __init__(self, h, index):
        super().__init__(h, index, REPORT, PHASES)
        reads, total = P(u64)(), P(u64)()
        check(lib.lsq_xb_table_arrays(h, C.byref(reads), C.byref(total)))
        self.reads = copied(reads, index.num_bins, np.uint64)
        self.total = copied(total, index.num_genes, np.uint64)

    def __len__(self):
        return len(self.reads)

    def rows(self):
        """[(gene, total[gene], gene:k, reads[bin])] in table order"""
        names, first = self.index.gene_names(), self.index.gene_first_bin
        return [(names[g], int(self.total[g]), "%s:%d" % (names[g], b - int(first[g]) + 1), int(self.reads[b]))
                for g in range(len(names)) for b in range(int(first[g]), int(first[g + 1]))]

    def text(self):
        return take_text(lib.lsq_xb_format, self.h)

    def bins_text(self):
        return self.index.bins_text()


class ExonBinIndex(Index):
    """lsq_xb_index_build: the annotation's chromosomes, every gene's bins, the lookup of the bins that overlap a block.
    library "forward" / "reverse" (lsq_xb_index_build_library): a read counts for the genes of its transcript strand alone"""
    PREFIX = "lsq_xb"

    def __init__(self, annotation, library="unstranded"):
        super().__init__(annotation, library)
        nb, ng = self.num_bins, self.num_genes
        ptrs = [P(i64)(), P(i64)(), P(u32)(), P(u32)(), P(u32)()]
        check(lib.lsq_xb_index_arrays(self.h, *[C.byref(p) for p in ptrs]))
        for (k, dt, n), p in zip((("bin_start", np.int64, nb), ("bin_end", np.int64, nb), ("bin_gene", np.uint32, nb), ("gene_first_bin", np.uint32, ng + 1),
                                  ("gene_chrom", np.uint32, ng)), ptrs):
            setattr(self, k, copied(p, n, dt))

    @property
    def num_genes(self):
        return lib.lsq_xb_index_num_genes(self.h)

    @property
    def num_bins(self):
        return lib.lsq_xb_index_num_bins(self.h)

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
        return take_text(lib.lsq_xb_format_bins, self.h, n=2)

    def host(self, read_format, path, skip_flags=0x904, min_mapq=0, n_threads=0):
        """lsq_xb_host: every read format lsq_reads_parse takes; no GPU touched"""
        return self._table(ExonBins, lib.lsq_xb_host, self.h, _b(read_format), _b(path), skip_flags, min_mapq, n_threads)

    def host_reads(self, reads, n_threads=0):
        """lsq_xb_host_reads: from arrays already parsed against this index (parse_host)"""
        return self._table(ExonBins, lib.lsq_xb_host_reads, self.h, reads.h, n_threads)

    def device(self, ctx, read_format, path):
        """lsq_xb_device: MRF_SINGLE, SAM_SINGLE or BAM_SINGLE under the context's sam_skip_flags / sam_min_mapq / bam_verify"""
        return self._table(ExonBins, lib.lsq_xb_device, ctx.h, self.h, _b(read_format), _b(path))


__all__ = ["ExonBinIndex", "ExonBins", "PHASES", "REPORT"]
