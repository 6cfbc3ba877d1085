"""Per-base read depth of a read file (include/lesseq_hip.h, lsq_cov_*): the bedGraph rows of constant depth and,
per isoform line of the annotation, the covered bases and the summed depth of its exons.  The device path parses the file and
extracts, sorts, scans and emits on the GPU; the host path runs from the host parsers and touches no GPU."""
import ctypes as C

import numpy as np

from ._lib import lib, check, u64, u32, i32, P, _b, take_text
from ._readtool import Index, Table, copied

SORT_TILE = lib.lsq_cov_sort_tile()     # records a workgroup of the device sort takes (two records per counted block)
PHASES = ("extract", "sort", "reduce_scan", "emit", "regions", "copy_back")
REPORT = ("reads", "blocks", "counted", "no_chromosome", "empty", "other_strand", "bases")


def _strand(s):
    if s in (None, "", 0):
        return 0
    if s in ("+", "-"):
        return ord(s)
    raise ValueError("strand must be None, '+' or '-'")


class Coverage(Table):
    """The tables of one read file: numpy arrays (copies) of the rows -- chrom, start, end, depth -- and of the regions -- region_chrom,
    bases, covered, depth_sum, with region_names and region_strands -- `report`, `times` (device ms per phase), text(), regions_text()."""
    PREFIX = "lsq_cov"

    def __init__(self, h, index):
        super().__init__(h, index, REPORT, PHASES)
        n = lib.lsq_cov_table_rows(h)
        ptrs = [P(u32)(), P(i32)(), P(i32)(), P(u32)()]
        check(lib.lsq_cov_table_arrays(h, *[C.byref(p) for p in ptrs]))
        for (k, dt), p in zip((("chrom", np.uint32), ("start", np.int32), ("end", np.int32), ("depth", np.uint32)), ptrs):
            setattr(self, k, copied(p, n, dt))
        m = lib.lsq_cov_table_regions(h)
        ptrs = [P(u32)(), P(u64)(), P(u64)(), P(u64)()]
        check(lib.lsq_cov_table_region_arrays(h, *[C.byref(p) for p in ptrs]))
        for (k, dt), p in zip((("region_chrom", np.uint32), ("bases", np.uint64), ("covered", np.uint64), ("depth_sum", np.uint64)), ptrs):
            setattr(self, k, copied(p, m, dt))
        self.region_names = [lib.lsq_cov_table_region_name(h, r).decode() for r in range(m)]
        self.region_strands = [lib.lsq_cov_table_region_strand(h, r).decode() for r in range(m)]

    def __len__(self):
        return len(self.chrom)

    def rows(self):
        """[(chromosome name, start, end, depth)] in row order"""
        names = self.index.chrom_names()
        return [(names[c], int(s), int(e), int(d)) for c, s, e, d in zip(self.chrom, self.start, self.end, self.depth)]

    def regions(self):
        """[(name, chromosome name, strand, bases, covered, depth_sum)] in the annotation's order"""
        names = self.index.chrom_names()
        return [(n, names[c], s, int(b), int(v), int(d)) for n, c, s, b, v, d in
                zip(self.region_names, self.region_chrom, self.region_strands, self.bases, self.covered, self.depth_sum)]

    def text(self, min_depth=0):
        """the bedGraph of the rows with depth >= min_depth"""
        return take_text(lib.lsq_cov_format, self.h, min_depth)

    def regions_text(self):
        return take_text(lib.lsq_cov_format_regions, self.h)


class CoverageIndex(Index):
    """lsq_cov_index_build: the annotation's chromosomes and the exon union of every isoform line"""
    PREFIX = "lsq_cov"

    @property
    def num_regions(self):
        return lib.lsq_cov_index_num_regions(self.h)

    def host(self, read_format, path, strand=None, min_depth=1, skip_flags=0x904, min_mapq=0, n_threads=0):
        """lsq_cov_host: every read format lsq_reads_parse takes; no GPU touched"""
        return self._table(Coverage, lib.lsq_cov_host, self.h, _b(read_format), _b(path), skip_flags, min_mapq, _strand(strand), min_depth, n_threads)

    def host_reads(self, reads, strand=None, min_depth=1, n_threads=0):
        """lsq_cov_host_reads: from arrays already parsed against this index (parse_host)"""
        return self._table(Coverage, lib.lsq_cov_host_reads, self.h, reads.h, _strand(strand), min_depth, n_threads)

    def device(self, ctx, read_format, path, strand=None, min_depth=1):
        """lsq_cov_device: MRF_SINGLE, SAM_SINGLE or BAM_SINGLE under the context's sam_skip_flags / sam_min_mapq / bam_verify"""
        return self._table(Coverage, lib.lsq_cov_device, ctx.h, self.h, _b(read_format), _b(path), _strand(strand), min_depth)


__all__ = ["CoverageIndex", "Coverage", "SORT_TILE", "PHASES", "REPORT"]
