"""Intron retention of a read file (include/lesseq_hip.h, lsq_ir_*): per intron of the annotation its sites row --
the spliced reads, the spliced reads of its two splice sites, the blocks that run through either -- and the depth over the bases of
its body that lie in no exon: clean and covered bases, the depth sum and the order statistics q25, q50, q75.  The device path
parses the file once, runs the sites and the coverage passes and selects the order statistics from the depth rows on the GPU; the
host path runs from the host parsers and touches no GPU."""
import ctypes as C

import numpy as np

from ._lib import lib, check, u32, i32, u8, u64, P, _b, take_text
from ._readtool import Index, Table, copied

PHASES = ("sites", "depth", "index", "select", "copy_back")
REPORT = ("reads", "blocks", "occurrences", "dropped_overhang", "no_chromosome", "boundaries", "through", "unsupported", "introns", "no_clean", "pieces", "depth_rows",
          "bases")
COLUMNS = (("chrom", np.uint32), ("start", np.int32), ("end", np.int32), ("ann", np.uint8), ("reads", np.uint64), ("left_spliced", np.uint64), ("left_through", np.uint64),
           ("right_spliced", np.uint64), ("right_through", np.uint64), ("clean", np.uint64), ("covered", np.uint64), ("depth_sum", np.uint64), ("q25", np.uint32),
           ("q50", np.uint32), ("q75", np.uint32))
_CTYPES = {np.uint32: u32, np.int32: i32, np.uint8: u8, np.uint64: u64}


class Retention(Table):
    """A retention table: numpy arrays (copies) in row order, `report`, `times` (device ms per phase), text()."""
    PREFIX = "lsq_ir"

    def __init__(self, h, index):
        super().__init__(h, index, REPORT, PHASES)
        n = lib.lsq_ir_table_rows(h)
        ptrs = [P(_CTYPES[dt])() for _, dt in COLUMNS]
        check(lib.lsq_ir_table_arrays(h, *[C.byref(p) for p in ptrs]))
        for (k, dt), p in zip(COLUMNS, ptrs):
            setattr(self, k, copied(p, n, dt))

    def __len__(self):
        return len(self.chrom)

    def rows(self):
        """[(chromosome name, start, end, ann, reads, left_spliced, left_through, right_spliced, right_through, clean, covered,
        depth_sum, q25, q50, q75)] in row order"""
        names = self.index.chrom_names()
        cols = [getattr(self, k) for k, _ in COLUMNS]
        return [(names[r[0]], int(r[1]), int(r[2]), chr(r[3])) + tuple(int(v) for v in r[4:]) for r in zip(*cols)]

    def text(self, ratios=False):
        return take_text(lib.lsq_ir_format, self.h, int(bool(ratios)))


class RetentionIndex(Index):
    """lsq_ir_index_build: the annotation's chromosomes, its distinct introns (the sites index) and every chromosome's exons"""
    PREFIX = "lsq_ir"

    @property
    def num_introns(self):
        return lib.lsq_ir_index_num_introns(self.h)

    def host(self, read_format, path, min_overhang=1, skip_flags=0x904, min_mapq=0, n_threads=0):
        """lsq_ir_host: every read format lsq_reads_parse takes; no GPU touched"""
        return self._table(Retention, lib.lsq_ir_host, self.h, _b(read_format), _b(path), skip_flags, min_mapq, min_overhang, n_threads)

    def host_reads(self, reads, min_overhang=1, n_threads=0):
        """lsq_ir_host_reads: from arrays already parsed against this index (parse_host)"""
        return self._table(Retention, lib.lsq_ir_host_reads, self.h, reads.h, min_overhang, n_threads)

    def device(self, ctx, read_format, path, min_overhang=1):
        """lsq_ir_device: MRF_SINGLE, SAM_SINGLE or BAM_SINGLE under the context's sam_skip_flags / sam_min_mapq / bam_verify"""
        return self._table(Retention, lib.lsq_ir_device, ctx.h, self.h, _b(read_format), _b(path), min_overhang)


__all__ = ["RetentionIndex", "Retention", "PHASES", "REPORT"]
