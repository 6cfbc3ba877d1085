"""Splice junctions of a read file (include/lesseq_hip.h, lsq_jn_*): the table of junctions a library supports,
each row marked with what the annotation knows of it.  The device path parses the file and extracts, sorts, reduces and
annotates on the GPU; the host path runs from the host parsers and touches no GPU."""
import ctypes as C

import numpy as np

from ._lib import lib, check, u32, i32, u8, P, _b, take_text
from ._readtool import Index, Table, copied

SORT_TILE = lib.lsq_jn_sort_tile()      # records a workgroup of the device sort takes
PHASES = ("extract", "sort", "reduce", "annotate", "copy_back")
REPORT = ("reads", "blocks", "occurrences", "dropped_overhang", "no_chromosome")


class Junctions(Table):
    """A junction table: numpy arrays (copies) in row order, `report`, `times` (device ms per phase), text()."""
    PREFIX = "lsq_jn"

    def __init__(self, h, index):
        super().__init__(h, index, REPORT, PHASES)
        n = lib.lsq_jn_table_rows(h)
        ptrs = [P(u32)(), P(i32)(), P(i32)(), P(u8)(), P(u32)(), P(u32)(), P(u32)(), P(u32)()]
        check(lib.lsq_jn_table_arrays(h, *[C.byref(p) for p in ptrs]))
        names = (("chrom", np.uint32), ("start", np.int32), ("end", np.int32), ("ann", np.uint8), ("reads", np.uint32), ("plus", np.uint32),
                 ("minus", np.uint32), ("max_overhang", np.uint32))
        for (k, dt), p in zip(names, ptrs):
            setattr(self, k, copied(p, n, dt))

    def __len__(self):
        return len(self.chrom)

    def rows(self):
        """[(chromosome name, start, end, ann, reads, plus, minus, max_overhang)] in row order"""
        names = self.index.chrom_names()
        return [(names[c], int(s), int(e), chr(a), int(r), int(p), int(m), int(o)) for c, s, e, a, r, p, m, o in
                zip(self.chrom, self.start, self.end, self.ann, self.reads, self.plus, self.minus, self.max_overhang)]

    def text(self, min_reads=0, novel_only=False):
        return take_text(lib.lsq_jn_format, self.h, min_reads, int(bool(novel_only)))


class JunctionIndex(Index):
    """lsq_jn_index_build: the annotation's chromosomes and its distinct introns"""
    PREFIX = "lsq_jn"

    @property
    def num_introns(self):
        return lib.lsq_jn_index_num_introns(self.h)

    def host(self, read_format, path, min_overhang=1, skip_flags=0x904, min_mapq=0, n_threads=0):
        """lsq_jn_host: every read format lsq_reads_parse takes; no GPU touched"""
        return self._table(Junctions, lib.lsq_jn_host, self.h, _b(read_format), _b(path), skip_flags, min_mapq, min_overhang, n_threads)

    def host_reads(self, reads, min_overhang=1, n_threads=0):
        """lsq_jn_host_reads: from arrays already parsed against this index (parse_host)"""
        return self._table(Junctions, lib.lsq_jn_host_reads, self.h, reads.h, min_overhang, n_threads)

    def device(self, ctx, read_format, path, min_overhang=1):
        """lsq_jn_device: MRF_SINGLE, SAM_SINGLE or BAM_SINGLE under the context's sam_skip_flags / sam_min_mapq / bam_verify"""
        return self._table(Junctions, lib.lsq_jn_device, ctx.h, self.h, _b(read_format), _b(path), min_overhang)


__all__ = ["JunctionIndex", "Junctions", "SORT_TILE", "PHASES", "REPORT"]
