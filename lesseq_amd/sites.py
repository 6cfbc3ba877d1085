"""Splice-site usage and read-through per junction of a read file (include/lesseq_hip.h, lsq_ss_*): per junction of
the file and per intron of the annotation the spliced reads, the spliced reads of its two splice sites whatever their partner,
and the blocks that run straight through either site.  The device path parses the file, makes the junction rows and counts the
boundaries on the GPU; the host path runs from the host parsers and touches no GPU."""
import ctypes as C

import numpy as np

from ._lib import lib, check, u32, i32, u8, u64, P, _b, take_text
from ._readtool import Index, Table, copied

LDS_SLOTS = lib.lsq_ss_lds_slots()      # boundary ids a workgroup of the device count keeps in LDS
PHASES = ("junctions", "index", "through", "copy_back")
REPORT = ("reads", "blocks", "occurrences", "dropped_overhang", "no_chromosome", "boundaries", "through", "unsupported")


class Sites(Table):
    """A sites table: numpy arrays (copies) in row order, `report`, `times` (device ms per phase), text()."""
    PREFIX = "lsq_ss"

    def __init__(self, h, index):
        super().__init__(h, index, REPORT, PHASES)
        n = lib.lsq_ss_table_rows(h)
        ptrs = [P(u32)(), P(i32)(), P(i32)(), P(u8)(), P(u64)(), P(u64)(), P(u64)(), P(u64)(), P(u64)()]
        check(lib.lsq_ss_table_arrays(h, *[C.byref(p) for p in ptrs]))
        names = (("chrom", np.uint32), ("start", np.int32), ("end", np.int32), ("ann", np.uint8), ("reads", np.uint64), ("left_spliced", np.uint64),
                 ("left_through", np.uint64), ("right_spliced", np.uint64), ("right_through", np.uint64))
        for (k, dt), p in zip(names, ptrs):
            setattr(self, k, copied(p, n, dt))

    def __len__(self):
        return len(self.chrom)

    def rows(self):
        """[(chromosome name, start, end, ann, reads, left_spliced, left_through, right_spliced, right_through)] in row order"""
        names = self.index.chrom_names()
        return [(names[c], int(s), int(e), chr(a), int(r), int(ls), int(lt), int(rs), int(rt)) for c, s, e, a, r, ls, lt, rs, rt in
                zip(self.chrom, self.start, self.end, self.ann, self.reads, self.left_spliced, self.left_through, self.right_spliced, self.right_through)]

    def text(self, min_reads=0, novel_only=False, ratios=False):
        return take_text(lib.lsq_ss_format, self.h, min_reads, int(bool(novel_only)), int(bool(ratios)))


class SiteIndex(Index):
    """lsq_ss_index_build: the annotation's chromosomes and its distinct introns (the junction index)"""
    PREFIX = "lsq_ss"

    @property
    def num_introns(self):
        return lib.lsq_ss_index_num_introns(self.h)

    def host(self, read_format, path, min_overhang=1, skip_flags=0x904, min_mapq=0, n_threads=0):
        """lsq_ss_host: every read format lsq_reads_parse takes; no GPU touched"""
        return self._table(Sites, lib.lsq_ss_host, self.h, _b(read_format), _b(path), skip_flags, min_mapq, min_overhang, n_threads)

    def host_reads(self, reads, min_overhang=1, n_threads=0):
        """lsq_ss_host_reads: from arrays already parsed against this index (parse_host)"""
        return self._table(Sites, lib.lsq_ss_host_reads, self.h, reads.h, min_overhang, n_threads)

    def device(self, ctx, read_format, path, min_overhang=1):
        """lsq_ss_device: MRF_SINGLE, SAM_SINGLE or BAM_SINGLE under the context's sam_skip_flags / sam_min_mapq / bam_verify"""
        return self._table(Sites, lib.lsq_ss_device, ctx.h, self.h, _b(read_format), _b(path), min_overhang)


__all__ = ["SiteIndex", "Sites", "LDS_SLOTS", "PHASES", "REPORT"]
