"""Which library type is this read file? (include/lesseq_hip.h, lsq_lt_*): reads classed by the strand of their
fragment's first mate and by whether they lie on exons of plus genes, of minus genes, of both or of none; the fraction that is
sense, and the verdict `--library` of exonbins, psi and evidence wants.  The device path parses the file and counts on the GPU;
the host path runs from the host parsers and touches no GPU."""
import ctypes as C

from ._lib import lib, check, u64, cs, _b, take_text
from ._readtool import Index, _Handle

PHASES = ("index_upload", "count", "copy_back")
COUNTS = ("reads", "no_strand", "plus_none", "plus_plus", "plus_minus", "plus_both", "minus_none", "minus_plus", "minus_minus", "minus_both", "unplaced_genes")


class LibType(_Handle):
    """The result for one read file: `counts` (dict: COUNTS, and the derived sense, antisense, ambiguous, no_gene),
    `forward_fraction` (None when no read is sense or antisense), `library` ("forward", "reverse", "unstranded" or
    "undetermined"), `times` (device ms per phase), text()."""
    PREFIX, KIND = "lsq_lt", "table"

    def __init__(self, h, index):
        self.h = h
        self.index = index
        raw = (u64 * len(COUNTS))()
        check(lib.lsq_lt_table_counts(h, raw))
        c = dict(zip(COUNTS, (int(v) for v in raw)))
        c["sense"] = c["plus_plus"] + c["minus_minus"]
        c["antisense"] = c["plus_minus"] + c["minus_plus"]
        c["ambiguous"] = c["plus_both"] + c["minus_both"]
        c["no_gene"] = c["plus_none"] + c["minus_none"]
        self.counts = c
        f, has, name = C.c_double(), C.c_int(), cs()
        check(lib.lsq_lt_table_verdict(h, C.byref(f), C.byref(has), C.byref(name)))
        self.forward_fraction = f.value if has.value else None
        self.library = name.value.decode()
        ms = (C.c_float * len(PHASES))()
        check(lib.lsq_lt_table_times(h, ms))
        self.times = dict(zip(PHASES, (float(v) for v in ms)))

    def text(self):
        return take_text(lib.lsq_lt_format, self.h)


class LibTypeIndex(Index):
    """lsq_lt_index_build: the annotation's chromosomes and, per chromosome and strand, the union of the exons of that strand's genes"""
    PREFIX = "lsq_lt"

    def __init__(self, annotation):
        super().__init__(annotation)

    @property
    def num_intervals(self):
        return lib.lsq_lt_index_num_intervals(self.h)

    @property
    def unplaced_genes(self):
        return lib.lsq_lt_index_unplaced_genes(self.h)

    def host(self, read_format, path, skip_flags=0x904, min_mapq=0, n_threads=0):
        """lsq_lt_host: every read format lsq_reads_parse takes; no GPU touched"""
        return self._table(LibType, lib.lsq_lt_host, self.h, _b(read_format), _b(path), skip_flags, min_mapq, n_threads)

    def host_reads(self, reads, n_threads=0):
        """lsq_lt_host_reads: from arrays already parsed against this index (parse_host)"""
        return self._table(LibType, lib.lsq_lt_host_reads, self.h, reads.h, n_threads)

    def device(self, ctx, read_format, path):
        """lsq_lt_device: MRF_SINGLE, SAM_SINGLE or BAM_SINGLE under the context's sam_skip_flags / sam_min_mapq / bam_verify"""
        return self._table(LibType, lib.lsq_lt_device, ctx.h, self.h, _b(read_format), _b(path))


__all__ = ["LibTypeIndex", "LibType", "PHASES", "COUNTS"]
