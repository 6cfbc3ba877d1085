"""Junction and exon-body reads per event form of a read file (include/lesseq_hip.h, lsq_fe_*): per form the reads
that cross an intron which tells the forms of a local event apart or that lie on exon bases not every form of the event has, per
event the reads that do either -- the junction counts plus exon counts of rMATS, and a count table `test_as fisher --tables` and
`test_as lrt --tables` read.  Where `psi` prints NA for a retained intron, this tool counts the reads inside it.  The device path
parses the file and counts on the GPU; the host path runs from the host parsers and touches no GPU."""
import ctypes as C

import numpy as np

from ._lib import lib, check, u64, u32, P, _b, take_text
from ._readtool import Index, Table, copied

PHASES = ("index_upload", "count", "copy_back")
REPORT = ("reads", "blocks", "occurrences", "dropped_overhang", "no_chromosome", "informative_occurrences", "skipped_blocks", "body_hits", "counted", "several_events",
          "counted_by_body_alone")


class Evidence(Table):
    """The table of one read file: numpy arrays (copies) `reads` per form and `total` per event, `report`, `times` (device ms per
    phase), rows(), text(psi=False, read_length=None), psi(read_length)."""
    PREFIX = "lsq_fe"

    def __init__(self, h, index):
        super().__init__(h, index, REPORT, PHASES)
        reads, total = P(u64)(), P(u64)()
        check(lib.lsq_fe_table_arrays(h, C.byref(reads), C.byref(total)))
        self.reads = copied(reads, index.num_forms, np.uint64)
        self.total = copied(total, index.num_events, np.uint64)

    def __len__(self):
        return len(self.reads)

    def rows(self):
        """[(event, total[event], form, reads[form])] in table order"""
        events, forms, first = self.index.event_names(), self.index.form_names(), self.index.event_first_form
        return [(events[e], int(self.total[e]), forms[f], int(self.reads[f])) for e in range(len(events)) for f in range(int(first[e]), int(first[e + 1]))]

    def text(self, psi=False, read_length=None):
        """four columns; with psi, under a read length, eight: introns, body, positions, psi"""
        if psi and read_length is None:
            raise ValueError("psi needs a read length")
        return take_text(lib.lsq_fe_format, self.h, 1 if psi else 0, read_length if psi else 0)

    def psi(self, read_length):
        """float64 per form: reads / positions over the event's sum of them, nan where the text prints NA"""
        out = np.zeros(len(self.reads), np.float64)
        check(lib.lsq_fe_table_psi(self.h, read_length, out.ctypes.data_as(P(C.c_double))))
        return out


class EvidenceIndex(Index):
    """lsq_fe_index_build: psi's index (events, forms, informative introns) and the informative body's regions with their lookup"""
    PREFIX = "lsq_fe"

    def __init__(self, annotation, library="unstranded"):
        super().__init__(annotation, library)
        first, introns, body = P(u32)(), P(u32)(), P(u64)()
        check(lib.lsq_fe_index_arrays(self.h, C.byref(first), C.byref(introns), C.byref(body)))
        self.event_first_form = copied(first, self.num_events + 1, np.uint32)
        self.form_introns = copied(introns, self.num_forms, np.uint32)
        self.form_body = copied(body, self.num_forms, np.uint64)

    @property
    def num_events(self):
        return lib.lsq_fe_index_num_events(self.h)

    @property
    def num_forms(self):
        return lib.lsq_fe_index_num_forms(self.h)

    @property
    def num_introns(self):
        return lib.lsq_fe_index_num_introns(self.h)

    @property
    def num_regions(self):
        return lib.lsq_fe_index_num_regions(self.h)

    def event_names(self):
        return [lib.lsq_fe_index_event_name(self.h, e).decode() for e in range(self.num_events)]

    def form_names(self):
        return [lib.lsq_fe_index_form_name(self.h, f).decode() for f in range(self.num_forms)]

    def positions(self, read_length, min_overhang=1, min_body=1):
        """uint64 per form: the starts of an ungapped read of that length along the form at which it counts for the form"""
        out = np.zeros(self.num_forms, np.uint64)
        check(lib.lsq_fe_index_positions(self.h, read_length, min_overhang, min_body, out.ctypes.data_as(P(u64))))
        return out

    def host(self, read_format, path, skip_flags=0x904, min_mapq=0, min_overhang=1, min_body=1, n_threads=0):
        """lsq_fe_host: every read format lsq_reads_parse takes; no GPU touched"""
        return self._table(Evidence, lib.lsq_fe_host, self.h, _b(read_format), _b(path), skip_flags, min_mapq, min_overhang, min_body, n_threads)

    def host_reads(self, reads, min_overhang=1, min_body=1, n_threads=0):
        """lsq_fe_host_reads: from arrays already parsed against this index (parse_host)"""
        return self._table(Evidence, lib.lsq_fe_host_reads, self.h, reads.h, min_overhang, min_body, n_threads)

    def device(self, ctx, read_format, path, min_overhang=1, min_body=1):
        """lsq_fe_device: MRF_SINGLE, SAM_SINGLE or BAM_SINGLE under the context's sam_skip_flags / sam_min_mapq / bam_verify"""
        return self._table(Evidence, lib.lsq_fe_device, ctx.h, self.h, _b(read_format), _b(path), min_overhang, min_body)


__all__ = ["EvidenceIndex", "Evidence", "PHASES", "REPORT"]
