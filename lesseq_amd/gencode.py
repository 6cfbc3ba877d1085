"""Annotation from GTF: what the reference's bin/parseGencode and bin/gencodeIsoformMap do (include/lesseq_hip.h,
lsq_gtf_*).  The GTF is parsed on the device -- fields, the `exon` filter, coordinates, gene_id / transcript_id -- and the
transcripts come back ordered as parseGencode prints them; gencodeIsoformMap's counter is host-only."""
import ctypes as C

import numpy as np

from ._lib import lib, check, vp, _b


class Gtf:
    """The transcripts of a GTF in parseGencode's output order (gene id, then transcript id, bytewise)."""

    def __init__(self, h):
        self.h = h

    def __del__(self, _free=lib.lsq_gtf_free):
        if getattr(self, "h", None):
            _free(self.h)
            self.h = None

    @property
    def num_transcripts(self):
        return lib.lsq_gtf_num_transcripts(self.h)

    @property
    def num_genes(self):
        return lib.lsq_gtf_num_genes(self.h)

    @property
    def num_exon_lines(self):
        return lib.lsq_gtf_num_exon_lines(self.h)

    def __len__(self):
        return self.num_transcripts

    def name(self, i):
        """b"<gene_id>|<transcript_id>" """
        return self._str(lib.lsq_gtf_transcript_name, i)

    def chrom(self, i):
        return self._str(lib.lsq_gtf_transcript_chrom, i)

    def strand(self, i):
        return self._str(lib.lsq_gtf_transcript_strand, i)

    def _str(self, f, i):
        s = f(self.h, i)
        if s is None:
            raise IndexError(i)
        return s

    def exons(self, i):
        """(starts, ends) of transcript i as int32 arrays (copies): field 4 minus 1 and field 5, each sorted on its own"""
        s, e = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        n = lib.lsq_gtf_transcript_exons(self.h, i, C.byref(s), C.byref(e))
        if n < 0:
            raise IndexError(i)
        return np.ctypeslib.as_array(s, (n,)).copy(), np.ctypeslib.as_array(e, (n,)).copy()

    def format(self):
        """(interval text, map text) as bytes: parseGencode's output and gencodeIsoformMap's on its first column"""
        a, b = vp(), vp()
        check(lib.lsq_gtf_format(self.h, C.byref(a), C.byref(b)))
        try:
            return C.string_at(a), C.string_at(b)
        finally:
            lib.lsq_free(a)
            lib.lsq_free(b)

    def times_ms(self):
        """HIP-event milliseconds: copy to HBM, newline scan, parse kernels, download"""
        ms = (C.c_double * 4)()
        check(lib.lsq_gtf_result_times(self.h, ms))
        return list(ms)


def parse_gtf(ctx, source):
    """source: a path (str) or the GTF's bytes"""
    h = vp()
    if isinstance(source, (bytes, bytearray, memoryview)):
        data = bytes(source)
        check(lib.lsq_gtf_parse_text(ctx.h, data, len(data), C.byref(h)))
    else:
        check(lib.lsq_gtf_parse(ctx.h, _b(source), C.byref(h)))
    return Gtf(h)


def isoform_map(names):
    """gencodeIsoformMap on a name list (bytes or str): bytes of the map.  No GPU is touched."""
    data = _b(names)
    out = vp()
    check(lib.lsq_gtf_isoform_map(data, len(data), C.byref(out)))
    try:
        return C.string_at(out)
    finally:
        lib.lsq_free(out)


__all__ = ["Gtf", "parse_gtf", "isoform_map"]
