"""What the tools that take an annotation and a read file share (junctions, coverage, exonbins, psi, evidence, sites, retention): the handle of an index with its
chromosome dictionary and host parse, the handle of a table with its report and phase times.  A subclass names its entry points'
prefix (`lsq_jn`: lsq_jn_index_build, lsq_jn_table_report, ...) and keeps what is its own."""
import ctypes as C

import numpy as np

from ._lib import lib, check, vp, u64, _b

LIBRARIES = ("unstranded", "forward", "reverse")
LIBRARY_REPORT = ("plus", "minus", "no_strand", "plus_counted", "minus_counted")


def copied(ptr, n, dtype):
    """n items behind a ctypes pointer as a numpy array of its own (n == 0: an empty one of `dtype`)"""
    return np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dtype)


class _Handle:
    PREFIX = KIND = None      # the entry points are lsq_<PREFIX>_<KIND>_<name>

    @classmethod
    def _entry(cls, name):
        return getattr(lib, "%s_%s_%s" % (cls.PREFIX, cls.KIND, name))

    def __init_subclass__(cls):
        if cls.PREFIX and cls.KIND:
            cls._free = cls._entry("free")      # (bound now: the module's globals may be gone when the last handle is)

    def __del__(self):
        if getattr(self, "h", None):
            self._free(self.h)
            self.h = None


class Table(_Handle):
    KIND = "table"

    def __init__(self, h, index, report, phases):
        self.h = h
        self.index = index
        rep = (u64 * len(report))()
        check(self._entry("report")(h, rep))
        self.report = dict(zip(report, (int(v) for v in rep)))
        ms = (C.c_float * len(phases))()
        check(self._entry("times")(h, ms))
        self.times = dict(zip(phases, (float(v) for v in ms)))

    def library_report(self):
        """lsq_*_table_library_report of a stranded table: reads with transcript strand +, with -, without one, and of the first two
        those that counted for a gene or event.  LsqError (LSQ_E_STATE) for the table of an unstranded index."""
        rep = (u64 * len(LIBRARY_REPORT))()
        check(self._entry("library_report")(self.h, rep))
        return dict(zip(LIBRARY_REPORT, (int(v) for v in rep)))


class Index(_Handle):
    KIND = "index"

    def __init__(self, annotation, library="unstranded"):
        """library: "unstranded" (the default), "forward" or "reverse" -- stranded counting (lsq_*_index_build_library), for the
        tools that have it"""
        h = vp()
        if library == "unstranded":
            check(self._entry("build")(annotation.h, C.byref(h)))
        else:
            code = lib.lsq_library_from_name(_b(library))
            if code < 0:
                raise ValueError("library is 'unstranded', 'forward' or 'reverse', not %r" % (library,))
            if not hasattr(lib, "%s_index_build_library" % self.PREFIX):
                raise ValueError("%s counts without regard to strand: it takes no library type" % type(self).__name__)
            check(self._entry("build_library")(annotation.h, code, C.byref(h)))
        self.h = h

    @property
    def library(self):
        """the index's library type; "unstranded" for the tools that have no stranded counting"""
        return LIBRARIES[self._entry("library")(self.h)] if hasattr(lib, "%s_index_library" % self.PREFIX) else "unstranded"

    @property
    def num_chroms(self):
        return self._entry("num_chroms")(self.h)

    def chrom_names(self):
        name = self._entry("chrom_name")
        return [name(self.h, c).decode() for c in range(self.num_chroms)]

    def parse_host(self, read_format, path, n_threads=0):
        """lsq_reads_parse against the index's dictionaries: an api.Reads for host_reads"""
        from .api import Reads

        class _Dictionaries:
            h = vp(self._entry("dictionaries")(self.h))
        return Reads.from_mrf(path, _Dictionaries, n_threads, read_format)

    def _table(self, cls, call, *args):
        """call(*args, a new table): the table as a `cls`"""
        t = vp()
        check(call(*args, C.byref(t)))
        return cls(t, self)
