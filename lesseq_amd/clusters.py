"""Intron clusters of several read files (include/lesseq_hip.h, lsq_cl_*): the junction rows of all samples pooled,
introns that share a splice site joined into clusters, a count table per sample with the same rows in every one.  The device
path sorts, reduces, filters and finds the connected components on the GPU; the host path touches no GPU."""
import ctypes as C

import numpy as np

from ._lib import lib, check, vp, u64, u32, i32, u8, P, _b, take_text
from ._readtool import Table, _Handle, copied

PHASES = ("upload", "sort", "reduce", "filter", "links", "components", "totals", "copy_back")
REPORT = ("samples", "pooled_rows", "introns", "long_rows", "weak_rows", "kept_rows", "components", "singletons", "weak_clusters", "clusters", "printed_rows")
STATUS = ("printed", "weak_row", "long_row", "singleton", "weak_cluster")


class Clusters(Table):
    """A cluster table: numpy arrays (copies) per distinct intron in table order, `counts` (introns x samples), `report`, `times`
    (device ms per phase), `rounds` (of the device's components loop), text() and sample_text(k)."""
    PREFIX = "lsq_cl"

    def __init__(self, h, pool):
        super().__init__(h, pool, REPORT, PHASES)
        n = lib.lsq_cl_table_rows(h)
        self.n_samples = lib.lsq_cl_table_samples(h)
        self.rounds = lib.lsq_cl_table_rounds(h)
        ptrs = [P(u32)(), P(i32)(), P(i32)(), P(u8)(), P(u64)(), P(u32)(), P(u32)(), P(u8)()]
        check(lib.lsq_cl_table_arrays(h, *[C.byref(p) for p in ptrs]))
        names = (("chrom", np.uint32), ("start", np.int32), ("end", np.int32), ("ann", np.uint8), ("reads", np.uint64), ("samples", np.uint32),
                 ("cluster", np.uint32), ("status", np.uint8))
        for (k, dt), p in zip(names, ptrs):
            setattr(self, k, copied(p, n, dt))
        cp = P(u32)()
        check(lib.lsq_cl_table_counts(h, C.byref(cp)))
        self.counts = copied(cp, n * self.n_samples, np.uint32).reshape(n, self.n_samples)

    def __len__(self):
        return len(self.chrom)

    def chrom_names(self):
        names, c = [], 0
        while lib.lsq_cl_table_chrom_name(self.h, c) is not None:
            names.append(lib.lsq_cl_table_chrom_name(self.h, c).decode())
            c += 1
        return names

    def rows(self):
        """[(chromosome name, start, end, ann, reads, samples, cluster, status)] in table order"""
        names = self.chrom_names()
        return [(names[c], int(s), int(e), chr(a), int(r), int(m), int(k), int(u)) for c, s, e, a, r, m, k, u in
                zip(self.chrom, self.start, self.end, self.ann, self.reads, self.samples, self.cluster, self.status)]

    def text(self):
        """lsq_cl_format: the cluster table"""
        return take_text(lib.lsq_cl_format, self.h)

    def sample_text(self, k):
        """lsq_cl_format_sample: the count table of sample k (0-based, the order the samples were added in)"""
        return take_text(lib.lsq_cl_format_sample, self.h, k)


class ClusterPool(_Handle):
    """lsq_cl_pool_create: the pool of the samples' junction rows under one JunctionIndex"""
    PREFIX = "lsq_cl"
    KIND = "pool"

    def __init__(self, index):
        h = vp()
        check(lib.lsq_cl_pool_create(index.h, C.byref(h)))
        self.h = h
        self.index = index

    @property
    def num_samples(self):
        return lib.lsq_cl_pool_samples(self.h)

    @property
    def num_rows(self):
        return lib.lsq_cl_pool_rows(self.h)

    def add(self, junctions):
        """one more sample: the rows of a junctions.Junctions of the pool's index"""
        check(lib.lsq_cl_pool_add_table(self.h, junctions.h))

    def add_rows(self, chrom, start, end, reads):
        """one more sample from arrays: chromosome indices, 0-based half-open coordinates, reads"""
        arrays = [np.ascontiguousarray(a, dt) for a, dt in ((chrom, np.uint32), (start, np.int32), (end, np.int32), (reads, np.uint32))]
        n = len(arrays[0])
        if any(len(a) != n for a in arrays):
            raise ValueError("chrom, start, end and reads differ in length")
        check(lib.lsq_cl_pool_add_rows(self.h, n, *[a.ctypes.data_as(P(t)) for a, t in zip(arrays, (u32, i32, i32, u32))]))

    def add_text(self, path):
        """one more sample from a file that `junctions` printed"""
        check(lib.lsq_cl_pool_add_text(self.h, _b(path)))

    def _table(self, call, *args):
        t = vp()
        check(call(*args, C.byref(t)))
        return Clusters(t, self)

    def host(self, min_reads=1, max_intron=100000, min_cluster_reads=30, n_threads=0):
        """lsq_cl_host: a sort, then a union-find; no GPU touched"""
        return self._table(lib.lsq_cl_host, self.h, min_reads, max_intron, min_cluster_reads, n_threads)

    def device(self, ctx, min_reads=1, max_intron=100000, min_cluster_reads=30):
        """lsq_cl_device: sort, reduce, filter, links, components and totals on the GPU"""
        return self._table(lib.lsq_cl_device, ctx.h, self.h, min_reads, max_intron, min_cluster_reads)


__all__ = ["ClusterPool", "Clusters", "PHASES", "REPORT", "STATUS"]
