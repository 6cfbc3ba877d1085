"""Thin object wrappers over the C ABI (include/lesseq_hip.h).  No compute lives here."""
import os
import ctypes as C

import numpy as np

from ._lib import lib, check, check_runtime_once, SynthSpecStruct, BamReportStruct, u64, u32, i32, u16, u8, i64, vp, cs, P, _b

EVENT_TYPES = ("SE", "RI", "A5SS", "A3SS", "MXE", "AFE", "ALE", "T3")


def _take_text(ptr):
    if not ptr:
        return ""
    s = C.string_at(ptr).decode()
    lib.lsq_free(ptr)
    return s


def _ptr(a, ct):
    return a.ctypes.data_as(P(ct))


class Annotation:
    """lsq_annotation_load: LH_GENE_TXT + UCSC_GENE2ISOFORM, genes [begin, end) of the sorted name set"""

    def __init__(self, isoforms_path, g2i_path, begin=0, end=2 ** 62, isoform_format="LH_GENE_TXT", g2i_format="UCSC_GENE2ISOFORM"):
        h = vp()
        check(lib.lsq_annotation_load(_b(isoform_format), _b(isoforms_path), _b(g2i_format), _b(g2i_path), begin, end, C.byref(h)))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None):
            lib.lsq_annotation_free(self.h)
            self.h = None

    @property
    def num_genes(self):
        return lib.lsq_annotation_num_genes(self.h)


class Events:
    """lsq_events_compile: segments, isoform masks, ARS per read file, covered regions, device plan.
    library: "unstranded" (the default), "forward" or "reverse" -- the job's library type (lsq_events_compile_library)."""

    def __init__(self, annotation, read_types=("SHORT_READ",), read_lengths=(100,), library="unstranded"):
        M = len(read_types)
        rt = (cs * max(M, 1))(*[_b(t) for t in read_types])
        rl = (u64 * max(M, 1))(*read_lengths)
        h = vp()
        code = lib.lsq_library_from_name(_b(library))
        if code < 0:
            raise ValueError("library is 'unstranded', 'forward' or 'reverse', not %r" % (library,))
        check(lib.lsq_events_compile_library(annotation.h, M, rt, rl, code, C.byref(h)))
        self.h = h
        self.n_methods = M

    @property
    def library(self):
        return ("unstranded", "forward", "reverse")[lib.lsq_events_library(self.h)]

    def covered(self, chrom, minus=False):
        """the covered regions the load-time filter uses: the chromosome's (unstranded events), or those of its plus /
        minus genes (stranded events), as (start, end) pairs (a developer entry: lsq_debug_events_covered)"""
        n = lib.lsq_debug_events_covered(self.h, _b(chrom), int(minus), None, None, 0)
        if n < 0:
            raise ValueError("bad argument")
        s, e = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))()
        lib.lsq_debug_events_covered(self.h, _b(chrom), int(minus), s, e, n)
        return [(s[q], e[q]) for q in range(n)]

    def bucket_events(self, bucket):
        """(kind, the bucket's events as output indices in the bucket's own order) -- kind 0: generic records, 1: packed,
        2: evaluated on the host (a developer entry: lsq_debug_bucket_events).  No GPU."""
        kind = C.c_int(0)
        n = lib.lsq_debug_bucket_events(self.h, bucket, C.byref(kind), None, 0)
        if n < 0:
            raise ValueError("bad argument")
        out = (C.c_int64 * max(n, 1))()
        lib.lsq_debug_bucket_events(self.h, bucket, None, out, n)
        return kind.value, [int(out[q]) for q in range(n)]

    # lsq_debug_upload_tables: name -> (table number, element type, columns of a record)
    UPLOAD_TABLES = {"em_order": (0, np.uint32, 1), "em_places": (1, np.uint32, 1), "pack_cls": (2, np.uint32, 1), "pack_iso": (3, np.uint32, 1),
                     "pack_ev": (4, np.uint32, 1), "G": (5, np.float64, 1), "route_chrom": (6, np.int32, 8), "cov": (7, np.int32, 2), "clu": (8, np.int32, 4),
                     "loc": (9, np.uint32, 2), "route_shift": (10, np.uint32, 1), "bin_base": (11, np.uint32, 1), "cell_base": (12, np.uint32, 1),
                     "jgroup_base": (13, np.uint32, 1), "group_totals": (14, np.uint32, 1), "gene_names": (15, np.uint8, 1), "gene_name_off": (16, np.uint32, 1),
                     "bucket_bins": (17, np.uint32, 1), "jg_base": (18, np.uint32, 1)}

    def upload_tables(self, *names):
        """the tables lsq_events_upload makes of these events, as the host works them out (a developer entry:
        lsq_debug_upload_tables; csrc/lsq_upload_tables.hpp says what each holds): {name: numpy array}, records as rows
        (route_chrom: loc_first, loc_nb, loc_base, cov0, cov1, clu0, clu1, 0; bucket_bins and jg_base are no tables of the upload
        but the events' own figures that bin_base and jgroup_base are summed from).  No names: every table.  No GPU."""
        out = {}
        for name in names or self.UPLOAD_TABLES:
            which, dtype, cols = self.UPLOAD_TABLES[name]
            n = u64()
            check(lib.lsq_debug_upload_tables(self.h, which, None, 0, C.byref(n)))
            a = np.zeros(max(n.value, 1), dtype)
            check(lib.lsq_debug_upload_tables(self.h, which, a.ctypes.data_as(vp), n.value, C.byref(n)))
            a = a[:n.value]
            out[name] = a.reshape(-1, cols) if cols > 1 else a
        return out

    def bucket_cells(self, bucket):
        """the shortcut table of a packed bucket as compiled: a list of (lo, hi, e1, e2, info, flags) per cell, in start
        order (a developer entry: lsq_debug_bucket_cells; csrc/lsq_internal.hpp says what the fields hold).  No GPU."""
        n = lib.lsq_debug_bucket_cells(self.h, bucket, None, None, None, None, None, None, 0)
        if n < 0:
            raise ValueError("bad argument")
        a = [np.zeros(max(n, 1), np.int32) for _ in range(4)] + [np.zeros(max(n, 1), np.uint32) for _ in range(2)]
        lib.lsq_debug_bucket_cells(self.h, bucket, *[_ptr(x, i32) for x in a[:4]], *[_ptr(x, u32) for x in a[4:]], n)
        return [tuple(int(x[q]) for x in a) for q in range(n)]

    def __del__(self):
        if getattr(self, "h", None):
            lib.lsq_events_free(self.h)
            self.h = None

    def __len__(self):
        return lib.lsq_events_count(self.h)

    @property
    def total_isoforms(self):
        return lib.lsq_events_total_isoforms(self.h)

    @property
    def num_buckets(self):
        return lib.lsq_events_num_buckets(self.h)

    @property
    def lds_table_bytes(self):
        return lib.lsq_events_lds_table_bytes(self.h)

    def gene_name(self, ev):
        return lib.lsq_events_gene_name(self.h, ev).decode()

    def chrom(self, ev):
        return lib.lsq_events_chrom(self.h, ev).decode()

    def strand(self, ev):
        return lib.lsq_events_strand(self.h, ev).decode()

    def K(self, ev):
        return lib.lsq_events_num_isoforms(self.h, ev)

    def N(self, ev):
        return lib.lsq_events_num_segments(self.h, ev)

    def isoform_name(self, ev, j):
        return lib.lsq_events_isoform_name(self.h, ev, j).decode()

    def segments(self, ev):
        out = []
        s, e = i64(), i64()
        for n in range(self.N(ev)):
            check(lib.lsq_events_segment(self.h, ev, n, C.byref(s), C.byref(e)))
            out.append((s.value, e.value))
        return out

    def isoform_mask(self, ev, j):
        return lib.lsq_events_isoform_mask(self.h, ev, j)

    def isoform_length(self, ev, j):
        return lib.lsq_events_isoform_length(self.h, ev, j)

    def ars(self, method, ev, j):
        return lib.lsq_events_ars(self.h, method, ev, j)

    def span(self, ev):
        s, e = i64(), i64()
        check(lib.lsq_events_span(self.h, ev, C.byref(s), C.byref(e)))
        return s.value, e.value

    def set_shard(self, first_event, n_events):
        check(lib.lsq_events_set_shard(self.h, first_event, n_events))

    def shard_bounds(self, world, weights=None):
        """lsq_shard_bounds: [(first, count)] per process, contiguous slices of equal weight"""
        first, count = (u64 * world)(), (u64 * world)()
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, np.float64)
            assert len(w) == len(self)
        check(lib.lsq_shard_bounds(self.h, world, _ptr(w, C.c_double) if w is not None else None, first, count))
        return [(int(first[r]), int(count[r])) for r in range(world)]

    def record_words(self, first, count):
        return int(lib.lsq_record_words(self.h, first, count))

    def gathered_unpack(self, bounds, blocks, stride_words):
        """blocks: uint64 array [world * stride_words] of packed records -> (cnt, bases, theta, logll) of the whole job"""
        world = len(bounds)
        first = (u64 * world)(*[b[0] for b in bounds])
        count = (u64 * world)(*[b[1] for b in bounds])
        off = self.class_offsets()
        n_cls, n_ev, M = off[-1], len(self), self.n_methods
        cnt = np.zeros((max(M, 1), max(n_cls, 1)), np.uint64)
        bases = np.zeros((max(M, 1), max(n_cls, 1)), np.uint64)
        theta = np.zeros(max(self.total_isoforms, 1), np.float64)
        ll = np.zeros(max(n_ev, 1), np.float64)
        blocks = np.ascontiguousarray(blocks).view(np.uint64)
        # the C side indexes [method][n_classes] rows of exactly n_cls entries
        c2 = np.zeros(max(M * n_cls, 1), np.uint64)
        b2 = np.zeros(max(M * n_cls, 1), np.uint64)
        check(lib.lsq_gathered_unpack(self.h, world, first, count, _ptr(blocks, u64), stride_words, _ptr(c2, u64), _ptr(b2, u64),
                                      _ptr(theta, C.c_double), _ptr(ll, C.c_double)))
        cnt = c2[:M * n_cls].reshape(M, n_cls) if M * n_cls else cnt[:M, :n_cls]
        bases = b2[:M * n_cls].reshape(M, n_cls) if M * n_cls else bases[:M, :n_cls]
        return cnt, bases, theta[:self.total_isoforms], ll[:n_ev]

    def chrom_id(self, name):
        return lib.lsq_events_chrom_id(self.h, _b(name))

    def strand_id(self, name):
        return lib.lsq_events_strand_id(self.h, _b(name))

    def class_offsets(self):
        off = [0]
        for ev in range(len(self)):
            off.append(off[-1] + (1 << self.K(ev)) - 1)
        return off


SAM_DEFAULT_SKIP_FLAGS = 0x904      # unmapped, secondary, supplementary


def sam_to_mrf(sam_bytes, skip_flags=SAM_DEFAULT_SKIP_FLAGS, min_mapq=0):
    """the MRF_SINGLE text (bytes) that defines what a SAM_SINGLE text means (lsq_sam_to_mrf)"""
    data = bytes(sam_bytes)
    out, n = vp(), u64()
    check(lib.lsq_sam_to_mrf(data, len(data), skip_flags, min_mapq, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value)
    finally:
        lib.lsq_free(out)


def bam_to_mrf(bam_bytes, skip_flags=SAM_DEFAULT_SKIP_FLAGS, min_mapq=0, verify=False):
    """the MRF_SINGLE text (bytes) that defines what a BAM_SINGLE file means (lsq_bam_to_mrf): that of its SAM equivalent;
    verify: every block's CRC32 and the end-of-file marker are checked on the way (lsq_bam_to_mrf_checked)"""
    data = bytes(bam_bytes)
    out, n = vp(), u64()
    check((lib.lsq_bam_to_mrf_checked if verify else lib.lsq_bam_to_mrf)(data, len(data), skip_flags, min_mapq, C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value)
    finally:
        lib.lsq_free(out)


def _bam_report(r):
    return {k: int(getattr(r, k)) for k, _ in r._fields_}


def bam_check_host(path, n_threads=0):
    """a whole BAM file checked on the host, CRC32s and end-of-file marker included, no annotation needed (lsq_bam_check_host):
    the report's fields as a dict"""
    r = BamReportStruct()
    check(lib.lsq_bam_check_host(_b(path), n_threads, C.byref(r)))
    return _bam_report(r)


class Reads:
    """A parsed read set in file order: from an MRF file, caller arrays, or the synthetic generator"""

    def __init__(self, handle, keep=None):
        self.h = handle
        self._keep = keep

    @classmethod
    def from_mrf(cls, path, events, n_threads=0, read_format="MRF_SINGLE"):
        h = vp()
        check(lib.lsq_reads_parse(_b(read_format), _b(path), events.h, n_threads, C.byref(h)))
        return cls(h)

    @classmethod
    def from_sam(cls, path, events, skip_flags=SAM_DEFAULT_SKIP_FLAGS, min_mapq=0, n_threads=0):
        """a SAM_SINGLE file through the host parser (lsq_sam_parse): the arrays from_mrf gives for its MRF equivalent"""
        h = vp()
        check(lib.lsq_sam_parse(_b(path), events.h, skip_flags, min_mapq, n_threads, C.byref(h)))
        return cls(h)

    @classmethod
    def from_bam(cls, path, events, skip_flags=SAM_DEFAULT_SKIP_FLAGS, min_mapq=0, n_threads=0, verify=False):
        """a BAM_SINGLE file through the host parser (lsq_bam_parse): the arrays from_sam gives for its SAM equivalent;
        verify: every block's CRC32 and the end-of-file marker are checked on the way (lsq_bam_parse_checked)"""
        h = vp()
        check((lib.lsq_bam_parse_checked if verify else lib.lsq_bam_parse)(_b(path), events.h, skip_flags, min_mapq, n_threads, C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, blk_off, line_no, blk_start, blk_end, blk_chrom, blk_strand):
        arrs = (np.ascontiguousarray(blk_off, np.uint64), np.ascontiguousarray(line_no, np.uint32),
                np.ascontiguousarray(blk_start, np.int32), np.ascontiguousarray(blk_end, np.int32),
                np.ascontiguousarray(blk_chrom, np.uint16), np.ascontiguousarray(blk_strand, np.uint8))
        h = vp()
        check(lib.lsq_reads_wrap(len(arrs[1]), _ptr(arrs[0], u64), _ptr(arrs[1], u32), _ptr(arrs[2], i32),
                                 _ptr(arrs[3], i32), _ptr(arrs[4], u16), _ptr(arrs[5], u8), C.byref(h)))
        return cls(h, keep=arrs)

    @classmethod
    def synthetic(cls, spec, events, n_threads=0):
        h = vp()
        check(lib.lsq_synth_reads(C.byref(spec.c), events.h, n_threads, C.byref(h)))
        return cls(h)

    def __del__(self):
        if getattr(self, "h", None):
            lib.lsq_reads_free(self.h)
            self.h = None

    def __len__(self):
        return lib.lsq_reads_count(self.h)

    @property
    def num_blocks(self):
        return lib.lsq_reads_num_blocks(self.h)

    def arrays(self):
        """copies of (blk_off, line_no, blk_start, blk_end, blk_chrom_id, blk_strand_id)"""
        ptrs = [vp() for _ in range(6)]
        check(lib.lsq_reads_arrays(self.h, *[C.byref(p) for p in ptrs]))
        n, nb = len(self), self.num_blocks
        spec = ((np.uint64, n + 1), (np.uint32, n), (np.int32, nb), (np.int32, nb), (np.uint16, nb), (np.uint8, nb))
        out = []
        for p, (dt, cnt) in zip(ptrs, spec):
            if cnt == 0 or not p.value:
                out.append(np.zeros(cnt, dt))
            else:
                buf = (C.c_char * (cnt * np.dtype(dt).itemsize)).from_address(p.value)
                out.append(np.frombuffer(buf, dtype=dt, count=cnt).copy())
        return tuple(out)


class Context:
    """One GPU: uploads, the count kernel, the EM kernel, result fetch"""

    def __init__(self, device=0):
        h = vp()
        check(lib.lsq_ctx_create(device, C.byref(h)))
        self.h = h
        self.events = None
        check_runtime_once()              # (the HIP runtime is up now: compiled-against and running versions are compared once)
        # LSQ_OPTIONS="name=value,...": the executables pass these to lsq_ctx_set_option (lsq_cli.cpp), so does this class
        for item in filter(None, os.environ.get("LSQ_OPTIONS", "").split(",")):
            if "=" in item:
                name, value = item.split("=", 1)
                self.set_option(name.strip(), float(value))

    def close(self):
        if getattr(self, "h", None):
            lib.lsq_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def upload_events(self, events):
        check(lib.lsq_events_upload(self.h, events.h))
        self.events = events

    def upload_reads(self, method, reads):
        check(lib.lsq_reads_upload(self.h, method, reads.h))

    def upload_reads_mrf(self, method, path, read_format="MRF_SINGLE"):
        """MRF text -> HBM -> parsed and ingested on the device (lsq_reads_upload_mrf)"""
        check(lib.lsq_reads_upload_mrf(self.h, method, _b(read_format), _b(path)))

    def parse_mrf_device(self, path, read_format="MRF_SINGLE"):
        """the device parser's blocks, copied back as a Reads (tests, tools)"""
        h = vp()
        check(lib.lsq_mrf_parse_device(self.h, _b(read_format), _b(path), C.byref(h)))
        return Reads(h)

    def upload_reads_sam(self, method, path):
        """SAM text -> HBM -> parsed and ingested on the device (lsq_reads_upload_mrf with "SAM_SINGLE"; the records that
        make no read: options sam_skip_flags / sam_min_mapq)"""
        check(lib.lsq_reads_upload_mrf(self.h, method, b"SAM_SINGLE", _b(path)))

    def parse_sam_device(self, path):
        """the device SAM parser's blocks, copied back as a Reads (tests, tools)"""
        return self.parse_mrf_device(path, read_format="SAM_SINGLE")

    def sam_paths(self):
        """(lines the tile kernel handed to the fall-back kernel, whole file through the byte-walking form) of the latest SAM ingest"""
        a, b = u32(), u32()
        check(lib.lsq_last_sam_paths(self.h, C.byref(a), C.byref(b)))
        return {"lines_to_fall_back_kernel": a.value, "whole_file_byte_walking": bool(b.value)}

    def upload_reads_bam(self, method, path):
        """BAM file -> HBM -> inflated, parsed and ingested on the device (lsq_reads_upload_mrf with "BAM_SINGLE"; the filters are
        SAM's options sam_skip_flags / sam_min_mapq)"""
        check(lib.lsq_reads_upload_mrf(self.h, method, b"BAM_SINGLE", _b(path)))

    def parse_bam_device(self, path):
        """the device BAM chain's blocks, copied back as a Reads (tests, tools)"""
        return self.parse_mrf_device(path, read_format="BAM_SINGLE")

    def bam_paths(self):
        """(BGZF blocks, blocks the repair pass walked again) of the latest BAM file: 0 repaired for a file as htslib writes it"""
        a, b = u64(), u64()
        check(lib.lsq_last_bam_paths(self.h, C.byref(a), C.byref(b)))
        return {"blocks": a.value, "blocks_repaired": b.value}

    def bgzf_inflate(self, data):
        """the inflated stream of a BGZF file's bytes through the staging and the inflate kernel alone (lsq_debug_bgzf_inflate)"""
        data = bytes(data)
        n = u64()
        cap = 1 << 16
        while True:
            out = C.create_string_buffer(cap)
            st = lib.lsq_debug_bgzf_inflate(self.h, data, len(data), out, cap, C.byref(n))
            if st == -5 and n.value > cap:
                cap = n.value
                continue
            check(st)
            return out.raw[:n.value]

    def bgzf_crc32(self, data):
        """the CRC32 the device computes for every BGZF block of a file's bytes, in file order, nothing compared (lsq_debug_bgzf_crc32)"""
        data = bytes(data)
        n = u64()
        cap = 1 << 10
        while True:
            out = (u32 * cap)()
            st = lib.lsq_debug_bgzf_crc32(self.h, data, len(data), out, cap, C.byref(n))
            if st == -5 and n.value > cap:
                cap = n.value
                continue
            check(st)
            return [int(v) for v in out[:n.value]]

    SCAN_FORMS = ("u32", "flag", "u64", "pad_p2", "pad_p1")

    def debug_scan(self, form, values):
        """the device prefix sum alone (lsq_debug_scan): len(values) + 1 uint64, the last the total.  form: an index into, or a
        name of, SCAN_FORMS -- 32-bit values, 32-bit values as 0 / 1 flags, 64-bit values, 32-bit values rounded up to the
        two-block / one-block pool's group padding"""
        form = self.SCAN_FORMS.index(form) if isinstance(form, str) else int(form)
        v = np.ascontiguousarray(values, dtype=np.uint64 if form == 2 else np.uint32)
        out = np.empty(len(v) + 1, dtype=np.uint64)
        check(lib.lsq_debug_scan(self.h, form, v.ctypes.data_as(vp), len(v), _ptr(out, u64)))
        return out

    def debug_sort(self, w0, w1, bits, drop_constant=False):
        """the device radix sort alone (lsq_debug_sort): the records (w0[i], w1[i]) in stable order by the 8-bit digits at `bits`
        (positions in the 128 bits w1:w0, least significant first as listed) as two new uint64 arrays, and the passes made"""
        a = np.array(w0, dtype=np.uint64)           # (copies: the call sorts in place)
        b = np.array(w1, dtype=np.uint64)
        if a.ndim != 1 or a.shape != b.shape:
            raise ValueError("w0 and w1 are two one-dimensional arrays of one length")
        bits = [int(x) for x in bits]
        cb = (C.c_uint * max(len(bits), 1))(*bits)
        n_passes = C.c_uint()
        check(lib.lsq_debug_sort(self.h, _ptr(a, u64), _ptr(b, u64), len(a), cb, len(bits), int(bool(drop_constant)), C.byref(n_passes)))
        return a, b, n_passes.value

    def bam_check(self, path):
        """a whole BAM file checked on the device chain, CRC32s and end-of-file marker included; the context needs no events
        (lsq_bam_check): the report's fields as a dict"""
        r = BamReportStruct()
        check(lib.lsq_bam_check(self.h, _b(path), C.byref(r)))
        return _bam_report(r)

    def mrf_timing(self):
        a, b = C.c_float(), C.c_float()
        check(lib.lsq_last_mrf_timing(self.h, C.byref(a), C.byref(b)))
        return {"h2d_ms": a.value, "parse_ms": b.value}

    def parse_paths(self):
        """(tiles handed to the byte-walking kernel, lines handed to the shared splitter, whole file through the byte-walking kernel)
        of the latest device parse (lsq_debug_last_parse_paths)"""
        a, b, c = C.c_uint(), C.c_uint(), C.c_uint()
        lib.lsq_debug_last_parse_paths.argtypes = [vp, P(C.c_uint), P(C.c_uint), P(C.c_uint)]
        lib.lsq_debug_last_parse_paths.restype = C.c_int
        check(lib.lsq_debug_last_parse_paths(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"tiles_to_byte_walking_kernel": a.value, "lines_to_shared_splitter": b.value, "whole_file_byte_walking": bool(c.value)}

    def ingest_stages(self):
        """device milliseconds and minimum bytes of every pass of the latest ingest (lsq_last_ingest_stages), in order"""
        n = lib.lsq_last_ingest_stage_count(self.h)
        ms, by = (C.c_float * n)(), (C.c_uint64 * n)()
        check(lib.lsq_last_ingest_stages(self.h, ms, by, n))
        return [{"stage": lib.lsq_last_ingest_stage_name(self.h, i).decode(), "ms": float(ms[i]), "bytes": int(by[i])} for i in range(n)]

    def retained(self, method):
        return lib.lsq_reads_retained(self.h, method)

    def library_report(self, method=0):
        """stranded jobs: (reads of the + strand, of the - strand, records without a strand, + reads retained, - reads
        retained) of the latest read file of `method` (lsq_last_library_report)"""
        out = (u64 * 5)()
        check(lib.lsq_last_library_report(self.h, method, out))
        return tuple(out)

    def pooled(self, method):
        """retained reads kept in the pools: those that start in the span of an event planned on this context"""
        return lib.lsq_reads_pooled(self.h, method)

    def pooled_blocks(self, method):
        """blocks of the pooled reads: what one count() streams"""
        return lib.lsq_reads_pooled_blocks(self.h, method)

    def pool_format(self, method):
        """lsq_reads_pool_format: (compact records?, bytes of block coordinates in HBM,
        reads kept as one-block / two-block records / with the many-block reads)"""
        a, n = C.c_int(0), C.c_uint64(0)
        k = (C.c_uint64 * 3)()
        check(lib.lsq_reads_pool_format(self.h, method, C.byref(a), C.byref(n), k))
        return bool(a.value), n.value, tuple(int(x) for x in k)

    POOL_NAMES = (None, "one", "two", "many")

    def pool_reads(self, method=0):
        """every read in the pools of the latest read set of `method`, the groups' padding left out, whichever format the
        pools have (a developer entry: lsq_debug_pool_reads): a list of (line_no, bucket, strand id, pool, blocks) -- pool
        "one", "two" or "many", blocks the merged (start, end) pairs as wide coordinates"""
        nr, nb = u64(), u64()
        check(lib.lsq_debug_pool_reads(self.h, method, C.byref(nr), C.byref(nb), None, None, None, None, None, None, None, 0, 0))
        n, m = nr.value, nb.value
        line, bucket = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        strand, pool = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        off = np.zeros(max(n, 1), np.uint64)
        s, e = np.zeros(max(m, 1), np.int64), np.zeros(max(m, 1), np.int64)
        check(lib.lsq_debug_pool_reads(self.h, method, C.byref(nr), C.byref(nb), _ptr(line, u32), _ptr(bucket, u32), _ptr(strand, u8), _ptr(pool, u8),
                                       _ptr(off, u64), _ptr(s, i64), _ptr(e, i64), max(n, 1), max(m, 1)))
        if (nr.value, nb.value) != (n, m):
            raise RuntimeError("the pools changed between two calls")
        ends = [int(x) for x in off[1:n]] + [m]
        return [(int(line[r]), int(bucket[r]), int(strand[r]), self.POOL_NAMES[pool[r]],
                 tuple((int(s[q]), int(e[q])) for q in range(int(off[r]), ends[r]))) for r in range(n)]

    def locator(self):
        """the locator grid of the uploaded events (a developer entry: lsq_debug_locator): {"shift": the bins are 2^shift
        bases wide, "tables": per chromosome table (loc_base -- the first base of bin 0, loc_nb -- its bins; 0: no record)}.
        Table of a chromosome: Events.chrom_id(name), or 2 * that + (1 for the minus strand) for stranded events."""
        shift, n = C.c_uint(), u64()
        check(lib.lsq_debug_locator(self.h, C.byref(shift), C.byref(n), None, None, 0))
        base, nb = (i64 * max(n.value, 1))(), (u64 * max(n.value, 1))()
        check(lib.lsq_debug_locator(self.h, C.byref(shift), C.byref(n), base, nb, n.value))
        return {"shift": int(shift.value), "tables": [(int(base[q]), int(nb[q])) for q in range(n.value)]}

    def retained_blocks(self, method):
        return lib.lsq_reads_retained_blocks(self.h, method)

    def count(self):
        check(lib.lsq_count(self.h))

    def solve(self):
        check(lib.lsq_solve(self.h))

    def set_option(self, name, value):
        """lsq_ctx_set_option: grid_multiplier, exception_capacity, recount_every_read, em_guard_band,
        snap_shares, em_regroup, em_flat_min_events, compact_pools, sam_skip_flags, sam_min_mapq, bam_verify, bootstrap_chunk,
        counter_sets (2 or 3; only while nothing is in flight)"""
        check(lib.lsq_ctx_set_option(self.h, _b(name), float(value)))

    def count_status(self):
        """per read file: (pairs handed to the exception pass, recount ran) of the latest count()"""
        M = max(self.events.n_methods, 1)
        e, r = (u32 * M)(), (u32 * M)()
        check(lib.lsq_count_status(self.h, e, r))
        return list(e)[:self.events.n_methods], list(r)[:self.events.n_methods]

    def counts_device_words(self):
        return int(lib.lsq_counts_device_words(self.h))

    def export_counts_device(self, d_ptr):
        """the latest count's class counts and matched bases, device order, into a device buffer (result stream)"""
        check(lib.lsq_counts_export_device(self.h, vp(d_ptr)))

    def import_counts_device(self, d_ptr):
        """such a buffer (e.g. summed over the ranks of a read-sharded job) becomes the counts solve() works on"""
        check(lib.lsq_counts_import_device(self.h, vp(d_ptr)))

    DEBUG_COUNTERS = ("parked1", "parked2", "walk_steps", "walk_lanes", "exceptions", "park1_no_cell", "park1_one_owner", "park1_two_owner",
                      "park2_no_owner", "park2_one_owner", "unused10", "steps1_parking", "steps1", "park2_follower_plain", "park2_follower_past", "unused15")

    def debug_counters(self):
        """the path counters of the latest count()'s streaming loops, by the names include/lesseq_hip_dev.h gives them
        (lsq_debug_counters).  Filled by the developer library (LSQ_LIB=.../liblesseq_hip_dev.so) under LSQ_ABLATE bit 256; the
        release library leaves all but `exceptions` zero."""
        out = (C.c_ulonglong * 16)()
        check(lib.lsq_debug_counters(self.h, out))
        return {k: int(out[i]) for i, k in enumerate(self.DEBUG_COUNTERS)}

    def launch_info(self):
        """(one-block reads a lane settles per table look, resident workgroups per compute unit) of the latest count()"""
        a, b = u32(), u32()
        check(lib.lsq_count_launch_info(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_em_guard_band(self, band):
        """events whose EM stop test comes within `band` of its threshold are replayed in the reference's per-read order"""
        check(lib.lsq_set_em_guard_band(self.h, float(band)))

    def solve_finalize(self):
        """the exact-order replay of flagged events on its own; returns how many were redone"""
        n = u32()
        check(lib.lsq_solve_finalize(self.h, C.byref(n)))
        return n.value

    EM_LEAN_FORMS = ("none", "four_lane", "four_lane_capped_tail", "head_tail", "four_lane_flat3", "four_lane_flat4")

    def em_launch(self):
        """what the latest solve() launched for the EM (lsq_debug_last_em_launch): the form the lean group went through, its
        places, the first place solved one lane per event (the lean places when none was), the general kernel's places, and
        whether the lean places were in an order learnt from an earlier solve"""
        out = (C.c_uint * 8)()
        check(lib.lsq_debug_last_em_launch(self.h, out))
        return {"lean_form": self.EM_LEAN_FORMS[out[0]], "lean_places": int(out[1]), "split": int(out[2]), "general_places": int(out[3]),
                "learnt_placement": bool(out[4]), "quad_cap": int(out[5]), "placement_learnt_after": bool(out[6]), "lane": int(out[7])}

    def synchronize(self):
        check(lib.lsq_ctx_synchronize(self.h))

    @property
    def stream(self):
        return lib.lsq_ctx_stream(self.h)

    def set_timing(self, on=True):
        """HIP events around the kernels of the following count()/solve() calls (off by default: they cost queue time)"""
        check(lib.lsq_set_timing(self.h, 1 if on else 0))

    def timing(self):
        a, b = C.c_float(), C.c_float()
        check(lib.lsq_last_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def copy_results_device(self, d_class_count=None, d_theta=None, d_logll=None):
        """raw device-order results into caller device buffers (integer addresses), async"""
        check(lib.lsq_results_copy_device(self.h, vp(d_class_count), vp(d_theta), vp(d_logll)))

    def pack_results_device(self, d_block):
        """the shard's per-event records in output order into a caller device buffer (integer address), async on the result stream"""
        check(lib.lsq_results_pack_device(self.h, vp(d_block)))

    @property
    def result_stream(self):
        return lib.lsq_ctx_result_stream(self.h)

    def device_order(self):
        o = np.zeros(max(len(self.events), 1), np.int32)
        check(lib.lsq_results_device_order(self.h, _ptr(o, i32)))
        return o[:len(self.events)]

    def fast_kernel_ms(self):
        a = C.c_float()
        check(lib.lsq_last_fast_kernel_ms(self.h, C.byref(a)))
        return a.value

    def counts(self):
        """(class_count, class_bases) as uint64 arrays of shape [n_methods, n_classes], output order"""
        n = lib.lsq_results_num_classes(self.h)
        M = self.events.n_methods
        cnt = np.zeros((max(M, 1), max(n, 1)), np.uint64)
        bases = np.zeros((max(M, 1), max(n, 1)), np.uint64)
        check(lib.lsq_results_counts(self.h, _ptr(cnt, u64), _ptr(bases, u64)))
        return cnt[:M, :n], bases[:M, :n]

    def set_counts(self, cnt, bases):
        """the inverse of counts(): arrays of shape [n_methods, n_classes] become the context's counts"""
        cnt = np.ascontiguousarray(cnt, np.uint64)
        bases = np.ascontiguousarray(bases, np.uint64)
        check(lib.lsq_results_set_counts(self.h, _ptr(cnt, u64), _ptr(bases, u64)))

    def stage_text(self, path, byte_begin=0, byte_end=2 ** 64 - 1):
        """bytes [byte_begin, byte_end) of an MRF file copied to HBM; returns an opaque handle"""
        h = vp()
        check(lib.lsq_text_stage_range(self.h, _b(path), byte_begin, byte_end, C.byref(h)))
        return h

    def text_lines(self, text):
        n = u64()
        check(lib.lsq_text_lines(self.h, text, C.byref(n)))
        return n.value

    def upload_reads_text(self, method, text, has_header=True, first_line=1, read_format="MRF_SINGLE", free=True):
        try:
            check(lib.lsq_reads_upload_text_at(self.h, method, _b(read_format), text, 1 if has_header else 0, first_line))
        finally:
            if free:
                lib.lsq_text_free(text)

    def solution(self):
        """(theta[n_isoforms], logll[n_events], iters, flags), output order"""
        ne, ni = len(self.events), self.events.total_isoforms
        theta = np.zeros(max(ni, 1), np.float64)
        ll = np.zeros(max(ne, 1), np.float64)
        it = np.zeros(max(ne, 1), np.uint32)
        fl = np.zeros(max(ne, 1), np.uint8)
        check(lib.lsq_results_solve(self.h, _ptr(theta, C.c_double), _ptr(ll, C.c_double), _ptr(it, u32), _ptr(fl, u8)))
        return theta[:ni], ll[:ne], it[:ne], fl[:ne]

    def fim(self):
        """after solve(): (offsets[n_events+1], fim[n_methods, size], var_by_diag[n_methods, n_events], var_by_inverse[...]) --
        the expected Fisher information per read of theta_1..theta_{K-1} at the solved theta and fim.h's two variance
        estimates (parity unpinned: dead code in the reference)"""
        check(lib.lsq_fim(self.h))
        ne, M = len(self.events), self.events.n_methods
        off = np.zeros(ne + 1, np.uint64)
        check(lib.lsq_results_fim_offsets(self.h, _ptr(off, C.c_uint64)))
        size = int(off[ne])
        f = np.zeros(max(M * size, 1), np.float64)
        vd = np.zeros(max(M * ne, 1), np.float64)
        vi = np.zeros(max(M * ne, 1), np.float64)
        check(lib.lsq_results_fim(self.h, _ptr(f, C.c_double), _ptr(vd, C.c_double), _ptr(vi, C.c_double)))
        return off, f[:M * size].reshape(M, size), vd[:M * ne].reshape(M, ne), vi[:M * ne].reshape(M, ne)

    def bootstrap(self, B, seed=0):
        """after solve(): B read-bootstrap replicates of theta (lsq_bootstrap) and their summaries per isoform in
        output order, a dict of arrays: n_ok (replicates with a finite theta), mean, sd, q025, q500, q975"""
        check(lib.lsq_bootstrap(self.h, int(B), int(seed)))
        ni = self.events.total_isoforms
        n_ok = np.zeros(max(ni, 1), np.uint32)
        out = {k: np.zeros(max(ni, 1), np.float64) for k in ("mean", "sd", "q025", "q500", "q975")}
        check(lib.lsq_results_bootstrap(self.h, _ptr(n_ok, u32), *[_ptr(out[k], C.c_double) for k in ("mean", "sd", "q025", "q500", "q975")]))
        res = {"n_ok": n_ok[:ni]}
        res.update((k, v[:ni]) for k, v in out.items())
        self._boot_B = int(B)
        return res

    def bootstrap_theta(self):
        """theta of every replicate of the latest bootstrap(): float64 [B, n_isoforms], output order"""
        B, ni = getattr(self, "_boot_B", 0), self.events.total_isoforms
        t = np.zeros(max(B * ni, 1), np.float64)
        check(lib.lsq_results_bootstrap_theta(self.h, _ptr(t, C.c_double)))
        return t[:B * ni].reshape(B, ni)

    def bootstrap_replicate(self, seed, b):
        """replicate b of the bootstrap with that seed on its own, through the same kernels (lsq_bootstrap_replicate):
        (class_count[n_methods, n_classes], theta, logll, iters, flags), output order"""
        n = lib.lsq_results_num_classes(self.h)
        M, ne, ni = self.events.n_methods, len(self.events), self.events.total_isoforms
        cnt = np.zeros((max(M, 1), max(n, 1)), np.uint64)
        theta = np.zeros(max(ni, 1), np.float64)
        ll = np.zeros(max(ne, 1), np.float64)
        it = np.zeros(max(ne, 1), np.uint32)
        fl = np.zeros(max(ne, 1), np.uint8)
        check(lib.lsq_bootstrap_replicate(self.h, int(seed), int(b), _ptr(cnt, u64), _ptr(theta, C.c_double), _ptr(ll, C.c_double), _ptr(it, u32), _ptr(fl, u8)))
        return cnt[:M, :n], theta[:ni], ll[:ne], it[:ne], fl[:ne]

    def bootstrap_times(self):
        """device milliseconds of the latest bootstrap() under set_timing(): resample, em, summary, and the replicates per chunk"""
        ms, chunk = (C.c_float * 3)(), C.c_uint()
        check(lib.lsq_debug_bootstrap_times(self.h, ms, C.byref(chunk)))
        return {"resample_ms": float(ms[0]), "em_ms": float(ms[1]), "summary_ms": float(ms[2]), "chunk": int(chunk.value)}


def bootstrap_resample_host(class_off, class_count, seed, b):
    """replicate b's counts on the CPU (lsq_bootstrap_resample_host): class_off[n_events + 1] and class_count[n_methods,
    n_classes] in the layout of Events.class_offsets() / Context.counts(); event e is the e-th of them.  No GPU."""
    off = np.ascontiguousarray(class_off, np.uint64)
    cnt = np.ascontiguousarray(class_count, np.uint64)
    assert cnt.ndim == 2 and len(off) >= 1 and cnt.shape[1] == int(off[-1])
    out = np.zeros((cnt.shape[0], max(cnt.shape[1], 1)), np.uint64)[:, :cnt.shape[1]]
    out = np.ascontiguousarray(out)
    check(lib.lsq_bootstrap_resample_host(cnt.shape[0], len(off) - 1, _ptr(off, u64), _ptr(cnt, u64), int(seed), int(b), _ptr(out, u64)))
    return out


def bootstrap_draws(class_count, seed, m, e, b, first_draw, n_draws):
    """the classes (1-based) of single draws of one (read file m, event e) of replicate b (lsq_debug_bootstrap_draws).  No GPU."""
    cnt = np.ascontiguousarray(class_count, np.uint64)
    out = np.zeros(max(int(n_draws), 1), np.uint32)
    check(lib.lsq_debug_bootstrap_draws(len(cnt), _ptr(cnt, u64), int(seed), int(m), int(e), int(b), int(first_draw), int(n_draws), _ptr(out, u32)))
    return out[:int(n_draws)]


class SynthSpec:
    def __init__(self, seed, n_events, n_reads, read_length=100, n_chrom=1, event_types=EVENT_TYPES, zipf=False, overlap_frac=0.10, first_read=0, sorted_reads=False):
        mask = 0
        for t in event_types:
            mask |= 1 << EVENT_TYPES.index(t)
        self.c = SynthSpecStruct(seed, n_events, n_reads, read_length, n_chrom, mask, 1 if zipf else 0, overlap_frac, first_read, 1 if sorted_reads else 0, 0)


def synth_write(spec, directory, stem, write_mrf=True):
    check(lib.lsq_synth_write(C.byref(spec.c), _b(directory), _b(stem), 1 if write_mrf else 0))


def synth_write_sam(spec, directory, stem):
    """<stem>.interval, <stem>.map and the reads of synth_write as <stem>.sam (lsq_synth_write_sam)"""
    check(lib.lsq_synth_write_sam(C.byref(spec.c), _b(directory), _b(stem)))


def format_count(events, cnt):
    out = vp()
    a = np.ascontiguousarray(cnt, np.uint64)
    check(lib.lsq_format_count(events.h, events.n_methods, _ptr(a, u64), C.byref(out)))
    return _take_text(out)


def format_solve(events, cnt, bases, theta, logll, total_read_bases):
    out = vp()
    a = np.ascontiguousarray(cnt, np.uint64)
    b = np.ascontiguousarray(bases, np.uint64)
    t = np.ascontiguousarray(theta, np.float64)
    l = np.ascontiguousarray(logll, np.float64)
    r = np.ascontiguousarray(total_read_bases, np.float64)
    check(lib.lsq_format_solve(events.h, events.n_methods, _ptr(a, u64), _ptr(b, u64), _ptr(t, C.c_double),
                               _ptr(l, C.c_double), _ptr(r, C.c_double), C.byref(out)))
    return _take_text(out)


def cli_run(tool, argv):
    """Runs count / solve / classify / test_as in-process with the reference's argv (without argv[0]).
    Returns (exit_status, stdout_text).  The log goes to this process's stderr."""
    full = [b"lsq"] + [_b(a) for a in argv]
    arr = (cs * len(full))(*full)
    out = vp()
    rc = lib.lsq_cli_run(_b(tool), len(full), arr, C.byref(out))
    return rc, _take_text(out)
