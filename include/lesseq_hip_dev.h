/* lesseq_hip_dev.h -- developer entry points of liblesseq_hip.so, beside the product ABI of
 * lesseq_hip.h.  Nothing here replaces anything in the reference; the tools under tools/ and a
 * few tests use them to look inside a run (tools/kbench.py, tools/step_bench.py,
 * tests/test_parity_gpu.py, tests/test_em_direct_gpu.py, tests/test_prims_direct_gpu.py).  They may change without notice.
 * The entries that need the developer build (liblesseq_hip_dev.so, -DLSQ_DEV: lsq_debug_counters, lsq_debug_wg_trace and the
 * LSQ_ABLATE / LSQ_GRID_WGS environment switches) are loaded by tools/*.py and, in child processes of their own, by
 * tests/test_count_paths_gpu.py (tests/count_paths_child.py); the release library answers them with zeros. */
#ifndef LESSEQ_HIP_DEV_H
#define LESSEQ_HIP_DEV_H

#include <stdint.h>
#include "lesseq_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Counters the count kernels fill when LSQ_ABLATE has bit 256 set: [0] parked one-block reads,
 * [1] parked two-block reads, [2] walk steps, [3] walk lanes, [4] exception-list entries,
 * [5..7] reasons for parking one-block reads, [8..10], [13], [14] reasons for parking two-block reads, [11] / [12]
 * one-block steps of a wave with a parked read / all of them.  out16 holds 16 values.
 * By name, in order (Context.debug_counters() of lesseq_amd/api.py returns them so): parked1, parked2, walk_steps, walk_lanes,
 * exceptions, park1_no_cell (the read starts outside the lane's cell, or in no cell), park1_one_owner (past e2 of a one-owner
 * cell), park1_two_owner (a two-owner cell: past an end), park2_no_owner (block 1 of a looked-at record starts in no one-owner
 * cell), park2_one_owner (... in one), unused10, steps1_parking, steps1, park2_follower_plain (compact pools: a record behind a
 * first record that crosses no junction), park2_follower_past (compact pools: block 2 runs past the junction's segments), unused15.
 * The wide two-block loop counts its second records in parked2 only.  The release library leaves all but `exceptions` zero. */
int lsq_debug_counters(lsq_ctx *c, unsigned long long *out16);
/* (start, end, steps of the general walk, reads those looked at) of each workgroup of the last count launch, times in 100 MHz
 * ticks (developer library with LSQ_ABLATE bit 4194304; otherwise *n = 0): out holds 4 * cap values; the first *n_workers
 * workgroups are the pool-n workers */
int lsq_debug_wg_trace(lsq_ctx *c, unsigned long long *out, unsigned long long cap, unsigned long long *n, unsigned long long *n_workers);

/* The combined slot offsets of a method's buckets (n_buckets + 1 values): the work partition of
 * the count kernels. */
int lsq_debug_slot_offsets(lsq_ctx *c, int method, unsigned long long *out, unsigned long long n);
/* The share plan of a count launch as lsq_count makes it, on given numbers (host only, no device): slot_off = the buckets' slot
 * offsets (n_buckets + 1), packed = 1 per bucket the streaming kernel visits, n1 / n2 / look1 / look2 = per bucket the records of
 * the one- and two-block pool and the walk's looks at each (null: every slot weighs the same), costs4 = {two-block record, walk
 * look, visit, taper}; writes grid + 1 bounds in slots. */
int lsq_debug_plan_shares(const unsigned long long *slot_off, const unsigned char *packed, const unsigned long long *n1, const unsigned long long *n2,
                          const unsigned *look1, const unsigned *look2, unsigned long long n_buckets, unsigned long long grid,
                          const double *costs4, int weighted, int snap, unsigned long long *cuts);
/* The compact pool record of a block, through the library's own pack and unpack helpers (host only, no device).  which = 0: a
 * block that starts `off` bases from the record's origin and is `len` long -- returns 0 when it does not fit a compact record,
 * else 1 with the record and the (start, end) it unpacks to; which = 1 / 2: the padding record of the one- / two-block pool
 * (block 1 of it) that is number `off` of its group and number `len` of its half group (1 to 15 each) -- returns 1 likewise:
 * padding unpacks to an empty block.  Negative: an error code. */
int lsq_debug_compact_record(int which, long long off, long long len, uint32_t *rec, int32_t *start, int32_t *end);
/* An offset table of a method -- which = 0: slots per bucket, 1 / 2: the one- / two-block pool per bucket (n_buckets + 1
 * values each), 3: the share bounds of the count launch's streaming workgroups (their number + 1), 4 / 5: the ingest's
 * estimate of the one- / two-block reads per bucket that the streaming loops leave to the general walk; *n = values written. */
int lsq_debug_offsets(lsq_ctx *c, int method, int which, unsigned long long *out, unsigned long long cap, unsigned long long *n);

/* Another placement of the events in the EM grid (sixteen per wave; 0xFFFFFFFF = empty place):
 * the first n_small_places entries go to the lean kernel and must be events with at most two
 * isoforms and one (method, class) pair per lane.  Results do not depend on the placement
 * (tests/test_parity_gpu.py::test_em_numbers_do_not_depend_on_which_events_share_a_wave). */
int lsq_debug_set_em_order(lsq_ctx *c, const uint32_t *order, unsigned n_small_places, unsigned n_places);

/* Which kernels the latest lsq_solve launched for the EM, from the launch code's own bookkeeping -- so that a test of one form of the
 * EM can hold that this form ran, and a silent choice of another cannot pass as it (tests/test_em_direct_gpu.py).  Waits for the
 * context's streams.  out[0]: the form the lean group (events with at most two isoforms and four (method, class) pairs) went through,
 * the library's EmForm (csrc/lsq_device.hpp) -- 0 EM_FORM_NONE: there is none, 1 EM_FORM_QUAD: four lanes an event, 2 EM_FORM_QUAD_CAPPED:
 * four lanes an event with a cap on the passes, then lsq_em_tail_kernel (option em_quad_cap), 3 EM_FORM_HEAD_TAIL: lsq_em_head_kernel, then
 * the closed form in lsq_em_tail_kernel (option em_closed_form), 4 EM_FORM_QUAD_FLAT3 / 5 EM_FORM_QUAD_FLAT4: four lanes an event below the
 * split and one lane an event from it on, with three / four slots an event (one / several read files);
 * out[1]: the places of the lean group (events and holes; sixteen to a wave of the four-lane form);
 * out[2]: the split -- the first place solved one lane per event, read back from the device; out[1] when no place was;
 * out[3]: the places of the general kernel (lsq_em_kernel);
 * out[4]: 1 when the lean places were in an order learnt from an earlier solve's iteration counts (option em_regroup);
 * out[5]: the cap of form 2, else 0;  out[6]: 1 when a new order was learnt behind this solve;  out[7]: the step lane (0 / 1). */
int lsq_debug_last_em_launch(lsq_ctx *c, unsigned out[8]);

/* The rate a plain streaming read of `bytes` of device memory reaches on this device, in GB/s (best launch over
 * eight grid / unroll combinations): the practical ceiling bench.py reports beside the nominal HBM peak. */
int lsq_debug_stream_read_rate(lsq_ctx *c, unsigned long long bytes, double *gb_per_s);

/* Throws a C++ exception below the boundary -- kind 0: std::bad_alloc, 1: std::length_error, 2: an int -- so that a test
 * can see what a caller gets: LSQ_E_INTERNAL and a message, never std::terminate (lesseq_hip.h "no exceptions across
 * the boundary").  kind 3 does the same from inside a helper thread of a ThreadGroup (lsq_internal.hpp). */
int lsq_debug_throw(int kind);

/* Which of the device parse's three kernels the latest MRF text of the context went through (lsq_reads_upload_mrf / _text): tiles the
 * fast kernel handed to the byte-walking kernel (more delimiters than its LDS tables hold), lines it handed to the shared splitter
 * (another shape than a read's), and whether the whole file went through the byte-walking kernel (more than 64 chromosomes, or a line
 * list that ran over).  A file of reads: 0, 0, 0 -- a test holds that, so that a silent fall-back cannot pass as the fast path. */
int lsq_debug_last_parse_paths(const lsq_ctx *c, unsigned *tiles_handed, unsigned *lines_listed, unsigned *all_slow);

/* The staging and the inflate kernel of the BAM_SINGLE chain alone (lsq_bam_device.hpp): the bytes of a BGZF file to HBM, every
 * block through the inflate kernel, the inflated stream back into out (cap bytes; *n = its length, also when cap is too small:
 * LSQ_E_RANGE then).  Status as lsq_bam_parse for the block chain and the deflate streams. */
int lsq_debug_bgzf_inflate(lsq_ctx *c, const void *bytes, uint64_t len, void *out, uint64_t cap, uint64_t *n);

/* The same staging and inflate, then the CRC32 pass of the chain (lsq_bgzf_crc_kernel) without its comparison: the checksum the
 * device COMPUTED for every block's inflated bytes, in file order, into crc (cap entries; *n = the number of blocks, also when
 * cap is too small: LSQ_E_RANGE then).  The stored values are not looked at; a test holds the result against zlib. */
int lsq_debug_bgzf_crc32(lsq_ctx *c, const void *bytes, uint64_t len, uint32_t *crc, uint64_t cap, uint64_t *n);

/* The device prefix sum alone (csrc/lsq_scan.hpp, device_scan): in (n values) uploaded, scanned on the context's stream, and
 * out[i] = the sum of f(in[0 .. i)) copied back, out[n] the total (n + 1 values; n == 0 gives out[0] == 0).  form names the
 * instantiations the library uses -- 0: 32-bit values as they are, 1: 32-bit values as 0 / 1 flags, 2: 64-bit values as they
 * are, 3 / 4: 32-bit values rounded up to a multiple of the two-block / one-block pool's group padding (P2_GROUP_PAD /
 * P1_GROUP_PAD of csrc/lsq_device.hpp); in holds uint64_t for form 2 and uint32_t otherwise.  Another form: LSQ_E_ARG. */
int lsq_debug_scan(lsq_ctx *c, int form, const void *in, uint64_t n, uint64_t *out /* n + 1 */);

/* The device radix sort alone (csrc/lsq_sort.hpp, device_radix_sort): the n records (w0[i], w1[i]) sorted in place, stably, by
 * the 8-bit digits that begin at the bit positions bits[0 .. n_bits) of the 128 bits w1:w0 (bit 64 + k = bit k of w1), least
 * significant first as listed; bits that no digit names ride along.  With drop_constant_digits the digits on which all
 * records agree are left out first (sort_digits), as the library's callers do.  *n_passes = the digits sorted by (0 for fewer
 * than two records, which take no pass).  A position above 120 or more than 16 digits: LSQ_E_ARG. */
int lsq_debug_sort(lsq_ctx *c, uint64_t *w0, uint64_t *w1, uint64_t n, const unsigned *bits, unsigned n_bits,
                   int drop_constant_digits, unsigned *n_passes);

/* The log-likelihood lsq_as_betabin maximises, alone (csrc/lsq_as.hip, bb_loglik -- the device function the fit itself calls): per
 * row r the sum over its n_samples samples of l_j(mu[r], rho[r]), y and n [n_rows][n_samples] whole numbers with
 * 0 <= y <= n, 0 <= mu <= 1, 0 <= rho < 1; -inf where a sample has y > 0 at mu = 0 or y < n at mu = 1.  1 <= n_samples <= 8192.
 * tests/test_betabin_gpu.py holds it against mpmath's loggamma. */
int lsq_debug_as_bb_loglik(lsq_ctx *c, uint64_t n_rows, int n_samples, const double *y, const double *n, const double *mu, const double *rho,
                           double *out);

/* HIP_VERSION the library was compiled against and hipRuntimeGetVersion() of the runtime it found in the process (0
 * when that call fails, e.g. without a driver): a binding that loads another runtime first (PyTorch's) can compare. */
int lsq_debug_hip_versions(int *compiled, int *runtime);

/* The covered regions the load-time filter tests a block against, as [start, end) pairs in ascending order: those of the
 * chromosome (unstranded events; `minus` is ignored), or of the chromosome's plus (minus = 0) or minus (minus = 1) genes
 * (stranded events, lsq_events_compile_library).  Returns their number and writes at most `capacity` of them; -1 for a bad
 * argument.  The tests hold a stranded compile's regions against those of the two split compiles with it. */
int64_t lsq_debug_events_covered(const lsq_events *e, const char *chrom, int minus, int64_t *starts, int64_t *ends, int64_t capacity);

/* The shortcut table of a packed bucket as the count kernels' streaming loops read it (host only, no device; csrc/lsq_internal.hpp
 * "Shortcut table of a packed bucket"): the Cell and CellX records of bucket `bucket`, copied out of its compiled image in start
 * order -- lo / hi: the cell, e1 / e2: its two thresholds, info: owner event (index in the bucket) << 8 | segment << 2 | "lo is the
 * segment's start", or CELL_INFO_SHARED / CELL_INFO_EMPTY, flags: CELLX_BOTH, the two no-abut flags and, in the low 16 bits, the
 * event of the owner that ends last.  Returns the number of cells and writes at most `capacity` of them; 0 for a bucket without
 * cells (generic records, or evaluated on the host); -1 for a bad argument.  tests/test_count_cells_host.py holds them against a
 * plain model over every base of the bucket (tests/count_cells_ref.py). */
int64_t lsq_debug_bucket_cells(const lsq_events *e, int64_t bucket, int32_t *lo, int32_t *hi, int32_t *e1, int32_t *e2, uint32_t *info, uint32_t *flags,
                               int64_t capacity);
/* The events of a bucket in the bucket's own order (span start, span end, output index), as output indices -- what the event
 * numbers of the cells refer to -- and the bucket's kind (0 generic records, 1 packed, 2 evaluated on the host; kind may be NULL).
 * Returns their number and writes at most `capacity`; -1 for a bad argument. */
int64_t lsq_debug_bucket_events(const lsq_events *e, int64_t bucket, int *kind, int64_t *events, int64_t capacity);

/* The locator grid as uploaded, read back from the device: its shift, the number of chromosome tables, and of the first `cap` of
 * them the first base of bin 0 and the number of bins (0: a table without a record). */
int lsq_debug_locator(lsq_ctx *c, unsigned *shift, unsigned long long *n_tables, int64_t *loc_base, unsigned long long *loc_nb, unsigned long long cap);
/* The tables lsq_events_upload makes of compiled events (csrc/lsq_upload_tables.hpp), as the host works them out: no context, no
 * device.  Writes at most `cap` values of table `which` to `out` (may be NULL with cap 0) and their number to *n.  Values are 32-bit
 * words unless said otherwise; records are laid out field by field.  tests/test_upload_tables_host.py holds each table against its
 * definition. */
enum {
	LSQ_UT_EM_ORDER = 0,        /* device event per EM place, 0xFFFFFFFF padding */
	LSQ_UT_EM_PLACES = 1,       /* places of the lean group, all places */
	LSQ_UT_PACK_CLS = 2, LSQ_UT_PACK_ISO = 3, LSQ_UT_PACK_EV = 4,      /* lsq_results_pack_device's lists, output order */
	LSQ_UT_START_WEIGHTS = 5,   /* G = 1 / ARS, doubles, [read file][device isoform] */
	LSQ_UT_ROUTE_CHROM = 6,     /* per table id: loc_first, loc_nb, loc_base (signed), cov0, cov1, clu0, clu1, 0 */
	LSQ_UT_ROUTE_COV = 7,       /* covered regions: start, end (signed) */
	LSQ_UT_ROUTE_CLU = 8,       /* cluster records: start, end, bucket, the bucket's first base (signed) */
	LSQ_UT_ROUTE_LOC = 9,       /* locator entries: lower bound among the covered starts, among the cluster starts */
	LSQ_UT_ROUTE_SHIFT = 10,    /* the locator's shift, the number of table ids */
	LSQ_UT_BIN_BASE = 11, LSQ_UT_CELL_BASE = 12, LSQ_UT_JGROUP_BASE = 13,      /* per bucket, n_buckets + 1 values each */
	LSQ_UT_GROUP_TOTALS = 14,   /* bins, one-block groups, two-block groups */
	LSQ_UT_GENE_NAMES = 15,     /* bytes: the gene names in device event order, back to back */
	LSQ_UT_GENE_NAME_OFF = 16,  /* their offsets, n_events + 1 */
	/* two inputs of the group bases, straight from the compiled events: what the test sums up itself */
	LSQ_UT_BUCKET_BINS = 17,    /* per bucket: its bins (BucketDesc::n_bins) */
	LSQ_UT_JG_BASE = 18         /* per bucket: the first of its junction-group keys (lsq_events::jg_base), n_buckets + 1 */
};
int lsq_debug_upload_tables(const lsq_events *e, int which, void *out, unsigned long long cap, unsigned long long *n);

/* The read bootstrap's draws one by one (host only, no device; csrc/lsq_philox.hpp): the classes (1-based) that the draws
 * first_draw .. first_draw + n_draws - 1 of replicate b take for read file m (< 256) and event e (the generator's event
 * number) whose n_cls classes hold class_count reads -- so that a test can look at the first draws of an event of 2^40
 * reads without making them all.  LSQ_E_RANGE when the draws run past the event's reads. */
int lsq_debug_bootstrap_draws(uint32_t n_cls, const uint64_t *class_count, uint64_t seed, uint32_t m, uint32_t e, uint32_t b, uint64_t first_draw,
                              uint64_t n_draws, uint32_t *cls);
/* Device milliseconds of the latest lsq_bootstrap's three phases -- resampling, EM, summaries; the first two summed over
 * its chunks -- when it ran with lsq_set_timing on (LSQ_E_STATE otherwise), and the replicates a chunk held (chunk may be NULL). */
int lsq_debug_bootstrap_times(lsq_ctx *c, float ms[3], unsigned *chunk);

#ifdef __cplusplus
}
#endif
#endif
