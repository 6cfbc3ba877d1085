// Shared by the HIP translation units of the device group (not part of the ABI): device buffers, the
// per-read-file state, the context, and the entry points one unit offers the others.
//   lsq_device.hip  context, event tables, result fetch         lsq_count.hip  count kernels
//   lsq_ingest.hip  loader chain (filter, partition, pools)      lsq_em.hip     EM kernel
//   lsq_text.hip    texts staged in HBM, their newline tiles     lsq_readfile.hip  read files parsed on the device
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "lsq_internal.hpp"

using namespace lsq;

#define HIP_TRY(expr)                                                                          \
	do {                                                                                       \
		hipError_t _e = (expr);                                                                \
		if (_e != hipSuccess) return fail(LSQ_E_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
	} while (0)


#ifndef LSQ_P1_PAD
#define LSQ_P1_PAD 8
#endif
#ifndef LSQ_P2_PAD
#define LSQ_P2_PAD 4
#endif
constexpr unsigned P2_GROUP_PAD = LSQ_P2_PAD;      // ... and a junction group of the two-block pool (eight, with eight two-block reads per look, measured 2 % slower on C3: more padding, longer steps)
constexpr unsigned P1_GROUP_PAD = LSQ_P1_PAD;      // records a cell's group of the one-block pool is padded to: what a lane of the count kernel takes per look
constexpr int LSQ_INGEST_STAGES = 7;     // newline count, route, partition count, partition scatter, group classify, group offsets, group place
constexpr int LSQ_INGEST_PASS_MAX = 16;  // ... and room for the passes a read file clocks ahead of its route (a BAM file: inflate, CRC32s, record starts)
constexpr int LSQ_COUNTER_SETS = 3;  // counter sets a context holds (lsq_ctx::set)

namespace lsq {

// Compact pool records.  A block is (end << 10 | length): 22 bits for where it ENDS, 10 bits of length, so that an unsigned
// compare of whole records orders blocks by their end -- all that the count kernel's loops ask of most records.  The end of a
// read's first block counts from the bucket's first base minus COMPACT_BIAS (the first bin of a bucket also holds reads that
// start before it), that of its second block from the end of the first (the bases between them plus its length: the
// "reach").  One-block reads take one such word, two-block reads two.  Reads with a longer block or a farther end are kept
// with the many-block reads.  The largest end value is kept for the padding of the one-block pool (COMPACT_PAD).
constexpr unsigned COMPACT_END_BITS = 22, COMPACT_LEN_BITS = 10, COMPACT_LEN_MASK = (1u << COMPACT_LEN_BITS) - 1u, COMPACT_MAX_LEN = 1u << COMPACT_LEN_BITS;
constexpr unsigned COMPACT_END_MAX = (1u << COMPACT_END_BITS) - 2u;      // the farthest end of a block
constexpr int COMPACT_BIAS = 1 << 21;
__host__ __device__ inline bool compact_block_fits(long long off, long long len) {
	return off >= 0 && len > 0 && len < (long long)COMPACT_MAX_LEN && off + len <= (long long)COMPACT_END_MAX;
}
// a block that starts `off` bases in and is `len` long (compact_block_fits holds), and back: where it starts and ends
__host__ __device__ inline unsigned compact_pack(const unsigned off, const unsigned len) { return ((off + len) << COMPACT_LEN_BITS) | len; }
// Padding of a group.  One-block pool: COMPACT_PAD | ranks, above every block and every threshold; two-block pool: block 1 =
// ranks << 10 (an empty block), block 2 = 0, below every block and every threshold but "nothing".  ranks: which padding record of
// its aligned group this is, counted from 1 (bits 0-3), and which of its aligned half group (bits 4-7): the last record a
// lane holds tells it how many of its records are padding, whether it takes a whole group per step or half of one.
constexpr unsigned COMPACT_PAD = ((1u << COMPACT_END_BITS) - 1u) << COMPACT_LEN_BITS;
__host__ __device__ inline bool compact_is_pad1(const unsigned rec) { return rec >= COMPACT_PAD; }
__host__ __device__ inline unsigned compact_pad_ranks(const unsigned in_group, const unsigned in_half) { return in_group | (in_half << 4); }
__host__ __device__ inline unsigned compact_pad1(const unsigned in_group, const unsigned in_half) { return COMPACT_PAD | compact_pad_ranks(in_group, in_half); }
__host__ __device__ inline unsigned compact_pad2_a(const unsigned in_group, const unsigned in_half) { return compact_pad_ranks(in_group, in_half) << COMPACT_LEN_BITS; }
// (padding unpacks to an empty block: of the one-block pool by the test here, of the two-block pool -- POOL2: no test -- by its own bits)
template <bool POOL2 = false>
__host__ __device__ inline void compact_unpack(const unsigned rec, int &off, int &end) {
	end = (int)(rec >> COMPACT_LEN_BITS);
	off = end - ((!POOL2 && compact_is_pad1(rec)) ? 0 : (int)(rec & COMPACT_LEN_MASK));
}
// "ends by e" for a whole record.  One-block pool: rec <= compact_ends_by(e) -- no block for e < 0, no padding ever.
// Two-block pool: rec < compact_past(e) -- no block and no padding for e < 0, blocks and the padding (0) for e >= 0.
__host__ __device__ inline unsigned compact_ends_by(const int e) {
	return e < 0 ? 0u : ((((unsigned)e < COMPACT_END_MAX ? (unsigned)e : COMPACT_END_MAX) << COMPACT_LEN_BITS) | COMPACT_LEN_MASK);
}
__host__ __device__ inline unsigned compact_past(const int e) { return e < 0 ? 0u : compact_ends_by(e) + 1u; }

// A (read, event) pair the fast kernel does not settle itself: span-start ties that need the
// strand/name order, two-block reads whose blocks touch, second looks that did not fit the LDS
// queue.  pool 0 = one-block pool, 1 = two-block pool; scan: continue with the following events.
struct ExcEntry {
	unsigned long long slot;       // index into the pool
	unsigned bucket;
	unsigned ev_pool_scan;         // event index in the bucket | pool << 29 (0 one block, 1 two blocks, 2 n blocks) | scan << 31
};

template <class T>
struct DevBuf {
	T *p = nullptr;
	size_t n = 0;
	~DevBuf() { if (p) (void)hipFree(p); }
	int alloc(size_t count) {
		if (p) { (void)hipFree(p); p = nullptr; }
		n = count;
		HIP_TRY(hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T)));
		return LSQ_OK;
	}
	int upload(const T *src, size_t count, hipStream_t st) {
		int rc = alloc(count);
		if (rc) return rc;
		if (count) HIP_TRY(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
		return LSQ_OK;
	}
};

template <class T>
struct DevView { T *p = nullptr; size_t n = 0; };     // a slice of somebody else's allocation

// The device times of a tool's N phases: N + 1 events, phase k between marks k and k + 1 (once the stream has been waited for).
// mark and ms hand on the runtime's status, for the caller to check or to ignore.
template <int N>
struct PhaseClock {
	hipEvent_t ev[N + 1] = {};
	~PhaseClock() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
	int make() { for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e)); return LSQ_OK; }
	hipError_t mark(int k, hipStream_t st) { return hipEventRecord(ev[k], st); }
	hipError_t ms(int k, float *out) { return hipEventElapsedTime(out, ev[k], ev[k + 1]); }
};

// workgroups of a launch over `items` at `per_block` a workgroup (at least one) ...
inline unsigned grid_for(unsigned long long items, unsigned per_block) {
	return (unsigned)std::max<unsigned long long>(1, (items + per_block - 1) / per_block);
}
// ... and no more than `per_cu` a compute unit (kernels that stride over their items)
inline unsigned grid_for(int n_cu, unsigned long long items, unsigned per_block, unsigned per_cu) {
	const unsigned long long want = (items + per_block - 1) / per_block, cap = (unsigned long long)n_cu * per_cu;
	return (unsigned)std::max<unsigned long long>(1, std::min(want, cap));
}

// What a workgroup of the count kernel needs to know about one visit to a bucket, in one 128-byte record per (read file,
// bucket), written once per read set (ingest): the bucket's description, where its slots and its one- and two-block
// records lie, and the next packed bucket that holds any.  A wave reads it with scalar loads -- one memory round trip
// where the kernel used to chase the description, three offset arrays and the bucket search one after the other.
struct VisitRec {
	BucketDesc d;
	unsigned long long bs, be;               // the bucket's slots
	unsigned long long p1o, p1n, p2o, p2n;   // first record and number of records of its one- and two-block pools
	unsigned b, next;                        // this bucket; the next packed bucket with slots (n_buckets: none)
	unsigned pad[2];
};
static_assert(sizeof(VisitRec) == 128, "VisitRec is read as 32 dwords");
// A workgroup's share of a count launch with the visit record of its first bucket beside it: one scalar load at the start of the
// workgroup where the share's bounds, its first bucket and that bucket's record were three, two of them one after the other.
struct WgPlan {
	unsigned long long s_begin, s_end;       // the share, in slots
	VisitRec first;                          // (b == n_buckets: the share holds no packed bucket's slots)
};
static_assert(sizeof(WgPlan) == 144, "WgPlan layout");

// one pass of the loader as the stage report knows it: its name, the events around its launches, the bytes it has to move at
// least, its device time (read once the stream has been waited for)
struct IngestPass {
	const char *name = nullptr;
	hipEvent_t ev[2] = {nullptr, nullptr};
	unsigned long long bytes = 0;
	float ms = 0;
	bool clocked = false;                  // by the latest ingest (a pass it lists and does not run reports zeros)
};

struct MethodReads {
	DevBuf<ExcEntry> exc;                  // exception lists: LSQ_COUNTER_SETS stretches of exc_cap entries, one per counter set
	size_t exc_cap = 0;
	bool present = false;
	uint64_t n_retained = 0, n_retained_blocks = 0, total_slots = 0;
	uint64_t lib_report[5] = {0, 0, 0, 0, 0};      // stranded jobs: lsq_last_library_report
	// one- and two-block pools: wide records (2 / 4 ints a read), or compact ones (1 / 2 ints a read, see COMPACT_*) when
	// at least 15 of 16 such reads fit them; compact pools are padded to whole 16-byte words
	DevBuf<int32_t> p1, p2, pn_se;
	bool compact = false;
	uint64_t n1_reads = 0, n2_reads = 0;    // one- and two-block reads in the pools (their slots also hold the groups' padding)
	DevBuf<uint8_t> p1_strand, p2_strand, pn_strand;
	DevBuf<uint32_t> p1_line, p2_line, pn_line, pn_blk_off, pn_nblk, pn_bucket;
	DevBuf<unsigned long long> p1_off, p2_off, pn_off, pnb_off, slot_off;
	double skew = 1.0;                      // reads of the fullest bucket / mean reads per bucket
	bool named = false;                     // the reads carry their own names (the *_line arrays index name_off)
	DevBuf<char> names;
	DevBuf<unsigned long long> name_off;
	DevBuf<unsigned> wg_first;             // per workgroup of the fast kernel's grid (`wg_grid` of them): the bucket its share starts in
	DevBuf<unsigned long long> wg_cut;     // ... and the shares' bounds in slots (wg_grid + 1 values)
	DevBuf<WgPlan> wg_plan;                // the same per workgroup, with its first visit record: what the kernel reads
	std::vector<VisitRec> visits_host;     // (for the plan)
	std::vector<unsigned long long> slot_off_host;   // the buckets' slot offsets (n_buckets + 1), for the share plan
	DevBuf<VisitRec> visits;               // per bucket (n_buckets + 1: the last one ends every chain)
	std::vector<unsigned long long> plan_n1, plan_n2;   // per bucket: records of the one- / two-block pool (padding included) ...
	// ... the same by cell and junction group, as stretches of slots (plan_share_cuts_seg): x[0 .. S] bounds, kind (0 one-block records, 1 two-block, 2 the rest),
	// the walk's looks at the stretch's reads, and per bucket its first stretch
	std::vector<unsigned long long> plan_seg_x;
	std::vector<unsigned char> plan_seg_kind;
	std::vector<unsigned> plan_seg_looks, plan_seg_first;
	std::vector<unsigned> plan_park1, plan_park2;       // ... and the looks of the general walk at the reads of each that the streaming loops leave to it (the ingest's estimate)
	std::vector<unsigned> next_packed_host;          // per bucket b: the first packed bucket >= b that holds slots (n_buckets: none), for the share plan
	unsigned long long wg_grid = 0;
};

} // namespace lsq

// how the lean group ran: out[0] of lsq_debug_last_em_launch, each form described there (include/lesseq_hip_dev.h)
enum EmForm : unsigned { EM_FORM_NONE = 0, EM_FORM_QUAD = 1, EM_FORM_QUAD_CAPPED = 2, EM_FORM_HEAD_TAIL = 3, EM_FORM_QUAD_FLAT3 = 4, EM_FORM_QUAD_FLAT4 = 5 };
// EmState::split: per step lane the first place of the one-lane-per-event form, written by the lane's regroup kernel; then a word that stays 0xFFFFFFFF
// (every place to the four-lane form) and the copy of a lane's word taken before the regroup kernel behind a launch wrote the next split into it
enum : unsigned { EM_SPLIT_NONE = 2, EM_SPLIT_KEPT = 3, EM_SPLIT_WORDS = 4 };
struct EmLane {                         // per step lane
	// Regrouping (option "em_regroup", on by default): a wave of the lean EM kernel runs until the slowest of its sixteen
	// events has converged, so events that take about as many iterations should share waves.  After a solve, a small kernel
	// on the same lane sorts the lean group's places by the iteration counts that solve just wrote; the lane's next solve
	// (two steps later) and the fifteen after it use that order.  A prediction, nothing more: an event's numbers do not depend on its wave mates.
	lsq::DevBuf<uint32_t> order;
	bool order_valid = false;
	unsigned age = 0;                   // solves since the order was last refreshed (every 16th solve refreshes it)
	// the list a capped or headed EM leaves for lsq_em_tail_kernel: event | iterations, flag, theta_0 | theta_1 | log-likelihood
	lsq::DevBuf<uint32_t> tail_u32;
	lsq::DevBuf<uint8_t> tail_flag;
	lsq::DevBuf<double> tail_f64;
};
// what the latest run_solve launched (lsq_debug_last_em_launch): host bookkeeping, no kernel knows of it
struct EmLaunch {
	unsigned form = EM_FORM_NONE, lean = 0, general = 0, cap = 0, lane = 0, split_word = EM_SPLIT_NONE;      // lean, general: places; split_word: the word of EmState::split the lean launch read
	bool learnt = false, regrouped = false;
};
struct EmState {                        // the EM of a context: placement, options, bookkeeping (lsq_em.hip: run_solve; lsq_device.hip: lsq_events_upload, options, developer aids)
	EmLane lane[2];
	EmLaunch last;
	lsq::DevBuf<uint32_t> order;        // device event per place of the EM grid, as lsq_events_upload laid them out
	lsq::DevBuf<uint32_t> split;        // EM_SPLIT_WORDS words
	lsq::DevBuf<uint32_t> tail_count;   // per lane: events on its tail list, tail workgroups done
	unsigned places = 0;
	unsigned small_places = 0;          // the first of them: events of the lean EM kernels
	bool opt_regroup = true;
	// "em_closed_form" (default off): two-isoform events with one read file run a few ordinary iterations and finish in the
	// closed form of their EM map (lsq_em.hip: lsq_em_head_kernel / lsq_em_tail_kernel)
	bool opt_closed = false;
	// "em_quad_cap" (0: off): the four-lane lean kernel hands events that still run after that many iterations to lsq_em_tail_kernel
	// (two-isoform events with one read file, where no placement by earlier iteration counts is in use: lsq_em.hip)
	unsigned opt_quad_cap = 0;
	unsigned opt_flat_min = 16384;      // "em_flat_min_events": lean events from which on the fast ones run one lane per event
	// room on both lanes' tail lists for `np` lean places (they only grow)
	int reserve_tails(size_t np) {
		np = std::max<size_t>(np, 1);
		for (EmLane &l : lane)
			if (l.tail_flag.n < np) { int rc; if ((rc = l.tail_u32.alloc(2 * np)) || (rc = l.tail_flag.alloc(np)) || (rc = l.tail_f64.alloc(3 * np))) return rc; }
		return LSQ_OK;
	}
};

// The read bootstrap of a context (lsq_boot.hip): the replicates' theta and their summaries, kept until the next
// lsq_bootstrap, a new event set or the end of the context
struct BootState {
	lsq::DevBuf<double> theta;          // [B][n_iso], device isoform order
	lsq::DevBuf<double> stats;          // [5][n_iso]: mean, sd, quantiles 0.025, 0.5, 0.975
	lsq::DevBuf<uint32_t> n_ok;         // [n_iso]: replicates with a finite theta
	unsigned B = 0;
	bool done = false;
	unsigned opt_chunk = 0;             // "bootstrap_chunk": replicates resampled and solved per launch (0: by BOOT_CHUNK_BYTES)
	unsigned last_chunk = 0;            // ... and what the latest lsq_bootstrap took
	float ms[3] = {0, 0, 0};            // resample, EM, summary of the latest lsq_bootstrap that ran with lsq_set_timing
	bool timed = false;
};

// The loader's tables of a context, as lsq_events_upload made them (written in lsq_device.hip, read by lsq_ingest.hip: route_tables and
// the ingest chain).  Per table id a RouteChrom; the covered regions as (start, end) pairs; the clusters (spans of the planned
// events) as (start, end, bucket, bucket's first base), cut at the bucket cuts; and the locator grid over both (lsq_upload_tables.hpp
// says how each is made)
struct LoaderTables {
	lsq::DevBuf<lsq::RouteChrom> route_chrom;
	lsq::DevBuf<int2> cov;
	lsq::DevBuf<int4> clu;
	lsq::DevBuf<uint2> loc;
	unsigned loc_shift = 10;
	unsigned n_chrom_tables = 0;
	lsq::DevBuf<unsigned> bin_base;        // per bucket: first of its bins among all bins (n_buckets + 1)
	size_t n_fine = 0;
	// The one-block pool is laid out by cell (lsq_internal.hpp: Cell), not by bin: per bucket its cells in order and one more
	// group for the reads that start in no cell, every group padded to eight records (P1_GROUP_PAD) -- a lane of the count kernel takes four or eight
	// neighbouring records and decides them against one cell.  cell_base: per bucket the first of its groups (n_buckets + 1).
	lsq::DevBuf<unsigned> cell_base;
	size_t n_cell_groups = 0;
	// The two-block pool is laid out by junction group (lsq_events::jg_keys), every group padded to four records, and per
	// bucket one more group for the reads that cross no known junction.  jgroup_base: per bucket the first of its groups.
	lsq::DevBuf<unsigned long long> jg_keys;
	lsq::DevBuf<unsigned> jg_base, jgroup_base;
	size_t n_junction_groups = 0;
};

// lsq_fim (fim.h / linalg.h) of a context (lsq_device.hip: lsq_fim and its results; lsq_em.hip: run_fim): per device event the offset
// of its accessible-start class counts and of its (K-1) x (K-1) matrix; counts per method; results
struct FimState {
	lsq::DevBuf<uint32_t> start_base, mat_base, starts;
	lsq::DevBuf<double> mat, var;
	size_t starts_total = 0, mat_total = 0;
	bool uploaded = false, done = false;
};

// The costs of a count launch's share plan (lsq_count.hip: plan_share_cuts_seg says what each weighs).  The defaults here are
// those of a bare plan, which lsq_debug_plan_shares fills from its arguments; a context's are CountOptions::share, below.
struct SharePlanCosts { bool weighted = true, snap = true; double two_block = 4.3, walk_look = 9.0, visit = 7000.0, taper = 0.5, hot = 0.0; };

// What lsq_ctx_set_option keeps for run_count alone (lsq_count.hip; "recount_every_read" is also read where an overflow is reported)
struct CountOptions {
	// "count_streams": a lane's counts run on a stream of the lane's own (lsq_ctx::stream_count2); 1: every count on `stream`, one after the other
	bool two_count_streams = true;
	int wg_per_cu = -1;                     // "workgroups_per_cu": resident workgroups of the count kernel per compute unit
	int counter_sets = LSQ_COUNTER_SETS;    // "counter_sets": 2 or 3 (set only while nothing is in flight)
	int reads_per_look = 0;                 // "reads_per_look": 0 = by the launch, 4, 8
	double grid_mult = 0;                   // "grid_multiplier" (fractions allowed; 0 = by the read set's skew)
	bool recount = false;                   // "recount_every_read": recount every read with the one-lane-per-read kernel (self-check)
	unsigned cleanup_grid = 0;              // "cleanup_workgroups": workgroups of the exception pass (0: one a compute unit)
	// "share_weighted" (the shares equal in cost, not in reads), "snap_shares" (cut on bucket boundaries where one is near),
	// "share_cost_two_block" (a two-block record, in one-block records), "share_cost_parked" (one look of the general walk at a
	// parked read), "share_cost_visit" (staging + flush of a bucket), "share_taper" (the last share of the grid as a fraction of the
	// first; 0 = automatic, run_count's rule), "share_cost_hot" (extra cost a record of a group of 8 192 records or more)
	// A context's defaults differ from a bare plan's in two costs, and these are the two:
	SharePlanCosts share;
	CountOptions() {
		share.taper = 0.0;                  // 0 = automatic (0.25 or 0.5 by the read set's skew), where a bare plan has 0.5
		share.hot = 0.5;                    // where a bare plan has none
	}
};

// What run_count keeps between launches and reports of the latest one (lsq_count.hip; lsq_device.hip reads fast_launched for
// lsq_last_fast_kernel_ms, drops the occupancy answer with "workgroups_per_cu" and sets dev_ablate in the developer build)
struct CountLaunch {
	unsigned occ_lds_bytes = 0; int occ_p1w = 0, occ_blocks = 0;      // the runtime's occupancy answer for the fast kernel at that LDS size
	unsigned last_reads_per_look = 4, last_wg_per_cu = 0;       // what the latest lsq_count ran with
	int fast_launched = 0;                  // bit m: read file m's streaming kernel ran (evf0 / evf1 bracket it)
	lsq::DevBuf<unsigned char> recount_args;      // the recount kernels' argument records, and the host's copy of what was last written
	std::vector<unsigned char> recount_args_host;
	lsq::DevBuf<unsigned long long> wg_trace;     // developer build (LSQ_ABLATE 4194304): lsq_debug_wg_trace
	unsigned long long wg_trace_n = 0, wg_trace_workers = 0;
	unsigned dev_ablate = 0;                // developer build only (LSQ_ABLATE)
};

struct lsq_ctx {
	// lsq_ctx_create_with(LSQ_CTX_LANES_IN_BACKGROUND): the helper thread that makes the lanes' streams and events, and how it ended
	std::thread lanes_thread;
	int lanes_status = 0;
	std::string lanes_error;
	int device = 0;
	int n_cu = 256;
	hipStream_t stream = nullptr;           // uploads, ingest and the count kernels
	// The EM and the hand-off of results run on a stream of their own: the EM ends in a long tail
	// of a few slow events on an otherwise idle device, and the next lsq_count may run beside it.
	// So do the zeroing of the counters and the exception pass of a count (lsq_count_cleanup_kernel).
	// For that the counters and the exception lists exist more than once (counter sets, below: a count writes a set
	// whose readers are steps back); ev_counted: end of the latest count's streaming kernels; ev_mark: recorded
	// on the result stream when a count is submitted, behind the zeroing of the set of the count before -- the count
	// that takes that set next waits for it, i.e. for the readers of its set and not for the EMs in between.
	// ... and the streams exist twice, as two LANES that consecutive counts take in turn: a count stream, a result
	// stream, the EM's output arrays and ev_counted.  The EM of step k (a chain of dependent passes on a
	// handful of waves) then runs beside the exception pass and the EM of step k+1 instead of ahead of them: with small
	// shards (a rank of an event-sharded job) the result stream's chain, not the count kernel, bounded the step.
	hipStream_t stream_em = nullptr;        // the latest count's lane (= stream_em2[lane])
	hipStream_t stream_em2[2] = {nullptr, nullptr};
	// A lane's counts run on a stream of the lane's own: consecutive counts write different counter sets and share only
	// what they read, so the next count's workgroups may fill the compute units the tail of this one leaves idle, and no
	// dispatch waits for the kernel before it (option "count_streams" 1: every count on `stream`, one after the other).
	hipStream_t stream_count2[2] = {nullptr, nullptr};
	// LANE and COUNTER SET are two things.  The lanes stay two -- streams, ev_counted2, the EM's outputs -- and consecutive
	// counts take them in turn.  The counter sets (counters, exception lists, the exception pass's argument records, ev_mark2) are
	// LSQ_COUNTER_SETS, of which counts take the first `count_opt.counter_sets` in turn: with three, count k+1 waits for the readers of step k-2
	// and not for those of step k-1, whose chain (exception pass, EM, hand-off, zeroing) otherwise stands between two counts of a lane.
	// Every set but the latest count's is zero or has its zeroing queued, its mark recorded behind that: whichever comes next may be taken.
	hipEvent_t ev_counted2[2] = {nullptr, nullptr}, ev_mark2[LSQ_COUNTER_SETS] = {};
	bool mark_recorded2[LSQ_COUNTER_SETS] = {};
	int lane = 0;                           // lane of the latest count
	int set = 0;                            // counter set of the latest count
	size_t counters_per_set = 0;
	hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
	hipEvent_t evt0 = nullptr, evt1 = nullptr;      // around a text copy (lsq_text_stage may run beside other host work)
	hipEvent_t evf0[LSQ_MAX_METHODS] = {}, evf1[LSQ_MAX_METHODS] = {};   // around each method's lsq_count_fast_kernel launch
	CountOptions count_opt;
	CountLaunch launch;
	bool time_events = false;               // lsq_set_timing: event records around the kernels cost ~4 us each in the queue
	bool count_timed = false, solve_timed = false;      // the last lsq_count / lsq_solve ran with them
	lsq_events *E = nullptr;                // must outlive the uploads made from it (its strand dictionary grows with the reads)
	DevBuf<BucketDesc> buckets;
	DevBuf<uint8_t> images, strand_rank, dK;
	DevBuf<TieRec> ties;
	DevBuf<uint32_t> cls_base, iso_base, gene_name_off;
	DevBuf<char> gene_names;                // device event order
	DevBuf<uint32_t> pack_cls, pack_iso, pack_ev;      // lsq_results_pack_device: device index of every class / isoform / event of the shard, in output order
	EmState em;
	BootState boot;
	DevBuf<double> G, theta2[2], logll2[2];
	DevBuf<uint32_t> iters2[2];
	DevBuf<uint8_t> flags2[2];
	DevView<double> theta, logll;           // the latest count's lane
	DevView<uint32_t> iters;
	DevView<uint8_t> flags;
	FimState fim;
	DevBuf<unsigned long long> counters;   // LSQ_COUNTER_SETS sets of cnt | bases | exc_count | dbg (one memset per count); the views below are the latest count's
	DevView<unsigned long long> cnt, bases, dbg;
	DevView<unsigned> exc_count;           // per method: [2m] appended, [2m+1] overflow flag
	LoaderTables loader;
	size_t opt_exc_cap = 0;                 // "exception_capacity": entries of a method's exception list (0 = a quarter of its reads, at least 64 Ki)
	bool opt_compact_pools = true;          // "compact_pools": 0 keeps wide pool records whatever the reads look like
	bool overflow_logged[LSQ_MAX_METHODS] = {};      // the warning about an overflowed exception list has been written for the latest count
	MethodReads reads[LSQ_MAX_METHODS];
	bool counted = false, solved = false;
	bool counts_external = false;           // lsq_results_set_counts: the counts are sums the reads here do not explain
	double em_band = 1E-11;                 // lsq_set_em_guard_band: events whose stop test comes this close to its threshold are replayed
	bool has_fast = false, has_generic = false, has_host = false;
	uint64_t host_genes = 0, host_reads = 0;     // host buckets of the latest count: their events, and the reads their clusters held
	std::map<size_t, std::vector<unsigned short>> host_seq;     // host buckets: [device event * M + method] -> classes of its valid reads, index order
	float count_ms = 0, solve_ms = 0;
	float mrf_h2d_ms = 0, mrf_parse_ms = 0;
	// how the latest device parse went (lsq_debug_last_parse_paths): tiles handed to the byte-walking kernel, lines handed to the shared
	// splitter, and whether the whole file went through the byte-walking kernel
	unsigned parse_tiles_handed = 0, parse_lines_listed = 0, parse_all_slow = 0;
	// SAM_SINGLE read files (lsq_sam_device.hpp): which records make no read ("sam_skip_flags", "sam_min_mapq") and what the
	// kernels of the latest one handed on (lsq_last_sam_paths)
	unsigned opt_sam_skip_flags = 0x904u, opt_sam_min_mapq = 0u;
	bool opt_bam_verify = false;            // "bam_verify": BAM_SINGLE files have their blocks' CRC32s and their end-of-file marker checked (lsq_bam_device.hpp)
	unsigned sam_lines_listed = 0, sam_all_slow = 0;
	unsigned long long bam_blocks = 0, bam_blocks_repaired = 0;      // the latest BAM_SINGLE file (lsq_last_bam_paths)
	// two pinned 32 MiB host buffers and their "drained" events, made at the first large host-to-device copy (lsq_text.hip: pinned_pipeline)
	unsigned char *pin_buf[2] = {nullptr, nullptr};
	hipEvent_t pin_ev[2] = {nullptr, nullptr};
	// the passes of the latest ingest in the order in which they were first clocked (lsq_text.hpp: StageClock; lsq_ingest.hip:
	// lsq_last_ingest_stages): the first ing_n entries, of which the latest ingest listed -- and the report shows -- ing_reported
	IngestPass ing_pass[LSQ_INGEST_PASS_MAX];
	int ing_n = 0, ing_reported = 0;
};

// The text of one file in HBM (lsq_text_stage).  Staging needs no event tables: the executables start it
// on a second thread while the first is still reading the annotation.
struct lsq_text {
	std::string path;
	unsigned long long offset = 0, len = 0;        // the bytes [offset, offset + len) of the file
	lsq::DevBuf<unsigned char> d_text;
	float h2d_ms = 0;
	bool scanned = false;                           // newlines counted (lsq_text_lines or the parse)
	unsigned long long n_nl = 0;
	lsq::DevBuf<unsigned long long> d_tile_base;    // per tile of the text (lsq_text.hpp: TEXT_TILE bytes): newlines ahead of it (n_tiles + 1)
};

namespace lsq {
int upload_strand_ranks(lsq_ctx *c);                 // lsq_device.hip
int run_count(lsq_ctx *c);                           // lsq_count.hip
int run_solve(lsq_ctx *c);
int run_fim(lsq_ctx *c);
int run_boot_em(lsq_ctx *c, unsigned n_rep, const unsigned long long *cnt, double *theta, double *logll, unsigned *iters, unsigned char *flags);      // lsq_em.hip, for lsq_boot.hip
int sync_all(lsq_ctx *c);                 // both streams
int ensure_lanes(lsq_ctx *c);             // lsq_device.hip: joins a context's helper thread (lanes made in the background), once
void note_overflow(lsq_ctx *c, const std::vector<unsigned> &exc_count);      // lsq_device.hip: the warning about an overflowed exception list, once per count
int host_count(lsq_ctx *c);                          // lsq_replay.hip: host buckets (genes beyond the kernels' limits)
int host_solve(lsq_ctx *c);
int replay_flagged(lsq_ctx *c, unsigned *n_done);    // lsq_replay.hip: the EM of guard-band events in the reference's per-read order
void select_counter_set(lsq_ctx *c, int lane, int set);                 // lsq_device.hip: the views of the latest count's lane and counter set
} // namespace lsq
