// What a routing kernel of the loader needs, whichever front end it belongs to (lsq_ingest.hip: parsed blocks from the host;
// lsq_mrf_device.hpp, lsq_sam_device.hpp, lsq_bam_device.hpp: a read file's own bytes); not a public header.
// Needs: lsq_device.hpp (RouteChrom, the compact record's limits).  Gives: the tables a routing pass searches (RouteTables) and what
// it leaves behind (RouteOut, the ROUTE_* keys); the containment filter against the covered regions (route_covered) and the chromosome
// records staged in LDS (route_stage_chroms); the blocks of one read merged as they come, then routed (ReadAcc, ReadBig).
#pragma once
#include "lsq_device.hpp"

constexpr int INGEST_MAX_BLOCKS = 16;                  // merged blocks per read the device ingest handles

// ---- what the routing pass knows and what it leaves behind ------------------------------------------------------------
struct RouteTables {
	const RouteChrom *chrom;       // per chromosome id (lsq_device.hpp); a kernel may point this at its own copy in LDS
	const int2 *cov;               // covered regions: (start, end), ascending per chromosome
	const int4 *clu;               // clusters (spans of the planned events) cut at the bucket cuts: (start, end -- inclusive --, bucket, bucket's first base)
	const uint2 *loc;              // locator grid (lsq_ctx::loc): entries k and k + 1 are read as one 16-byte pair
	unsigned loc_shift;
	unsigned n_chrom;
};
constexpr unsigned ROUTE_CHROM_LDS = 64;      // chromosome records a kernel stages in LDS (more chromosomes: read from global memory)

// A read's key: pool in bits 0-1 (0 one merged block, 1 two, 2 three or more, 3 one or two that do not fit compact
// records), bucket in bits 2-23, strand id in bits 24-31.  Bucket 0x3FFFFF: not routed -- dropped (all ones), or
// retained by the filter but a candidate of no planned event (low bits 01, the number of its merged blocks in bits 24-31).
constexpr unsigned ROUTE_KEY_DROPPED = 0xFFFFFFFFu;
constexpr unsigned ROUTE_NO_BUCKET = 0x3FFFFFu;
__host__ __device__ inline unsigned route_key(unsigned bucket, unsigned pool, unsigned strand) { return (strand << 24) | (bucket << 2) | pool; }
__host__ __device__ inline unsigned route_key_unrouted(unsigned n_blocks) { return (n_blocks << 24) | (ROUTE_NO_BUCKET << 2) | 1u; }
__host__ __device__ inline bool route_key_is_routed(unsigned k) { return ((k >> 2) & ROUTE_NO_BUCKET) != ROUTE_NO_BUCKET; }

struct RouteOut {
	unsigned *key;                 // per read
	int4 *rec;                     // per read: its first two merged blocks (s0, e0, s1, e1)
	// reads of pools 2 and 3: a list (they are few in short-read files; a file of long reads fills it, and the ingest sizes it again)
	unsigned long long *nb_tot;    // [0] entries wanted, [1] blocks wanted, [2] error flag (a read beyond the tables' range); from [ROUTE_LIB_WORD0] on: a stranded pass's library report (LibTally)
	unsigned long long nb_cap, nbb_cap;
	uint4 *nb_ent;                 // read index, bucket, blocks | strand << 8, first block in nb_blk
	int2 *nb_blk;
	unsigned *cntn, *cntnb;        // per bucket: such reads, their blocks
	unsigned compact;              // compact pool records: one- and two-block reads that do not fit them go to pool 3
};

// ---- stranded jobs.  Every routing kernel has a stranded form, a template parameter: it derives the transcript
// strand t of a record (0 plus, 1 minus, ROUTE_NO_STRAND none), and everything it does with the record's chromosome -- the
// chromosome record, route_covered, ReadAcc::add / finish, route_cluster -- it does with the TABLE id route_table(chromosome, t)
// instead (lsq_events::table_of); a record without t makes no read; the read carries t's string as its strand.  The word `lib`
// such a kernel takes as its last argument (route_lib_word): bit 0 -- the library is `reverse`; bits 8-15 / 16-23 -- the strand
// ids of "+" / "-".  The argument is a parameter pack, empty in the unstranded form (kernel<false>; kernel<true, unsigned>): that
// form's arguments, and so its code, are what they were before there was a stranded one.
constexpr unsigned ROUTE_NO_STRAND = 2u;
constexpr unsigned ROUTE_LIB_SLOTS = 1024u, ROUTE_LIB_WORD0 = 8u;      // the library report's places behind RouteOut::nb_tot: eight words each, five used
__host__ __device__ inline unsigned route_lib_word(bool reverse, unsigned plus_id, unsigned minus_id) { return (reverse ? 1u : 0u) | (plus_id << 8) | (minus_id << 16); }
__host__ __device__ inline unsigned route_lib_arg() { return 0u; }
__host__ __device__ inline unsigned route_lib_arg(unsigned lib) { return lib; }
__host__ __device__ inline unsigned route_table(unsigned chrom, unsigned t) { return 2u * chrom + t; }
// t of an alignment strand (minus: 0 / 1; SAM and BAM: already XOR mate2)
__host__ __device__ inline unsigned route_transcript(unsigned lib, unsigned minus) { return (minus ^ lib) & 1u; }
// ... of a strand id
__host__ __device__ inline unsigned route_transcript_of_id(unsigned lib, unsigned sid) {
	return sid == ((lib >> 8) & 0xFFu) ? route_transcript(lib, 0u) : sid == ((lib >> 16) & 0xFFu) ? route_transcript(lib, 1u) : ROUTE_NO_STRAND;
}
__host__ __device__ inline unsigned route_strand_id(unsigned lib, unsigned t) { return (lib >> (t ? 16 : 8)) & 0xFFu; }

namespace {      // (device code of the unit that includes it: internal linkage, as the kernels that call it)

// The library report of a stranded pass: per lane what its records came to, summed over the wave when the kernel ends, one atomic a
// wave and counter -- reads made with t = plus / minus, records without t, and of the first two those the filter retained.  The
// waves spread their sums over ROUTE_LIB_SLOTS places of 64 bytes behind RouteOut::nb_tot (the host adds the places up): a tile
// kernel runs a workgroup a tile, and that many atomics on five addresses took twelve times the routing itself.
struct LibTally {
	unsigned made0, made1, none, kept0, kept1;
	__device__ inline void init() { made0 = made1 = none = kept0 = kept1 = 0u; }
	__device__ inline void note(const unsigned t, const bool kept) {
		made0 += (unsigned)(t == 0u); made1 += (unsigned)(t == 1u); none += (unsigned)(t >= ROUTE_NO_STRAND);
		kept0 += (unsigned)(t == 0u && kept); kept1 += (unsigned)(t == 1u && kept);
	}
	// (every lane of the wave comes here: the end of the kernel, outside its loops)
	__device__ inline void flush(const RouteOut &O) const {
		unsigned v[5] = {made0, made1, none, kept0, kept1};
#pragma unroll
		for (int q = 0; q < 5; ++q) {
			unsigned x = v[q];
			for (int d = 32; d > 0; d >>= 1) x += (unsigned)__shfl_down((int)x, d);
			const unsigned slot = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (ROUTE_LIB_SLOTS - 1u);
			if ((threadIdx.x & 63u) == 0u && x) atomicAdd(&O.nb_tot[ROUTE_LIB_WORD0 + 8u * slot + q], (unsigned long long)x);
		}
	}
};
// (a helper of a stranded kernel takes the word and the kernel's tally as its pack)
__device__ inline unsigned route_helper_lib() { return 0u; }
__device__ inline unsigned route_helper_lib(unsigned lib, LibTally *) { return lib; }
__device__ inline LibTally *route_tally_arg(unsigned, LibTally *tally) { return tally; }

// The locator entry of base x on a chromosome: where, among the chromosome's covered regions and clusters, the records that
// start inside x's bin lie.  Kept per lane from one look-up to the next: a read's blocks and its first base mostly share a bin.
struct LocProbe {
	int chrom; long long bin;
	unsigned cov_a, cov_b, clu_a, clu_b;       // lower_bound(starts, x) lies in [a, b]
};
__device__ inline void loc_probe(const RouteTables &T, const RouteChrom &R, const int chrom, const int x, LocProbe &P) {
	const long long d = (long long)x - (long long)R.loc_base;
	long long k = d >> T.loc_shift;
	if (R.loc_nb == 0u || d <= 0) k = -1;                       // at or below the first bin's first base: nothing starts left of x
	else if (k >= (long long)R.loc_nb) k = (long long)R.loc_nb; // beyond the last bin: everything does
	if (P.chrom == chrom && P.bin == k) return;
	P.chrom = chrom; P.bin = k;
	if (k < 0) { P.cov_a = P.cov_b = R.cov0; P.clu_a = P.clu_b = R.clu0; }
	else if (k >= (long long)R.loc_nb) { P.cov_a = P.cov_b = R.cov1; P.clu_a = P.clu_b = R.clu1; }
	else {
		uint4 e;                                                  // (8-byte aligned: two entries in one load)
		__builtin_memcpy(&e, T.loc + (R.loc_first + (unsigned)k), 16);
		P.cov_a = e.x; P.clu_a = e.y; P.cov_b = e.z; P.clu_b = e.w;
	}
}

// interval_list::contains_interval against the covered regions of the block's chromosome (interval_list.hpp:396-422):
// lo = lower_bound(starts, start); the interval at lo (when it starts exactly there) or the one before it must reach `end`
__device__ inline bool route_covered(const RouteTables &T, const RouteChrom &R, const int chrom, const int start, const int end, LocProbe &P) {
	if (!(start < end)) return true;
	loc_probe(T, R, chrom, start, P);
	const unsigned a = P.cov_a, b = P.cov_b;
	int2 at, before;                        // the records at lo and at lo - 1
	bool has_at, has_before;
	if (b - a <= 3u) {
		// records a - 1 .. a + 3 hold both, wherever in [a, b] lo falls: five loads in flight at once, no dependent probe
		int2 c[5];
		unsigned below = 0;
#pragma unroll
		for (unsigned q = 0; q < 5; ++q) {
			const unsigned idx = a + q - 1u;
			const bool ok = idx + 1u > R.cov0 && idx < R.cov1 && idx <= b;     // (a - 1 may be R.cov0 - 1, or wrap below zero: both fail here)
			c[q] = ok ? T.cov[idx] : make_int2(0, 0);
			below += (unsigned)(ok && q >= 1u && idx < b && c[q].x < start);
		}
		const unsigned lo = a + below;
		at = make_int2(0, 0); before = make_int2(0, 0);
#pragma unroll
		for (unsigned q = 0; q < 5; ++q) { if (a + q - 1u == lo) at = c[q]; if (a + q == lo) before = c[q]; }
		has_at = lo < R.cov1; has_before = lo > R.cov0;
	} else {
		unsigned lo = a, hi = b;
		while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (T.cov[mid].x < start) lo = mid + 1; else hi = mid; }
		has_at = lo < R.cov1; has_before = lo > R.cov0;
		at = has_at ? T.cov[lo] : make_int2(0, 0);
		before = has_before ? T.cov[lo - 1u] : make_int2(0, 0);
	}
	if (has_at && at.x <= start && end <= at.y) return true;
	if (has_before && before.x <= start && end <= before.y) return true;
	return false;
}

// the cluster record of base p: the last one that starts at or left of p, if p is inside it -- its bucket is p's bucket
// (what the reference's candidate window comes to for a read's first base: count/count.cpp:429-432,463)
__device__ inline bool route_cluster(const RouteTables &T, const RouteChrom &R, const int chrom, const int p, LocProbe &P, int4 &rec) {
	if (p >= 0x7FFFFFFF) return false;
	loc_probe(T, R, chrom, p + 1, P);
	const unsigned a = P.clu_a, b = P.clu_b;       // upper_bound(starts, p) = lower_bound(starts, p + 1) lies in [a, b]
	if (b - a <= 3u) {
		int4 c[4];                                   // records a - 1 .. a + 2: the one before the upper bound is among them
		unsigned below = 0;
#pragma unroll
		for (unsigned q = 0; q < 4; ++q) {
			const unsigned idx = a + q - 1u;
			const bool ok = idx + 1u > R.clu0 && idx < R.clu1 && idx < b;      // (q = 0: a - 1 < b unless it wrapped, which the first test catches)
			c[q] = ok ? T.clu[idx] : make_int4(0, 0, 0, 0);
			below += (unsigned)(ok && q >= 1u && c[q].x <= p);
		}
		const unsigned ub = a + below;
		if (ub == R.clu0) return false;
		rec = make_int4(0, -1, 0, 0);
#pragma unroll
		for (unsigned q = 0; q < 4; ++q) if (a + q == ub) rec = c[q];
		return p <= rec.y;
	}
	unsigned lo = a, hi = b;
	while (lo < hi) { const unsigned mid = (lo + hi) >> 1; if (T.clu[mid].x <= p) lo = mid + 1; else hi = mid; }
	if (lo == R.clu0) return false;
	rec = T.clu[lo - 1u];
	return p <= rec.y;
}

// the chromosome records into a workgroup's LDS when they are few (every workgroup of the routing kernels starts with this)
__device__ inline const RouteChrom *route_stage_chroms(const RouteTables &T, RouteChrom *lds) {
	if (T.n_chrom > ROUTE_CHROM_LDS) return T.chrom;
	for (unsigned q = threadIdx.x; q < 2u * T.n_chrom; q += blockDim.x) reinterpret_cast<uint4 *>(lds)[q] = reinterpret_cast<const uint4 *>(T.chrom)[q];
	__syncthreads();
	return lds;
}

// interval_list::add_interval on a small sorted array (see lsq::IntervalList::add)
__device__ inline bool small_add_interval(int *s, int *e, int &n, int start, int end) {
	if (!(start < end)) return true;
	int ss = 0, se = 0, es = 0, ee = 0;
	for (int i = 0; i < n; ++i) { ss += s[i] < start; se += e[i] < start; es += s[i] < end; ee += e[i] < end; }
	const bool start_inside = (ss - se == 1), end_inside = (es - ee == 1);
	// starts: erase [ss, es), insert `start` at ss unless start_inside; ends: erase [se, ee), insert `end` at se unless end_inside
	const int ns = n - (es - ss) + (start_inside ? 0 : 1);
	if (ns > INGEST_MAX_BLOCKS) return false;
	int ts[INGEST_MAX_BLOCKS], te[INGEST_MAX_BLOCKS];
	int k = 0;
	for (int i = 0; i < ss; ++i) ts[k++] = s[i];
	if (!start_inside) ts[k++] = start;
	for (int i = es; i < n; ++i) ts[k++] = s[i];
	k = 0;
	for (int i = 0; i < se; ++i) te[k++] = e[i];
	if (!end_inside) te[k++] = end;
	for (int i = ee; i < n; ++i) te[k++] = e[i];
	n = ns;
	for (int i = 0; i < n; ++i) { s[i] = ts[i]; e[i] = te[i]; }
	return true;
}

__device__ inline void push3(int &a0, int &a1, int &a2, int &k, const int v) {
	a0 = k == 0 ? v : a0; a1 = k == 1 ? v : a1; a2 = k == 2 ? v : a2;
	++k;
}

// The kept blocks of one read as they come, merged by interval_list's rule.  Nearly every read keeps one or two merged
// blocks: those live in registers (the rule written out for a list of at most two); a third block moves the read to arrays.
// (the arrays are an object of their own: as members they kept the whole accumulator in the private segment -- every field a
// scratch store and load per block, 10 GB of scratch traffic per C3 file -- where now only a read's third block touches it)
struct ReadBig { int bs[INGEST_MAX_BLOCKS], be[INGEST_MAX_BLOCKS]; };
struct ReadAcc {
	int s0, e0, s1, e1;
	int n;                          // merged blocks
	int chrom;
	unsigned strand;
	bool any, ok, big;
	__device__ inline void init() { s0 = e0 = s1 = e1 = 0; n = 0; chrom = -1; strand = 0; any = false; ok = true; big = false; }
	// a block that passed the containment filter (count/count.cpp:319-323)
	__device__ inline void add(ReadBig &B, const unsigned c, const unsigned sid, const int start, const int end) {
		any = true; chrom = (int)c; strand = sid;
		if (!(start < end)) return;
		if (big) { ok = small_add_interval(B.bs, B.be, n, start, end) && ok; return; }
		if (n == 0) { s0 = start; e0 = end; n = 1; return; }
		const bool h0 = n > 0, h1 = n > 1;
		const int ss = (int)(h0 && s0 < start) + (int)(h1 && s1 < start), se = (int)(h0 && e0 < start) + (int)(h1 && e1 < start);
		const int es = (int)(h0 && s0 < end) + (int)(h1 && s1 < end), ee = (int)(h0 && e0 < end) + (int)(h1 && e1 < end);
		const bool start_inside = (ss - se == 1), end_inside = (es - ee == 1);
		int a0 = 0, a1 = 0, a2 = 0, ka = 0, b0 = 0, b1 = 0, b2 = 0, kb = 0;
		if (h0 && 0 < ss) push3(a0, a1, a2, ka, s0);
		if (h1 && 1 < ss) push3(a0, a1, a2, ka, s1);
		if (!start_inside) push3(a0, a1, a2, ka, start);
		if (h0 && 0 >= es) push3(a0, a1, a2, ka, s0);
		if (h1 && 1 >= es) push3(a0, a1, a2, ka, s1);
		if (h0 && 0 < se) push3(b0, b1, b2, kb, e0);
		if (h1 && 1 < se) push3(b0, b1, b2, kb, e1);
		if (!end_inside) push3(b0, b1, b2, kb, end);
		if (h0 && 0 >= ee) push3(b0, b1, b2, kb, e0);
		if (h1 && 1 >= ee) push3(b0, b1, b2, kb, e1);
		if (ka <= 2) { s0 = a0; s1 = a1; e0 = b0; e1 = b1; n = ka; }
		else { B.bs[0] = a0; B.bs[1] = a1; B.bs[2] = a2; B.be[0] = b0; B.be[1] = b1; B.be[2] = b2; n = 3; big = true; }
	}
	__device__ inline bool kept() const { return any && n > 0; }          // (finish gives such a read a key other than ROUTE_KEY_DROPPED)
	// the read is complete: its key and blocks to their place (index i of the pass)
	__device__ inline void finish(const ReadBig &B, const RouteTables &T, const RouteChrom *chroms, LocProbe &P, const RouteOut &O, const unsigned i) {
		unsigned key = ROUTE_KEY_DROPPED;
		int4 rec = make_int4(0, 0, 0, 0);
		if (any && n > 0) {
			long long tot = 0;
			if (big) {
				s0 = B.bs[0]; e0 = B.be[0];
				if (n > 1) { s1 = B.bs[1]; e1 = B.be[1]; }
				for (int q = 0; q < n; ++q) tot += B.be[q] - B.bs[q];
			} else tot = (long long)(e0 - s0) + (n > 1 ? (long long)(e1 - s1) : 0ll);
			if (!ok || tot >= (1 << 18)) atomicMax(&O.nb_tot[2], 1ull);
			key = route_key_unrouted((unsigned)n);
			rec = make_int4(s0, e0, n > 1 ? s1 : 0, n > 1 ? e1 : 0);
			const RouteChrom R = chroms[chrom];
			// the bucket of the first merged base, if that base lies in the span of some planned event (a cluster): otherwise the
			// read is a candidate of none of them (count/count.cpp:429-432,463) -- with a shard, the other shards' reads
			int4 cl;
			if (route_cluster(T, R, chrom, s0, P, cl)) {
				const unsigned b = (unsigned)cl.z;
				const int lo = cl.w;
				unsigned pool = n == 1 ? 0u : (n == 2 ? 1u : 2u);
				if (pool < 2u && O.compact) {
					bool fits = lsq::compact_block_fits((long long)s0 - lo + lsq::COMPACT_BIAS, (long long)e0 - s0);
					if (n == 2) fits = fits && lsq::compact_block_fits((long long)s1 - e0, (long long)e1 - s1);
					if (!fits) pool = 3u;
				}
				key = route_key(b, pool, strand);
				if (pool >= 2u) {
					const unsigned long long idx = atomicAdd(&O.nb_tot[0], 1ull), boff = atomicAdd(&O.nb_tot[1], (unsigned long long)n);
					atomicAdd(&O.cntn[b], 1u); atomicAdd(&O.cntnb[b], (unsigned)n);
					if (idx < O.nb_cap && boff + (unsigned)n <= O.nbb_cap) {
						O.nb_ent[idx] = make_uint4(i, b, (unsigned)n | (strand << 8), (unsigned)boff);
						if (big) { for (int q = 0; q < n; ++q) O.nb_blk[boff + q] = make_int2(B.bs[q], B.be[q]); }
						else { O.nb_blk[boff] = make_int2(s0, e0); if (n > 1) O.nb_blk[boff + 1] = make_int2(s1, e1); }
					}
				}
			}
		}
		O.key[i] = key;
		O.rec[i] = rec;
	}
};

} // namespace
