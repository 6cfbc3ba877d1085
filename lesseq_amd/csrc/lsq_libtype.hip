// Which library type is this read file, on the device (include/lesseq_hip.h, lsq_lt_device): three phases over device
// arrays -- index upload, count (a lane a read: r from the strand id of its first block, every block a binary search in each of
// the two exon unions of its chromosome, a strand no longer once it has hit; nine tallies a lane in registers), copy-back (the
// nine counters).  Every number is an integer and sums commute: no result depends on the order in which lanes arrive.
#include "lsq_wave.hpp"
#include "lsq_libtype.hpp"

namespace {

struct LtIndex {
	const unsigned *tab_first;                           // 2 * n_chroms + 1
	const int *iv_start, *iv_end;                        // n_intervals = tab_first[2 * n_chroms]
	unsigned n_chroms;
};

// Whether [s, e) shares a base with table tb's union.  tb < 2 * n_chroms: tab_first[tb] and [tb + 1] are entries of its
// 2 * n_chroms + 1, they ascend and end at n_intervals, so lo <= mid < hi <= n_intervals, and the last load is guarded by lo < end
__device__ inline bool lt_meets(const LtIndex &I, unsigned tb, int s, int e) {
	unsigned lo = I.tab_first[tb], hi = I.tab_first[tb + 1u];
	const unsigned end = hi;
	while (lo < hi) {
		const unsigned mid = lo + ((hi - lo) >> 1);
		if (I.iv_end[mid] <= s) lo = mid + 1u; else hi = mid;
	}
	return lo < end && I.iv_start[lo] < e;
}

// A lane a read, a fixed number of workgroups striding over the reads.  No LDS counters and no per-lane list: the class of a read
// is one of nine, kept as nine sums a lane over the stride, summed over the workgroup once (three tallies of four words) and added
// by one lane, one 64-bit atomic a workgroup and counter that is not zero.  `lib`: route_lib_word of a forward library -- t is r.
__global__ void __launch_bounds__(256) lsq_lt_count_kernel(ParsedReads R, LtIndex I, unsigned lib, unsigned long long *cls) {
	__shared__ unsigned long long part_a[4][4], part_b[4][4], part_c[4][4];
	unsigned long long n[LT_CLASSES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
	for (unsigned long long r = (unsigned long long)blockIdx.x * 256u + threadIdx.x; r < R.n_reads; r += stride) {
		// r < n_reads: blk_off[r] and [r + 1] are entries of its n_reads + 1; they ascend and end at n_blocks
		const unsigned long long b0 = R.blk_off[r], b1 = R.blk_off[r + 1];
		const unsigned t = b0 < b1 ? route_transcript_of_id(lib, R.bst[b0]) : ROUTE_NO_STRAND;
		bool plus = false, minus = false;
		for (unsigned long long b = b0; t < ROUTE_NO_STRAND && b < b1 && !(plus && minus); ++b) {
			const unsigned c = R.bc[b];
			const int s = R.bs[b], e = R.be[b];
			if (c == NO_CHROM || c >= I.n_chroms || e <= s) continue;      // no table is read for such a block
			if (!plus) plus = lt_meets(I, 2u * c, s, e);
			if (!minus) minus = lt_meets(I, 2u * c + 1u, s, e);
		}
		const unsigned k = lt_class(t, plus, minus);
#pragma unroll
		for (unsigned q = 0; q < (unsigned)LT_CLASSES; ++q) n[q] += (unsigned)(k == q);
	}
	unsigned long long u[4] = {n[0], n[1], n[2], n[3]}, v[4] = {n[4], n[5], n[6], n[7]}, w[4] = {n[8], 0ull, 0ull, 0ull};
	workgroup_tally<false>(u, part_a);
	workgroup_tally<false>(v, part_b);
	workgroup_tally<false>(w, part_c);
	if (threadIdx.x == 0) {
#pragma unroll
		for (unsigned q = 0; q < 4; ++q) {
			if (u[q]) atomicAdd(&cls[q], u[q]);
			if (v[q]) atomicAdd(&cls[4u + q], v[q]);
		}
		if (w[0]) atomicAdd(&cls[8], w[0]);
	}
}

} // namespace

int lsq::lt_device_reads(lsq_ctx *c, const lsq_lt_index &ix, const ParsedReads &R, lsq_lt_table &t) {
	hipStream_t st = c->stream;
	int rc;
	PhaseClock<LT_PHASES> PC;
	if ((rc = PC.make())) return rc;
	t = lsq_lt_table();
	t.reads = R.n_reads; t.unplaced_genes = ix.unplaced_genes;
	const size_t n_tab = ix.E.covered.size(), ni = ix.iv_start.size();

	// ---- index upload
	HIP_TRY(PC.mark(0, st));
	DevBuf<unsigned> d_tf;
	DevBuf<int> d_is, d_ie;
	DevBuf<unsigned long long> d_cls;
	if ((rc = d_tf.upload(ix.tab_first.data(), n_tab + 1, st)) || (rc = d_is.upload(ix.iv_start.data(), ni, st)) || (rc = d_ie.upload(ix.iv_end.data(), ni, st)) ||
	    (rc = d_cls.alloc(LT_CLASSES))) return rc;
	HIP_TRY(hipMemsetAsync(d_cls.p, 0, LT_CLASSES * 8, st));

	// ---- count
	HIP_TRY(PC.mark(1, st));
	if (R.n_reads) {
		const LtIndex I{d_tf.p, d_is.p, d_ie.p, (unsigned)ix.E.n_table_chroms()};
		hipLaunchKernelGGL(lsq_lt_count_kernel, dim3(stride_grid(c, "LSQ_LT_GRID", R.n_reads)), dim3(256), 0, st, R, I,
		                   route_lib_word(false, (unsigned)ix.E.strand_plus, (unsigned)ix.E.strand_minus), d_cls.p);
		HIP_TRY(hipGetLastError());
	}

	// ---- copy-back
	HIP_TRY(PC.mark(2, st));
	HIP_TRY(hipMemcpyAsync(t.cls, d_cls.p, LT_CLASSES * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(PC.mark(3, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (int k = 0; k < LT_PHASES; ++k) (void)PC.ms(k, &t.ms[k]);
	return LSQ_OK;
}
