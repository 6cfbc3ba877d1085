// The splice junctions of a parsed read file on the device (include/lesseq_hip.h, lsq_jn_device): five phases over
// device arrays -- extract (a lane a read: count, prefix sum, emit a record per occurrence), sort (lsq_sort.hpp: stable LSD radix
// sort by chromosome, start, end), reduce (run heads, then sums and maxima per run), annotate (a lane a distinct junction: binary
// search in the index's introns), copy-back (the distinct rows alone).  Every number is an integer and no result depends on the
// order in which lanes arrive: sums and maxima only.
#include "lsq_wave.hpp"
#include "lsq_scan.hpp"
#include "lsq_sort.hpp"
#include "lsq_junc.hpp"

namespace {

// A record: w0 = jn_key(start, end); w1 = chromosome index << 32 | payload (overhang, JN_PLUS, JN_MINUS)
struct JnAcc { unsigned long long dropped, nochrom, any0, any1, all0, all1; };

// A lane a read, a fixed number of workgroups striding over the reads.  EMIT false: the read's occurrences counted (cnt), the
// pairs that make none for the report.  EMIT true: the records written at the read's place (off), the OR and the AND of all of
// them kept for the sort's choice of digits.  The tallies are kept per lane over the stride, summed over the workgroup once, and
// added to `acc` by one lane: a few thousand atomics a launch (one a wave of reads was 6e6 on four addresses, and most of the pass).
template <bool EMIT>
__global__ void __launch_bounds__(256) lsq_jn_extract_kernel(ParsedReads R, unsigned min_overhang, unsigned *cnt, const unsigned long long *off,
                                                             unsigned long long *w0, unsigned long long *w1, JnAcc *acc) {
	__shared__ unsigned long long part[4][4];
	unsigned long long dropped = 0, nochrom = 0, any0 = 0, any1 = 0, all0 = ~0ull, all1 = ~0ull;
	for (unsigned long long r = (unsigned long long)blockIdx.x * 256u + threadIdx.x; r < R.n_reads; r += (unsigned long long)gridDim.x * 256u) {
		const unsigned long long b0 = R.blk_off[r], b1 = R.blk_off[r + 1];
		unsigned long long at = EMIT ? off[r] : 0ull;
		unsigned m = 0;
		if (b1 > b0 + 1) {
			int s0 = R.bs[b0], e0 = R.be[b0];
			unsigned c0 = R.bc[b0], st0 = R.bst[b0];
			for (unsigned long long k = b0 + 1; k < b1; ++k) {
				const int s1 = R.bs[k], e1 = R.be[k];
				const unsigned c1 = R.bc[k], st1 = R.bst[k];
				if (c0 == NO_CHROM || c1 == NO_CHROM) ++nochrom;
				else if (c0 == c1 && s1 > e0) {
					const long long ov = min((long long)e0 - s0, (long long)e1 - s1);
					if (ov < (long long)min_overhang) ++dropped;
					else {
						if (EMIT) {
							const unsigned long long a = jn_key(e0, s1);
							const unsigned long long b = ((unsigned long long)c0 << 32) | ((unsigned)ov & JN_OV_MASK) | (st0 == 0u ? JN_PLUS : 0u) | (st0 == 1u ? JN_MINUS : 0u);
							w0[at] = a; w1[at] = b; ++at;
							any0 |= a; any1 |= b; all0 &= a; all1 &= b;
						}
						++m;
					}
				}
				s0 = s1; e0 = e1; c0 = c1; st0 = st1;
			}
		}
		if (!EMIT) cnt[r] = m;
	}
	unsigned long long v[4] = {EMIT ? any0 : dropped, EMIT ? any1 : nochrom, EMIT ? ~all0 : 0ull, EMIT ? ~all1 : 0ull};      // (the ANDs as the OR of the complements)
	workgroup_tally<EMIT>(v, part);
	if (threadIdx.x == 0) {
		if (EMIT) {
			if (v[0]) atomicOr(&acc->any0, v[0]);
			if (v[1]) atomicOr(&acc->any1, v[1]);
			if (v[2]) atomicAnd(&acc->all0, ~v[2]);
			if (v[3]) atomicAnd(&acc->all1, ~v[3]);
		} else {
			if (v[0]) atomicAdd(&acc->dropped, v[0]);
			if (v[1]) atomicAdd(&acc->nochrom, v[1]);
		}
	}
}

__device__ inline bool jn_same(unsigned long long a0, unsigned long long a1, unsigned long long b0, unsigned long long b1) { return a0 == b0 && (a1 >> 32) == (b1 >> 32); }

// sorted records -> 1 where a run begins
__global__ void __launch_bounds__(256) lsq_jn_heads_kernel(const unsigned long long *w0, const unsigned long long *w1, unsigned long long n, unsigned *head) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i < n) head[i] = (i == 0 || !jn_same(w0[i], w1[i], w0[i - 1], w1[i - 1])) ? 1u : 0u;
}

// A lane a sorted record; rid[i] = run heads ahead of i.  A wave sums the strand flags and takes the largest overhang over each
// stretch of one run it holds (a segmented scan through shuffles); the last lane of a stretch adds them to the run's row: an
// atomic a stretch -- at most one a run and wave -- not one an occurrence.  The head's lane notes where the run begins.
__global__ void __launch_bounds__(256) lsq_jn_reduce_kernel(const unsigned long long *w1, const unsigned *head, const unsigned long long *rid, unsigned long long n,
                                                            unsigned *first, unsigned *plus, unsigned *minus, unsigned *max_ov) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	const unsigned lane = threadIdx.x & 63u;
	const bool ok = i < n;
	const unsigned h = ok ? head[i] : 1u;
	const unsigned run = ok ? (unsigned)(rid[i] + h - 1ull) : 0u;
	const unsigned p = ok ? (unsigned)w1[i] : 0u;
	unsigned np = (p & JN_PLUS) ? 1u : 0u, nm = (p & JN_MINUS) ? 1u : 0u, ov = p & JN_OV_MASK;
	const unsigned long long starts = __ballot(h != 0u || lane == 0u);
	const unsigned s = 63u - (unsigned)__clzll(starts & ((2ull << lane) - 1ull));       // the lane my stretch begins on
#pragma unroll
	for (unsigned d = 1; d < 64; d <<= 1) {
		const unsigned tp = __shfl_up(np, d), tm = __shfl_up(nm, d), to = __shfl_up(ov, d);
		if (lane >= s + d) { np += tp; nm += tm; ov = max(ov, to); }
	}
	const bool last = lane == 63u || ((starts >> (lane + 1u)) & 1ull);
	if (ok && h) first[run] = (unsigned)i;
	if (ok && last) {
		if (np) atomicAdd(&plus[run], np);
		if (nm) atomicAdd(&minus[run], nm);
		atomicMax(&max_ov[run], ov);
	}
}

// A lane a distinct junction: its row from the run's first record, its reads from where the next run begins, its `ann` from a
// binary search in the index's introns (ascending in chromosome, key)
struct JnIntrons { const unsigned *chrom; const unsigned long long *key; const unsigned char *ann; unsigned n; };
struct JnRows { unsigned *chrom; int *start, *end; unsigned char *ann; unsigned *reads; };
__global__ void __launch_bounds__(256) lsq_jn_annotate_kernel(const unsigned long long *w0, const unsigned long long *w1, unsigned long long n, const unsigned *first, unsigned n_rows,
                                                              JnIntrons I, JnRows O) {
	const unsigned r = blockIdx.x * 256u + threadIdx.x;
	if (r >= n_rows) return;
	const unsigned i0 = first[r];
	const unsigned long long i1 = r + 1u < n_rows ? (unsigned long long)first[r + 1u] : n;
	const unsigned long long key = w0[i0];
	const unsigned chrom = (unsigned)(w1[i0] >> 32);
	unsigned lo = 0, hi = I.n;
	while (lo < hi) {
		const unsigned mid = lo + ((hi - lo) >> 1);
		const unsigned mc = I.chrom[mid];
		if (mc < chrom || (mc == chrom && I.key[mid] < key)) lo = mid + 1u; else hi = mid;
	}
	O.chrom[r] = chrom; O.start[r] = jn_key_start(key); O.end[r] = jn_key_end(key);
	O.ann[r] = (lo < I.n && I.chrom[lo] == chrom && I.key[lo] == key) ? I.ann[lo] : (unsigned char)'.';
	O.reads[r] = (unsigned)(i1 - i0);
}

} // namespace

int lsq::jn_device_reads(lsq_ctx *c, const lsq_jn_index &ix, const ParsedReads &R, uint32_t min_overhang, lsq_jn_table &t) {
	hipStream_t st = c->stream;
	int rc;
	PhaseClock<JN_PHASES> PC;
	if ((rc = PC.make())) return rc;
	if (R.n_reads > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32 reads");
	t.resize(0);
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks; t.report[2] = t.report[3] = t.report[4] = 0;
	for (float &m : t.ms) m = 0;
	if (!R.n_reads) return LSQ_OK;

	// ---- extract
	HIP_TRY(PC.mark(0, st));
	DevBuf<unsigned> d_cnt;
	DevBuf<unsigned long long> d_off;
	DevBuf<JnAcc> d_acc;
	ScanScratch SS;
	const JnAcc acc0{0, 0, 0, 0, ~0ull, ~0ull};
	JnAcc acc = acc0;
	unsigned long long n_occ = 0;
	const unsigned grid = stride_grid(c, "LSQ_JN_EXTRACT_GRID", R.n_reads);
	if ((rc = d_cnt.alloc((size_t)R.n_reads)) || (rc = d_off.alloc((size_t)R.n_reads + 1)) || (rc = d_acc.upload(&acc0, 1, st)) || (rc = SS.reserve(R.n_reads))) return rc;
	hipLaunchKernelGGL((lsq_jn_extract_kernel<false>), dim3(grid), dim3(256), 0, st, R, min_overhang, d_cnt.p, (const unsigned long long *)nullptr,
	                   (unsigned long long *)nullptr, (unsigned long long *)nullptr, d_acc.p);
	HIP_TRY(hipGetLastError());
	if ((rc = device_scan<1, false>(SS, d_cnt.p, R.n_reads, d_off.p, st))) return rc;
	HIP_TRY(hipMemcpyAsync(&n_occ, d_off.p + R.n_reads, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (n_occ > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32-1 junction occurrences");
	SortBuf B;                                  // (allocations follow the counted occurrences)
	if ((rc = B.reserve(n_occ))) return rc;
	if (n_occ) {
		hipLaunchKernelGGL((lsq_jn_extract_kernel<true>), dim3(grid), dim3(256), 0, st, R, min_overhang, (unsigned *)nullptr, (const unsigned long long *)d_off.p,
		                   B.w0[0].p, B.w1[0].p, d_acc.p);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMemcpyAsync(&acc, d_acc.p, sizeof(acc), hipMemcpyDeviceToHost, st));
	HIP_TRY(PC.mark(1, st));
	HIP_TRY(hipStreamSynchronize(st));
	d_cnt.alloc(0); d_off.alloc(0);
	t.report[2] = n_occ; t.report[3] = acc.dropped; t.report[4] = acc.nochrom;

	// ---- sort: the digits of start and end, then the chromosome's; those on which every record agrees are left out
	unsigned n_rows = 0;
	DevBuf<unsigned> d_head, d_first, d_plus, d_minus, d_maxov, d_chrom, d_reads, d_ichrom;
	DevBuf<unsigned long long> d_rid, d_ikey;
	DevBuf<int> d_start, d_end;
	DevBuf<unsigned char> d_ann, d_iann;
	if (n_occ) {
		static const unsigned ALL_DIGITS[10] = {0, 8, 16, 24, 32, 40, 48, 56, 64 + 32, 64 + 40};
		unsigned digits[10];
		const unsigned long long any[2] = {acc.any0, acc.any1}, all[2] = {acc.all0, acc.all1};
		const unsigned n_digits = sort_digits(any, all, ALL_DIGITS, 10, digits);
		if ((rc = device_radix_sort(B, digits, n_digits, st))) return rc;
		HIP_TRY(PC.mark(2, st));

		// ---- reduce
		const unsigned long long *w0 = B.w0[B.cur].p, *w1 = B.w1[B.cur].p;
		unsigned long long n_heads = 0;
		if ((rc = d_head.alloc((size_t)n_occ)) || (rc = d_rid.alloc((size_t)n_occ + 1)) || (rc = SS.reserve(n_occ))) return rc;
		hipLaunchKernelGGL(lsq_jn_heads_kernel, dim3(grid_for(n_occ, 256)), dim3(256), 0, st, w0, w1, n_occ, d_head.p);
		HIP_TRY(hipGetLastError());
		if ((rc = device_scan<1, true>(SS, d_head.p, n_occ, d_rid.p, st))) return rc;
		HIP_TRY(hipMemcpyAsync(&n_heads, d_rid.p + n_occ, 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		n_rows = (unsigned)n_heads;
		if ((rc = d_first.alloc(n_rows)) || (rc = d_plus.alloc(n_rows)) || (rc = d_minus.alloc(n_rows)) || (rc = d_maxov.alloc(n_rows))) return rc;
		HIP_TRY(hipMemsetAsync(d_plus.p, 0, (size_t)n_rows * 4, st));
		HIP_TRY(hipMemsetAsync(d_minus.p, 0, (size_t)n_rows * 4, st));
		HIP_TRY(hipMemsetAsync(d_maxov.p, 0, (size_t)n_rows * 4, st));
		hipLaunchKernelGGL(lsq_jn_reduce_kernel, dim3(grid_for(n_occ, 256)), dim3(256), 0, st, w1, (const unsigned *)d_head.p, (const unsigned long long *)d_rid.p, n_occ,
		                   d_first.p, d_plus.p, d_minus.p, d_maxov.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(PC.mark(3, st));

		// ---- annotate
		const size_t ni = ix.in_key.size();
		if ((rc = d_ichrom.upload(ix.in_chrom.data(), ni, st)) || (rc = d_ikey.upload((const unsigned long long *)ix.in_key.data(), ni, st)) || (rc = d_iann.upload(ix.in_ann.data(), ni, st)) ||
		    (rc = d_chrom.alloc(n_rows)) || (rc = d_start.alloc(n_rows)) || (rc = d_end.alloc(n_rows)) || (rc = d_ann.alloc(n_rows)) || (rc = d_reads.alloc(n_rows))) return rc;
		const JnIntrons I{d_ichrom.p, d_ikey.p, d_iann.p, (unsigned)ni};
		const JnRows O{d_chrom.p, d_start.p, d_end.p, d_ann.p, d_reads.p};
		hipLaunchKernelGGL(lsq_jn_annotate_kernel, dim3(grid_for(n_rows, 256)), dim3(256), 0, st, w0, w1, n_occ, (const unsigned *)d_first.p, n_rows, I, O);
		HIP_TRY(hipGetLastError());
		HIP_TRY(PC.mark(4, st));

		// ---- copy-back: the distinct rows
		t.resize(n_rows);
		HIP_TRY(hipMemcpyAsync(t.chrom.data(), d_chrom.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.start.data(), d_start.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.end.data(), d_end.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.ann.data(), d_ann.p, (size_t)n_rows, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.reads.data(), d_reads.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.plus.data(), d_plus.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.minus.data(), d_minus.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.max_overhang.data(), d_maxov.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(PC.mark(5, st));
		HIP_TRY(hipStreamSynchronize(st));
		for (int k = 1; k < JN_PHASES; ++k) (void)PC.ms(k, &t.ms[k]);
	}
	(void)PC.ms(0, &t.ms[0]);
	return LSQ_OK;
}

// the records a workgroup of the sort takes (tests place their cases around it)
extern "C" int lsq_jn_sort_tile(void) { return (int)SORT_TILE; }
