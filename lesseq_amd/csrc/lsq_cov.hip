// The per-base depth of a parsed read file on the device (include/lesseq_hip.h, lsq_cov_device): six phases over
// device arrays -- extract (a lane a read: count, prefix sum, two records per counted block: where it begins and where it ends),
// sort (lsq_sort.hpp: stable LSD radix sort by chromosome and position), reduce and scan (the depth behind every run of equal
// positions from one prefix sum of the "begins" flags; the stretches of positive depth between neighbouring runs compacted), emit
// (neighbouring stretches of one depth joined into rows by a second compaction), regions (a lane an exon-union interval: two binary
// searches in the rows, sums from cumulative 64-bit arrays), copy-back.  Every number is an integer and no result depends on the
// order in which lanes arrive: sums only.
#include "lsq_wave.hpp"
#include "lsq_scan.hpp"
#include "lsq_sort.hpp"
#include "lsq_cov_dev.hpp"

namespace {

// A record: w0 = position + 2^30; w1 = chromosome index << 32 | COV_START where a block begins
struct CovAcc { unsigned long long nochrom, empty, other, bases, any0, any1, all0, all1; };

// A lane a read, a fixed number of workgroups striding over the reads.  EMIT false: the read's counted blocks (cnt), the blocks
// that are not counted and the counted bases for the report.  EMIT true: two records per counted block written at the read's place
// (off counts blocks), the OR and the AND of all of them kept for the sort's choice of digits.  The tallies are kept per lane over
// the stride, summed over the workgroup once, and added to `acc` by one lane (lsq_junc.hip's extract: what an atomic a wave costs).
// strand_id: the strand a counted block must carry (0 "+", 1 "-"), or a value no block carries the other way round: 0xFFFFFFFF = any.
template <bool EMIT>
__global__ void __launch_bounds__(256) lsq_cov_extract_kernel(ParsedReads R, unsigned strand_id, unsigned *cnt, const unsigned long long *off,
                                                              unsigned long long *w0, unsigned long long *w1, CovAcc *acc) {
	__shared__ unsigned long long part[4][4];
	unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0;          // EMIT: any0, any1, ~all0, ~all1; else nochrom, empty, other, bases
	for (unsigned long long r = (unsigned long long)blockIdx.x * 256u + threadIdx.x; r < R.n_reads; r += (unsigned long long)gridDim.x * 256u) {
		const unsigned long long b0 = R.blk_off[r], b1 = R.blk_off[r + 1];
		unsigned long long at = EMIT ? 2ull * off[r] : 0ull;
		unsigned m = 0;
		for (unsigned long long k = b0; k < b1; ++k) {
			const int s = R.bs[k], e = R.be[k];
			const unsigned ch = R.bc[k];
			if (ch == NO_CHROM) { if (!EMIT) ++t0; continue; }
			if (e <= s) { if (!EMIT) ++t1; continue; }
			if (strand_id != 0xFFFFFFFFu && (unsigned)R.bst[k] != strand_id) { if (!EMIT) ++t2; continue; }
			if (EMIT) {
				const unsigned long long a0 = (unsigned long long)((long long)s + COV_BIAS), a1 = (unsigned long long)((long long)e + COV_BIAS);
				const unsigned long long hi = (unsigned long long)ch << 32;
				w0[at] = a0; w1[at] = hi | COV_START; w0[at + 1] = a1; w1[at + 1] = hi; at += 2;
				t0 |= a0 | a1; t1 |= hi | COV_START; t2 |= ~a0 | ~a1; t3 |= ~hi;
			} else t3 += (unsigned long long)((long long)e - s);
			++m;
		}
		if (!EMIT) cnt[r] = m;
	}
	unsigned long long v[4] = {t0, t1, t2, t3};
	workgroup_tally<EMIT>(v, part);
	if (threadIdx.x == 0) {
		if (EMIT) {
			if (v[0]) atomicOr(&acc->any0, v[0]);
			if (v[1]) atomicOr(&acc->any1, v[1]);
			if (v[2]) atomicAnd(&acc->all0, ~v[2]);
			if (v[3]) atomicAnd(&acc->all1, ~v[3]);
		} else {
			if (v[0]) atomicAdd(&acc->nochrom, v[0]);
			if (v[1]) atomicAdd(&acc->empty, v[1]);
			if (v[2]) atomicAdd(&acc->other, v[2]);
			if (v[3]) atomicAdd(&acc->bases, v[3]);
		}
	}
}

// sorted records -> 1 where a block begins
__global__ void __launch_bounds__(256) lsq_cov_begins_kernel(const unsigned long long *w1, unsigned long long n, unsigned *flag) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i < n) flag[i] = (unsigned)(w1[i] & COV_START);
}

// The depth behind the run that ends at record i - 1, S[i] of the first i records beginning a block: 2 S[i] - i (the others end one).
// A piece is the stretch between two neighbouring runs with a depth above 0: it is noted at the head i of the later run.  A block
// begins and ends on one chromosome, so the depth behind a chromosome's last run is 0 and a piece never spans two chromosomes.
__device__ inline unsigned cov_piece_depth(const unsigned long long *w0, const unsigned long long *w1, const unsigned long long *S, unsigned long long i) {
	if (i == 0 || (w0[i] == w0[i - 1] && (w1[i] >> 32) == (w1[i - 1] >> 32))) return 0u;
	return (unsigned)(2ull * S[i] - i);
}
__global__ void __launch_bounds__(256) lsq_cov_piece_flags_kernel(const unsigned long long *w0, const unsigned long long *w1, const unsigned long long *S, unsigned long long n, unsigned *flag) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i < n) flag[i] = cov_piece_depth(w0, w1, S, i) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) lsq_cov_pieces_kernel(const unsigned long long *w0, const unsigned long long *w1, const unsigned long long *S, unsigned long long n,
                                                             const unsigned *flag, const unsigned long long *at, CovPieces P) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i >= n || !flag[i]) return;
	const unsigned long long k = at[i];                          // < the pieces counted: the flags' own prefix sum
	P.chrom[k] = (unsigned)(w1[i] >> 32);
	P.start[k] = (int)((long long)w0[i - 1] - COV_BIAS);
	P.end[k] = (int)((long long)w0[i] - COV_BIAS);
	P.depth[k] = cov_piece_depth(w0, w1, S, i);
}

// pieces ascend in (chromosome, start): 1 where a row begins -- the piece before it lies elsewhere, does not abut or has another depth
__global__ void __launch_bounds__(256) lsq_cov_row_heads_kernel(CovPieces P, unsigned long long n, unsigned *head) {
	const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (k < n) head[k] = (k == 0 || P.chrom[k] != P.chrom[k - 1] || P.start[k] != P.end[k - 1] || P.depth[k] != P.depth[k - 1]) ? 1u : 0u;
}
// rid[k] = row heads ahead of k.  A row's first piece gives its chromosome, start and depth, its last piece its end
__global__ void __launch_bounds__(256) lsq_cov_rows_kernel(CovPieces P, unsigned long long n, const unsigned *head, const unsigned long long *rid, CovPieces O) {
	const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (k >= n) return;
	const unsigned h = head[k];
	const unsigned long long row = rid[k] + h - 1ull;            // (head[0] = 1: never below 0; < the heads counted)
	if (h) { O.chrom[row] = P.chrom[k]; O.start[row] = P.start[k]; O.depth[row] = P.depth[k]; }
	if (k + 1 == n || head[k + 1]) O.end[row] = P.end[k];
}

// per row its bases with depth >= min_depth, and bases times depth: what the regions' cumulative arrays are the prefix sums of
__global__ void __launch_bounds__(256) lsq_cov_row_weights_kernel(CovPieces O, unsigned n_rows, unsigned min_depth, unsigned long long *wc, unsigned long long *ws) {
	const unsigned r = blockIdx.x * 256u + threadIdx.x;
	if (r >= n_rows) return;
	const unsigned long long len = (unsigned long long)((long long)O.end[r] - O.start[r]);
	wc[r] = O.depth[r] >= min_depth ? len : 0ull;
	ws[r] = len * O.depth[r];
}

// A lane an interval of a line's exon union (coordinates clipped to +-2^30, beyond which there is no depth): the rows it overlaps
// by two binary searches -- rows ascend in (chromosome, start) and do not overlap, so they ascend in (chromosome, end) too -- their
// sums from the cumulative arrays, the parts of the first and the last row that lie outside the interval taken off again.  Integer
// atomics add the interval's sums to its line's: the order of arrival does not matter.
struct CovIntervals { const unsigned *chrom; const int *start, *end; const unsigned *line; unsigned n; };
__global__ void __launch_bounds__(256) lsq_cov_regions_kernel(CovIntervals I, CovPieces O, unsigned n_rows, unsigned min_depth, const unsigned long long *cum_c, const unsigned long long *cum_s,
                                                              unsigned long long *covered, unsigned long long *depth_sum) {
	const unsigned q = blockIdx.x * 256u + threadIdx.x;
	if (q >= I.n) return;
	const unsigned c = I.chrom[q];
	const int s = I.start[q], e = I.end[q];
	unsigned lo = 0, hi = n_rows;
	while (lo < hi) {                                            // the first row that ends behind s
		const unsigned mid = lo + ((hi - lo) >> 1);
		const unsigned mc = O.chrom[mid];
		if (mc < c || (mc == c && O.end[mid] <= s)) lo = mid + 1u; else hi = mid;
	}
	const unsigned first = lo;
	hi = n_rows;
	while (lo < hi) {                                            // the first row that begins at or behind e
		const unsigned mid = lo + ((hi - lo) >> 1);
		const unsigned mc = O.chrom[mid];
		if (mc < c || (mc == c && O.start[mid] < e)) lo = mid + 1u; else hi = mid;
	}
	const unsigned end = lo;
	if (first >= end) return;
	unsigned long long cov = cum_c[end] - cum_c[first], sum = cum_s[end] - cum_s[first];
	if (O.start[first] < s) {
		const unsigned long long cut = (unsigned long long)((long long)s - O.start[first]);
		const unsigned d = O.depth[first];
		if (d >= min_depth) cov -= cut;
		sum -= cut * d;
	}
	if (O.end[end - 1u] > e) {
		const unsigned long long cut = (unsigned long long)((long long)O.end[end - 1u] - e);
		const unsigned d = O.depth[end - 1u];
		if (d >= min_depth) cov -= cut;
		sum -= cut * d;
	}
	const unsigned line = I.line[q];
	if (cov) atomicAdd(&covered[line], cov);
	if (sum) atomicAdd(&depth_sum[line], sum);
}

} // namespace

// extract, sort, reduce and scan, emit: the rows left on the device (lsq_cov_dev.hpp), for the regions and the copy-back below and
// for lsq_retention.hip's selection
int lsq::cov_device_rows(lsq_ctx *c, const ParsedReads &R, int strand, PhaseClock<COV_PHASES> &PC, DevPieces &rows, unsigned &n_rows, uint64_t *report) {
	hipStream_t st = c->stream;
	int rc;
	n_rows = 0;
	for (int k = 0; k < COV_REPORT; ++k) report[k] = 0;
	report[0] = R.n_reads; report[1] = R.n_blocks;
	const unsigned strand_id = strand == '+' ? 0u : strand == '-' ? 1u : 0xFFFFFFFFu;

	// ---- extract
	HIP_TRY(PC.mark(0, st));
	DevBuf<unsigned> d_cnt;
	DevBuf<unsigned long long> d_off;
	DevBuf<CovAcc> d_acc;
	ScanScratch SS;
	const CovAcc acc0{0, 0, 0, 0, 0, 0, ~0ull, ~0ull};
	CovAcc acc = acc0;
	unsigned long long n_counted = 0;
	const unsigned grid = stride_grid(c, "LSQ_COV_EXTRACT_GRID", R.n_reads);
	if ((rc = d_cnt.alloc((size_t)R.n_reads)) || (rc = d_off.alloc((size_t)R.n_reads + 1)) || (rc = d_acc.upload(&acc0, 1, st)) || (rc = SS.reserve(R.n_reads))) return rc;
	hipLaunchKernelGGL((lsq_cov_extract_kernel<false>), dim3(grid), dim3(256), 0, st, R, strand_id, d_cnt.p, (const unsigned long long *)nullptr,
	                   (unsigned long long *)nullptr, (unsigned long long *)nullptr, d_acc.p);
	HIP_TRY(hipGetLastError());
	if ((rc = device_scan<1, false>(SS, d_cnt.p, R.n_reads, d_off.p, st))) return rc;
	HIP_TRY(hipMemcpyAsync(&n_counted, d_off.p + R.n_reads, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (n_counted > 0x7FFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32-1 sort records (two per counted block)");
	const unsigned long long n = 2ull * n_counted;
	SortBuf B;                                  // (allocations follow the counted blocks)
	if ((rc = B.reserve(n))) return rc;
	if (n) {
		hipLaunchKernelGGL((lsq_cov_extract_kernel<true>), dim3(grid), dim3(256), 0, st, R, strand_id, (unsigned *)nullptr, (const unsigned long long *)d_off.p,
		                   B.w0[0].p, B.w1[0].p, d_acc.p);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipMemcpyAsync(&acc, d_acc.p, sizeof(acc), hipMemcpyDeviceToHost, st));
	HIP_TRY(PC.mark(1, st));
	HIP_TRY(hipStreamSynchronize(st));
	d_cnt.alloc(0); d_off.alloc(0);
	report[2] = n_counted; report[3] = acc.nochrom; report[4] = acc.empty; report[5] = acc.other; report[6] = acc.bases;

	if (n) {
		// ---- sort: the digits of the position, then the chromosome's; those on which every record agrees are left out
		static const unsigned ALL_DIGITS[6] = {0, 8, 16, 24, 64 + 32, 64 + 40};
		unsigned digits[6];
		const unsigned long long any[2] = {acc.any0, acc.any1}, all[2] = {acc.all0, acc.all1};
		const unsigned n_digits = sort_digits(any, all, ALL_DIGITS, 6, digits);
		if ((rc = device_radix_sort(B, digits, n_digits, st))) return rc;
		HIP_TRY(PC.mark(2, st));
		HIP_TRY(hipStreamSynchronize(st));
		B.w0[B.cur ^ 1].alloc(0); B.w1[B.cur ^ 1].alloc(0); B.hist.alloc(0); B.base.alloc(0);      // (the sort's other half: room for the scans)

		// ---- reduce and scan: the begins ahead of every record, the pieces of positive depth
		const unsigned long long *w0 = B.w0[B.cur].p, *w1 = B.w1[B.cur].p;
		DevBuf<unsigned> d_flag;
		DevBuf<unsigned long long> d_S, d_at;
		unsigned long long n_pieces = 0;
		if ((rc = d_flag.alloc((size_t)n)) || (rc = d_S.alloc((size_t)n + 1)) || (rc = d_at.alloc((size_t)n + 1)) || (rc = SS.reserve(n))) return rc;
		hipLaunchKernelGGL(lsq_cov_begins_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, w1, n, d_flag.p);
		HIP_TRY(hipGetLastError());
		if ((rc = device_scan<1, true>(SS, d_flag.p, n, d_S.p, st))) return rc;
		hipLaunchKernelGGL(lsq_cov_piece_flags_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, w0, w1, (const unsigned long long *)d_S.p, n, d_flag.p);
		HIP_TRY(hipGetLastError());
		if ((rc = device_scan<1, true>(SS, d_flag.p, n, d_at.p, st))) return rc;
		HIP_TRY(hipMemcpyAsync(&n_pieces, d_at.p + n, 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		DevPieces pieces;
		if ((rc = pieces.alloc((size_t)n_pieces))) return rc;
		hipLaunchKernelGGL(lsq_cov_pieces_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, w0, w1, (const unsigned long long *)d_S.p, n, (const unsigned *)d_flag.p,
		                   (const unsigned long long *)d_at.p, pieces.view());
		HIP_TRY(hipGetLastError());
		HIP_TRY(PC.mark(3, st));

		// ---- emit: neighbouring pieces of one depth are one row
		unsigned long long n_heads = 0;
		if (n_pieces) {
			hipLaunchKernelGGL(lsq_cov_row_heads_kernel, dim3(grid_for(n_pieces, 256)), dim3(256), 0, st, pieces.view(), n_pieces, d_flag.p);      // (n_pieces < n: the flags' and the scans' room serves again)
			HIP_TRY(hipGetLastError());
			if ((rc = device_scan<1, true>(SS, d_flag.p, n_pieces, d_at.p, st))) return rc;
			HIP_TRY(hipMemcpyAsync(&n_heads, d_at.p + n_pieces, 8, hipMemcpyDeviceToHost, st));
		}
		HIP_TRY(hipStreamSynchronize(st));
		for (int k = 0; k < 2; ++k) { B.w0[k].alloc(0); B.w1[k].alloc(0); }
		d_S.alloc(0);
		n_rows = (unsigned)n_heads;
		if ((rc = rows.alloc(n_rows))) return rc;
		if (n_rows) {
			hipLaunchKernelGGL(lsq_cov_rows_kernel, dim3(grid_for(n_pieces, 256)), dim3(256), 0, st, pieces.view(), n_pieces, (const unsigned *)d_flag.p, (const unsigned long long *)d_at.p, rows.view());
			HIP_TRY(hipGetLastError());
		}
		HIP_TRY(PC.mark(4, st));
		HIP_TRY(hipStreamSynchronize(st));      // (the pieces, the flags and the places are freed on leaving the block)
	} else { for (int k = 2; k <= 4; ++k) HIP_TRY(PC.mark(k, st)); }
	return LSQ_OK;
}

int lsq::cov_device_reads(lsq_ctx *c, const lsq_cov_index &ix, const ParsedReads &R, int strand, uint32_t min_depth, lsq_cov_table &t) {
	hipStream_t st = c->stream;
	int rc;
	PhaseClock<COV_PHASES> PC;
	if ((rc = PC.make())) return rc;
	if (R.n_reads > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32 reads");
	const size_t n_regions = ix.name.size();
	t.resize(0);
	t.r_covered.assign(n_regions, 0); t.r_depth_sum.assign(n_regions, 0);
	for (uint64_t &v : t.report) v = 0;
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks;
	for (float &m : t.ms) m = 0;
	if (!R.n_reads) return LSQ_OK;
	unsigned n_rows = 0;
	DevPieces rows;
	ScanScratch SS;
	if ((rc = cov_device_rows(c, R, strand, PC, rows, n_rows, t.report))) return rc;

	// ---- regions
	DevBuf<unsigned long long> d_cov, d_sum;
	if (n_rows && n_regions) {
		std::vector<unsigned> ic, il;
		std::vector<int> is, ie;
		for (size_t r = 0; r < n_regions; ++r)
			for (uint64_t q = ix.iv_off[r]; q < ix.iv_off[r + 1]; ++q) {
				const int64_t s = std::max<int64_t>(ix.iv_s[q], -COV_BIAS), e = std::min<int64_t>(ix.iv_e[q], COV_BIAS);
				if (e <= s) continue;
				ic.push_back(ix.chrom[r]); il.push_back((unsigned)r); is.push_back((int)s); ie.push_back((int)e);
			}
		if (ic.size() > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32-1 exon intervals");
		const unsigned ni = (unsigned)ic.size();
		DevBuf<unsigned> d_ic, d_il;
		DevBuf<int> d_is, d_ie;
		DevBuf<unsigned long long> d_wc, d_ws, d_cc, d_cs;
		if ((rc = d_ic.upload(ic.data(), ni, st)) || (rc = d_il.upload(il.data(), ni, st)) || (rc = d_is.upload(is.data(), ni, st)) || (rc = d_ie.upload(ie.data(), ni, st)) ||
		    (rc = d_wc.alloc(n_rows)) || (rc = d_ws.alloc(n_rows)) || (rc = d_cc.alloc((size_t)n_rows + 1)) || (rc = d_cs.alloc((size_t)n_rows + 1)) ||
		    (rc = d_cov.alloc(n_regions)) || (rc = d_sum.alloc(n_regions)) || (rc = SS.reserve(n_rows))) return rc;
		HIP_TRY(hipMemsetAsync(d_cov.p, 0, n_regions * 8, st));
		HIP_TRY(hipMemsetAsync(d_sum.p, 0, n_regions * 8, st));
		hipLaunchKernelGGL(lsq_cov_row_weights_kernel, dim3(grid_for(n_rows, 256)), dim3(256), 0, st, rows.view(), n_rows, (unsigned)min_depth, d_wc.p, d_ws.p);
		HIP_TRY(hipGetLastError());
		// (the sum of bases times depth over all rows is the counted bases: below 2^31 blocks of below 2^31 bases)
		if ((rc = device_scan<1, false, unsigned long long>(SS, d_wc.p, n_rows, d_cc.p, st)) || (rc = device_scan<1, false, unsigned long long>(SS, d_ws.p, n_rows, d_cs.p, st))) return rc;
		if (ni) {
			const CovIntervals I{d_ic.p, d_is.p, d_ie.p, d_il.p, ni};
			hipLaunchKernelGGL(lsq_cov_regions_kernel, dim3(grid_for(ni, 256)), dim3(256), 0, st, I, rows.view(), n_rows, (unsigned)min_depth, (const unsigned long long *)d_cc.p,
			                   (const unsigned long long *)d_cs.p, d_cov.p, d_sum.p);
			HIP_TRY(hipGetLastError());
		}
		HIP_TRY(PC.mark(5, st));
		HIP_TRY(hipMemcpyAsync(t.r_covered.data(), d_cov.p, n_regions * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.r_depth_sum.data(), d_sum.p, n_regions * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));      // (the uploads' host vectors and this block's buffers end here)
	} else HIP_TRY(PC.mark(5, st));

	// ---- copy-back: the rows
	t.resize(n_rows);
	if (n_rows) {
		HIP_TRY(hipMemcpyAsync(t.chrom.data(), rows.chrom.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.start.data(), rows.start.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.end.data(), rows.end.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.depth.data(), rows.depth.p, (size_t)n_rows * 4, hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(PC.mark(6, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (int k = 0; k < COV_PHASES; ++k) (void)PC.ms(k, &t.ms[k]);
	return LSQ_OK;
}

// the records a workgroup of the sort takes (tests place their cases around it)
extern "C" int lsq_cov_sort_tile(void) { return (int)SORT_TILE; }
