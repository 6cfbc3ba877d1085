// Intron retention of a parsed read file on the device (include/lesseq_hip.h, lsq_ir_device): five phases -- sites
// (lsq_sites.hip's four as they are: the rows of columns 1-9), depth (lsq_cov.hip's extract, sort, reduce and scan, emit as they
// are: the depth rows, left on the device), index (the introns' clean pieces, made on the host by lsq_retention.cpp, uploaded),
// select (a lane a piece: the depth rows it overlaps by two binary searches; then a wave an intron: covered bases, depth sum and
// largest depth in one pass over the rows of its pieces, the three order statistics by bisection on the depth), copy-back (five
// arrays of one entry an intron).  Every number is an integer; a wave's lanes are combined by sums and a maximum, every result is
// written once: no atomics, nothing depends on the order in which lanes arrive.
#include "lsq_wave.hpp"
#include "lsq_cov_dev.hpp"
#include "lsq_retention.hpp"

namespace {

struct IrPieceView { const unsigned *chrom; const int *start, *end; unsigned n; };

// A lane a piece [s, e) of chromosome c: the depth rows it overlaps are first .. end.  Rows ascend in (chromosome, start) and do
// not overlap, so they ascend in (chromosome, end) too (lsq_cov_regions_kernel's two searches).
__global__ void __launch_bounds__(256) lsq_ir_ranges_kernel(IrPieceView P, CovPieces O, unsigned n_rows, unsigned *row_first, unsigned *row_end) {
	const unsigned q = blockIdx.x * 256u + threadIdx.x;
	if (q >= P.n) return;
	const unsigned c = P.chrom[q];
	const int s = P.start[q], e = P.end[q];
	unsigned lo = 0, hi = n_rows;
	while (lo < hi) {                                            // the first row that ends behind s
		const unsigned mid = lo + ((hi - lo) >> 1);
		const unsigned mc = O.chrom[mid];
		if (mc < c || (mc == c && O.end[mid] <= s)) lo = mid + 1u; else hi = mid;
	}
	row_first[q] = lo;
	hi = n_rows;
	while (lo < hi) {                                            // the first row that begins at or behind e
		const unsigned mid = lo + ((hi - lo) >> 1);
		const unsigned mc = O.chrom[mid];
		if (mc < c || (mc == c && O.start[mid] < e)) lo = mid + 1u; else hi = mid;
	}
	row_end[q] = lo;
}

__device__ inline unsigned wave_max(unsigned v) {
	for (unsigned d = 32; d; d >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, (int)d));
	return v;
}

struct IrIntrons { const unsigned *piece_off; const unsigned long long *clean; unsigned n; };
struct IrOut { unsigned long long *covered, *depth_sum; unsigned *q25, *q50, *q75; };

// A wave an intron, a fixed number of workgroups striding over the introns.  The lanes stride over the rows of the intron's pieces,
// piece by piece; a row is clipped to its piece (only a piece's first and last row reach beyond it).  The first pass gives the
// covered bases, the depth sum and the largest depth m; the clean bases without a row are the zeros.  Order statistic q is the
// smallest v in [0, m] with zeros + (bases of depth 1 .. v) >= rank q: [lo, hi] halves with every further pass, all three ranks
// counted in one pass, until all three have closed -- at most ceil(log2(m + 1)) passes.  The rows of a piece are neighbours in
// memory, so the lanes' loads coalesce.  Lane 0 writes the intron's five results.
__global__ void __launch_bounds__(256) lsq_ir_select_kernel(IrIntrons I, IrPieceView P, const unsigned *row_first, const unsigned *row_end, CovPieces O, IrOut out) {
	const unsigned lane = threadIdx.x & 63u;
	for (unsigned long long i = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6); i < I.n; i += (unsigned long long)gridDim.x * 4u) {
		const unsigned p0 = I.piece_off[i], p1 = I.piece_off[i + 1u];
		const unsigned long long n = I.clean[i];
		unsigned long long covered = 0, sum = 0;
		unsigned m = 0;
		for (unsigned p = p0; p < p1; ++p) {
			const int s = P.start[p], e = P.end[p];
			for (unsigned r = row_first[p] + lane, r1 = row_end[p]; r < r1; r += 64u) {
				const unsigned long long len = (unsigned long long)((long long)min(e, O.end[r]) - max(s, O.start[r]));
				const unsigned d = O.depth[r];
				covered += len; sum += len * d; m = max(m, d);
			}
		}
		covered = wave_sum(covered); sum = wave_sum(sum); m = wave_max(m);
		const unsigned long long zeros = n - covered;
		unsigned long long rank[3];
		unsigned lo[3], hi[3];
#pragma unroll
		for (unsigned q = 0; q < 3; ++q) {
			rank[q] = n ? ir_rank(q + 1u, n) : 0ull;
			lo[q] = 0u; hi[q] = rank[q] <= zeros ? 0u : m;           // (a rank among the zeros, or no clean base: 0)
		}
		while (lo[0] < hi[0] || lo[1] < hi[1] || lo[2] < hi[2]) {    // (uniform over the wave: every term is)
			unsigned mid[3];
			unsigned long long upto[3] = {0ull, 0ull, 0ull};         // bases of depth 1 .. mid
#pragma unroll
			for (unsigned q = 0; q < 3; ++q) mid[q] = lo[q] + ((hi[q] - lo[q]) >> 1);
			for (unsigned p = p0; p < p1; ++p) {
				const int s = P.start[p], e = P.end[p];
				for (unsigned r = row_first[p] + lane, r1 = row_end[p]; r < r1; r += 64u) {
					const unsigned long long len = (unsigned long long)((long long)min(e, O.end[r]) - max(s, O.start[r]));
					const unsigned d = O.depth[r];
#pragma unroll
					for (unsigned q = 0; q < 3; ++q) upto[q] += d <= mid[q] ? len : 0ull;
				}
			}
#pragma unroll
			for (unsigned q = 0; q < 3; ++q) {
				const unsigned long long below = zeros + wave_sum(upto[q]);
				if (lo[q] < hi[q]) { if (below >= rank[q]) hi[q] = mid[q]; else lo[q] = mid[q] + 1u; }
			}
		}
		if (lane == 0) { out.covered[i] = covered; out.depth_sum[i] = sum; out.q25[i] = lo[0]; out.q50[i] = lo[1]; out.q75[i] = lo[2]; }
	}
}

} // namespace

int lsq::ir_device_reads(lsq_ctx *c, const lsq_ir_index &ix, const ParsedReads &R, uint32_t min_overhang, lsq_ir_table &t) {
	hipStream_t st = c->stream;
	int rc;
	PhaseClock<COV_PHASES> CC;                    // coverage's own marks: extract .. emit are its first four phases
	PhaseClock<3> PC;                             // index, select, copy-back
	if ((rc = CC.make()) || (rc = PC.make())) return rc;
	if (R.n_reads > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32 reads");

	// ---- sites
	lsq_ss_table sites;
	if ((rc = ss_device_reads(c, *ix.S, R, min_overhang, sites))) return rc;

	// ---- depth: the rows stay on the device
	DevPieces rows;
	unsigned n_rows = 0;
	uint64_t cov_report[COV_REPORT] = {R.n_reads, R.n_blocks, 0, 0, 0, 0, 0};
	if (R.n_reads) { if ((rc = cov_device_rows(c, R, 0, CC, rows, n_rows, cov_report))) return rc; }
	else if ((rc = rows.alloc(0))) return rc;

	// ---- index: the rows and their pieces, on the host; the pieces uploaded
	HIP_TRY(PC.mark(0, st));
	IrPieces P;
	if ((rc = ir_rows_and_pieces(ix, sites, t, P))) return rc;
	t.report[11] = n_rows; t.report[12] = cov_report[6];
	const size_t n = t.chrom.size(), np = P.chrom.size();
	DevBuf<unsigned> d_off, d_pc, d_first, d_end, d_q25, d_q50, d_q75;
	DevBuf<int> d_ps, d_pe;
	DevBuf<unsigned long long> d_clean, d_cov, d_sum;
	if ((rc = d_off.upload(P.piece_off.data(), n + 1, st)) || (rc = d_pc.upload(P.chrom.data(), np, st)) || (rc = d_ps.upload(P.start.data(), np, st)) ||
	    (rc = d_pe.upload(P.end.data(), np, st)) || (rc = d_clean.upload((const unsigned long long *)t.clean.data(), n, st)) || (rc = d_first.alloc(np)) || (rc = d_end.alloc(np)) ||
	    (rc = d_cov.alloc(n)) || (rc = d_sum.alloc(n)) || (rc = d_q25.alloc(n)) || (rc = d_q50.alloc(n)) || (rc = d_q75.alloc(n))) return rc;

	// ---- select
	HIP_TRY(PC.mark(1, st));
	if (n) {
		const IrPieceView V{d_pc.p, d_ps.p, d_pe.p, (unsigned)np};
		if (np) {
			hipLaunchKernelGGL(lsq_ir_ranges_kernel, dim3(grid_for(np, 256)), dim3(256), 0, st, V, rows.view(), n_rows, d_first.p, d_end.p);
			HIP_TRY(hipGetLastError());
		}
		const IrIntrons I{d_off.p, d_clean.p, (unsigned)n};
		const IrOut out{d_cov.p, d_sum.p, d_q25.p, d_q50.p, d_q75.p};
		// (a wave an intron: 64 lanes each)
		hipLaunchKernelGGL(lsq_ir_select_kernel, dim3(stride_grid(c, "LSQ_IR_GRID", 64ull * n)), dim3(256), 0, st, I, V, (const unsigned *)d_first.p, (const unsigned *)d_end.p, rows.view(), out);
		HIP_TRY(hipGetLastError());
	}

	// ---- copy-back
	HIP_TRY(PC.mark(2, st));
	if (n) {
		HIP_TRY(hipMemcpyAsync(t.covered.data(), d_cov.p, n * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.depth_sum.data(), d_sum.p, n * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.q25.data(), d_q25.p, n * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.q50.data(), d_q50.p, n * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(t.q75.data(), d_q75.p, n * 4, hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(PC.mark(3, st));
	HIP_TRY(hipStreamSynchronize(st));
	t.ms[0] = t.ms[1] = 0;
	for (float v : sites.ms) t.ms[0] += v;
	if (R.n_reads) for (int k = 0; k < 4; ++k) { float v = 0; (void)CC.ms(k, &v); t.ms[1] += v; }
	for (int k = 0; k < 3; ++k) (void)PC.ms(k, &t.ms[k + 2]);
	return LSQ_OK;
}
