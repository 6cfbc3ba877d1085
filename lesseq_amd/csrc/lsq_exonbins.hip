// The reads per exon bin and per gene of a parsed read file on the device (include/lesseq_hip.h, lsq_xb_device): three
// phases over device arrays -- index upload, count (a lane a read: every block a binary search in its chromosome's cells and a
// walk over them; a read counts once a bin and once a gene by predicates alone, no per-lane list; equal ids are combined inside the
// wave, then added to the workgroup's own counters in LDS, or to the global ones where the id has no slot there: lsq_wave.hpp), copy-back (the
// counters).  Every number is an integer and sums commute: no result depends on the order in which lanes arrive.
#include "lsq_wave.hpp"
#include "lsq_exonbins.hpp"

namespace {

struct XbIndex {
	const int *bin_start, *bin_end;                      // clamped to [-2^30, 2^30]
	const unsigned *bin_gene, *gene_first_bin;
	const unsigned *chrom_first_cell;
	const int *cell_start, *cell_end;
	const unsigned *cell_off, *cell_bins;
	unsigned n_chroms;
};
struct XbAcc { unsigned long long bad_blocks, no_gene, multi_gene, bin_hits; };

// Whether block [s, e) overlaps any bin of a gene: its bins first .. last ascend and are disjoint, so the first that ends behind s decides
__device__ inline bool xb_gene_overlaps(const XbIndex &I, unsigned first, unsigned last, int s, int e) {
	unsigned lo = first, hi = last;
	while (lo < hi) {
		const unsigned mid = lo + ((hi - lo) >> 1);
		if (I.bin_end[mid] <= s) lo = mid + 1u; else hi = mid;
	}
	return lo < last && I.bin_start[lo] < e;
}

// A lane a read, a fixed number of workgroups striding over the reads.  A lane walks its read's (block, cell, bin) triples up to
// the next one that counts, then the whole wave combines what its lanes found (lsq_wave.hpp's wave_add_ids) and goes on: as many rounds as the
// wave's busiest read has hits.  What counts:
//   a (block k, bin) pair is looked at in the bin's first cell of block k's walk: the walk's first cell, or the cell the bin begins at;
//   the bin counts unless an earlier block j < k of the read overlaps it too (the blocks come in any order: every j is tried);
//   the gene is looked at with its first bin that block k overlaps -- the gene's first, or one whose predecessor ends at or ahead
//   of the block's start -- and counts unless an earlier block overlaps any bin of the gene (xb_gene_overlaps).  A gene that
//   counts has a bin that counts: an earlier block on the bin is an earlier block on the gene.
// The report's tallies are kept per lane over the stride, summed over the workgroup once and added by one lane.  The LDS counters
// (36 KiB: four workgroups a compute unit) are added to the global ones behind the same barrier.
__global__ void __launch_bounds__(256) lsq_xb_count_kernel(ParsedReads R, XbIndex I, unsigned long long *reads, unsigned long long *total, XbAcc *acc) {
	__shared__ unsigned long long part[4][4];
	__shared__ WgCounters<2048> local_bins;
	__shared__ WgCounters<1024> local_genes;
	local_bins.clear(); local_genes.clear();
	__syncthreads();
	const unsigned lane = threadIdx.x & 63u;
	unsigned long long bad = 0, none = 0, multi = 0, hits = 0;
	const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
	// (the wave's first read decides whether the wave has any: the loop is uniform, a lane beyond the last read has no block)
	for (unsigned long long base = (unsigned long long)blockIdx.x * 256u + (threadIdx.x & ~63u); base < R.n_reads; base += stride) {
		const unsigned long long r = base + lane;
		const bool have = r < R.n_reads;
		const unsigned long long b0 = have ? R.blk_off[r] : 0ull, b1 = have ? R.blk_off[r + 1] : 0ull;
		unsigned long long k = b0;                       // the next block to begin
		int s = 0, e = 0;                                // the block being walked
		unsigned cell = 0, cell_hi = 0, p = 0, p_end = 0;
		bool walking = false, first = false;
		unsigned genes = 0;
		for (;;) {
			unsigned hit_bin = XB_NONE, hit_gene = XB_NONE;
			while (hit_bin == XB_NONE) {
				if (p < p_end) {
					const unsigned bin = I.cell_bins[p++];
					const int bs = I.bin_start[bin], be = I.bin_end[bin];
					if (!first && bs != I.cell_start[cell]) continue;      // met in an earlier cell of this walk
					const unsigned ch = R.bc[k - 1];
					bool fresh = true;
					for (unsigned long long j = b0; j + 1 < k && fresh; ++j)
						if (R.bc[j] == ch && R.be[j] > R.bs[j] && R.bs[j] < be && R.be[j] > bs) fresh = false;
					if (!fresh) continue;
					hit_bin = bin;
					const unsigned g = I.bin_gene[bin], g0 = I.gene_first_bin[g], g1 = I.gene_first_bin[g + 1];
					if (bin == g0 || I.bin_end[bin - 1u] <= s) {
						bool fresh_gene = true;
						for (unsigned long long j = b0; j + 1 < k && fresh_gene; ++j)
							if (R.bc[j] == ch && R.be[j] > R.bs[j] && xb_gene_overlaps(I, g0, g1, R.bs[j], R.be[j])) fresh_gene = false;
						if (fresh_gene) hit_gene = g;
					}
				} else if (walking) {                     // the next cell of the walk
					++cell; first = false;
					if (cell < cell_hi && I.cell_start[cell] < e) { p = I.cell_off[cell]; p_end = I.cell_off[cell + 1u]; }
					else walking = false;
				} else if (k < b1) {                      // the next block
					s = R.bs[k]; e = R.be[k];
					const unsigned ch = R.bc[k];
					++k;
					if (ch == NO_CHROM || ch >= I.n_chroms || e <= s) { ++bad; continue; }
					unsigned lo = I.chrom_first_cell[ch];
					cell_hi = I.chrom_first_cell[ch + 1u];
					unsigned hi = cell_hi;
					while (lo < hi) {                     // the first cell that ends behind s
						const unsigned mid = lo + ((hi - lo) >> 1);
						if (I.cell_end[mid] <= s) lo = mid + 1u; else hi = mid;
					}
					if (lo < cell_hi && I.cell_start[lo] < e) { cell = lo; walking = true; first = true; p = I.cell_off[lo]; p_end = I.cell_off[lo + 1u]; }
				} else break;                             // the read is done
			}
			if (!__any(hit_bin != XB_NONE)) break;
			if (hit_bin != XB_NONE) ++hits;
			if (hit_gene != XB_NONE) ++genes;
			wave_add_ids(local_bins, reads, hit_bin, lane);
			wave_add_ids(local_genes, total, hit_gene, lane);
		}
		if (have && genes == 0) ++none;
		if (genes > 1) ++multi;
	}
	unsigned long long v[4] = {bad, none, multi, hits};
	workgroup_tally<false>(v, part);                 // (its barrier is the one the LDS counters wait behind)
	local_bins.flush(reads); local_genes.flush(total);
	if (threadIdx.x == 0) {
		if (v[0]) atomicAdd(&acc->bad_blocks, v[0]);
		if (v[1]) atomicAdd(&acc->no_gene, v[1]);
		if (v[2]) atomicAdd(&acc->multi_gene, v[2]);
		if (v[3]) atomicAdd(&acc->bin_hits, v[3]);
	}
}

} // namespace

int lsq::xb_device_reads(lsq_ctx *c, const lsq_xb_index &ix, const ParsedReads &R, lsq_xb_table &t) {
	hipStream_t st = c->stream;
	int rc;
	PhaseClock<XB_PHASES> PC;
	if ((rc = PC.make())) return rc;
	xb_start_table(ix, t);
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks;
	const size_t nb = ix.bin_gene.size(), ng = ix.gene_name.size(), nc = ix.E.covered.size(), n_cells = ix.cell_start.size();

	// ---- index upload
	HIP_TRY(PC.mark(0, st));
	DevBuf<int> d_bs, d_be, d_cs, d_ce;
	DevBuf<unsigned> d_bg, d_gf, d_cf, d_co, d_cb;
	DevBuf<unsigned long long> d_reads, d_total;
	DevBuf<XbAcc> d_acc;
	const XbAcc acc0{0, 0, 0, 0};
	XbAcc acc = acc0;
	if ((rc = d_bs.upload(ix.c_bin_start.data(), nb, st)) || (rc = d_be.upload(ix.c_bin_end.data(), nb, st)) || (rc = d_bg.upload(ix.bin_gene.data(), nb, st)) ||
	    (rc = d_gf.upload(ix.gene_first_bin.data(), ng + 1, st)) || (rc = d_cf.upload(ix.chrom_first_cell.data(), nc + 1, st)) ||
	    (rc = d_cs.upload(ix.cell_start.data(), n_cells, st)) || (rc = d_ce.upload(ix.cell_end.data(), n_cells, st)) ||
	    (rc = d_co.upload(ix.cell_off.data(), n_cells + 1, st)) || (rc = d_cb.upload(ix.cell_bins.data(), ix.cell_bins.size(), st)) ||
	    (rc = d_reads.alloc(nb)) || (rc = d_total.alloc(ng)) || (rc = d_acc.upload(&acc0, 1, st))) return rc;
	if (nb) HIP_TRY(hipMemsetAsync(d_reads.p, 0, nb * 8, st));
	if (ng) HIP_TRY(hipMemsetAsync(d_total.p, 0, ng * 8, st));

	// ---- count
	HIP_TRY(PC.mark(1, st));
	if (R.n_reads) {
		const XbIndex I{d_bs.p, d_be.p, d_bg.p, d_gf.p, d_cf.p, d_cs.p, d_ce.p, d_co.p, d_cb.p, (unsigned)nc};
		hipLaunchKernelGGL(lsq_xb_count_kernel, dim3(stride_grid(c, "LSQ_XB_GRID", R.n_reads)), dim3(256), 0, st, R, I, d_reads.p, d_total.p, d_acc.p);
		HIP_TRY(hipGetLastError());
	}

	// ---- copy-back
	HIP_TRY(PC.mark(2, st));
	if (nb) HIP_TRY(hipMemcpyAsync(t.reads.data(), d_reads.p, nb * 8, hipMemcpyDeviceToHost, st));
	if (ng) HIP_TRY(hipMemcpyAsync(t.total.data(), d_total.p, ng * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&acc, d_acc.p, sizeof(acc), hipMemcpyDeviceToHost, st));
	HIP_TRY(PC.mark(3, st));
	HIP_TRY(hipStreamSynchronize(st));
	t.report[2] = acc.bad_blocks; t.report[3] = acc.no_gene; t.report[4] = acc.multi_gene; t.report[5] = acc.bin_hits;
	for (int k = 0; k < XB_PHASES; ++k) (void)PC.ms(k, &t.ms[k]);
	return LSQ_OK;
}
