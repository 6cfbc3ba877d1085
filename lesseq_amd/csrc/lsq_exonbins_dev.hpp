// The count kernel of the exon-bin table in its two forms: what lsq_exonbins.hip, which launches the unstranded
// form, and lsq_stranded.hip, which launches the stranded one, share.  Two translation units, so that the unstranded kernel is
// compiled beside exactly the code it was compiled beside before there was a stranded form: its instructions are what they were.
#pragma once

#include "lsq_wave.hpp"
#include "lsq_exonbins.hpp"

namespace lsq {

struct XbIndex {
	const int *bin_start, *bin_end;                      // clamped to [-2^30, 2^30]
	const unsigned *bin_gene, *gene_first_bin;
	const unsigned *chrom_first_cell;                    // per chromosome; the stranded form: per table 2 * chromosome + t
	const int *cell_start, *cell_end;
	const unsigned *cell_off, *cell_bins;
	unsigned n_chroms;
};
struct XbAcc { unsigned long long bad_blocks, no_gene, multi_gene, bin_hits; };
// lsq_stranded.hip: the stranded form launched (lib_word: route_lib_word; lib: the library report's five counters, zeroed)
void xb_launch_stranded(unsigned grid, hipStream_t st, const ParsedReads &R, const XbIndex &I, unsigned long long *reads, unsigned long long *total, XbAcc *acc, unsigned lib_word, unsigned long long *lib);

} // namespace lsq

namespace {      // (device code of the unit that includes it: internal linkage)
using namespace lsq;

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
// The stranded form (kernel<true, unsigned, unsigned long long *>: the word of lsq_route.hpp's route_lib_word and the
// library report's five counters -- a parameter pack, empty in the unstranded form, whose arguments and code stay what they
// were): the read's transcript strand t from the strand id of its first block, every cell search in table 2 * chromosome + t in
// place of the chromosome's, a read without t searching no table -- its blocks are still tallied, and the loop stays
// uniform.  The predicates compare blocks of one read, which share t: they are the unstranded form's.
template <bool STRANDED, class... LIB>
__global__ void __launch_bounds__(256) lsq_xb_count_kernel(ParsedReads R, XbIndex I, unsigned long long *reads, unsigned long long *total, XbAcc *acc, LIB... lib) {
	__shared__ unsigned long long part[4][4];
	__shared__ WgCounters<2048> local_bins;
	__shared__ WgCounters<1024> local_genes;
	local_bins.clear(); local_genes.clear();
	__syncthreads();
	const unsigned lane = threadIdx.x & 63u;
	unsigned long long bad = 0, none = 0, multi = 0, hits = 0;
	LibLane LL;                                      // (the stranded form's)
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
					unsigned lo;
					if constexpr (STRANDED) {
						// (the read has a block, so b0 < n_blocks.  t lives in no variable of the kernel's: a local more, even a dead
						// one, gave the unstranded form other registers)
						const unsigned t = route_transcript_of_id(lib_word(lib...), R.bst[b0]);
						if (t >= ROUTE_NO_STRAND) continue;      // a read without t: its blocks are tallied, and that is all
						// ch < n_chroms and t < 2: table 2 * ch + t and its successor are entries of the 2 * n_chroms + 1 offsets
						const unsigned tb = route_table(ch, t);
						lo = I.chrom_first_cell[tb];
						cell_hi = I.chrom_first_cell[tb + 1u];
					} else {
						lo = I.chrom_first_cell[ch];
						cell_hi = I.chrom_first_cell[ch + 1u];
					}
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
		if constexpr (STRANDED) {
			if (have) {
				const unsigned t = b0 < b1 ? route_transcript_of_id(lib_word(lib...), R.bst[b0]) : ROUTE_NO_STRAND;
				LL.note(t, genes > 0);
				if (t < ROUTE_NO_STRAND && genes == 0) ++none;
			}
		} else {
			if (have && genes == 0) ++none;
		}
		if (genes > 1) ++multi;
	}
	if constexpr (STRANDED) LL.flush(lib_counters(lib...));
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
