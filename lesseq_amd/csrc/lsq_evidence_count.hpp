// The count kernel of the evidence table in its two forms: what lsq_evidence.hip, which launches the unstranded
// form, and lsq_stranded.hip, which launches the stranded one, share.  Two translation units, so that the unstranded kernel is
// compiled beside exactly the code it was compiled beside before there was a stranded form: its instructions are what they were.
#pragma once

#include "lsq_psi_dev.hpp"
#include "lsq_evidence.hpp"

namespace lsq {

struct FeIndex {
	const int *region_start, *region_end;                // clamped to [-2^30, 2^30]; n_regions = form_first_region[n_forms]
	const unsigned *region_form, *form_first_region;     // n_regions; n_forms + 1
	const unsigned *form_chrom;                          // n_forms
	const unsigned *chrom_first_cell;                    // n_chroms + 1
	const int *cell_start, *cell_end;                    // n_cells = chrom_first_cell[n_chroms]
	const unsigned *cell_off, *cell_regions;             // n_cells + 1; cell_off[n_cells]
};
struct FeAcc { unsigned long long occurrences, dropped, nochrom, found, skipped, body_hits, counted, multi_event, body_alone; };
// lsq_stranded.hip: the stranded form launched (lib_word: route_lib_word; lib: the library report's five counters, zeroed)
void fe_launch_stranded(unsigned grid, hipStream_t st, const ParsedReads &R, const PsIndex &I, const FeIndex &F, unsigned min_overhang, unsigned min_body, unsigned long long *reads,
                        unsigned long long *total, FeAcc *acc, unsigned lib_word, unsigned long long *lib);

} // namespace lsq

namespace {      // (device code of the unit that includes it: internal linkage)
using namespace lsq;


// Whether block j of the read (j < n_blocks) hits, under min_body, a region with an id below g_stop of a form in [f_lo, f_hi)
// (f_hi <= n_forms: form_first_region[f] and [f + 1] are entries of its n_forms + 1, they ascend and end at n_regions).  A form's
// regions ascend and lie apart, so the first that ends behind the block's start begins the few the block can reach.
__device__ inline bool fe_block_hits(const ParsedReads &R, const FeIndex &F, unsigned n_chroms, unsigned long long j, unsigned f_lo, unsigned f_hi, unsigned g_stop, unsigned min_body) {
	const unsigned c = R.bc[j];
	const int s = R.bs[j], e = R.be[j];
	if (c == NO_CHROM || c >= n_chroms || e <= s) return false;
	for (unsigned f = f_lo; f < f_hi; ++f) {
		unsigned lo = F.form_first_region[f], hi = min(F.form_first_region[f + 1u], g_stop);
		if (lo >= g_stop) break;
		if (F.form_chrom[f] != c) continue;
		const unsigned end = hi;
		while (lo < hi) {
			const unsigned mid = lo + ((hi - lo) >> 1);
			if (F.region_end[mid] <= s) lo = mid + 1u; else hi = mid;
		}
		for (; lo < end && F.region_start[lo] < e; ++lo)
			if (fe_overlap_hits(s, e, F.region_start[lo], F.region_end[lo], min_body)) return true;
	}
	return false;
}

// Whether, ahead of the couple (block k, region g), the read holds evidence for a form in [f_lo, f_hi): any pair of the read (all
// of them are walked before the first block: pairs b0 .. b1 - 2) on an informative intron of such a form, an earlier block on a
// region of such a form, or block k itself on such a region with a lower id.  b0 <= k < b1: at most 15 pairs and 16 blocks.
// (lib: the pack of the kernel's stranded form -- the pairs are sought in the tables of the read's strand; the regions of the
// forms asked about are of one event, whose strand is the read's: fe_block_hits needs no strand)
template <class... LIB>
__device__ inline bool fe_met_before(const ParsedReads &R, const PsIndex &I, const FeIndex &F, unsigned long long b0, unsigned long long b1, unsigned long long k, unsigned g,
                                     unsigned min_overhang, unsigned min_body, unsigned f_lo, unsigned f_hi, LIB... lib) {
	if (ps_met_before(R, I, b0, b1 - 1ull, min_overhang, f_lo, f_hi, lib...)) return true;
	for (unsigned long long j = b0; j < k; ++j) if (fe_block_hits(R, F, I.n_chroms, j, f_lo, f_hi, NO_ID, min_body)) return true;
	return fe_block_hits(R, F, I.n_chroms, k, f_lo, f_hi, g, min_body);
}

// A lane a read, a fixed number of workgroups striding over the reads.  A lane walks its read up to the next couple that counts,
// then the whole wave combines what its lanes found (wave_add_ids) and goes on: as many rounds as the wave's busiest read has hits.
//   First the pairs, as lsq_ps_count_kernel walks them: the rule's verdict goes to the report, an informative intron opens its form
//   list, a form counts unless an earlier pair holds it, the event with its first form in the list unless an earlier pair holds
//   any of its forms.
//   Then the blocks: a block on no chromosome or empty is skipped; the others search the first cell that ends behind their start
//   and walk the cells up to their end.  A region is looked at in the first of its cells the walk meets -- the walk's first cell,
//   or the cell the region begins at -- and hits when it shares min_body bases with the block.  The hit's event counts unless the
//   read met any form of the event before (fe_met_before), and with it the form; else the form counts unless the read met it before.  Regions are
//   numbered form-major and an event's forms are neighbours, so "a lower id of the event" is a range.  An event that counts has a
//   form that counts: what came before the couple for the form came before it for the event.
// The report's tallies are kept per lane over the stride, summed over the workgroup once and added by one lane.  The LDS counters
// (36 KiB: four workgroups a compute unit) are added to the global ones behind the tallies' barrier.
// The stranded form (kernel<true, unsigned, unsigned long long *>: the word of lsq_route.hpp's route_lib_word and the
// library report's five counters -- a parameter pack, empty in the unstranded form, whose arguments and code stay what they
// were): every intron search and every cell search goes to table 2 * chromosome + t of the read's transcript strand t -- that of
// the strand id of its first block -- and a read without t searches none: its pairs' verdicts and its skipped blocks are still
// tallied, and the loop stays uniform.  The predicates compare pairs and blocks of one read, which share t.
template <bool STRANDED, class... LIB>
__global__ void __launch_bounds__(256) lsq_fe_count_kernel(ParsedReads R, PsIndex I, FeIndex F, unsigned min_overhang, unsigned min_body, unsigned long long *reads, unsigned long long *total, FeAcc *acc, LIB... lib) {
	__shared__ unsigned long long part_a[4][4], part_b[4][4], part_c[4][4];
	__shared__ WgCounters<2048> local_forms;
	__shared__ WgCounters<1024> local_events;
	local_forms.clear(); local_events.clear();
	__syncthreads();
	const unsigned lane = threadIdx.x & 63u;
	unsigned long long occ = 0, dropped = 0, nochrom = 0, found = 0, skipped = 0, body_hits = 0, counted = 0, multi = 0, alone = 0;
	LibLane LL;                                      // (the stranded form's)
	const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
	// (the wave's first read decides whether the wave has any: the loop is uniform, a lane beyond the last read has no block)
	for (unsigned long long base = (unsigned long long)blockIdx.x * 256u + (threadIdx.x & ~63u); base < R.n_reads; base += stride) {
		const unsigned long long r = base + lane;
		const bool have = r < R.n_reads;
		// r < n_reads: blk_off[r] and [r + 1] are entries of its n_reads + 1; they ascend and end at n_blocks
		const unsigned long long b0 = have ? R.blk_off[r] : 0ull, b1 = have ? R.blk_off[r + 1] : 0ull;
		unsigned long long k = b0, kc = b0;              // pairs: the next pair to begin (blocks k, k + 1), the pair being walked; blocks: the next block to begin
		unsigned p = 0, p_begin = 0, p_end = 0;          // the list being walked (an intron's forms, a cell's regions) and where the walk is in it
		int s = 0, e = 0;                                // the block being walked
		unsigned cell = 0, cell_hi = 0;
		bool blocks = false, walking = false, first = false;
		unsigned events = 0, found_here = 0;
		for (;;) {
			unsigned hit_form = NO_ID, hit_event = NO_ID;
			while (hit_form == NO_ID) {
				if (!blocks) {
					if (p < p_end) {
						// intron_off[i] <= p_begin <= p < p_end = intron_off[i + 1] <= the list's size; p - 1 is read only behind p_begin
						const unsigned f = I.intron_forms[p];
						const bool heads_event_range = p == p_begin || I.intron_forms[p - 1u] < I.event_first_form[I.form_event[f]];
						++p;
						if (ps_met_before(R, I, b0, kc, min_overhang, f, f + 1u, lib...)) continue;
						hit_form = f;
						// f < n_forms (the index lists form ids only), its event < n_events: both offsets are entries of n_events + 1
						const unsigned ev = I.form_event[f];
						if (heads_event_range && !ps_met_before(R, I, b0, kc, min_overhang, I.event_first_form[ev], I.event_first_form[ev + 1u], lib...)) hit_event = ev;
					} else if (k + 1 < b1) {                 // the next pair: blocks k and k + 1 < b1 <= n_blocks
						kc = k++;
						unsigned what;
						const unsigned i = ps_pair_of_read(R, I, b0, kc, min_overhang, what, lib...);
						if (what == PS_PAIR_NO_CHROM) ++nochrom;
						else if (what == PS_PAIR_BELOW) ++dropped;
						else if (what == PS_PAIR_PASSES) ++occ;
						if (i != PS_NONE) { ++found; ++found_here; p = p_begin = I.intron_off[i]; p_end = I.intron_off[i + 1u]; }
					} else { blocks = true; k = b0; p = p_end = 0; }      // the pairs are done
				} else if (p < p_end) {
					// cell < n_cells: cell_off[cell] <= p < p_end = cell_off[cell + 1] <= the list's size, whose entries are region ids
					const unsigned g = F.cell_regions[p++];
					const int a = F.region_start[g], z = F.region_end[g];
					if (!first && a != F.cell_start[cell]) continue;       // met in an earlier cell of this walk
					if (!fe_overlap_hits(s, e, a, z, min_body)) continue;
					++body_hits;
					// g < n_regions: its form < n_forms, the form's event < n_events; the block walked is k - 1, b0 <= k - 1 < b1
					// the event is asked first: what came before the couple for the form came before it for the event, so a fresh
					// event has a fresh form, and most hits need no second predicate
					const unsigned f = F.region_form[g], ev = I.form_event[f];
					if (!fe_met_before(R, I, F, b0, b1, k - 1ull, g, min_overhang, min_body, I.event_first_form[ev], I.event_first_form[ev + 1u], lib...)) hit_event = ev;
					else if (fe_met_before(R, I, F, b0, b1, k - 1ull, g, min_overhang, min_body, f, f + 1u, lib...)) continue;
					hit_form = f;
				} else if (walking) {                        // the next cell of the walk
					++cell; first = false;
					if (cell < cell_hi && F.cell_start[cell] < e) { p = F.cell_off[cell]; p_end = F.cell_off[cell + 1u]; }
					else walking = false;
				} else if (k < b1) {                         // the next block: k < b1 <= n_blocks
					s = R.bs[k]; e = R.be[k];
					const unsigned ch = R.bc[k];
					++k;
					// no table is read for a block on no chromosome, or on one beyond the index's
					if (ch == NO_CHROM || ch >= I.n_chroms || e <= s) { ++skipped; continue; }
					// ch < n_chroms: chrom_first_cell[ch] and [ch + 1] are entries of its n_chroms + 1; they ascend and end at n_cells
					unsigned lo;
					if constexpr (STRANDED) {
						// (the read has a block, so b0 < n_blocks; t lives in no variable of the kernel's, as in lsq_xb_count_kernel)
						const unsigned t = ps_read_t(R, b0, lib...);
						if (t >= ROUTE_NO_STRAND) continue;      // a read without t: its blocks are tallied, and that is all
						// ch < n_chroms and t < 2: table 2 * ch + t and its successor are entries of the 2 * n_chroms + 1 offsets
						const unsigned tb = route_table(ch, t);
						lo = F.chrom_first_cell[tb];
						cell_hi = F.chrom_first_cell[tb + 1u];
					} else {
						lo = F.chrom_first_cell[ch];
						cell_hi = F.chrom_first_cell[ch + 1u];
					}
					unsigned hi = cell_hi;
					while (lo < hi) {                        // the first cell that ends behind s
						const unsigned mid = lo + ((hi - lo) >> 1);
						if (F.cell_end[mid] <= s) lo = mid + 1u; else hi = mid;
					}
					if (lo < cell_hi && F.cell_start[lo] < e) { cell = lo; walking = true; first = true; p = F.cell_off[lo]; p_end = F.cell_off[lo + 1u]; }
				} else break;                                // the read is done
			}
			if (!__any(hit_form != NO_ID)) break;
			if (hit_event != NO_ID) ++events;
			wave_add_ids(local_forms, reads, hit_form, lane);
			wave_add_ids(local_events, total, hit_event, lane);
		}
		if (events > 0) ++counted;
		if (events > 1) ++multi;
		if (events > 0 && found_here == 0) ++alone;
		if constexpr (STRANDED) {
			if (have) LL.note(b0 < b1 ? ps_read_t(R, b0, lib...) : ROUTE_NO_STRAND, events > 0);
		}
	}
	if constexpr (STRANDED) LL.flush(lib_counters(lib...));
	unsigned long long u[4] = {occ, dropped, nochrom, found}, v[4] = {skipped, body_hits, counted, multi}, w[4] = {alone, 0ull, 0ull, 0ull};
	workgroup_tally<false>(u, part_a);
	workgroup_tally<false>(v, part_b);
	workgroup_tally<false>(w, part_c);               // (its barrier is the one the LDS counters wait behind)
	local_forms.flush(reads); local_events.flush(total);
	if (threadIdx.x == 0) {
		if (u[0]) atomicAdd(&acc->occurrences, u[0]);
		if (u[1]) atomicAdd(&acc->dropped, u[1]);
		if (u[2]) atomicAdd(&acc->nochrom, u[2]);
		if (u[3]) atomicAdd(&acc->found, u[3]);
		if (v[0]) atomicAdd(&acc->skipped, v[0]);
		if (v[1]) atomicAdd(&acc->body_hits, v[1]);
		if (v[2]) atomicAdd(&acc->counted, v[2]);
		if (v[3]) atomicAdd(&acc->multi_event, v[3]);
		if (w[0]) atomicAdd(&acc->body_alone, w[0]);
	}
}

} // namespace
