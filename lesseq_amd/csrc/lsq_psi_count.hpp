// The count kernel of the psi table in its two forms: what lsq_psi.hip, which launches the unstranded form, and
// lsq_stranded.hip, which launches the stranded one, share.  Two translation units, so that the unstranded kernel is compiled
// beside exactly the code it was compiled beside before there was a stranded form: its instructions are what they were.
#pragma once

#include "lsq_wave.hpp"
#include "lsq_psi_dev.hpp"

namespace lsq {

struct PsAcc { unsigned long long occurrences, dropped, nochrom, found, counted, multi_event; };
// lsq_stranded.hip: the stranded form launched (lib_word: route_lib_word; lib: the library report's five counters, zeroed)
void ps_launch_stranded(unsigned grid, hipStream_t st, const ParsedReads &R, const PsIndex &I, unsigned min_overhang, unsigned long long *reads, unsigned long long *total, PsAcc *acc,
                        unsigned lib_word, unsigned long long *lib);

} // namespace lsq

namespace {      // (device code of the unit that includes it: internal linkage)
using namespace lsq;

// A lane a read, a fixed number of workgroups striding over the reads.  A lane walks its read's (pair, form) couples up to the next
// one that counts, then the whole wave combines what its lanes found (wave_add_ids) and goes on: as many rounds as the wave's
// busiest read has hits.  What counts:
//   a pair is looked at once, when the walk begins it: the rule's verdict goes to the report, an informative intron opens its form list;
//   a form of the list counts unless an earlier pair of the read that passes the rule is an intron whose list holds it too;
//   the event is looked at with its first form in the list -- the list's first, or one whose predecessor lies ahead of the event's
//   first form: an event's forms are neighbours -- and counts unless an earlier pair's list holds any form of the event.  An
//   event that counts has a form that counts: an earlier pair on that form is an earlier pair on the event.
// A read keeps at most 16 blocks, so "earlier pairs" are at most 15 searches.  The report's tallies are kept per lane over the
// stride, summed over the workgroup once and added by one lane.  The LDS counters (36 KiB: four workgroups a compute unit) are
// added to the global ones behind the tallies' barrier.
// The stranded form (kernel<true, unsigned, unsigned long long *>: the word of lsq_route.hpp's route_lib_word and the
// library report's five counters -- a parameter pack, empty in the unstranded form, whose arguments and code stay what they
// were): every intron search, those of the predicates included, goes to table 2 * chromosome + t of the read's transcript strand
// t -- that of the strand id of its first block -- and a read without t finds no intron: its pairs' verdicts are still tallied,
// and the loop stays uniform.  The predicates compare pairs of one read, which share t.
template <bool STRANDED, class... LIB>
__global__ void __launch_bounds__(256) lsq_ps_count_kernel(ParsedReads R, PsIndex I, unsigned min_overhang, unsigned long long *reads, unsigned long long *total, PsAcc *acc, LIB... lib) {
	__shared__ unsigned long long part_a[4][4], part_b[4][4];
	__shared__ WgCounters<2048> local_forms;
	__shared__ WgCounters<1024> local_events;
	local_forms.clear(); local_events.clear();
	__syncthreads();
	const unsigned lane = threadIdx.x & 63u;
	unsigned long long occ = 0, dropped = 0, nochrom = 0, found = 0, counted = 0, multi = 0;
	LibLane LL;                                      // (the stranded form's)
	const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
	// (the wave's first read decides whether the wave has any: the loop is uniform, a lane beyond the last read has no pair)
	for (unsigned long long base = (unsigned long long)blockIdx.x * 256u + (threadIdx.x & ~63u); base < R.n_reads; base += stride) {
		const unsigned long long r = base + lane;
		const bool have = r < R.n_reads;
		// r < n_reads: blk_off[r] and [r + 1] are entries of its n_reads + 1; they ascend and end at n_blocks
		const unsigned long long b0 = have ? R.blk_off[r] : 0ull, b1 = have ? R.blk_off[r + 1] : 0ull;
		unsigned long long k = b0, kc = b0;              // the next pair to begin (blocks k, k + 1); the pair being walked
		unsigned p = 0, p_begin = 0, p_end = 0;          // its intron's form list, and where the walk is in it
		unsigned events = 0;
		for (;;) {
			unsigned hit_form = NO_ID, hit_event = NO_ID;
			while (hit_form == NO_ID) {
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
					if (i != PS_NONE) { ++found; p = p_begin = I.intron_off[i]; p_end = I.intron_off[i + 1u]; }
				} else break;                            // the read is done
			}
			if (!__any(hit_form != NO_ID)) break;
			if (hit_event != NO_ID) ++events;
			wave_add_ids(local_forms, reads, hit_form, lane);
			wave_add_ids(local_events, total, hit_event, lane);
		}
		if (events > 0) ++counted;
		if (events > 1) ++multi;
		if constexpr (STRANDED) {
			if (have) LL.note(b0 < b1 ? ps_read_t(R, b0, lib...) : ROUTE_NO_STRAND, events > 0);
		}
	}
	if constexpr (STRANDED) LL.flush(lib_counters(lib...));
	unsigned long long v[4] = {occ, dropped, nochrom, found}, w[4] = {counted, multi, 0ull, 0ull};
	workgroup_tally<false>(v, part_a);
	workgroup_tally<false>(w, part_b);               // (its barrier is the one the LDS counters wait behind)
	local_forms.flush(reads); local_events.flush(total);
	if (threadIdx.x == 0) {
		if (v[0]) atomicAdd(&acc->occurrences, v[0]);
		if (v[1]) atomicAdd(&acc->dropped, v[1]);
		if (v[2]) atomicAdd(&acc->nochrom, v[2]);
		if (v[3]) atomicAdd(&acc->found, v[3]);
		if (w[0]) atomicAdd(&acc->counted, w[0]);
		if (w[1]) atomicAdd(&acc->multi_event, w[1]);
	}
}

} // namespace
