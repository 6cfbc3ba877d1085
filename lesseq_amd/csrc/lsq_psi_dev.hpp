// What the kernels that match a read's block pairs against the informative introns share (lsq_psi.hip, lsq_evidence.hip; DESIGN
// 4.16, 4.17): the index's lookup on the device, the junction rule on one pair with the search for its intron, and the two
// predicates by which a read counts once a form and once an event without a per-lane list.
#pragma once

#include "lsq_wave.hpp"
#include "lsq_psi.hpp"

namespace lsq {

struct PsIndex {
	const unsigned *chrom_first_intron;                  // n_chroms + 1; a stranded index: 2 * n_chroms + 1, per table 2 * chromosome + t
	const unsigned long long *intron_key;                // n_introns = chrom_first_intron[n_chroms]
	const unsigned *intron_off, *intron_forms;           // n_introns + 1; intron_off[n_introns]
	const unsigned *form_event, *event_first_form;       // n_forms; n_events + 1
	unsigned n_chroms;
};

// the lookup of an lsq_ps_index in device memory
struct PsDeviceIndex {
	DevBuf<unsigned> cf, io, ifo, fe, ef;
	DevBuf<unsigned long long> key;
	int upload(const lsq_ps_index &ix, hipStream_t st) {
		const size_t nf = ix.form_name.size(), ne = ix.event_name.size(), nc = ix.E.covered.size(), ni = ix.intron_key.size();
		int rc;
		if ((rc = cf.upload(ix.chrom_first_intron.data(), nc + 1, st)) || (rc = key.upload((const unsigned long long *)ix.intron_key.data(), ni, st)) ||
		    (rc = io.upload(ix.intron_off.data(), ni + 1, st)) || (rc = ifo.upload(ix.intron_forms.data(), ix.intron_forms.size(), st)) ||
		    (rc = fe.upload(ix.form_event.data(), nf, st)) || (rc = ef.upload(ix.event_first_form.data(), ne + 1, st))) return rc;
		return LSQ_OK;
	}
	PsIndex view(const lsq_ps_index &ix) const { return PsIndex{cf.p, key.p, io.p, ifo.p, fe.p, ef.p, (unsigned)ix.E.n_table_chroms()}; }
};

enum : unsigned { PS_PAIR_NO_JUNCTION, PS_PAIR_NO_CHROM, PS_PAIR_BELOW, PS_PAIR_PASSES };

// The stranded forms of the searches below take the read's transcript strand t, or the pack of the kernel's stranded
// form (lsq_wave.hpp: the library word, the report's counters), as a parameter pack that is empty in the unstranded forms: those
// search the chromosome's introns, as they always did; with t they search table 2 * chromosome + t, and nothing for a read without t.
__device__ inline unsigned ps_table(unsigned chrom) { return chrom; }
__device__ inline unsigned ps_table(unsigned chrom, unsigned t) { return route_table(chrom, t); }
__device__ inline bool ps_has_table() { return true; }
__device__ inline bool ps_has_table(unsigned t) { return t < ROUTE_NO_STRAND; }
// t of the read whose first block is b0 (b0 < n_blocks: the read has a block)
__device__ inline unsigned ps_read_t(const ParsedReads &R, unsigned long long b0, unsigned lib_word, unsigned long long *) { return route_transcript_of_id(lib_word, R.bst[b0]); }

// Blocks j and j + 1 of one read (the caller holds j + 1 < blk_off[r + 1] <= n_blocks: both block loads are in bounds): what the
// junction rule says of the pair and, where it passes, the informative intron it is (PS_NONE: none of them)
template <class... T>
__device__ inline unsigned ps_pair_intron(const ParsedReads &R, const PsIndex &I, unsigned long long j, unsigned min_overhang, unsigned &what, T... t) {
	const unsigned c0 = R.bc[j], c1 = R.bc[j + 1];
	// no table is read for a block on no chromosome, or on one beyond the index's
	if (c0 == NO_CHROM || c1 == NO_CHROM || c0 >= I.n_chroms || c1 >= I.n_chroms) { what = PS_PAIR_NO_CHROM; return PS_NONE; }
	const int s0 = R.bs[j], e0 = R.be[j], s1 = R.bs[j + 1], e1 = R.be[j + 1];
	if (c0 != c1 || s1 <= e0) { what = PS_PAIR_NO_JUNCTION; return PS_NONE; }
	if (min((long long)e0 - s0, (long long)e1 - s1) < (long long)min_overhang) { what = PS_PAIR_BELOW; return PS_NONE; }
	what = PS_PAIR_PASSES;
	if constexpr (sizeof...(T) != 0) {
		if (!ps_has_table(t...)) return PS_NONE;
	}
	const unsigned long long key = jn_key(e0, s1);
	// c0 < n_chroms: chrom_first_intron[c0] and [c0 + 1] are entries of its n_chroms + 1; they ascend and end at n_introns, so
	// lo <= mid < hi <= n_introns in the search, and the last load is guarded by lo < end (with t < 2: table 2 * c0 + t and its
	// successor are entries of the 2 * n_chroms + 1)
	unsigned lo = I.chrom_first_intron[ps_table(c0, t...)], hi = I.chrom_first_intron[ps_table(c0, t...) + 1u];
	const unsigned end = hi;
	while (lo < hi) {
		const unsigned mid = lo + ((hi - lo) >> 1);
		if (I.intron_key[mid] < key) lo = mid + 1u; else hi = mid;
	}
	return lo < end && I.intron_key[lo] == key ? lo : PS_NONE;
}

// Whether intron i's form list holds a form in [f_lo, f_hi): the list ascends, so the first entry at or behind f_lo decides.
// i < n_introns: intron_off[i] and [i + 1] are entries of its n_introns + 1, they ascend and end at the list's size
__device__ inline bool ps_list_holds(const PsIndex &I, unsigned i, unsigned f_lo, unsigned f_hi) {
	unsigned lo = I.intron_off[i], hi = I.intron_off[i + 1u];
	const unsigned end = hi;
	while (lo < hi) {
		const unsigned mid = lo + ((hi - lo) >> 1);
		if (I.intron_forms[mid] < f_lo) lo = mid + 1u; else hi = mid;
	}
	return lo < end && I.intron_forms[lo] < f_hi;
}

// ps_pair_intron in the tables of the pair's read, whose first block is b0 <= j (lib: the pack of the kernel's stranded form)
__device__ inline unsigned ps_pair_of_read(const ParsedReads &R, const PsIndex &I, unsigned long long, unsigned long long j, unsigned min_overhang, unsigned &what) {
	return ps_pair_intron(R, I, j, min_overhang, what);
}
__device__ inline unsigned ps_pair_of_read(const ParsedReads &R, const PsIndex &I, unsigned long long b0, unsigned long long j, unsigned min_overhang, unsigned &what, unsigned lib_word, unsigned long long *lib) {
	return ps_pair_intron(R, I, j, min_overhang, what, ps_read_t(R, b0, lib_word, lib));
}
// whether a pair of the read ahead of pair k that passes the rule is an informative intron with a form in [f_lo, f_hi)
template <class... LIB>
__device__ inline bool ps_met_before(const ParsedReads &R, const PsIndex &I, unsigned long long b0, unsigned long long k, unsigned min_overhang, unsigned f_lo, unsigned f_hi, LIB... lib) {
	for (unsigned long long j = b0; j < k; ++j) {      // (j + 1 <= k, and k + 1 < the read's last offset)
		unsigned what;
		const unsigned i = ps_pair_of_read(R, I, b0, j, min_overhang, what, lib...);
		if (i != PS_NONE && ps_list_holds(I, i, f_lo, f_hi)) return true;
	}
	return false;
}

} // namespace lsq
