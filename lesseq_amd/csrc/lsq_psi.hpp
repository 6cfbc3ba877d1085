// Junction reads per event form of a read file (include/lesseq_hip.h, lsq_ps_*): what lsq_psi.cpp (index, host path,
// text, the psi executable), lsq_psi.hip (the device count) and lsq_readfile.hip (the entry that opens the read file) share.
// The parsed reads, the dictionaries and the executables' frame are lsq_readtool.hpp's; a junction's key is lsq_junc.hpp's.
#pragma once

#include "lsq_junc.hpp"

namespace lsq {
constexpr int PS_PHASES = 3;                   // index upload, count, copy-back
// reads, blocks, occurrences that pass the junction rule, block pairs below the overhang, block pairs with a block on no chromosome,
// occurrences found among the informative introns, reads counted for at least one event, reads counted for more than one
constexpr int PS_REPORT = 8;
constexpr uint32_t PS_NONE = 0xFFFFFFFFu;
}

struct lsq_ps_index {
	// the dictionaries the parsers intern against (annotation_dictionaries): the annotation's chromosomes, "+" (0) and "-" (1), one
	// whole-line interval a chromosome
	lsq_events E;
	// events in the loader's order (count's), an event's forms in the order of its lines in the gene->isoform file: event e's forms
	// are the ids event_first_form[e] .. event_first_form[e + 1]
	std::vector<std::string> event_name, form_name;
	std::vector<std::string> event_strand;     // the strand string its lines share, "." where they differ or the event has none
	std::vector<uint32_t> event_first_form, form_event;
	std::vector<uint32_t> form_introns;        // |D(f)|
	// The lookup: the distinct informative introns ascending in (chromosome index, jn_key), chromosome c's are
	// chrom_first_intron[c] .. chrom_first_intron[c + 1]; the forms that hold intron i as an informative one, ascending, are
	// intron_forms[intron_off[i] .. intron_off[i + 1]] (never empty).  A stranded index (E.library) keeps the lookup
	// per table id 2 * c + (the event's strand is "-") instead of per chromosome c: 2 * chromosomes + 1 offsets, and an intron
	// that events of both strands hold is two introns, one in either table.
	std::vector<uint32_t> chrom_first_intron;
	std::vector<uint64_t> intron_key;
	std::vector<uint32_t> intron_off, intron_forms;
};

struct lsq_ps_table {
	std::vector<std::string> event_name, form_name;      // the index's (the table outlives the index)
	std::vector<uint32_t> event_first_form, form_introns;
	std::vector<uint64_t> reads, total;        // per form, per event
	uint64_t report[lsq::PS_REPORT] = {0, 0, 0, 0, 0, 0, 0, 0};
	int library = LSQ_LIBRARY_UNSTRANDED;      // the index's
	uint64_t lib[lsq::LIB_REPORT] = {0, 0, 0, 0, 0};       // a stranded table's library report
	float ms[lsq::PS_PHASES] = {0, 0, 0};
};

namespace lsq {

// the informative intron of chromosome (stranded index: table) c with key `key` (PS_NONE: none)
inline uint32_t ps_find_intron(const lsq_ps_index &ix, size_t c, uint64_t key) {
	uint32_t lo = ix.chrom_first_intron[c], hi = ix.chrom_first_intron[c + 1];
	const uint32_t end = hi;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (ix.intron_key[mid] < key) lo = mid + 1; else hi = mid;
	}
	return lo < end && ix.intron_key[lo] == key ? lo : PS_NONE;
}
// The junction rule on blocks b and b + 1 of one read on the host (psi's and evidence's host paths): the verdict is tallied in
// n -- [0] passes, [1] below the overhang, [2] a block on no chromosome -- and the informative intron the pair is comes back
// (PS_NONE: no junction, or none of them).  t: the read's transcript strand under a stranded index -- the intron is sought in the
// tables of that strand, and a read without one (2) finds none.
inline uint32_t ps_host_pair(const lsq_ps_index &ix, const ParsedReads &R, uint64_t b, uint32_t min_overhang, uint64_t *n, unsigned t = 0) {
	const size_t nc = ix.E.n_table_chroms();
	const unsigned c0 = R.bc[b], c1 = R.bc[b + 1];
	if (c0 == NO_CHROM || c1 == NO_CHROM || c0 >= nc || c1 >= nc) { ++n[2]; return PS_NONE; }
	if (c0 != c1 || R.bs[b + 1] <= R.be[b]) return PS_NONE;
	const int64_t ov = std::min((int64_t)R.be[b] - R.bs[b], (int64_t)R.be[b + 1] - R.bs[b + 1]);
	if (ov < (int64_t)min_overhang) { ++n[1]; return PS_NONE; }
	++n[0];
	if (t >= 2u) return PS_NONE;
	return ps_find_intron(ix, ix.E.table_of(c0, t), jn_key(R.be[b], R.bs[b + 1]));
}

// lsq_psi.cpp: lsq_ps_index_build_library for `tool` ("psi"; "evidence": its junction half), whose name the message of an event without a strand carries
int ps_index_build(const lsq_annotation *a, int library, const char *tool, lsq_ps_index **out);
// lsq_psi.cpp: the table's names and sizes from the index, every count zero
void ps_start_table(const lsq_ps_index &ix, lsq_ps_table &t);
int ps_host_reads(const lsq_ps_index &ix, const ParsedReads &R, uint32_t min_overhang, int n_threads, lsq_ps_table &t);
int run_psi(int argc, const char *const *argv, std::string &out);            // the psi executable
// lsq_psi.hip: the count over device arrays
int ps_device_reads(lsq_ctx *c, const lsq_ps_index &ix, const ParsedReads &R, uint32_t min_overhang, lsq_ps_table &t);

} // namespace lsq
