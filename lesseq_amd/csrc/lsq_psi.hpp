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
	std::vector<uint32_t> event_first_form, form_event;
	std::vector<uint32_t> form_introns;        // |D(f)|
	// The lookup: the distinct informative introns ascending in (chromosome index, jn_key), chromosome c's are
	// chrom_first_intron[c] .. chrom_first_intron[c + 1]; the forms that hold intron i as an informative one, ascending, are
	// intron_forms[intron_off[i] .. intron_off[i + 1]] (never empty)
	std::vector<uint32_t> chrom_first_intron;
	std::vector<uint64_t> intron_key;
	std::vector<uint32_t> intron_off, intron_forms;
};

struct lsq_ps_table {
	std::vector<std::string> event_name, form_name;      // the index's (the table outlives the index)
	std::vector<uint32_t> event_first_form, form_introns;
	std::vector<uint64_t> reads, total;        // per form, per event
	uint64_t report[lsq::PS_REPORT] = {0, 0, 0, 0, 0, 0, 0, 0};
	float ms[lsq::PS_PHASES] = {0, 0, 0};
};

namespace lsq {

// lsq_psi.cpp: the table's names and sizes from the index, every count zero
void ps_start_table(const lsq_ps_index &ix, lsq_ps_table &t);
int ps_host_reads(const lsq_ps_index &ix, const ParsedReads &R, uint32_t min_overhang, int n_threads, lsq_ps_table &t);
int run_psi(int argc, const char *const *argv, std::string &out);            // the psi executable
// lsq_psi.hip: the count over device arrays
int ps_device_reads(lsq_ctx *c, const lsq_ps_index &ix, const ParsedReads &R, uint32_t min_overhang, lsq_ps_table &t);

} // namespace lsq
