// Junction and exon-body reads per event form of a read file (include/lesseq_hip.h, lsq_fe_*): what lsq_evidence.cpp
// (index, host path, positions, text, the evidence executable), lsq_evidence.hip (the device count) and lsq_readfile.hip (the entry
// that opens the read file) share.  The junction half is psi's (lsq_psi.hpp: the index holds an lsq_ps_index), the cells of the
// region lookup are lsq_readtool.hpp's build_cells, as the exon bins'.
#pragma once

#include <memory>

#include "lsq_psi.hpp"

namespace lsq {
constexpr int FE_PHASES = 3;                   // index upload, count, copy-back
// reads, blocks, occurrences that pass the junction rule, block pairs below the overhang, block pairs with a block on no chromosome,
// occurrences found among the informative introns (psi's 1-6); blocks on no chromosome, out of range or empty; (block, region)
// couples that pass the body rule; reads counted for at least one event; for more than one; counted reads none of whose junctions
// is an informative intron
constexpr int FE_REPORT = 11;
constexpr int64_t FE_LIM = (int64_t)1 << 30;   // coordinates of a block with a chromosome lie in (-2^30, 2^30)
constexpr uint32_t FE_MAX_READ_LENGTH = (1u << 18) - 1;

// What positions(f) is computed from, shared by an index and the tables made from it (a table outlives its index): per form the
// maximal intervals of its exon union as the annotation gives them, whether the gap behind an interval is an informative intron
// of the form, and its regions (clamped)
struct FeGeometry {
	std::vector<uint32_t> form_first_iv;       // n_forms + 1
	std::vector<int64_t> iv_start, iv_end;
	std::vector<uint8_t> iv_gap_informative;   // the gap between interval i and i + 1 of the same form
	std::vector<uint32_t> form_first_region;   // n_forms + 1
	std::vector<int32_t> region_start, region_end;
};
}

struct lsq_fe_index {
	lsq_events E;                              // the dictionaries the parsers intern against: the same as P->E, entry for entry
	std::unique_ptr<lsq_ps_index, void (*)(lsq_ps_index *)> P{nullptr, lsq_ps_index_free};      // events, forms, informative introns: psi's, to the letter
	// The informative body: regions numbered form-major (form f's are G->form_first_region[f] .. [f + 1], ascending and apart), on
	// coordinates clamped to [-2^30, 2^30]; form_chrom: the chromosome index of the form's line
	std::shared_ptr<lsq::FeGeometry> G;
	std::vector<uint32_t> form_chrom, region_form;
	std::vector<uint64_t> form_body;           // the bases of B(f)
	// the lookup (build_cells): the cells of every chromosome with the regions that cover them; a stranded index (E.library, and
	// P->E.library): of every table 2 * chromosome + (the event's strand is "-"), 2 * chromosomes + 1 offsets
	std::vector<uint32_t> chrom_first_cell;
	std::vector<int32_t> cell_start, cell_end;
	std::vector<uint32_t> cell_off, cell_regions;
};

struct lsq_fe_table {
	std::vector<std::string> event_name, form_name;      // the index's (the table outlives the index)
	std::vector<uint32_t> event_first_form, form_introns;
	std::vector<uint64_t> form_body;
	std::shared_ptr<const lsq::FeGeometry> G;
	uint32_t min_overhang = 1, min_body = 1;             // what the counts were made under: positions use the same
	std::vector<uint64_t> reads, total;        // per form, per event
	uint64_t report[lsq::FE_REPORT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	int library = LSQ_LIBRARY_UNSTRANDED;      // the index's
	uint64_t lib[lsq::LIB_REPORT] = {0, 0, 0, 0, 0};       // a stranded table's library report
	float ms[lsq::FE_PHASES] = {0, 0, 0};
};

namespace lsq {

// Whether block [s, e) hits region [a, z) under min_body (both on one chromosome, the block not empty): the shared bases
// (constexpr: the device count calls it too)
constexpr bool fe_overlap_hits(int32_t s, int32_t e, int32_t a, int32_t z, uint32_t min_body) {
	return (int64_t)(e < z ? e : z) - (int64_t)(s > a ? s : a) >= (int64_t)min_body;
}

// lsq_evidence.cpp: the table's names and sizes from the index, every count zero
void fe_start_table(const lsq_fe_index &ix, uint32_t min_overhang, uint32_t min_body, lsq_fe_table &t);
int fe_host_reads(const lsq_fe_index &ix, const ParsedReads &R, uint32_t min_overhang, uint32_t min_body, int n_threads, lsq_fe_table &t);
int run_evidence(int argc, const char *const *argv, std::string &out);       // the evidence executable
// lsq_evidence.hip: the count over device arrays
int fe_device_reads(lsq_ctx *c, const lsq_fe_index &ix, const ParsedReads &R, uint32_t min_overhang, uint32_t min_body, lsq_fe_table &t);

} // namespace lsq
