// Reads per exon bin and per gene of a read file (include/lesseq_hip.h, lsq_xb_*): what lsq_exonbins.cpp (index, host
// path, text, the exonbins executable), lsq_exonbins.hip (the device count) and lsq_readfile.hip (the entry that opens the read
// file) share.
// The parsed reads, the dictionaries and the executables' frame are lsq_readtool.hpp's.
#pragma once

#include "lsq_readtool.hpp"

namespace lsq {
constexpr int XB_PHASES = 3;                   // index upload, count, copy-back
constexpr int XB_REPORT = 6;                   // reads, blocks, blocks without chromosome or empty, reads on no gene, reads on several genes, bin hits
constexpr int64_t XB_LIM = (int64_t)1 << 30;   // coordinates of a block with a chromosome lie in (-2^30, 2^30)
constexpr uint32_t XB_NONE = 0xFFFFFFFFu;
}

struct lsq_xb_index {
	// the dictionaries the parsers intern against (annotation_dictionaries): the annotation's chromosomes, "+" (0) and "-" (1), one
	// whole-line interval a chromosome
	lsq_events E;
	// genes in the loader's order (count's); gene g's bins are gene_first_bin[g] .. gene_first_bin[g + 1], ascending and disjoint
	std::vector<std::string> gene_name, gene_strand;
	std::vector<uint32_t> gene_chrom;          // XB_NONE: a gene without an isoform line
	std::vector<uint32_t> gene_first_bin;
	std::vector<int64_t> bin_start, bin_end;   // as the annotation gives them
	std::vector<uint32_t> bin_gene;
	// The lookup, on coordinates clamped to [-2^30, 2^30] (no block with a chromosome reaches beyond; a bin that lies outside is
	// empty there and in no cell).  A chromosome cut at every bin boundary: the cells that at least one bin covers, ascending and
	// disjoint, chromosome c's are chrom_first_cell[c] .. chrom_first_cell[c + 1]; the bins that cover cell i, ascending, are
	// cell_bins[cell_off[i] .. cell_off[i + 1]].  A bin covers every cell between its start and its end: they are neighbours.
	// A stranded index (E.library) keeps the lookup per table id 2 * c + (the gene's strand is "-") instead of per
	// chromosome c: chrom_first_cell has 2 * chromosomes + 1 entries, and a cell holds bins of one strand only.
	std::vector<int32_t> c_bin_start, c_bin_end;
	std::vector<uint32_t> chrom_first_cell;
	std::vector<int32_t> cell_start, cell_end;
	std::vector<uint32_t> cell_off, cell_bins;
};

struct lsq_xb_table {
	std::vector<std::string> gene_name;        // the index's (the table outlives the index)
	std::vector<uint32_t> gene_first_bin;
	std::vector<uint64_t> reads, total;        // per bin, per gene
	uint64_t report[lsq::XB_REPORT] = {0, 0, 0, 0, 0, 0};
	int library = LSQ_LIBRARY_UNSTRANDED;      // the index's
	uint64_t lib[lsq::LIB_REPORT] = {0, 0, 0, 0, 0};       // a stranded table's library report
	float ms[lsq::XB_PHASES] = {0, 0, 0};
};

namespace lsq {

// lsq_exonbins.cpp: the table's names and sizes from the index, every count zero
void xb_start_table(const lsq_xb_index &ix, lsq_xb_table &t);
int xb_host_reads(const lsq_xb_index &ix, const ParsedReads &R, int n_threads, lsq_xb_table &t);
int run_exonbins(int argc, const char *const *argv, std::string &out);       // the exonbins executable
// lsq_exonbins.hip: the count over device arrays
int xb_device_reads(lsq_ctx *c, const lsq_xb_index &ix, const ParsedReads &R, lsq_xb_table &t);

} // namespace lsq
