// Splice-site usage and read-through per junction of a read file (include/lesseq_hip.h, lsq_ss_*): what lsq_sites.cpp
// (index, the merge of junction rows with annotated introns, the boundary arrays, host path, text, the sites executable),
// lsq_sites.hip (the device count of the blocks that run through a boundary) and lsq_readfile.hip (the entry that opens the read
// file) share.  The junction rows are lsq_junc.hpp's, made by its passes as they are; the parsed reads, the dictionaries and the
// executables' frame are lsq_readtool.hpp's.
#pragma once

#include "lsq_junc.hpp"

namespace lsq {
constexpr int SS_PHASES = 4;                   // junctions (the sum of its five), index, through, copy-back
constexpr int SS_REPORT = 8;                   // junctions' five, distinct boundaries, the sum of all boundary counts, rows with reads 0
}

// The junction index under another name: the dictionaries the parsers intern against and the sorted distinct introns
struct lsq_ss_index {
	lsq_jn_index *J;
	lsq_events &E;                             // J's (lsq_readtool.hpp's templates take an index by its E)
	explicit lsq_ss_index(lsq_jn_index *j) : J(j), E(j->E) {}
	lsq_ss_index(const lsq_ss_index &) = delete;
	lsq_ss_index &operator=(const lsq_ss_index &) = delete;
	~lsq_ss_index() { lsq_jn_index_free(J); }
};

struct lsq_ss_table {
	std::vector<std::string> chrom_names;      // the index's dictionary (the table outlives the index)
	std::vector<uint32_t> chrom;
	std::vector<int32_t> start, end;
	std::vector<uint8_t> ann;
	std::vector<uint64_t> reads, left_spliced, left_through, right_spliced, right_through;
	uint64_t report[lsq::SS_REPORT] = {0, 0, 0, 0, 0, 0, 0, 0};
	float ms[lsq::SS_PHASES] = {0, 0, 0, 0};
};

namespace lsq {

// What both paths count against, made on the host from a junction table (its rows in any order) and the index's introns: the
// rows -- the table's united with every intron, ascending in (chromosome index, start, end) -- and the boundaries, the distinct
// starts and ends of all rows: chromosome c's are pos[chrom_first_boundary[c] .. chrom_first_boundary[c + 1]], ascending; a
// row's left boundary (its start) is row_left, its right one (its end) row_right.
struct SsPlan {
	std::vector<uint32_t> chrom;
	std::vector<int32_t> start, end;
	std::vector<uint8_t> ann;
	std::vector<uint64_t> reads;
	std::vector<uint32_t> chrom_first_boundary;
	std::vector<int32_t> pos;
	std::vector<uint32_t> row_left, row_right;
};

// the overhang the through count asks of a block on either side of a boundary: a boundary lies between two bases, so at least 1
inline uint64_t ss_through_overhang(uint32_t min_overhang) { return std::max<uint64_t>(min_overhang, 1); }

// lsq_sites.cpp
int ss_plan(const lsq_ss_index &ix, const lsq_jn_table &jt, SsPlan &P);            // LSQ_E_RANGE beyond 2^32-2 boundaries
// the table from the plan, the boundaries' counts and the junction table's report: the spliced sums, the rows in the table's order
void ss_finish_table(const lsq_ss_index &ix, const SsPlan &P, const std::vector<uint64_t> &through, const lsq_jn_table &jt, lsq_ss_table &t);
int ss_host_reads(const lsq_ss_index &ix, const ParsedReads &R, uint32_t min_overhang, int n_threads, lsq_ss_table &t);
int run_sites(int argc, const char *const *argv, std::string &out);                // the sites executable
// lsq_sites.hip: the junction passes, the plan uploaded, the through count over device arrays
int ss_device_reads(lsq_ctx *c, const lsq_ss_index &ix, const ParsedReads &R, uint32_t min_overhang, lsq_ss_table &t);

} // namespace lsq
