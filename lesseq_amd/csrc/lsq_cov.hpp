// Per-base read depth of a read file (include/lesseq_hip.h, lsq_cov_*): what lsq_cov.cpp (index, host path, text, the
// coverage executable), lsq_cov.hip (the device passes) and lsq_readfile.hip (the entry that opens the read file) share.
// The parsed reads, the dictionaries and the executables' frame are lsq_readtool.hpp's.
#pragma once

#include "lsq_readtool.hpp"

namespace lsq {
constexpr int COV_PHASES = 6;                  // extract, sort, reduce and scan, emit, regions, copy-back
constexpr int COV_REPORT = 7;                  // reads, blocks, counted, without chromosome, empty or descending, other strand, bases
constexpr int64_t COV_BIAS = (int64_t)1 << 30; // coordinates of a block with a chromosome lie in (-2^30, 2^30)
constexpr unsigned long long COV_START = 1ull; // a sort record's payload (w1, below the chromosome): the block begins here (else: it ends here)
}

struct lsq_cov_index {
	// the dictionaries the parsers intern against (annotation_dictionaries): the annotation's chromosomes, "+" (0) and "-" (1), one
	// whole-line interval a chromosome
	lsq_events E;
	// a region per isoform line, in file order; its exon union as maximal intervals, ascending: iv_off[r] .. iv_off[r + 1]
	std::vector<std::string> name, strand;
	std::vector<uint32_t> chrom;
	std::vector<uint64_t> bases;
	std::vector<uint64_t> iv_off;
	std::vector<int64_t> iv_s, iv_e;
};

struct lsq_cov_table {
	std::vector<std::string> chrom_names;      // the index's dictionary (the table outlives the index)
	std::vector<uint32_t> chrom;               // rows
	std::vector<int32_t> start, end;
	std::vector<uint32_t> depth;
	std::vector<std::string> r_name, r_strand; // regions
	std::vector<uint32_t> r_chrom;
	std::vector<uint64_t> r_bases, r_covered, r_depth_sum;
	uint32_t min_depth = 1;
	uint64_t report[lsq::COV_REPORT] = {0, 0, 0, 0, 0, 0, 0};
	float ms[lsq::COV_PHASES] = {0, 0, 0, 0, 0, 0};
	void resize(size_t n) { chrom.resize(n); start.resize(n); end.resize(n); depth.resize(n); }
};

namespace lsq {

// strand: 0 every block, '+' or '-' the blocks of that strand string (the dictionaries' ids 0 and 1)
inline bool cov_strand_ok(int strand) { return strand == 0 || strand == '+' || strand == '-'; }

// lsq_cov.cpp: rows in (chromosome index, start) order -> the table's order (chromosome names bytewise); the regions' names and
// sizes attached (covered and depth_sum are the caller's)
void cov_finish_table(const lsq_cov_index &ix, lsq_cov_table &t);
int cov_host_reads(const lsq_cov_index &ix, const ParsedReads &R, int strand, uint32_t min_depth, int n_threads, lsq_cov_table &t);
int run_coverage(int argc, const char *const *argv, std::string &out);       // the coverage executable
// lsq_cov.hip: the device passes over device arrays; rows come back in (chromosome index, start) order, r_covered and r_depth_sum filled
int cov_device_reads(lsq_ctx *c, const lsq_cov_index &ix, const ParsedReads &R, int strand, uint32_t min_depth, lsq_cov_table &t);

} // namespace lsq
