// Which library type is this read file? (include/lesseq_hip.h, lsq_lt_*): what lsq_libtype.cpp (index, host path,
// text, the libtype executable), lsq_libtype.hip (the device count) and lsq_readfile.hip (the entry that opens the read file)
// share.  The parsed reads, the dictionaries and the executables' frame are lsq_readtool.hpp's.
#pragma once

#include "lsq_readtool.hpp"

namespace lsq {
constexpr int LT_PHASES = 3;                   // index upload, count, copy-back
// reads without a first-mate strand; then, for r = + and for r = -: reads on no gene, on plus genes only, on minus genes only, on both
constexpr int LT_CLASSES = 9;
constexpr int64_t LT_LIM = (int64_t)1 << 30;   // coordinates of a block with a chromosome lie in (-2^30, 2^30)
// the class of a read: r (0 plus, 1 minus, 2 none), whether a block of it met the plus union, the minus union
constexpr unsigned lt_class(unsigned r, bool plus, bool minus) { return r >= 2u ? 0u : 1u + 4u * r + (plus ? 1u : 0u) + (minus ? 2u : 0u); }
}

struct lsq_lt_index {
	// stranded dictionaries (annotation_dictionaries under a library type): the parsers deliver the strand of a fragment's first
	// mate, r = s XOR mate2, as the strand id -- "+" 0, "-" 1
	lsq_events E;
	// per table id 2 * chromosome + (strand == "-"): the union of all exons of that strand's genes on the chromosome as sorted
	// disjoint intervals, clamped to [-2^30, 2^30]; table tb's are tab_first[tb] .. tab_first[tb + 1]
	std::vector<uint32_t> tab_first;
	std::vector<int32_t> iv_start, iv_end;
	uint64_t unplaced_genes = 0;               // genes without a strand of their own (or a line on another chromosome's table): left out
};

struct lsq_lt_table {
	uint64_t reads = 0, cls[lsq::LT_CLASSES] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
	uint64_t unplaced_genes = 0;
	float ms[lsq::LT_PHASES] = {0, 0, 0};
};

namespace lsq {

int lt_host_reads(const lsq_lt_index &ix, const ParsedReads &R, int n_threads, lsq_lt_table &t);
int run_libtype(int argc, const char *const *argv, std::string &out);        // the libtype executable
// lsq_libtype.hip: the count over device arrays
int lt_device_reads(lsq_ctx *c, const lsq_lt_index &ix, const ParsedReads &R, lsq_lt_table &t);

} // namespace lsq
