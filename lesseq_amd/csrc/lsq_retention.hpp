// Intron retention of a read file (include/lesseq_hip.h, lsq_ir_*): per intron of the annotation its sites row and
// the depth over its clean bases -- those in no exon of any isoform line -- as covered bases, depth sum and three order
// statistics.  What lsq_retention.cpp (index, the pieces, host path, text, the retention executable), lsq_retention.hip (the device
// selection over coverage's rows) and lsq_readfile.hip (the entry that opens the read file) share.  The sites rows are
// lsq_sites.hpp's, the depth rows lsq_cov.hpp's, both made by their passes as they are.
#pragma once

#include "lsq_sites.hpp"
#include "lsq_cov.hpp"

namespace lsq {
constexpr int IR_PHASES = 5;                   // sites (the sum of its four), depth (coverage's extract .. emit), index, select, copy-back
constexpr int IR_REPORT = 13;                  // sites' eight, introns, introns without a clean base, pieces, depth rows, counted bases
}

// The sites index, the dictionaries again as the depth rows' host path takes them, and every chromosome's exons
struct lsq_ir_index {
	lsq_ss_index *S;
	lsq_events &E;                             // S's (lsq_readtool.hpp's templates take an index by its E)
	lsq_cov_index C;                           // the same dictionaries and no region
	// chromosome c's exon union over all its isoform lines, both strands: maximal intervals, clamped to +-2^30, ascending,
	// ex_s / ex_e [ex_off[c] .. ex_off[c + 1])
	std::vector<uint64_t> ex_off;
	std::vector<int32_t> ex_s, ex_e;
	explicit lsq_ir_index(lsq_ss_index *s) : S(s), E(s->E) {}
	lsq_ir_index(const lsq_ir_index &) = delete;
	lsq_ir_index &operator=(const lsq_ir_index &) = delete;
	~lsq_ir_index() { lsq_ss_index_free(S); }
};

struct lsq_ir_table {
	std::vector<std::string> chrom_names;      // the index's dictionary (the table outlives the index)
	std::vector<uint32_t> chrom;
	std::vector<int32_t> start, end;
	std::vector<uint8_t> ann;
	std::vector<uint64_t> reads, left_spliced, left_through, right_spliced, right_through;
	std::vector<uint64_t> clean, covered, depth_sum;
	std::vector<uint32_t> q25, q50, q75;
	uint64_t report[lsq::IR_REPORT] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	float ms[lsq::IR_PHASES] = {0, 0, 0, 0, 0};
};

namespace lsq {

// The clean bases of the table's introns as maximal intervals: intron i's pieces are piece_off[i] .. piece_off[i + 1], each
// [start, end) on `chrom` (a chromosome index), ascending
struct IrPieces {
	std::vector<uint32_t> piece_off, chrom;
	std::vector<int32_t> start, end;
};

// the rank of order statistic q (1, 2, 3) among n sorted depths, from 1: ceil(q n / 4); n >= 1
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned long long ir_rank(unsigned q, unsigned long long n) { return (q * n + 3ull) / 4ull; }

// lsq_retention.cpp: the table's rows -- the sites table's with an ann other than '.', in its order, columns 1-9 unchanged --
// their pieces, `clean`, and the report's entries 0 .. 10; covered, depth_sum and the order statistics are sized and zero.
// LSQ_E_RANGE beyond 2^32-2 pieces.
int ir_rows_and_pieces(const lsq_ir_index &ix, const lsq_ss_table &st, lsq_ir_table &t, IrPieces &P);
int ir_host_reads(const lsq_ir_index &ix, const ParsedReads &R, uint32_t min_overhang, int n_threads, lsq_ir_table &t);
int run_retention(int argc, const char *const *argv, std::string &out);            // the retention executable
// lsq_retention.hip: the sites passes, coverage's rows left on the device, the pieces uploaded, the selection
int ir_device_reads(lsq_ctx *c, const lsq_ir_index &ix, const ParsedReads &R, uint32_t min_overhang, lsq_ir_table &t);

} // namespace lsq
