// Splice junctions of a read file (include/lesseq_hip.h, lsq_jn_*): what lsq_junc.cpp (index, host path, text, the
// junctions executable), lsq_junc.hip (the device passes) and lsq_readfile.hip (the entry that opens the read file) share.
// The parsed reads, the dictionaries and the executables' frame are lsq_readtool.hpp's.
#pragma once

#include "lsq_readtool.hpp"

// The key of a junction: the chromosome's index, and start and end biased by 2^30 (coordinates lie in (-2^30, 2^30)) in one word
namespace lsq {
constexpr int64_t JN_BIAS = (int64_t)1 << 30;
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint64_t jn_key(int64_t start, int64_t end) { return ((uint64_t)(start + JN_BIAS) << 31) | (uint64_t)(end + JN_BIAS); }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int32_t jn_key_start(uint64_t k) { return (int32_t)((int64_t)(k >> 31) - JN_BIAS); }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int32_t jn_key_end(uint64_t k) { return (int32_t)((int64_t)(k & 0x7FFFFFFFull) - JN_BIAS); }
constexpr int JN_PHASES = 5;                   // extract, sort, reduce, annotate, copy-back
}

struct lsq_jn_index {
	// the dictionaries the parsers intern against (annotation_dictionaries): `chroms` the annotation's chromosomes, `strands` seeded with "+" (0) and "-" (1),
	// `covered` one whole-line interval a chromosome (the name-keyed formats of lsq_reads_parse keep every line of a known chromosome)
	lsq_events E;
	// the distinct introns, ascending in (chromosome index, key)
	std::vector<uint32_t> in_chrom;
	std::vector<uint64_t> in_key;
	std::vector<uint8_t> in_ann;               // '+', '-' or '*'
};

struct lsq_jn_table {
	std::vector<std::string> chrom_names;      // the index's dictionary (the table outlives the index)
	std::vector<uint32_t> chrom;
	std::vector<int32_t> start, end;
	std::vector<uint8_t> ann;
	std::vector<uint32_t> reads, plus, minus, max_overhang;
	uint64_t report[5] = {0, 0, 0, 0, 0};      // reads, blocks, occurrences, pairs dropped by the overhang, pairs with a block without chromosome
	float ms[lsq::JN_PHASES] = {0, 0, 0, 0, 0};
	void resize(size_t n) { chrom.resize(n); start.resize(n); end.resize(n); ann.resize(n); reads.resize(n); plus.resize(n); minus.resize(n); max_overhang.resize(n); }
};

namespace lsq {

constexpr unsigned JN_OV_MASK = 0x3FFFFFFFu, JN_PLUS = 1u << 30, JN_MINUS = 1u << 31;      // an occurrence's payload: overhang (< 2^30), strand flags

// lsq_junc.cpp: rows in (chromosome index, start, end) order -> the table's order (chromosome names bytewise), names attached
void jn_finish_table(const lsq_jn_index &ix, lsq_jn_table &t);
int jn_host_reads(const lsq_jn_index &ix, const ParsedReads &R, uint32_t min_overhang, int n_threads, lsq_jn_table &t);
int run_junctions(int argc, const char *const *argv, std::string &out);      // the junctions executable
// lsq_junc.hip: the device passes over device arrays; the table's rows come back in (chromosome index, start, end) order
int jn_device_reads(lsq_ctx *c, const lsq_jn_index &ix, const ParsedReads &R, uint32_t min_overhang, lsq_jn_table &t);

} // namespace lsq
