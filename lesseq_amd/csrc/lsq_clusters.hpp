// Intron clusters of several read files (include/lesseq_hip.h, lsq_cl_*): what lsq_clusters.cpp (the pool, the
// reader of `junctions` text, the host path, the numbering, the texts, the clusters executable) and lsq_clusters.hip (the device
// passes) share.  The junction rows, the key of an intron and the index are lsq_junc.hpp's.
#pragma once

#include "lsq_junc.hpp"

namespace lsq {
constexpr int CL_PHASES = 8;                   // upload, sort, reduce, filter, links, components, totals, copy-back
constexpr int CL_REPORT = 11;
constexpr uint32_t CL_NONE = 0xFFFFFFFFu;      // no row: the root of a row that is not kept, the totals' slot of a singleton
constexpr size_t CL_MAX_SAMPLES = 65535;
constexpr uint64_t CL_MAX_CELLS = (uint64_t)1 << 31;      // introns x samples
constexpr unsigned CL_CHROM_SHIFT = 48;        // of a pooled record's second word
inline uint64_t cl_rec(uint32_t chrom, uint32_t sample, uint32_t reads) { return ((uint64_t)chrom << CL_CHROM_SHIFT) | ((uint64_t)sample << 32) | reads; }
enum : uint8_t { CL_PRINTED = 0, CL_WEAK_ROW = 1, CL_LONG_ROW = 2, CL_SINGLETON = 3, CL_WEAK_CLUSTER = 4 };
}

// The pooled rows of the samples added so far, in the order they came; what the table needs of the index is copied (the pool
// and its tables outlive the index)
struct lsq_cl_pool {
	std::vector<std::string> chrom_names;
	std::vector<uint32_t> in_chrom;            // the index's distinct introns, ascending in (chromosome index, key)
	std::vector<uint64_t> in_key;
	std::vector<uint8_t> in_ann;
	uint32_t n_samples = 0;
	// a row as the two-word record the device sorts (lsq_sort.hpp), so that the upload is two copies: key = jn_key(start, end),
	// rec = chromosome index << 48 | sample << 32 | reads; the OR and the AND of all of them for the sorts' choice of digits
	std::vector<uint64_t> key, rec;
	uint64_t any[2] = {0, 0}, all[2] = {~(uint64_t)0, ~(uint64_t)0};
};

struct lsq_cl_table {
	std::vector<std::string> chrom_names;
	uint32_t n_samples = 0;
	// per distinct intron, in table order
	std::vector<uint32_t> chrom;
	std::vector<int32_t> start, end;
	std::vector<uint8_t> ann;
	std::vector<uint64_t> reads;
	std::vector<uint32_t> samples, cluster;
	std::vector<uint8_t> status;
	std::vector<uint32_t> counts;              // [introns][samples]
	// the printed rows by (cluster number, table order); per printed cluster and sample the sum of its rows' reads
	std::vector<uint32_t> printed;
	std::vector<uint32_t> totals;              // [printed clusters][samples]
	uint64_t report[lsq::CL_REPORT] = {};
	float ms[lsq::CL_PHASES] = {};
	uint32_t rounds = 0;
};

namespace lsq {

// What either path hands to the finish, rows ascending in (chromosome index, start, end): the distinct introns, the count matrix,
// the filters' verdict per row (CL_PRINTED for a kept row), and the components of the kept rows -- root[j] the smallest row of
// j's component (CL_NONE for a row that is not kept) and, at every row that is its own root, the component's size, its pooled
// reads and, for a component of two rows or more, the slot of its per-sample sums in slot_totals ([slots][samples])
struct ClSolved {
	std::vector<uint32_t> chrom;
	std::vector<uint64_t> key, reads;
	std::vector<uint32_t> samples, counts;
	std::vector<uint8_t> status;
	std::vector<uint32_t> root, comp_size, comp_slot;
	std::vector<uint64_t> comp_reads;
	std::vector<uint32_t> slot_totals;
	void resize(size_t n, size_t n_samples) {
		chrom.resize(n); key.resize(n); reads.resize(n); samples.resize(n); counts.resize(n * n_samples); status.resize(n);
		root.resize(n); comp_size.resize(n); comp_slot.resize(n); comp_reads.resize(n);
	}
};

#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool cl_long(int32_t start, int32_t end, uint32_t max_intron) { return max_intron != 0 && (int64_t)end - start > (int64_t)max_intron; }
// the pool's size against the limits of either path: LSQ_E_RANGE beyond 2^32-1 pooled rows
int cl_check_pool(const lsq_cl_pool &p);
// lsq_clusters.cpp: singletons and weak clusters marked, `ann` looked up, the rows in table order, the clusters numbered, the
// printed rows listed, the report filled from `S` and the pool
int cl_finish_table(const lsq_cl_pool &p, ClSolved &S, uint64_t min_cluster_reads, lsq_cl_table &t);
int run_clusters(int argc, const char *const *argv, std::string &out);       // the clusters executable
// lsq_clusters.hip: the device passes; S comes back in (chromosome index, start, end) order
int cl_device_solve(lsq_ctx *c, const lsq_cl_pool &p, uint64_t min_reads, uint32_t max_intron, ClSolved &S, float ms[CL_PHASES], uint32_t &rounds);

} // namespace lsq
