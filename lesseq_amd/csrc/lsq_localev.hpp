// Local events of bin/Events.r (step 2 of the pipeline): the packed splicing graphs and the detected records, shared by
// the host side (lsq_localev.cpp: readers, formatter, the events executable) and the kernels (lsq_localev.hip).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "lsq_internal.hpp"

namespace lsq {

constexpr int LE_TYPES = 8;                      // ES RI A5SS A3SS MXE AFE ALE T3 (Events.r's output order)
enum { LE_ES, LE_RI, LE_A5SS, LE_A3SS, LE_MXE, LE_AFE, LE_ALE, LE_T3 };
enum { LE_PLUS = 0, LE_MINUS = 1, LE_OTHER = 2 };

// One record: gene index (low 32 bits) and, above it, the 1-based column i of ES / RI / A5SS / A3SS / MXE, or the block
// of AFE / ALE (0: first-exon block, Events.r:109-124; 1: last-exon block, :126-141) and of T3 (0: the + form, :143-149;
// 1: the - form, :150-156).
inline uint64_t le_record(uint32_t gene, uint32_t code) { return (uint64_t)code << 32 | gene; }

int run_events(int argc, const char *const *argv, std::string &out);      // the events executable

} // namespace lsq

// Genes in Events.r's order (select, :40-42).  Gene g has N columns and K isoform rows; for N >= 3 its 2N coordinates
// (the digit runs of the header, :53) are pos[pos_off[g] .. pos_off[g] + 2N) and column n's membership bits are
// bits[bit_off[g] + n * W .. + W), W = ceil(K / 64), isoform r at bit r % 64 of word r / 64, the bits above K zero.
// A gene with N < 3 is printed and skipped (:57); it holds no coordinates and no bits.
struct lsq_le_graphs {
	std::vector<std::string> names, chrom, strand;
	std::vector<int32_t> strand_code, N, K;
	std::vector<uint64_t> pos_off, bit_off;      // G + 1 each
	std::vector<int32_t> pos;
	std::vector<uint64_t> bits;
	size_t size() const { return names.size(); }
	void add_gene(const std::string &name, const std::string &ch, const std::string &st, int n, int k);
};

// Records per type in Events.r's order (genes in order, then the script's loop order); the counter of record q of a
// type is q + 1.  Formatting reads the graphs, which must outlive the result.
struct lsq_le_result {
	const lsq_le_graphs *g = nullptr;
	std::vector<uint64_t> rec[lsq::LE_TYPES];
	double ms[4] = {0, 0, 0, 0};                 // HIP-event times: upload, count kernel + scan, emit kernel, download
};
