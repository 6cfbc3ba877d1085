// Annotation from GTF (bin/parseGencode, bin/gencodeIsoformMap): what the kernels (lsq_gtf.hip) and the host side
// (lsq_gtf.cpp: assembly of the transcripts, formatter, the two executables) share.  DESIGN.md 4.8 holds the rules.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "lsq_internal.hpp"

namespace lsq {

// One `exon` line, as the device hands it over.  Offsets count from the line's first byte (the chromosome starts at 0).
// aux: in the compacted array 1 where (gene id, transcript id) differs bytewise from the kept line before it; in the array
// of run heads the index of the line among the kept lines.  On a line with an unquoted id (GTF_E_UNQUOTED_*) gene_off /
// gene_len bound the offending item instead.
struct GtfRec {
	uint64_t line_off;
	uint32_t line_no;                // 1-based
	uint32_t chrom_len;
	uint32_t strand_off, strand_len;
	uint32_t gene_off, gene_len;
	uint32_t tx_off, tx_len;
	int32_t start, end;              // field 4 minus 1, field 5 (atoi into 32 bits)
	uint32_t aux;
	uint32_t pad;
};
static_assert(sizeof(GtfRec) == 56, "GtfRec is copied from the device verbatim");

// the error word: line index (0-based) << 8 | kind; the smallest word is the first failing line
enum { GTF_E_SHORT = 1, GTF_E_NO_GENE = 2, GTF_E_UNQUOTED_GENE = 3, GTF_E_NO_TX = 4, GTF_E_UNQUOTED_TX = 5 };
constexpr uint64_t GTF_NO_ERR = ~0ull;

struct GtfTranscript {
	std::string name;                // <gene_id>|<transcript_id>
	size_t gene_len = 0;             // bytes of the gene id in it
	std::string chrom, strand;
	std::vector<int32_t> starts, ends;      // each sorted on its own
};

// the kept lines of a text as the device returned them -> transcripts in output order (host: O(runs log runs + exons))
int gtf_assemble(const unsigned char *text, const GtfRec *heads, size_t n_heads, const int32_t *se /* [n_kept][2] */, size_t n_kept,
                 std::vector<GtfTranscript> &out, uint64_t &n_genes);
int run_parse_gencode(int argc, const char *const *argv, std::string &out);        // the parseGencode executable
int run_isoform_map(int argc, const char *const *argv, std::string &out);          // the gencodeIsoformMap executable
int read_all(const char *path /* null: standard input */, std::string &bytes);

} // namespace lsq

struct lsq_gtf {
	std::vector<lsq::GtfTranscript> tx;     // output order: gene id, then transcript id, bytewise
	uint64_t n_genes = 0, n_lines = 0, n_kept = 0, n_skipped = 0;
	double ms[4] = {0, 0, 0, 0};            // HIP-event times: copy, newline scan, parse kernels, download
};
