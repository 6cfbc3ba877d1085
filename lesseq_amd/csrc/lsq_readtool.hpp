// What the tools that take an annotation and a read file share on the host (junctions, coverage, exonbins, psi, evidence, sites, retention):
// the view of parsed reads their passes take, the dictionaries a read file is parsed against without events, a line's exon
// union and its introns, the split of the reads over host threads, the entry points that differ by the index's or the table's type alone, and
// the frame of their executables, whose owned handles (CliOwned), library type and read options of the environment count, solve,
// classify and bamcheck take too (lsq_cli.cpp, lsq_cli_job.cpp).  lsq_readtool.cpp defines what is no template.
#pragma once

#include <algorithm>
#include <cstring>
#include <functional>
#include <utility>

#include "lsq_internal.hpp"

namespace lsq {

// parsed reads in file order (lsq_reads' arrays), on the host or on the device
struct ParsedReads {
	uint64_t n_reads, n_blocks;
	const unsigned long long *blk_off;
	const int32_t *bs, *be;
	const uint16_t *bc;
	const uint8_t *bst;
};
constexpr unsigned NO_CHROM = 0xFFFFu;         // bc of a block on no chromosome of the dictionaries
inline ParsedReads host_view(const lsq_reads &r) {
	return ParsedReads{r.n_reads, r.n_blocks, (const unsigned long long *)r.blk_off, r.blk_start, r.blk_end, r.blk_chrom, r.blk_strand};
}

// The dictionaries a read file is parsed against without events (an index's `lsq_events E`): "+" and "-" as strands 0 and 1, the
// distinct chromosome strings of the annotation's isoform lines in file order, one whole-line interval a chromosome.
// A library type other than unstranded makes them a stranded job's dictionaries (lsq_events::library): the parsers
// deliver the strand of a fragment's first mate as the strand id, and `covered` holds a whole-line interval per TABLE id
// 2 * chromosome + (strand == "-"), so n_table_chroms() stays the number of chromosomes.
int annotation_dictionaries(const lsq_annotation &a, lsq_events &E, int library = LSQ_LIBRARY_UNSTRANDED);
// A stranded index needs a strand of its own for every gene or event (strands[i]: "+", "-", or anything else where the isoform
// lines differ or carry neither): LSQ_E_UNSUPPORTED naming the first that has none and how many there are
int require_strands(const std::vector<std::string> &names, const std::vector<std::string> &strands, const char *noun, const char *tool);
// a stranded table's library report: reads with t = +, with t = -, without t; of the first two, those that counted for a gene or event
constexpr int LIB_REPORT = 5;
// The transcript strand of a read under an index's dictionaries from the strand id of its first block: 0 plus,
// 1 minus, 2 none (the strand string is neither "+" nor "-")
inline unsigned read_transcript(const lsq_events &E, unsigned strand_id) {
	return strand_id == (unsigned)E.strand_plus ? E.transcript_minus(false, false) : strand_id == (unsigned)E.strand_minus ? E.transcript_minus(true, false) : 2u;
}
// what a host thread notes of one read (t: 0, 1, or 2 for none) in its LIB_REPORT tallies
inline void lib_note(uint64_t *lib, unsigned t, bool counted) { ++lib[t]; if (t < 2u && counted) ++lib[3 + t]; }
const char *library_name(int library);         // "unstranded", "forward", "reverse"
// --library of an executable: the value behind argv[i] (i moves on to it); where the option is not given, LSQ_LIBRARY of the
// environment (unset or empty: `library` stays).  false, with the message logged, for anything but unstranded, forward or reverse
bool cli_library_option(int argc, const char *const *argv, int &i, int &library);
// (count and solve, which have no --library, take an LSQ_LIBRARY that is set and empty for a wrong name: empty_is_unset false)
bool cli_library_env(int &library, bool empty_is_unset = true);
// the library report of a stranded table as the executables log it
void cli_log_library(const char *tool, int library, const uint64_t *lib);
// A read file through the host parser of its format, against dictionaries E; verify: a BAM file's CRC32s and end-of-file marker checked
int host_parse_reads(lsq_events *E, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, bool verify, int n_threads, lsq_reads **r);
// The one parse of LSQ_SAM_SKIP_FLAGS, LSQ_SAM_MIN_MAPQ and LSQ_BAM_VERIFY of the environment (k = 0, 1, 2; as strtoul reads them in
// base 0): use(k, value) for every one that is set, in this order; a value that is no number (LSQ_E_ARG) or a status of use ends it.
// A variable that is not set is the caller's default.
int cli_read_option_env(const std::function<int(int, unsigned long)> &use);
// ... over the host parsers' defaults (LSQ_SAM_DEFAULT_*, no verification): the executables' --host
int cli_host_parse(lsq_events *E, const char *read_format, const char *path, lsq_reads **r);
int cli_env_options(lsq_ctx *c);               // lsq_cli.cpp: ... as options of a context, which keeps its own defaults; then LSQ_OPTIONS
// rows ascending in chromosome index -> where each row of the tables' order (chromosome names bytewise) comes from
std::vector<size_t> rows_by_chrom_name(const std::vector<std::string> &names, const std::vector<uint32_t> &chrom);
// The exons of a line that are not empty (no more than exonCount of them) merged into `sorted_exons` (empty, or other lines'
// exons in order): the exon union is what a walk with a running maximum of the ends makes of the list
void exon_union(const IsoRec &r, std::vector<std::pair<int64_t, int64_t>> &sorted_exons);
// The introns of a line appended to `introns`, ascending: the gaps between the maximal intervals of its exon union (`ex`: the
// union, scratch), each as (end of the left interval, start of the right one); a gap with an end outside (-2^30, 2^30) -- where no
// block with a chromosome reaches -- is left out
void line_introns(const IsoRec &r, std::vector<std::pair<int64_t, int64_t>> &ex, std::vector<std::pair<int64_t, int64_t>> &introns);
// The cells of a lookup over items with an interval each, clamped to [-2^30, 2^30], item b on chromosome item_chrom[b] (an item with
// end <= start is in no cell): every chromosome cut at every item boundary, the stretches that at least one item covers as cells,
// ascending and disjoint -- chromosome c's are chrom_first_cell[c] .. chrom_first_cell[c + 1] -- and the items that cover cell i,
// ascending, as cell_items[cell_off[i] .. cell_off[i + 1]].  An item covers every cell between its start and its end.
// LSQ_E_RANGE with the text `too_many` beyond 2^32-1 list entries.
int build_cells(size_t n_chroms, const std::vector<uint32_t> &item_chrom, const std::vector<int32_t> &start, const std::vector<int32_t> &end, std::vector<uint32_t> &chrom_first_cell,
                std::vector<int32_t> &cell_start, std::vector<int32_t> &cell_end, std::vector<uint32_t> &cell_off, std::vector<uint32_t> &cell_items, const char *too_many);
bool write_file(const char *path, const char *text);       // false: the status and text of the failure are set (LSQ_E_IO)

// ---- the reads over host threads: T slices of whole reads, one slice below 2^16 reads; f(k, r0, r1) on a thread of its own
inline int read_slices(uint64_t n_reads, int n_threads) { return n_reads < (1u << 16) ? 1 : host_threads(n_threads); }
template <class F>
int for_read_slices(uint64_t n_reads, int T, F f) {
	ThreadGroup th;
	for (int k = 0; k < T; ++k) th.spawn([=] { f(k, n_reads * (uint64_t)k / (uint64_t)T, n_reads * (uint64_t)(k + 1) / (uint64_t)T); });
	th.join();
	return th.failed() ? fail(LSQ_E_INTERNAL, "%s", th.error().c_str()) : LSQ_OK;
}
// the slices' parts, each sorted and folded (fold: sorted items with equal keys -> one each), merged into one such list
template <class X, class Less, class Fold>
std::vector<X> merge_folded(std::vector<std::vector<X>> &parts, Less less, Fold fold) {
	std::vector<X> all = std::move(parts[0]);
	for (size_t k = 1; k < parts.size(); ++k) {
		std::vector<X> m(all.size() + parts[k].size());
		std::merge(all.begin(), all.end(), parts[k].begin(), parts[k].end(), m.begin(), less);
		fold(m);
		all.swap(m);
		std::vector<X>().swap(parts[k]);
	}
	return all;
}

// ---- the bodies of the entry points that differ by the type alone (every index begins with `lsq_events E`)
template <class IX> int64_t index_num_chroms(const IX *ix) { return ix ? (int64_t)ix->E.n_table_chroms() : 0; }
template <class IX> const char *index_chrom_name(const IX *ix, int64_t chrom) {
	return ix && chrom >= 0 && (size_t)chrom < ix->E.n_table_chroms() ? ix->E.chroms.names[(size_t)chrom].c_str() : nullptr;
}
template <class IX> int index_library(const IX *ix) { return ix ? ix->E.library : LSQ_LIBRARY_UNSTRANDED; }
// the library report of a table (its `lib`, under its index's `library`): all zeros and LSQ_E_STATE for an unstranded one
template <class T> int table_library_report(const T *t, uint64_t *report) {
	if (!t || !report) return fail(LSQ_E_ARG, "null argument");
	memcpy(report, t->lib, sizeof(t->lib));
	return t->library != LSQ_LIBRARY_UNSTRANDED ? LSQ_OK : fail(LSQ_E_STATE, "the table is unstranded: there is no library report");
}
template <class IX> lsq_events *index_dictionaries(IX *ix) { return ix ? &ix->E : nullptr; }
template <class T> int table_report(const T *t, uint64_t *report) {
	if (!t || !report) return fail(LSQ_E_ARG, "null argument");
	memcpy(report, t->report, sizeof(t->report));
	return LSQ_OK;
}
template <class T> int table_times(const T *t, float *ms) {
	if (!t || !ms) return fail(LSQ_E_ARG, "null argument");
	memcpy(ms, t->ms, sizeof(t->ms));
	return LSQ_OK;
}
// a new table filled by fill(table), handed out when that succeeds
template <class T, class F> int new_table(T **out, F fill) {
	std::unique_ptr<T> t(new T);
	const int rc = fill(*t);
	if (rc) return rc;
	*out = t.release();
	return LSQ_OK;
}
// lsq_*_host: the file parsed on the host, the arrays through the tool's lsq_*_host_reads, the arrays freed
template <class F> int host_file(lsq_events &E, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, int n_threads, F host_reads) {
	lsq_reads *r = nullptr;
	int rc = host_parse_reads(&E, read_format, path, skip_flags, min_mapq, false, n_threads, &r);
	if (rc) return rc;
	rc = host_reads(r);
	lsq_reads_free(r);
	return rc;
}

// ---- the frame of the executables: <isoform_format> <isoforms_path> <g2i_format> <g2i_path> <read_format> <reads_path> [<out>]
// The value behind a number option argv[i]: decimal, at most 2^32-1, nothing before or behind it; i moves on to it
bool cli_u32_option(int argc, const char *const *argv, int &i, unsigned long &v);
// the last error to the log; the exit status of a failure: 2 for LSQ_E_DEVICE and LSQ_E_INTERNAL, else 1
int cli_failed(int st);
template <class T, void (*FREE)(T *)> struct CliOwned {
	T *p = nullptr;
	CliOwned() = default;
	CliOwned(const CliOwned &) = delete;
	CliOwned &operator=(const CliOwned &) = delete;
	~CliOwned() { FREE(p); }
};
struct CliFrame {
	const std::vector<const char *> &pos;      // the positional arguments: six or seven
	lsq_annotation *a = nullptr;
	lsq_ctx *c = nullptr;
	lsq_reads *reads = nullptr;
	char *text[3] = {nullptr, nullptr, nullptr};       // the tool's output texts
	explicit CliFrame(const std::vector<const char *> &p) : pos(p) {}
	CliFrame(const CliFrame &) = delete;
	CliFrame &operator=(const CliFrame &) = delete;
	~CliFrame();
	int load_annotation();                     // pos[0..3] -> a
	int host_parse(lsq_events *E);             // --host: pos[4], pos[5] -> reads (cli_host_parse)
	void free_reads();
	int create_context();                      // c on cli_device(), under cli_env_options
	int deliver(const char *t, std::string &out) const;       // t into pos[6], or into `out` without one or with "-"; the exit status
};

} // namespace lsq
