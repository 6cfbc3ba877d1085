// What the tools that take an annotation and a read file share on the host (lsq_readtool.hpp): the dictionaries of an index, a
// read file through its host parser, a line's exon union and introns, the cells of an interval lookup, the tables' row order,
// and the frame of the junctions, coverage, exonbins, psi, evidence, sites, retention and clusters executables -- arguments, owned handles, the log on failure, the output file.
#include <cerrno>
#include <cstdlib>
#include <numeric>

#include "lsq_readtool.hpp"

using namespace lsq;

char *lsq::dup_text(const std::string &s) {
	char *p = (char *)malloc(s.size() + 1);
	if (p) { memcpy(p, s.data(), s.size()); p[s.size()] = 0; }
	return p;
}

bool lsq::write_file(const char *path, const char *text) {
	FILE *fp = fopen(path, "wb");
	const size_t n = strlen(text);
	const bool ok = fp && fwrite(text, 1, n, fp) == n;
	if ((fp && fclose(fp) != 0) || !ok) { fail(LSQ_E_IO, "cannot write %s", path); return false; }
	return true;
}

// the chromosomes' groups reordered, every group as it is
std::vector<size_t> lsq::rows_by_chrom_name(const std::vector<std::string> &names, const std::vector<uint32_t> &chrom) {
	const size_t n = chrom.size(), nc = names.size();
	std::vector<size_t> first(nc + 1, 0);
	for (size_t i = 0; i < n; ++i) ++first[chrom[i] + 1];
	for (size_t c = 0; c < nc; ++c) first[c + 1] += first[c];
	std::vector<uint32_t> order(nc);
	std::iota(order.begin(), order.end(), 0u);
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
	std::vector<size_t> from;
	from.reserve(n);
	for (uint32_t c : order) for (size_t i = first[c]; i < first[c + 1]; ++i) from.push_back(i);
	return from;
}

int lsq::annotation_dictionaries(const lsq_annotation &a, lsq_events &E, int library) {
	if (library != LSQ_LIBRARY_UNSTRANDED && library != LSQ_LIBRARY_FORWARD && library != LSQ_LIBRARY_REVERSE) return fail(LSQ_E_ARG, "unknown library type %d", library);
	E.library = library;
	E.strand_plus = E.strands.intern("+"); E.strand_minus = E.strands.intern("-");
	for (const auto &rp : a.recs) if (E.chroms.intern(rp->chrom) >= (int)NO_CHROM) return fail(LSQ_E_RANGE, "more than 65 535 chromosomes");
	E.covered.resize(E.table_of(E.chroms.names.size(), 0));
	for (IntervalList &il : E.covered) il.add(-((int64_t)1 << 40), (int64_t)1 << 40);
	return LSQ_OK;
}

int lsq::require_strands(const std::vector<std::string> &names, const std::vector<std::string> &strands, const char *noun, const char *tool) {
	size_t first_bad = names.size(), n_bad = 0;
	for (size_t i = 0; i < names.size(); ++i) if (strands[i] != "+" && strands[i] != "-") { if (!n_bad) first_bad = i; ++n_bad; }
	if (!n_bad) return LSQ_OK;
	return fail(LSQ_E_UNSUPPORTED, "%s %s has no strand of its own (its isoforms do not all carry the same one of + / -): a stranded %s index cannot place it; %zu such %s(s)",
	            noun, names[first_bad].c_str(), tool, n_bad, noun);
}

const char *lsq::library_name(int library) { return library == LSQ_LIBRARY_FORWARD ? "forward" : library == LSQ_LIBRARY_REVERSE ? "reverse" : "unstranded"; }

bool lsq::cli_library_option(int argc, const char *const *argv, int &i, int &library) {
	if (i + 1 >= argc) return false;
	library = lsq_library_from_name(argv[++i]);
	if (library >= 0) return true;
	cli_log(0, (std::string("--library ") + argv[i] + ": the library type is unstranded, forward or reverse").c_str());
	return false;
}
bool lsq::cli_library_env(int &library, bool empty_is_unset) {
	const char *e = getenv("LSQ_LIBRARY");
	if (!e || (!*e && empty_is_unset)) return true;
	library = lsq_library_from_name(e);
	if (library >= 0) return true;
	cli_log(0, (std::string("LSQ_LIBRARY=") + e + ": the library type is unstranded, forward or reverse").c_str());
	return false;
}
void lsq::cli_log_library(const char *tool, int library, const uint64_t *lib) {
	char msg[320];
	snprintf(msg, sizeof msg, "%s: %s library: %llu reads of the + strand, %llu retained; %llu of the - strand, %llu retained; %llu without a strand", tool, library_name(library),
	         (unsigned long long)lib[0], (unsigned long long)lib[3], (unsigned long long)lib[1], (unsigned long long)lib[4], (unsigned long long)lib[2]);
	cli_log(2, msg);
}

int lsq::host_parse_reads(lsq_events *E, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, bool verify, int n_threads, lsq_reads **r) {
	if (strcmp(read_format, "SAM_SINGLE") == 0) return lsq_sam_parse(path, E, skip_flags, min_mapq, n_threads, r);
	if (strcmp(read_format, "BAM_SINGLE") == 0) return verify ? lsq_bam_parse_checked(path, E, skip_flags, min_mapq, n_threads, r) : lsq_bam_parse(path, E, skip_flags, min_mapq, n_threads, r);
	return lsq_reads_parse(read_format, path, E, n_threads, r);
}

int lsq::cli_read_option_env(const std::function<int(int, unsigned long)> &use) {
	const char *names[3] = {"LSQ_SAM_SKIP_FLAGS", "LSQ_SAM_MIN_MAPQ", "LSQ_BAM_VERIFY"};
	for (int k = 0; k < 3; ++k) if (const char *e = getenv(names[k])) {
		char *end = nullptr;
		const unsigned long v = strtoul(e, &end, 0);
		if (end == e || *end) return fail(LSQ_E_ARG, "%s=%s is not a number", names[k], e);
		const int st = use(k, v);
		if (st) return st;
	}
	return LSQ_OK;
}

int lsq::cli_host_parse(lsq_events *E, const char *read_format, const char *path, lsq_reads **r) {
	unsigned long opt[3] = {LSQ_SAM_DEFAULT_SKIP_FLAGS, LSQ_SAM_DEFAULT_MIN_MAPQ, 0};
	const int st = cli_read_option_env([&](int k, unsigned long v) { opt[k] = v; return LSQ_OK; });
	return st ? st : host_parse_reads(E, read_format, path, (unsigned)opt[0], (unsigned)opt[1], opt[2] != 0, 0, r);
}

void lsq::exon_union(const IsoRec &r, std::vector<std::pair<int64_t, int64_t>> &sorted_exons) {
	const size_t ne = std::min<size_t>({(size_t)r.exonCount, r.exonStarts.size(), r.exonEnds.size()}), held = sorted_exons.size();
	for (size_t i = 0; i < ne; ++i) if (r.exonEnds[i] > r.exonStarts[i]) sorted_exons.emplace_back(r.exonStarts[i], r.exonEnds[i]);
	std::sort(sorted_exons.begin() + held, sorted_exons.end());
	std::inplace_merge(sorted_exons.begin(), sorted_exons.begin() + held, sorted_exons.end());
}

void lsq::line_introns(const IsoRec &r, std::vector<std::pair<int64_t, int64_t>> &ex, std::vector<std::pair<int64_t, int64_t>> &introns) {
	constexpr int64_t LIM = (int64_t)1 << 30;
	ex.clear();
	exon_union(r, ex);
	int64_t reach = 0;
	for (size_t i = 0; i < ex.size(); ++i) {
		if (i && ex[i].first > reach && reach > -LIM && ex[i].first < LIM) introns.emplace_back(reach, ex[i].first);
		reach = i ? std::max(reach, ex[i].second) : ex[i].second;
	}
}

// The cells of a lookup over intervals clamped to [-2^30, 2^30] (the exon bins' and the evidence regions'; lsq_readtool.hpp): per
// chromosome the boundaries, the items over every stretch between two of them counted, the stretches with any compacted into
// cells, their lists filled item by item (so they ascend)
int lsq::build_cells(size_t nc, const std::vector<uint32_t> &item_chrom, const std::vector<int32_t> &start, const std::vector<int32_t> &end, std::vector<uint32_t> &chrom_first_cell,
                     std::vector<int32_t> &cell_start, std::vector<int32_t> &cell_end, std::vector<uint32_t> &cell_off, std::vector<uint32_t> &cell_items, const char *too_many) {
	const size_t nb = item_chrom.size();
	std::vector<std::vector<uint32_t>> of_chrom(nc);
	for (size_t b = 0; b < nb; ++b) if (end[b] > start[b]) of_chrom[item_chrom[b]].push_back((uint32_t)b);
	chrom_first_cell.assign(nc + 1, 0);
	cell_off.assign(1, 0);
	std::vector<int32_t> cut;
	std::vector<uint64_t> cnt;
	std::vector<uint32_t> cell_of;
	uint64_t n_entries = 0;
	for (size_t c = 0; c < nc; ++c) {
		const std::vector<uint32_t> &items = of_chrom[c];
		cut.clear();
		for (uint32_t b : items) { cut.push_back(start[b]); cut.push_back(end[b]); }
		std::sort(cut.begin(), cut.end());
		cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
		auto at = [&](int32_t x) { return (size_t)(std::lower_bound(cut.begin(), cut.end(), x) - cut.begin()); };
		cnt.assign(cut.size(), 0);
		for (uint32_t b : items) for (size_t i = at(start[b]), e = at(end[b]); i < e; ++i) ++cnt[i];
		cell_of.assign(cut.size(), 0xFFFFFFFFu);
		for (size_t i = 0; i + 1 < cut.size(); ++i) if (cnt[i]) {
			n_entries += cnt[i];
			if (n_entries > 0xFFFFFFFFull || cell_start.size() >= 0xFFFFFFFEull) return fail(LSQ_E_RANGE, "%s", too_many);
			cell_of[i] = (uint32_t)cell_start.size();
			cell_start.push_back(cut[i]); cell_end.push_back(cut[i + 1]);
			cell_off.push_back((uint32_t)n_entries);
		}
		chrom_first_cell[c + 1] = (uint32_t)cell_start.size();
		cell_items.resize((size_t)n_entries);
		const uint32_t c0 = chrom_first_cell[c];
		std::vector<uint32_t> next(cell_off.begin() + c0, cell_off.begin() + chrom_first_cell[c + 1]);      // every cell's next free place
		for (uint32_t b : items) for (size_t i = at(start[b]), e = at(end[b]); i < e; ++i) cell_items[next[cell_of[i] - c0]++] = b;
	}
	return LSQ_OK;
}

bool lsq::cli_u32_option(int argc, const char *const *argv, int &i, unsigned long &v) {
	char *end = nullptr;
	if (i + 1 >= argc) return false;
	errno = 0;
	v = strtoul(argv[++i], &end, 10);
	return !(end == argv[i] || *end || errno || v > 0xFFFFFFFFul || argv[i][0] == '-');
}

int lsq::cli_failed(int st) {
	cli_log(0, lsq_last_error());
	if (st == LSQ_E_PARSE) cli_log(0, LEXICAL_CAST_ERROR);
	return st == LSQ_E_DEVICE || st == LSQ_E_INTERNAL ? 2 : 1;
}

CliFrame::~CliFrame() {
	free_reads();
	if (c) lsq_ctx_destroy(c);
	lsq_annotation_free(a);
	for (char *t : text) lsq_free(t);
}
int CliFrame::load_annotation() { return lsq_annotation_load(pos[0], pos[1], pos[2], pos[3], 0, (uint64_t)1 << 62, &a); }
int CliFrame::host_parse(lsq_events *E) { return cli_host_parse(E, pos[4], pos[5], &reads); }
void CliFrame::free_reads() { lsq_reads_free(reads); reads = nullptr; }
int CliFrame::create_context() {
	const int st = lsq_ctx_create(cli_device(), &c);
	return st ? st : cli_env_options(c);
}
int CliFrame::deliver(const char *t, std::string &out) const {
	if (pos.size() == 7 && strcmp(pos[6], "-") != 0) return write_file(pos[6], t) ? 0 : cli_failed(LSQ_E_IO);
	out = t;
	return 0;
}
