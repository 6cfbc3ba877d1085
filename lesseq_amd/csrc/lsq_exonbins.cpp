// Reads per exon bin and per gene of a read file (include/lesseq_hip.h, lsq_xb_*): the index made from an annotation,
// the host path over the host parsers' arrays, the tables' text and the exonbins executable.  The device count is
// lsq_exonbins.hip, the entry that opens a read file on the device is lsq_readfile.hip's lsq_xb_device; what the tool shares with
// junctions and coverage is lsq_readtool.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "lsq_exonbins.hpp"

using namespace lsq;

namespace {

inline int32_t clamped(int64_t x) { return (int32_t)std::max<int64_t>(-XB_LIM, std::min<int64_t>(XB_LIM, x)); }

// The bins of one gene from its isoform lines' exons: the stretches between neighbouring boundaries that an exon covers.  The
// union of the exons as maximal intervals decides "covered": a stretch between two neighbouring boundaries lies inside one
// maximal interval or outside all of them.
void gene_bins(const Gene &g, std::vector<std::pair<int64_t, int64_t>> &ex, std::vector<int64_t> &cut, std::vector<int64_t> &bs, std::vector<int64_t> &be) {
	ex.clear(); cut.clear();
	for (const IsoRec *r : g.isos) exon_union(*r, ex);
	for (const auto &x : ex) { cut.push_back(x.first); cut.push_back(x.second); }
	std::sort(cut.begin(), cut.end());
	cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
	size_t q = 0;                               // the boundary the next stretch begins at
	for (size_t i = 0; i < ex.size();) {
		int64_t s = ex[i].first, e = ex[i].second;
		for (++i; i < ex.size() && ex[i].first <= e; ++i) e = std::max(e, ex[i].second);
		while (cut[q] < s) ++q;                 // (s and e are boundaries themselves)
		for (; cut[q] < e; ++q) { bs.push_back(cut[q]); be.push_back(cut[q + 1]); }
	}
}

// the first cell of chromosome (stranded index: table) c that ends behind s (chrom_first_cell[c + 1]: none)
inline uint32_t first_cell(const lsq_xb_index &ix, size_t c, int32_t s) {
	uint32_t lo = ix.chrom_first_cell[c], hi = ix.chrom_first_cell[c + 1];
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (ix.cell_end[mid] <= s) lo = mid + 1; else hi = mid;
	}
	return lo;
}

} // namespace

void lsq::xb_start_table(const lsq_xb_index &ix, lsq_xb_table &t) {
	t.gene_name = ix.gene_name; t.gene_first_bin = ix.gene_first_bin;
	t.reads.assign(ix.bin_gene.size(), 0); t.total.assign(ix.gene_name.size(), 0);
	t.library = ix.E.library;
	for (uint64_t &v : t.report) v = 0;
	for (uint64_t &v : t.lib) v = 0;
	for (float &m : t.ms) m = 0;
}

// A thread a stretch of reads, counters of its own: the bins of every cell a block's walk meets are listed per read, sorted and
// made distinct (a read counts once a bin), the genes are the distinct bin_gene of that list (bins are gene-major: they ascend).
// Under a stranded index a read looks in the tables of its transcript strand t alone; one without t is skipped
// behind the tallies of its blocks.
int lsq::xb_host_reads(const lsq_xb_index &ix, const ParsedReads &R, int n_threads, lsq_xb_table &t) {
	const int T = read_slices(R.n_reads, n_threads);
	const size_t nb = ix.bin_gene.size(), ng = ix.gene_name.size(), nc = ix.E.n_table_chroms();
	const bool stranded = ix.E.stranded();
	xb_start_table(ix, t);
	std::vector<std::vector<uint64_t>> part((size_t)T);
	constexpr int NT = 4 + LIB_REPORT;
	std::vector<uint64_t> tally((size_t)T * NT, 0);      // blocks without chromosome or empty, reads on no gene, on several, bin hits; the library report
	const int rc = for_read_slices(R.n_reads, T, [&](int k, uint64_t r0, uint64_t r1) {
		std::vector<uint64_t> &cnt = part[(size_t)k];
		cnt.assign(nb + ng, 0);
		uint64_t *n = &tally[(size_t)k * NT];
		std::vector<uint32_t> hit;
		for (uint64_t r = r0; r < r1; ++r) {
			hit.clear();
			const unsigned tr = !stranded ? 0u : R.blk_off[r] < R.blk_off[r + 1] ? read_transcript(ix.E, R.bst[R.blk_off[r]]) : 2u;
			for (uint64_t b = R.blk_off[r]; b < R.blk_off[r + 1]; ++b) {
				const unsigned c = R.bc[b];
				const int32_t s = R.bs[b], e = R.be[b];
				if (c == NO_CHROM || c >= nc || e <= s) { ++n[0]; continue; }
				if (tr == 2u) continue;
				const size_t tb = ix.E.table_of(c, tr);
				for (uint32_t i = first_cell(ix, tb, s); i < ix.chrom_first_cell[tb + 1] && ix.cell_start[i] < e; ++i)
					hit.insert(hit.end(), ix.cell_bins.begin() + ix.cell_off[i], ix.cell_bins.begin() + ix.cell_off[i + 1]);
			}
			if (stranded) lib_note(n + 4, tr, !hit.empty());
			if (tr == 2u) continue;
			std::sort(hit.begin(), hit.end());
			hit.erase(std::unique(hit.begin(), hit.end()), hit.end());
			uint32_t genes = 0, last = XB_NONE;
			for (uint32_t b : hit) {
				++cnt[b];
				if (ix.bin_gene[b] != last) { last = ix.bin_gene[b]; ++cnt[nb + last]; ++genes; }
			}
			n[3] += hit.size();
			if (genes == 0) ++n[1];
			if (genes > 1) ++n[2];
		}
	});
	if (rc) return rc;
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks;
	for (int k = 0; k < T; ++k) {
		for (size_t b = 0; b < nb; ++b) t.reads[b] += part[(size_t)k][b];
		for (size_t g = 0; g < ng; ++g) t.total[g] += part[(size_t)k][nb + g];
		for (int q = 0; q < 4; ++q) t.report[2 + q] += tally[(size_t)k * NT + q];
		for (int q = 0; q < LIB_REPORT; ++q) t.lib[q] += tally[(size_t)k * NT + 4 + q];
	}
	return LSQ_OK;
}

extern "C" {

int lsq_xb_index_build(const lsq_annotation *a, lsq_xb_index **out) { return lsq_xb_index_build_library(a, LSQ_LIBRARY_UNSTRANDED, out); }

int lsq_xb_index_build_library(const lsq_annotation *a, int library, lsq_xb_index **out) LSQ_API_TRY {
	if (!a || !out) return fail(LSQ_E_ARG, "null argument");
	std::unique_ptr<lsq_xb_index> ix(new lsq_xb_index);
	int rc;
	if ((rc = annotation_dictionaries(*a, ix->E, library))) return rc;
	std::vector<std::pair<int64_t, int64_t>> ex;
	std::vector<int64_t> cut;
	ix->gene_first_bin.push_back(0);
	for (const Gene &g : a->selected) {
		uint32_t chrom = XB_NONE;
		std::string strand = g.isos.empty() ? "." : g.isos[0]->strand;
		for (const IsoRec *r : g.isos) {
			const uint32_t c = (uint32_t)ix->E.chroms.find(r->chrom);
			if (chrom != XB_NONE && c != chrom)
				return fail(LSQ_E_UNSUPPORTED, "gene %s has isoforms on more than one chromosome (%s and %s): it has no exon bins", g.name.c_str(), ix->E.chroms.names[chrom].c_str(), r->chrom.c_str());
			chrom = c;
			if (r->strand != strand) strand = ".";
		}
		gene_bins(g, ex, cut, ix->bin_start, ix->bin_end);
		if (ix->bin_start.size() > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32-1 exon bins");
		ix->bin_gene.resize(ix->bin_start.size(), (uint32_t)ix->gene_name.size());
		ix->gene_name.push_back(g.name); ix->gene_strand.push_back(strand); ix->gene_chrom.push_back(chrom);
		ix->gene_first_bin.push_back((uint32_t)ix->bin_start.size());
	}
	if (ix->E.stranded() && (rc = require_strands(ix->gene_name, ix->gene_strand, "gene", "exonbins"))) return rc;
	const size_t nb = ix->bin_start.size();
	ix->c_bin_start.resize(nb); ix->c_bin_end.resize(nb);
	for (size_t b = 0; b < nb; ++b) { ix->c_bin_start[b] = clamped(ix->bin_start[b]); ix->c_bin_end[b] = clamped(ix->bin_end[b]); }
	std::vector<uint32_t> bin_chrom(nb);
	for (size_t b = 0; b < nb; ++b) {          // (a stranded index: the bin's table id; a gene with bins has a chromosome)
		const uint32_t g = ix->bin_gene[b];
		bin_chrom[b] = (uint32_t)ix->E.table_of(ix->gene_chrom[g], ix->gene_strand[g] == "-" ? 1u : 0u);
	}
	if ((rc = build_cells(ix->E.covered.size(), bin_chrom, ix->c_bin_start, ix->c_bin_end, ix->chrom_first_cell, ix->cell_start, ix->cell_end, ix->cell_off, ix->cell_bins,
	                      "more than 2^32-1 entries in the bin lookup (overlapping genes)"))) return rc;
	*out = ix.release();
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_xb_index_free(lsq_xb_index *ix) { delete ix; }
int lsq_xb_index_library(const lsq_xb_index *ix) { return index_library(ix); }
int64_t lsq_xb_index_num_chroms(const lsq_xb_index *ix) { return index_num_chroms(ix); }
int64_t lsq_xb_index_num_genes(const lsq_xb_index *ix) { return ix ? (int64_t)ix->gene_name.size() : 0; }
int64_t lsq_xb_index_num_bins(const lsq_xb_index *ix) { return ix ? (int64_t)ix->bin_gene.size() : 0; }
const char *lsq_xb_index_chrom_name(const lsq_xb_index *ix, int64_t chrom) { return index_chrom_name(ix, chrom); }
const char *lsq_xb_index_gene_name(const lsq_xb_index *ix, int64_t gene) {
	return ix && gene >= 0 && (size_t)gene < ix->gene_name.size() ? ix->gene_name[(size_t)gene].c_str() : nullptr;
}
const char *lsq_xb_index_gene_strand(const lsq_xb_index *ix, int64_t gene) {
	return ix && gene >= 0 && (size_t)gene < ix->gene_strand.size() ? ix->gene_strand[(size_t)gene].c_str() : nullptr;
}
lsq_events *lsq_xb_index_dictionaries(lsq_xb_index *ix) { return index_dictionaries(ix); }
int lsq_xb_index_arrays(const lsq_xb_index *ix, const int64_t **bin_start, const int64_t **bin_end, const uint32_t **bin_gene, const uint32_t **gene_first_bin, const uint32_t **gene_chrom) {
	if (!ix) return fail(LSQ_E_ARG, "null argument");
	if (bin_start) *bin_start = ix->bin_start.data();
	if (bin_end) *bin_end = ix->bin_end.data();
	if (bin_gene) *bin_gene = ix->bin_gene.data();
	if (gene_first_bin) *gene_first_bin = ix->gene_first_bin.data();
	if (gene_chrom) *gene_chrom = ix->gene_chrom.data();
	return LSQ_OK;
}

int lsq_xb_host_reads(lsq_xb_index *ix, const lsq_reads *r, int n_threads, lsq_xb_table **out) LSQ_API_TRY {
	if (!ix || !r || !out) return fail(LSQ_E_ARG, "null argument");
	return new_table(out, [&](lsq_xb_table &t) { return xb_host_reads(*ix, host_view(*r), n_threads, t); });
} LSQ_API_CATCH

int lsq_xb_host(lsq_xb_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, int n_threads, lsq_xb_table **out) LSQ_API_TRY {
	if (!ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	return host_file(ix->E, read_format, path, skip_flags, min_mapq, n_threads, [&](const lsq_reads *r) { return lsq_xb_host_reads(ix, r, n_threads, out); });
} LSQ_API_CATCH

void lsq_xb_table_free(lsq_xb_table *t) { delete t; }
int lsq_xb_table_arrays(const lsq_xb_table *t, const uint64_t **reads, const uint64_t **total) {
	if (!t) return fail(LSQ_E_ARG, "null argument");
	if (reads) *reads = t->reads.data();
	if (total) *total = t->total.data();
	return LSQ_OK;
}
int lsq_xb_table_report(const lsq_xb_table *t, uint64_t report[6]) { return table_report(t, report); }
int lsq_xb_table_library_report(const lsq_xb_table *t, uint64_t report[5]) { return table_library_report(t, report); }
int lsq_xb_table_times(const lsq_xb_table *t, float ms[3]) { return table_times(t, ms); }

int lsq_xb_format(const lsq_xb_table *t, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	char buf[96];
	for (size_t g = 0; g < t->gene_name.size(); ++g)
		for (uint32_t b = t->gene_first_bin[g]; b < t->gene_first_bin[g + 1]; ++b) {
			o += t->gene_name[g];
			snprintf(buf, sizeof buf, "\t%llu\t", (unsigned long long)t->total[g]);
			o += buf; o += t->gene_name[g];
			snprintf(buf, sizeof buf, ":%u\t%llu\n", b - t->gene_first_bin[g] + 1u, (unsigned long long)t->reads[b]);
			o += buf;
		}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

int lsq_xb_format_bins(const lsq_xb_index *ix, char **interval_text, char **map_text) LSQ_API_TRY {
	if (!ix || !interval_text || !map_text) return fail(LSQ_E_ARG, "null argument");
	std::string iv, mp;
	char buf[160];
	for (size_t g = 0; g < ix->gene_name.size(); ++g)
		for (uint32_t b = ix->gene_first_bin[g]; b < ix->gene_first_bin[g + 1]; ++b) {
			snprintf(buf, sizeof buf, ":%u", b - ix->gene_first_bin[g] + 1u);
			const std::string id = ix->gene_name[g] + buf;
			const long long s = (long long)ix->bin_start[b], e = (long long)ix->bin_end[b];
			iv += id; iv += '\t'; iv += ix->E.chroms.names[ix->gene_chrom[g]]; iv += '\t'; iv += ix->gene_strand[g];
			snprintf(buf, sizeof buf, "\t%lld\t%lld\t1\t%lld\t%lld\n", s, e, s, e);
			iv += buf;
			mp += ix->gene_name[g]; mp += '\t'; mp += id; mp += '\n';
		}
	*interval_text = dup_text(iv);
	*map_text = dup_text(mp);
	if (!*interval_text || !*map_text) { free(*interval_text); free(*map_text); *interval_text = *map_text = nullptr; return fail(LSQ_E_INTERNAL, "out of memory"); }
	return LSQ_OK;
} LSQ_API_CATCH

} // extern "C"

// exonbins [--host] [--bins <prefix>] [--library unstranded|forward|reverse] <isoform_format> <isoforms_path> <g2i_format> <g2i_path> <read_format> <reads_path> [<out>]
// The table on standard output (or in <out>; "-": standard output), the bins as an annotation in <prefix>.interval and
// <prefix>.map, the report in the log.  Without --library the library type is LSQ_LIBRARY's (unstranded without either); a
// stranded run logs its library report behind the report.  Exit status 1, nothing on standard output and no file, for a gene on two chromosomes
// and for a file that does not open or parse.
int lsq::run_exonbins(int argc, const char *const *argv, std::string &out) {
	static const char *USAGE = "Usage:\nexonbins [--host] [--bins prefix] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]";
	bool host = false, bad = false, lib_given = false;
	int library = LSQ_LIBRARY_UNSTRANDED;
	const char *prefix = nullptr;
	std::vector<const char *> pos;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (strcmp(argv[i], "--bins") == 0) {
			if (i + 1 < argc) prefix = argv[++i]; else bad = true;
		} else if (strcmp(argv[i], "--library") == 0) {
			if (i + 1 >= argc) bad = true;
			else if (!cli_library_option(argc, argv, i, library)) return 1;
			lib_given = true;
		} else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else pos.push_back(argv[i]);
	}
	if (bad || pos.size() < 6 || pos.size() > 7) { cli_log(0, USAGE); return 1; }
	if (!lib_given && !cli_library_env(library)) return 1;
	CliFrame F(pos);                                       // text[0] the table, text[1] and text[2] the bins' two files
	CliOwned<lsq_xb_index, lsq_xb_index_free> ix;
	CliOwned<lsq_xb_table, lsq_xb_table_free> t;
	int st = F.load_annotation();
	if (!st) st = lsq_xb_index_build_library(F.a, library, &ix.p);
	if (st) return cli_failed(st);
	if (host) {
		if (!(st = F.host_parse(&ix.p->E))) st = lsq_xb_host_reads(ix.p, F.reads, 0, &t.p);
		F.free_reads();
	} else if (!(st = F.create_context())) st = lsq_xb_device(F.c, ix.p, pos[4], pos[5], &t.p);
	if (!st) st = lsq_xb_format(t.p, &F.text[0]);
	if (!st && prefix) st = lsq_xb_format_bins(ix.p, &F.text[1], &F.text[2]);
	if (st) return cli_failed(st);
	const uint64_t *rep = t.p->report;
	char msg[384];
	snprintf(msg, sizeof msg, "exonbins: %llu read(s), %llu block(s), %llu without a chromosome of the annotation or empty; %lld bin(s) of %lld gene(s): %llu read(s) on no gene, %llu on more than one, %llu bin hit(s)",
	         (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2], (long long)lsq_xb_index_num_bins(ix.p), (long long)lsq_xb_index_num_genes(ix.p),
	         (unsigned long long)rep[3], (unsigned long long)rep[4], (unsigned long long)rep[5]);
	cli_log(2, msg);
	if (library != LSQ_LIBRARY_UNSTRANDED) cli_log_library("exonbins", library, t.p->lib);
	if (prefix && (!write_file((std::string(prefix) + ".interval").c_str(), F.text[1]) || !write_file((std::string(prefix) + ".map").c_str(), F.text[2]))) return cli_failed(LSQ_E_IO);
	return F.deliver(F.text[0], out);
}
