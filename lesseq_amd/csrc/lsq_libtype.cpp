// Which library type is this read file? (include/lesseq_hip.h, lsq_lt_*): the index made from an annotation -- per
// chromosome and strand the union of the exons of that strand's genes --, the host path over the host parsers' arrays, the
// derived values with the verdict, the text and the libtype executable.  The device count is lsq_libtype.hip, the entry that
// opens a read file on the device is lsq_readfile.hip's lsq_lt_device.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "lsq_libtype.hpp"

using namespace lsq;

namespace {

inline int32_t clamped(int64_t x) { return (int32_t)std::max<int64_t>(-LT_LIM, std::min<int64_t>(LT_LIM, x)); }

// whether [s, e) shares a base with table tb's union: the first interval that ends behind s hits iff it starts before e
inline bool meets(const lsq_lt_index &ix, size_t tb, int32_t s, int32_t e) {
	uint32_t lo = ix.tab_first[tb], hi = ix.tab_first[tb + 1];
	const uint32_t end = hi;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (ix.iv_end[mid] <= s) lo = mid + 1; else hi = mid;
	}
	return lo < end && ix.iv_start[lo] < e;
}

// sense, antisense, ambiguous, no_gene of the eight classes
struct Derived { uint64_t sense, antisense, ambiguous, no_gene; };
Derived derived_of(const lsq_lt_table &t) {
	const uint64_t *c = t.cls;
	return Derived{c[lt_class(0, true, false)] + c[lt_class(1, false, true)], c[lt_class(0, false, true)] + c[lt_class(1, true, false)],
	               c[lt_class(0, true, true)] + c[lt_class(1, true, true)], c[lt_class(0, false, false)] + c[lt_class(1, false, false)]};
}
// The conventions of how_are_we_stranded_here / RSeQC's infer_experiment users: fewer than 100 informative reads decide nothing;
// at least 0.9 of them sense: forward; at most 0.1: reverse; 0.4 .. 0.6: unstranded; anything between: undetermined
const char *verdict_of(uint64_t sense, uint64_t antisense) {
	const uint64_t n = sense + antisense;
	if (n < 100) return "undetermined";
	const double f = (double)sense / (double)n;
	return f >= 0.9 ? "forward" : f <= 0.1 ? "reverse" : (f >= 0.4 && f <= 0.6) ? "unstranded" : "undetermined";
}

} // namespace

// A thread a stretch of reads, tallies of its own: per read r from the strand id of its first block, then every block that lies
// on a chromosome and is not empty against the two unions of its chromosome, a strand no longer once it has hit
int lsq::lt_host_reads(const lsq_lt_index &ix, const ParsedReads &R, int n_threads, lsq_lt_table &t) {
	const int T = read_slices(R.n_reads, n_threads);
	const size_t nc = ix.E.n_table_chroms();
	std::vector<uint64_t> tally((size_t)T * LT_CLASSES, 0);
	const int rc = for_read_slices(R.n_reads, T, [&](int k, uint64_t r0, uint64_t r1) {
		uint64_t *n = &tally[(size_t)k * LT_CLASSES];
		for (uint64_t r = r0; r < r1; ++r) {
			const unsigned tr = R.blk_off[r] < R.blk_off[r + 1] ? read_transcript(ix.E, R.bst[R.blk_off[r]]) : 2u;
			bool plus = false, minus = false;
			for (uint64_t b = R.blk_off[r]; tr < 2u && b < R.blk_off[r + 1] && !(plus && minus); ++b) {
				const unsigned c = R.bc[b];
				const int32_t s = R.bs[b], e = R.be[b];
				if (c == NO_CHROM || c >= nc || e <= s) continue;
				if (!plus) plus = meets(ix, 2 * (size_t)c, s, e);
				if (!minus) minus = meets(ix, 2 * (size_t)c + 1, s, e);
			}
			++n[lt_class(tr, plus, minus)];
		}
	});
	if (rc) return rc;
	t = lsq_lt_table();
	t.reads = R.n_reads; t.unplaced_genes = ix.unplaced_genes;
	for (int k = 0; k < T; ++k) for (int q = 0; q < LT_CLASSES; ++q) t.cls[q] += tally[(size_t)k * LT_CLASSES + q];
	return LSQ_OK;
}

extern "C" {

int lsq_lt_index_build(const lsq_annotation *a, lsq_lt_index **out) LSQ_API_TRY {
	if (!a || !out) return fail(LSQ_E_ARG, "null argument");
	std::unique_ptr<lsq_lt_index> ix(new lsq_lt_index);
	int rc;
	// (forward: r itself is what read_transcript gives)
	if ((rc = annotation_dictionaries(*a, ix->E, LSQ_LIBRARY_FORWARD))) return rc;
	const size_t n_tab = ix->E.covered.size();
	std::vector<std::vector<std::pair<int64_t, int64_t>>> of_tab(n_tab);
	for (const Gene &g : a->selected) {
		bool placed = !g.isos.empty() && (g.isos[0]->strand == "+" || g.isos[0]->strand == "-");
		for (const IsoRec *r : g.isos) placed = placed && r->strand == g.isos[0]->strand;
		if (!placed) { ++ix->unplaced_genes; continue; }
		for (const IsoRec *r : g.isos) exon_union(*r, of_tab[ix->E.table_of((size_t)ix->E.chroms.find(r->chrom), r->strand == "-" ? 1u : 0u)]);
	}
	ix->tab_first.assign(1, 0);
	for (size_t tb = 0; tb < n_tab; ++tb) {
		int32_t s = 0, e = 0;
		bool open = false;
		for (const auto &x : of_tab[tb]) {         // (sorted by start: exon_union merges every line's exons into the list)
			const int32_t xs = clamped(x.first), xe = clamped(x.second);
			if (xe <= xs) continue;
			if (open && xs <= e) { e = std::max(e, xe); continue; }
			if (open) { ix->iv_start.push_back(s); ix->iv_end.push_back(e); }
			s = xs; e = xe; open = true;
		}
		if (open) { ix->iv_start.push_back(s); ix->iv_end.push_back(e); }
		if (ix->iv_start.size() > 0xFFFFFFFEull) return fail(LSQ_E_RANGE, "more than 2^32-2 intervals in the exon unions");
		ix->tab_first.push_back((uint32_t)ix->iv_start.size());
	}
	*out = ix.release();
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_lt_index_free(lsq_lt_index *ix) { delete ix; }
int64_t lsq_lt_index_num_chroms(const lsq_lt_index *ix) { return index_num_chroms(ix); }
const char *lsq_lt_index_chrom_name(const lsq_lt_index *ix, int64_t chrom) { return index_chrom_name(ix, chrom); }
lsq_events *lsq_lt_index_dictionaries(lsq_lt_index *ix) { return index_dictionaries(ix); }
int64_t lsq_lt_index_num_intervals(const lsq_lt_index *ix) { return ix ? (int64_t)ix->iv_start.size() : 0; }
int64_t lsq_lt_index_unplaced_genes(const lsq_lt_index *ix) { return ix ? (int64_t)ix->unplaced_genes : 0; }

int lsq_lt_host_reads(lsq_lt_index *ix, const lsq_reads *r, int n_threads, lsq_lt_table **out) LSQ_API_TRY {
	if (!ix || !r || !out) return fail(LSQ_E_ARG, "null argument");
	return new_table(out, [&](lsq_lt_table &t) { return lt_host_reads(*ix, host_view(*r), n_threads, t); });
} LSQ_API_CATCH

int lsq_lt_host(lsq_lt_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, int n_threads, lsq_lt_table **out) LSQ_API_TRY {
	if (!ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	return host_file(ix->E, read_format, path, skip_flags, min_mapq, n_threads, [&](const lsq_reads *r) { return lsq_lt_host_reads(ix, r, n_threads, out); });
} LSQ_API_CATCH

void lsq_lt_table_free(lsq_lt_table *t) { delete t; }
int lsq_lt_table_counts(const lsq_lt_table *t, uint64_t counts[11]) {
	if (!t || !counts) return fail(LSQ_E_ARG, "null argument");
	counts[0] = t->reads;
	for (int q = 0; q < LT_CLASSES; ++q) counts[1 + q] = t->cls[q];
	counts[10] = t->unplaced_genes;
	return LSQ_OK;
}
int lsq_lt_table_times(const lsq_lt_table *t, float ms[3]) { return table_times(t, ms); }
int lsq_lt_table_verdict(const lsq_lt_table *t, double *forward_fraction, int *has_fraction, const char **library) {
	if (!t) return fail(LSQ_E_ARG, "null argument");
	const Derived d = derived_of(*t);
	if (has_fraction) *has_fraction = d.sense + d.antisense ? 1 : 0;
	if (forward_fraction) *forward_fraction = d.sense + d.antisense ? (double)d.sense / (double)(d.sense + d.antisense) : 0.0;
	if (library) *library = verdict_of(d.sense, d.antisense);
	return LSQ_OK;
}

int lsq_lt_format(const lsq_lt_table *t, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	static const char *NAMES[LT_CLASSES] = {"no_strand", "plus_none", "plus_plus", "plus_minus", "plus_both", "minus_none", "minus_plus", "minus_minus", "minus_both"};
	const Derived d = derived_of(*t);
	std::string o;
	char buf[96];
	auto line = [&](const char *key, uint64_t v) { snprintf(buf, sizeof buf, "%s\t%llu\n", key, (unsigned long long)v); o += buf; };
	line("reads", t->reads);
	for (int q = 0; q < LT_CLASSES; ++q) line(NAMES[q], t->cls[q]);
	line("sense", d.sense); line("antisense", d.antisense); line("ambiguous", d.ambiguous); line("no_gene", d.no_gene);
	line("unplaced_genes", t->unplaced_genes);
	if (d.sense + d.antisense) { snprintf(buf, sizeof buf, "forward_fraction\t%.6f\n", (double)d.sense / (double)(d.sense + d.antisense)); o += buf; }
	else o += "forward_fraction\tNA\n";
	o += "library\t"; o += verdict_of(d.sense, d.antisense); o += '\n';
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

} // extern "C"

// libtype [--host] <isoform_format> <isoforms_path> <g2i_format> <g2i_path> <read_format> <reads_path> [<out>]
// key TAB value lines on standard output (or in <out>; "-": standard output), one info line in the log.  Exit status 0 whatever
// the verdict; 1, with nothing on standard output and no file, for a file that does not open or parse.
int lsq::run_libtype(int argc, const char *const *argv, std::string &out) {
	static const char *USAGE = "Usage:\nlibtype [--host] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]";
	bool host = false, bad = false;
	std::vector<const char *> pos;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else pos.push_back(argv[i]);
	}
	if (bad || pos.size() < 6 || pos.size() > 7) { cli_log(0, USAGE); return 1; }
	CliFrame F(pos);
	CliOwned<lsq_lt_index, lsq_lt_index_free> ix;
	CliOwned<lsq_lt_table, lsq_lt_table_free> t;
	int st = F.load_annotation();
	if (!st) st = lsq_lt_index_build(F.a, &ix.p);
	if (st) return cli_failed(st);
	if (host) {
		if (!(st = F.host_parse(&ix.p->E))) st = lsq_lt_host_reads(ix.p, F.reads, 0, &t.p);
		F.free_reads();
	} else if (!(st = F.create_context())) st = lsq_lt_device(F.c, ix.p, pos[4], pos[5], &t.p);
	if (!st) st = lsq_lt_format(t.p, &F.text[0]);
	if (st) return cli_failed(st);
	const Derived d = derived_of(*t.p);
	char msg[384];
	snprintf(msg, sizeof msg, "libtype: %llu read(s), %llu without a strand; %llu sense, %llu antisense, %llu on genes of both strands, %llu on no gene; %llu gene(s) without a strand left out: %s",
	         (unsigned long long)t.p->reads, (unsigned long long)t.p->cls[0], (unsigned long long)d.sense, (unsigned long long)d.antisense, (unsigned long long)d.ambiguous,
	         (unsigned long long)d.no_gene, (unsigned long long)t.p->unplaced_genes, verdict_of(d.sense, d.antisense));
	cli_log(2, msg);
	return F.deliver(F.text[0], out);
}
