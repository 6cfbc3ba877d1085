// Junction reads per event form of a read file (include/lesseq_hip.h, lsq_ps_*): the index made from an annotation,
// the host path over the host parsers' arrays, the table's text and the psi executable.  The device count is lsq_psi.hip, the
// entry that opens a read file on the device is lsq_readfile.hip's lsq_ps_device; what the tool shares with junctions, coverage
// and exonbins is lsq_readtool.hpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iterator>

#include "lsq_psi.hpp"

using namespace lsq;

namespace {

typedef std::pair<uint32_t, uint64_t> Intron;        // (chromosome index -- a stranded index: table id --, jn_key): pairs compare as the lookup is ordered

// psi per form from the integers, NaN for NA: x_f = reads_f / introns_f, den the sum of x_g over the event's forms in row order,
// psi_f = x_f / den; NA for every form of an event that has a form without an informative intron or whose den is 0
void psi_of(const lsq_ps_table &t, std::vector<double> &psi) {
	psi.assign(t.reads.size(), std::nan(""));
	for (size_t e = 0; e + 1 < t.event_first_form.size(); ++e) {
		const uint32_t f0 = t.event_first_form[e], f1 = t.event_first_form[e + 1];
		bool ok = f1 > f0;
		double den = 0;
		for (uint32_t f = f0; f < f1 && ok; ++f) {
			if (t.form_introns[f] == 0) ok = false;
			else den += (double)t.reads[f] / (double)t.form_introns[f];
		}
		if (!ok || den == 0) continue;
		for (uint32_t f = f0; f < f1; ++f) psi[f] = (double)t.reads[f] / (double)t.form_introns[f] / den;
	}
}

} // namespace

void lsq::ps_start_table(const lsq_ps_index &ix, lsq_ps_table &t) {
	t.event_name = ix.event_name; t.form_name = ix.form_name; t.event_first_form = ix.event_first_form; t.form_introns = ix.form_introns;
	t.reads.assign(ix.form_name.size(), 0); t.total.assign(ix.event_name.size(), 0);
	t.library = ix.E.library;
	for (uint64_t &v : t.report) v = 0;
	for (uint64_t &v : t.lib) v = 0;
	for (float &m : t.ms) m = 0;
}

// A thread a stretch of reads, counters of its own: the forms of every informative intron a read's block pairs meet are listed
// per read, sorted and made distinct (a read counts once a form); the events are the distinct form_event of that list (forms are
// event-major: they ascend).  Under a stranded index a read looks in the tables of its transcript strand t alone;
// one without t finds nothing, behind the tallies of its pairs.
int lsq::ps_host_reads(const lsq_ps_index &ix, const ParsedReads &R, uint32_t min_overhang, int n_threads, lsq_ps_table &t) {
	const int T = read_slices(R.n_reads, n_threads);
	const size_t nf = ix.form_name.size(), ne = ix.event_name.size();
	ps_start_table(ix, t);
	std::vector<std::vector<uint64_t>> part((size_t)T);
	const bool stranded = ix.E.stranded();
	constexpr int NT = 6 + LIB_REPORT;
	std::vector<uint64_t> tally((size_t)T * NT, 0);      // occurrences, below the overhang, no chromosome, found, reads on an event, on several; the library report
	const int rc = for_read_slices(R.n_reads, T, [&](int k, uint64_t r0, uint64_t r1) {
		std::vector<uint64_t> &cnt = part[(size_t)k];
		cnt.assign(nf + ne, 0);
		uint64_t *n = &tally[(size_t)k * NT];
		std::vector<uint32_t> hit;
		for (uint64_t r = r0; r < r1; ++r) {
			hit.clear();
			const unsigned tr = !stranded ? 0u : R.blk_off[r] < R.blk_off[r + 1] ? read_transcript(ix.E, R.bst[R.blk_off[r]]) : 2u;
			for (uint64_t b = R.blk_off[r]; b + 1 < R.blk_off[r + 1]; ++b) {
				const uint32_t i = ps_host_pair(ix, R, b, min_overhang, n, tr);
				if (i == PS_NONE) continue;
				++n[3];
				hit.insert(hit.end(), ix.intron_forms.begin() + ix.intron_off[i], ix.intron_forms.begin() + ix.intron_off[i + 1]);
			}
			std::sort(hit.begin(), hit.end());
			hit.erase(std::unique(hit.begin(), hit.end()), hit.end());
			uint32_t events = 0, last = PS_NONE;
			for (uint32_t f : hit) {
				++cnt[f];
				if (ix.form_event[f] != last) { last = ix.form_event[f]; ++cnt[nf + last]; ++events; }
			}
			if (events > 0) ++n[4];
			if (events > 1) ++n[5];
			if (stranded) lib_note(n + 6, tr, events > 0);
		}
	});
	if (rc) return rc;
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks;
	for (int k = 0; k < T; ++k) {
		for (size_t f = 0; f < nf; ++f) t.reads[f] += part[(size_t)k][f];
		for (size_t e = 0; e < ne; ++e) t.total[e] += part[(size_t)k][nf + e];
		for (int q = 0; q < 6; ++q) t.report[2 + q] += tally[(size_t)k * NT + q];
		for (int q = 0; q < LIB_REPORT; ++q) t.lib[q] += tally[(size_t)k * NT + 6 + q];
	}
	return LSQ_OK;
}

extern "C" {

int lsq_ps_index_build(const lsq_annotation *a, lsq_ps_index **out) { return lsq_ps_index_build_library(a, LSQ_LIBRARY_UNSTRANDED, out); }

int lsq_ps_index_build_library(const lsq_annotation *a, int library, lsq_ps_index **out) LSQ_API_TRY {
	return ps_index_build(a, library, "psi", out);
} LSQ_API_CATCH

} // extern "C"

int lsq::ps_index_build(const lsq_annotation *a, int library, const char *tool, lsq_ps_index **out) {
	if (!a || !out) return fail(LSQ_E_ARG, "null argument");
	std::unique_ptr<lsq_ps_index> ix(new lsq_ps_index);
	int rc;
	if ((rc = annotation_dictionaries(*a, ix->E, library))) return rc;
	// an event's strand: the one its lines share (a stranded index needs "+" or "-": checked once all are known, so that the message counts them)
	for (const Gene &g : a->selected) {
		std::string strand = g.isos.empty() ? "." : g.isos[0]->strand;
		for (const IsoRec *r : g.isos) if (r->strand != strand) strand = ".";
		ix->event_strand.push_back(strand);
	}
	if (ix->E.stranded()) {
		std::vector<std::string> names;
		for (const Gene &g : a->selected) names.push_back(g.name);
		if ((rc = require_strands(names, ix->event_strand, "event", tool))) return rc;
	}
	struct Entry { Intron in; uint32_t form; };
	std::vector<Entry> entries;
	std::vector<std::pair<int64_t, int64_t>> ex, gaps;
	std::vector<std::vector<Intron>> of_form;
	std::vector<Intron> common, both;
	ix->event_first_form.push_back(0);
	for (const Gene &g : a->selected) {
		if (ix->form_name.size() + g.isos.size() > 0xFFFFFFFEull) return fail(LSQ_E_RANGE, "more than 2^32-2 event forms");
		// every form's introns (a line's gaps ascend and differ, and so do their keys), and those that all forms of the event hold
		of_form.assign(g.isos.size(), std::vector<Intron>());
		for (size_t j = 0; j < g.isos.size(); ++j) {
			const IsoRec &r = *g.isos[j];
			const uint32_t c = (uint32_t)ix->E.table_of((size_t)ix->E.chroms.find(r.chrom), ix->event_strand[ix->event_name.size()] == "-" ? 1u : 0u);
			gaps.clear();
			line_introns(r, ex, gaps);
			for (const auto &gap : gaps) of_form[j].emplace_back(c, jn_key(gap.first, gap.second));
			if (j == 0) common = of_form[0];
			else {
				both.clear();
				std::set_intersection(common.begin(), common.end(), of_form[j].begin(), of_form[j].end(), std::back_inserter(both));
				common.swap(both);
			}
		}
		for (size_t j = 0; j < g.isos.size(); ++j) {
			const uint32_t f = (uint32_t)ix->form_name.size();
			uint32_t n = 0;
			for (const Intron &in : of_form[j]) if (!std::binary_search(common.begin(), common.end(), in)) { entries.push_back(Entry{in, f}); ++n; }
			ix->form_name.push_back(g.isos[j]->name); ix->form_event.push_back((uint32_t)ix->event_name.size()); ix->form_introns.push_back(n);
		}
		ix->event_name.push_back(g.name);
		ix->event_first_form.push_back((uint32_t)ix->form_name.size());
	}
	if (entries.size() > 0xFFFFFFFEull) return fail(LSQ_E_RANGE, "more than 2^32-2 informative introns over all event forms");
	std::sort(entries.begin(), entries.end(), [](const Entry &x, const Entry &y) { return x.in != y.in ? x.in < y.in : x.form < y.form; });
	const size_t nc = ix->E.covered.size();
	ix->chrom_first_intron.assign(nc + 1, 0);
	ix->intron_off.push_back(0);
	for (size_t i = 0; i < entries.size(); ++i) {
		if (i == 0 || entries[i].in != entries[i - 1].in) {
			if (i) ix->intron_off.push_back((uint32_t)i);
			ix->intron_key.push_back(entries[i].in.second);
			++ix->chrom_first_intron[entries[i].in.first + 1];
		}
		ix->intron_forms.push_back(entries[i].form);
	}
	if (!entries.empty()) ix->intron_off.push_back((uint32_t)entries.size());
	for (size_t c = 0; c < nc; ++c) ix->chrom_first_intron[c + 1] += ix->chrom_first_intron[c];
	*out = ix.release();
	return LSQ_OK;
}

extern "C" {

void lsq_ps_index_free(lsq_ps_index *ix) { delete ix; }
int lsq_ps_index_library(const lsq_ps_index *ix) { return index_library(ix); }
int64_t lsq_ps_index_num_chroms(const lsq_ps_index *ix) { return index_num_chroms(ix); }
int64_t lsq_ps_index_num_events(const lsq_ps_index *ix) { return ix ? (int64_t)ix->event_name.size() : 0; }
int64_t lsq_ps_index_num_forms(const lsq_ps_index *ix) { return ix ? (int64_t)ix->form_name.size() : 0; }
int64_t lsq_ps_index_num_introns(const lsq_ps_index *ix) { return ix ? (int64_t)ix->intron_key.size() : 0; }
const char *lsq_ps_index_chrom_name(const lsq_ps_index *ix, int64_t chrom) { return index_chrom_name(ix, chrom); }
const char *lsq_ps_index_event_name(const lsq_ps_index *ix, int64_t event) {
	return ix && event >= 0 && (size_t)event < ix->event_name.size() ? ix->event_name[(size_t)event].c_str() : nullptr;
}
const char *lsq_ps_index_form_name(const lsq_ps_index *ix, int64_t form) {
	return ix && form >= 0 && (size_t)form < ix->form_name.size() ? ix->form_name[(size_t)form].c_str() : nullptr;
}
lsq_events *lsq_ps_index_dictionaries(lsq_ps_index *ix) { return index_dictionaries(ix); }
int lsq_ps_index_arrays(const lsq_ps_index *ix, const uint32_t **event_first_form, const uint32_t **form_introns) {
	if (!ix) return fail(LSQ_E_ARG, "null argument");
	if (event_first_form) *event_first_form = ix->event_first_form.data();
	if (form_introns) *form_introns = ix->form_introns.data();
	return LSQ_OK;
}

int lsq_ps_host_reads(lsq_ps_index *ix, const lsq_reads *r, uint32_t min_overhang, int n_threads, lsq_ps_table **out) LSQ_API_TRY {
	if (!ix || !r || !out) return fail(LSQ_E_ARG, "null argument");
	if (min_overhang < 1) return fail(LSQ_E_ARG, "min_overhang must be at least 1");
	return new_table(out, [&](lsq_ps_table &t) { return ps_host_reads(*ix, host_view(*r), min_overhang, n_threads, t); });
} LSQ_API_CATCH

int lsq_ps_host(lsq_ps_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, uint32_t min_overhang, int n_threads,
                lsq_ps_table **out) LSQ_API_TRY {
	if (!ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	if (min_overhang < 1) return fail(LSQ_E_ARG, "min_overhang must be at least 1");
	return host_file(ix->E, read_format, path, skip_flags, min_mapq, n_threads, [&](const lsq_reads *r) { return lsq_ps_host_reads(ix, r, min_overhang, n_threads, out); });
} LSQ_API_CATCH

void lsq_ps_table_free(lsq_ps_table *t) { delete t; }
int lsq_ps_table_arrays(const lsq_ps_table *t, const uint64_t **reads, const uint64_t **total) {
	if (!t) return fail(LSQ_E_ARG, "null argument");
	if (reads) *reads = t->reads.data();
	if (total) *total = t->total.data();
	return LSQ_OK;
}
int lsq_ps_table_report(const lsq_ps_table *t, uint64_t report[8]) { return table_report(t, report); }
int lsq_ps_table_library_report(const lsq_ps_table *t, uint64_t report[5]) { return table_library_report(t, report); }
int lsq_ps_table_times(const lsq_ps_table *t, float ms[3]) { return table_times(t, ms); }
int lsq_ps_table_psi(const lsq_ps_table *t, double *psi) LSQ_API_TRY {
	if (!t || (!psi && !t->reads.empty())) return fail(LSQ_E_ARG, "null argument");
	std::vector<double> v;
	psi_of(*t, v);
	if (!v.empty()) memcpy(psi, v.data(), v.size() * sizeof(double));
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_ps_format(const lsq_ps_table *t, int with_psi, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	char buf[96];
	std::vector<double> psi;
	if (with_psi) psi_of(*t, psi);
	for (size_t e = 0; e < t->event_name.size(); ++e)
		for (uint32_t f = t->event_first_form[e]; f < t->event_first_form[e + 1]; ++f) {
			o += t->event_name[e];
			snprintf(buf, sizeof buf, "\t%llu\t", (unsigned long long)t->total[e]);
			o += buf; o += t->form_name[f];
			snprintf(buf, sizeof buf, "\t%llu", (unsigned long long)t->reads[f]);
			o += buf;
			if (with_psi) {
				if (std::isnan(psi[f])) snprintf(buf, sizeof buf, "\t%u\tNA", t->form_introns[f]);
				else snprintf(buf, sizeof buf, "\t%u\t%.6f", t->form_introns[f], psi[f]);
				o += buf;
			}
			o += '\n';
		}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

} // extern "C"

// psi [--host] [--psi] [--min-overhang N] [--library unstranded|forward|reverse] <isoform_format> <isoforms_path> <g2i_format> <g2i_path> <read_format> <reads_path> [<out>]
// The table on standard output (or in <out>; "-": standard output), the report in the log.  Without --library the library type is
// LSQ_LIBRARY's (unstranded without either); a stranded run logs its library report behind the report.  Exit status 1, nothing on
// standard output and no file, for a file that does not open or parse, and for a stranded run over an event without a strand.
int lsq::run_psi(int argc, const char *const *argv, std::string &out) {
	static const char *USAGE = "Usage:\npsi [--host] [--psi] [--min-overhang N] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]";
	bool host = false, with_psi = false, bad = false, lib_given = false;
	int library = LSQ_LIBRARY_UNSTRANDED;
	unsigned long min_ov = 1;
	std::vector<const char *> pos;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (strcmp(argv[i], "--psi") == 0) with_psi = true;
		else if (strcmp(argv[i], "--min-overhang") == 0) bad = !cli_u32_option(argc, argv, i, min_ov);
		else if (strcmp(argv[i], "--library") == 0) {
			if (i + 1 >= argc) bad = true;
			else if (!cli_library_option(argc, argv, i, library)) return 1;
			lib_given = true;
		} else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else pos.push_back(argv[i]);
	}
	if (bad || pos.size() < 6 || pos.size() > 7 || min_ov < 1) { cli_log(0, USAGE); return 1; }
	if (!lib_given && !cli_library_env(library)) return 1;
	CliFrame F(pos);
	CliOwned<lsq_ps_index, lsq_ps_index_free> ix;
	CliOwned<lsq_ps_table, lsq_ps_table_free> t;
	int st = F.load_annotation();
	if (!st) st = lsq_ps_index_build_library(F.a, library, &ix.p);
	if (st) return cli_failed(st);
	if (host) {
		if (!(st = F.host_parse(&ix.p->E))) st = lsq_ps_host_reads(ix.p, F.reads, (uint32_t)min_ov, 0, &t.p);
		F.free_reads();
	} else if (!(st = F.create_context())) st = lsq_ps_device(F.c, ix.p, pos[4], pos[5], (uint32_t)min_ov, &t.p);
	if (!st) st = lsq_ps_format(t.p, with_psi ? 1 : 0, &F.text[0]);
	if (st) return cli_failed(st);
	const uint64_t *rep = t.p->report;
	char msg[512];
	snprintf(msg, sizeof msg, "psi: %llu read(s), %llu block(s), %llu junction occurrence(s), %llu block pair(s) below the overhang, %llu with a block on no chromosome of the annotation; "
	         "%lld informative intron(s) of %lld form(s) in %lld event(s): %llu occurrence(s) on them, %llu read(s) counted, %llu for more than one event",
	         (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2], (unsigned long long)rep[3], (unsigned long long)rep[4],
	         (long long)lsq_ps_index_num_introns(ix.p), (long long)lsq_ps_index_num_forms(ix.p), (long long)lsq_ps_index_num_events(ix.p),
	         (unsigned long long)rep[5], (unsigned long long)rep[6], (unsigned long long)rep[7]);
	cli_log(2, msg);
	if (library != LSQ_LIBRARY_UNSTRANDED) cli_log_library("psi", library, t.p->lib);
	return F.deliver(F.text[0], out);
}
