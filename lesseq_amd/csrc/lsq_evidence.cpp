// Junction and exon-body reads per event form of a read file (include/lesseq_hip.h, lsq_fe_*): the index made from an
// annotation -- psi's index for the junction half, the informative body's regions with their cell lookup for the other -- the host
// path over the host parsers' arrays, positions(f), the table's text and the evidence executable.  The device count is
// lsq_evidence.hip, the entry that opens a read file on the device is lsq_readfile.hip's lsq_fe_device; what the tool shares with
// junctions, coverage, exonbins and psi is lsq_readtool.hpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "lsq_evidence.hpp"

using namespace lsq;

namespace {

typedef std::pair<int64_t, int64_t> Iv;

// the maximal intervals of a line's exon union (`ex`: scratch): what line_introns takes the gaps of
void union_intervals(const IsoRec &r, std::vector<Iv> &ex, std::vector<Iv> &out) {
	ex.clear(); out.clear();
	exon_union(r, ex);
	for (const Iv &x : ex) {
		if (!out.empty() && x.first <= out.back().second) out.back().second = std::max(out.back().second, x.second);
		else out.push_back(x);
	}
}

// a and b ascending, disjoint and apart: the bases in both, as such a list
void intersect(const std::vector<Iv> &a, const std::vector<Iv> &b, std::vector<Iv> &out) {
	out.clear();
	for (size_t i = 0, j = 0; i < a.size() && j < b.size();) {
		const int64_t s = std::max(a[i].first, b[j].first), e = std::min(a[i].second, b[j].second);
		if (s < e) out.emplace_back(s, e);
		if (a[i].second < b[j].second) ++i; else ++j;
	}
}

inline int32_t clamped(int64_t x) { return (int32_t)std::max<int64_t>(-FE_LIM, std::min<int64_t>(FE_LIM, x)); }

// the first cell of chromosome (stranded index: table) c that ends behind s (chrom_first_cell[c + 1]: none)
inline uint32_t first_cell(const lsq_fe_index &ix, size_t c, int32_t s) {
	uint32_t lo = ix.chrom_first_cell[c], hi = ix.chrom_first_cell[c + 1];
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (ix.cell_end[mid] <= s) lo = mid + 1; else hi = mid;
	}
	return lo;
}

// positions(f) by the definition's enumeration: every start of an ungapped L-base read along the form's concatenated exon union,
// its blocks the pieces of the union's intervals it covers, counted where the counting rule counts the read for f.  The closed
// form below stands for it wherever the form lies inside (-2^30, 2^30); a form that reaches beyond comes here, where a piece
// that leaves the range is a block on no chromosome.
uint64_t positions_enumerated(const FeGeometry &G, uint32_t f, uint64_t T, uint32_t L, uint32_t mo, uint32_t mb) {
	const uint32_t i0 = G.form_first_iv[f], i1 = G.form_first_iv[f + 1], g0 = G.form_first_region[f], g1 = G.form_first_region[f + 1];
	uint64_t n = 0;
	for (uint64_t s = 0; s + L <= T; ++s) {
		bool counts = false, prev_have = false, prev_ok = false;
		int64_t prev_len = 0;
		uint64_t off = 0;
		for (uint32_t i = i0; i < i1 && !counts; ++i) {
			const uint64_t len = (uint64_t)(G.iv_end[i] - G.iv_start[i]), lo = std::max(s, off), hi = std::min(s + L, off + len);
			const bool have = lo < hi;
			bool ok = false;
			int64_t ps = 0, pe = 0;
			if (have) {
				ps = G.iv_start[i] + (int64_t)(lo - off); pe = G.iv_start[i] + (int64_t)(hi - off);
				ok = ps > -FE_LIM && pe < FE_LIM;
				if (prev_have && prev_ok && ok && G.iv_gap_informative[i - 1] && std::min(prev_len, pe - ps) >= (int64_t)mo) counts = true;
				for (uint32_t g = g0; g < g1 && ok && !counts; ++g)
					if (std::min<int64_t>(pe, G.region_end[g]) - std::max<int64_t>(ps, G.region_start[g]) >= (int64_t)mb) counts = true;
			}
			prev_have = have; prev_ok = ok; prev_len = pe - ps;
			off += len;
		}
		n += counts;
	}
	return n;
}

// positions(f): the size of the union, clipped to [0, T - L], of the windows of starts at which an informative intron or a region
// counts the read (include/lesseq_hip.h)
uint64_t positions_of(const FeGeometry &G, uint32_t f, uint32_t L, uint32_t mo, uint32_t mb) {
	const uint32_t i0 = G.form_first_iv[f], i1 = G.form_first_iv[f + 1];
	uint64_t T = 0;
	bool inside = true;
	for (uint32_t i = i0; i < i1; ++i) { T += (uint64_t)(G.iv_end[i] - G.iv_start[i]); inside = inside && G.iv_start[i] > -FE_LIM && G.iv_end[i] < FE_LIM; }
	if (T < L) return 0;
	if (!inside) return positions_enumerated(G, f, T, L, mo, mb);
	std::vector<Iv> win;                        // closed windows of starts
	int64_t off = 0;
	uint32_t g = G.form_first_region[f];
	const uint32_t g1 = G.form_first_region[f + 1];
	for (uint32_t i = i0; i < i1; ++i) {
		const int64_t len = G.iv_end[i] - G.iv_start[i];
		if (i + 1 < i1 && G.iv_gap_informative[i] && len >= (int64_t)mo && G.iv_end[i + 1] - G.iv_start[i + 1] >= (int64_t)mo)
			win.emplace_back(off + len - (int64_t)L + (int64_t)mo, off + len - (int64_t)mo);
		for (; g < g1 && G.region_end[g] <= G.iv_end[i]; ++g) {      // (a form's regions ascend, each inside one interval of its union)
			const int64_t a = off + (G.region_start[g] - G.iv_start[i]), z = off + (G.region_end[g] - G.iv_start[i]);
			if (z - a >= (int64_t)mb && (int64_t)L >= (int64_t)mb) win.emplace_back(a - (int64_t)L + (int64_t)mb, z - (int64_t)mb);
		}
		off += len;
	}
	std::sort(win.begin(), win.end());
	const int64_t last = (int64_t)(T - L);
	int64_t reach = -1;                         // the last start counted so far
	uint64_t n = 0;
	for (const Iv &w : win) {
		const int64_t lo = std::max<int64_t>(std::max<int64_t>(w.first, 0), reach + 1), hi = std::min(w.second, last);
		if (lo <= hi) { n += (uint64_t)(hi - lo + 1); reach = hi; }
	}
	return n;
}

void positions_all(const lsq_fe_table &t, uint32_t L, std::vector<uint64_t> &pos) {
	pos.resize(t.reads.size());
	for (size_t f = 0; f < pos.size(); ++f) pos[f] = positions_of(*t.G, (uint32_t)f, L, t.min_overhang, t.min_body);
}

// psi per form from the integers, NaN for NA: x_f = reads_f / positions_f, den the sum of x_g over the event's forms in row order,
// psi_f = x_f / den; NA for every form of an event that has a form with positions 0 or whose den is 0
void psi_of(const lsq_fe_table &t, const std::vector<uint64_t> &pos, std::vector<double> &psi) {
	psi.assign(t.reads.size(), std::nan(""));
	for (size_t e = 0; e + 1 < t.event_first_form.size(); ++e) {
		const uint32_t f0 = t.event_first_form[e], f1 = t.event_first_form[e + 1];
		bool ok = f1 > f0;
		double den = 0;
		for (uint32_t f = f0; f < f1 && ok; ++f) {
			if (pos[f] == 0) ok = false;
			else den += (double)t.reads[f] / (double)pos[f];
		}
		if (!ok || den == 0) continue;
		for (uint32_t f = f0; f < f1; ++f) psi[f] = (double)t.reads[f] / (double)pos[f] / den;
	}
}

inline bool options_ok(uint32_t min_overhang, uint32_t min_body) {
	if (min_overhang < 1) { fail(LSQ_E_ARG, "min_overhang must be at least 1"); return false; }
	if (min_body < 1) { fail(LSQ_E_ARG, "min_body must be at least 1"); return false; }
	return true;
}

} // namespace

void lsq::fe_start_table(const lsq_fe_index &ix, uint32_t min_overhang, uint32_t min_body, lsq_fe_table &t) {
	const lsq_ps_index &P = *ix.P;
	t.event_name = P.event_name; t.form_name = P.form_name; t.event_first_form = P.event_first_form; t.form_introns = P.form_introns;
	t.form_body = ix.form_body; t.G = ix.G; t.min_overhang = min_overhang; t.min_body = min_body;
	t.reads.assign(P.form_name.size(), 0); t.total.assign(P.event_name.size(), 0);
	t.library = ix.E.library;
	for (uint64_t &v : t.report) v = 0;
	for (uint64_t &v : t.lib) v = 0;
	for (float &m : t.ms) m = 0;
}

// A thread a stretch of reads, counters of its own: the forms of every informative intron a read's block pairs meet (psi's walk) and
// of every region a block hits (the cells' walk: a region is taken at the first of its cells the block overlaps) are listed per
// read, sorted and made distinct (a read counts once a form); the events are the distinct form_event of that list (forms are
// event-major: they ascend).  Under a stranded index a read looks in the tables of its transcript strand t alone;
// one without t finds nothing, behind the tallies of its pairs and blocks.
int lsq::fe_host_reads(const lsq_fe_index &ix, const ParsedReads &R, uint32_t min_overhang, uint32_t min_body, int n_threads, lsq_fe_table &t) {
	const lsq_ps_index &P = *ix.P;
	const FeGeometry &G = *ix.G;
	const int T = read_slices(R.n_reads, n_threads);
	const size_t nf = P.form_name.size(), ne = P.event_name.size(), nc = ix.E.n_table_chroms();
	const bool stranded = ix.E.stranded();
	constexpr int NT = 9 + LIB_REPORT;
	fe_start_table(ix, min_overhang, min_body, t);
	std::vector<std::vector<uint64_t>> part((size_t)T);
	// occurrences, below the overhang, no chromosome, found, skipped blocks, body hits, reads on an event, on several, by body alone
	std::vector<uint64_t> tally((size_t)T * NT, 0);      // (behind the nine: the library report)
	const int rc = for_read_slices(R.n_reads, T, [&](int k, uint64_t r0, uint64_t r1) {
		std::vector<uint64_t> &cnt = part[(size_t)k];
		cnt.assign(nf + ne, 0);
		uint64_t *n = &tally[(size_t)k * NT];
		std::vector<uint32_t> hit;
		for (uint64_t r = r0; r < r1; ++r) {
			hit.clear();
			const uint64_t found_before = n[3];
			const unsigned tr = !stranded ? 0u : R.blk_off[r] < R.blk_off[r + 1] ? read_transcript(ix.E, R.bst[R.blk_off[r]]) : 2u;
			for (uint64_t b = R.blk_off[r]; b + 1 < R.blk_off[r + 1]; ++b) {
				const uint32_t i = ps_host_pair(P, R, b, min_overhang, n, tr);
				if (i == PS_NONE) continue;
				++n[3];
				hit.insert(hit.end(), P.intron_forms.begin() + P.intron_off[i], P.intron_forms.begin() + P.intron_off[i + 1]);
			}
			for (uint64_t b = R.blk_off[r]; b < R.blk_off[r + 1]; ++b) {
				const unsigned c = R.bc[b];
				const int32_t s = R.bs[b], e = R.be[b];
				if (c == NO_CHROM || c >= nc || e <= s) { ++n[4]; continue; }
				if (tr == 2u) continue;
				const size_t tb = ix.E.table_of(c, tr);
				const uint32_t first = first_cell(ix, tb, s);
				for (uint32_t i = first; i < ix.chrom_first_cell[tb + 1] && ix.cell_start[i] < e; ++i)
					for (uint32_t q = ix.cell_off[i]; q < ix.cell_off[i + 1]; ++q) {
						const uint32_t g = ix.cell_regions[q];
						if (i != first && G.region_start[g] != ix.cell_start[i]) continue;      // met in an earlier cell of this walk
						if (!fe_overlap_hits(s, e, G.region_start[g], G.region_end[g], min_body)) continue;
						++n[5];
						hit.push_back(ix.region_form[g]);
					}
			}
			std::sort(hit.begin(), hit.end());
			hit.erase(std::unique(hit.begin(), hit.end()), hit.end());
			uint32_t events = 0, last = PS_NONE;
			for (uint32_t f : hit) {
				++cnt[f];
				if (P.form_event[f] != last) { last = P.form_event[f]; ++cnt[nf + last]; ++events; }
			}
			if (events > 0) ++n[6];
			if (events > 1) ++n[7];
			if (events > 0 && n[3] == found_before) ++n[8];
			if (stranded) lib_note(n + 9, tr, events > 0);
		}
	});
	if (rc) return rc;
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks;
	for (int k = 0; k < T; ++k) {
		for (size_t f = 0; f < nf; ++f) t.reads[f] += part[(size_t)k][f];
		for (size_t e = 0; e < ne; ++e) t.total[e] += part[(size_t)k][nf + e];
		for (int q = 0; q < 9; ++q) t.report[2 + q] += tally[(size_t)k * NT + q];
		for (int q = 0; q < LIB_REPORT; ++q) t.lib[q] += tally[(size_t)k * NT + 9 + q];
	}
	return LSQ_OK;
}

extern "C" {

int lsq_fe_index_build(const lsq_annotation *a, lsq_fe_index **out) { return lsq_fe_index_build_library(a, LSQ_LIBRARY_UNSTRANDED, out); }

int lsq_fe_index_build_library(const lsq_annotation *a, int library, lsq_fe_index **out) LSQ_API_TRY {
	if (!a || !out) return fail(LSQ_E_ARG, "null argument");
	std::unique_ptr<lsq_fe_index> ix(new lsq_fe_index);
	int rc;
	if ((rc = annotation_dictionaries(*a, ix->E, library))) return rc;
	lsq_ps_index *p = nullptr;
	if ((rc = ps_index_build(a, library, "evidence", &p))) return rc;      // (a stranded index: every event has a strand of its own, or this fails)
	ix->P.reset(p);
	ix->G = std::make_shared<FeGeometry>();
	FeGeometry &G = *ix->G;
	std::vector<Iv> ex, common, both;
	std::vector<std::vector<Iv>> of_form;
	G.form_first_iv.push_back(0); G.form_first_region.push_back(0);
	size_t event = 0;
	for (const Gene &g : a->selected) {
		const unsigned e_minus = p->event_strand[event++] == "-" ? 1u : 0u;      // (the tables of the event: a stranded index's alone)
		// every form's exon union, and the bases all forms of the event hold: none where two forms lie on different chromosomes
		of_form.assign(g.isos.size(), std::vector<Iv>());
		bool one_chrom = true;
		for (size_t j = 0; j < g.isos.size(); ++j) {
			union_intervals(*g.isos[j], ex, of_form[j]);
			if (j == 0) common = of_form[0];
			else {
				if (g.isos[j]->chrom != g.isos[0]->chrom) one_chrom = false;
				intersect(common, of_form[j], both);
				common.swap(both);
			}
		}
		if (!one_chrom) common.clear();
		for (size_t j = 0; j < g.isos.size(); ++j) {
			const uint32_t f = (uint32_t)ix->form_chrom.size(), c = (uint32_t)ix->E.chroms.find(g.isos[j]->chrom);
			const std::vector<Iv> &U = of_form[j];
			uint64_t body = 0;
			size_t q = 0;                           // the first common interval that ends behind the walk
			for (size_t i = 0; i < U.size(); ++i) {
				// the gap behind interval i: an intron where line_introns makes it one, informative where psi's lookup lists this form
				bool informative = false;
				if (i + 1 < U.size() && U[i].second > -FE_LIM && U[i + 1].first < FE_LIM) {
					const uint32_t in = ps_find_intron(*p, p->E.table_of(c, e_minus), jn_key(U[i].second, U[i + 1].first));
					informative = in != PS_NONE && std::binary_search(p->intron_forms.begin() + p->intron_off[in], p->intron_forms.begin() + p->intron_off[in + 1], f);
				}
				G.iv_start.push_back(U[i].first); G.iv_end.push_back(U[i].second); G.iv_gap_informative.push_back(informative ? 1 : 0);
				// U(f) \ C(e) inside this interval (C(e) lies inside U(f)): the stretches between the common intervals
				int64_t at = U[i].first;
				auto region = [&](int64_t s, int64_t e) {
					const int32_t cs = clamped(s), ce = clamped(e);
					if (ce <= cs) return;
					G.region_start.push_back(cs); G.region_end.push_back(ce); ix->region_form.push_back(f);
					body += (uint64_t)((int64_t)ce - cs);
				};
				for (; q < common.size() && common[q].second <= U[i].second; ++q) {
					if (common[q].first > at) region(at, common[q].first);
					at = common[q].second;
				}
				if (at < U[i].second) region(at, U[i].second);
			}
			if (G.region_start.size() > 0xFFFFFFFEull) return fail(LSQ_E_RANGE, "more than 2^32-2 informative body regions over all event forms");
			ix->form_chrom.push_back(c); ix->form_body.push_back(body);
			G.form_first_iv.push_back((uint32_t)G.iv_start.size()); G.form_first_region.push_back((uint32_t)G.region_start.size());
		}
	}
	if (ix->form_chrom.size() != p->form_name.size()) return fail(LSQ_E_INTERNAL, "the evidence index and the psi index differ in their forms");
	std::vector<uint32_t> region_chrom(ix->region_form.size());
	for (size_t r = 0; r < region_chrom.size(); ++r) {      // (a stranded index: the region's table id)
		const uint32_t f = ix->region_form[r];
		region_chrom[r] = (uint32_t)ix->E.table_of(ix->form_chrom[f], p->event_strand[p->form_event[f]] == "-" ? 1u : 0u);
	}
	if ((rc = build_cells(ix->E.covered.size(), region_chrom, G.region_start, G.region_end, ix->chrom_first_cell, ix->cell_start, ix->cell_end, ix->cell_off, ix->cell_regions,
	                      "more than 2^32-1 entries in the region lookup (overlapping events)"))) return rc;
	*out = ix.release();
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_fe_index_free(lsq_fe_index *ix) { delete ix; }
int lsq_fe_index_library(const lsq_fe_index *ix) { return index_library(ix); }
int64_t lsq_fe_index_num_chroms(const lsq_fe_index *ix) { return index_num_chroms(ix); }
int64_t lsq_fe_index_num_events(const lsq_fe_index *ix) { return ix ? lsq_ps_index_num_events(ix->P.get()) : 0; }
int64_t lsq_fe_index_num_forms(const lsq_fe_index *ix) { return ix ? lsq_ps_index_num_forms(ix->P.get()) : 0; }
int64_t lsq_fe_index_num_introns(const lsq_fe_index *ix) { return ix ? lsq_ps_index_num_introns(ix->P.get()) : 0; }
int64_t lsq_fe_index_num_regions(const lsq_fe_index *ix) { return ix ? (int64_t)ix->region_form.size() : 0; }
const char *lsq_fe_index_chrom_name(const lsq_fe_index *ix, int64_t chrom) { return index_chrom_name(ix, chrom); }
const char *lsq_fe_index_event_name(const lsq_fe_index *ix, int64_t event) { return ix ? lsq_ps_index_event_name(ix->P.get(), event) : nullptr; }
const char *lsq_fe_index_form_name(const lsq_fe_index *ix, int64_t form) { return ix ? lsq_ps_index_form_name(ix->P.get(), form) : nullptr; }
lsq_events *lsq_fe_index_dictionaries(lsq_fe_index *ix) { return index_dictionaries(ix); }
int lsq_fe_index_arrays(const lsq_fe_index *ix, const uint32_t **event_first_form, const uint32_t **form_introns, const uint64_t **form_body) {
	if (!ix) return fail(LSQ_E_ARG, "null argument");
	if (event_first_form) *event_first_form = ix->P->event_first_form.data();
	if (form_introns) *form_introns = ix->P->form_introns.data();
	if (form_body) *form_body = ix->form_body.data();
	return LSQ_OK;
}
int lsq_fe_index_positions(const lsq_fe_index *ix, uint32_t read_length, uint32_t min_overhang, uint32_t min_body, uint64_t *positions) LSQ_API_TRY {
	if (!ix || (!positions && !ix->form_chrom.empty())) return fail(LSQ_E_ARG, "null argument");
	if (read_length < 1 || read_length > FE_MAX_READ_LENGTH) return fail(LSQ_E_ARG, "read_length must be at least 1 and below 2^18");
	if (!options_ok(min_overhang, min_body)) return LSQ_E_ARG;
	for (size_t f = 0; f < ix->form_chrom.size(); ++f) positions[f] = positions_of(*ix->G, (uint32_t)f, read_length, min_overhang, min_body);
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_fe_host_reads(lsq_fe_index *ix, const lsq_reads *r, uint32_t min_overhang, uint32_t min_body, int n_threads, lsq_fe_table **out) LSQ_API_TRY {
	if (!ix || !r || !out) return fail(LSQ_E_ARG, "null argument");
	if (!options_ok(min_overhang, min_body)) return LSQ_E_ARG;
	return new_table(out, [&](lsq_fe_table &t) { return fe_host_reads(*ix, host_view(*r), min_overhang, min_body, n_threads, t); });
} LSQ_API_CATCH

int lsq_fe_host(lsq_fe_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, uint32_t min_overhang, uint32_t min_body, int n_threads,
                lsq_fe_table **out) LSQ_API_TRY {
	if (!ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	if (!options_ok(min_overhang, min_body)) return LSQ_E_ARG;
	return host_file(ix->E, read_format, path, skip_flags, min_mapq, n_threads, [&](const lsq_reads *r) { return lsq_fe_host_reads(ix, r, min_overhang, min_body, n_threads, out); });
} LSQ_API_CATCH

void lsq_fe_table_free(lsq_fe_table *t) { delete t; }
int lsq_fe_table_arrays(const lsq_fe_table *t, const uint64_t **reads, const uint64_t **total) {
	if (!t) return fail(LSQ_E_ARG, "null argument");
	if (reads) *reads = t->reads.data();
	if (total) *total = t->total.data();
	return LSQ_OK;
}
int lsq_fe_table_report(const lsq_fe_table *t, uint64_t report[11]) { return table_report(t, report); }
int lsq_fe_table_library_report(const lsq_fe_table *t, uint64_t report[5]) { return table_library_report(t, report); }
int lsq_fe_table_times(const lsq_fe_table *t, float ms[3]) { return table_times(t, ms); }
int lsq_fe_table_psi(const lsq_fe_table *t, uint32_t read_length, double *psi) LSQ_API_TRY {
	if (!t || (!psi && !t->reads.empty())) return fail(LSQ_E_ARG, "null argument");
	if (read_length < 1 || read_length > FE_MAX_READ_LENGTH) return fail(LSQ_E_ARG, "read_length must be at least 1 and below 2^18");
	std::vector<uint64_t> pos;
	std::vector<double> v;
	positions_all(*t, read_length, pos);
	psi_of(*t, pos, v);
	if (!v.empty()) memcpy(psi, v.data(), v.size() * sizeof(double));
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_fe_format(const lsq_fe_table *t, int with_psi, uint32_t read_length, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	if (with_psi && (read_length < 1 || read_length > FE_MAX_READ_LENGTH)) return fail(LSQ_E_ARG, "read_length must be at least 1 and below 2^18");
	std::string o;
	char buf[160];
	std::vector<uint64_t> pos;
	std::vector<double> psi;
	if (with_psi) { positions_all(*t, read_length, pos); psi_of(*t, pos, psi); }
	for (size_t e = 0; e < t->event_name.size(); ++e)
		for (uint32_t f = t->event_first_form[e]; f < t->event_first_form[e + 1]; ++f) {
			o += t->event_name[e];
			snprintf(buf, sizeof buf, "\t%llu\t", (unsigned long long)t->total[e]);
			o += buf; o += t->form_name[f];
			snprintf(buf, sizeof buf, "\t%llu", (unsigned long long)t->reads[f]);
			o += buf;
			if (with_psi) {
				snprintf(buf, sizeof buf, "\t%u\t%llu\t%llu\t", t->form_introns[f], (unsigned long long)t->form_body[f], (unsigned long long)pos[f]);
				o += buf;
				if (std::isnan(psi[f])) o += "NA";
				else { snprintf(buf, sizeof buf, "%.6f", psi[f]); o += buf; }
			}
			o += '\n';
		}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

} // extern "C"

// evidence [--host] [--psi --read-length L] [--min-overhang N] [--min-body N] [--library unstranded|forward|reverse] <isoform_format> <isoforms_path> <g2i_format> <g2i_path> <read_format> <reads_path> [<out>]
// The table on standard output (or in <out>; "-": standard output), the report in the log.  Without --library the library type is
// LSQ_LIBRARY's (unstranded without either); a stranded run logs its library report behind the report.  Exit status 1, nothing on
// standard output and no file, for a file that does not open or parse, and for a stranded run over an event without a strand.
int lsq::run_evidence(int argc, const char *const *argv, std::string &out) {
	static const char *USAGE = "Usage:\nevidence [--host] [--psi --read-length L] [--min-overhang N] [--min-body N] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]";
	bool host = false, with_psi = false, bad = false, lib_given = false;
	int library = LSQ_LIBRARY_UNSTRANDED;
	unsigned long min_ov = 1, min_body = 1, L = 0;
	std::vector<const char *> pos;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (strcmp(argv[i], "--psi") == 0) with_psi = true;
		else if (strcmp(argv[i], "--min-overhang") == 0) bad = !cli_u32_option(argc, argv, i, min_ov);
		else if (strcmp(argv[i], "--min-body") == 0) bad = !cli_u32_option(argc, argv, i, min_body);
		else if (strcmp(argv[i], "--read-length") == 0) bad = !cli_u32_option(argc, argv, i, L) || L < 1 || L > FE_MAX_READ_LENGTH;
		else if (strcmp(argv[i], "--library") == 0) {
			if (i + 1 >= argc) bad = true;
			else if (!cli_library_option(argc, argv, i, library)) return 1;
			lib_given = true;
		} else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else pos.push_back(argv[i]);
	}
	if (bad || pos.size() < 6 || pos.size() > 7 || min_ov < 1 || min_body < 1 || (with_psi && L == 0)) { cli_log(0, USAGE); return 1; }
	if (!lib_given && !cli_library_env(library)) return 1;
	CliFrame F(pos);
	CliOwned<lsq_fe_index, lsq_fe_index_free> ix;
	CliOwned<lsq_fe_table, lsq_fe_table_free> t;
	int st = F.load_annotation();
	if (!st) st = lsq_fe_index_build_library(F.a, library, &ix.p);
	if (st) return cli_failed(st);
	if (host) {
		if (!(st = F.host_parse(&ix.p->E))) st = lsq_fe_host_reads(ix.p, F.reads, (uint32_t)min_ov, (uint32_t)min_body, 0, &t.p);
		F.free_reads();
	} else if (!(st = F.create_context())) st = lsq_fe_device(F.c, ix.p, pos[4], pos[5], (uint32_t)min_ov, (uint32_t)min_body, &t.p);
	if (!st) st = lsq_fe_format(t.p, with_psi ? 1 : 0, (uint32_t)L, &F.text[0]);
	if (st) return cli_failed(st);
	const uint64_t *rep = t.p->report;
	char msg[768];
	snprintf(msg, sizeof msg, "evidence: %llu read(s), %llu block(s), %llu junction occurrence(s), %llu block pair(s) below the overhang, %llu with a block on no chromosome of the annotation, "
	         "%llu block(s) skipped; %lld informative intron(s) and %lld body region(s) of %lld form(s) in %lld event(s): %llu occurrence(s) and %llu body hit(s) on them, "
	         "%llu read(s) counted, %llu for more than one event, %llu by body alone; min-overhang %lu, min-body %lu",
	         (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2], (unsigned long long)rep[3], (unsigned long long)rep[4], (unsigned long long)rep[6],
	         (long long)lsq_fe_index_num_introns(ix.p), (long long)lsq_fe_index_num_regions(ix.p), (long long)lsq_fe_index_num_forms(ix.p), (long long)lsq_fe_index_num_events(ix.p),
	         (unsigned long long)rep[5], (unsigned long long)rep[7], (unsigned long long)rep[8], (unsigned long long)rep[9], (unsigned long long)rep[10], min_ov, min_body);
	cli_log(2, msg);
	if (library != LSQ_LIBRARY_UNSTRANDED) cli_log_library("evidence", library, t.p->lib);
	return F.deliver(F.text[0], out);
}
