// The tables of lsq_events_upload, from compiled events alone (lsq_upload_tables.hpp).
#include "lsq_upload_tables.hpp"
#include "../../include/lesseq_hip_dev.h"

#include <algorithm>
#include <cstring>
#include <numeric>

namespace lsq {

EmPlacement em_placement(const lsq_events &E) {
	const size_t n_dev = E.dev2out.size();
	std::vector<bool> host_event(n_dev, false);
	for (const BucketDesc &bd : E.buckets) if (bd.kind == 2) for (uint32_t q = 0; q < bd.n_events; ++q) host_event[bd.ev_base + q] = true;
	EmPlacement P;
	P.order.reserve(n_dev + 32);
	for (int pass = 0; pass < 2; ++pass) {
		for (size_t d = 0; d < n_dev; ++d) {
			const int K = E.dev_K[d];
			if (host_event[d]) continue;            // solved on the host (host_solve)
			// (an isoform with ONE accessible start, G = 1: the general kernel's loop with the reference's own quotients,
			// lsq_em.hip em_quad_body)
			bool unit_g = false;
			for (int m = 0; m < E.n_methods; ++m) for (int j = 0; j < K; ++j) unit_g = unit_g || E.ev[E.dev2out[d]].ars[m][j] == 1;
			const bool small = K <= 2 && E.n_methods * ((1 << K) - 1) <= EM_LANES && !unit_g;
			if (small == (pass == 0)) P.order.push_back((uint32_t)d);
		}
		while (P.order.size() % (64 / EM_LANES)) P.order.push_back(0xFFFFFFFFu);
		if (pass == 0) P.small_places = (unsigned)P.order.size();
	}
	P.places = (unsigned)P.order.size();
	return P;
}

PackLists pack_lists(const lsq_events &E) {
	const size_t n_dev = E.dev2out.size();
	std::vector<uint32_t> order(n_dev);
	std::iota(order.begin(), order.end(), 0u);
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return E.dev2out[a] < E.dev2out[b]; });
	PackLists L;
	for (uint32_t dd : order) {
		const int K = E.dev_K[dd];
		for (uint32_t k = 0; k < (1u << K) - 1u; ++k) L.cls.push_back(E.dev_cls_base[dd] + k);
		for (int j = 0; j < K; ++j) L.iso.push_back(E.dev_iso_base[dd] + (uint32_t)j);
		L.ev.push_back(dd);
	}
	return L;
}

std::vector<double> start_weights(const lsq_events &E) {
	const size_t n_iso = E.n_iso_total, M = (size_t)E.n_methods;
	std::vector<double> G(M * n_iso, 0.0);
	for (size_t d = 0; d < E.dev2out.size(); ++d) {
		const Event &ev = E.ev[E.dev2out[d]];
		for (size_t m = 0; m < M; ++m)
			for (int j = 0; j < ev.K; ++j) {
				double nd = (double)ev.ars[m][j];
				G[m * n_iso + E.dev_iso_base[d] + j] = nd <= 0 ? 0.0 : (double)1.0 / nd;
			}
	}
	return G;
}

RouteHostTables route_host_tables(const lsq_events &E) {
	const size_t nc = E.covered.size();
	RouteHostTables T;
	T.n_chrom = (unsigned)nc;
	T.chrom.resize(std::max<size_t>(nc, 1));
	std::vector<RouteChrom> &chrom = T.chrom;
	std::vector<CovRec> &cov = T.cov;
	std::vector<CluRec> &clu = T.clu;
	for (size_t ch = 0; ch < nc; ++ch) {
		RouteChrom &R = chrom[ch];
		memset(&R, 0, sizeof(R));
		R.cov0 = (unsigned)cov.size();
		for (size_t q = 0; q < E.covered[ch].s.size(); ++q) cov.push_back({(int)E.covered[ch].s[q], (int)E.covered[ch].e[q]});
		R.cov1 = (unsigned)cov.size();
		R.clu0 = (unsigned)clu.size();
		// A cluster with the bucket of its bases.  Buckets are cut where no span crosses, so a cluster lies in one; the records are
		// cut at the bucket cuts all the same, and a stretch left of the chromosome's first cut (in no bucket) gets none: a
		// look-up of "the last record that starts at or left of p" then IS the bucket search and the cluster test of p.
		const int first = ch < E.chrom_first_bucket.size() ? E.chrom_first_bucket[ch] : -1;
		if (first >= 0 && ch < E.clu_s.size() && ch < E.cut_lo.size()) {
			const std::vector<int32_t> &cuts = E.cut_lo[ch];
			for (size_t q = 0; q < E.clu_s[ch].size(); ++q) {
				long long s = E.clu_s[ch][q];
				const long long e = E.clu_e[ch][q];           // (inclusive: a read whose first base is e is still inside)
				while (s <= e) {
					const size_t ub = (size_t)(std::upper_bound(cuts.begin(), cuts.end(), (int32_t)s) - cuts.begin());
					const long long next_cut = ub < cuts.size() ? (long long)cuts[ub] : e + 1;
					const long long stop = std::min(e, next_cut - 1);
					if (ub > 0) {
						const unsigned b = (unsigned)first + (unsigned)(ub - 1);
						clu.push_back({(int)s, (int)std::min<long long>(stop, E.buckets[b].hi), (int)b, E.buckets[b].lo});
					}
					s = stop + 1;
				}
			}
		}
		R.clu1 = (unsigned)clu.size();
	}
	// the locator: bins of 2^shift bases over each chromosome's range of starts (covered regions and cluster records), the
	// shift raised until all chromosomes together take at most 2^22 entries.  Entry k of a chromosome, for the bin's first
	// base x and the next bin's first base y: lower bounds of x and of y among the covered starts (.x, .y) and among the
	// cluster starts: entry k holds the lower bounds of x (.x covered, .y clusters), entry k + 1 those of y -- read as one
	// 16-byte pair, a search starts one load away from a handful of candidates; eight bytes a bin keep the bins of the
	// events (where the reads are) inside the L2.
	unsigned shift = 10;
	std::vector<long long> lo(nc, 0), hi(nc, -1);
	for (size_t ch = 0; ch < nc; ++ch) {
		bool any = false;
		auto see = [&](long long v) { if (!any) { lo[ch] = hi[ch] = v; any = true; } lo[ch] = std::min(lo[ch], v); hi[ch] = std::max(hi[ch], v); };
		for (unsigned q = chrom[ch].cov0; q < chrom[ch].cov1; ++q) see(cov[q].x);
		for (unsigned q = chrom[ch].clu0; q < chrom[ch].clu1; ++q) see(clu[q].x);
	}
	for (;; ++shift) {
		unsigned long long total = 0;
		for (size_t ch = 0; ch < nc; ++ch) if (hi[ch] >= lo[ch]) total += (unsigned long long)(((hi[ch] >> shift) - (lo[ch] >> shift)) + 2);
		if (total <= (1ull << 22) || shift >= 30) break;
	}
	std::vector<LocRec> &loc = T.loc;
	for (size_t ch = 0; ch < nc; ++ch) {
		RouteChrom &R = chrom[ch];
		R.loc_first = (unsigned)loc.size();
		if (hi[ch] < lo[ch]) continue;
		const long long base = (lo[ch] >> shift) << shift;          // (arithmetic shift: rounds towards minus infinity)
		const long long nb = ((hi[ch] - base) >> shift) + 1;
		R.loc_base = (int)base; R.loc_nb = (unsigned)nb;
		unsigned a = R.cov0, u = R.clu0;
		for (long long k = 0; k <= nb; ++k) {               // (nb + 1 entries: a bin's upper bounds are the next entry's lower bounds)
			const long long x = base + (k << shift);
			while (a < R.cov1 && cov[a].x < x) ++a;
			while (u < R.clu1 && clu[u].x < x) ++u;
			loc.push_back({a, u});
		}
	}
	loc.push_back({0, 0}); loc.push_back({0, 0});      // (an entry is read as a pair with its successor)
	if (cov.empty()) cov.push_back({0, 0});
	if (clu.empty()) clu.push_back({0, 0, 0, 0});
	T.shift = shift;
	return T;
}

GroupBases group_bases(const lsq_events &E) {
	const size_t B = E.buckets.size();
	GroupBases G;
	G.bin_base.assign(B + 1, 0);
	for (size_t b = 0; b < B; ++b) G.bin_base[b + 1] = G.bin_base[b] + E.buckets[b].n_bins;
	G.n_fine = G.bin_base.back();
	G.cell_base.assign(B + 1, 0);
	for (size_t b = 0; b < B; ++b) G.cell_base[b + 1] = G.cell_base[b] + (E.buckets[b].kind == 1 ? (E.buckets[b].iso_off & 0xFFFFu) : 0u) + 1u;
	G.n_cell_groups = G.cell_base.back();
	G.jgroup_base.assign(B + 1, 0);
	// the bucket's junction groups, then -- round 3 -- one group per cell (and one for "no cell") for the two-block reads
	// that cross no junction of the annotation: a quadruple of those shares the cell of its first record too
	for (size_t b = 0; b <= B; ++b) G.jgroup_base[b] = E.jg_base[b] + G.cell_base[b];
	G.n_junction_groups = G.jgroup_base.back();
	return G;
}

GeneNames gene_names(const lsq_events &E) {
	const size_t n_dev = E.dev2out.size();
	GeneNames N;
	N.off.assign(n_dev + 1, 0);
	for (size_t d = 0; d < n_dev; ++d) { N.blob += E.ev[E.dev2out[d]].gname; N.off[d + 1] = (uint32_t)N.blob.size(); }
	return N;
}

} // namespace lsq

// Developer view of those tables (include/lesseq_hip_dev.h says which is which): no context, no device
extern "C" int lsq_debug_upload_tables(const lsq_events *E, int which, void *out, unsigned long long cap, unsigned long long *n) LSQ_API_TRY {
	using namespace lsq;
	if (!E || !n || (cap && !out)) return fail(LSQ_E_ARG, "bad argument");
	if (E->jg_base.size() != E->buckets.size() + 1) return fail(LSQ_E_STATE, "the events carry no device plan");
	// at most `cap` of `count` values of `size` bytes each
	auto give = [&](const void *src, size_t count, size_t size) {
		*n = count;
		if (out && count) memcpy(out, src, (size_t)std::min<unsigned long long>(cap, count) * size);
		return LSQ_OK;
	};
	if (which == LSQ_UT_EM_ORDER || which == LSQ_UT_EM_PLACES) {
		const EmPlacement P = em_placement(*E);
		const uint32_t places[2] = {P.small_places, P.places};
		return which == LSQ_UT_EM_ORDER ? give(P.order.data(), P.order.size(), 4) : give(places, 2, 4);
	}
	if (which == LSQ_UT_PACK_CLS || which == LSQ_UT_PACK_ISO || which == LSQ_UT_PACK_EV) {
		const PackLists L = pack_lists(*E);
		const std::vector<uint32_t> &v = which == LSQ_UT_PACK_CLS ? L.cls : (which == LSQ_UT_PACK_ISO ? L.iso : L.ev);
		return give(v.data(), v.size(), 4);
	}
	if (which == LSQ_UT_START_WEIGHTS) { const std::vector<double> G = start_weights(*E); return give(G.data(), G.size(), 8); }
	if (which >= LSQ_UT_ROUTE_CHROM && which <= LSQ_UT_ROUTE_SHIFT) {
		const RouteHostTables T = route_host_tables(*E);
		const uint32_t word[2] = {T.shift, T.n_chrom};
		if (which == LSQ_UT_ROUTE_CHROM) return give(T.chrom.data(), 8 * T.chrom.size(), 4);
		if (which == LSQ_UT_ROUTE_COV) return give(T.cov.data(), 2 * T.cov.size(), 4);
		if (which == LSQ_UT_ROUTE_CLU) return give(T.clu.data(), 4 * T.clu.size(), 4);
		if (which == LSQ_UT_ROUTE_LOC) return give(T.loc.data(), 2 * T.loc.size(), 4);
		return give(word, 2, 4);
	}
	if (which >= LSQ_UT_BIN_BASE && which <= LSQ_UT_GROUP_TOTALS) {
		const GroupBases G = group_bases(*E);
		const uint32_t totals[3] = {(uint32_t)G.n_fine, (uint32_t)G.n_cell_groups, (uint32_t)G.n_junction_groups};
		if (which == LSQ_UT_GROUP_TOTALS) return give(totals, 3, 4);
		const std::vector<unsigned> &v = which == LSQ_UT_BIN_BASE ? G.bin_base : (which == LSQ_UT_CELL_BASE ? G.cell_base : G.jgroup_base);
		return give(v.data(), v.size(), 4);
	}
	if (which == LSQ_UT_GENE_NAMES || which == LSQ_UT_GENE_NAME_OFF) {
		const GeneNames N = gene_names(*E);
		return which == LSQ_UT_GENE_NAMES ? give(N.blob.data(), N.blob.size(), 1) : give(N.off.data(), N.off.size(), 4);
	}
	if (which == LSQ_UT_BUCKET_BINS) {
		std::vector<uint32_t> nb;
		for (const BucketDesc &bd : E->buckets) nb.push_back(bd.n_bins);
		return give(nb.data(), nb.size(), 4);
	}
	if (which == LSQ_UT_JG_BASE) return give(E->jg_base.data(), E->jg_base.size(), 4);
	return fail(LSQ_E_ARG, "no such table: %d", which);
} LSQ_API_CATCH
