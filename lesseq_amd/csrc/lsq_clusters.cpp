// Intron clusters of several read files (include/lesseq_hip.h, lsq_cl_*): the pool of the samples' junction rows, the
// reader of the text `junctions` prints, the host path (a sort, then a union-find), and what both paths share behind their
// components -- singletons and weak clusters, `ann`, the table's order, the numbering, the two texts -- and the clusters
// executable.  The device passes are lsq_clusters.hip; the junction rows per read file are lsq_junc.cpp's and lsq_junc.hip's.
// No HIP in this unit.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "lsq_clusters.hpp"

using namespace lsq;

namespace {

constexpr int64_t LIM = JN_BIAS;

// One sample's rows checked as a whole, then appended: a sample that fails leaves the pool as it was
int pool_add(lsq_cl_pool &p, size_t n, const uint32_t *chrom, const int32_t *start, const int32_t *end, const uint32_t *reads) {
	if (p.n_samples >= CL_MAX_SAMPLES) return fail(LSQ_E_RANGE, "more than 65 535 samples");
	uint64_t sum = 0;
	for (size_t i = 0; i < n; ++i) {
		if (chrom[i] >= p.chrom_names.size()) return fail(LSQ_E_ARG, "row %zu: chromosome %u out of range", i, chrom[i]);
		if (start[i] >= end[i]) return fail(LSQ_E_ARG, "row %zu: start %d is not below end %d", i, start[i], end[i]);
		if (start[i] <= -LIM || end[i] >= LIM) return fail(LSQ_E_RANGE, "row %zu: a coordinate outside (-2^30, 2^30)", i);
		sum += reads[i];
	}
	// (so that no cell of the count matrix, and no cluster's total in one sample, leaves 32 bits however rows repeat)
	if (sum > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "the reads of one sample's rows sum beyond 2^32-1");
	if (p.key.size() + n > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32-1 pooled rows");
	const size_t at = p.key.size();
	p.key.resize(at + n); p.rec.resize(at + n);
	for (size_t i = 0; i < n; ++i) {
		const uint64_t a = jn_key(start[i], end[i]), b = cl_rec(chrom[i], p.n_samples, reads[i]);
		p.key[at + i] = a; p.rec[at + i] = b;
		p.any[0] |= a; p.any[1] |= b; p.all[0] &= a; p.all[1] &= b;
	}
	++p.n_samples;
	return LSQ_OK;
}

// A field of a `junctions` line as a number: decimal digits (a sign only where `is_signed`), nothing else, inside [lo, hi]
bool text_number(const char *b, const char *e, bool is_signed, int64_t lo, int64_t hi, int64_t &v) {
	const char *p = b;
	bool neg = false;
	if (is_signed && p < e && *p == '-') { neg = true; ++p; }
	if (p == e || e - p > 18) return false;
	int64_t x = 0;
	for (; p < e; ++p) { if (*p < '0' || *p > '9') return false; x = x * 10 + (*p - '0'); }
	v = neg ? -x : x;
	return v >= lo && v <= hi;
}

struct PoolRow { uint16_t chrom, sample; uint32_t reads; uint64_t key; };
inline bool pool_row_less(const PoolRow &a, const PoolRow &b) { return a.chrom != b.chrom ? a.chrom < b.chrom : a.key < b.key; }

struct UnionFind {
	std::vector<uint32_t> parent;
	explicit UnionFind(size_t n) : parent(n) { std::iota(parent.begin(), parent.end(), 0u); }
	uint32_t find(uint32_t x) {
		uint32_t r = x;
		while (parent[r] != r) r = parent[r];
		while (parent[x] != r) { const uint32_t nx = parent[x]; parent[x] = r; x = nx; }
		return r;
	}
	// the smaller root stays a root: a set's root is its smallest member
	void unite(uint32_t a, uint32_t b) {
		a = find(a); b = find(b);
		if (a != b) parent[std::max(a, b)] = std::min(a, b);
	}
};

// The host path: the pooled rows sorted by (chromosome index, key) -- slices on threads of their own, then merged --, equal keys
// folded into the distinct introns and the count matrix, the two row filters, and a union-find over the kept rows: neighbours with
// one (chromosome, start) in this order, neighbours with one (chromosome, end) in a second order of the kept rows
int host_solve(const lsq_cl_pool &p, uint64_t min_reads, uint32_t max_intron, int n_threads, ClSolved &S) {
	const size_t np = p.key.size(), ns = p.n_samples;
	std::vector<PoolRow> rows(np);
	for (size_t i = 0; i < np; ++i) rows[i] = PoolRow{(uint16_t)(p.rec[i] >> CL_CHROM_SHIFT), (uint16_t)(p.rec[i] >> 32), (uint32_t)p.rec[i], p.key[i]};
	const int T = np < (1u << 16) ? 1 : host_threads(n_threads);
	{
		ThreadGroup th;
		for (int k = 0; k < T; ++k) th.spawn([&rows, np, k, T] { std::sort(rows.begin() + (ptrdiff_t)(np * (size_t)k / (size_t)T), rows.begin() + (ptrdiff_t)(np * (size_t)(k + 1) / (size_t)T), pool_row_less); });
		th.join();
		if (th.failed()) return fail(LSQ_E_INTERNAL, "%s", th.error().c_str());
	}
	for (int k = 1; k < T; ++k)
		std::inplace_merge(rows.begin(), rows.begin() + (ptrdiff_t)(np * (size_t)k / (size_t)T), rows.begin() + (ptrdiff_t)(np * (size_t)(k + 1) / (size_t)T), pool_row_less);
	size_t n = 0;
	for (size_t i = 0; i < np; ++i) if (!i || pool_row_less(rows[i - 1], rows[i])) ++n;
	if ((uint64_t)n * ns > CL_MAX_CELLS) return fail(LSQ_E_RANGE, "%zu introns x %zu samples: more than 2^31 cells in the count matrix", n, ns);
	S.resize(n, ns);
	std::fill(S.counts.begin(), S.counts.end(), 0u);
	size_t j = 0;
	for (size_t i = 0; i < np; ++i) {
		if (!i || pool_row_less(rows[i - 1], rows[i])) { j = i ? j + 1 : 0; S.chrom[j] = rows[i].chrom; S.key[j] = rows[i].key; S.reads[j] = 0; S.samples[j] = 0; }
		uint32_t &cell = S.counts[j * ns + rows[i].sample];
		if (!cell && rows[i].reads) ++S.samples[j];
		cell += rows[i].reads;
		S.reads[j] += rows[i].reads;
	}
	std::vector<uint32_t> kept;
	for (size_t r = 0; r < n; ++r) {
		S.status[r] = cl_long(jn_key_start(S.key[r]), jn_key_end(S.key[r]), max_intron) ? CL_LONG_ROW : S.reads[r] < min_reads ? CL_WEAK_ROW : CL_PRINTED;
		if (S.status[r] == CL_PRINTED) kept.push_back((uint32_t)r);
	}
	const size_t nk = kept.size();
	UnionFind U(nk);
	for (size_t k = 1; k < nk; ++k) {
		const uint32_t a = kept[k - 1], b = kept[k];
		if (S.chrom[a] == S.chrom[b] && jn_key_start(S.key[a]) == jn_key_start(S.key[b])) U.unite((uint32_t)(k - 1), (uint32_t)k);
	}
	std::vector<uint32_t> by_end(nk);
	std::iota(by_end.begin(), by_end.end(), 0u);
	auto end_of = [&](uint32_t k) { return std::make_pair(S.chrom[kept[k]], jn_key_end(S.key[kept[k]])); };
	std::stable_sort(by_end.begin(), by_end.end(), [&](uint32_t a, uint32_t b) { return end_of(a) < end_of(b); });
	for (size_t q = 1; q < nk; ++q) if (end_of(by_end[q - 1]) == end_of(by_end[q])) U.unite(by_end[q - 1], by_end[q]);
	std::fill(S.root.begin(), S.root.end(), CL_NONE);
	std::fill(S.comp_size.begin(), S.comp_size.end(), 0u);
	std::fill(S.comp_slot.begin(), S.comp_slot.end(), CL_NONE);
	std::fill(S.comp_reads.begin(), S.comp_reads.end(), 0ull);
	for (size_t k = 0; k < nk; ++k) {
		const uint32_t r = kept[U.find((uint32_t)k)];
		S.root[kept[k]] = r; ++S.comp_size[r]; S.comp_reads[r] += S.reads[kept[k]];
	}
	uint32_t n_slots = 0;
	for (size_t k = 0; k < nk; ++k) if (S.root[kept[k]] == kept[k] && S.comp_size[kept[k]] >= 2) S.comp_slot[kept[k]] = n_slots++;
	S.slot_totals.assign((size_t)n_slots * ns, 0u);
	for (size_t k = 0; k < nk; ++k) {
		const uint32_t slot = S.comp_slot[S.root[kept[k]]];
		if (slot != CL_NONE) for (size_t s = 0; s < ns; ++s) S.slot_totals[(size_t)slot * ns + s] += S.counts[(size_t)kept[k] * ns + s];
	}
	return LSQ_OK;
}

int check_solve_args(const void *p, const void *out, uint32_t max_intron) {
	if (!p || !out) return fail(LSQ_E_ARG, "null argument");
	if ((int64_t)max_intron >= 2 * LIM) return fail(LSQ_E_ARG, "max_intron must be below 2^31");
	return LSQ_OK;
}

} // namespace

int lsq::cl_check_pool(const lsq_cl_pool &p) {
	return p.key.size() > 0xFFFFFFFFull ? fail(LSQ_E_RANGE, "more than 2^32-1 pooled rows") : LSQ_OK;
}

int lsq::cl_finish_table(const lsq_cl_pool &p, ClSolved &S, uint64_t min_cluster_reads, lsq_cl_table &t) {
	const size_t n = S.chrom.size(), ns = p.n_samples;
	uint64_t n_long = 0, n_weak = 0, n_kept = 0, n_comp = 0, n_single = 0, n_weak_clusters = 0;
	for (size_t j = 0; j < n; ++j) {
		if (S.status[j] == CL_LONG_ROW) { ++n_long; continue; }
		if (S.status[j] == CL_WEAK_ROW) { ++n_weak; continue; }
		++n_kept;
		const uint32_t r = S.root[j];
		const bool single = S.comp_size[r] == 1, weak = !single && S.comp_reads[r] < min_cluster_reads;
		if (r == j) { ++n_comp; n_single += single; n_weak_clusters += weak; }
		if (single) S.status[j] = CL_SINGLETON; else if (weak) S.status[j] = CL_WEAK_CLUSTER;
	}
	t.chrom_names = p.chrom_names;
	t.n_samples = p.n_samples;
	const std::vector<size_t> from = rows_by_chrom_name(t.chrom_names, S.chrom);
	t.chrom.resize(n); t.start.resize(n); t.end.resize(n); t.ann.resize(n); t.reads.resize(n); t.samples.resize(n); t.cluster.assign(n, 0u); t.status.resize(n);
	t.counts.resize(n * ns);
	t.printed.clear(); t.totals.clear();
	// a cluster lies on one chromosome, whose rows keep their order: its root is its first row in the table's order too
	std::vector<uint32_t> number(n, 0u);
	uint32_t n_clusters = 0;
	for (size_t i = 0; i < n; ++i) {
		const size_t f = from[i];
		const uint32_t c = S.chrom[f];
		const uint64_t key = S.key[f];
		t.chrom[i] = c; t.start[i] = jn_key_start(key); t.end[i] = jn_key_end(key); t.reads[i] = S.reads[f]; t.samples[i] = S.samples[f]; t.status[i] = S.status[f];
		size_t lo = 0, hi = p.in_key.size();
		while (lo < hi) {
			const size_t mid = lo + (hi - lo) / 2;
			if (p.in_chrom[mid] < c || (p.in_chrom[mid] == c && p.in_key[mid] < key)) lo = mid + 1; else hi = mid;
		}
		t.ann[i] = (lo < p.in_key.size() && p.in_chrom[lo] == c && p.in_key[lo] == key) ? p.in_ann[lo] : (uint8_t)'.';
		if (ns) memcpy(&t.counts[i * ns], &S.counts[f * ns], ns * sizeof(uint32_t));
		if (S.status[f] != CL_PRINTED) continue;
		if (S.root[f] == f) {
			number[f] = ++n_clusters;
			const uint32_t *tot = &S.slot_totals[(size_t)S.comp_slot[f] * ns];
			t.totals.insert(t.totals.end(), tot, tot + ns);
		}
		t.cluster[i] = number[S.root[f]];
		t.printed.push_back((uint32_t)i);
	}
	std::stable_sort(t.printed.begin(), t.printed.end(), [&](uint32_t a, uint32_t b) { return t.cluster[a] < t.cluster[b]; });
	const uint64_t rep[CL_REPORT] = {ns, p.key.size(), n, n_long, n_weak, n_kept, n_comp, n_single, n_weak_clusters, n_clusters, t.printed.size()};
	memcpy(t.report, rep, sizeof rep);
	return LSQ_OK;
}

extern "C" {

int lsq_cl_pool_create(const lsq_jn_index *ix, lsq_cl_pool **out) LSQ_API_TRY {
	if (!ix || !out) return fail(LSQ_E_ARG, "null argument");
	std::unique_ptr<lsq_cl_pool> p(new lsq_cl_pool);
	p->chrom_names = ix->E.chroms.names;
	p->in_chrom = ix->in_chrom; p->in_key = ix->in_key; p->in_ann = ix->in_ann;
	*out = p.release();
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_cl_pool_free(lsq_cl_pool *p) { delete p; }
int64_t lsq_cl_pool_samples(const lsq_cl_pool *p) { return p ? (int64_t)p->n_samples : 0; }
int64_t lsq_cl_pool_rows(const lsq_cl_pool *p) { return p ? (int64_t)p->key.size() : 0; }

int lsq_cl_pool_add_rows(lsq_cl_pool *p, uint64_t n, const uint32_t *chrom, const int32_t *start, const int32_t *end, const uint32_t *reads) LSQ_API_TRY {
	if (!p || (n && (!chrom || !start || !end || !reads))) return fail(LSQ_E_ARG, "null argument");
	return pool_add(*p, (size_t)n, chrom, start, end, reads);
} LSQ_API_CATCH

int lsq_cl_pool_add_table(lsq_cl_pool *p, const lsq_jn_table *t) LSQ_API_TRY {
	if (!p || !t) return fail(LSQ_E_ARG, "null argument");
	if (t->chrom_names != p->chrom_names) return fail(LSQ_E_ARG, "the junction table was made under another annotation's chromosomes");
	return pool_add(*p, t->chrom.size(), t->chrom.data(), t->start.data(), t->end.data(), t->reads.data());
} LSQ_API_CATCH

int lsq_cl_pool_add_text(lsq_cl_pool *p, const char *path) LSQ_API_TRY {
	if (!p || !path) return fail(LSQ_E_ARG, "null argument");
	FILE *fp = fopen(path, "rb");
	if (!fp) return fail(LSQ_E_IO, "cannot open %s", path);
	std::string text;
	char buf[1 << 16];
	size_t got;
	while ((got = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, got);
	const bool read_error = ferror(fp) != 0;
	fclose(fp);
	if (read_error) return fail(LSQ_E_IO, "cannot read %s", path);
	std::unordered_map<std::string, uint32_t> ids;
	for (size_t c = 0; c < p->chrom_names.size(); ++c) ids.emplace(p->chrom_names[c], (uint32_t)c);
	std::vector<uint32_t> chrom, reads;
	std::vector<int32_t> start, end;
	size_t line_no = 0;
	for (size_t at = 0; at < text.size();) {
		size_t nl = text.find('\n', at);
		if (nl == std::string::npos) nl = text.size();
		++line_no;
		const char *b = text.data() + at, *e = text.data() + nl;
		at = nl + 1;
		// chrom, first base, last base, ann, reads, plus, minus, max_overhang
		const char *f[9];
		int nf = 0;
		f[nf++] = b;
		for (const char *q = b; q < e && nf < 9; ++q) if (*q == '\t') f[nf++] = q + 1;
		bool ok = nf == 8 && memchr(f[7], '\t', (size_t)(e - f[7])) == nullptr;
		int64_t first = 0, last = 0, v[4] = {0, 0, 0, 0};
		uint32_t cid = 0;
		if (ok) {
			f[8] = e + 1;
			const auto it = ids.find(std::string(f[0], (size_t)(f[1] - 1 - f[0])));
			ok = it != ids.end() && text_number(f[1], f[2] - 1, true, -LIM + 2, LIM - 1, first) && text_number(f[2], f[3] - 1, true, -LIM + 2, LIM - 1, last) && first <= last &&
			     f[4] - 1 - f[3] == 1 && strchr(".+-*", *f[3]) != nullptr && *f[3];
			for (int k = 0; ok && k < 4; ++k) ok = text_number(f[4 + k], f[5 + k] - 1, false, 0, 0xFFFFFFFFll, v[k]);
			if (ok) cid = it->second;
		}
		if (!ok) return fail(LSQ_E_PARSE, "%s: #%zu:%s", path, line_no, std::string(b, (size_t)(e - b)).c_str());
		chrom.push_back(cid); start.push_back((int32_t)(first - 1)); end.push_back((int32_t)last); reads.push_back((uint32_t)v[0]);
	}
	return pool_add(*p, chrom.size(), chrom.data(), start.data(), end.data(), reads.data());
} LSQ_API_CATCH

int lsq_cl_host(const lsq_cl_pool *p, uint64_t min_reads, uint32_t max_intron, uint64_t min_cluster_reads, int n_threads, lsq_cl_table **out) LSQ_API_TRY {
	int rc = check_solve_args(p, out, max_intron);
	if (rc || (rc = cl_check_pool(*p))) return rc;
	return new_table(out, [&](lsq_cl_table &t) {
		ClSolved S;
		const int st = host_solve(*p, min_reads, max_intron, n_threads, S);
		return st ? st : cl_finish_table(*p, S, min_cluster_reads, t);
	});
} LSQ_API_CATCH

void lsq_cl_table_free(lsq_cl_table *t) { delete t; }
int64_t lsq_cl_table_rows(const lsq_cl_table *t) { return t ? (int64_t)t->chrom.size() : 0; }
int64_t lsq_cl_table_samples(const lsq_cl_table *t) { return t ? (int64_t)t->n_samples : 0; }
int64_t lsq_cl_table_rounds(const lsq_cl_table *t) { return t ? (int64_t)t->rounds : 0; }
const char *lsq_cl_table_chrom_name(const lsq_cl_table *t, int64_t chrom) {
	return t && chrom >= 0 && (size_t)chrom < t->chrom_names.size() ? t->chrom_names[(size_t)chrom].c_str() : nullptr;
}
int lsq_cl_table_arrays(const lsq_cl_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint8_t **ann, const uint64_t **reads,
                        const uint32_t **samples, const uint32_t **cluster, const uint8_t **status) {
	if (!t) return fail(LSQ_E_ARG, "null argument");
	if (chrom) *chrom = t->chrom.data();
	if (start) *start = t->start.data();
	if (end) *end = t->end.data();
	if (ann) *ann = t->ann.data();
	if (reads) *reads = t->reads.data();
	if (samples) *samples = t->samples.data();
	if (cluster) *cluster = t->cluster.data();
	if (status) *status = t->status.data();
	return LSQ_OK;
}
int lsq_cl_table_counts(const lsq_cl_table *t, const uint32_t **counts) {
	if (!t || !counts) return fail(LSQ_E_ARG, "null argument");
	*counts = t->counts.data();
	return LSQ_OK;
}
int lsq_cl_table_report(const lsq_cl_table *t, uint64_t report[11]) { return table_report(t, report); }
int lsq_cl_table_times(const lsq_cl_table *t, float ms[8]) { return table_times(t, ms); }

int lsq_cl_format(const lsq_cl_table *t, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	char buf[128];
	for (uint32_t i : t->printed) {
		snprintf(buf, sizeof buf, "clu_%u\t", t->cluster[i]);
		o += buf;
		o += t->chrom_names[t->chrom[i]];
		snprintf(buf, sizeof buf, "\t%lld\t%lld\t%c\t%llu\t%u\n", (long long)t->start[i] + 1, (long long)t->end[i], (char)t->ann[i], (unsigned long long)t->reads[i], t->samples[i]);
		o += buf;
	}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

int lsq_cl_format_sample(const lsq_cl_table *t, int64_t sample, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	if (sample < 0 || sample >= (int64_t)t->n_samples) return fail(LSQ_E_ARG, "sample %lld out of range", (long long)sample);
	const size_t ns = t->n_samples, k = (size_t)sample;
	std::string o;
	char buf[128];
	for (uint32_t i : t->printed) {
		snprintf(buf, sizeof buf, "clu_%u\t%u\t", t->cluster[i], t->totals[(size_t)(t->cluster[i] - 1) * ns + k]);
		o += buf;
		o += t->chrom_names[t->chrom[i]];
		snprintf(buf, sizeof buf, ":%lld:%lld\t%u\n", (long long)t->start[i] + 1, (long long)t->end[i], t->counts[(size_t)i * ns + k]);
		o += buf;
	}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

} // extern "C"

// clusters [--host] [--min-overhang N] [--min-reads N] [--max-intron L] [--min-cluster-reads N] <isoform_format> <isoforms_path>
//          <g2i_format> <g2i_path> <read_format> <out_prefix> <reads_1> [<reads_2> ...]
// clusters [--host] [--min-reads N] [--max-intron L] [--min-cluster-reads N] --tables <isoform_format> <isoforms_path> <g2i_format>
//          <g2i_path> <out_prefix> <junctions_1> [<junctions_2> ...]
// <out_prefix>.clusters.tab and <out_prefix>.<k>.tab (k = 1 ..: the samples in argument order), written once every file has been
// read and the clusters are made; with <out_prefix> "-" the cluster table on standard output and no file.  The report in the log.
// Exit status 1, nothing written, for a file that does not open or parse: the message names the file.  The frame's positional
// arguments end with the annotation here, so the reads go through cli_host_parse and lsq_jn_device file by file.
int lsq::run_clusters(int argc, const char *const *argv, std::string &out) {
	static const char *USAGE = "Usage:\nclusters [--host] [--min-overhang N] [--min-reads N] [--max-intron L] [--min-cluster-reads N] isoform_format isoforms_path g2i_format g2i_path "
	                           "read_format out_prefix reads_path_1 [reads_path_2 ...]\n"
	                           "clusters [--host] [--min-reads N] [--max-intron L] [--min-cluster-reads N] --tables isoform_format isoforms_path g2i_format g2i_path "
	                           "out_prefix junctions_path_1 [junctions_path_2 ...]";
	bool host = false, tables = false, bad = false, have_ov = false;
	unsigned long min_ov = 1, min_reads = 1, max_intron = 100000, min_cluster = 30;
	std::vector<const char *> pos;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (strcmp(argv[i], "--tables") == 0) tables = true;
		else if (strcmp(argv[i], "--min-overhang") == 0) { bad = !cli_u32_option(argc, argv, i, min_ov); have_ov = true; }
		else if (strcmp(argv[i], "--min-reads") == 0) bad = !cli_u32_option(argc, argv, i, min_reads);
		else if (strcmp(argv[i], "--max-intron") == 0) bad = !cli_u32_option(argc, argv, i, max_intron);
		else if (strcmp(argv[i], "--min-cluster-reads") == 0) bad = !cli_u32_option(argc, argv, i, min_cluster);
		else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else pos.push_back(argv[i]);
	}
	const size_t first_file = tables ? 5 : 6;
	if (bad || pos.size() <= first_file || min_ov < 1 || (tables && have_ov) || max_intron > 0x7FFFFFFFul || pos.size() - first_file > CL_MAX_SAMPLES) { cli_log(0, USAGE); return 1; }
	const char *prefix = pos[first_file - 1];
	CliFrame F(pos);
	CliOwned<lsq_jn_index, lsq_jn_index_free> ix;
	CliOwned<lsq_cl_pool, lsq_cl_pool_free> pool;
	CliOwned<lsq_cl_table, lsq_cl_table_free> t;
	int st = F.load_annotation();
	if (!st) st = lsq_jn_index_build(F.a, &ix.p);
	if (!st) st = lsq_cl_pool_create(ix.p, &pool.p);
	if (!st && !host) st = F.create_context();
	if (st) return cli_failed(st);
	for (size_t k = first_file; k < pos.size(); ++k) {
		if (tables) st = lsq_cl_pool_add_text(pool.p, pos[k]);
		else {
			// one file at a time: its parsed arrays (host) or its staged text and device arrays (lsq_jn_device) are gone before the next
			CliOwned<lsq_jn_table, lsq_jn_table_free> jt;
			if (host) {
				if (!(st = cli_host_parse(&ix.p->E, pos[4], pos[k], &F.reads))) st = lsq_jn_host_reads(ix.p, F.reads, (uint32_t)min_ov, 0, &jt.p);
				F.free_reads();
			} else st = lsq_jn_device(F.c, ix.p, pos[4], pos[k], (uint32_t)min_ov, &jt.p);
			if (st) { const std::string text = lsq_last_error(); fail(st, "%s: %s", pos[k], text.c_str()); }
			else st = lsq_cl_pool_add_table(pool.p, jt.p);
		}
		if (st) return cli_failed(st);
	}
	st = host ? lsq_cl_host(pool.p, min_reads, (uint32_t)max_intron, min_cluster, 0, &t.p) : lsq_cl_device(F.c, pool.p, min_reads, (uint32_t)max_intron, min_cluster, &t.p);
	if (st) return cli_failed(st);
	const size_t ns = t.p->n_samples;
	struct Texts { std::vector<char *> v; ~Texts() { for (char *x : v) lsq_free(x); } } texts;
	texts.v.assign(ns + 1, nullptr);
	st = lsq_cl_format(t.p, &texts.v[0]);
	const bool files = strcmp(prefix, "-") != 0;
	for (size_t k = 0; !st && files && k < ns; ++k) st = lsq_cl_format_sample(t.p, (int64_t)k, &texts.v[k + 1]);
	if (st) return cli_failed(st);
	const uint64_t *rep = t.p->report;
	char msg[512];
	snprintf(msg, sizeof msg, "clusters: %llu sample(s), %llu pooled row(s), %llu distinct intron(s); %llu long, %llu weak, %llu kept; %llu component(s), %llu singleton(s), "
	         "%llu weak cluster(s); %llu cluster(s) of %llu row(s) printed",
	         (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2], (unsigned long long)rep[3], (unsigned long long)rep[4], (unsigned long long)rep[5],
	         (unsigned long long)rep[6], (unsigned long long)rep[7], (unsigned long long)rep[8], (unsigned long long)rep[9], (unsigned long long)rep[10]);
	cli_log(1, msg);
	if (!files) { out = texts.v[0]; return 0; }
	std::vector<std::string> paths{std::string(prefix) + ".clusters.tab"};
	for (size_t k = 1; k <= ns; ++k) paths.push_back(std::string(prefix) + "." + std::to_string(k) + ".tab");
	for (size_t k = 0; k < paths.size(); ++k) if (!write_file(paths[k].c_str(), texts.v[k])) {
		for (size_t q = 0; q <= k; ++q) remove(paths[q].c_str());       // all files or none
		return cli_failed(LSQ_E_IO);
	}
	return 0;
}
