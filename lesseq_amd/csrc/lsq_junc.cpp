// Splice junctions of a read file (include/lesseq_hip.h, lsq_jn_*): the index made from an annotation, the host
// path over the host parsers' arrays, the table's text and the junctions executable.  The device passes are lsq_junc.hip, the
// entry that opens a read file on the device is lsq_readfile.hip's lsq_jn_device; what the tool shares with coverage and
// exonbins is lsq_readtool.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "lsq_junc.hpp"

using namespace lsq;

namespace {

struct Row { uint32_t chrom; uint64_t key; uint32_t reads, plus, minus, max_ov; };
inline bool row_less(const Row &a, const Row &b) { return a.chrom != b.chrom ? a.chrom < b.chrom : a.key < b.key; }

// sorted rows with equal keys -> one row each
void fold_rows(std::vector<Row> &v) {
	size_t o = 0;
	for (size_t i = 0; i < v.size(); ++i) {
		if (o && v[o - 1].chrom == v[i].chrom && v[o - 1].key == v[i].key) {
			Row &r = v[o - 1];
			r.reads += v[i].reads; r.plus += v[i].plus; r.minus += v[i].minus; r.max_ov = std::max(r.max_ov, v[i].max_ov);
		} else v[o++] = v[i];
	}
	v.resize(o);
}

} // namespace

void lsq::jn_finish_table(const lsq_jn_index &ix, lsq_jn_table &t) {
	t.chrom_names = ix.E.chroms.names;
	const size_t n = t.chrom.size();
	// rows arrive ascending in (chromosome index, start, end)
	const std::vector<size_t> from = rows_by_chrom_name(t.chrom_names, t.chrom);
	auto permute = [&](auto &v) { auto w = v; for (size_t i = 0; i < n; ++i) w[i] = v[from[i]]; v.swap(w); };
	permute(t.chrom); permute(t.start); permute(t.end); permute(t.ann); permute(t.reads); permute(t.plus); permute(t.minus); permute(t.max_overhang);
}

int lsq::jn_host_reads(const lsq_jn_index &ix, const ParsedReads &R, uint32_t min_overhang, int n_threads, lsq_jn_table &t) {
	const int T = read_slices(R.n_reads, n_threads);
	std::vector<std::vector<Row>> part((size_t)T);
	std::vector<uint64_t> dropped((size_t)T, 0), nochrom((size_t)T, 0), occ((size_t)T, 0);
	const int rc = for_read_slices(R.n_reads, T, [&](int k, uint64_t r0, uint64_t r1) {
		std::vector<Row> &v = part[(size_t)k];
		for (uint64_t r = r0; r < r1; ++r)
			for (uint64_t b = R.blk_off[r]; b + 1 < R.blk_off[r + 1]; ++b) {
				const unsigned c0 = R.bc[b], c1 = R.bc[b + 1];
				if (c0 == NO_CHROM || c1 == NO_CHROM) { ++nochrom[(size_t)k]; continue; }
				if (c0 != c1 || R.bs[b + 1] <= R.be[b]) continue;
				const int64_t ov = std::min((int64_t)R.be[b] - R.bs[b], (int64_t)R.be[b + 1] - R.bs[b + 1]);
				if (ov < (int64_t)min_overhang) { ++dropped[(size_t)k]; continue; }
				v.push_back(Row{c0, jn_key(R.be[b], R.bs[b + 1]), 1u, R.bst[b] == 0 ? 1u : 0u, R.bst[b] == 1 ? 1u : 0u, (uint32_t)ov});
			}
		occ[(size_t)k] = v.size();
		std::sort(v.begin(), v.end(), row_less);
		fold_rows(v);
	});
	if (rc) return rc;
	uint64_t n_occ = 0;
	for (uint64_t o : occ) n_occ += o;
	if (n_occ > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32-1 junction occurrences");
	const std::vector<Row> all = merge_folded(part, row_less, fold_rows);
	t.resize(all.size());
	for (size_t i = 0; i < all.size(); ++i) {
		const Row &r = all[i];
		t.chrom[i] = r.chrom; t.start[i] = jn_key_start(r.key); t.end[i] = jn_key_end(r.key);
		t.reads[i] = r.reads; t.plus[i] = r.plus; t.minus[i] = r.minus; t.max_overhang[i] = r.max_ov;
		size_t lo = 0, hi = ix.in_key.size();
		while (lo < hi) {
			const size_t mid = lo + (hi - lo) / 2;
			if (ix.in_chrom[mid] < r.chrom || (ix.in_chrom[mid] == r.chrom && ix.in_key[mid] < r.key)) lo = mid + 1; else hi = mid;
		}
		t.ann[i] = (lo < ix.in_key.size() && ix.in_chrom[lo] == r.chrom && ix.in_key[lo] == r.key) ? ix.in_ann[lo] : (uint8_t)'.';
	}
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks; t.report[2] = n_occ; t.report[3] = t.report[4] = 0;
	for (int k = 0; k < T; ++k) { t.report[3] += dropped[(size_t)k]; t.report[4] += nochrom[(size_t)k]; }
	for (float &m : t.ms) m = 0;
	jn_finish_table(ix, t);
	return LSQ_OK;
}

extern "C" {

int lsq_jn_index_build(const lsq_annotation *a, lsq_jn_index **out) LSQ_API_TRY {
	if (!a || !out) return fail(LSQ_E_ARG, "null argument");
	std::unique_ptr<lsq_jn_index> ix(new lsq_jn_index);
	lsq_events &E = ix->E;
	int rc;
	if ((rc = annotation_dictionaries(*a, E))) return rc;
	struct Intron { uint32_t chrom; uint64_t key; uint8_t ann; };
	std::vector<Intron> in;
	std::vector<std::pair<int64_t, int64_t>> ex, gaps;
	for (const auto &rp : a->recs) {
		const IsoRec &r = *rp;
		const int cid = E.chroms.find(r.chrom);
		// the union of the line's exons: its maximal intervals, and the gaps between them
		gaps.clear();
		line_introns(r, ex, gaps);
		const uint8_t ann = r.strand == "+" ? '+' : r.strand == "-" ? '-' : '*';
		for (const auto &g : gaps) in.push_back(Intron{(uint32_t)cid, jn_key(g.first, g.second), ann});
	}
	std::sort(in.begin(), in.end(), [](const Intron &x, const Intron &y) { return x.chrom != y.chrom ? x.chrom < y.chrom : x.key < y.key; });
	for (const Intron &i : in) {
		if (!ix->in_key.empty() && ix->in_chrom.back() == i.chrom && ix->in_key.back() == i.key) {
			if (ix->in_ann.back() != i.ann) ix->in_ann.back() = '*';
		} else { ix->in_chrom.push_back(i.chrom); ix->in_key.push_back(i.key); ix->in_ann.push_back(i.ann); }
	}
	*out = ix.release();
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_jn_index_free(lsq_jn_index *ix) { delete ix; }
int64_t lsq_jn_index_num_chroms(const lsq_jn_index *ix) { return index_num_chroms(ix); }
const char *lsq_jn_index_chrom_name(const lsq_jn_index *ix, int64_t chrom) { return index_chrom_name(ix, chrom); }
lsq_events *lsq_jn_index_dictionaries(lsq_jn_index *ix) { return index_dictionaries(ix); }
int64_t lsq_jn_index_num_introns(const lsq_jn_index *ix) { return ix ? (int64_t)ix->in_key.size() : 0; }

int lsq_jn_host_reads(lsq_jn_index *ix, const lsq_reads *r, uint32_t min_overhang, int n_threads, lsq_jn_table **out) LSQ_API_TRY {
	if (!ix || !r || !out) return fail(LSQ_E_ARG, "null argument");
	if (min_overhang < 1) return fail(LSQ_E_ARG, "min_overhang must be at least 1");
	return new_table(out, [&](lsq_jn_table &t) { return jn_host_reads(*ix, host_view(*r), min_overhang, n_threads, t); });
} LSQ_API_CATCH

int lsq_jn_host(lsq_jn_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, uint32_t min_overhang, int n_threads,
                lsq_jn_table **out) LSQ_API_TRY {
	if (!ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	if (min_overhang < 1) return fail(LSQ_E_ARG, "min_overhang must be at least 1");
	return host_file(ix->E, read_format, path, skip_flags, min_mapq, n_threads, [&](const lsq_reads *r) { return lsq_jn_host_reads(ix, r, min_overhang, n_threads, out); });
} LSQ_API_CATCH

void lsq_jn_table_free(lsq_jn_table *t) { delete t; }
int64_t lsq_jn_table_rows(const lsq_jn_table *t) { return t ? (int64_t)t->chrom.size() : 0; }
int lsq_jn_table_arrays(const lsq_jn_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint8_t **ann,
                        const uint32_t **reads, const uint32_t **plus, const uint32_t **minus, const uint32_t **max_overhang) {
	if (!t) return fail(LSQ_E_ARG, "null argument");
	if (chrom) *chrom = t->chrom.data();
	if (start) *start = t->start.data();
	if (end) *end = t->end.data();
	if (ann) *ann = t->ann.data();
	if (reads) *reads = t->reads.data();
	if (plus) *plus = t->plus.data();
	if (minus) *minus = t->minus.data();
	if (max_overhang) *max_overhang = t->max_overhang.data();
	return LSQ_OK;
}
int lsq_jn_table_report(const lsq_jn_table *t, uint64_t report[5]) { return table_report(t, report); }
int lsq_jn_table_times(const lsq_jn_table *t, float ms[5]) { return table_times(t, ms); }

int lsq_jn_format(const lsq_jn_table *t, uint32_t min_reads, int novel_only, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	char buf[96];
	for (size_t i = 0; i < t->chrom.size(); ++i) {
		if (t->reads[i] < min_reads || (novel_only && t->ann[i] != '.')) continue;
		o += t->chrom_names[t->chrom[i]];
		snprintf(buf, sizeof buf, "\t%lld\t%lld\t%c\t%u\t%u\t%u\t%u\n", (long long)t->start[i] + 1, (long long)t->end[i], (char)t->ann[i], t->reads[i], t->plus[i], t->minus[i], t->max_overhang[i]);
		o += buf;
	}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

} // extern "C"

// junctions [--host] [--min-overhang N] [--min-reads N] [--novel] <isoform_format> <isoforms_path> <g2i_format> <g2i_path>
//           <read_format> <reads_path> [<out>]
// The table on standard output (or in <out>; "-": standard output), the report in the log.  Exit status 1, nothing on standard
// output, for a file that does not open or parse.
int lsq::run_junctions(int argc, const char *const *argv, std::string &out) {
	static const char *USAGE = "Usage:\njunctions [--host] [--min-overhang N] [--min-reads N] [--novel] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]";
	bool host = false, novel = false, bad = false;
	unsigned long min_ov = 1, min_reads = 0;
	std::vector<const char *> pos;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (strcmp(argv[i], "--novel") == 0) novel = true;
		else if (strcmp(argv[i], "--min-overhang") == 0) bad = !cli_u32_option(argc, argv, i, min_ov);
		else if (strcmp(argv[i], "--min-reads") == 0) bad = !cli_u32_option(argc, argv, i, min_reads);
		else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else pos.push_back(argv[i]);
	}
	if (bad || pos.size() < 6 || pos.size() > 7 || min_ov < 1) { cli_log(0, USAGE); return 1; }
	CliFrame F(pos);
	CliOwned<lsq_jn_index, lsq_jn_index_free> ix;
	CliOwned<lsq_jn_table, lsq_jn_table_free> t;
	int st = F.load_annotation();
	if (!st) st = lsq_jn_index_build(F.a, &ix.p);
	if (st) return cli_failed(st);
	if (host) {
		if (!(st = F.host_parse(&ix.p->E))) st = lsq_jn_host_reads(ix.p, F.reads, (uint32_t)min_ov, 0, &t.p);
		F.free_reads();
	} else if (!(st = F.create_context())) st = lsq_jn_device(F.c, ix.p, pos[4], pos[5], (uint32_t)min_ov, &t.p);
	if (!st) st = lsq_jn_format(t.p, (uint32_t)min_reads, novel ? 1 : 0, &F.text[0]);
	if (st) return cli_failed(st);
	char msg[256];
	snprintf(msg, sizeof msg, "junctions: %llu read(s), %llu block(s), %llu occurrence(s) of %lld junction(s); %llu block pair(s) below the overhang, %llu with a block on no chromosome of the annotation",
	         (unsigned long long)t.p->report[0], (unsigned long long)t.p->report[1], (unsigned long long)t.p->report[2], (long long)lsq_jn_table_rows(t.p),
	         (unsigned long long)t.p->report[3], (unsigned long long)t.p->report[4]);
	cli_log(1, msg);
	return F.deliver(F.text[0], out);
}
