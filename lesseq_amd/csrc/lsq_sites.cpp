// Splice-site usage and read-through per junction of a read file (include/lesseq_hip.h, lsq_ss_*): the index (the
// junction index), the merge of junction rows with annotated introns and the boundary arrays both paths count against, the host
// path over the host parsers' arrays, the table's text and the sites executable.  The device count is lsq_sites.hip, the entry
// that opens a read file on the device is lsq_readfile.hip's lsq_ss_device; the junction rows are lsq_junc.cpp's and
// lsq_junc.hip's, what the tool shares with the other read-file tools is lsq_readtool.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "lsq_sites.hpp"

using namespace lsq;

int lsq::ss_plan(const lsq_ss_index &ix, const lsq_jn_table &jt, SsPlan &P) {
	const lsq_jn_index &J = *ix.J;
	const size_t nc = J.E.covered.size();
	struct Row { uint32_t chrom; uint64_t key; uint8_t ann; uint64_t reads; };
	std::vector<Row> rows;
	rows.reserve(jt.chrom.size() + J.in_key.size());
	for (size_t i = 0; i < jt.chrom.size(); ++i) rows.push_back(Row{jt.chrom[i], jn_key(jt.start[i], jt.end[i]), jt.ann[i], jt.reads[i]});
	for (size_t i = 0; i < J.in_key.size(); ++i) rows.push_back(Row{J.in_chrom[i], J.in_key[i], J.in_ann[i], 0});
	// (a junction the annotation has comes twice, with one ann: the intron's row adds nothing to it)
	std::sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.chrom != b.chrom ? a.chrom < b.chrom : a.key < b.key; });
	size_t n = 0;
	for (size_t i = 0; i < rows.size(); ++i) {
		if (n && rows[n - 1].chrom == rows[i].chrom && rows[n - 1].key == rows[i].key) rows[n - 1].reads += rows[i].reads;
		else rows[n++] = rows[i];
	}
	rows.resize(n);
	P.chrom.resize(n); P.start.resize(n); P.end.resize(n); P.ann.resize(n); P.reads.resize(n); P.row_left.resize(n); P.row_right.resize(n);
	P.chrom_first_boundary.assign(nc + 1, 0);
	P.pos.clear();
	std::vector<int32_t> cut;
	for (size_t i = 0; i < n;) {                            // a chromosome's rows: its boundaries, then the rows' places among them
		const uint32_t c = rows[i].chrom;
		size_t j = i;
		cut.clear();
		for (; j < n && rows[j].chrom == c; ++j) { cut.push_back(jn_key_start(rows[j].key)); cut.push_back(jn_key_end(rows[j].key)); }
		std::sort(cut.begin(), cut.end());
		cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
		const size_t first = P.pos.size();
		if (first + cut.size() >= 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32-2 splice-site boundaries");
		P.pos.insert(P.pos.end(), cut.begin(), cut.end());
		for (size_t k = i; k < j; ++k) {
			const Row &r = rows[k];
			P.chrom[k] = c; P.start[k] = jn_key_start(r.key); P.end[k] = jn_key_end(r.key); P.ann[k] = r.ann; P.reads[k] = r.reads;
			P.row_left[k] = (uint32_t)(first + (size_t)(std::lower_bound(cut.begin(), cut.end(), P.start[k]) - cut.begin()));
			P.row_right[k] = (uint32_t)(first + (size_t)(std::lower_bound(cut.begin(), cut.end(), P.end[k]) - cut.begin()));
		}
		P.chrom_first_boundary[c + 1] = (uint32_t)P.pos.size();
		i = j;
	}
	for (size_t c = 0; c < nc; ++c) P.chrom_first_boundary[c + 1] = std::max(P.chrom_first_boundary[c + 1], P.chrom_first_boundary[c]);      // a chromosome without a row
	return LSQ_OK;
}

void lsq::ss_finish_table(const lsq_ss_index &ix, const SsPlan &P, const std::vector<uint64_t> &through, const lsq_jn_table &jt, lsq_ss_table &t) {
	const size_t n = P.chrom.size(), nb = P.pos.size();
	// the spliced reads of a boundary as a left end and as a right end: two sums, the place may be both
	std::vector<uint64_t> as_left(nb, 0), as_right(nb, 0);
	for (size_t i = 0; i < n; ++i) { as_left[P.row_left[i]] += P.reads[i]; as_right[P.row_right[i]] += P.reads[i]; }
	t.chrom_names = ix.E.chroms.names;
	const std::vector<size_t> from = rows_by_chrom_name(t.chrom_names, P.chrom);
	t.chrom.resize(n); t.start.resize(n); t.end.resize(n); t.ann.resize(n);
	t.reads.resize(n); t.left_spliced.resize(n); t.left_through.resize(n); t.right_spliced.resize(n); t.right_through.resize(n);
	uint64_t unsupported = 0, sum = 0;
	for (size_t i = 0; i < n; ++i) {
		const size_t f = from[i];
		t.chrom[i] = P.chrom[f]; t.start[i] = P.start[f]; t.end[i] = P.end[f]; t.ann[i] = P.ann[f]; t.reads[i] = P.reads[f];
		t.left_spliced[i] = as_left[P.row_left[f]]; t.left_through[i] = through[P.row_left[f]];
		t.right_spliced[i] = as_right[P.row_right[f]]; t.right_through[i] = through[P.row_right[f]];
		if (!P.reads[f]) ++unsupported;
	}
	for (uint64_t v : through) sum += v;
	for (int k = 0; k < 5; ++k) t.report[k] = jt.report[k];
	t.report[5] = nb; t.report[6] = sum; t.report[7] = unsupported;
}

// The junction rows by lsq_junc.cpp's host path, then a thread a stretch of reads with boundary counters of its own: per block
// a binary search for the first boundary at or behind s + m and a walk up to e - m
int lsq::ss_host_reads(const lsq_ss_index &ix, const ParsedReads &R, uint32_t min_overhang, int n_threads, lsq_ss_table &t) {
	lsq_jn_table jt;
	SsPlan P;
	int rc;
	if ((rc = jn_host_reads(*ix.J, R, min_overhang, n_threads, jt)) || (rc = ss_plan(ix, jt, P))) return rc;
	const int T = read_slices(R.n_reads, n_threads);
	const size_t nb = P.pos.size(), nc = ix.E.covered.size();
	const int64_t m = (int64_t)ss_through_overhang(min_overhang);
	std::vector<std::vector<uint64_t>> part((size_t)T);
	rc = for_read_slices(R.n_reads, T, [&](int k, uint64_t r0, uint64_t r1) {
		std::vector<uint64_t> &cnt = part[(size_t)k];
		cnt.assign(nb, 0);
		for (uint64_t b = r0 < r1 ? R.blk_off[r0] : 0, b1 = r0 < r1 ? R.blk_off[r1] : 0; b < b1; ++b) {      // (every block on its own, whatever read it belongs to)
			const unsigned c = R.bc[b];
			const int64_t lo = (int64_t)R.bs[b] + m, hi = (int64_t)R.be[b] - m;
			if (c == NO_CHROM || c >= nc || lo > hi) continue;
			const int32_t *p0 = P.pos.data() + P.chrom_first_boundary[c], *p1 = P.pos.data() + P.chrom_first_boundary[c + 1];
			for (const int32_t *p = std::lower_bound(p0, p1, lo, [](int32_t x, int64_t v) { return x < v; }); p < p1 && *p <= hi; ++p) ++cnt[(size_t)(p - P.pos.data())];
		}
	});
	if (rc) return rc;
	std::vector<uint64_t> through(nb, 0);
	for (int k = 0; k < T; ++k) for (size_t b = 0; b < nb; ++b) through[b] += part[(size_t)k][b];
	ss_finish_table(ix, P, through, jt, t);
	return LSQ_OK;
}

extern "C" {

int lsq_ss_index_build(const lsq_annotation *a, lsq_ss_index **out) LSQ_API_TRY {
	if (!a || !out) return fail(LSQ_E_ARG, "null argument");
	lsq_jn_index *j = nullptr;
	const int rc = lsq_jn_index_build(a, &j);
	if (rc) return rc;
	std::unique_ptr<lsq_jn_index, void (*)(lsq_jn_index *)> hold(j, lsq_jn_index_free);
	lsq_ss_index *ix = new lsq_ss_index(j);
	hold.release();
	*out = ix;
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_ss_index_free(lsq_ss_index *ix) { delete ix; }
int64_t lsq_ss_index_num_chroms(const lsq_ss_index *ix) { return index_num_chroms(ix); }
const char *lsq_ss_index_chrom_name(const lsq_ss_index *ix, int64_t chrom) { return index_chrom_name(ix, chrom); }
lsq_events *lsq_ss_index_dictionaries(lsq_ss_index *ix) { return index_dictionaries(ix); }
int64_t lsq_ss_index_num_introns(const lsq_ss_index *ix) { return ix ? lsq_jn_index_num_introns(ix->J) : 0; }

int lsq_ss_host_reads(lsq_ss_index *ix, const lsq_reads *r, uint32_t min_overhang, int n_threads, lsq_ss_table **out) LSQ_API_TRY {
	if (!ix || !r || !out) return fail(LSQ_E_ARG, "null argument");
	return new_table(out, [&](lsq_ss_table &t) { return ss_host_reads(*ix, host_view(*r), min_overhang, n_threads, t); });
} LSQ_API_CATCH

int lsq_ss_host(lsq_ss_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, uint32_t min_overhang, int n_threads,
                lsq_ss_table **out) LSQ_API_TRY {
	if (!ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	return host_file(ix->E, read_format, path, skip_flags, min_mapq, n_threads, [&](const lsq_reads *r) { return lsq_ss_host_reads(ix, r, min_overhang, n_threads, out); });
} LSQ_API_CATCH

void lsq_ss_table_free(lsq_ss_table *t) { delete t; }
int64_t lsq_ss_table_rows(const lsq_ss_table *t) { return t ? (int64_t)t->chrom.size() : 0; }
int lsq_ss_table_arrays(const lsq_ss_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint8_t **ann, const uint64_t **reads,
                        const uint64_t **left_spliced, const uint64_t **left_through, const uint64_t **right_spliced, const uint64_t **right_through) {
	if (!t) return fail(LSQ_E_ARG, "null argument");
	if (chrom) *chrom = t->chrom.data();
	if (start) *start = t->start.data();
	if (end) *end = t->end.data();
	if (ann) *ann = t->ann.data();
	if (reads) *reads = t->reads.data();
	if (left_spliced) *left_spliced = t->left_spliced.data();
	if (left_through) *left_through = t->left_through.data();
	if (right_spliced) *right_spliced = t->right_spliced.data();
	if (right_through) *right_through = t->right_through.data();
	return LSQ_OK;
}
int lsq_ss_table_report(const lsq_ss_table *t, uint64_t report[8]) { return table_report(t, report); }
int lsq_ss_table_times(const lsq_ss_table *t, float ms[4]) { return table_times(t, ms); }

int lsq_ss_format(const lsq_ss_table *t, uint32_t min_reads, int novel_only, int ratios, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	char buf[192];
	auto ratio = [&](uint64_t num, uint64_t den) {
		if (!den) { o += "\tNA"; return; }
		snprintf(buf, sizeof buf, "\t%.6f", (double)num / (double)den);
		o += buf;
	};
	for (size_t i = 0; i < t->chrom.size(); ++i) {
		if (t->reads[i] < min_reads || (novel_only && t->ann[i] != '.')) continue;
		const uint64_t ls = t->left_spliced[i], lt = t->left_through[i], rs = t->right_spliced[i], rt = t->right_through[i];
		o += t->chrom_names[t->chrom[i]];
		snprintf(buf, sizeof buf, "\t%lld\t%lld\t%c\t%llu\t%llu\t%llu\t%llu\t%llu", (long long)t->start[i] + 1, (long long)t->end[i], (char)t->ann[i], (unsigned long long)t->reads[i],
		         (unsigned long long)ls, (unsigned long long)lt, (unsigned long long)rs, (unsigned long long)rt);
		o += buf;
		if (ratios) { ratio(t->reads[i], ls); ratio(t->reads[i], rs); ratio(ls, ls + lt); ratio(rs, rs + rt); }
		o += '\n';
	}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

} // extern "C"

// sites [--host] [--ratios] [--min-overhang N] [--min-reads N] [--novel] <isoform_format> <isoforms_path> <g2i_format> <g2i_path>
//       <read_format> <reads_path> [<out>]
// The table on standard output (or in <out>; "-": standard output), the report in the log.  Exit status 1, nothing on standard
// output, for a file that does not open or parse.  --min-overhang 0 is taken: the junction rule then asks nothing of the flanks,
// the through count asks one base on either side as it does for 1.
int lsq::run_sites(int argc, const char *const *argv, std::string &out) {
	static const char *USAGE = "Usage:\nsites [--host] [--ratios] [--min-overhang N] [--min-reads N] [--novel] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]";
	bool host = false, novel = false, ratios = false, bad = false;
	unsigned long min_ov = 1, min_reads = 0;
	std::vector<const char *> pos;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (strcmp(argv[i], "--novel") == 0) novel = true;
		else if (strcmp(argv[i], "--ratios") == 0) ratios = true;
		else if (strcmp(argv[i], "--min-overhang") == 0) bad = !cli_u32_option(argc, argv, i, min_ov);
		else if (strcmp(argv[i], "--min-reads") == 0) bad = !cli_u32_option(argc, argv, i, min_reads);
		else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else pos.push_back(argv[i]);
	}
	if (bad || pos.size() < 6 || pos.size() > 7) { cli_log(0, USAGE); return 1; }
	CliFrame F(pos);
	CliOwned<lsq_ss_index, lsq_ss_index_free> ix;
	CliOwned<lsq_ss_table, lsq_ss_table_free> t;
	int st = F.load_annotation();
	if (!st) st = lsq_ss_index_build(F.a, &ix.p);
	if (st) return cli_failed(st);
	if (host) {
		if (!(st = F.host_parse(&ix.p->E))) st = lsq_ss_host_reads(ix.p, F.reads, (uint32_t)min_ov, 0, &t.p);
		F.free_reads();
	} else if (!(st = F.create_context())) st = lsq_ss_device(F.c, ix.p, pos[4], pos[5], (uint32_t)min_ov, &t.p);
	if (!st) st = lsq_ss_format(t.p, (uint32_t)min_reads, novel ? 1 : 0, ratios ? 1 : 0, &F.text[0]);
	if (st) return cli_failed(st);
	const uint64_t *rep = t.p->report;
	char msg[512];
	snprintf(msg, sizeof msg, "sites: %llu read(s), %llu block(s), %llu occurrence(s) of junctions; %llu block pair(s) below the overhang, %llu with a block on no chromosome of the annotation; "
	         "%lld row(s), %llu without a spliced read; %llu boundary(ies), %llu block(s) through one",
	         (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2], (unsigned long long)rep[3], (unsigned long long)rep[4],
	         (long long)lsq_ss_table_rows(t.p), (unsigned long long)rep[7], (unsigned long long)rep[5], (unsigned long long)rep[6]);
	cli_log(1, msg);
	return F.deliver(F.text[0], out);
}
