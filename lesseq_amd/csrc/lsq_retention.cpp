// Intron retention of a read file (include/lesseq_hip.h, lsq_ir_*): the index (the sites index and every
// chromosome's exon union), the introns' clean pieces both paths select over, the host path over the host parsers' arrays, the
// table's text and the retention executable.  The device selection is lsq_retention.hip, the entry that opens a read file on the
// device is lsq_readfile.hip's lsq_ir_device; the sites rows are lsq_sites.cpp's, the depth rows lsq_cov.cpp's and lsq_cov.hip's.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "lsq_retention.hpp"

using namespace lsq;

int lsq::ir_rows_and_pieces(const lsq_ir_index &ix, const lsq_ss_table &st, lsq_ir_table &t, IrPieces &P) {
	t.chrom_names = st.chrom_names;
	P.piece_off.assign(1, 0);
	uint64_t no_clean = 0;
	for (size_t i = 0; i < st.chrom.size(); ++i) {
		if (st.ann[i] == '.') continue;
		const uint32_t c = st.chrom[i];
		const int32_t a = st.start[i], b = st.end[i];
		t.chrom.push_back(c); t.start.push_back(a); t.end.push_back(b); t.ann.push_back(st.ann[i]); t.reads.push_back(st.reads[i]);
		t.left_spliced.push_back(st.left_spliced[i]); t.left_through.push_back(st.left_through[i]);
		t.right_spliced.push_back(st.right_spliced[i]); t.right_through.push_back(st.right_through[i]);
		// [a, b) less the chromosome's exons: the first exon that ends behind a, then every one that begins ahead of b
		const int32_t *s0 = ix.ex_s.data() + ix.ex_off[c], *e0 = ix.ex_e.data() + ix.ex_off[c];
		const size_t ne = (size_t)(ix.ex_off[c + 1] - ix.ex_off[c]);
		uint64_t clean = 0;
		int32_t at = a;
		for (size_t k = (size_t)(std::upper_bound(e0, e0 + ne, a) - e0); k < ne && s0[k] < b; ++k) {
			if (s0[k] > at) { P.chrom.push_back(c); P.start.push_back(at); P.end.push_back(s0[k]); clean += (uint64_t)((int64_t)s0[k] - at); }
			at = std::max(at, e0[k]);
		}
		if (at < b) { P.chrom.push_back(c); P.start.push_back(at); P.end.push_back(b); clean += (uint64_t)((int64_t)b - at); }
		if (P.chrom.size() >= 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32-2 intron pieces");
		P.piece_off.push_back((uint32_t)P.chrom.size());
		t.clean.push_back(clean);
		if (!clean) ++no_clean;
	}
	const size_t n = t.chrom.size();
	t.covered.assign(n, 0); t.depth_sum.assign(n, 0); t.q25.assign(n, 0); t.q50.assign(n, 0); t.q75.assign(n, 0);
	for (int k = 0; k < SS_REPORT; ++k) t.report[k] = st.report[k];
	t.report[8] = n; t.report[9] = no_clean; t.report[10] = P.chrom.size(); t.report[11] = 0; t.report[12] = 0;
	return LSQ_OK;
}

// The sites table and the depth rows by their host paths; per intron the (depth, bases) pairs of the rows its pieces overlap,
// sorted by depth, and a walk up to each rank behind the zeros
int lsq::ir_host_reads(const lsq_ir_index &ix, const ParsedReads &R, uint32_t min_overhang, int n_threads, lsq_ir_table &t) {
	lsq_ss_table st;
	lsq_cov_table ct;
	IrPieces P;
	int rc;
	if ((rc = ss_host_reads(*ix.S, R, min_overhang, n_threads, st)) || (rc = cov_host_reads(ix.C, R, 0, 1, n_threads, ct)) || (rc = ir_rows_and_pieces(ix, st, t, P))) return rc;
	t.report[11] = ct.chrom.size(); t.report[12] = ct.report[6];
	// (the depth rows come in the order of the chromosomes' names: a chromosome's rows are one stretch, ascending)
	const size_t nc = ix.E.covered.size(), nr = ct.chrom.size();
	std::vector<size_t> first(nc, 0), last(nc, 0);
	for (size_t r = 0; r < nr; ++r) {
		const uint32_t c = ct.chrom[r];
		if (r == 0 || ct.chrom[r - 1] != c) first[c] = r;
		last[c] = r + 1;
	}
	std::vector<std::pair<uint32_t, uint64_t>> runs;
	for (size_t i = 0; i < t.chrom.size(); ++i) {
		runs.clear();
		uint64_t covered = 0, sum = 0;
		for (uint32_t p = P.piece_off[i]; p < P.piece_off[i + 1]; ++p) {
			const uint32_t c = P.chrom[p];
			const int32_t s = P.start[p], e = P.end[p];
			const int32_t *e0 = ct.end.data();
			for (size_t k = (size_t)(std::upper_bound(e0 + first[c], e0 + last[c], s) - e0); k < last[c] && ct.start[k] < e; ++k) {
				const uint64_t ov = (uint64_t)((int64_t)std::min(e, ct.end[k]) - std::max(s, ct.start[k]));
				runs.emplace_back(ct.depth[k], ov);
				covered += ov; sum += ov * ct.depth[k];
			}
		}
		t.covered[i] = covered; t.depth_sum[i] = sum;
		if (!t.clean[i]) continue;
		std::sort(runs.begin(), runs.end());
		uint32_t *q[3] = {&t.q25[i], &t.q50[i], &t.q75[i]};
		uint64_t below = t.clean[i] - covered;                // the bases ahead of runs[at]: the zeros first
		size_t at = 0;
		for (unsigned k = 0; k < 3; ++k) {                    // (the ranks ascend: the walk goes on where it stood)
			const uint64_t rank = ir_rank(k + 1, t.clean[i]);
			while (below < rank) below += runs[at++].second;
			*q[k] = at ? runs[at - 1].first : 0u;
		}
	}
	for (float &m : t.ms) m = 0;
	return LSQ_OK;
}

extern "C" {

int lsq_ir_index_build(const lsq_annotation *a, lsq_ir_index **out) LSQ_API_TRY {
	if (!a || !out) return fail(LSQ_E_ARG, "null argument");
	lsq_ss_index *s = nullptr;
	int rc = lsq_ss_index_build(a, &s);
	if (rc) return rc;
	std::unique_ptr<lsq_ir_index> ix(new lsq_ir_index(s));
	if ((rc = annotation_dictionaries(*a, ix->C.E))) return rc;
	ix->C.iv_off.push_back(0);
	const size_t nc = ix->E.covered.size();
	constexpr int64_t LIM = (int64_t)1 << 30;
	std::vector<std::vector<std::pair<int64_t, int64_t>>> of_chrom(nc);
	std::vector<std::pair<int64_t, int64_t>> ex;
	for (const auto &rp : a->recs) {
		ex.clear();
		exon_union(*rp, ex);
		std::vector<std::pair<int64_t, int64_t>> &v = of_chrom[(size_t)ix->E.chroms.find(rp->chrom)];
		v.insert(v.end(), ex.begin(), ex.end());
	}
	ix->ex_off.assign(1, 0);
	for (std::vector<std::pair<int64_t, int64_t>> &v : of_chrom) {
		std::sort(v.begin(), v.end());
		const size_t held = ix->ex_s.size();
		for (const auto &x : v) {
			const int64_t s0 = std::max(x.first, -LIM), e0 = std::min(x.second, LIM);
			if (e0 <= s0) continue;
			if (ix->ex_s.size() > held && s0 <= ix->ex_e.back()) ix->ex_e.back() = std::max<int32_t>(ix->ex_e.back(), (int32_t)e0);
			else { ix->ex_s.push_back((int32_t)s0); ix->ex_e.push_back((int32_t)e0); }
		}
		ix->ex_off.push_back(ix->ex_s.size());
	}
	*out = ix.release();
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_ir_index_free(lsq_ir_index *ix) { delete ix; }
int64_t lsq_ir_index_num_chroms(const lsq_ir_index *ix) { return index_num_chroms(ix); }
const char *lsq_ir_index_chrom_name(const lsq_ir_index *ix, int64_t chrom) { return index_chrom_name(ix, chrom); }
lsq_events *lsq_ir_index_dictionaries(lsq_ir_index *ix) { return index_dictionaries(ix); }
int64_t lsq_ir_index_num_introns(const lsq_ir_index *ix) { return ix ? lsq_ss_index_num_introns(ix->S) : 0; }

int lsq_ir_host_reads(lsq_ir_index *ix, const lsq_reads *r, uint32_t min_overhang, int n_threads, lsq_ir_table **out) LSQ_API_TRY {
	if (!ix || !r || !out) return fail(LSQ_E_ARG, "null argument");
	return new_table(out, [&](lsq_ir_table &t) { return ir_host_reads(*ix, host_view(*r), min_overhang, n_threads, t); });
} LSQ_API_CATCH

int lsq_ir_host(lsq_ir_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, uint32_t min_overhang, int n_threads,
                lsq_ir_table **out) LSQ_API_TRY {
	if (!ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	return host_file(ix->E, read_format, path, skip_flags, min_mapq, n_threads, [&](const lsq_reads *r) { return lsq_ir_host_reads(ix, r, min_overhang, n_threads, out); });
} LSQ_API_CATCH

void lsq_ir_table_free(lsq_ir_table *t) { delete t; }
int64_t lsq_ir_table_rows(const lsq_ir_table *t) { return t ? (int64_t)t->chrom.size() : 0; }
int lsq_ir_table_arrays(const lsq_ir_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint8_t **ann, const uint64_t **reads,
                        const uint64_t **left_spliced, const uint64_t **left_through, const uint64_t **right_spliced, const uint64_t **right_through,
                        const uint64_t **clean, const uint64_t **covered, const uint64_t **depth_sum, const uint32_t **q25, const uint32_t **q50, const uint32_t **q75) {
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
	if (clean) *clean = t->clean.data();
	if (covered) *covered = t->covered.data();
	if (depth_sum) *depth_sum = t->depth_sum.data();
	if (q25) *q25 = t->q25.data();
	if (q50) *q50 = t->q50.data();
	if (q75) *q75 = t->q75.data();
	return LSQ_OK;
}
int lsq_ir_table_report(const lsq_ir_table *t, uint64_t report[13]) { return table_report(t, report); }
int lsq_ir_table_times(const lsq_ir_table *t, float ms[5]) { return table_times(t, ms); }

int lsq_ir_format(const lsq_ir_table *t, int ratios, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	char buf[320];
	auto ratio = [&](uint64_t num, uint64_t den) {
		if (!den) { o += "\tNA"; return; }
		snprintf(buf, sizeof buf, "\t%.6f", (double)num / (double)den);
		o += buf;
	};
	for (size_t i = 0; i < t->chrom.size(); ++i) {
		o += t->chrom_names[t->chrom[i]];
		snprintf(buf, sizeof buf, "\t%lld\t%lld\t%c\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%u\t%u\t%u", (long long)t->start[i] + 1, (long long)t->end[i], (char)t->ann[i],
		         (unsigned long long)t->reads[i], (unsigned long long)t->left_spliced[i], (unsigned long long)t->left_through[i], (unsigned long long)t->right_spliced[i],
		         (unsigned long long)t->right_through[i], (unsigned long long)t->clean[i], (unsigned long long)t->covered[i], (unsigned long long)t->depth_sum[i],
		         t->q25[i], t->q50[i], t->q75[i]);
		o += buf;
		if (ratios) {
			ratio(t->depth_sum[i], t->clean[i]); ratio(t->covered[i], t->clean[i]);
			if (t->clean[i]) ratio(t->q50[i], (uint64_t)t->q50[i] + std::max(t->left_spliced[i], t->right_spliced[i])); else o += "\tNA";
		}
		o += '\n';
	}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

} // extern "C"

// retention [--host] [--ratios] [--min-overhang N] <isoform_format> <isoforms_path> <g2i_format> <g2i_path> <read_format> <reads_path> [<out>]
// The table on standard output (or in <out>; "-": standard output), the report in the log.  Exit status 1, nothing on standard
// output, for a file that does not open or parse.  --min-overhang is sites': it bears on columns 5-9, the depth does not depend on it.
int lsq::run_retention(int argc, const char *const *argv, std::string &out) {
	static const char *USAGE = "Usage:\nretention [--host] [--ratios] [--min-overhang N] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]";
	bool host = false, ratios = false, bad = false;
	unsigned long min_ov = 1;
	std::vector<const char *> pos;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (strcmp(argv[i], "--ratios") == 0) ratios = true;
		else if (strcmp(argv[i], "--min-overhang") == 0) bad = !cli_u32_option(argc, argv, i, min_ov);
		else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else pos.push_back(argv[i]);
	}
	if (bad || pos.size() < 6 || pos.size() > 7) { cli_log(0, USAGE); return 1; }
	CliFrame F(pos);
	CliOwned<lsq_ir_index, lsq_ir_index_free> ix;
	CliOwned<lsq_ir_table, lsq_ir_table_free> t;
	int st = F.load_annotation();
	if (!st) st = lsq_ir_index_build(F.a, &ix.p);
	if (st) return cli_failed(st);
	if (host) {
		if (!(st = F.host_parse(&ix.p->E))) st = lsq_ir_host_reads(ix.p, F.reads, (uint32_t)min_ov, 0, &t.p);
		F.free_reads();
	} else if (!(st = F.create_context())) st = lsq_ir_device(F.c, ix.p, pos[4], pos[5], (uint32_t)min_ov, &t.p);
	if (!st) st = lsq_ir_format(t.p, ratios ? 1 : 0, &F.text[0]);
	if (st) return cli_failed(st);
	const uint64_t *rep = t.p->report;
	char msg[768];
	snprintf(msg, sizeof msg, "retention: %llu read(s), %llu block(s), %llu occurrence(s) of junctions; %llu block pair(s) below the overhang, %llu with a block on no chromosome of the annotation; "
	         "%llu boundary(ies), %llu block(s) through one, %llu sites row(s) without a spliced read; %llu intron(s), %llu without a clean base, %llu piece(s); "
	         "%llu depth row(s), %llu base(s) in the counted blocks",
	         (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2], (unsigned long long)rep[3], (unsigned long long)rep[4],
	         (unsigned long long)rep[5], (unsigned long long)rep[6], (unsigned long long)rep[7], (unsigned long long)rep[8], (unsigned long long)rep[9], (unsigned long long)rep[10],
	         (unsigned long long)rep[11], (unsigned long long)rep[12]);
	cli_log(1, msg);
	return F.deliver(F.text[0], out);
}
