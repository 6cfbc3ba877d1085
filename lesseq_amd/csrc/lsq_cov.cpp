// Per-base read depth of a read file (include/lesseq_hip.h, lsq_cov_*): the index made from an annotation, the host
// path over the host parsers' arrays, the tables' text and the coverage executable.  The device passes are lsq_cov.hip, the
// entry that opens a read file on the device is lsq_readfile.hip's lsq_cov_device; what the tool shares with junctions and
// exonbins is lsq_readtool.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "lsq_cov.hpp"

using namespace lsq;

namespace {

// a position at which the depth changes by `delta`: key = chromosome index << 32 | position + 2^30
struct Step { uint64_t key; int64_t delta; };
inline bool step_less(const Step &a, const Step &b) { return a.key < b.key; }

// sorted steps with equal keys -> one each
void fold_steps(std::vector<Step> &v) {
	size_t o = 0;
	for (size_t i = 0; i < v.size(); ++i) {
		if (o && v[o - 1].key == v[i].key) v[o - 1].delta += v[i].delta;
		else v[o++] = v[i];
	}
	v.resize(o);
}

// covered and depth_sum of every region from rows in (chromosome index, start) order: the rows an interval overlaps, one by one
void host_regions(const lsq_cov_index &ix, lsq_cov_table &t) {
	const size_t nr = t.chrom.size();
	for (size_t r = 0; r < ix.name.size(); ++r)
		for (uint64_t q = ix.iv_off[r]; q < ix.iv_off[r + 1]; ++q) {
			const uint32_t c = ix.chrom[r];
			const int64_t s = ix.iv_s[q], e = ix.iv_e[q];
			size_t lo = 0, hi = nr;
			while (lo < hi) {
				const size_t mid = lo + (hi - lo) / 2;
				if (t.chrom[mid] < c || (t.chrom[mid] == c && (int64_t)t.end[mid] <= s)) lo = mid + 1; else hi = mid;
			}
			for (size_t k = lo; k < nr && t.chrom[k] == c && (int64_t)t.start[k] < e; ++k) {
				const uint64_t ov = (uint64_t)(std::min<int64_t>(e, t.end[k]) - std::max<int64_t>(s, t.start[k]));
				if (t.depth[k] >= t.min_depth) t.r_covered[r] += ov;
				t.r_depth_sum[r] += ov * t.depth[k];
			}
		}
}

} // namespace

void lsq::cov_finish_table(const lsq_cov_index &ix, lsq_cov_table &t) {
	t.chrom_names = ix.E.chroms.names;
	const std::vector<size_t> from = rows_by_chrom_name(t.chrom_names, t.chrom);
	auto permute = [&](auto &v) { auto w = v; for (size_t i = 0; i < from.size(); ++i) w[i] = v[from[i]]; v.swap(w); };
	permute(t.chrom); permute(t.start); permute(t.end); permute(t.depth);
	t.r_name = ix.name; t.r_strand = ix.strand; t.r_chrom = ix.chrom; t.r_bases = ix.bases;
}

int lsq::cov_host_reads(const lsq_cov_index &ix, const ParsedReads &R, int strand, uint32_t min_depth, int n_threads, lsq_cov_table &t) {
	const int T = read_slices(R.n_reads, n_threads);
	const unsigned strand_id = strand == '+' ? 0u : strand == '-' ? 1u : 0xFFFFFFFFu;
	std::vector<std::vector<Step>> part((size_t)T);
	std::vector<uint64_t> tally((size_t)T * 5, 0);       // counted, without chromosome, empty or descending, other strand, bases
	const int rc = for_read_slices(R.n_reads, T, [&](int k, uint64_t r0, uint64_t r1) {
		std::vector<Step> &v = part[(size_t)k];
		uint64_t *n = &tally[(size_t)k * 5];
		for (uint64_t b = R.blk_off[r0]; b < R.blk_off[r1]; ++b) {
			const unsigned c = R.bc[b];
			if (c == NO_CHROM) { ++n[1]; continue; }
			if (R.be[b] <= R.bs[b]) { ++n[2]; continue; }
			if (strand_id != 0xFFFFFFFFu && R.bst[b] != strand_id) { ++n[3]; continue; }
			++n[0]; n[4] += (uint64_t)((int64_t)R.be[b] - R.bs[b]);
			v.push_back(Step{((uint64_t)c << 32) | (uint64_t)((int64_t)R.bs[b] + COV_BIAS), 1});
			v.push_back(Step{((uint64_t)c << 32) | (uint64_t)((int64_t)R.be[b] + COV_BIAS), -1});
		}
		std::sort(v.begin(), v.end(), step_less);
		fold_steps(v);
	});
	if (rc) return rc;
	for (uint64_t &v : t.report) v = 0;
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks;
	for (int k = 0; k < T; ++k) for (int q = 0; q < 5; ++q) t.report[2 + q] += tally[(size_t)k * 5 + q];
	if (t.report[2] > 0x7FFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32-1 sort records (two per counted block)");
	const std::vector<Step> all = merge_folded(part, step_less, fold_steps);
	// the sweep: the depth behind every step; a stretch of positive depth joins the row before it when it abuts it at the same depth
	t.resize(0);
	int64_t depth = 0;
	for (size_t i = 0; i + 1 < all.size(); ++i) {
		depth += all[i].delta;
		if (depth <= 0) continue;                         // (0 behind a chromosome's last step: every block ends where it began)
		const uint32_t c = (uint32_t)(all[i].key >> 32);
		const int32_t s = (int32_t)((int64_t)(all[i].key & 0xFFFFFFFFull) - COV_BIAS), e = (int32_t)((int64_t)(all[i + 1].key & 0xFFFFFFFFull) - COV_BIAS);
		if (!t.chrom.empty() && t.chrom.back() == c && t.end.back() == s && t.depth.back() == (uint32_t)depth) t.end.back() = e;
		else { t.chrom.push_back(c); t.start.push_back(s); t.end.push_back(e); t.depth.push_back((uint32_t)depth); }
	}
	t.min_depth = min_depth;
	t.r_covered.assign(ix.name.size(), 0); t.r_depth_sum.assign(ix.name.size(), 0);
	host_regions(ix, t);
	for (float &m : t.ms) m = 0;
	cov_finish_table(ix, t);
	return LSQ_OK;
}

extern "C" {

int lsq_cov_index_build(const lsq_annotation *a, lsq_cov_index **out) LSQ_API_TRY {
	if (!a || !out) return fail(LSQ_E_ARG, "null argument");
	std::unique_ptr<lsq_cov_index> ix(new lsq_cov_index);
	int rc;
	if ((rc = annotation_dictionaries(*a, ix->E))) return rc;
	std::vector<std::pair<int64_t, int64_t>> ex;
	ix->iv_off.push_back(0);
	for (const auto &rp : a->recs) {
		const IsoRec &r = *rp;
		// the union of the line's exons as maximal intervals
		ex.clear();
		exon_union(r, ex);
		uint64_t bases = 0;
		const size_t first = ix->iv_s.size();
		for (const auto &x : ex) {
			if (ix->iv_s.size() > first && x.first <= ix->iv_e.back()) ix->iv_e.back() = std::max(ix->iv_e.back(), x.second);
			else { ix->iv_s.push_back(x.first); ix->iv_e.push_back(x.second); }
		}
		for (size_t q = first; q < ix->iv_s.size(); ++q) bases += (uint64_t)(ix->iv_e[q] - ix->iv_s[q]);
		ix->name.push_back(r.name); ix->strand.push_back(r.strand); ix->chrom.push_back((uint32_t)ix->E.chroms.find(r.chrom));
		ix->bases.push_back(bases); ix->iv_off.push_back(ix->iv_s.size());
	}
	*out = ix.release();
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_cov_index_free(lsq_cov_index *ix) { delete ix; }
int64_t lsq_cov_index_num_chroms(const lsq_cov_index *ix) { return index_num_chroms(ix); }
const char *lsq_cov_index_chrom_name(const lsq_cov_index *ix, int64_t chrom) { return index_chrom_name(ix, chrom); }
int64_t lsq_cov_index_num_regions(const lsq_cov_index *ix) { return ix ? (int64_t)ix->name.size() : 0; }
lsq_events *lsq_cov_index_dictionaries(lsq_cov_index *ix) { return index_dictionaries(ix); }

int lsq_cov_host_reads(lsq_cov_index *ix, const lsq_reads *r, int strand, uint32_t min_depth, int n_threads, lsq_cov_table **out) LSQ_API_TRY {
	if (!ix || !r || !out) return fail(LSQ_E_ARG, "null argument");
	if (!cov_strand_ok(strand)) return fail(LSQ_E_ARG, "strand must be 0, '+' or '-'");
	return new_table(out, [&](lsq_cov_table &t) { return cov_host_reads(*ix, host_view(*r), strand, min_depth, n_threads, t); });
} LSQ_API_CATCH

int lsq_cov_host(lsq_cov_index *ix, const char *read_format, const char *path, unsigned skip_flags, unsigned min_mapq, int strand, uint32_t min_depth, int n_threads,
                 lsq_cov_table **out) LSQ_API_TRY {
	if (!ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	if (!cov_strand_ok(strand)) return fail(LSQ_E_ARG, "strand must be 0, '+' or '-'");
	return host_file(ix->E, read_format, path, skip_flags, min_mapq, n_threads, [&](const lsq_reads *r) { return lsq_cov_host_reads(ix, r, strand, min_depth, n_threads, out); });
} LSQ_API_CATCH

void lsq_cov_table_free(lsq_cov_table *t) { delete t; }
int64_t lsq_cov_table_rows(const lsq_cov_table *t) { return t ? (int64_t)t->chrom.size() : 0; }
int64_t lsq_cov_table_regions(const lsq_cov_table *t) { return t ? (int64_t)t->r_bases.size() : 0; }
int lsq_cov_table_arrays(const lsq_cov_table *t, const uint32_t **chrom, const int32_t **start, const int32_t **end, const uint32_t **depth) {
	if (!t) return fail(LSQ_E_ARG, "null argument");
	if (chrom) *chrom = t->chrom.data();
	if (start) *start = t->start.data();
	if (end) *end = t->end.data();
	if (depth) *depth = t->depth.data();
	return LSQ_OK;
}
int lsq_cov_table_region_arrays(const lsq_cov_table *t, const uint32_t **chrom, const uint64_t **bases, const uint64_t **covered, const uint64_t **depth_sum) {
	if (!t) return fail(LSQ_E_ARG, "null argument");
	if (chrom) *chrom = t->r_chrom.data();
	if (bases) *bases = t->r_bases.data();
	if (covered) *covered = t->r_covered.data();
	if (depth_sum) *depth_sum = t->r_depth_sum.data();
	return LSQ_OK;
}
const char *lsq_cov_table_region_name(const lsq_cov_table *t, int64_t region) {
	return t && region >= 0 && (size_t)region < t->r_name.size() ? t->r_name[(size_t)region].c_str() : nullptr;
}
const char *lsq_cov_table_region_strand(const lsq_cov_table *t, int64_t region) {
	return t && region >= 0 && (size_t)region < t->r_strand.size() ? t->r_strand[(size_t)region].c_str() : nullptr;
}
int lsq_cov_table_report(const lsq_cov_table *t, uint64_t report[7]) { return table_report(t, report); }
int lsq_cov_table_times(const lsq_cov_table *t, float ms[6]) { return table_times(t, ms); }

int lsq_cov_format(const lsq_cov_table *t, uint32_t min_depth, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	char buf[64];
	for (size_t i = 0; i < t->chrom.size(); ++i) {
		if (t->depth[i] < min_depth) continue;
		o += t->chrom_names[t->chrom[i]];
		snprintf(buf, sizeof buf, "\t%d\t%d\t%u\n", t->start[i], t->end[i], t->depth[i]);
		o += buf;
	}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

int lsq_cov_format_regions(const lsq_cov_table *t, char **out_text) LSQ_API_TRY {
	if (!t || !out_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	char buf[128];
	for (size_t r = 0; r < t->r_bases.size(); ++r) {
		o += t->r_name[r]; o += '\t'; o += t->chrom_names[t->r_chrom[r]]; o += '\t'; o += t->r_strand[r];
		const double mean = t->r_bases[r] ? (double)t->r_depth_sum[r] / (double)t->r_bases[r] : 0.0;
		snprintf(buf, sizeof buf, "\t%llu\t%llu\t%llu\t%.4f\n", (unsigned long long)t->r_bases[r], (unsigned long long)t->r_covered[r], (unsigned long long)t->r_depth_sum[r], mean);
		o += buf;
	}
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

} // extern "C"

// coverage [--host] [--strand +|-] [--min-depth N] [--regions <regions_path>] <isoform_format> <isoforms_path> <g2i_format> <g2i_path>
//          <read_format> <reads_path> [<out>]
// The bedGraph on standard output (or in <out>; "-": standard output), the per-line summary in <regions_path>, the report in the
// log.  --min-depth: the rows printed and the bases a line counts as covered.  Exit status 1, nothing on standard output, for a
// file that does not open or parse.
int lsq::run_coverage(int argc, const char *const *argv, std::string &out) {
	static const char *USAGE = "Usage:\ncoverage [--host] [--strand +|-] [--min-depth N] [--regions regions_path] isoform_format isoforms_path g2i_format g2i_path read_format reads_path [out_path]";
	bool host = false, bad = false;
	unsigned long min_depth = 1;
	int strand = 0;
	const char *regions_path = nullptr;
	std::vector<const char *> pos;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (strcmp(argv[i], "--strand") == 0) {
			if (i + 1 < argc && (strcmp(argv[i + 1], "+") == 0 || strcmp(argv[i + 1], "-") == 0)) strand = argv[++i][0]; else bad = true;
		} else if (strcmp(argv[i], "--min-depth") == 0) bad = !cli_u32_option(argc, argv, i, min_depth);
		else if (strcmp(argv[i], "--regions") == 0) {
			if (i + 1 < argc) regions_path = argv[++i]; else bad = true;
		} else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else pos.push_back(argv[i]);
	}
	if (bad || pos.size() < 6 || pos.size() > 7) { cli_log(0, USAGE); return 1; }
	CliFrame F(pos);                                       // text[0] the bedGraph, text[1] the regions
	CliOwned<lsq_cov_index, lsq_cov_index_free> ix;
	CliOwned<lsq_cov_table, lsq_cov_table_free> t;
	int st = F.load_annotation();
	if (!st) st = lsq_cov_index_build(F.a, &ix.p);
	if (st) return cli_failed(st);
	if (host) {
		if (!(st = F.host_parse(&ix.p->E))) st = lsq_cov_host_reads(ix.p, F.reads, strand, (uint32_t)min_depth, 0, &t.p);
		F.free_reads();
	} else if (!(st = F.create_context())) st = lsq_cov_device(F.c, ix.p, pos[4], pos[5], strand, (uint32_t)min_depth, &t.p);
	if (!st) st = lsq_cov_format(t.p, (uint32_t)min_depth, &F.text[0]);
	if (!st && regions_path) st = lsq_cov_format_regions(t.p, &F.text[1]);
	if (st) return cli_failed(st);
	const uint64_t *rep = t.p->report;
	char msg[384];
	snprintf(msg, sizeof msg, "coverage: %llu read(s), %llu block(s), %llu counted in %lld row(s); %llu on no chromosome of the annotation, %llu empty or descending, %llu of the other strand; "
	         "%llu base(s) in the counted blocks (solve's total_read_bases)",
	         (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2], (long long)lsq_cov_table_rows(t.p), (unsigned long long)rep[3], (unsigned long long)rep[4],
	         (unsigned long long)rep[5], (unsigned long long)rep[6]);
	cli_log(1, msg);
	if (regions_path && !write_file(regions_path, F.text[1])) return cli_failed(LSQ_E_IO);
	return F.deliver(F.text[0], out);
}
