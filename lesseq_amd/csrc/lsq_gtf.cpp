// Host side of the annotation from GTF (bin/parseGencode, bin/gencodeIsoformMap): the transcripts put
// together from the records the device returns (lsq_gtf.hip), the two formatters, gencodeIsoformMap's counter (host-only)
// and the two executables.  Nothing here walks the GTF's bytes: names are sliced out of the text by the device's offsets.
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "lsq_gtf.hpp"
#include "lsq_localev.hpp"

using namespace lsq;

namespace lsq {

int le_graphs_from_texts(const std::string &interval_text, const std::string &map_text, const char *label, lsq_le_graphs &out);   // lsq_localev.cpp

int read_all(const char *path, std::string &bytes) {
	FILE *f = path ? fopen(path, "rb") : stdin;
	if (!f) return fail(LSQ_E_IO, "cannot open %s: %s", path, strerror(errno));
	char buf[1 << 16];
	size_t n;
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) bytes.append(buf, n);
	const bool bad = ferror(f);
	if (path) fclose(f);
	return bad ? fail(LSQ_E_IO, "read error on %s", path ? path : "standard input") : LSQ_OK;
}

namespace {

struct Slice {
	const unsigned char *p; size_t n;
	int cmp(const Slice &o) const {               // std::string's order: bytes as unsigned, a prefix first
		const int c = memcmp(p, o.p, std::min(n, o.n));
		return c ? c : (n < o.n ? -1 : (n > o.n ? 1 : 0));
	}
};

void put_int(std::string &o, long long v) {
	char b[24];
	const int n = snprintf(b, sizeof b, "%lld", v);
	o.append(b, (size_t)n);
}

} // namespace

// Runs of one name in file order -> transcripts ordered by gene id, then transcript id.  A stable sort keeps the runs of
// one name in file order, so that the first of them gives the chromosome and strand (the transcript's first kept line).
int gtf_assemble(const unsigned char *text, const GtfRec *heads, size_t n_heads, const int32_t *se, size_t n_kept,
                 std::vector<GtfTranscript> &out, uint64_t &n_genes) {
	out.clear(); n_genes = 0;
	// the names once out of the text (one visit per run head, in file order) into one block: the sort then compares there
	std::string arena;
	std::vector<size_t> at(n_heads + 1, 0);
	for (size_t h = 0; h < n_heads; ++h) at[h + 1] = at[h] + heads[h].gene_len + heads[h].tx_len;
	arena.resize(at[n_heads]);
	for (size_t h = 0; h < n_heads; ++h) {
		memcpy(&arena[at[h]], text + heads[h].line_off + heads[h].gene_off, heads[h].gene_len);
		memcpy(&arena[at[h] + heads[h].gene_len], text + heads[h].line_off + heads[h].tx_off, heads[h].tx_len);
	}
	const unsigned char *names = (const unsigned char *)arena.data();
	std::vector<uint32_t> order(n_heads);
	std::iota(order.begin(), order.end(), 0u);
	auto gene = [&](uint32_t h) { return Slice{names + at[h], heads[h].gene_len}; };
	auto tx = [&](uint32_t h) { return Slice{names + at[h] + heads[h].gene_len, heads[h].tx_len}; };
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
		const int g = gene(a).cmp(gene(b));
		return g ? g < 0 : tx(a).cmp(tx(b)) < 0;
	});
	for (size_t i = 0; i < n_heads;) {
		const uint32_t h0 = order[i];
		size_t j = i + 1;
		while (j < n_heads && gene(order[j]).cmp(gene(h0)) == 0 && tx(order[j]).cmp(tx(h0)) == 0) ++j;
		if (out.empty() || i == 0 || gene(order[i - 1]).cmp(gene(h0)) != 0) ++n_genes;
		out.emplace_back();
		GtfTranscript &t = out.back();
		const Slice g = gene(h0), x = tx(h0);
		t.name.assign((const char *)g.p, g.n); t.name += '|'; t.name.append((const char *)x.p, x.n);
		t.gene_len = g.n;
		t.chrom.assign((const char *)text + heads[h0].line_off, heads[h0].chrom_len);
		t.strand.assign((const char *)text + heads[h0].line_off + heads[h0].strand_off, heads[h0].strand_len);
		for (size_t q = i; q < j; ++q) {
			const uint32_t h = order[q];
			const size_t k0 = heads[h].aux, k1 = (size_t)h + 1 < n_heads ? heads[h + 1].aux : n_kept;      // the run: up to the next head in file order
			if (k1 < k0 || k1 > n_kept) return fail(LSQ_E_INTERNAL, "run heads out of order");
			for (size_t k = k0; k < k1; ++k) { t.starts.push_back(se[2 * k]); t.ends.push_back(se[2 * k + 1]); }
		}
		std::sort(t.starts.begin(), t.starts.end());
		std::sort(t.ends.begin(), t.ends.end());
		i = j;
	}
	return LSQ_OK;
}

namespace {

void format_interval(const lsq_gtf &g, std::string &o) {
	for (const GtfTranscript &t : g.tx) {
		o += t.name; o += '\t'; o += t.chrom; o += '\t'; o += t.strand; o += '\t';
		put_int(o, t.starts.front()); o += '\t'; put_int(o, t.ends.back()); o += '\t'; put_int(o, (long long)t.starts.size()); o += '\t';
		for (size_t a = 0; a < t.starts.size(); ++a) { if (a) o += ','; put_int(o, t.starts[a]); }
		o += '\t';
		for (size_t a = 0; a < t.ends.size(); ++a) { if (a) o += ','; put_int(o, t.ends[a]); }
		o += '\n';
	}
}

// gencodeIsoformMap: a counter and a TAB ahead of every line; the counter starts at 1 and goes up where the text before
// the line's first '|' differs from the line before.  "\r\n" ends a line as "\n" does; empty lines are dropped; the last
// line needs no newline.  A line without '|' is an input error, except as the only line (the reference prints that one).
int isoform_map(const char *s, size_t len, std::string &o) {
	struct Line { size_t p, n, bar; uint64_t no; };
	std::vector<Line> lines;
	uint64_t no = 0;
	for (size_t p = 0; p < len;) {
		const char *nl = (const char *)memchr(s + p, '\n', len - p);
		const size_t e = nl ? (size_t)(nl - s) : len;
		size_t n = e - p;
		if (nl && n && s[e - 1] == '\r') --n;
		++no;
		if (n) {
			const char *bar = (const char *)memchr(s + p, '|', n);
			lines.push_back(Line{p, n, bar ? (size_t)(bar - (s + p)) : n, no});
		}
		p = e + 1;
	}
	if (lines.size() > 1)
		for (const Line &l : lines)
			if (l.bar == l.n) return fail(LSQ_E_PARSE, "PROBLEM: line %llu has no '|' between gene and transcript id", (unsigned long long)l.no);
	uint64_t counter = 1;
	for (size_t i = 0; i < lines.size(); ++i) {
		const Line &l = lines[i];
		if (i && (l.bar != lines[i - 1].bar || memcmp(s + l.p, s + lines[i - 1].p, l.bar) != 0)) ++counter;
		put_int(o, (long long)counter); o += '\t'; o.append(s + l.p, l.n); o += '\n';
	}
	return LSQ_OK;
}

} // namespace

// parseGencode [gtf_path]: the GTF from standard input (or the file) to the LH_GENE_TXT text.  Exit status 0; 1 for an
// input error (the reference's own "PROBLEM: ..." line on standard error), 2 otherwise; nothing on standard output then.
int run_parse_gencode(int argc, const char *const *argv, std::string &out) {
	if (argc > 2) { cli_log(0, "Usage:\nparseGencode [gtf_path]      (standard input without a path)"); return 1; }
	std::string bytes;
	if (argc < 2 && read_all(nullptr, bytes)) { cli_log(0, lsq_last_error()); return 1; }
	lsq_ctx *c = nullptr;
	int st = lsq_ctx_create(cli_device(), &c);
	std::unique_ptr<lsq_ctx, void (*)(lsq_ctx *)> ctx(c, lsq_ctx_destroy);
	if (st) { cli_log(0, lsq_last_error()); return 2; }
	lsq_gtf *raw = nullptr;
	st = argc == 2 ? lsq_gtf_parse(c, argv[1], &raw) : lsq_gtf_parse_text(c, bytes.data(), bytes.size(), &raw);
	std::unique_ptr<lsq_gtf, void (*)(lsq_gtf *)> g(raw, lsq_gtf_free);
	if (st == LSQ_E_PARSE) { fprintf(stderr, "%s\n", lsq_last_error()); fflush(stderr); return 1; }
	if (st) { cli_log(0, lsq_last_error()); return st == LSQ_E_IO ? 1 : 2; }
	format_interval(*g, out);
	return 0;
}

// gencodeIsoformMap [names_path]: no GPU touched
int run_isoform_map(int argc, const char *const *argv, std::string &out) {
	if (argc > 2) { cli_log(0, "Usage:\ngencodeIsoformMap [names_path]      (standard input without a path)"); return 1; }
	std::string bytes;
	if (read_all(argc == 2 ? argv[1] : nullptr, bytes)) { cli_log(0, lsq_last_error()); return 1; }
	const int st = isoform_map(bytes.data(), bytes.size(), out);
	if (st) { out.clear(); fprintf(stderr, "%s\n", lsq_last_error()); fflush(stderr); return 1; }
	return 0;
}

} // namespace lsq

extern "C" {

void lsq_gtf_free(lsq_gtf *g) { delete g; }
int64_t lsq_gtf_num_transcripts(const lsq_gtf *g) { return g ? (int64_t)g->tx.size() : 0; }
int64_t lsq_gtf_num_genes(const lsq_gtf *g) { return g ? (int64_t)g->n_genes : 0; }
int64_t lsq_gtf_num_exon_lines(const lsq_gtf *g) { return g ? (int64_t)g->n_kept : 0; }
#define TX_OR(bad) if (!g || i < 0 || (size_t)i >= g->tx.size()) return bad
const char *lsq_gtf_transcript_name(const lsq_gtf *g, int64_t i) { TX_OR(nullptr); return g->tx[(size_t)i].name.c_str(); }
const char *lsq_gtf_transcript_chrom(const lsq_gtf *g, int64_t i) { TX_OR(nullptr); return g->tx[(size_t)i].chrom.c_str(); }
const char *lsq_gtf_transcript_strand(const lsq_gtf *g, int64_t i) { TX_OR(nullptr); return g->tx[(size_t)i].strand.c_str(); }
int64_t lsq_gtf_transcript_exons(const lsq_gtf *g, int64_t i, const int32_t **starts, const int32_t **ends) {
	TX_OR(-1);
	if (starts) *starts = g->tx[(size_t)i].starts.data();
	if (ends) *ends = g->tx[(size_t)i].ends.data();
	return (int64_t)g->tx[(size_t)i].starts.size();
}
int lsq_gtf_result_times(const lsq_gtf *g, double *ms) {
	if (!g || !ms) return LSQ_E_ARG;
	for (int q = 0; q < 4; ++q) ms[q] = g->ms[q];
	return LSQ_OK;
}

int lsq_gtf_format(const lsq_gtf *g, char **interval_text, char **map_text) LSQ_API_TRY {
	if (!g || (!interval_text && !map_text)) return fail(LSQ_E_ARG, "null argument");
	std::string iv, names, mp;
	format_interval(*g, iv);
	if (map_text) {
		for (const GtfTranscript &t : g->tx) { names += t.name; names += '\n'; }      // `cut -f1` of the interval text
		const int rc = isoform_map(names.data(), names.size(), mp);
		if (rc) return rc;
	}
	char *a = interval_text ? dup_text(iv) : nullptr, *b = map_text ? dup_text(mp) : nullptr;
	if ((interval_text && !a) || (map_text && !b)) { free(a); free(b); return fail(LSQ_E_INTERNAL, "out of memory"); }
	if (interval_text) *interval_text = a;
	if (map_text) *map_text = b;
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_gtf_isoform_map(const char *names_text, uint64_t len, char **map_text) LSQ_API_TRY {
	if ((!names_text && len) || !map_text) return fail(LSQ_E_ARG, "null argument");
	*map_text = nullptr;
	std::string mp;
	const int rc = isoform_map(names_text, (size_t)len, mp);
	if (rc) return rc;
	*map_text = dup_text(mp);
	return *map_text ? LSQ_OK : fail(LSQ_E_INTERNAL, "out of memory");
} LSQ_API_CATCH

int lsq_le_load_gtf(lsq_ctx *c, const char *path, lsq_le_graphs **out) LSQ_API_TRY {
	if (!c || !path || !out) return fail(LSQ_E_ARG, "null argument");
	*out = nullptr;
	lsq_gtf *raw = nullptr;
	int rc = lsq_gtf_parse(c, path, &raw);
	std::unique_ptr<lsq_gtf, void (*)(lsq_gtf *)> g(raw, lsq_gtf_free);
	if (rc) return rc;
	std::string iv, names, mp;
	format_interval(*g, iv);
	for (const GtfTranscript &t : g->tx) { names += t.name; names += '\n'; }
	if ((rc = isoform_map(names.data(), names.size(), mp))) return rc;
	std::unique_ptr<lsq_le_graphs> graphs(new lsq_le_graphs);
	if ((rc = le_graphs_from_texts(iv, mp, path, *graphs))) return rc;
	*out = graphs.release();
	return LSQ_OK;
} LSQ_API_CATCH

} // extern "C"
