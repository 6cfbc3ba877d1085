// Host side of the local events (step 2 of the pipeline, bin/Events.r): the reader of the gene list (read.table + table,
// :40-42), the reader of classify's .matrix files (:47-55), the in-memory classify of annotation mode, the formatter of
// the eight .interval / .map pairs and the events executable.  The detection itself is lsq_localev.hip.  Every input is
// read and checked before the first HIP call; nothing is printed or written before the device has answered.
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "lsq_localev.hpp"

using namespace lsq;

namespace lsq { int compile_events(const lsq_annotation *a, int n_methods, const char *const *read_types,
                                   const uint64_t *lens, bool device_plan, lsq_events **out);
int annotation_load(const char *isoform_format, const char *isoforms_path, const std::string *isoforms_text,
                    const char *g2i_format, const char *g2i_path, const std::string *g2i_text,
                    uint64_t gene_begin_idx, uint64_t gene_end_idx, lsq_annotation **out); }      // lsq_annot.cpp

void lsq_le_graphs::add_gene(const std::string &name, const std::string &ch, const std::string &st, int n, int k) {
	if (pos_off.empty()) { pos_off.push_back(0); bit_off.push_back(0); }
	names.push_back(name); chrom.push_back(ch); strand.push_back(st);
	strand_code.push_back(st == "+" ? LE_PLUS : (st == "-" ? LE_MINUS : LE_OTHER));
	N.push_back(n); K.push_back(k);
	const bool used = n >= 3;
	pos.resize(pos.size() + (used ? 2 * (size_t)n : 0), 0);
	bits.resize(bits.size() + (used ? (size_t)n * (((size_t)k + 63) / 64) : 0), 0);
	pos_off.push_back(pos.size());
	bit_off.push_back(bits.size());
}

namespace {

const char *const TYPE_NAME[LE_TYPES] = {"ES", "RI", "A5SS", "A3SS", "MXE", "AFE", "ALE", "T3"};

int read_file(const std::string &path, std::string &text) {
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return fail(LSQ_E_IO, "%s: cannot open: %s", path.c_str(), strerror(errno));
	char buf[1 << 16];
	size_t n;
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
	const bool bad = ferror(f);
	fclose(f);
	return bad ? fail(LSQ_E_IO, "%s: read error", path.c_str()) : LSQ_OK;
}

// the lines of a text, a trailing '\r' dropped; an unterminated last line counts (R's readLines / read.table read it)
std::vector<std::pair<size_t, size_t>> split_lines(const std::string &t) {
	std::vector<std::pair<size_t, size_t>> v;
	size_t p = 0;
	while (p < t.size()) {
		size_t e = t.find('\n', p);
		if (e == std::string::npos) e = t.size();
		size_t s = e;
		if (s > p && t[s - 1] == '\r') --s;
		v.emplace_back(p, s - p);
		p = e + 1;
	}
	return v;
}

// read.table's fields: runs of blanks (space, tab) separate them
void split_blank(const char *s, size_t len, std::vector<std::pair<size_t, size_t>> &out) {
	out.clear();
	size_t i = 0;
	while (i < len) {
		while (i < len && (s[i] == ' ' || s[i] == '\t')) ++i;
		if (i == len) break;
		size_t j = i;
		while (j < len && s[j] != ' ' && s[j] != '\t') ++j;
		out.emplace_back(i, j - i);
		i = j;
	}
}

// ---- the gene list: read.table(group, as.is = T), table() on column 1, the names with more than one line ------------
//
// type.convert turns the column into integers when every id is one (sign and digits, within R's 32-bit integer), into
// doubles when every id is a decimal number, and leaves strings otherwise.  table() sorts the levels: numerically for
// numbers, printed as R prints them ("01" -> "1", "1.50" -> "1.5"); strings in byte order (LC_COLLATE=C).  Ids R would
// read as NA, as logical or as hexadecimal (and Inf / NaN) are refused, as are '#' and quotes, which read.table treats
// as comment and quote characters.
enum IdMode { ID_INT, ID_DOUBLE, ID_STRING };

bool is_int_id(const std::string &s, long long &v) {
	size_t i = (s[0] == '+' || s[0] == '-') ? 1 : 0;
	if (i == s.size() || s.size() - i > 12) return false;
	for (size_t j = i; j < s.size(); ++j) if (s[j] < '0' || s[j] > '9') return false;
	v = strtoll(s.c_str(), nullptr, 10);
	return v > INT_MIN && v <= INT_MAX;            // INT_MIN is R's NA_integer_
}

bool is_decimal_id(const std::string &s, double &v) {
	size_t i = (s[0] == '+' || s[0] == '-') ? 1 : 0, digits = 0;
	while (i < s.size() && s[i] >= '0' && s[i] <= '9') { ++i; ++digits; }
	if (i < s.size() && s[i] == '.') { ++i; while (i < s.size() && s[i] >= '0' && s[i] <= '9') { ++i; ++digits; } }
	if (!digits) return false;
	if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
		++i;
		if (i < s.size() && (s[i] == '+' || s[i] == '-')) ++i;
		size_t ed = 0;
		while (i < s.size() && s[i] >= '0' && s[i] <= '9') { ++i; ++ed; }
		if (!ed) return false;
	}
	if (i != s.size()) return false;
	v = strtod(s.c_str(), nullptr);
	return true;
}

bool refused_id(const std::string &s) {
	static const char *const bad[] = {"NA", "T", "F", "TRUE", "FALSE", "true", "false", "True", "False",
	                                  "Inf", "inf", "-Inf", "-inf", "+Inf", "NaN", "nan", "-nan"};
	for (const char *b : bad) if (s == b) return true;
	size_t i = (s[0] == '+' || s[0] == '-') ? 1 : 0;
	return s.size() > i + 1 && s[i] == '0' && (s[i + 1] == 'x' || s[i + 1] == 'X');
}

struct IdKey {
	IdMode mode;
	long long iv = 0;
	double dv = 0;
	std::string sv;
	bool operator<(const IdKey &o) const { return mode == ID_INT ? iv < o.iv : (mode == ID_DOUBLE ? dv < o.dv : sv < o.sv); }
};

std::string r_number(double v) {
	char b[64];
	if (lsq_as_format_number(v, b, sizeof b)) throw std::runtime_error("formatting a number");
	return b;
}

struct GeneList {
	IdMode mode = ID_STRING;
	std::map<IdKey, uint64_t> lines;      // lines per id, in table()'s order
	bool key_of(const std::string &raw, IdKey &k) const {
		k.mode = mode;
		if (mode == ID_INT) return is_int_id(raw, k.iv);
		if (mode == ID_DOUBLE) return is_decimal_id(raw, k.dv);
		k.sv = raw;
		return true;
	}
	static std::string name_of(const IdKey &k) {
		if (k.mode == ID_INT) return std::to_string(k.iv);
		if (k.mode == ID_DOUBLE) return r_number(k.dv);
		return k.sv;
	}
};

int gene_list_of(const char *path, const std::string &text, GeneList &G);
int read_gene_list(const char *path, GeneList &G) {
	std::string text;
	int rc = read_file(path, text);
	if (rc) return rc;
	return gene_list_of(path, text, G);
}
// (path names the text in messages)
int gene_list_of(const char *path, const std::string &text, GeneList &G) {
	std::vector<std::string> ids;
	std::vector<uint64_t> line_of;
	std::vector<std::pair<size_t, size_t>> f;
	size_t cols = 0;
	uint64_t no = 0;
	for (const auto &ln : split_lines(text)) {
		++no;
		const char *s = text.data() + ln.first;
		for (size_t q = 0; q < ln.second; ++q)
			if (s[q] == '#' || s[q] == '"' || s[q] == '\'')
				return fail(LSQ_E_PARSE, "%s:%llu: '%c' (read.table's comment and quote characters are not supported in the gene list)", path, (unsigned long long)no, s[q]);
		split_blank(s, ln.second, f);
		if (f.empty()) continue;                   // blank.lines.skip
		if (!cols) cols = f.size();
		else if (f.size() != cols) return fail(LSQ_E_PARSE, "%s:%llu: %zu fields, the first line has %zu", path, (unsigned long long)no, f.size(), cols);
		ids.emplace_back(s + f[0].first, f[0].second);
		line_of.push_back(no);
		if (refused_id(ids.back()))
			return fail(LSQ_E_PARSE, "%s:%llu: id '%s' would be read by R as NA, logical, hexadecimal or non-finite (not supported)", path, (unsigned long long)no, ids.back().c_str());
	}
	if (ids.empty()) return fail(LSQ_E_PARSE, "%s: no lines available in input", path);
	bool all_int = true, all_num = true;
	for (const std::string &s : ids) {
		long long iv; double dv;
		if (!is_int_id(s, iv)) all_int = false;
		if (!is_decimal_id(s, dv)) { all_num = false; break; }
	}
	G.mode = all_int ? ID_INT : (all_num ? ID_DOUBLE : ID_STRING);
	for (const std::string &s : ids) {
		IdKey k;
		G.key_of(s, k);
		++G.lines[k];
	}
	return LSQ_OK;
}

// ---- classify's .matrix files (Events.r:47-55) --------------------------------------------------------------------

// pos: the digit runs of the header's third field (gsub("[^0-9]", " "), split on blanks, the first piece dropped: the
// empty piece before a leading non-digit, or the first run itself when the field starts with a digit), as.integer
int header_positions(const std::string &path, const char *s, size_t len, std::vector<int32_t> &pos) {
	pos.clear();
	size_t i = 0;
	bool first = true;
	while (i < len) {
		if (s[i] < '0' || s[i] > '9') { ++i; first = false; continue; }
		size_t j = i;
		while (j < len && s[j] >= '0' && s[j] <= '9') ++j;
		if (!(first && i == 0)) {
			size_t a = i;
			while (a + 1 < j && s[a] == '0') ++a;          // leading zeros
			if (j - a > 10 || strtoll(std::string(s + a, j - a).c_str(), nullptr, 10) > INT_MAX)
				return fail(LSQ_E_PARSE, "%s:1: coordinate %.*s is beyond R's integer range (as.integer gives NA)", path.c_str(), (int)(j - i), s + i);
			pos.push_back((int32_t)strtol(std::string(s + a, j - a).c_str(), nullptr, 10));
		}
		first = false;
		i = j;
	}
	return LSQ_OK;
}

int read_matrix_file(const std::string &path, const std::string &name, lsq_le_graphs &out) {
	std::string text;
	int rc = read_file(path, text);
	if (rc) return rc;
	const auto lines = split_lines(text);
	if (lines.empty()) return fail(LSQ_E_PARSE, "%s: empty file", path.c_str());
	// header: strsplit(cor, "\t", fixed = T)
	const char *h = text.data() + lines[0].first;
	const size_t hl = lines[0].second;
	std::vector<std::string> hf;
	size_t p = 0;
	while (p <= hl && hf.size() < 3) {
		size_t q = p;
		while (q < hl && h[q] != '\t') ++q;
		hf.emplace_back(h + p, q - p);
		p = q + 1;
	}
	if (hf.size() < 3 || hf[2].empty()) return fail(LSQ_E_PARSE, "%s:1: the header needs chromosome, strand and segments separated by tabs", path.c_str());
	std::vector<int32_t> pos;
	if ((rc = header_positions(path, hf[2].data(), hf[2].size(), pos))) return rc;
	// read.table(file, skip = 1): 0 / 1 fields, every line as many
	std::vector<std::pair<size_t, size_t>> f;
	size_t ncol = 0;
	std::vector<std::vector<uint8_t>> rows;
	for (size_t li = 1; li < lines.size(); ++li) {
		split_blank(text.data() + lines[li].first, lines[li].second, f);
		if (f.empty()) continue;
		if (!ncol) ncol = f.size();
		else if (f.size() != ncol) return fail(LSQ_E_PARSE, "%s:%zu: %zu fields, the first row has %zu", path.c_str(), li + 1, f.size(), ncol);
		rows.emplace_back(ncol);
		for (size_t c = 0; c < ncol; ++c) {
			const char *v = text.data() + lines[li].first + f[c].first;
			if (f[c].second != 1 || (v[0] != '0' && v[0] != '1')) return fail(LSQ_E_PARSE, "%s:%zu: field %zu is not 0 or 1", path.c_str(), li + 1, c + 1);
			rows.back()[c] = (uint8_t)(v[0] - '0');
		}
	}
	if (rows.empty()) return fail(LSQ_E_PARSE, "%s: no isoform rows (read.table: no lines available in input)", path.c_str());
	if (ncol > (size_t)INT_MAX / 2 || rows.size() > (size_t)INT_MAX) return fail(LSQ_E_RANGE, "%s: matrix too large", path.c_str());
	const int N = (int)ncol, K = (int)rows.size();
	if (N >= 3 && pos.size() != 2 * ncol)
		return fail(LSQ_E_PARSE, "%s:1: %zu coordinates in the header for %zu columns (Events.r would index NA)", path.c_str(), pos.size(), ncol);
	out.add_gene(name, hf[0], hf[1], N, K);
	if (N < 3) return LSQ_OK;                       // Events.r:57: skipped after its line is printed
	std::copy(pos.begin(), pos.end(), out.pos.end() - 2 * ncol);
	const size_t W = ((size_t)K + 63) / 64;
	uint64_t *b = out.bits.data() + out.bit_off[out.size() - 1];
	for (size_t r = 0; r < rows.size(); ++r)
		for (size_t c = 0; c < ncol; ++c)
			if (rows[r][c]) b[c * W + r / 64] |= 1ull << (r % 64);
	return LSQ_OK;
}

int load_matrices(const char *prefix, const char *group, lsq_le_graphs &out) {
	GeneList G;
	int rc = read_gene_list(group, G);
	if (rc) return rc;
	std::vector<std::string> sel;
	for (const auto &kv : G.lines) if (kv.second > 1) sel.push_back(GeneList::name_of(kv.first));
	if (sel.empty()) return fail(LSQ_E_ARG, "%s: no gene has more than one line (Events.r's 1:0 loop would read %sNA.matrix)", group, prefix);
	for (const std::string &name : sel)
		if ((rc = read_matrix_file(std::string(prefix) + name + ".matrix", name, out))) return rc;
	return LSQ_OK;
}

// annotation mode: classify's genes and matrices (lsq_cli.cpp run_classify), in memory; named and ordered as Events.r
// names and orders the map's ids
// iso_text / g2i_text: the two files' content where it is held in memory (lsq_le_load_gtf; the paths then name it in messages)
int load_annotation(const char *iso_fmt, const char *iso_path, const char *g2i_fmt, const char *g2i_path, lsq_le_graphs &out,
                    const std::string *iso_text = nullptr, const std::string *g2i_text = nullptr) {
	if (strcmp(iso_fmt, "LH_GENE_TXT") != 0 || strcmp(g2i_fmt, "UCSC_GENE2ISOFORM") != 0)
		return fail(LSQ_E_FORMAT, "Unknown file format error: %s", strcmp(iso_fmt, "LH_GENE_TXT") ? iso_fmt : g2i_fmt);
	GeneList G;
	int rc = g2i_text ? gene_list_of(g2i_path, *g2i_text, G) : read_gene_list(g2i_path, G);
	if (rc) return rc;
	lsq_annotation *a = nullptr;
	if ((rc = annotation_load(iso_fmt, iso_path, iso_text, g2i_fmt, g2i_path, g2i_text, 0, UINT64_MAX, &a))) return rc;
	std::unique_ptr<lsq_annotation, void (*)(lsq_annotation *)> ann(a, lsq_annotation_free);
	lsq_events *e = nullptr;
	if ((rc = compile_events(a, 0, nullptr, nullptr, false, &e))) return rc;
	std::unique_ptr<lsq_events, void (*)(lsq_events *)> ev(e, lsq_events_free);
	std::map<IdKey, const Event *> order;
	for (const Event &x : e->ev) {
		if (x.K < 2) continue;                       // classify/classify.cpp:159
		IdKey k;
		if (!G.key_of(x.gname, k)) return fail(LSQ_E_PARSE, "%s: gene %s does not convert like the other ids", g2i_path, x.gname.c_str());
		if (!order.emplace(k, &x).second)
			return fail(LSQ_E_ARG, "%s: genes %s and %s are the same id to R", g2i_path, order[k]->gname.c_str(), x.gname.c_str());
	}
	if (order.empty()) return fail(LSQ_E_ARG, "%s: no gene has more than one isoform", g2i_path);
	for (const auto &kv : order) {
		const Event &x = *kv.second;
		out.add_gene(GeneList::name_of(kv.first), x.chrom, x.strand, x.N, x.K);
		if (x.N < 3) continue;
		int32_t *p = out.pos.data() + out.pos_off[out.size() - 1];
		for (int n = 0; n < x.N; ++n) {               // the header's digit runs: a minus sign is not part of them
			p[2 * n] = (int32_t)std::llabs(x.seg_s[n]);
			p[2 * n + 1] = (int32_t)std::llabs(x.seg_e[n]);
		}
		const size_t W = ((size_t)x.K + 63) / 64, nw = ((size_t)x.N + 63) / 64;
		uint64_t *b = out.bits.data() + out.bit_off[out.size() - 1];
		for (int r = 0; r < x.K; ++r)
			for (int n = 0; n < x.N; ++n)
				if (x.iso_wide[(size_t)r * nw + (size_t)n / 64] >> (n % 64) & 1) b[(size_t)n * W + (size_t)r / 64] |= 1ull << (r % 64);
	}
	return LSQ_OK;
}

// ---- output (Events.r's write(..., sep = "\t", ncolumns = 8), append = T) ------------------------------------------

void put_int(std::string &o, long long v) {
	char b[24];
	int n = snprintf(b, sizeof b, "%lld", v);
	o.append(b, (size_t)n);
}

// The two .interval lines and the two .map lines of record q of type t
void format_record(const lsq_le_graphs &g, int t, uint64_t rec, uint64_t q, std::string &iv, std::string &mp) {
	const uint32_t gi = (uint32_t)rec, code = (uint32_t)(rec >> 32);
	const int32_t *pos = g.pos.data() + g.pos_off[gi];
	auto P = [&](long long j) { return (long long)pos[j - 1]; };          // pos[j], 1-based as in the script
	const long long i = code, k = 2LL * g.N[gi];
	long long sp0, sp1, cnt[2];
	std::vector<long long> st[2], en[2];
	if (t <= LE_A3SS) {                                // :62-93
		sp0 = P(2 * i - 3); sp1 = P(2 * i + 2);
		cnt[0] = 3; st[0] = {P(2 * i - 3), P(2 * i - 1), P(2 * i + 1)}; en[0] = {P(2 * i - 2), P(2 * i), P(2 * i + 2)};
		cnt[1] = 2; st[1] = {P(2 * i - 3), P(2 * i + 1)}; en[1] = {P(2 * i - 2), P(2 * i + 2)};
	} else if (t == LE_MXE) {                          // :95-107
		sp0 = P(2 * i - 7); sp1 = P(2 * i);
		cnt[0] = 3; st[0] = {P(2 * i - 7), P(2 * i - 5), P(2 * i - 1)}; en[0] = {P(2 * i - 6), P(2 * i - 4), P(2 * i)};
		cnt[1] = 3; st[1] = {P(2 * i - 7), P(2 * i - 3), P(2 * i - 1)}; en[1] = {P(2 * i - 6), P(2 * i - 2), P(2 * i)};
	} else if (t == LE_AFE || t == LE_ALE) {
		cnt[0] = cnt[1] = 2;
		if (code == 0) {                               // :109-124
			st[0] = {P(3), P(5)}; en[0] = {P(4), P(6)};
			st[1] = {P(1), P(5)}; en[1] = {P(2), P(6)};
		} else {                                       // :126-141
			st[0] = {P(k - 5), P(k - 3)}; en[0] = {P(k - 4), P(k - 2)};
			st[1] = {P(k - 5), P(k - 1)}; en[1] = {P(k - 4), P(k)};
		}
		sp0 = sp1 = 0;
	} else {                                           // T3, :143-156
		cnt[0] = cnt[1] = 1;
		if (code == 0) { st[0] = {P(k - 3)}; en[0] = {P(k)}; st[1] = {P(k - 3)}; en[1] = {P(k - 2)}; }
		else { st[0] = {P(1)}; en[0] = {P(4)}; st[1] = {P(3)}; en[1] = {P(4)}; }
		sp0 = sp1 = 0;
	}
	const std::string counter = r_number((double)(q + 1));      // a double: as.character (1e+05)
	for (int w = 0; w < 2; ++w) {
		std::string id = g.names[gi];
		id += '|';
		if (t <= LE_MXE) id += std::to_string(i); else id += TYPE_NAME[t];
		id += w == 0 ? "|1" : "|2";
		iv += id; iv += '\t'; iv += g.chrom[gi]; iv += '\t'; iv += g.strand[gi]; iv += '\t';
		if (t <= LE_MXE) { put_int(iv, sp0); iv += '\t'; put_int(iv, sp1); }
		else { put_int(iv, st[w].front()); iv += '\t'; put_int(iv, en[w].back()); }
		iv += '\t'; put_int(iv, cnt[w]); iv += '\t';
		for (size_t a = 0; a < st[w].size(); ++a) { if (a) iv += ','; put_int(iv, st[w][a]); }
		iv += '\t';
		for (size_t a = 0; a < en[w].size(); ++a) { if (a) iv += ','; put_int(iv, en[w][a]); }
		iv += '\n';
		mp += counter; mp += '\t'; mp += id; mp += '\n';
	}
}

void format_type(const lsq_le_result &r, int t, std::string &iv, std::string &mp) {
	iv.clear(); mp.clear();
	for (uint64_t q = 0; q < r.rec[t].size(); ++q) format_record(*r.g, t, r.rec[t][q], q, iv, mp);
}

std::string dir_of(const std::string &prefix) {
	const size_t s = prefix.rfind('/');
	if (s == std::string::npos) return ".";
	return s == 0 ? "/" : prefix.substr(0, s);
}

// the files write() would append to can be opened: the directory takes new files, an existing file takes writes
int check_out_prefix(const char *prefix) {
	const std::string dir = dir_of(prefix);
	struct stat sb;
	if (stat(dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) return fail(LSQ_E_IO, "%s: output directory %s does not exist", prefix, dir.c_str());
	for (int t = 0; t < LE_TYPES; ++t)
		for (const char *ext : {".interval", ".map"}) {
			const std::string path = std::string(prefix) + TYPE_NAME[t] + ext;
			if (stat(path.c_str(), &sb) == 0) {
				if (S_ISDIR(sb.st_mode) || access(path.c_str(), W_OK) != 0) return fail(LSQ_E_IO, "%s: cannot open for appending", path.c_str());
			} else if (access(dir.c_str(), W_OK | X_OK) != 0) {
				return fail(LSQ_E_IO, "%s: cannot create (directory %s is not writable)", path.c_str(), dir.c_str());
			}
		}
	return LSQ_OK;
}

int append_file(const std::string &path, const std::string &text) {
	FILE *f = fopen(path.c_str(), "ab");
	if (!f) return fail(LSQ_E_IO, "%s: cannot open for appending: %s", path.c_str(), strerror(errno));
	const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
	if (fclose(f) != 0 || !ok) return fail(LSQ_E_IO, "%s: write error", path.c_str());
	return LSQ_OK;
}

int write_result(const lsq_le_result &r, const char *prefix) {
	std::string iv, mp;
	for (int t = 0; t < LE_TYPES; ++t) {
		if (r.rec[t].empty()) continue;                 // no write(), no file
		format_type(r, t, iv, mp);
		int rc;
		if ((rc = append_file(std::string(prefix) + TYPE_NAME[t] + ".interval", iv))) return rc;
		if ((rc = append_file(std::string(prefix) + TYPE_NAME[t] + ".map", mp))) return rc;
	}
	return LSQ_OK;
}

// print(paste("processing gene: ", id, sep = "")) (:45)
std::string processing_lines(const lsq_le_graphs &g) {
	std::string o;
	for (const std::string &n : g.names) {
		o += "[1] \"processing gene: ";
		for (char c : n) { if (c == '"' || c == '\\') o += '\\'; o += c; }
		o += "\"\n";
	}
	return o;
}

const char *USAGE =
	"Usage:\n"
	"events <matrix_prefix> <group_file> <out_prefix>\n"
	"events --annotation <isoform_format> <isoforms_path> <g2i_format> <g2i_path> <out_prefix>\n"
	"events --gtf <gtf_path> <out_prefix>";

} // namespace

namespace lsq {

// classify in memory on an annotation that is held as text: lsq_le_load_gtf (lsq_gtf.cpp)
int le_graphs_from_texts(const std::string &interval_text, const std::string &map_text, const char *label, lsq_le_graphs &out) {
	const std::string a = std::string(label) + " (as LH_GENE_TXT)", b = std::string(label) + " (as UCSC_GENE2ISOFORM)";
	return load_annotation("LH_GENE_TXT", a.c_str(), "UCSC_GENE2ISOFORM", b.c_str(), out, &interval_text, &map_text);
}

// events (argv[0] ignored).  Exit status: 0, 1 for a usage or input error (reported before any HIP call), 2 otherwise.
int run_events(int argc, const char *const *argv, std::string &out) {
	const bool annot = argc >= 2 && strcmp(argv[1], "--annotation") == 0, gtf = argc >= 2 && strcmp(argv[1], "--gtf") == 0;
	if (annot ? argc != 7 : argc != 4) { cli_log(0, USAGE); return 1; }
	lsq_ctx *c = nullptr;
	std::unique_ptr<lsq_ctx, void (*)(lsq_ctx *)> ctx(nullptr, lsq_ctx_destroy);
	lsq_le_graphs *raw = nullptr;
	int st;
	if (gtf) {
		// the GTF is parsed on the device (lsq_gtf.hip), so the context comes first; the output directory is still checked before anything is written
		if ((st = check_out_prefix(argv[3]))) { cli_log(0, lsq_last_error()); return 1; }
		st = lsq_ctx_create(cli_device(), &c);
		ctx.reset(c);
		if (st) { cli_log(0, lsq_last_error()); return 2; }
		st = lsq_le_load_gtf(c, argv[2], &raw);
		if (st == LSQ_E_PARSE && strncmp(lsq_last_error(), "PROBLEM:", 8) == 0) { fprintf(stderr, "%s\n", lsq_last_error()); fflush(stderr); return 1; }
		if (st == LSQ_E_DEVICE) { cli_log(0, lsq_last_error()); return 2; }
	} else {
		st = annot ? lsq_le_load_annotation(argv[2], argv[3], argv[4], argv[5], &raw) : lsq_le_load_matrices(argv[1], argv[2], &raw);
	}
	if (st) { cli_log(0, lsq_last_error()); return st == LSQ_E_INTERNAL ? 2 : 1; }
	std::unique_ptr<lsq_le_graphs, void (*)(lsq_le_graphs *)> g(raw, lsq_le_graphs_free);
	const char *prefix = annot ? argv[6] : argv[3];
	if ((st = check_out_prefix(prefix))) { cli_log(0, lsq_last_error()); return 1; }
	lsq_le_result *res = nullptr;
	if (!c) {
		st = lsq_ctx_create(cli_device(), &c);
		ctx.reset(c);
	}
	if (!st) st = lsq_le_detect(c, g.get(), &res);
	std::unique_ptr<lsq_le_result, void (*)(lsq_le_result *)> r(res, lsq_le_result_free);
	if (st) { cli_log(0, lsq_last_error()); return 2; }
	if ((st = write_result(*r, prefix))) { cli_log(0, lsq_last_error()); return 2; }
	out = processing_lines(*g);
	return 0;
}

} // namespace lsq

extern "C" {

int lsq_le_load_matrices(const char *matrix_prefix, const char *group_path, lsq_le_graphs **out) LSQ_API_TRY {
	if (!out || !matrix_prefix || !group_path) return fail(LSQ_E_ARG, "null argument");
	*out = nullptr;
	std::unique_ptr<lsq_le_graphs> g(new lsq_le_graphs);
	const int rc = load_matrices(matrix_prefix, group_path, *g);
	if (rc) return rc;
	*out = g.release();
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_le_load_annotation(const char *isoform_format, const char *isoforms_path, const char *g2i_format, const char *g2i_path,
                           lsq_le_graphs **out) LSQ_API_TRY {
	if (!out || !isoform_format || !isoforms_path || !g2i_format || !g2i_path) return fail(LSQ_E_ARG, "null argument");
	*out = nullptr;
	std::unique_ptr<lsq_le_graphs> g(new lsq_le_graphs);
	const int rc = load_annotation(isoform_format, isoforms_path, g2i_format, g2i_path, *g);
	if (rc) return rc;
	*out = g.release();
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_le_graphs_free(lsq_le_graphs *g) { delete g; }
int64_t lsq_le_num_genes(const lsq_le_graphs *g) { return g ? (int64_t)g->size() : 0; }
const char *lsq_le_gene_name(const lsq_le_graphs *g, int64_t i) { return g && i >= 0 && (size_t)i < g->size() ? g->names[(size_t)i].c_str() : nullptr; }
int lsq_le_gene_shape(const lsq_le_graphs *g, int64_t i, int *n_columns, int *n_isoforms) {
	if (!g || i < 0 || (size_t)i >= g->size() || !n_columns || !n_isoforms) return LSQ_E_ARG;
	*n_columns = g->N[(size_t)i]; *n_isoforms = g->K[(size_t)i];
	return LSQ_OK;
}

int64_t lsq_le_gene_positions(const lsq_le_graphs *g, int64_t i, const int32_t **pos) {
	if (!g || i < 0 || (size_t)i >= g->size() || !pos) return -1;
	*pos = g->pos.data() + g->pos_off[(size_t)i];
	return (int64_t)(g->pos_off[(size_t)i + 1] - g->pos_off[(size_t)i]);
}

void lsq_le_result_free(lsq_le_result *r) { delete r; }
int64_t lsq_le_num_events(const lsq_le_result *r, int type) { return r && type >= 0 && type < LE_TYPES ? (int64_t)r->rec[type].size() : -1; }
int lsq_le_event(const lsq_le_result *r, int type, int64_t q, int64_t *gene, int32_t *code) {
	if (!r || type < 0 || type >= LE_TYPES || q < 0 || (size_t)q >= r->rec[type].size() || !gene || !code) return LSQ_E_ARG;
	*gene = (int64_t)(uint32_t)r->rec[type][(size_t)q];
	*code = (int32_t)(r->rec[type][(size_t)q] >> 32);
	return LSQ_OK;
}
int lsq_le_result_times(const lsq_le_result *r, double *ms) {
	if (!r || !ms) return LSQ_E_ARG;
	for (int q = 0; q < 4; ++q) ms[q] = r->ms[q];
	return LSQ_OK;
}
const char *lsq_le_type_name(int type) { return type >= 0 && type < LE_TYPES ? TYPE_NAME[type] : nullptr; }

int lsq_le_format(const lsq_le_result *r, int type, char **interval_text, char **map_text) LSQ_API_TRY {
	if (!r || type < 0 || type >= LE_TYPES || !interval_text || !map_text) return fail(LSQ_E_ARG, "bad argument");
	std::string iv, mp;
	format_type(*r, type, iv, mp);
	*interval_text = (char *)malloc(iv.size() + 1);
	*map_text = (char *)malloc(mp.size() + 1);
	if (!*interval_text || !*map_text) { free(*interval_text); free(*map_text); *interval_text = *map_text = nullptr; return fail(LSQ_E_INTERNAL, "out of memory"); }
	memcpy(*interval_text, iv.c_str(), iv.size() + 1);
	memcpy(*map_text, mp.c_str(), mp.size() + 1);
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_le_write(const lsq_le_result *r, const char *out_prefix) LSQ_API_TRY {
	if (!r || !out_prefix) return fail(LSQ_E_ARG, "null argument");
	int rc = check_out_prefix(out_prefix);
	return rc ? rc : write_result(*r, out_prefix);
} LSQ_API_CATCH

} // extern "C"
