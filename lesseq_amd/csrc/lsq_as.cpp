// Host side of the differential splicing tests (step 4 of the pipeline, bin/Test_AS.r, and the beta-binomial test beside
// them): the readers of the script's matrices and of this project's count / solve tables, R's as.character formatting, and
// the test_as executable.  The kernels and the five compute entry points are lsq_as.hip.  Every input is read and checked before the first HIP call.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "lsq_internal.hpp"

using namespace lsq;

struct lsq_as_input {
	int columns = 0;                 // 4 (Fisher: A B C D) or n1 + n2
	std::vector<std::string> ids;
	std::vector<double> values;      // [rows][columns]: cells, counts or values
	std::vector<double> totals;      // LRT: [rows][columns] event totals; empty otherwise
	uint64_t left_out = 0;           // tables mode, Fisher: events without exactly two forms
};

namespace {

enum Test { T_FISHER, T_LRT, T_WILCOX, T_BETABIN, T_NONE };

// the tests that read a count and a total per sample
bool has_totals(Test t) { return t == T_LRT || t == T_BETABIN; }

Test test_of(const char *s) {
	if (!s) return T_NONE;
	if (strcmp(s, "fisher") == 0) return T_FISHER;
	if (strcmp(s, "lrt") == 0) return T_LRT;
	if (strcmp(s, "wilcox") == 0) return T_WILCOX;
	if (strcmp(s, "betabin") == 0) return T_BETABIN;
	return T_NONE;
}

// A field: a number, NA (NA, NaN, nan, -nan) or an infinity (Inf, -Inf, inf, -inf).
bool parse_field(const char *s, size_t len, double &v) {
	if (len == 0 || len > 63) return false;
	char b[64];
	memcpy(b, s, len);
	b[len] = 0;
	if (!strcmp(b, "NA") || !strcmp(b, "NaN") || !strcmp(b, "nan") || !strcmp(b, "-nan")) { v = NAN; return true; }
	if (!strcmp(b, "Inf") || !strcmp(b, "inf")) { v = INFINITY; return true; }
	if (!strcmp(b, "-Inf") || !strcmp(b, "-inf")) { v = -INFINITY; return true; }
	for (size_t i = 0; i < len; ++i)
		if (!strchr("0123456789+-.eE", b[i])) return false;
	char *e;
	errno = 0;
	v = strtod(b, &e);
	return e == b + len && e != b;
}

// One tab-separated text file, split into lines of fields (a trailing '\r' dropped, empty lines skipped).
struct Lines {
	std::string path, text;
	std::vector<uint64_t> line_no;                       // 1-based line number in the file
	std::vector<std::vector<std::pair<size_t, size_t>>> fields;      // (offset, length) into text
	std::string field(size_t row, size_t q) const { const auto &f = fields[row][q]; return text.substr(f.first, f.second); }
	const char *ptr(size_t row, size_t q) const { return text.data() + fields[row][q].first; }
	size_t len(size_t row, size_t q) const { return fields[row][q].second; }
};

int read_lines(const char *path, bool skip_header, Lines &L) {
	FILE *f = fopen(path, "rb");
	if (!f) return fail(LSQ_E_IO, "%s: cannot open: %s", path, strerror(errno));
	L.path = path;
	char buf[1 << 16];
	size_t n;
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) L.text.append(buf, n);
	const bool bad = ferror(f);
	fclose(f);
	if (bad) return fail(LSQ_E_IO, "%s: read error", path);
	size_t pos = 0;
	uint64_t no = 0;
	while (pos < L.text.size()) {
		size_t end = L.text.find('\n', pos);
		if (end == std::string::npos) end = L.text.size();
		size_t stop = end;
		if (stop > pos && L.text[stop - 1] == '\r') --stop;
		++no;
		if (!(skip_header && no == 1) && stop > pos) {
			std::vector<std::pair<size_t, size_t>> fl;
			size_t a = pos;
			for (;;) {
				size_t t = L.text.find('\t', a);
				if (t == std::string::npos || t > stop) t = stop;
				fl.emplace_back(a, t - a);
				if (t == stop) break;
				a = t + 1;
			}
			L.fields.push_back(std::move(fl));
			L.line_no.push_back(no);
		}
		pos = end + 1;
	}
	return LSQ_OK;
}

int number(const Lines &L, size_t row, size_t q, double &v) {
	if (!parse_field(L.ptr(row, q), L.len(row, q), v))
		return fail(LSQ_E_PARSE, "%s:%llu: field %zu is not a number: '%s'", L.path.c_str(), (unsigned long long)L.line_no[row], q + 1, L.field(row, q).c_str());
	return LSQ_OK;
}

int no_duplicates(const Lines &L, size_t id_col) {
	std::unordered_set<std::string> seen;
	seen.reserve(L.fields.size());
	for (size_t r = 0; r < L.fields.size(); ++r)
		if (!seen.insert(L.field(r, id_col)).second)
			return fail(LSQ_E_ARG, "%s:%llu: duplicate ID '%s'", L.path.c_str(), (unsigned long long)L.line_no[r], L.field(r, id_col).c_str());
	return LSQ_OK;
}

int too_few_for_betabin(int n1, int n2) {
	return fail(LSQ_E_ARG, "betabin needs at least 3 samples (n1 + n2 = %d): a mean per condition and one shared dispersion", n1 + n2);
}

int negative(const Lines &L, size_t row, double v) {
	return fail(LSQ_E_ARG, "%s:%llu: negative count %g", L.path.c_str(), (unsigned long long)L.line_no[row], v);
}

// The script's input (read.delim, header = T, row.names = 1): a header line, then an ID and `cols` values per line.
int read_matrix(const char *path, int cols, bool counts, Lines &L, std::vector<double> &vals) {
	int rc = read_lines(path, true, L);
	if (rc) return rc;
	vals.assign(L.fields.size() * (size_t)cols, 0.0);
	for (size_t r = 0; r < L.fields.size(); ++r) {
		if (L.fields[r].size() != (size_t)cols + 1)
			return fail(LSQ_E_ARG, "%s:%llu: %zu value columns, expected %d", path, (unsigned long long)L.line_no[r], L.fields[r].size() - 1, cols);
		for (int j = 0; j < cols; ++j) {
			double &v = vals[r * (size_t)cols + (size_t)j];
			if ((rc = number(L, r, (size_t)j + 1, v))) return rc;
			if (counts && std::rint(v) < 0) return negative(L, r, v);
		}
	}
	return no_duplicates(L, 0);
}

int read_matrix_input(Test t, int n_paths, const char *const *paths, int n1, int n2, lsq_as_input &in) {
	const int want_paths = has_totals(t) ? 2 : 1;
	if (n_paths != want_paths || !paths) return fail(LSQ_E_ARG, "%d matrix file(s) expected, %d given", want_paths, n_paths);
	for (int q = 0; q < n_paths; ++q) if (!paths[q]) return fail(LSQ_E_ARG, "null path");
	if (t != T_FISHER && (n1 < 1 || n2 < 1)) return fail(LSQ_E_ARG, "replicates per condition must be at least 1 (n1 = %d, n2 = %d)", n1, n2);
	if (t == T_BETABIN && n1 + n2 < 3) return too_few_for_betabin(n1, n2);
	const int cols = t == T_FISHER ? 2 : n1 + n2;
	Lines L;
	std::vector<double> v;
	int rc = read_matrix(paths[0], cols, t != T_WILCOX, L, v);
	if (rc) return rc;
	if (t == T_FISHER) {
		// rows in pairs (1,2), (3,4), ...; an odd last row is ignored; the ID is the second row's (Test_AS.r:36-45)
		const size_t n = L.fields.size() / 2;
		in.columns = 4;
		in.values.resize(n * 4);
		in.ids.resize(n);
		for (size_t q = 0; q < n; ++q) {
			const double *a = &v[2 * q * 2], *b = &v[(2 * q + 1) * 2];
			double *c = &in.values[q * 4];
			c[0] = a[0]; c[1] = a[1]; c[2] = b[0]; c[3] = b[1];
			in.ids[q] = L.field(2 * q + 1, 0);
		}
		return LSQ_OK;
	}
	in.columns = cols;
	in.values = std::move(v);
	in.ids.resize(L.fields.size());
	for (size_t r = 0; r < L.fields.size(); ++r) in.ids[r] = L.field(r, 0);
	if (has_totals(t)) {
		Lines L2;
		if ((rc = read_matrix(paths[1], cols, true, L2, in.totals))) return rc;
		for (size_t r = 0; r < std::max(L.fields.size(), L2.fields.size()); ++r) {
			if (r >= L.fields.size() || r >= L2.fields.size())
				return fail(LSQ_E_ARG, "%s and %s list different IDs: %zu and %zu rows", paths[0], paths[1], L.fields.size(), L2.fields.size());
			if (L2.field(r, 0) != in.ids[r])
				return fail(LSQ_E_ARG, "%s:%llu: ID '%s' where %s:%llu has '%s'", paths[1], (unsigned long long)L2.line_no[r], L2.field(r, 0).c_str(),
				            paths[0], (unsigned long long)L.line_no[r], in.ids[r].c_str());
		}
	}
	return LSQ_OK;
}

// One count table (M + 3 columns) or solve table (M + 5 columns) per sample, as `count` / `solve` print them: gene, the M
// event totals, form ID, then the form's count (count table) or theta (solve table).
int read_tables_input(Test t, int n_paths, const char *const *paths, int n1, int n2, lsq_as_input &in) {
	if (!paths) return fail(LSQ_E_ARG, "null argument");
	if (t == T_FISHER) { n1 = 1; n2 = 1; }
	if (n1 < 1 || n2 < 1) return fail(LSQ_E_ARG, "replicates per condition must be at least 1 (n1 = %d, n2 = %d)", n1, n2);
	if (t == T_BETABIN && n1 + n2 < 3) return too_few_for_betabin(n1, n2);
	if (n_paths != n1 + n2) return fail(LSQ_E_ARG, "n1 + n2 = %d tables expected, %d given", n1 + n2, n_paths);
	const int extra = t == T_WILCOX ? 5 : 3;
	std::vector<Lines> T((size_t)n_paths);
	int rc, M = -1;
	for (int s = 0; s < n_paths; ++s) {
		if (!paths[s]) return fail(LSQ_E_ARG, "null path");
		Lines &L = T[(size_t)s];
		if ((rc = read_lines(paths[s], false, L))) return rc;
		for (size_t r = 0; r < L.fields.size(); ++r) {
			const int cols = (int)L.fields[r].size();
			if (M < 0) {
				M = cols - extra;
				if (M < 1) return fail(LSQ_E_ARG, "%s:%llu: %d columns: not a %s table", paths[s], (unsigned long long)L.line_no[r], cols, t == T_WILCOX ? "solve" : "count");
			}
			if (cols != M + extra)
				return fail(LSQ_E_ARG, "%s:%llu: %d columns, expected %d (%d read files)", paths[s], (unsigned long long)L.line_no[r], cols, M + extra, M);
		}
		if (s > 0) {
			const Lines &F = T[0];
			for (size_t r = 0; r < std::max(F.fields.size(), L.fields.size()); ++r) {
				if (r >= F.fields.size() || r >= L.fields.size())
					return fail(LSQ_E_ARG, "%s and %s list different form IDs: %zu and %zu rows", paths[0], paths[s], F.fields.size(), L.fields.size());
				if (L.field(r, (size_t)M + 1) != F.field(r, (size_t)M + 1))
					return fail(LSQ_E_ARG, "%s:%llu: form ID '%s' where %s:%llu has '%s'", paths[s], (unsigned long long)L.line_no[r], L.field(r, (size_t)M + 1).c_str(),
					            paths[0], (unsigned long long)F.line_no[r], F.field(r, (size_t)M + 1).c_str());
			}
		}
	}
	if (M < 0) M = 1;
	if ((rc = no_duplicates(T[0], (size_t)M + 1))) return rc;
	const size_t rows = T[0].fields.size();
	const int N = n_paths;
	// per sample and form: the value (column M + 3) and the event total (sum of columns 2 .. M + 1)
	std::vector<double> val(rows * (size_t)N), tot(rows * (size_t)N);
	for (int s = 0; s < N; ++s) {
		const Lines &L = T[(size_t)s];
		for (size_t r = 0; r < rows; ++r) {
			double v, sum = 0.0;
			for (int m = 0; m < M; ++m) {
				if ((rc = number(L, r, (size_t)m + 1, v))) return rc;
				sum += v;
			}
			if ((rc = number(L, r, (size_t)M + 2, v))) return rc;
			if (t != T_WILCOX && (std::rint(v) < 0 || std::rint(sum) < 0)) return negative(L, r, std::rint(v) < 0 ? v : sum);
			val[r * (size_t)N + (size_t)s] = v;
			tot[r * (size_t)N + (size_t)s] = sum;
		}
	}
	const Lines &F = T[0];
	if (t == T_FISHER) {
		// one table per event (consecutive rows of one gene) with exactly two forms
		in.columns = 4;
		for (size_t r = 0; r < rows;) {
			size_t e = r + 1;
			while (e < rows && F.len(e, 0) == F.len(r, 0) && memcmp(F.ptr(e, 0), F.ptr(r, 0), F.len(r, 0)) == 0) ++e;
			if (e - r == 2) {
				const double c[4] = {val[r * 2], val[r * 2 + 1], val[(r + 1) * 2], val[(r + 1) * 2 + 1]};
				in.values.insert(in.values.end(), c, c + 4);
				in.ids.push_back(F.field(r + 1, (size_t)M + 1));
			} else {
				++in.left_out;
			}
			r = e;
		}
		return LSQ_OK;
	}
	in.columns = N;
	in.values = std::move(val);
	if (has_totals(t)) in.totals = std::move(tot);
	in.ids.resize(rows);
	for (size_t r = 0; r < rows; ++r) in.ids[r] = F.field(r, (size_t)M + 1);
	return LSQ_OK;
}

// R's as.character(double): 15 significant digits, trailing zeros dropped, fixed notation unless scientific is strictly
// shorter, exponents with a sign and at least two digits, NaN as NA.
void put_r(std::string &o, double v) {
	if (std::isnan(v)) { o += "NA"; return; }
	if (std::isinf(v)) { o += v > 0 ? "Inf" : "-Inf"; return; }
	if (v == 0.0) { o += "0"; return; }
	char b[64];
	snprintf(b, sizeof b, "%.14e", v);                    // [-]d.dddddddddddddde[+-]xx
	const char *p = b + (b[0] == '-');
	const char *e = strchr(p, 'e');
	const int exp10 = atoi(e + 1);
	int nsig = 15;
	while (nsig > 1 && p[nsig] == '0') --nsig;           // p[0] is the first digit, p[1] the point: digit q >= 2 is p[q]
	const int neg = v < 0;
	const int sci_w = neg + nsig + (nsig > 1 ? 1 : 0) + (std::abs(exp10) >= 100 ? 5 : 4);
	const int dec = std::max(0, nsig - 1 - exp10);
	const int fix_w = neg + (exp10 >= 0 ? exp10 + 1 : 1) + (dec ? dec + 1 : 0);
	if (fix_w <= sci_w) snprintf(b, sizeof b, "%.*f", dec, v);
	else snprintf(b, sizeof b, "%.*e", nsig - 1, v);
	o += b;
}

// The fitted full model of "betabin", printed between the ID and the statistic
struct BetabinFit { std::vector<double> mu1, mu2, rho; };

// The output table (Test_AS.r:45-47, :129-131, :173-175): header, then ID [psi1 psi2 rho] [stat] rawP bonP bhP per row.
std::string format_output(Test t, const lsq_as_input &in, const BetabinFit &fit, const std::vector<double> &stat, const std::vector<double> &p,
                          const std::vector<double> &bon, const std::vector<double> &bh) {
	const size_t n = in.ids.size();
	const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
	const size_t T = n < 16384 ? 1 : std::min<size_t>({8, hw, n / 8192});
	std::vector<std::string> parts(T);
	auto run = [&](size_t k) {
		std::string &o = parts[k];
		for (size_t i = n * k / T; i < n * (k + 1) / T; ++i) {
			o += in.ids[i]; o += '\t';
			if (t == T_BETABIN) { put_r(o, fit.mu1[i]); o += '\t'; put_r(o, fit.mu2[i]); o += '\t'; put_r(o, fit.rho[i]); o += '\t'; }
			if (t != T_FISHER) { put_r(o, stat[i]); o += '\t'; }
			put_r(o, p[i]); o += '\t'; put_r(o, bon[i]); o += '\t'; put_r(o, bh[i]); o += '\n';
		}
	};
	{
		ThreadGroup th;
		for (size_t k = 1; k < T; ++k) th.spawn([&run, k] { run(k); });
		th.run_here([&run] { run(0); });
		th.join();
		if (th.failed()) throw std::runtime_error("formatting the rows: " + th.error());
	}
	std::string o = t == T_FISHER ? "ID\trawP\tbonP\tbhP\n" : (t == T_LRT ? "ID\tLRT_statistics\trawP\tbonP\tbhP\n" :
	                (t == T_BETABIN ? "ID\tpsi1\tpsi2\trho\tLRT_statistics\trawP\tbonP\tbhP\n" : "ID\tDiff\trawP\tbonP\tbhP\n"));
	for (const auto &s : parts) o += s;
	return o;
}

bool positive_int(const char *s, int &v) {
	if (!s || !*s) return false;
	for (const char *q = s; *q; ++q) if (*q < '0' || *q > '9') return false;
	errno = 0;
	const long x = strtol(s, nullptr, 10);
	if (errno || x < 1 || x > 4096) return false;
	v = (int)x;
	return true;
}

const char *USAGE =
	"Usage:\n"
	"test_as fisher <count_matrix> <out>\n"
	"test_as lrt    <count_one_matrix> <count_all_matrix> <n1> <n2> <out>\n"
	"test_as wilcox <value_matrix> <n1> <n2> <out>\n"
	"test_as betabin <count_one_matrix> <count_all_matrix> <n1> <n2> <out>\n"
	"test_as fisher --tables <out> <count_table_a> <count_table_b>\n"
	"test_as lrt    --tables <n1> <n2> <out> <count_table_1> ... <count_table_{n1+n2}>\n"
	"test_as wilcox --tables <n1> <n2> <out> <solve_table_1> ... <solve_table_{n1+n2}>\n"
	"test_as betabin --tables <n1> <n2> <out> <count_table_1> ... <count_table_{n1+n2}>\n"
	"(<out> '-': standard output)";

} // namespace

namespace lsq {

// test_as (argv[0] ignored).  Exit status: 0, 1 for a usage or input error (reported before any HIP call), 2 otherwise.
int run_test_as(int argc, const char *const *argv, std::string &out) {
	const Test t = argc >= 2 ? test_of(argv[1]) : T_NONE;
	if (t == T_NONE) { cli_log(0, USAGE); return 1; }
	const bool tables = argc >= 3 && strcmp(argv[2], "--tables") == 0;
	int n1 = 1, n2 = 1;
	const char *out_path = nullptr;
	std::vector<const char *> inputs;
	const int a = tables ? 3 : 2;       // first argument after the mode
	if (tables) {
		if (t == T_FISHER) {
			if (argc != a + 3) { cli_log(0, USAGE); return 1; }
			out_path = argv[a];
			inputs.assign(argv + a + 1, argv + argc);
		} else {
			if (argc < a + 4) { cli_log(0, USAGE); return 1; }
			if (!positive_int(argv[a], n1) || !positive_int(argv[a + 1], n2)) { cli_log(0, "n1 and n2 must be whole numbers in [1, 4096]"); return 1; }
			out_path = argv[a + 2];
			inputs.assign(argv + a + 3, argv + argc);
		}
	} else {
		const int want = t == T_FISHER ? 2 : (has_totals(t) ? 5 : 4);
		if (argc != a + want) { cli_log(0, USAGE); return 1; }
		if (t == T_FISHER) { inputs.push_back(argv[a]); out_path = argv[a + 1]; }
		else {
			const int k = has_totals(t) ? 2 : 1;
			inputs.assign(argv + a, argv + a + k);
			if (!positive_int(argv[a + k], n1) || !positive_int(argv[a + k + 1], n2)) { cli_log(0, "n1 and n2 must be whole numbers in [1, 4096]"); return 1; }
			out_path = argv[a + k + 2];
		}
	}
	if (t == T_BETABIN && n1 + n2 < 3) { cli_log(0, USAGE); return 1; }
	lsq_as_input *raw = nullptr;
	int st = tables ? lsq_as_read_tables(argv[1], (int)inputs.size(), inputs.data(), n1, n2, &raw)
	                : lsq_as_read_matrix(argv[1], (int)inputs.size(), inputs.data(), n1, n2, &raw);
	if (st) { cli_log(0, lsq_last_error()); return st == LSQ_E_INTERNAL ? 2 : 1; }
	std::unique_ptr<lsq_as_input, void (*)(lsq_as_input *)> in(raw, lsq_as_input_free);
	const size_t n = in->ids.size();
	{
		char msg[256];
		snprintf(msg, sizeof msg, "%zu %s", n, t == T_FISHER ? "tables" : "rows");
		cli_log(2, msg);
		if (tables && t == T_FISHER) {
			snprintf(msg, sizeof msg, "left out %llu event(s) without exactly two forms", (unsigned long long)in->left_out);
			cli_log(2, msg);
		}
	}
	FILE *of = nullptr;
	if (strcmp(out_path, "-") != 0 && !(of = fopen(out_path, "w"))) {
		std::string msg = std::string(out_path) + ": cannot open for writing: " + strerror(errno);
		cli_log(0, msg.c_str());
		return 1;
	}
	std::unique_ptr<FILE, int (*)(FILE *)> close_of(of, [](FILE *f) { return f ? fclose(f) : 0; });
	lsq_ctx *c = nullptr;
	std::vector<double> stat(n, 0.0), p(n), bon(n), bh(n);
	BetabinFit fit;
	if (t == T_BETABIN) { fit.mu1.resize(n); fit.mu2.resize(n); fit.rho.resize(n); }
	st = lsq_ctx_create(cli_device(), &c);
	std::unique_ptr<lsq_ctx, void (*)(lsq_ctx *)> ctx(c, lsq_ctx_destroy);
	if (!st) {
		if (t == T_FISHER) st = lsq_as_fisher(c, n, in->values.data(), p.data());
		else if (t == T_LRT) st = lsq_as_lrt(c, n, n1, n2, in->values.data(), in->totals.data(), stat.data(), p.data());
		else if (t == T_BETABIN) st = lsq_as_betabin(c, n, n1, n2, in->values.data(), in->totals.data(), fit.mu1.data(), fit.mu2.data(), fit.rho.data(), stat.data(), p.data());
		else st = lsq_as_wilcox(c, n, n1, n2, in->values.data(), stat.data(), p.data());
	}
	if (!st) st = lsq_as_adjust(c, n, p.data(), bon.data(), bh.data());
	if (st) { cli_log(0, lsq_last_error()); return 2; }
	std::string text = format_output(t, *in, fit, stat, p, bon, bh);
	if (!of) { out = std::move(text); return 0; }
	if (fwrite(text.data(), 1, text.size(), of) != text.size() || fflush(of) != 0) {
		std::string msg = std::string(out_path) + ": write error: " + strerror(errno);
		cli_log(0, msg.c_str());
		return 2;
	}
	return 0;
}

} // namespace lsq

extern "C" {

int lsq_as_read_matrix(const char *test, int n_paths, const char *const *paths, int n1, int n2, lsq_as_input **out) LSQ_API_TRY {
	if (!out) return fail(LSQ_E_ARG, "null argument");
	*out = nullptr;
	const Test t = test_of(test);
	if (t == T_NONE) return fail(LSQ_E_ARG, "unknown test '%s' (fisher, lrt, wilcox, betabin)", test ? test : "(null)");
	std::unique_ptr<lsq_as_input> in(new lsq_as_input);
	const int rc = read_matrix_input(t, n_paths, paths, n1, n2, *in);
	if (rc) return rc;
	*out = in.release();
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_as_read_tables(const char *test, int n_paths, const char *const *paths, int n1, int n2, lsq_as_input **out) LSQ_API_TRY {
	if (!out) return fail(LSQ_E_ARG, "null argument");
	*out = nullptr;
	const Test t = test_of(test);
	if (t == T_NONE) return fail(LSQ_E_ARG, "unknown test '%s' (fisher, lrt, wilcox, betabin)", test ? test : "(null)");
	std::unique_ptr<lsq_as_input> in(new lsq_as_input);
	const int rc = read_tables_input(t, n_paths, paths, n1, n2, *in);
	if (rc) return rc;
	*out = in.release();
	return LSQ_OK;
} LSQ_API_CATCH

void lsq_as_input_free(lsq_as_input *in) { delete in; }
uint64_t lsq_as_input_rows(const lsq_as_input *in) { return in ? (uint64_t)in->ids.size() : 0; }
int lsq_as_input_columns(const lsq_as_input *in) { return in ? in->columns : 0; }
const char *lsq_as_input_id(const lsq_as_input *in, uint64_t row) { return in && row < in->ids.size() ? in->ids[(size_t)row].c_str() : nullptr; }
const double *lsq_as_input_values(const lsq_as_input *in) { return in && !in->values.empty() ? in->values.data() : nullptr; }
const double *lsq_as_input_totals(const lsq_as_input *in) { return in && !in->totals.empty() ? in->totals.data() : nullptr; }
uint64_t lsq_as_input_left_out(const lsq_as_input *in) { return in ? in->left_out : 0; }

int lsq_as_format_number(double v, char *buf, size_t cap) LSQ_API_TRY {
	if (!buf || cap == 0) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	put_r(o, v);
	if (o.size() + 1 > cap) return fail(LSQ_E_ARG, "buffer of %zu bytes too small", cap);
	memcpy(buf, o.c_str(), o.size() + 1);
	return LSQ_OK;
} LSQ_API_CATCH

} // extern "C"
