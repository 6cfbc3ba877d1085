// Host side of the path, part 3: output rows (count/count.cpp:486-492, solve/solve.cpp:808-847), and the `#fim` and `#boot`
// lines that solve's extensions append behind them.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "lsq_cli.hpp"

using namespace lsq;

namespace {

// C++ `ostream << double` with default flags prints like printf("%g")
void put_g(std::string &o, double v) {
	char t[64];
	int n = snprintf(t, sizeof t, "%g", v);
	o.append(t, (size_t)n);
}

// The rows of the events [0, n), event by event in order: formatted by a few threads over contiguous runs of events
// (100 000 rows through the reference's six-digit formatting take 0.05 s on one core), joined in order.
template <class F>
std::string format_events_parallel(size_t n, F &&one) {
	const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
	const size_t T = n < 8192 ? 1 : std::min<size_t>({8, hw, n / 4096});
	std::vector<std::string> parts(T);
	auto run = [&](size_t k) { for (size_t i = n * k / T; i < n * (k + 1) / T; ++i) one(parts[k], i); };
	{
		ThreadGroup th;          // joined on every way out; a body's exception (out of memory) is rethrown here, on the caller's thread
		for (size_t k = 1; k < T; ++k) th.spawn([&run, k] { run(k); });
		th.run_here([&run] { run(0); });
		th.join();
		if (th.failed()) throw std::runtime_error("formatting the rows: " + th.error());
	}
	if (T == 1) return std::move(parts[0]);
	size_t total = 0;
	for (const auto &s : parts) total += s.size();
	std::string o;
	o.reserve(total);
	for (const auto &s : parts) o += s;
	return o;
}

void put_17g(std::string &o, double v) {
	char t[64];
	snprintf(t, sizeof t, "%.17g", v);
	o += t;
}

} // namespace

// `solve --fim`: one line per event and read file -- gene, file, fim.h's two variance estimates, the matrix row by row
int lsq::append_fim_lines(lsq_ctx *c, const lsq_events *e, int M, std::string &out) {
	int st = lsq_fim(c);
	if (st) return st;
	const int64_t n_ev = lsq_events_count(e);
	std::vector<uint64_t> off((size_t)n_ev + 1);
	lsq_results_fim_offsets(c, off.data());
	const size_t total = (size_t)off[(size_t)n_ev];
	std::vector<double> fim(std::max<size_t>((size_t)M * total, 1)), vd(std::max<size_t>((size_t)M * (size_t)n_ev, 1)), vi(vd.size());
	if ((st = lsq_results_fim(c, fim.data(), vd.data(), vi.data()))) return st;
	for (int64_t i = 0; i < n_ev; ++i)
		for (int m = 0; m < M; ++m) {
			out += "#fim\t"; out += lsq_events_gene_name(e, i); out += "\t"; out += std::to_string(m); out += "\t";
			put_17g(out, vd[(size_t)m * (size_t)n_ev + (size_t)i]); out += "\t"; put_17g(out, vi[(size_t)m * (size_t)n_ev + (size_t)i]);
			for (uint64_t q = off[(size_t)i]; q < off[(size_t)i + 1]; ++q) { out += "\t"; put_17g(out, fim[(size_t)m * total + (size_t)q]); }
			out += "\n";
		}
	return LSQ_OK;
}

// `solve --bootstrap B`: one line per event form -- gene, isoform, the replicates that solved, their five summaries (NA: no number)
int lsq::append_boot_lines(lsq_ctx *c, const lsq_events *e, unsigned long B, unsigned long seed, std::string &out) {
	int st = lsq_bootstrap(c, (uint32_t)B, (uint64_t)seed);
	if (st) return st;
	const size_t n_iso = std::max<size_t>((size_t)lsq_events_total_isoforms(e), 1);
	std::vector<uint32_t> n_ok(n_iso);
	std::vector<double> s[5];
	for (auto &v : s) v.resize(n_iso);
	if ((st = lsq_results_bootstrap(c, n_ok.data(), s[0].data(), s[1].data(), s[2].data(), s[3].data(), s[4].data()))) return st;
	size_t io = 0;
	for (int64_t i = 0, n_ev = lsq_events_count(e); i < n_ev; ++i)
		for (int j = 0; j < lsq_events_num_isoforms(e, i); ++j, ++io) {
			out += "#boot\t"; out += lsq_events_gene_name(e, i); out += "\t"; out += lsq_events_isoform_name(e, i, j);
			out += "\t"; out += std::to_string(n_ok[io]);
			for (const auto &v : s) {
				out += "\t";
				if (v[io] != v[io]) out += "NA"; else put_17g(out, v[io]);
			}
			out += "\n";
		}
	return LSQ_OK;
}

extern "C" {

int lsq_format_count(const lsq_events *E, int M, const uint64_t *cnt, char **out_text) LSQ_API_TRY {
	if (!E || !cnt || !out_text || M != E->n_methods) return fail(LSQ_E_ARG, "bad argument");
	const size_t n_cls = E->class_off.back();
	const std::string o = format_events_parallel(E->ev.size(), [&](std::string &o, size_t i) {
		const Event &e = E->ev[i];
		const size_t nc = (1u << e.K) - 1u;
		std::vector<double> supports(M, 0.0), iso_count(e.K, 0.0);
		for (int m = 0; m < M; ++m)
			for (size_t c = 1; c <= nc; ++c) {
				double v = (double)cnt[(size_t)m * n_cls + E->class_off[i] + c - 1];
				supports[m] += v;
				for (int j = 0; j < e.K; ++j) if (c >> j & 1) iso_count[j] += v;
			}
		for (int j = 0; j < e.K; ++j) {
			o += e.gname; o += '\t';
			for (int m = 0; m < M; ++m) { put_g(o, supports[m]); o += '\t'; }
			o += e.iso_names[j]; o += '\t'; put_g(o, iso_count[j]); o += '\n';
		}
	});
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_ARG, "out of memory");
} LSQ_API_CATCH

int lsq_format_solve(const lsq_events *E, int M, const uint64_t *cnt, const uint64_t *bases,
                     const double *theta, const double *logll, const double *total_read_bases, char **out_text) LSQ_API_TRY {
	if (!E || !cnt || !bases || !theta || !logll || !total_read_bases || !out_text || M != E->n_methods) return fail(LSQ_E_ARG, "bad argument");
	const size_t n_cls = E->class_off.back();
	const std::string o = format_events_parallel(E->ev.size(), [&](std::string &o, size_t i) {
		const Event &e = E->ev[i];
		const size_t nc = (1u << e.K) - 1u;
		std::vector<double> supports(M, 0.0), support_bases(M, 0.0);
		for (int m = 0; m < M; ++m) {
			uint64_t s = 0, b = 0;
			for (size_t c = 0; c < nc; ++c) { s += cnt[(size_t)m * n_cls + E->class_off[i] + c]; b += bases[(size_t)m * n_cls + E->class_off[i] + c]; }
			supports[m] = (double)s; support_bases[m] = (double)b;
		}
		const double *th = theta + E->iso_off[i];
		// solve/solve.cpp:808-821, same operation order
		std::vector<double> rpkm(e.K, 0.0);
		double total_read_mbases = 0.0;
		for (int m = 0; m < M; ++m) {
			total_read_mbases += total_read_bases[m] / 1.0E6;
			for (int j = 0; j < e.K; ++j) rpkm[j] += support_bases[m] * th[j];
		}
		for (int j = 0; j < e.K; ++j) {
			rpkm[j] /= ((double)e.iso_len[j] / 1.0E3);
			rpkm[j] /= total_read_mbases;
		}
		double sum_supports = 0.0;
		for (int m = 0; m < M; ++m) sum_supports += supports[m];
		for (int j = 0; j < e.K; ++j) {
			o += e.gname; o += '\t';
			for (int m = 0; m < M; ++m) { put_g(o, supports[m]); o += '\t'; }
			o += e.iso_names[j]; o += '\t'; put_g(o, th[j]); o += '\t'; put_g(o, rpkm[j]);
			if (sum_supports > 1E-5) { o += '\t'; put_g(o, logll[i] / sum_supports); o += '\n'; }
			else o += "\t0\n";
		}
	});
	*out_text = dup_text(o);
	return *out_text ? LSQ_OK : fail(LSQ_E_ARG, "out of memory");
} LSQ_API_CATCH

} // extern "C"
