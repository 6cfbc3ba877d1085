// The executables' frame: the stderr log, the exit-status rules, the environment's options, classify, bamcheck, and the one
// table of tools behind lsq_cli_main / lsq_cli_run.  (count / solve: lsq_cli_job.cpp; the output rows: lsq_format.cpp)
#include <cerrno>
#include <cstdarg>
#include <cstring>
#include <ctime>

#include "lsq_cli.hpp"
#include "lsq_readtool.hpp"
#include "lsq_localev.hpp"
#include "lsq_gtf.hpp"
#include "lsq_junc.hpp"
#include "lsq_cov.hpp"
#include "lsq_exonbins.hpp"
#include "lsq_libtype.hpp"
#include "lsq_psi.hpp"
#include "lsq_evidence.hpp"
#include "lsq_sites.hpp"
#include "lsq_retention.hpp"
#include "lsq_clusters.hpp"

using namespace lsq;

bool lsq::g_exit_after_output = false;
bool lsq::g_is_executable = false;

static int g_log_level = 2;
void lsq::set_cli_log_level(int level) { g_log_level = level; lsq_set_log_level(level); }

void lsq::logf(int level, const char *fmt, ...) {
	if (level > g_log_level) return;
	static const char *names[] = {"ERROR", "WARNING", "INFO", "DEBUG"};
	time_t raw; time(&raw);
	struct tm tmv; localtime_r(&raw, &tmv);
	char msg[2048];
	va_list ap; va_start(ap, fmt); vsnprintf(msg, sizeof msg, fmt, ap); va_end(ap);
	fprintf(stderr, "[LOG %d-%02d-%02d %02d:%02d:%02d %s] %s\n", tmv.tm_year + 1900, tmv.tm_mon + 1, tmv.tm_mday,
	        tmv.tm_hour, tmv.tm_min, tmv.tm_sec, names[level < 3 ? level : 3], msg);
	fflush(stderr);
}
void lsq::cli_log(int level, const char *text) { logf(level, "%s", text); }
int lsq::cli_device() { const char *e = getenv("LSQ_DEVICE"); return e ? atoi(e) : 0; }

int lsq::status_to_exit(int st) {
	switch (st) {
	case LSQ_OK: return 0;
	case LSQ_E_IO: return EXIT_ABORT;          // assert(ifs.is_open()) (count/count.cpp:139,185,278)
	case LSQ_E_FORMAT: case LSQ_E_PARSE: return 1;
	default: return 2;                         // conditions the reference has no defined behaviour for
	}
}

int lsq::job_failed(At at, int st, const char *text) {
	logf(0, "%s", text);
	switch (at) {
	case At::Annotation: return status_to_exit(st);
	case At::ReadsFile:
		if (st == LSQ_E_PARSE) logf(0, "%s", LEXICAL_CAST_ERROR);
		return st == LSQ_E_DEVICE ? 3 : st == LSQ_E_IO || st == LSQ_E_FORMAT || st == LSQ_E_PARSE ? status_to_exit(st) : 2;
	case At::Device: return 3;
	case At::Results: break;
	}
	return 2;
}

// `count` and `classify` know LH_GENE_TXT and UCSC_GENE2ISOFORM only (count/count.cpp:141,188,
// classify/classify.cpp:91,138); `solve` takes the wider set lsq_annotation_load reads.  The
// reference opens a file (assert) before it looks at the format literal.
int lsq::count_formats_only(const char *iso_fmt, const char *iso_path, const char *g2i_fmt, const char *g2i_path) {
	FILE *f = fopen(iso_path, "rb");
	if (!f) return LSQ_OK;                 // lsq_annotation_load reports the unopenable file
	fclose(f);
	if (strcmp(iso_fmt, "LH_GENE_TXT") != 0) return fail(LSQ_E_FORMAT, "Unknown file format error: %s", iso_fmt);
	f = fopen(g2i_path, "rb");
	if (!f) return LSQ_OK;
	fclose(f);
	if (strcmp(g2i_fmt, "UCSC_GENE2ISOFORM") != 0) return fail(LSQ_E_FORMAT, "Unknown file format error: %s", g2i_fmt);
	return LSQ_OK;
}

// LSQ_SAM_SKIP_FLAGS, LSQ_SAM_MIN_MAPQ, LSQ_BAM_VERIFY where they are set (cli_read_option_env; unset: the context's own
// default stays), then LSQ_OPTIONS="name=value,...": tuning knobs for lsq_ctx_set_option
int lsq::cli_env_options(lsq_ctx *c) {
	static const char *const option[3] = {"sam_skip_flags", "sam_min_mapq", "bam_verify"};
	const int st = cli_read_option_env([&](int k, unsigned long v) { return lsq_ctx_set_option(c, option[k], (double)v); });
	if (st) return st;
	const char *o = getenv("LSQ_OPTIONS");
	if (!o) return LSQ_OK;
	const std::string all(o);
	size_t pos = 0;
	while (pos < all.size()) {
		size_t end = all.find(',', pos);
		if (end == std::string::npos) end = all.size();
		const std::string item = all.substr(pos, end - pos);
		const size_t eq = item.find('=');
		if (eq != std::string::npos) { const int st = lsq_ctx_set_option(c, item.substr(0, eq).c_str(), atof(item.c_str() + eq + 1)); if (st) return st; }
		pos = end + 1;
	}
	return LSQ_OK;
}

namespace {

int run_classify(int argc, const char *const *argv, std::string &) {
	if (argc < 10) { logf(0, "Usage:\nclassify\n\tlog_level(0,1,2,...) proj_name out_prefix\n\tisoform_format isoforms_path g2i_format g2i_path gene_begin_idx gene_end_idx"); return 1; }
	long lvl;
	if (!cast_long(argv[1], lvl)) return EXIT_ABORT;
	set_cli_log_level((int)lvl);
	std::string out_prefix = argv[3];
	unsigned long gb, ge;
	if (!cast_ulong(argv[8], gb) || !cast_ulong(argv[9], ge)) { logf(0, "%s", LEXICAL_CAST_ERROR); return 1; }
	CliOwned<lsq_annotation, lsq_annotation_free> a;
	CliOwned<lsq_events, lsq_events_free> ev;
	int st = count_formats_only(argv[4], argv[5], argv[6], argv[7]);
	if (!st) st = lsq_annotation_load(argv[4], argv[5], argv[6], argv[7], gb, ge, &a.p);
	if (st) return job_failed(At::Annotation, st);
	logf(2, "Loaded %lld isoforms", (long long)lsq_annotation_num_isoforms_loaded(a.p));
	logf(2, "Loaded %lld genes", (long long)lsq_annotation_num_genes_loaded(a.p));
	st = compile_events(a.p, 0, nullptr, nullptr, false, LSQ_LIBRARY_UNSTRANDED, &ev.p);
	if (st) return job_failed(At::Annotation, st);
	size_t written = 0;
	for (const Event &e : ev.p->ev) {
		if (e.K < 2) continue;                                       // classify/classify.cpp:159
		std::string path = out_prefix + e.gname + ".matrix";
		FILE *f = fopen(path.c_str(), "w");
		if (!f) { logf(0, "cannot write %s", path.c_str()); return EXIT_ABORT; }
		fprintf(f, "%s\t%s\t", e.chrom.c_str(), e.strand.c_str());
		for (int n = 0; n < e.N; ++n) fprintf(f, "[%lld,%lld)-", (long long)e.seg_s[n], (long long)e.seg_e[n]);
		fputc('\n', f);
		const size_t nw = ((size_t)e.N + 63) / 64;        // any N: compile_events keeps the masks in iso_wide here
		for (int k = 0; k < e.K; ++k) {
			for (int n = 0; n < e.N; ++n) fprintf(f, "%d\t", (int)(e.iso_wide[(size_t)k * nw + (size_t)n / 64] >> (n % 64) & 1));
			fputc('\n', f);
		}
		fclose(f);
		++written;
	}
	logf(2, "Built isoform structures for the %zu selected gene(s)", written);
	return 0;
}

// bamcheck [--host] reads.bam: the whole-file check of a BAM file (lsq_bam_check; --host: lsq_bam_check_host, no GPU) -- a
// "key<TAB>value" line per field of the report on standard output.  Exit status 0; 1 with the message on standard error, and
// nothing on standard output, for a file that fails the check or does not open (as bam2mrf).
int run_bamcheck(int argc, const char *const *argv, std::string &out) {
	bool host = false, bad = false;
	const char *path = nullptr;
	for (int i = 1; i < argc && !bad; ++i) {
		if (strcmp(argv[i], "--host") == 0) host = true;
		else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else if (!path) path = argv[i];
		else bad = true;
	}
	if (bad || !path) { logf(0, "Usage:\nbamcheck [--host] bam_path"); return 1; }
	lsq_bam_report r;
	CliOwned<lsq_ctx, lsq_ctx_destroy> c;
	int st;
	if (host) st = lsq_bam_check_host(path, 0, &r);
	else {
		st = lsq_ctx_create(cli_device(), &c.p);
		if (!st) st = cli_env_options(c.p);
		if (!st) st = lsq_bam_check(c.p, path, &r);
	}
	if (st) { logf(0, "%s", lsq_last_error()); if (st == LSQ_E_PARSE) logf(0, "%s", LEXICAL_CAST_ERROR); return 1; }
	const std::pair<const char *, uint64_t> fields[] = {{"file_bytes", r.file_bytes}, {"blocks", r.blocks}, {"inflated_bytes", r.inflated_bytes}, {"header_lines", r.header_lines},
	                                                     {"references", r.references}, {"records", r.records}, {"reads", r.reads}, {"read_blocks", r.read_blocks},
	                                                     {"blocks_repaired", r.blocks_repaired}};
	for (const auto &f : fields) { out += f.first; out += '\t'; out += std::to_string(f.second); out += '\n'; }
	return 0;
}

// Every tool: its name, as lsq_cli_run takes it and as an executable's name holds it, and its function.  The order is the
// precedence among names that hold one another when an executable's own name chooses (lsq_cli_main): the first entry whose
// name is a substring of the program's, else the last one, count.
typedef int (*ToolFn)(int argc, const char *const *argv, std::string &out);
const struct Tool { const char *name; ToolFn run; } TOOLS[] = {
	{"libtype", run_libtype}, {"clusters", run_clusters}, {"retention", run_retention}, {"sites", run_sites}, {"evidence", run_evidence}, {"psi", run_psi},
	{"exonbins", run_exonbins}, {"coverage", run_coverage}, {"junctions", run_junctions},
	{"sam2mrf", [](int n, const char *const *v, std::string &o) { return run_sam2mrf(false, n, v, o); }},
	{"bam2mrf", [](int n, const char *const *v, std::string &o) { return run_sam2mrf(true, n, v, o); }},
	{"bamcheck", run_bamcheck}, {"parseGencode", run_parse_gencode}, {"gencodeIsoformMap", run_isoform_map}, {"events", run_events},
	{"test_as", run_test_as},
	{"solve", [](int n, const char *const *v, std::string &o) { return run_count_solve(true, n, v, o); }},
	{"classify", run_classify},
	{"count", [](int n, const char *const *v, std::string &o) { return run_count_solve(false, n, v, o); }},
};

} // namespace

extern "C" {

int lsq_cli_main(const char *tool, int argc, const char *const *argv) LSQ_API_TRY {
	g_is_executable = true;
	g_exit_after_output = getenv("LSQ_CLI_TEARDOWN") == nullptr;
	if (!tool) {
		const char *base = argc > 0 && argv && argv[0] ? argv[0] : "";
		if (const char *slash = strrchr(base, '/')) base = slash + 1;
		tool = "count";
		for (const Tool &t : TOOLS) if (strstr(base, t.name)) { tool = t.name; break; }
	}
	char *text = nullptr;
	int rc = lsq_cli_run(tool, argc, argv, &text);
	if (text) {
		const size_t n = strlen(text);
		if ((fwrite(text, 1, n, stdout) != n || fflush(stdout) != 0) && rc == 0) { logf(0, "cannot write the table to stdout: %s", strerror(errno)); rc = 2; }
		free(text);
	}
	return rc;
} LSQ_API_CATCH

int lsq_cli_run(const char *tool, int argc, const char *const *argv, char **out_text) LSQ_API_TRY {
	const Tool *chosen = nullptr;
	for (const Tool &t : TOOLS) if (tool && strcmp(tool, t.name) == 0) chosen = &t;
	if (!chosen) { fail(LSQ_E_ARG, "unknown tool"); return 2; }
	std::string out;
	const int rc = chosen->run(argc, argv, out);
	if (out_text) *out_text = dup_text(out);
	return rc;
} catch (...) {
	// exit status 2: "a condition the reference has no defined behaviour for" (it would have died of the exception)
	lsq::fail_exception(__func__);
	logf(0, "%s", lsq_last_error());
	return 2;
}

} // extern "C"
