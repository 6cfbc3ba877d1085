// What the units of the executables share (internal): the stderr log, the exit-status rules, the phase clock, the job handed
// to the sharded jobs.  lsq_cli.cpp: log, environment options, classify, bamcheck, the table of tools; lsq_cli_job.cpp: the
// count / solve job; lsq_cli_shard.cpp: that job over several GPUs; lsq_format.cpp: the output rows.
#pragma once

#include <chrono>
#include <cstdlib>
#include <string>
#include <vector>

#include "lsq_internal.hpp"
#include "lsq_jobargs.hpp"

namespace lsq {

// jsc/util/log.hpp:22-79: "[LOG YYYY-MM-DD hh:mm:ss LEVEL] text" on stderr when level <= reporting level
void logf(int level, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void set_cli_log_level(int level);       // the executables' reporting level, and the library's (lsq_set_log_level)

extern bool g_exit_after_output;         // set by lsq_cli_main
extern bool g_is_executable;             // set by lsq_cli_main: the process is ours alone

constexpr int EXIT_ABORT = 134;          // the reference dies on assert / an uncaught exception
int status_to_exit(int st);

// One rule for a failed call of count, solve or classify: the text to the log, and the exit status by where the job stands.
//   Annotation  loading the annotation, compiling the events: status_to_exit(st)
//   ReadsFile   opening, parsing, ingesting a read file: the Lexical_cast line behind the text for LSQ_E_PARSE; 3 for
//               LSQ_E_DEVICE, status_to_exit(st) for LSQ_E_IO, LSQ_E_FORMAT and LSQ_E_PARSE, else 2
//   Device      the context, an upload, a kernel, fetching its results: 3
//   Results     putting the fetched results together (shard bounds, unpacking, formatting): 2
// (the read-file tools have statuses of their own: cli_failed, lsq_readtool.hpp)
enum class At { Annotation, ReadsFile, Device, Results };
int job_failed(At at, int st, const char *text = lsq_last_error());

// developer aid: LSQ_CLI_TIMING=1 prints the seconds each phase took on stderr
struct PhaseTimer {
	bool on = getenv("LSQ_CLI_TIMING") != nullptr;
	std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
	void mark(const char *what) {
		if (!on) return;
		const auto n = std::chrono::steady_clock::now();
		fprintf(stderr, "[timing] %-28s %.3f s\n", what, std::chrono::duration<double>(n - t).count());
		t = n;
	}
};

// `count` and `classify` know LH_GENE_TXT and UCSC_GENE2ISOFORM only; LSQ_OK where lsq_annotation_load is to report an unopenable file
int count_formats_only(const char *iso_fmt, const char *iso_path, const char *g2i_fmt, const char *g2i_path);

// ---- lsq_cli_job.cpp
int run_count_solve(bool solve, int argc, const char *const *argv, std::string &out);

// ---- lsq_cli_shard.cpp: one job over several GPUs
struct ShardedJob {
	bool solve; int G; int M; int library;
	const lsq_annotation *ann;
	std::vector<const char *> fmts, types, paths;
	std::vector<uint64_t> lens;
	std::vector<int> devices;
};
int load_read_file(lsq_ctx *c, lsq_events *e, int m, const char *fmt, const char *path, lsq_text *staged_text);
int run_read_sharded_job(const ShardedJob &J, lsq_ctx *ctx0, lsq_events *ev0);
int run_sharded_job(const ShardedJob &J, lsq_ctx *ctx0, lsq_events *ev0, const std::vector<lsq_text *> &texts0, const std::vector<double> &trb, std::string &out);

// ---- lsq_format.cpp: the lines `solve --fim` / `--bootstrap B` append behind the table (JobArgs); a status other than LSQ_OK is the device's
int append_fim_lines(lsq_ctx *c, const lsq_events *e, int M, std::string &out);
int append_boot_lines(lsq_ctx *c, const lsq_events *e, unsigned long B, unsigned long seed, std::string &out);

} // namespace lsq
