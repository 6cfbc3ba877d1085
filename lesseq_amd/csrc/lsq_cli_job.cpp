// count and solve: the reference's argv, stderr log and exit statuses (count/count.cpp:88-129, solve/solve.cpp:102-146) around
// the device path, as phases -- arguments (lsq_jobargs.hpp), environment, device start, annotation and events, reads, then
// either sharded job (lsq_cli_shard.cpp) or the single GPU's solve and rows.
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <thread>

#include "lsq_cli.hpp"
#include "lsq_readtool.hpp"

using namespace lsq;

namespace {

int usage(bool solve) {
	logf(0, "Usage:\n%s\n\tlog_level(0,1,2,...) proj_name out_prefix\n\tisoform_format isoforms_path g2i_format g2i_path gene_begin_idx gene_end_idx\n  (read_format read_type expected_read_length reads_path%s)+",
	     solve ? "solve" : "count", solve ? " total_read_bases" : "");
	return 1;
}

// What the environment and the annotation decide about a job beyond its argv
struct JobPlan {
	int library = LSQ_LIBRARY_UNSTRANDED;      // LSQ_LIBRARY=unstranded|forward|reverse; the argv stays the reference's
	int G = 1;                                 // LSQ_GPUS=N runs the job over N GPUs
	std::vector<int> devices;                  // LSQ_DEVICE picks the one (cli_device); LSQ_DEVICES="a,b,..." names the N, default 0..N-1
	bool shard_reads = false;                  // LSQ_SHARD=reads: the GPUs share the READS instead of the events (run_read_sharded_job): MRF_SINGLE files only
	const char *gather_mode = nullptr;         // LSQ_GATHER (set at all: the staged texts are kept for the event-sharded job, its one-slice self-check included)
	bool gather_self_check = false;            // LSQ_GPUS=1 with LSQ_GATHER=rccl spelled out: the event-sharded job with one slice
	std::vector<const char *> use_types;       // the read types the events are compiled with
	const char *bad_type = nullptr;            // the first read type that is neither SHORT_READ nor MEDIUM_READ
};

bool job_environment(const JobArgs &A, JobPlan &P) {
	if (!cli_library_env(P.library, false)) return false;
	const bool extensions = A.want_fim || A.boot_B;
	if (const char *e = getenv("LSQ_GPUS")) P.G = std::max(1, atoi(e));
	if (extensions) P.G = 1;
	if (const char *e = getenv("LSQ_DEVICES")) { const char *q = e; while (*q) { P.devices.push_back(atoi(q)); q = strchr(q, ','); if (!q) break; ++q; } }
	if (P.G > 1 && P.devices.size() < (size_t)P.G) { P.devices.clear(); for (int r = 0; r < P.G; ++r) P.devices.push_back(r); }
	if (P.G == 1) P.devices.assign(1, cli_device());
	P.devices.resize((size_t)P.G);
	P.gather_mode = getenv("LSQ_GATHER");
	P.gather_self_check = getenv("LSQ_GPUS") && P.gather_mode && strcmp(P.gather_mode, "rccl") == 0 && !extensions;
	if (const char *e = getenv("LSQ_SHARD")) P.shard_reads = strcmp(e, "reads") == 0 && P.G > 1 && !extensions;
	for (const char *f : A.fmts) if (strcmp(f, "MRF_SINGLE") != 0) P.shard_reads = false;
	if (P.shard_reads && P.library != LSQ_LIBRARY_UNSTRANDED) {
		logf(1, "LSQ_SHARD=reads: a stranded job (LSQ_LIBRARY=%s) is sharded by events instead", library_name(P.library));
		P.shard_reads = false;
	}
	return true;
}

// The device context (HIP start-up, a tenth of a second or more) is made on a second thread while the caller reads the
// annotation, and the same thread goes on to copy the text of every read file the device parses to HBM (that needs no event
// table); a file that does not open is left to the caller, which reports it.  Only an executable overlaps the two
// (lsq_cli_main: a process of its own, 0.1-0.3 s of HIP start-up to hide).  Inside a host process (lsq_cli_run) nothing is made
// before join(), and then on the calling thread, in order: the host may hold other contexts and other runtimes' threads, and a
// call that returns must leave no thread of its own behind.  The status is looked at only where the reference would be past
// every check it makes before the reads.
class DeviceStart {
	ThreadGroup thread_;
	std::atomic<int> ready_{0};            // 1: the context exists (the thread goes on to stage the reads' text), 2: the thread has given up
	int status_ = LSQ_OK;
	std::string error_;                    // the message lives in the thread that failed: kept here
	lsq_ctx *ctx_ = nullptr;
	bool taken_ = false, in_background_ = false, stage_texts_ = false;
	int device_ = 0;
	const std::vector<const char *> *paths_ = nullptr, *fmts_ = nullptr;
	std::vector<lsq_text *> texts_;
	void make() {
		status_ = lsq_ctx_create_with(device_, in_background_ ? LSQ_CTX_LANES_IN_BACKGROUND : 0u, &ctx_);
		if (!status_) status_ = cli_env_options(ctx_);
		if (status_) { error_ = lsq_last_error(); ready_.store(2, std::memory_order_release); return; }
		ready_.store(1, std::memory_order_release);
		if (!stage_texts_) return;
		for (size_t m = 0; m < texts_.size(); ++m)
			if (device_read_format((*fmts_)[m]) && lsq_text_stage(ctx_, (*paths_)[m], &texts_[m]) != LSQ_OK) texts_[m] = nullptr;
	}
public:
	// On every way out: the thread is joined first, so nothing is being written any more; then the staged texts go, and then --
	// unless the job took it, and frees it after this -- the context they lie in.
	~DeviceStart() {
		thread_.join();
		for (lsq_text *x : texts_) lsq_text_free(x);
		if (ctx_ && !taken_) lsq_ctx_destroy(ctx_);
	}
	// in_background: on a thread of its own, from now (an executable); else by join().  stage_texts: false where every GPU stages its own byte ranges later
	void start(int device, bool in_background, const std::vector<const char *> &paths, const std::vector<const char *> &fmts, bool stage_texts) {
		device_ = device; in_background_ = in_background; stage_texts_ = stage_texts; paths_ = &paths; fmts_ = &fmts;
		texts_.assign(paths.size(), nullptr);
		if (in_background_) thread_.spawn([this] { make(); });
	}
	// in the background only: until the thread has a context or has given up; true: context() is there, the texts still on their way
	bool wait_ready() {
		while (ready_.load(std::memory_order_acquire) == 0) std::this_thread::yield();
		return ready_.load(std::memory_order_acquire) == 1;
	}
	void join() {
		if (in_background_) thread_.join();
		else if (!ctx_ && status_ == LSQ_OK) make();
		if (thread_.failed() && status_ == LSQ_OK) { status_ = LSQ_E_INTERNAL; error_ = thread_.error(); }
	}
	int status() const { return status_; }
	const char *error() const { return error_.c_str(); }
	lsq_ctx *context() const { return ctx_; }
	lsq_ctx *take_context() { taken_ = true; return ctx_; }
	const std::vector<lsq_text *> &texts() const { return texts_; }
	lsq_text *text(int m) const { return texts_[(size_t)m]; }
	void release_text(int m) { lsq_text_free(texts_[(size_t)m]); texts_[(size_t)m] = nullptr; }
};

int load_annotation(bool solve, const JobArgs &A, lsq_annotation **a) {
	logf(2, "Loading isoforms...");
	const char *const *f = A.annotation;
	int st = solve ? LSQ_OK : count_formats_only(f[0], f[1], f[2], f[3]);
	if (!st) st = lsq_annotation_load(f[0], f[1], f[2], f[3], A.gb, A.ge, a);
	if (st) return job_failed(At::Annotation, st);
	logf(2, "Loaded %lld isoforms", (long long)lsq_annotation_num_isoforms_loaded(*a));
	logf(2, "Loaded %lld genes", (long long)lsq_annotation_num_genes_loaded(*a));
	logf(2, "Selected %lld gene(s)", (long long)lsq_annotation_num_genes(*a));
	return 0;
}

// An unknown read type is only noticed inside the per-gene loop of the reference (count/count.cpp:417-419), i.e. after every
// read file was loaded and only when at least one gene is selected; keep that precedence: compile with SHORT_READ in its place.
int compile_job_events(const JobArgs &A, JobPlan &P, const lsq_annotation *a, lsq_events **e) {
	P.use_types = A.types;
	for (int m = 0; m < A.M(); ++m)
		if (strcmp(A.types[m], "SHORT_READ") != 0 && strcmp(A.types[m], "MEDIUM_READ") != 0) {
			if (!P.bad_type) P.bad_type = A.types[m];
			P.use_types[m] = "SHORT_READ";
		}
	const int st = lsq_events_compile_library(a, A.M(), P.use_types.data(), A.lens.data(), P.library, e);
	if (st) return job_failed(At::Annotation, st);
	logf(2, "Built isoform structures for the %lld selected gene(s)", (long long)lsq_events_count(*e));
	return 0;
}
int unknown_read_type(const JobPlan &P) { logf(0, "Unknown read type error: %s", P.bad_type); return 1; }

// what the reference decides about a read file before it reads a line: the file opens (assert) and the format literal is known
// (the name-keyed formats: solve only, solve/solve.cpp:413,487,552)
int precheck_reads_file(const char *fmt, const char *path, bool solve) {
	FILE *f = fopen(path, "rb");
	if (!f) return fail(LSQ_E_IO, "cannot open reads file %s", path);
	fclose(f);
	const bool named = strcmp(fmt, "UCSC_GFF") == 0 || strcmp(fmt, "UCSC_BED") == 0 || strcmp(fmt, "WORMBASE_GFF3") == 0;
	if (!device_read_format(fmt) && !(solve && named)) return fail(LSQ_E_FORMAT, "Unknown file format error: %s", fmt);
	return LSQ_OK;
}

// The hand-over of the started device to the job, with the event tables on it.  An executable's second thread is still copying
// the reads' text to HBM when its context is ready: the event tables go up beside that copy (small uploads on the same stream,
// between two slices of the text), then this thread waits for the copy.  A context that failed is reported here, first.
int take_device(DeviceStart &dev, lsq_events *e, lsq_ctx **c, PhaseTimer &T) {
	if (g_is_executable) {
		const bool ready = dev.wait_ready();
		T.mark("wait for the device context");
		if (ready) {
			if (lsq_events_upload(dev.context(), e)) { const std::string msg = lsq_last_error(); dev.join(); return job_failed(At::Device, 0, msg.c_str()); }
			T.mark("event tables upload");
		}
	}
	dev.join();
	T.mark("wait for the text copy");
	if (dev.status()) return job_failed(At::Device, dev.status(), dev.error());
	*c = dev.take_context();
	if (!g_is_executable) {
		if (const int st = lsq_events_upload(*c, e)) return job_failed(At::Device, st);
		T.mark("event tables upload");
	}
	return 0;
}

// Every read file: prechecked, then (the device taken with the first) copied, parsed and ingested -- MRF text -> HBM -> parsed
// and ingested there; the name-keyed formats are grouped by name on the host first.  A read-sharded job only prechecks here.
int load_reads(bool solve, const JobArgs &A, JobPlan &P, DeviceStart &dev, lsq_events *e, lsq_ctx **c, PhaseTimer &T) {
	logf(2, "Loading the reads from %d sampling method(s)", A.M());
	for (int m = 0; m < A.M(); ++m) {
		int st = precheck_reads_file(A.fmts[m], A.paths[m], solve);
		if (st) return job_failed(At::ReadsFile, st);
		if (!*c) { const int rc = take_device(dev, e, c, T); if (rc) return rc; }
		if (P.shard_reads && lsq_events_host_genes(e) > 0) {
			logf(1, "LSQ_SHARD=reads: %lld gene(s) beyond the device kernels' limits need all of their reads in one place; the job is sharded by events instead", (long long)lsq_events_host_genes(e));
			P.shard_reads = false;
		}
		if (P.shard_reads) continue;          // (the files open and are MRF_SINGLE: the GPUs read their slices later)
		st = load_read_file(*c, e, m, A.fmts[m], A.paths[m], dev.text(m));
		if ((P.G == 1 && !P.gather_mode) || st) dev.release_text(m);      // several GPUs: GPU 0 ingests it again, for its slice
		if (st) return job_failed(At::ReadsFile, st);
		logf(2, "Sampling method #%d: loaded %llu reads associated with the selected gene regions", m, (unsigned long long)lsq_reads_retained(*c, m));
		// the library report of a stranded job's read file: how a wrongly chosen library type shows
		uint64_t lib[LIB_REPORT];
		if (lsq_events_library(e) != LSQ_LIBRARY_UNSTRANDED && lsq_last_library_report(*c, m, lib) == LSQ_OK)
			cli_log_library(("Sampling method #" + std::to_string(m)).c_str(), lsq_events_library(e), lib);
		T.mark("reads: copy, parse, ingest");
		if (T.on) { float h2d = 0, parse = 0; lsq_last_mrf_timing(*c, &h2d, &parse); fprintf(stderr, "[timing] %-28s %.3f s\n[timing] %-28s %.3f s\n", "  of which text copy", h2d * 1e-3, "  of which parse kernels", parse * 1e-3); }
	}
	return 0;
}

// An executable (lsq_cli_main) whose table is complete writes it and leaves.  Freeing gigabytes of HBM pools buffer by buffer,
// joining the helper threads and unloading the runtime is work the end of the process does for nothing.
// (profilers and coverage tools that write their output at exit want LSQ_CLI_TEARDOWN=1)
[[noreturn]] void leave_with(const std::string &out) {
	const bool written = fwrite(out.data(), 1, out.size(), stdout) == out.size() && fflush(stdout) == 0;
	if (!written) logf(0, "cannot write the table to stdout: %s", strerror(errno));
	fflush(stderr);
	_exit(written ? 0 : 2);
}

// the counted job on one GPU: solve, fetch, the rows and what the extensions append
int finish_single_gpu(bool solve, const JobArgs &A, lsq_ctx *c, lsq_events *e, std::string &out, PhaseTimer &T) {
	const int M = A.M();
	const int64_t n_ev = lsq_events_count(e);
	int st = solve ? lsq_solve(c) : LSQ_OK;
	if (st) return job_failed(At::Device, st);
	const size_t n_cls = (size_t)lsq_results_num_classes(c);
	std::vector<uint64_t> cnt(std::max<size_t>((size_t)M * n_cls, 1)), bases(cnt.size());
	if ((st = lsq_results_counts(c, cnt.data(), bases.data()))) return job_failed(At::Device, st);
	T.mark("count + solve + fetch");
	char *text = nullptr;
	if (!solve) {
		st = lsq_format_count(e, M, cnt.data(), &text);
	} else {
		std::vector<double> theta(std::max<size_t>((size_t)lsq_events_total_isoforms(e), 1)), ll(std::max<size_t>((size_t)n_ev, 1));
		std::vector<uint8_t> flags(std::max<size_t>((size_t)n_ev, 1));
		if ((st = lsq_results_solve(c, theta.data(), ll.data(), nullptr, flags.data()))) return job_failed(At::Device, st);
		for (int64_t i = 0; i < n_ev; ++i)
			if (flags[i] & 4) logf(3, "gene %s: EM stop criterion within the guard band of its threshold; solved again in per-read summation order", lsq_events_gene_name(e, i));
			else if (flags[i] & 1) logf(1, "gene %s: EM stop criterion within the guard band of its threshold and no exact-order replay was possible", lsq_events_gene_name(e, i));
		st = lsq_format_solve(e, M, cnt.data(), bases.data(), theta.data(), ll.data(), A.trb.data(), &text);
	}
	if (st || !text) return job_failed(At::Results, st);
	out.assign(text);
	free(text);
	if (A.want_fim && (st = append_fim_lines(c, e, M, out))) return job_failed(At::Device, st);
	if (A.boot_B && (st = append_boot_lines(c, e, A.boot_B, A.boot_seed, out))) return job_failed(At::Device, st);
	T.mark("format rows");
	logf(2, "Processed %lld genes... Done", (long long)n_ev);
	if (g_exit_after_output) leave_with(out);
	return 0;
}

} // namespace

int lsq::run_count_solve(bool solve, int argc, const char *const *argv, std::string &out) {
	PhaseTimer T;
	JobArgs A;
	const ArgsResult parsed = parse_job_args(solve, argc, argv, A);
	if (A.have_log_level) set_cli_log_level(A.log_level);
	switch (parsed) {
	case ArgsResult::Ok: break;
	case ArgsResult::Usage: return usage(solve);
	case ArgsResult::Abort: return EXIT_ABORT;
	case ArgsResult::BadNumber: logf(0, "%s", LEXICAL_CAST_ERROR); return 1;
	case ArgsResult::TooManyFiles: logf(0, "more than %d read files", LSQ_MAX_METHODS); return 2;
	}
	JobPlan P;
	if (!job_environment(A, P)) return 1;
	// (in this order: the device start goes first on every way out, then the context, the events, the annotation)
	CliOwned<lsq_annotation, lsq_annotation_free> ann;
	CliOwned<lsq_events, lsq_events_free> ev;
	CliOwned<lsq_ctx, lsq_ctx_destroy> ctx;
	DeviceStart dev;
	dev.start(P.devices[0], g_is_executable, A.paths, A.fmts, !P.shard_reads);
	if (const int rc = load_annotation(solve, A, &ann.p)) return rc;
	T.mark("annotation load");
	if (const int rc = compile_job_events(A, P, ann.p, &ev.p)) return rc;
	T.mark("event compile + device plan");
	if (const int rc = load_reads(solve, A, P, dev, ev.p, &ctx.p, T)) return rc;
	const int64_t n_ev = lsq_events_count(ev.p);
	// (read-sharded: the reads are loaded below, and a line that fails the cast there comes first, as in the reference)
	if (P.bad_type && n_ev > 0 && !P.shard_reads) return unknown_read_type(P);
	logf(2, "Processing reads info for genes");
	ShardedJob J{solve, P.G, A.M(), P.library, ann.p, A.fmts, P.use_types, A.paths, A.lens, P.devices};
	if (P.shard_reads && n_ev > 0) {
		const int rc = run_read_sharded_job(J, ctx.p, ev.p);
		T.mark("read-sharded ingest + count + sum");
		if (rc) return rc;
		if (P.bad_type) return unknown_read_type(P);
		J.G = P.G = 1;            // the sums are GPU 0's counts now: the rest is a single-GPU run
	} else if (const int st = lsq_count(ctx.p)) return job_failed(At::Device, st);
	uint64_t hg = 0, hr = 0;
	if (lsq_host_evaluated(ctx.p, &hg, &hr) == LSQ_OK && hg)
		logf(1, "%llu gene(s) beyond the device kernels' limits (more than %d isoforms or %d segments, or a cluster too large for the LDS) are evaluated on the host: %llu reads",
		     (unsigned long long)hg, LSQ_MAX_ISOFORMS, LSQ_MAX_SEGMENTS, (unsigned long long)hr);
	if ((P.G > 1 || P.gather_self_check) && n_ev > 0) {
		const int rc = run_sharded_job(J, ctx.p, ev.p, dev.texts(), A.trb, out);
		T.mark("sharded job");
		return rc;
	}
	return finish_single_gpu(solve, A, ctx.p, ev.p, out, T);
}
