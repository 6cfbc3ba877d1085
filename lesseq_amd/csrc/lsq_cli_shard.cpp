// One count / solve job over several GPUs (LSQ_GPUS=N): the reference's scale-out -- a process per slice
// gene_begin_idx..gene_end_idx of the sorted gene list, stdout concatenated (count/count.cpp:204-215) -- inside one
// process: a host thread per GPU, slices of equal read weight (the first, unsharded count on GPU 0 is the pre-pass),
// every thread compiles the whole selected range (so the load-time filter is the unsharded one), takes its slice,
// ingests, counts, solves, packs its per-event records on its GPU; an RCCL all-gather (liblesseq_rccl.so, loaded here
// on demand; LSQ_GATHER=host moves the blocks through host memory instead -- for boxes where the "GPUs" are one device)
// puts the blocks together and thread 0 prints the table, byte-identical to the single-GPU run.  (ShardedJob: lsq_cli.hpp)
#include <dlfcn.h>

#include <algorithm>
#include <cstring>

#include "lsq_cli.hpp"
#include "lsq_readtool.hpp"
#include "lsq_team.hpp"

using namespace lsq;

namespace {

struct RcclApi {
	void *handle = nullptr;
	int (*init_all)(int, const int *, double, void **) = nullptr;     // lsq_comm_init_all_for
	void (*destroy)(void *) = nullptr, (*abort_comm)(void *) = nullptr;
	int (*gather)(lsq_ctx *, void *, const void *, void *, uint64_t) = nullptr;
	int (*allreduce_counts)(lsq_ctx *, void *, void *) = nullptr;
	const char *(*last_error)(void) = nullptr;
	std::string why;                       // dlerror() of the failing dlopen (read once: the call clears it)
	bool load() {
		Dl_info info;
		std::string dir;
		if (dladdr((const void *)&lsq_abi_version, &info) && info.dli_fname) { dir = info.dli_fname; const size_t s = dir.rfind('/'); dir = s == std::string::npos ? "" : dir.substr(0, s + 1); }
		handle = dlopen((dir + "liblesseq_rccl.so").c_str(), RTLD_NOW | RTLD_LOCAL);
		if (!handle) { if (const char *e = dlerror()) why = e; handle = dlopen("liblesseq_rccl.so", RTLD_NOW | RTLD_LOCAL); }
		if (!handle) { if (const char *e = dlerror()) { if (!why.empty()) why += "; "; why += e; } return false; }
		init_all = (int (*)(int, const int *, double, void **))dlsym(handle, "lsq_comm_init_all_for");
		destroy = (void (*)(void *))dlsym(handle, "lsq_comm_destroy");
		abort_comm = (void (*)(void *))dlsym(handle, "lsq_comm_abort");
		gather = (int (*)(lsq_ctx *, void *, const void *, void *, uint64_t))dlsym(handle, "lsq_gather");
		allreduce_counts = (int (*)(lsq_ctx *, void *, void *))dlsym(handle, "lsq_allreduce_counts");
		last_error = (const char *(*)(void))dlsym(handle, "lsq_rccl_last_error");
		return init_all && destroy && abort_comm && gather && allreduce_counts && last_error;
	}
};

// What both jobs need around their collective: how the blocks travel, the communicators, and the time limit (default 120 s).
// Nothing on this path waits without one: the communicator set-up, and the collective, whose kernel spins until every peer has joined it.
struct Collective {
	bool via_host = false; double time_limit = 120.0;
	RcclApi rccl; std::vector<void *> comms;
	Collective() {
		if (const char *e = getenv("LSQ_GATHER")) via_host = strcmp(e, "host") == 0;
		if (const char *e = getenv("LSQ_COLLECTIVE_TIMEOUT")) { const double v = atof(e); if (v > 0) time_limit = v; }
	}
	~Collective() { for (void *cm : comms) if (cm) rccl.destroy(cm); }
	// a communicator per slice; 0, or the exit status with the reason logged
	int init(const ShardedJob &J) {
		comms.assign((size_t)J.G, nullptr);
		if (via_host) return 0;
		if (!rccl.load()) { logf(0, "LSQ_GPUS=%d needs liblesseq_rccl.so beside the library (%s)", J.G, rccl.why.empty() ? "symbols missing" : rccl.why.c_str()); return 3; }
		if (rccl.init_all(J.G, J.devices.data(), time_limit, comms.data())) return job_failed(At::Device, 0, rccl.last_error());
		return 0;
	}
	// slice r waits for its collective, with the limit; on expiry it aborts its communicator, which ends the spinning kernel
	int wait(lsq_ctx *c, int r) {
		const int q = lsq_ctx_synchronize_for(c, time_limit);
		if (q == LSQ_E_TIMEOUT) { rccl.abort_comm(comms[(size_t)r]); comms[(size_t)r] = nullptr; }
		return q;
	}
};

// What a slice works on.  Slice 0 borrows the caller's context and events; every other slice makes its own -- a context on
// its device under the job's options, the whole selected range compiled -- and releases them with its scope.
struct SliceContext {
	lsq_ctx *c = nullptr; lsq_events *e = nullptr; bool own = true;
	SliceContext() = default; SliceContext(const SliceContext &) = delete;
	~SliceContext() { if (own) { if (c) lsq_ctx_destroy(c); lsq_events_free(e); } }
	void borrow(lsq_ctx *c0, lsq_events *e0) { c = c0; e = e0; own = false; }
	int create(const ShardedJob &J, int r) {
		int q = lsq_ctx_create(J.devices[(size_t)r], &c);
		if (!q) q = cli_env_options(c);
		return q ? q : lsq_events_compile_library(J.ann, J.M, J.types.data(), J.lens.data(), J.library, &e);
	}
};
// the developer's way to see the meeting at work: a slice whose number this variable holds fails where its job asks this
int failure_requested(SliceTeam &team, int r) {
	const char *fr = getenv("LSQ_FAIL_RANK");
	return fr && atoi(fr) == r ? team.fail(r, LSQ_E_STATE, "failure of this slice requested (LSQ_FAIL_RANK)") : LSQ_OK;
}
// the first failing slice in slice order speaks (read-sharded: file order -- a field that fails the cast: the reference reports the first such line)
int report_failure(const SliceTeam &team, const std::vector<int> &devices) {
	const int r = team.first_failure();
	if (r < 0) return 0;
	if (team.status(r) == LSQ_E_PARSE) return job_failed(At::ReadsFile, LSQ_E_PARSE, team.error(r).c_str());
	logf(0, "GPU %d: %s", devices[(size_t)r], team.error(r).c_str());
	return 3;
}
// G + 1 byte cuts of a file, moved to line starts (the first slice keeps the header line); false: the file does not open
bool line_cuts(const char *path, int G, std::vector<uint64_t> &cuts) {
	FILE *f = fopen(path, "rb");
	if (!f) return false;
	fseeko(f, 0, SEEK_END);
	const uint64_t size = (uint64_t)ftello(f);
	cuts.assign((size_t)G + 1, size); cuts[0] = 0;
	for (int r = 1; r < G; ++r) {
		uint64_t at = std::max(size / (uint64_t)G * (uint64_t)r, cuts[(size_t)r - 1]);
		fseeko(f, (off_t)at, SEEK_SET);
		for (int ch; at < size && (ch = fgetc(f)) != EOF;) { ++at; if (ch == '\n') break; }      // to the first byte after the next newline
		cuts[(size_t)r] = std::min(at, size);
	}
	fclose(f);
	return true;
}

} // namespace

// One read file into method m of a context: the staged text where there is one, else the file's text through the device
// parser, else -- name-keyed formats, strand strings beyond the device parser's 7 bytes -- the host parser.
int lsq::load_read_file(lsq_ctx *c, lsq_events *e, int m, const char *fmt, const char *path, lsq_text *staged_text) {
	int st = staged_text ? lsq_reads_upload_text(c, m, fmt, staged_text) : device_read_format(fmt) ? lsq_reads_upload_mrf(c, m, fmt, path) : LSQ_E_UNSUPPORTED;
	if (st != LSQ_E_UNSUPPORTED) return st;
	lsq_reads *rd = nullptr;
	st = lsq_reads_parse(fmt, path, e, 0, &rd);
	if (!st) { st = lsq_reads_upload(c, m, rd); lsq_reads_free(rd); }
	return st;
}

// The other way to cut one job (LSQ_SHARD=reads; SURVEY 8(e)'s alternative): every GPU takes a slice of the READS -- a byte
// range of each MRF file, cut at line starts, copied and parsed on that GPU only -- against ALL events; the slices' newline
// counts give every slice the file-wide number of its first line (read names "read-<line>" decide span-start ties,
// count/count.cpp:64-85,293-295); the class counts and matched bases are summed over the GPUs (integer sums: any order,
// count.cpp:378,467-482) with one ncclAllReduce (liblesseq_rccl's lsq_allreduce_counts; LSQ_GATHER=host: through host
// memory), and GPU 0 goes on with the sums as a single-GPU run does (EM, rows).  Here the loader scales with the GPUs (the
// event-sharded job parses the whole text on every GPU, twice); MRF_SINGLE files and genes within the kernels' limits only
// -- the caller falls back to the event-sharded job otherwise -- and an event inside the EM guard band cannot be replayed in
// per-read order (no GPU holds all of its reads): it keeps the kernel's numbers and is named at log level 1.
// On return ctx0 holds the whole job's counts (lsq_counts_import_device).
int lsq::run_read_sharded_job(const ShardedJob &J, lsq_ctx *ctx0, lsq_events *ev0) {
	const int G = J.G, M = J.M;
	Collective coll;
	if (const int rc = coll.init(J)) return rc;
	std::vector<std::vector<uint64_t>> cuts((size_t)M);
	for (int m = 0; m < M; ++m)
		if (!line_cuts(J.paths[(size_t)m], G, cuts[(size_t)m])) { logf(0, "cannot open reads file %s", J.paths[(size_t)m]); return EXIT_ABORT; }
	const uint64_t words = lsq_counts_device_words(ctx0);
	std::vector<std::vector<uint64_t>> lines((size_t)G, std::vector<uint64_t>((size_t)M, 0));     // newlines per slice and file
	std::vector<std::vector<uint64_t>> host_words(coll.via_host ? (size_t)G : 0, std::vector<uint64_t>(std::max<uint64_t>(words, 1), 0));
	std::vector<SliceContext> slices((size_t)G);
	slices[0].borrow(ctx0, ev0);
	SliceTeam team(G);
	team.run([&](int r) {
		SliceContext &S = slices[(size_t)r];
		std::vector<lsq_text *> text((size_t)M, nullptr);
		void *d_words = nullptr;
		// 1. context, event tables, this GPU's byte range of every file, its newline counts
		team.guard(r, lsq_last_error, [&]() -> int {
			int q;
			if (r > 0 && ((q = S.create(J, r)) || (q = lsq_events_upload(S.c, S.e)))) return q;
			for (int m = 0; m < M; ++m)
				if ((q = lsq_text_stage_range(S.c, J.paths[(size_t)m], cuts[(size_t)m][(size_t)r], cuts[(size_t)m][(size_t)r + 1], &text[(size_t)m])) ||
				    (q = lsq_text_lines(S.c, text[(size_t)m], &lines[(size_t)r][(size_t)m]))) return q;
			return LSQ_OK;
		});
		bool everyone = team.meet(r);
		// 2. parse and ingest the slice under its file-wide line numbers, count, hand the counters over
		if (everyone) team.guard(r, lsq_last_error, [&]() -> int {
			int q;
			for (int m = 0; m < M; ++m) {
				uint64_t before = 0;
				for (int p = 0; p < r; ++p) before += lines[(size_t)p][(size_t)m];
				if ((q = lsq_reads_upload_text_at(S.c, m, J.fmts[(size_t)m], text[(size_t)m], r == 0 ? 1 : 0, r == 0 ? 1 : before))) return q;
				lsq_text_free(text[(size_t)m]); text[(size_t)m] = nullptr;
			}
			if ((q = lsq_count(S.c)) || (q = lsq_device_alloc(S.c, std::max<uint64_t>(words, 1) * 8, &d_words))) return q;
			if (coll.via_host && ((q = lsq_counts_export_device(S.c, d_words)) || (q = lsq_device_read(S.c, host_words[(size_t)r].data(), d_words, words * 8)))) return q;
			return failure_requested(team, r);
		});
		everyone = team.meet(r);
		// 3. the sum over the GPUs; GPU 0 takes it as its counts
		if (everyone) team.guard(r, lsq_last_error, [&]() -> int {
			int q;
			if (!coll.via_host) {
				if ((q = coll.rccl.allreduce_counts(S.c, coll.comms[(size_t)r], d_words))) return team.fail(r, q, coll.rccl.last_error());
				if ((q = coll.wait(S.c, r))) return q;
			}
			if (r > 0) return LSQ_OK;
			if (coll.via_host) {
				for (int p = 1; p < G; ++p) for (uint64_t w = 0; w < words; ++w) host_words[0][(size_t)w] += host_words[(size_t)p][(size_t)w];
				if ((q = lsq_device_write(S.c, d_words, host_words[0].data(), words * 8))) return q;
			}
			return (q = lsq_counts_import_device(S.c, d_words)) ? q : lsq_ctx_synchronize(S.c);
		});
		for (auto *&t : text) { lsq_text_free(t); t = nullptr; }
		if (S.c) lsq_device_free(S.c, d_words);
		if (everyone && !team.status(r))
			logf(2, "GPU %d: bytes %llu..%llu of %s%s, %llu reads retained of them", J.devices[(size_t)r], (unsigned long long)cuts[0][(size_t)r], (unsigned long long)cuts[0][(size_t)r + 1],
			     J.paths[0], M > 1 ? " (and the like of the other files)" : "", (unsigned long long)lsq_reads_retained(S.c, 0));
	});
	if (const int rc = report_failure(team, J.devices)) return rc;
	uint64_t retained_all = 0;
	for (const SliceContext &S : slices) retained_all += lsq_reads_retained(S.c, 0);
	logf(2, "Sampling method #0: loaded %llu reads associated with the selected gene regions (over %d GPUs)", (unsigned long long)retained_all, G);
	return 0;
}

// the job sharded by events; ctx0 / ev0: GPU 0's context with the whole job counted on it (the pre-pass); texts0: its staged texts (kept)
int lsq::run_sharded_job(const ShardedJob &J, lsq_ctx *ctx0, lsq_events *ev0, const std::vector<lsq_text *> &texts0, const std::vector<double> &trb, std::string &out) {
	const int G = J.G, M = J.M;
	const int64_t n_ev = lsq_events_count(ev0);
	// pre-pass: reads per event from the unsharded count
	const size_t n_cls = (size_t)lsq_results_num_classes(ctx0);
	std::vector<uint64_t> cnt0(std::max<size_t>((size_t)M * n_cls, 1));
	int st = lsq_results_counts(ctx0, cnt0.data(), nullptr);
	if (st) return job_failed(At::Device, st);
	std::vector<uint64_t> coff((size_t)n_ev + 1);
	lsq_results_class_offsets(ctx0, coff.data());
	std::vector<double> weights((size_t)n_ev, 0.0);
	for (int64_t i = 0; i < n_ev; ++i)
		for (int m = 0; m < M; ++m)
			for (uint64_t k = coff[(size_t)i]; k < coff[(size_t)i + 1]; ++k) weights[(size_t)i] += (double)cnt0[(size_t)m * n_cls + k];
	std::vector<uint64_t> first((size_t)G), count((size_t)G);
	st = lsq_shard_bounds(ev0, G, weights.data(), first.data(), count.data());
	if (st) return job_failed(At::Results, st);
	uint64_t stride = 1;
	for (int r = 0; r < G; ++r) stride = std::max(stride, lsq_record_words(ev0, first[(size_t)r], count[(size_t)r]));
	std::vector<uint64_t> host_blocks((size_t)G * stride, 0);
	Collective coll;
	if (const int rc = coll.init(J)) return rc;
	std::vector<SliceContext> slices((size_t)G);
	slices[0].borrow(ctx0, ev0);
	// Every GPU's thread does its slice up to the packed block, then all of them MEET before any enters the collective
	// (lsq_team.hpp).  One failure -- no context, a file it cannot parse, out of memory: nobody gathers, the job exits 3 with the message.
	SliceTeam team(G);
	team.run([&](int r) {
		SliceContext &S = slices[(size_t)r];
		void *d_block = nullptr, *d_all = nullptr;
		uint32_t replayed = 0;
		team.guard(r, lsq_last_error, [&]() -> int {
			int s;
			if ((r > 0 && (s = S.create(J, r))) || (s = lsq_events_set_shard(S.e, first[(size_t)r], count[(size_t)r])) || (s = lsq_events_upload(S.c, S.e))) return s;
			for (int m = 0; m < M; ++m)
				if ((s = load_read_file(S.c, S.e, m, J.fmts[(size_t)m], J.paths[(size_t)m], r == 0 ? texts0[(size_t)m] : nullptr))) return s;
			if ((s = lsq_count(S.c)) || (s = lsq_solve(S.c)) || (s = lsq_solve_finalize(S.c, &replayed)) || (s = lsq_device_alloc(S.c, stride * 8, &d_block)) ||
			    (!coll.via_host && (s = lsq_device_alloc(S.c, (uint64_t)G * stride * 8, &d_all))) || (s = lsq_results_pack_device(S.c, d_block))) return s;
			return failure_requested(team, r);
		});
		const bool everyone = team.meet(r);
		if (everyone) team.guard(r, lsq_last_error, [&]() -> int {
			int s;
			if (coll.via_host) return lsq_device_read(S.c, host_blocks.data() + (size_t)r * stride, d_block, stride * 8);
			if ((s = coll.rccl.gather(S.c, coll.comms[(size_t)r], d_block, d_all, stride))) return team.fail(r, s, coll.rccl.last_error());
			if ((s = coll.wait(S.c, r)) || r > 0) return s;
			return lsq_device_read(S.c, host_blocks.data(), d_all, (uint64_t)G * stride * 8);
		});
		if (S.c) { lsq_device_free(S.c, d_all); lsq_device_free(S.c, d_block); }
		if (everyone && !team.status(r)) {
			unsigned long long pooled = 0;
			for (int m = 0; m < M; ++m) pooled += lsq_reads_pooled(S.c, m);
			logf(2, "GPU %d: events %llu..%llu of the sorted list, %llu reads pooled for them%s", J.devices[(size_t)r], (unsigned long long)first[(size_t)r],
			     (unsigned long long)(first[(size_t)r] + count[(size_t)r]), pooled, replayed ? " (guard-band events solved again in per-read order)" : "");
		}
	});
	if (const int rc = report_failure(team, J.devices)) return rc;
	// the whole job's tables, in output order
	const size_t n_iso = (size_t)lsq_events_total_isoforms(ev0);
	std::vector<uint64_t> cnt(std::max<size_t>((size_t)M * n_cls, 1)), bases(cnt.size());
	std::vector<double> theta(std::max<size_t>(n_iso, 1)), ll(std::max<size_t>((size_t)n_ev, 1));
	st = lsq_gathered_unpack(ev0, G, first.data(), count.data(), host_blocks.data(), stride, cnt.data(), bases.data(), theta.data(), ll.data());
	if (st) return job_failed(At::Results, st);
	char *text = nullptr;
	st = J.solve ? lsq_format_solve(ev0, M, cnt.data(), bases.data(), theta.data(), ll.data(), trb.data(), &text) : lsq_format_count(ev0, M, cnt.data(), &text);
	if (st || !text) return job_failed(At::Results, st);
	out.assign(text);
	free(text);
	logf(2, "Processed %lld genes on %d GPUs... Done", (long long)n_ev, G);
	return 0;
}
