// The read bootstrap of `solve`: B replicates of the latest count's class counts resampled on the device, each solved by
// the EM of lsq_em.hip, and theta summarised per isoform.  lsq_philox.hpp defines what a replicate draws; lsq_boot.cpp runs the same
// header on the host.
//   resample   work items are tiles of at most BOOT_TILE draws of one (read file, event); the tile table is a prefix sum over the
//              pairs' tile counts, made once per lsq_bootstrap from the counts as they lie in HBM.  A wave takes a tile: cumulative
//              counts (<= 63 classes) and a histogram in LDS, then 64-bit atomic adds to the replicate's [file][class] counts --
//              integer adds commute, so a replicate's counts do not depend on which wave adds first.  Grid y: the replicate of the chunk.
//   EM         run_boot_em (lsq_em.hip): the existing bodies, grid y the replicate.
//   summary    a workgroup per isoform sorts its <= 4096 replicate values in LDS.
#include "lsq_device.hpp"
#include "lsq_philox.hpp"
#include "lsq_scan.hpp"
#include "../../include/lesseq_hip_dev.h"

namespace {

constexpr unsigned BOOT_TILE = 4096;               // draws of a tile (even: a Philox block's two draws stay in one tile)
constexpr unsigned BOOT_MAX_REPLICATES = 4096;     // what the summary kernel sorts in LDS
constexpr unsigned BOOT_MAX_CLASSES = (1u << LSQ_MAX_ISOFORMS) - 1u;
constexpr unsigned BOOT_HIST_COPIES = 4;           // LDS histograms a wave spreads its adds over (a deep event has a handful of classes)
constexpr size_t BOOT_CHUNK_BYTES = (size_t)256 << 20;      // "bootstrap_chunk" 0: replicates whose count buffers stay below this
constexpr unsigned BOOT_NO_EVENT = 0xFFFFFFFFu;    // BootArgs::eid of an event evaluated on the host: not resampled
static_assert(BOOT_TILE % 2 == 0 && BOOT_MAX_CLASSES <= 64, "tile and class limits");

struct BootArgs {
	unsigned n_events, n_methods, n_pairs;
	size_t n_cls;                          // class slots of a read file (device order)
	const unsigned long long *cnt;         // [method][n_cls]: the counts resampled
	const unsigned char *K;
	const unsigned *cls_base;
	const unsigned *eid;                   // per device event: its index in output order (the generator's e), or BOOT_NO_EVENT
	unsigned long long *tiles;             // per pair p = method * n_events + event: its tiles ...
	const unsigned long long *tile_off;    // ... and their exclusive prefix sum (n_pairs + 1)
	unsigned long long n_tiles;
	unsigned long long seed;
	unsigned b0;                           // replicate of grid y = 0
	unsigned long long *out;               // [replicate of the chunk][method][n_cls], zero before the launch
};

// tiles per (read file, event)
__global__ void __launch_bounds__(256) lsq_boot_tiles_kernel(BootArgs A) {
	const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= A.n_pairs) return;
	const unsigned m = p / A.n_events, d = p - m * A.n_events;
	const unsigned K = A.K[d];
	unsigned long long n = 0;
	if (A.eid[d] != BOOT_NO_EVENT && K <= LSQ_MAX_ISOFORMS) {
		const unsigned long long *k = A.cnt + (size_t)m * A.n_cls + A.cls_base[d];
		for (unsigned q = 0; q < (1u << K) - 1u; ++q) n += k[q];
	}
	A.tiles[p] = n / BOOT_TILE + (n % BOOT_TILE ? 1ull : 0ull);
}

__global__ void __launch_bounds__(64) lsq_boot_resample_kernel(BootArgs A) {
	__shared__ unsigned long long cum[64];
	__shared__ unsigned hist[BOOT_HIST_COPIES][64];
	const unsigned long long tile = blockIdx.x;
	const unsigned lane = threadIdx.x;
	if (tile >= A.n_tiles) return;
	// the pair whose tiles hold this one: tile_off[p] <= tile < tile_off[p + 1] (pairs without reads have no tile)
	unsigned lo = 0, hi = A.n_pairs;
	while (hi - lo > 1u) {
		const unsigned mid = lo + (hi - lo) / 2u;
		if (A.tile_off[mid] <= tile) lo = mid; else hi = mid;
	}
	const unsigned m = lo / A.n_events, d = lo - m * A.n_events;
	const unsigned K = A.K[d], e = A.eid[d];
	if (K > LSQ_MAX_ISOFORMS || e == BOOT_NO_EVENT) return;         // (such a pair has no tile: lsq_boot_tiles_kernel)
	const unsigned nc = (1u << K) - 1u;
	const size_t slot0 = (size_t)m * A.n_cls + A.cls_base[d];
	cum[lane] = scan_wave_incl(lane < nc ? A.cnt[slot0 + lane] : 0ull);
#pragma unroll
	for (unsigned q = 0; q < BOOT_HIST_COPIES; ++q) hist[q][lane] = 0;
	__syncthreads();
	const unsigned long long n = cum[nc - 1u];
	const unsigned long long i0 = (tile - A.tile_off[lo]) * BOOT_TILE;
	if (i0 >= n) return;
	const unsigned long long i1 = n - i0 > BOOT_TILE ? i0 + BOOT_TILE : n;
	const unsigned b = A.b0 + blockIdx.y;
	unsigned *h = hist[lane % BOOT_HIST_COPIES];
	for (unsigned long long j = i0 / 2u + lane; 2u * j < i1; j += 64u) {
		const PhiloxBlock B = boot_block(A.seed, m, e, b, j);
		atomicAdd(&h[boot_class_of(cum, nc, mul_hi_u64(boot_bits(B, 0), n))], 1u);
		if (2u * j + 1u < i1) atomicAdd(&h[boot_class_of(cum, nc, mul_hi_u64(boot_bits(B, 1), n))], 1u);
	}
	__syncthreads();
	if (lane < nc) {
		unsigned long long k = 0;
#pragma unroll
		for (unsigned q = 0; q < BOOT_HIST_COPIES; ++q) k += hist[q][lane];
		if (k) atomicAdd(A.out + (size_t)blockIdx.y * ((size_t)A.n_methods * A.n_cls) + slot0 + lane, k);
	}
}

// One workgroup per isoform (device order): the replicates' finite values sorted in LDS (bitonic, the others as +inf behind
// them), then n_ok, the mean, the two-pass standard deviation (denominator n_ok - 1) and the quantiles 0.025, 0.5, 0.975 by
// linear interpolation at h = (n_ok - 1) p (R type 7).  The sums run over the sorted values in a fixed order.
__device__ inline double boot_block_sum(double x, double *red) {
	red[threadIdx.x] = x;
	__syncthreads();
	for (unsigned s = 128; s > 0; s >>= 1) {
		if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
		__syncthreads();
	}
	const double total = red[0];
	__syncthreads();
	return total;
}
__global__ void __launch_bounds__(256) lsq_boot_summary_kernel(const double *theta, unsigned B, size_t n_iso, unsigned *n_ok, double *stats) {
	__shared__ double v[BOOT_MAX_REPLICATES];
	__shared__ double red[256];
	const size_t iso = blockIdx.x;
	const unsigned tid = threadIdx.x;
	unsigned P = 2;
	while (P < B) P <<= 1;                                   // (B <= BOOT_MAX_REPLICATES, a power of two)
	const double inf = __longlong_as_double(0x7FF0000000000000ll);
	double mine = 0;
	for (unsigned b = tid; b < P; b += 256) {
		const double x = b < B ? theta[(size_t)b * n_iso + iso] : inf;
		const bool ok = fabs(x) < inf;                       // (false for no number)
		v[b] = ok ? x : inf;
		mine += ok ? 1.0 : 0.0;
	}
	const unsigned n = (unsigned)boot_block_sum(mine, red);  // (exact: at most 4096 ones; the call's barriers also cover v)
	for (unsigned k = 2; k <= P; k <<= 1)
		for (unsigned j = k >> 1; j > 0; j >>= 1) {
			for (unsigned i = tid; i < P; i += 256) {
				const unsigned q = i ^ j;
				if (q > i) {
					const double a = v[i], c = v[q];
					if ((a > c) == ((i & k) == 0u)) { v[i] = c; v[q] = a; }
				}
			}
			__syncthreads();
		}
	double s = 0;
	for (unsigned i = tid; i < n; i += 256) s += v[i];
	const double nan = __longlong_as_double(0x7FF8000000000000ll);
	const double mean = n ? boot_block_sum(s, red) / (double)n : nan;
	s = 0;
	for (unsigned i = tid; i < n; i += 256) { const double dx = v[i] - mean; s += dx * dx; }
	const double ss = boot_block_sum(s, red);
	if (tid == 0) {
		n_ok[iso] = n;
		stats[iso] = mean;
		stats[n_iso + iso] = n >= 2u ? sqrt(ss / (double)(n - 1u)) : nan;
		const double ps[3] = {0.025, 0.5, 0.975};
		for (int q = 0; q < 3; ++q) {
			double r = nan;
			if (n) {
				const double hh = (double)(n - 1u) * ps[q], fl = floor(hh);
				const unsigned at = (unsigned)fl;
				r = at + 1u < n ? v[at] + (hh - fl) * (v[at + 1u] - v[at]) : v[n - 1u];
			}
			stats[(size_t)(2 + q) * n_iso + iso] = r;
		}
	}
}

// what one lsq_bootstrap / lsq_bootstrap_replicate sets up once: the generator's event numbers and the tile table
struct BootPlan {
	DevBuf<unsigned> eid;
	DevBuf<unsigned long long> tiles, tile_off;
	ScanScratch scan;
	BootArgs A{};
};

int boot_plan(lsq_ctx *c, BootPlan &P) {
	const lsq_events &E = *c->E;
	const size_t n_ev = E.dev2out.size(), M = (size_t)E.n_methods;
	hipStream_t st = c->stream_em;
	std::vector<unsigned> eid(std::max<size_t>(n_ev, 1), BOOT_NO_EVENT);
	for (size_t d = 0; d < n_ev; ++d) eid[d] = (unsigned)E.dev2out[d];
	for (const BucketDesc &bd : E.buckets) if (bd.kind == 2) for (uint32_t q = 0; q < bd.n_events; ++q) eid[bd.ev_base + q] = BOOT_NO_EVENT;      // evaluated on the host
	if (n_ev * M > 0x7FFFFFFFull) return fail(LSQ_E_RANGE, "lsq_bootstrap: %zu (read file, event) pairs", n_ev * M);
	int rc;
	if ((rc = P.eid.alloc(eid.size()))) return rc;
	HIP_TRY(hipMemcpyAsync(P.eid.p, eid.data(), eid.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
	BootArgs &A = P.A;
	A.n_events = (unsigned)n_ev; A.n_methods = (unsigned)M; A.n_pairs = (unsigned)(n_ev * M); A.n_cls = E.n_cls_total;
	A.cnt = c->cnt.p; A.K = c->dK.p; A.cls_base = c->cls_base.p; A.eid = P.eid.p;
	if ((rc = P.tiles.alloc(A.n_pairs)) || (rc = P.tile_off.alloc((size_t)A.n_pairs + 1)) || (rc = P.scan.reserve(A.n_pairs))) return rc;
	A.tiles = P.tiles.p; A.tile_off = P.tile_off.p;
	if (A.n_pairs) {
		hipLaunchKernelGGL(lsq_boot_tiles_kernel, dim3(grid_for(A.n_pairs, 256)), dim3(256), 0, st, A);
		HIP_TRY(hipGetLastError());
	}
	if ((rc = device_scan<1, false, unsigned long long>(P.scan, P.tiles.p, A.n_pairs, P.tile_off.p, st))) return rc;
	HIP_TRY(hipMemcpyAsync(&A.n_tiles, P.tile_off.p + A.n_pairs, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));          // (the host vector and A.n_tiles)
	if (A.n_tiles > 0x7FFFFFFFull) return fail(LSQ_E_RANGE, "lsq_bootstrap: %llu tiles of %u draws a replicate (at most 2^31 - 1)", A.n_tiles, BOOT_TILE);
	return LSQ_OK;
}

// the replicates b0 .. b0 + n_rep - 1: counts into cnt ([n_rep][method][n_cls]), then their EM
int boot_chunk(lsq_ctx *c, BootPlan &P, unsigned long long seed, unsigned b0, unsigned n_rep, unsigned long long *cnt, double *theta, double *logll,
               unsigned *iters, unsigned char *flags, hipEvent_t *ev3) {
	hipStream_t st = c->stream_em;
	const size_t per = (size_t)P.A.n_methods * P.A.n_cls;
	if (ev3) HIP_TRY(hipEventRecord(ev3[0], st));
	if (per) HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)n_rep * per * sizeof(unsigned long long), st));
	if (P.A.n_tiles) {
		BootArgs A = P.A;
		A.seed = seed; A.b0 = b0; A.out = cnt;
		hipLaunchKernelGGL(lsq_boot_resample_kernel, dim3((unsigned)A.n_tiles, n_rep), dim3(64), 0, st, A);
		HIP_TRY(hipGetLastError());
	}
	if (ev3) HIP_TRY(hipEventRecord(ev3[1], st));
	const int rc = run_boot_em(c, n_rep, cnt, theta, logll, iters, flags);
	if (ev3) HIP_TRY(hipEventRecord(ev3[2], st));
	return rc;
}

// the outputs as no EM has written them yet: the theta of n_theta replicates no number (events evaluated on the host keep it),
// log-likelihoods, iteration counts and flags of n_rep replicates 0
int boot_clear(lsq_ctx *c, unsigned n_theta, double *theta, unsigned n_rep, double *logll, unsigned *iters, unsigned char *flags) {
	const size_t n_iso = c->E->n_iso_total, n_ev = c->E->dev2out.size();
	hipStream_t st = c->stream_em;
	if (n_iso) HIP_TRY(hipMemsetAsync(theta, 0xFF, (size_t)n_theta * n_iso * sizeof(double), st));
	if (n_ev) {
		HIP_TRY(hipMemsetAsync(logll, 0, (size_t)n_rep * n_ev * sizeof(double), st));
		HIP_TRY(hipMemsetAsync(iters, 0, (size_t)n_rep * n_ev * sizeof(unsigned), st));
		HIP_TRY(hipMemsetAsync(flags, 0, (size_t)n_rep * n_ev, st));
	}
	return LSQ_OK;
}

int boot_ready(lsq_ctx *c, const char *what) {
	if (!c) return fail(LSQ_E_ARG, "null context");
	if (!c->counted || !c->solved) return fail(LSQ_E_STATE, "%s: lsq_count and lsq_solve must come first", what);
	return LSQ_OK;
}

} // namespace

extern "C" {

int lsq_bootstrap_tile(void) { return (int)BOOT_TILE; }

int lsq_bootstrap(lsq_ctx *c, uint32_t n_replicates, uint64_t seed) LSQ_API_TRY {
	if (!c) return fail(LSQ_E_ARG, "null context");
	if (n_replicates < 1 || n_replicates > BOOT_MAX_REPLICATES) return fail(LSQ_E_ARG, "lsq_bootstrap: %u replicates (1 .. %u)", n_replicates, BOOT_MAX_REPLICATES);
	{ const int rc = boot_ready(c, "lsq_bootstrap"); if (rc) return rc; }
	HIP_TRY(hipSetDevice(c->device));
	const lsq_events &E = *c->E;
	BootState &S = c->boot;
	const unsigned B = n_replicates;
	const size_t n_iso = E.n_iso_total, n_ev = E.dev2out.size(), per = (size_t)E.n_methods * E.n_cls_total;
	S.done = false;
	// the store of the call before goes first: its bytes count as free below
	int rc;
	if ((rc = S.theta.alloc(0)) || (rc = S.stats.alloc(0)) || (rc = S.n_ok.alloc(0))) return rc;
	const size_t rep_bytes = per * sizeof(unsigned long long) + n_ev * (sizeof(double) + sizeof(unsigned) + 1);
	const size_t store_bytes = (size_t)B * n_iso * sizeof(double) + n_iso * (5 * sizeof(double) + sizeof(uint32_t));
	size_t free_b = 0, total_b = 0;
	HIP_TRY(hipMemGetInfo(&free_b, &total_b));
	unsigned chunk = S.opt_chunk ? S.opt_chunk : (unsigned)std::max<size_t>(1, BOOT_CHUNK_BYTES / std::max<size_t>(per * sizeof(unsigned long long), 1));
	chunk = std::min(chunk, B);
	if (store_bytes + (size_t)chunk * rep_bytes > free_b && !S.opt_chunk) chunk = (unsigned)std::max<size_t>(1, free_b > store_bytes ? (free_b - store_bytes) / std::max<size_t>(rep_bytes, 1) : 1);
	chunk = std::min(chunk, B);
	if (store_bytes + (size_t)chunk * rep_bytes > free_b)
		return fail(LSQ_E_RANGE, "lsq_bootstrap: the theta of %u replicates (%zu bytes) and a chunk of %u replicates (%zu bytes) exceed the %zu bytes free on the device",
		            B, store_bytes, chunk, (size_t)chunk * rep_bytes, free_b);
	if ((rc = S.theta.alloc((size_t)B * n_iso)) || (rc = S.stats.alloc(5 * n_iso)) || (rc = S.n_ok.alloc(n_iso))) return rc;
	DevBuf<unsigned long long> cnt;
	DevBuf<double> logll;
	DevBuf<unsigned> iters;
	DevBuf<unsigned char> flags;
	if ((rc = cnt.alloc((size_t)chunk * per)) || (rc = logll.alloc((size_t)chunk * n_ev)) || (rc = iters.alloc((size_t)chunk * n_ev)) || (rc = flags.alloc((size_t)chunk * n_ev))) return rc;
	BootPlan P;
	if ((rc = boot_plan(c, P))) return rc;
	hipStream_t st = c->stream_em;
	// device times of the three phases (lsq_set_timing): three marks a chunk, two around the summary
	const bool timed = c->time_events;
	const unsigned n_chunks = (B + chunk - 1) / chunk;
	std::vector<hipEvent_t> ev(timed ? 3 * (size_t)n_chunks + 2 : 0, nullptr);
	struct EvFree { std::vector<hipEvent_t> &v; ~EvFree() { for (hipEvent_t e : v) if (e) (void)hipEventDestroy(e); } } ev_free{ev};
	for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
	if ((rc = boot_clear(c, B, S.theta.p, chunk, logll.p, iters.p, flags.p))) return rc;          // (logll, iters, flags: a chunk's; nobody reads them)
	for (unsigned k = 0, b0 = 0; b0 < B; ++k, b0 += chunk) {
		const unsigned n_rep = std::min(chunk, B - b0);
		if ((rc = boot_chunk(c, P, seed, b0, n_rep, cnt.p, S.theta.p + (size_t)b0 * n_iso, logll.p, iters.p, flags.p, timed ? &ev[3 * (size_t)k] : nullptr))) return rc;
	}
	if (timed) HIP_TRY(hipEventRecord(ev[3 * (size_t)n_chunks], st));
	if (n_iso) {
		hipLaunchKernelGGL(lsq_boot_summary_kernel, dim3((unsigned)n_iso), dim3(256), 0, st, (const double *)S.theta.p, B, n_iso, S.n_ok.p, S.stats.p);
		HIP_TRY(hipGetLastError());
	}
	if (timed) HIP_TRY(hipEventRecord(ev[3 * (size_t)n_chunks + 1], st));
	HIP_TRY(hipStreamSynchronize(st));          // the chunk's buffers go out of scope
	S.timed = timed;
	if (timed) {
		S.ms[0] = S.ms[1] = S.ms[2] = 0;
		for (unsigned k = 0; k < n_chunks; ++k)
			for (int q = 0; q < 2; ++q) { float t = 0; HIP_TRY(hipEventElapsedTime(&t, ev[3 * (size_t)k + q], ev[3 * (size_t)k + q + 1])); S.ms[q] += t; }
		HIP_TRY(hipEventElapsedTime(&S.ms[2], ev[3 * (size_t)n_chunks], ev[3 * (size_t)n_chunks + 1]));
	}
	S.B = B; S.last_chunk = chunk; S.done = true;
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_results_bootstrap(lsq_ctx *c, uint32_t *n_ok, double *mean, double *sd, double *q025, double *q500, double *q975) LSQ_API_TRY {
	if (!c || !n_ok || !mean || !sd || !q025 || !q500 || !q975) return fail(LSQ_E_ARG, "null argument");
	if (!c->boot.done) return fail(LSQ_E_STATE, "lsq_bootstrap must come first");
	HIP_TRY(hipSetDevice(c->device));
	const lsq_events &E = *c->E;
	const size_t n_iso = E.n_iso_total;
	std::vector<double> hs(std::max<size_t>(5 * n_iso, 1));
	std::vector<uint32_t> hn(std::max<size_t>(n_iso, 1));
	HIP_TRY(hipStreamSynchronize(c->stream_em));
	if (n_iso) {
		HIP_TRY(hipMemcpy(hs.data(), c->boot.stats.p, 5 * n_iso * sizeof(double), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(hn.data(), c->boot.n_ok.p, n_iso * sizeof(uint32_t), hipMemcpyDeviceToHost));
	}
	double *const dst[5] = {mean, sd, q025, q500, q975};
	const double nan = std::nan("");
	for (size_t o = 0; o < E.ev.size(); ++o)          // events outside the shard: no replicate
		for (int j = 0; j < E.ev[o].K; ++j) { n_ok[E.iso_off[o] + j] = 0; for (double *p : dst) p[E.iso_off[o] + j] = nan; }
	for (size_t d = 0; d < E.dev2out.size(); ++d) {
		const size_t o = (size_t)E.dev2out[d];
		for (int j = 0; j < E.ev[o].K; ++j) {
			const size_t from = E.dev_iso_base[d] + (size_t)j, to = E.iso_off[o] + (size_t)j;
			n_ok[to] = hn[from];
			for (int q = 0; q < 5; ++q) dst[q][to] = hs[(size_t)q * n_iso + from];
		}
	}
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_results_bootstrap_theta(lsq_ctx *c, double *theta) LSQ_API_TRY {
	if (!c || !theta) return fail(LSQ_E_ARG, "null argument");
	if (!c->boot.done) return fail(LSQ_E_STATE, "lsq_bootstrap must come first");
	HIP_TRY(hipSetDevice(c->device));
	const lsq_events &E = *c->E;
	const size_t n_iso = E.n_iso_total, n_out = (size_t)E.iso_off.back(), B = c->boot.B;
	std::vector<double> h(std::max<size_t>(B * n_iso, 1));
	HIP_TRY(hipStreamSynchronize(c->stream_em));
	if (n_iso) HIP_TRY(hipMemcpy(h.data(), c->boot.theta.p, B * n_iso * sizeof(double), hipMemcpyDeviceToHost));
	const double nan = std::nan("");
	for (size_t i = 0; i < B * n_out; ++i) theta[i] = nan;
	for (size_t d = 0; d < E.dev2out.size(); ++d) {
		const size_t o = (size_t)E.dev2out[d];
		for (int j = 0; j < E.ev[o].K; ++j)
			for (size_t b = 0; b < B; ++b) theta[b * n_out + E.iso_off[o] + (size_t)j] = h[b * n_iso + E.dev_iso_base[d] + (size_t)j];
	}
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_bootstrap_replicate(lsq_ctx *c, uint64_t seed, uint32_t b, uint64_t *class_count, double *theta, double *logll, uint32_t *iters, uint8_t *flags) LSQ_API_TRY {
	if (!c || !class_count || !theta || !logll) return fail(LSQ_E_ARG, "null argument");
	if (b >= (1u << 24)) return fail(LSQ_E_ARG, "lsq_bootstrap_replicate: replicate %u (below 2^24)", b);
	{ const int rc = boot_ready(c, "lsq_bootstrap_replicate"); if (rc) return rc; }
	HIP_TRY(hipSetDevice(c->device));
	const lsq_events &E = *c->E;
	const size_t n_iso = E.n_iso_total, n_ev = E.dev2out.size(), M = (size_t)E.n_methods, n_cls = E.n_cls_total, n_out = (size_t)E.class_off.back();
	DevBuf<unsigned long long> d_cnt;
	DevBuf<double> d_theta, d_ll;
	DevBuf<unsigned> d_it;
	DevBuf<unsigned char> d_fl;
	int rc;
	if ((rc = d_cnt.alloc(M * n_cls)) || (rc = d_theta.alloc(n_iso)) || (rc = d_ll.alloc(n_ev)) || (rc = d_it.alloc(n_ev)) || (rc = d_fl.alloc(n_ev))) return rc;
	BootPlan P;
	if ((rc = boot_plan(c, P))) return rc;
	if ((rc = boot_clear(c, 1, d_theta.p, 1, d_ll.p, d_it.p, d_fl.p))) return rc;
	if ((rc = boot_chunk(c, P, seed, b, 1, d_cnt.p, d_theta.p, d_ll.p, d_it.p, d_fl.p, nullptr))) return rc;
	std::vector<unsigned long long> hc(std::max<size_t>(M * n_cls, 1));
	std::vector<double> ht(std::max<size_t>(n_iso, 1)), hl(std::max<size_t>(n_ev, 1));
	std::vector<uint32_t> hi(std::max<size_t>(n_ev, 1));
	std::vector<uint8_t> hf(std::max<size_t>(n_ev, 1));
	HIP_TRY(hipStreamSynchronize(c->stream_em));
	if (M * n_cls) HIP_TRY(hipMemcpy(hc.data(), d_cnt.p, M * n_cls * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	if (n_ev) {
		HIP_TRY(hipMemcpy(ht.data(), d_theta.p, n_iso * sizeof(double), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(hl.data(), d_ll.p, n_ev * sizeof(double), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(hi.data(), d_it.p, n_ev * sizeof(uint32_t), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(hf.data(), d_fl.p, n_ev * sizeof(uint8_t), hipMemcpyDeviceToHost));
	}
	const double nan = std::nan("");
	memset(class_count, 0, M * n_out * sizeof(uint64_t));
	for (size_t o = 0; o < E.ev.size(); ++o) {        // events outside the shard: no replicate
		for (int j = 0; j < E.ev[o].K; ++j) theta[E.iso_off[o] + j] = nan;
		logll[o] = 0.0;
		if (iters) iters[o] = 0;
		if (flags) flags[o] = 0;
	}
	for (size_t d = 0; d < n_ev; ++d) {
		const size_t o = (size_t)E.dev2out[d];
		const size_t nc = ((size_t)1 << E.ev[o].K) - 1u;
		for (size_t m = 0; m < M; ++m)
			for (size_t k = 0; k < nc; ++k) class_count[m * n_out + E.class_off[o] + k] = hc[m * n_cls + E.dev_cls_base[d] + k];
		for (int j = 0; j < E.ev[o].K; ++j) theta[E.iso_off[o] + j] = ht[E.dev_iso_base[d] + j];
		logll[o] = hl[d];
		if (iters) iters[o] = hi[d];
		if (flags) flags[o] = hf[d];
	}
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_debug_bootstrap_times(lsq_ctx *c, float ms[3], unsigned *chunk) LSQ_API_TRY {
	if (!c || !ms) return fail(LSQ_E_ARG, "null argument");
	if (!c->boot.done || !c->boot.timed) return fail(LSQ_E_STATE, "the last lsq_bootstrap ran without timing (lsq_set_timing)");
	for (int q = 0; q < 3; ++q) ms[q] = c->boot.ms[q];
	if (chunk) *chunk = c->boot.last_chunk;
	return LSQ_OK;
} LSQ_API_CATCH

} // extern "C"
