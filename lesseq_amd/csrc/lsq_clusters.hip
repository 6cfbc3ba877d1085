// Intron clusters of several read files on the device (include/lesseq_hip.h, lsq_cl_device): eight phases over device
// arrays -- upload (the pooled rows as two-word records), sort (lsq_sort.hpp: by chromosome, start, end), reduce (run heads by
// lsq_scan.hpp, then a lane a record: the distinct introns with reads and samples, the count matrix), filter (the two row filters,
// the kept rows compacted), links (a kept row's predecessor with its start; a second sort of the kept rows' indices by
// (chromosome, end), then its predecessor with its end), components (below), totals (per component its size and reads, and for
// those of two rows or more their sums per sample), copy-back.  Statuses, numbering and texts are lsq_clusters.cpp's.
//
// Components.  label[k] <= k is a kept row of k's component, at first k itself.  A round is two launches.  hook: a lane a row, for
// each of its at most two links (u, v) the labels of the two labels (gu, gv) are compared and the larger side's label and row are
// lowered to the smaller (atomicMin).  jump: label[k] is lowered to label[label[k]].  Labels are read and lowered with agent-scope
// atomics only, values only ever fall, and every value a lane can read is a row of the same component: a stale read may cost a
// round, never a result.  A launch that lowers a label sets one word; the host reads it after the round and stops on 0.  Then
// every label is its own label (jump changed nothing) and equal across every link (hook changed nothing): the smallest row of the
// component, whatever order lanes and workgroups came in.  Nothing waits inside a kernel; what one round wrote is the next round's
// to see because a kernel boundary lies between.  Hooking the labels' labels with jumping halves the length of a chain of links a
// round (FastSV, Zhang, Azad and Hu 2020): rounds grow with its logarithm.  Every number is an integer and sums commute.
#include "lsq_wave.hpp"
#include "lsq_scan.hpp"
#include "lsq_sort.hpp"
#include "lsq_clusters.hpp"

namespace {

// A pooled record (lsq_clusters.hpp, the pool's own form): w0 = jn_key(start, end); w1 = chromosome index << 48 | sample << 32 | reads
constexpr unsigned long long CL_END_MASK = 0x7FFFFFFFull;      // jn_key's low 31 bits: the end, biased

// sorted records -> 1 where a run of one intron begins
__global__ void __launch_bounds__(256) lsq_cl_heads_kernel(const unsigned long long *w0, const unsigned long long *w1, unsigned long long n, unsigned *head) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i < n) head[i] = (i == 0 || w0[i] != w0[i - 1] || (w1[i] >> CL_CHROM_SHIFT) != (w1[i - 1] >> CL_CHROM_SHIFT)) ? 1u : 0u;
}

// A lane a sorted record; rid[i] = run heads ahead of i.  The head's lane writes the intron; every lane adds its reads to the
// intron's and to its cell of the count matrix, and the one add that finds the cell at 0 counts the sample.  (A run is as long as
// the samples that have the intron: the adds on one address are few.)
struct ClIntrons { unsigned *chrom; unsigned long long *key, *reads; unsigned *samples, *counts; };
__global__ void __launch_bounds__(256) lsq_cl_reduce_kernel(const unsigned long long *w0, const unsigned long long *w1, const unsigned *head, const unsigned long long *rid,
                                                            unsigned long long n, unsigned n_samples, ClIntrons O) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const unsigned h = head[i];
	const unsigned long long run = rid[i] + h - 1ull, b = w1[i];
	if (h) { O.chrom[run] = (unsigned)(b >> CL_CHROM_SHIFT); O.key[run] = w0[i]; }
	const unsigned reads = (unsigned)b, sample = (unsigned)(b >> 32) & 0xFFFFu;
	if (!reads) return;
	atomicAdd(&O.reads[run], (unsigned long long)reads);
	if (atomicAdd(&O.counts[run * n_samples + sample], reads) == 0u) atomicAdd(&O.samples[run], 1u);
}

// A lane a distinct intron: long, else weak, else kept
__global__ void __launch_bounds__(256) lsq_cl_filter_kernel(const unsigned long long *key, const unsigned long long *reads, unsigned n, unsigned long long min_reads, unsigned max_intron,
                                                            unsigned char *status, unsigned *keep) {
	const unsigned j = blockIdx.x * 256u + threadIdx.x;
	if (j >= n) return;
	const unsigned long long k = key[j];
	const unsigned char s = cl_long(jn_key_start(k), jn_key_end(k), max_intron) ? CL_LONG_ROW : reads[j] < min_reads ? CL_WEAK_ROW : CL_PRINTED;
	status[j] = s;
	keep[j] = s == CL_PRINTED ? 1u : 0u;
}

// kept rows compacted (at[j] = kept rows ahead of j); the end-order's records: w0 = the end, w1 = chromosome << 32 | the kept row's index
__global__ void __launch_bounds__(256) lsq_cl_compact_kernel(const unsigned *keep, const unsigned long long *at, const unsigned *chrom, const unsigned long long *key, unsigned n,
                                                             unsigned *kept_row, unsigned long long *e0, unsigned long long *e1) {
	const unsigned j = blockIdx.x * 256u + threadIdx.x;
	if (j >= n || !keep[j]) return;
	const unsigned k = (unsigned)at[j];
	kept_row[k] = j;
	e0[k] = key[j] & CL_END_MASK;
	e1[k] = ((unsigned long long)chrom[j] << 32) | k;
}

// A lane a kept row, in (chromosome, start, end) order: the row before it where that has its chromosome and start
__global__ void __launch_bounds__(256) lsq_cl_link_start_kernel(const unsigned *kept_row, const unsigned *chrom, const unsigned long long *key, unsigned nk, unsigned *pred_s) {
	const unsigned k = blockIdx.x * 256u + threadIdx.x;
	if (k >= nk) return;
	unsigned p = CL_NONE;
	if (k) {
		const unsigned a = kept_row[k - 1], b = kept_row[k];
		if (chrom[a] == chrom[b] && (key[a] >> 31) == (key[b] >> 31)) p = k - 1u;
	}
	pred_s[k] = p;
}
// A lane a place of the (chromosome, end) order: the row before it there where that has its chromosome and end (the sort is stable:
// of equal ends the smaller index comes first)
__global__ void __launch_bounds__(256) lsq_cl_link_end_kernel(const unsigned long long *e0, const unsigned long long *e1, unsigned nk, unsigned *pred_e) {
	const unsigned q = blockIdx.x * 256u + threadIdx.x;
	if (q >= nk) return;
	unsigned p = CL_NONE;
	if (q && e0[q] == e0[q - 1u] && (e1[q] >> 32) == (e1[q - 1u] >> 32)) p = (unsigned)e1[q - 1u];
	pred_e[(unsigned)e1[q]] = p;
}

__global__ void __launch_bounds__(256) lsq_cl_label_init_kernel(unsigned *label, unsigned nk) {
	const unsigned k = blockIdx.x * 256u + threadIdx.x;
	if (k < nk) label[k] = k;
}

__device__ inline unsigned cl_label(const unsigned *label, unsigned k) { return __hip_atomic_load(label + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline bool cl_lower(unsigned *label, unsigned k, unsigned v) { return atomicMin(label + k, v) > v; }

// one link: the side whose label's label is larger is hooked onto the other's -- its label, then the row itself
__device__ inline bool cl_hook(unsigned *label, unsigned u, unsigned v) {
	const unsigned pu = cl_label(label, u), pv = cl_label(label, v);
	const unsigned gu = cl_label(label, pu), gv = cl_label(label, pv);
	if (gu == gv) return false;
	const unsigned lo = min(gu, gv), hi_p = gu > gv ? pu : pv, hi = gu > gv ? u : v;
	const bool a = cl_lower(label, hi_p, lo), b = cl_lower(label, hi, lo);
	return a || b;
}
__device__ inline void cl_note_change(bool ch, unsigned *changed) {
	if (__any(ch) && (threadIdx.x & 63u) == 0u) atomicOr(changed, 1u);
}
// `keep` (null: every row) masks rows out of the components without a new compaction
__global__ void __launch_bounds__(256) lsq_cl_hook_kernel(unsigned *label, const unsigned *pred_s, const unsigned *pred_e, const unsigned char *keep, unsigned nk, unsigned *changed) {
	const unsigned k = blockIdx.x * 256u + threadIdx.x;
	bool ch = false;
	if (k < nk && (!keep || keep[k])) {
		const unsigned a = pred_s[k], b = pred_e[k];
		if (a != CL_NONE && (!keep || keep[a])) ch = cl_hook(label, k, a);
		if (b != CL_NONE && (!keep || keep[b])) ch = cl_hook(label, k, b) || ch;
	}
	cl_note_change(ch, changed);
}
__global__ void __launch_bounds__(256) lsq_cl_jump_kernel(unsigned *label, unsigned nk, unsigned *changed) {
	const unsigned k = blockIdx.x * 256u + threadIdx.x;
	bool ch = false;
	if (k < nk) {
		const unsigned p = cl_label(label, k), g = cl_label(label, p);
		if (g < p) ch = cl_lower(label, k, g);
	}
	cl_note_change(ch, changed);
}

// Per distinct intron its component's root (the smallest row of the component, as a distinct intron), and at the root the
// component's rows and reads
struct ClComps { unsigned *root, *size, *slot; unsigned long long *reads; };
__global__ void __launch_bounds__(256) lsq_cl_sizes_kernel(const unsigned *label, const unsigned *kept_row, const unsigned long long *reads, unsigned nk, ClComps C) {
	const unsigned k = blockIdx.x * 256u + threadIdx.x;
	if (k >= nk) return;
	const unsigned j = kept_row[k], r = kept_row[label[k]];
	C.root[j] = r;
	atomicAdd(&C.size[r], 1u);
	atomicAdd(&C.reads[r], reads[j]);
}
// 1 for a kept row that is the root of a component of two rows or more
__global__ void __launch_bounds__(256) lsq_cl_multi_kernel(const unsigned *label, const unsigned *kept_row, const unsigned *size, unsigned nk, unsigned *multi) {
	const unsigned k = blockIdx.x * 256u + threadIdx.x;
	if (k < nk) multi[k] = (label[k] == k && size[kept_row[k]] >= 2u) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) lsq_cl_slots_kernel(const unsigned *multi, const unsigned long long *at, const unsigned *kept_row, unsigned nk, unsigned *slot) {
	const unsigned k = blockIdx.x * 256u + threadIdx.x;
	if (k < nk && multi[k]) slot[kept_row[k]] = (unsigned)at[k];
}
// A lane a cell of the kept rows' part of the count matrix: added to its component's sum of that sample
__global__ void __launch_bounds__(256) lsq_cl_sample_totals_kernel(const unsigned *label, const unsigned *kept_row, const unsigned *counts, const unsigned *slot, unsigned nk,
                                                                   unsigned n_samples, unsigned *slot_totals) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i >= (unsigned long long)nk * n_samples) return;
	const unsigned k = (unsigned)(i / n_samples), s = (unsigned)(i % n_samples);
	const unsigned v = counts[(unsigned long long)kept_row[k] * n_samples + s];
	if (!v) return;
	const unsigned sl = slot[kept_row[label[k]]];
	if (sl != CL_NONE) atomicAdd(&slot_totals[(unsigned long long)sl * n_samples + s], v);
}

template <class T> int zeroed(DevBuf<T> &b, size_t n, int byte, hipStream_t st) {
	const int rc = b.alloc(n);
	if (rc) return rc;
	if (n) HIP_TRY(hipMemsetAsync(b.p, byte, n * sizeof(T), st));
	return LSQ_OK;
}
template <class T> int copy_back(std::vector<T> &to, const DevBuf<T> &from, size_t n, hipStream_t st) {
	if (n) HIP_TRY(hipMemcpyAsync(to.data(), from.p, n * sizeof(T), hipMemcpyDeviceToHost, st));
	return LSQ_OK;
}

} // namespace

int lsq::cl_device_solve(lsq_ctx *c, const lsq_cl_pool &p, uint64_t min_reads, uint32_t max_intron, ClSolved &S, float ms[CL_PHASES], uint32_t &rounds) {
	hipStream_t st = c->stream;
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	PhaseClock<CL_PHASES> PC;
	if ((rc = PC.make())) return rc;
	const unsigned long long np = p.key.size();
	const unsigned ns = p.n_samples;
	rounds = 0;
	for (int k = 0; k < CL_PHASES; ++k) ms[k] = 0;
	S.resize(0, ns);
	S.slot_totals.clear();
	if (!np) return LSQ_OK;

	// ---- upload: the pool keeps its rows as the records; their OR and AND came with them
	HIP_TRY(PC.mark(0, st));
	static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the pool's words are the records' words");
	const unsigned long long any[2] = {p.any[0], p.any[1]}, all[2] = {p.all[0], p.all[1]};
	SortBuf B;
	if ((rc = B.reserve(np))) return rc;
	HIP_TRY(hipMemcpyAsync(B.w0[0].p, p.key.data(), (size_t)np * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemcpyAsync(B.w1[0].p, p.rec.data(), (size_t)np * 8, hipMemcpyHostToDevice, st));

	// ---- sort: the digits of start and end, then the chromosome's; those on which every record agrees are left out
	HIP_TRY(PC.mark(1, st));
	{
		static const unsigned ALL_DIGITS[10] = {0, 8, 16, 24, 32, 40, 48, 56, 64 + CL_CHROM_SHIFT, 64 + CL_CHROM_SHIFT + 8};
		unsigned digits[10];
		const unsigned n_digits = sort_digits(any, all, ALL_DIGITS, 10, digits);
		if ((rc = device_radix_sort(B, digits, n_digits, st))) return rc;
	}

	// ---- reduce
	HIP_TRY(PC.mark(2, st));
	const unsigned long long *w0 = B.w0[B.cur].p, *w1 = B.w1[B.cur].p;
	DevBuf<unsigned> d_head, d_chrom, d_samples, d_counts;
	DevBuf<unsigned long long> d_rid, d_key, d_reads;
	ScanScratch SS;
	unsigned long long n_heads = 0;
	if ((rc = d_head.alloc((size_t)np)) || (rc = d_rid.alloc((size_t)np + 1)) || (rc = SS.reserve(np))) return rc;
	hipLaunchKernelGGL(lsq_cl_heads_kernel, dim3(grid_for(np, 256)), dim3(256), 0, st, w0, w1, np, d_head.p);
	HIP_TRY(hipGetLastError());
	if ((rc = device_scan<1, true>(SS, d_head.p, np, d_rid.p, st))) return rc;
	HIP_TRY(hipMemcpyAsync(&n_heads, d_rid.p + np, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (n_heads * ns > CL_MAX_CELLS) return fail(LSQ_E_RANGE, "%llu introns x %u samples: more than 2^31 cells in the count matrix", n_heads, ns);
	const unsigned n = (unsigned)n_heads;
	const size_t cells = (size_t)n * ns;
	if ((rc = d_chrom.alloc(n)) || (rc = d_key.alloc(n)) || (rc = zeroed(d_reads, n, 0, st)) || (rc = zeroed(d_samples, n, 0, st)) || (rc = zeroed(d_counts, cells, 0, st))) return rc;
	hipLaunchKernelGGL(lsq_cl_reduce_kernel, dim3(grid_for(np, 256)), dim3(256), 0, st, w0, w1, (const unsigned *)d_head.p, (const unsigned long long *)d_rid.p, np, ns,
	                   ClIntrons{d_chrom.p, d_key.p, d_reads.p, d_samples.p, d_counts.p});
	HIP_TRY(hipGetLastError());

	// ---- filter: the verdicts, the kept rows compacted, the end-order's records beside them
	HIP_TRY(PC.mark(3, st));
	DevBuf<unsigned char> d_status;
	DevBuf<unsigned> d_keep, d_kept_row;
	DevBuf<unsigned long long> d_at;
	unsigned long long n_kept = 0;
	if ((rc = d_status.alloc(n)) || (rc = d_keep.alloc(n)) || (rc = d_at.alloc((size_t)n + 1))) return rc;
	hipLaunchKernelGGL(lsq_cl_filter_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, (const unsigned long long *)d_key.p, (const unsigned long long *)d_reads.p, n,
	                   (unsigned long long)min_reads, max_intron, d_status.p, d_keep.p);
	HIP_TRY(hipGetLastError());
	if ((rc = device_scan<1, true>(SS, d_keep.p, n, d_at.p, st))) return rc;
	HIP_TRY(hipMemcpyAsync(&n_kept, d_at.p + n, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	const unsigned nk = (unsigned)n_kept;
	SortBuf E;                                  // the kept rows in (chromosome, end) order
	if ((rc = d_kept_row.alloc(nk)) || (rc = E.reserve(nk))) return rc;
	if (nk) {
		hipLaunchKernelGGL(lsq_cl_compact_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, (const unsigned *)d_keep.p, (const unsigned long long *)d_at.p, (const unsigned *)d_chrom.p,
		                   (const unsigned long long *)d_key.p, n, d_kept_row.p, E.w0[0].p, E.w1[0].p);
		HIP_TRY(hipGetLastError());
	}

	// ---- links: a digit on which the pooled records agree is one on which the kept rows agree
	HIP_TRY(PC.mark(4, st));
	DevBuf<unsigned> d_pred_s, d_pred_e, d_label, d_changed;
	if ((rc = d_pred_s.alloc(nk)) || (rc = d_pred_e.alloc(nk)) || (rc = d_label.alloc(nk)) || (rc = d_changed.alloc(1))) return rc;
	if (nk) {
		static const unsigned END_DIGITS[6] = {0, 8, 16, 24, 64 + 32, 64 + 40};
		unsigned digits[6];
		const unsigned long long e_any[2] = {any[0] & CL_END_MASK, (any[1] >> CL_CHROM_SHIFT) << 32}, e_all[2] = {all[0] & CL_END_MASK, (all[1] >> CL_CHROM_SHIFT) << 32};
		const unsigned n_digits = sort_digits(e_any, e_all, END_DIGITS, 6, digits);
		hipLaunchKernelGGL(lsq_cl_link_start_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, st, (const unsigned *)d_kept_row.p, (const unsigned *)d_chrom.p, (const unsigned long long *)d_key.p,
		                   nk, d_pred_s.p);
		HIP_TRY(hipGetLastError());
		if ((rc = device_radix_sort(E, digits, n_digits, st))) return rc;
		hipLaunchKernelGGL(lsq_cl_link_end_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, st, (const unsigned long long *)E.w0[E.cur].p, (const unsigned long long *)E.w1[E.cur].p, nk, d_pred_e.p);
		HIP_TRY(hipGetLastError());
	}

	// ---- components: a round is a hook and a jump; the host reads the round's word
	HIP_TRY(PC.mark(5, st));
	if (nk) {
		hipLaunchKernelGGL(lsq_cl_label_init_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, st, d_label.p, nk);
		HIP_TRY(hipGetLastError());
		for (unsigned changed = 1; changed;) {
			if (rounds >= 100000u) return fail(LSQ_E_INTERNAL, "the components had not settled after %u rounds", rounds);
			HIP_TRY(hipMemsetAsync(d_changed.p, 0, 4, st));
			hipLaunchKernelGGL(lsq_cl_hook_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, st, d_label.p, (const unsigned *)d_pred_s.p, (const unsigned *)d_pred_e.p,
			                   (const unsigned char *)nullptr, nk, d_changed.p);
			hipLaunchKernelGGL(lsq_cl_jump_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, st, d_label.p, nk, d_changed.p);
			HIP_TRY(hipGetLastError());
			HIP_TRY(hipMemcpyAsync(&changed, d_changed.p, 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			++rounds;
		}
	}

	// ---- totals
	HIP_TRY(PC.mark(6, st));
	DevBuf<unsigned> d_root, d_csize, d_cslot, d_multi, d_slot_totals;
	DevBuf<unsigned long long> d_creads, d_slot_at;
	unsigned long long n_slots = 0;
	if ((rc = zeroed(d_root, n, 0xFF, st)) || (rc = zeroed(d_csize, n, 0, st)) || (rc = zeroed(d_cslot, n, 0xFF, st)) || (rc = zeroed(d_creads, n, 0, st)) ||
	    (rc = d_multi.alloc(nk)) || (rc = d_slot_at.alloc((size_t)nk + 1)) || (rc = SS.reserve(nk))) return rc;
	if (nk) {
		const ClComps C{d_root.p, d_csize.p, d_cslot.p, d_creads.p};
		hipLaunchKernelGGL(lsq_cl_sizes_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, st, (const unsigned *)d_label.p, (const unsigned *)d_kept_row.p, (const unsigned long long *)d_reads.p, nk, C);
		hipLaunchKernelGGL(lsq_cl_multi_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, st, (const unsigned *)d_label.p, (const unsigned *)d_kept_row.p, (const unsigned *)d_csize.p, nk, d_multi.p);
		HIP_TRY(hipGetLastError());
		if ((rc = device_scan<1, true>(SS, d_multi.p, nk, d_slot_at.p, st))) return rc;
		HIP_TRY(hipMemcpyAsync(&n_slots, d_slot_at.p + nk, 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	const size_t slot_cells = (size_t)n_slots * ns;
	if ((rc = zeroed(d_slot_totals, slot_cells, 0, st))) return rc;
	if (n_slots) {
		hipLaunchKernelGGL(lsq_cl_slots_kernel, dim3(grid_for(nk, 256)), dim3(256), 0, st, (const unsigned *)d_multi.p, (const unsigned long long *)d_slot_at.p, (const unsigned *)d_kept_row.p, nk,
		                   d_cslot.p);
		hipLaunchKernelGGL(lsq_cl_sample_totals_kernel, dim3(grid_for((unsigned long long)nk * ns, 256)), dim3(256), 0, st, (const unsigned *)d_label.p, (const unsigned *)d_kept_row.p,
		                   (const unsigned *)d_counts.p, (const unsigned *)d_cslot.p, nk, ns, d_slot_totals.p);
		HIP_TRY(hipGetLastError());
	}

	// ---- copy-back
	HIP_TRY(PC.mark(7, st));
	S.resize(n, ns);
	S.slot_totals.resize(slot_cells);
	if ((rc = copy_back(S.chrom, d_chrom, n, st)) || (rc = copy_back(S.status, d_status, n, st)) || (rc = copy_back(S.samples, d_samples, n, st)) ||
	    (rc = copy_back(S.counts, d_counts, cells, st)) || (rc = copy_back(S.root, d_root, n, st)) || (rc = copy_back(S.comp_size, d_csize, n, st)) ||
	    (rc = copy_back(S.comp_slot, d_cslot, n, st)) || (rc = copy_back(S.slot_totals, d_slot_totals, slot_cells, st))) return rc;
	HIP_TRY(hipMemcpyAsync(S.key.data(), d_key.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(S.reads.data(), d_reads.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(S.comp_reads.data(), d_creads.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(PC.mark(8, st));
	HIP_TRY(hipStreamSynchronize(st));
	for (int k = 0; k < CL_PHASES; ++k) (void)PC.ms(k, &ms[k]);
	return LSQ_OK;
}

extern "C" int lsq_cl_device(lsq_ctx *c, const lsq_cl_pool *p, uint64_t min_reads, uint32_t max_intron, uint64_t min_cluster_reads, lsq_cl_table **out) LSQ_API_TRY {
	if (!c || !p || !out) return fail(LSQ_E_ARG, "null argument");
	if (max_intron > 0x7FFFFFFFu) return fail(LSQ_E_ARG, "max_intron must be below 2^31");
	const int rc = cl_check_pool(*p);
	if (rc) return rc;
	return new_table(out, [&](lsq_cl_table &t) {
		ClSolved S;
		const int st = cl_device_solve(c, *p, min_reads, max_intron, S, t.ms, t.rounds);
		return st ? st : cl_finish_table(*p, S, min_cluster_reads, t);
	});
} LSQ_API_CATCH
