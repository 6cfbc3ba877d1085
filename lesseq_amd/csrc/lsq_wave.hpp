// What the kernels that stride over parsed reads share (lsq_junc.hip, lsq_cov.hip, lsq_exonbins.hip, lsq_psi.hip, lsq_evidence.hip, lsq_sites.hip): 64-bit
// reductions over a wave, the tail that combines a workgroup's four tally words, the counters a workgroup keeps in LDS for the ids
// it meets with the wave's combining add into them (the exon-bin, the psi, the evidence and the sites count), and the grid of such a kernel.
#pragma once

#include "lsq_device.hpp"
#include "lsq_route.hpp"       // (the library word of a stranded kernel and what it says of a strand id)

constexpr unsigned NO_ID = 0xFFFFFFFFu;        // a lane that holds no id; a free slot of WgCounters

__device__ inline unsigned long long wave_sum(unsigned long long v) {
	for (unsigned d = 32; d; d >>= 1) v += __shfl_xor(v, d);
	return v;
}
__device__ inline unsigned long long wave_or(unsigned long long v) {
	for (unsigned d = 32; d; d >>= 1) v |= __shfl_xor(v, d);
	return v;
}

// The tail of a kernel of 256 lanes whose lanes each hold four tally words: the words combined (OR: ored, else summed) over the
// wave, a wave's results in `part` (the kernel's own LDS), one barrier, the four waves' combined in v on thread 0 -- every other
// lane's v holds its wave's.  What follows the barrier in the kernel (the atomics of thread 0, a flush of other LDS) is the kernel's.
template <bool OR>
__device__ inline void workgroup_tally(unsigned long long (&v)[4], unsigned long long (*part)[4]) {
	const unsigned wave = threadIdx.x >> 6;
#pragma unroll
	for (unsigned q = 0; q < 4; ++q) v[q] = OR ? wave_or(v[q]) : wave_sum(v[q]);
	if ((threadIdx.x & 63u) == 0) {
#pragma unroll
		for (unsigned q = 0; q < 4; ++q) part[wave][q] = v[q];
	}
	__syncthreads();
	if (threadIdx.x == 0) {
#pragma unroll
		for (unsigned q = 0; q < 4; ++q) {
			v[q] = 0;
#pragma unroll
			for (unsigned w = 0; w < 4; ++w) v[q] = OR ? (v[q] | part[w][q]) : (v[q] + part[w][q]);
		}
	}
}

// A workgroup's own counters in LDS, for the ids it meets first: SLOTS keys (NO_ID: free) and 64-bit counts.  A key is set once
// and never changes.  An id whose slot another id holds goes to the global counter at once; the slots are added to the global
// counters when the workgroup has done all its reads.  With every hit a global atomic, a shuffled 100 M-read library -- whose
// largest gene takes 12 M exon-bin hits -- spent 65 of that count's 77 ms on them: a wave's lanes mostly differ there, and the
// atomics of all waves on a hot id queue at one address.  A hot id is met early, so it finds a slot: one global atomic a workgroup.
template <unsigned SLOTS>
struct WgCounters {
	unsigned key[SLOTS];
	unsigned long long cnt[SLOTS];
	__device__ void clear() {
		for (unsigned i = threadIdx.x; i < SLOTS; i += 256u) { key[i] = NO_ID; cnt[i] = 0ull; }
	}
	__device__ void add(unsigned long long *counter, unsigned id, unsigned long long n) {
		const unsigned slot = (id * 2654435761u) >> 16 & (SLOTS - 1u);
		const unsigned was = atomicCAS(&key[slot], NO_ID, id);
		if (was == NO_ID || was == id) atomicAdd(&cnt[slot], n);
		else atomicAdd(&counter[id], n);
	}
	__device__ void flush(unsigned long long *counter) const {
		for (unsigned i = threadIdx.x; i < SLOTS; i += 256u) if (key[i] != NO_ID && cnt[i]) atomicAdd(&counter[key[i]], cnt[i]);
	}
};

// Every lane of the wave arrives (the callers' loops are uniform): the lanes that hold an id, equal ids found by a ballot on the
// first such lane's id; that lane keeps their number.  When every id has its lane, those lanes add, all in one instruction.  In
// a coordinate-sorted file the 64 reads of a wave mostly hold one id: one round and one add where there were 64 on one address.
template <unsigned SLOTS>
__device__ inline void wave_add_ids(WgCounters<SLOTS> &local, unsigned long long *counter, unsigned id, unsigned lane) {
	unsigned long long todo = __ballot(id != NO_ID);
	unsigned mine = 0;
	while (todo) {
		const unsigned leader = (unsigned)__ffsll((long long)todo) - 1u;
		const unsigned id0 = (unsigned)__shfl((int)id, (int)leader);
		const unsigned long long same = __ballot(id == id0);      // (id0 is not NO_ID: lanes without an id never match)
		if (lane == leader) mine = (unsigned)__popcll(same);
		todo &= ~same;
	}
	if (mine) local.add(counter, id, mine);
}

// ---- the stranded form of a count kernel (exonbins, psi, evidence).  It takes, as a parameter pack that is empty in
// the unstranded form, the word of lsq_route.hpp's route_lib_word and the five counters of the table's library report.
__device__ inline unsigned lib_word() { return 0u; }
__device__ inline unsigned lib_word(unsigned word, unsigned long long *) { return word; }
__device__ inline unsigned long long *lib_counters() { return nullptr; }
__device__ inline unsigned long long *lib_counters(unsigned, unsigned long long *counters) { return counters; }
// The library report: per lane, in registers, what its reads came to -- t plus, t minus, no t, and of the first two those that
// counted for a gene or event -- summed over the workgroup when it has done all its reads: one atomic a workgroup and counter
// that is not zero (DESIGN 4.11 records what an atomic a wave on five addresses costs).
struct LibLane {
	unsigned long long plus = 0, minus = 0, none = 0, kept_plus = 0, kept_minus = 0;
	__device__ inline void note(const unsigned t, const bool counted) {
		plus += (unsigned)(t == 0u); minus += (unsigned)(t == 1u); none += (unsigned)(t >= ROUTE_NO_STRAND);
		kept_plus += (unsigned)(t == 0u && counted); kept_minus += (unsigned)(t == 1u && counted);
	}
	// (every lane of the workgroup comes here, outside the kernel's loops; the LDS is this call's own: another tally may follow at once)
	__device__ inline void flush(unsigned long long *out) const {
		__shared__ unsigned long long part_a[4][4], part_b[4][4];
		unsigned long long v[4] = {plus, minus, none, kept_plus}, w[4] = {kept_minus, 0ull, 0ull, 0ull};
		workgroup_tally<false>(v, part_a);
		workgroup_tally<false>(w, part_b);
		if (threadIdx.x == 0) {
#pragma unroll
			for (unsigned q = 0; q < 4; ++q) if (v[q]) atomicAdd(&out[q], v[q]);
			if (w[0]) atomicAdd(&out[4], w[0]);
		}
	}
};

// workgroups of a kernel that strides over the reads, a lane a read: eight a compute unit at most (the environment's `env_name`:
// another bound -- tests: the stride on a small file)
inline unsigned stride_grid(const lsq_ctx *c, const char *env_name, unsigned long long n_reads) {
	if (const char *e = getenv(env_name)) { const long long v = atoll(e); if (v >= 1 && v <= 1 << 20) return std::min(grid_for(n_reads, 256), (unsigned)v); }
	return grid_for(c->n_cu, n_reads, 256, 8);
}
