// What the kernels that stride over parsed reads share (lsq_junc.hip, lsq_cov.hip, lsq_exonbins.hip): 64-bit reductions over a
// wave, the tail that combines a workgroup's four tally words, and the grid of such a kernel.
#pragma once

#include "lsq_device.hpp"

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

// workgroups of a kernel that strides over the reads, a lane a read: eight a compute unit at most (the environment's `env_name`:
// another bound -- tests: the stride on a small file)
inline unsigned stride_grid(const lsq_ctx *c, const char *env_name, unsigned long long n_reads) {
	if (const char *e = getenv(env_name)) { const long long v = atoll(e); if (v >= 1 && v <= 1 << 20) return std::min(grid_for(n_reads, 256), (unsigned)v); }
	return grid_for(c->n_cu, n_reads, 256, 8);
}
