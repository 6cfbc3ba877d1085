// A stable LSD radix sort on the device for data at the scale of a read file (included by the translation units that sort;
// not a public header; needs lsq_device.hpp and lsq_scan.hpp ahead of it).
//
// A record is two 64-bit words (w0, w1), kept as two arrays.  The caller names the 8-bit digits to sort by as bit positions
// in the 128 bits w1:w0 (bit 64 + k = bit k of w1), least significant first; bits that no digit names ride along as payload
// (lsq_junc.hip: 32 bits of w1).  Digits on which every record agrees are skipped by the caller (sort_digits).
//
// One pass = three launches over tiles of SORT_TILE records:
//   histogram   a workgroup counts its tile's digit values in LDS and writes 256 counters, digit-major (hist[d * n_tiles + t]),
//               so that ONE exclusive prefix sum over the table (lsq_scan.hpp) gives every (digit value, tile) its first place;
//   scatter     the tile again: a wave takes a quarter of the tile, in order; its records' ranks among equals come from wave
//               ballots (no atomics: the order of equals is the input's, so the sort is stable and the same from run to run).
// The digit table is 1 KiB a tile against 64 KiB of records.
// tests/test_prims_direct_gpu.py holds the whole permutation against the definition (lsq_prims.hip: lsq_debug_sort).
#pragma once

namespace {

constexpr unsigned SORT_TILE = 4096;           // records per workgroup: 4 waves x 16 rounds x 64 lanes
constexpr unsigned SORT_WAVE_SPAN = SORT_TILE / 4;

struct SortBuf {                               // the two buffers a sort alternates between, and its digit table
	DevBuf<unsigned long long> w0[2], w1[2];
	DevBuf<unsigned> hist;
	DevBuf<unsigned long long> base;
	ScanScratch SS;
	unsigned long long n = 0;
	int cur = 0;                               // which of the two holds the records
	int reserve(unsigned long long count) {
		n = count;
		const unsigned long long nt = (n + SORT_TILE - 1) / SORT_TILE;
		int rc;
		for (int k = 0; k < 2; ++k) if ((rc = w0[k].alloc((size_t)n)) || (rc = w1[k].alloc((size_t)n))) return rc;
		if ((rc = hist.alloc((size_t)(256 * nt))) || (rc = base.alloc((size_t)(256 * nt + 1))) || (rc = SS.reserve(256 * nt))) return rc;
		cur = 0;
		return LSQ_OK;
	}
};

__device__ inline unsigned sort_digit(unsigned long long w0, unsigned long long w1, unsigned bit) {
	return (unsigned)((bit < 64 ? w0 >> bit : w1 >> (bit - 64)) & 0xFFu);
}

__global__ void __launch_bounds__(256) lsq_sort_hist_kernel(const unsigned long long *w0, const unsigned long long *w1, unsigned long long n, unsigned bit,
                                                            unsigned n_tiles, unsigned *hist) {
	__shared__ unsigned cnt[256];
	cnt[threadIdx.x] = 0;
	__syncthreads();
	const unsigned long long *w = bit < 64 ? w0 : w1;
	const unsigned sh = bit & 63u;
	const unsigned long long t0 = (unsigned long long)blockIdx.x * SORT_TILE;
#pragma unroll 4
	for (unsigned q = 0; q < SORT_TILE / 256; ++q) {
		const unsigned long long i = t0 + q * 256u + threadIdx.x;
		if (i < n) atomicAdd(&cnt[(unsigned)(w[i] >> sh) & 0xFFu], 1u);
	}
	__syncthreads();
	hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];
}

__global__ void __launch_bounds__(256) lsq_sort_scatter_kernel(const unsigned long long *w0, const unsigned long long *w1, unsigned long long n, unsigned bit,
                                                               unsigned n_tiles, const unsigned long long *base, unsigned long long *o0, unsigned long long *o1) {
	__shared__ unsigned cnt[4][256];           // per wave: its span's digit counts, then the next free place of every digit value (tile-relative)
	__shared__ unsigned long long first[256];  // the tile's first place per digit value
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	for (unsigned w = 0; w < 4; ++w) cnt[w][threadIdx.x] = 0;
	first[threadIdx.x] = base[(size_t)threadIdx.x * n_tiles + blockIdx.x];
	__syncthreads();
	const unsigned long long s0 = (unsigned long long)blockIdx.x * SORT_TILE + (unsigned long long)wave * SORT_WAVE_SPAN;
	for (unsigned q = 0; q < SORT_WAVE_SPAN / 64; ++q) {
		const unsigned long long i = s0 + q * 64u + lane;
		if (i < n) atomicAdd(&cnt[wave][sort_digit(w0[i], w1[i], bit)], 1u);
	}
	__syncthreads();
	{	// digit value d = threadIdx.x: the waves' counts -> where each wave's records of that value begin, behind the waves before it
		unsigned run = 0;
		for (unsigned w = 0; w < 4; ++w) { const unsigned c = cnt[w][threadIdx.x]; cnt[w][threadIdx.x] = run; run += c; }
	}
	__syncthreads();
	const unsigned long long lt = (1ull << lane) - 1ull;
	for (unsigned q = 0; q < SORT_WAVE_SPAN / 64; ++q) {
		const unsigned long long i = s0 + q * 64u + lane;
		const bool ok = i < n;
		const unsigned long long a = ok ? w0[i] : 0ull, b = ok ? w1[i] : 0ull;
		const unsigned d = sort_digit(a, b, bit);
		// the lanes of this round that hold the same digit value
		unsigned long long same = __ballot(ok);
#pragma unroll
		for (unsigned k = 0; k < 8; ++k) {
			const unsigned long long m = __ballot((d >> k) & 1u);
			same &= ((d >> k) & 1u) ? m : ~m;
		}
		const unsigned rank = (unsigned)__popcll(same & lt);
		const unsigned at = ok ? cnt[wave][d] : 0u;
		__builtin_amdgcn_wave_barrier();       // every lane has read its digit's counter before a group's first lane moves it on
		if (ok && rank == 0) cnt[wave][d] = at + (unsigned)__popcll(same);
		__builtin_amdgcn_wave_barrier();
		if (ok) {
			const unsigned long long p = first[d] + at + rank;       // < n: the places of all records form a permutation of 0 .. n-1
			o0[p] = a; o1[p] = b;
		}
	}
}

// The digits (bit positions, ascending) on which the records differ: `any` / `all` are the OR and the AND of every record's words
static inline unsigned sort_digits(const unsigned long long any[2], const unsigned long long all[2], const unsigned *bits, unsigned n_bits, unsigned *out) {
	unsigned k = 0;
	for (unsigned q = 0; q < n_bits; ++q) {
		const unsigned b = bits[q];
		const unsigned long long diff = (any[b >> 6] ^ all[b >> 6]) >> (b & 63u) & 0xFFull;
		if (diff) out[k++] = b;
	}
	return k;
}

// Sorts B's records by the given digits, least significant first.  Afterwards B.cur names the buffers that hold them.
static int device_radix_sort(SortBuf &B, const unsigned *bits, unsigned n_bits, hipStream_t st) {
	if (B.n < 2) return LSQ_OK;
	const unsigned long long nt = (B.n + SORT_TILE - 1) / SORT_TILE;
	if (nt > 0x7FFFFFFFull) return fail(LSQ_E_RANGE, "sort of more than 2^43 records");
	for (unsigned q = 0; q < n_bits; ++q) {
		const int s = B.cur, d = B.cur ^ 1;
		int rc;
		hipLaunchKernelGGL(lsq_sort_hist_kernel, dim3((unsigned)nt), dim3(256), 0, st, (const unsigned long long *)B.w0[s].p, (const unsigned long long *)B.w1[s].p, B.n, bits[q], (unsigned)nt, B.hist.p);
		HIP_TRY(hipGetLastError());
		if ((rc = device_scan<1, false>(B.SS, B.hist.p, 256 * nt, B.base.p, st))) return rc;
		hipLaunchKernelGGL(lsq_sort_scatter_kernel, dim3((unsigned)nt), dim3(256), 0, st, (const unsigned long long *)B.w0[s].p, (const unsigned long long *)B.w1[s].p, B.n, bits[q], (unsigned)nt,
		                   (const unsigned long long *)B.base.p, B.w0[d].p, B.w1[d].p);
		HIP_TRY(hipGetLastError());
		B.cur = d;
	}
	return LSQ_OK;
}

} // namespace
