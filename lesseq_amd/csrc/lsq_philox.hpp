// The random numbers of the read bootstrap (lsq_bootstrap): one source for the host (lsq_boot.cpp) and the
// device (lsq_boot.hip), as lsq_inflate.hpp is for BGZF.  Integer arithmetic throughout: what a replicate draws depends on
// (seed, read file, event, replicate, draw index) alone, never on how the draws are spread over lanes, tiles, chunks or devices.
//
//   Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten
//   rounds, the key bumped before rounds 2 to 10.
//   key = (seed low word, seed high word); counter = (j low word, j high word, e, (m << 24) | b) with j = i >> 1 for draw i
//   of replicate b (< 2^24) of read file m and event e (its index in the output order of the compiled events).
//   The block's words x0..x3: even i takes u = x0 | x1 << 32, odd i takes u = x2 | x3 << 32.
//   r = (u * n) >> 64 (n: reads of the pair (m, e)); the class drawn is the smallest c whose inclusive cumulative count exceeds r.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LSQ_HD __host__ __device__
#else
#define LSQ_HD
#endif

namespace lsq {

struct PhiloxBlock { uint32_t x[4]; };

LSQ_HD inline PhiloxBlock philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
	for (int round = 0; round < 10; ++round) {
		if (round) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
		const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
		c0 = n0; c1 = n1; c2 = n2; c3 = n3;
	}
	PhiloxBlock b;
	b.x[0] = c0; b.x[1] = c1; b.x[2] = c2; b.x[3] = c3;
	return b;
}

// the block that holds the draws 2 j and 2 j + 1 of (seed, read file m, event e, replicate b)
LSQ_HD inline PhiloxBlock boot_block(uint64_t seed, uint32_t m, uint32_t e, uint32_t b, uint64_t j) {
	return philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), e, (m << 24) | b, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// ... and the 64 random bits of draw i out of it
LSQ_HD inline uint64_t boot_bits(const PhiloxBlock &B, uint64_t i) {
	return (i & 1u) ? ((uint64_t)B.x[2] | (uint64_t)B.x[3] << 32) : ((uint64_t)B.x[0] | (uint64_t)B.x[1] << 32);
}

// (u * n) >> 64: uniform on 0 .. n - 1 up to 2^-64 n
LSQ_HD inline uint64_t mul_hi_u64(uint64_t u, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
	return __umul64hi(u, n);
#else
	return (uint64_t)(((unsigned __int128)u * n) >> 64);
#endif
}

// the smallest c (0-based, < n_cls) with cum[c] > r, cum the inclusive cumulative counts and r < cum[n_cls - 1]: classes
// without reads repeat the value before them and are never the smallest
template <class CumT>
LSQ_HD inline uint32_t boot_class_of(const CumT *cum, uint32_t n_cls, uint64_t r) {
	uint32_t lo = 0, hi = n_cls - 1u;              // the answer lies in [lo, hi]
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if ((uint64_t)cum[mid] > r) hi = mid; else lo = mid + 1u;
	}
	return lo;
}

} // namespace lsq
