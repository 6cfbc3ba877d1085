// The read bootstrap on the host (lsq_boot.hip is the device half): the resampling of lsq_philox.hpp run on the CPU, for
// callers without a GPU and for the tests that hold the device's replicate counts against it.  No device call here.
#include <cstring>

#include "lsq_internal.hpp"
#include "lsq_philox.hpp"
#include "../../include/lesseq_hip_dev.h"

using namespace lsq;

extern "C" {

int lsq_bootstrap_resample_host(int n_methods, uint64_t n_events, const uint64_t *class_off, const uint64_t *class_count, uint64_t seed, uint32_t b,
                                uint64_t *out) LSQ_API_TRY {
	if (n_methods < 0 || n_methods > LSQ_MAX_METHODS) return fail(LSQ_E_ARG, "lsq_bootstrap_resample_host: %d read files (at most %d)", n_methods, LSQ_MAX_METHODS);
	if (!class_off || (n_methods && n_events && (!class_count || !out))) return fail(LSQ_E_ARG, "null argument");
	if (b >= (1u << 24)) return fail(LSQ_E_ARG, "lsq_bootstrap_resample_host: replicate %u (below 2^24)", b);
	if (n_events >= (1ull << 32)) return fail(LSQ_E_ARG, "lsq_bootstrap_resample_host: more than 2^32 events");
	const uint64_t n_out = class_off[n_events];
	for (uint64_t e = 0; e < n_events; ++e)
		if (class_off[e + 1] < class_off[e] || class_off[e + 1] - class_off[e] > 0xFFFFFFFFull) return fail(LSQ_E_ARG, "lsq_bootstrap_resample_host: class offsets of event %llu", (unsigned long long)e);
	std::vector<uint64_t> cum;
	for (int m = 0; m < n_methods; ++m)
		for (uint64_t e = 0; e < n_events; ++e) {
			const uint64_t *cnt = class_count + (size_t)m * n_out + class_off[e];
			uint64_t *o = out + (size_t)m * n_out + class_off[e];
			const uint32_t nc = (uint32_t)(class_off[e + 1] - class_off[e]);
			cum.resize(nc);
			uint64_t n = 0;
			for (uint32_t k = 0; k < nc; ++k) { n += cnt[k]; cum[k] = n; o[k] = 0; }
			for (uint64_t j = 0; 2 * j < n; ++j) {
				const PhiloxBlock B = boot_block(seed, (uint32_t)m, (uint32_t)e, b, j);
				for (uint64_t i = 2 * j; i < 2 * j + 2 && i < n; ++i) ++o[boot_class_of(cum.data(), nc, mul_hi_u64(boot_bits(B, i), n))];
			}
		}
	return LSQ_OK;
} LSQ_API_CATCH

int lsq_debug_bootstrap_draws(uint32_t n_cls, const uint64_t *class_count, uint64_t seed, uint32_t m, uint32_t e, uint32_t b, uint64_t first_draw,
                              uint64_t n_draws, uint32_t *cls) LSQ_API_TRY {
	if (!n_cls || !class_count || (n_draws && !cls)) return fail(LSQ_E_ARG, "null argument");
	if (b >= (1u << 24) || m >= 256u) return fail(LSQ_E_ARG, "lsq_debug_bootstrap_draws: replicate %u (below 2^24), read file %u (below 256)", b, m);
	std::vector<uint64_t> cum(n_cls);
	uint64_t n = 0;
	for (uint32_t k = 0; k < n_cls; ++k) { n += class_count[k]; cum[k] = n; }
	if (first_draw > n || n_draws > n - first_draw) return fail(LSQ_E_RANGE, "lsq_debug_bootstrap_draws: draws %llu .. +%llu of %llu", (unsigned long long)first_draw, (unsigned long long)n_draws, (unsigned long long)n);
	for (uint64_t i = first_draw; i < first_draw + n_draws; ++i) {
		const PhiloxBlock B = boot_block(seed, m, e, b, i >> 1);
		cls[i - first_draw] = 1u + boot_class_of(cum.data(), n_cls, mul_hi_u64(boot_bits(B, i), n));
	}
	return LSQ_OK;
} LSQ_API_CATCH

} // extern "C"
