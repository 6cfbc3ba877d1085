// The two device primitives alone (developer entries, include/lesseq_hip_dev.h): the prefix sum of lsq_scan.hpp and the radix sort
// of lsq_sort.hpp, each run on the caller's numbers and copied back, so that a test can hold them against a reference written from
// their definitions (tests/test_prims_direct_gpu.py).  The two headers live in an anonymous namespace: this unit compiles one more
// copy of the kernels every scanning and sorting unit has, from the same source and flags.  No kernel of its own.
#include "lsq_device.hpp"
#include "lsq_scan.hpp"
#include "lsq_sort.hpp"
#include "../../include/lesseq_hip_dev.h"

namespace {

template <unsigned PAD, bool FLAG, class T>
int scan_alone(lsq_ctx *c, const void *in, uint64_t n, uint64_t *out) {
	hipStream_t st = c->stream;
	DevBuf<T> d_in;
	DevBuf<unsigned long long> d_out;
	ScanScratch S;
	int rc;
	if ((rc = d_in.upload((const T *)in, (size_t)n, st)) || (rc = d_out.alloc((size_t)n + 1)) || (rc = S.reserve(n))) return rc;
	if ((rc = device_scan<PAD, FLAG, T>(S, (const T *)d_in.p, n, d_out.p, st))) return rc;
	HIP_TRY(hipMemcpyAsync(out, d_out.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return LSQ_OK;
}

} // namespace

extern "C" {

int lsq_debug_scan(lsq_ctx *c, int form, const void *in, uint64_t n, uint64_t *out) LSQ_API_TRY {
	if (!c || (!in && n) || !out) return fail(LSQ_E_ARG, "null argument");
	if (form < 0 || form > 4) return fail(LSQ_E_ARG, "scan form %d: 0 .. 4 are the forms the library uses", form);
	HIP_TRY(hipSetDevice(c->device));
	switch (form) {
	case 0: return scan_alone<1, false, unsigned>(c, in, n, out);
	case 1: return scan_alone<1, true, unsigned>(c, in, n, out);
	case 2: return scan_alone<1, false, unsigned long long>(c, in, n, out);
	case 3: return scan_alone<P2_GROUP_PAD, false, unsigned>(c, in, n, out);
	default: return scan_alone<P1_GROUP_PAD, false, unsigned>(c, in, n, out);
	}
} LSQ_API_CATCH

int lsq_debug_sort(lsq_ctx *c, uint64_t *w0, uint64_t *w1, uint64_t n, const unsigned *bits, unsigned n_bits, int drop_constant_digits,
                   unsigned *n_passes) LSQ_API_TRY {
	if (!c || (n && (!w0 || !w1)) || (n_bits && !bits) || !n_passes) return fail(LSQ_E_ARG, "null argument");
	if (n_bits > 16) return fail(LSQ_E_ARG, "%u digits: at most 16 (the 128 bits of a record)", n_bits);
	for (unsigned q = 0; q < n_bits; ++q)
		if (bits[q] > 120) return fail(LSQ_E_ARG, "digit %u at bit %u: a digit begins at bit 120 at the latest", q, bits[q]);
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	unsigned digits[16];
	unsigned n_digits = n_bits;
	for (unsigned q = 0; q < n_bits; ++q) digits[q] = bits[q];
	if (drop_constant_digits) {       // as lsq_junc.hip and lsq_cov.hip choose theirs: the OR and the AND of every record's words (there on the device)
		unsigned long long any[2] = {0, 0}, all[2] = {n ? ~0ull : 0ull, n ? ~0ull : 0ull};
		for (uint64_t i = 0; i < n; ++i) { any[0] |= w0[i]; any[1] |= w1[i]; all[0] &= w0[i]; all[1] &= w1[i]; }
		n_digits = sort_digits(any, all, bits, n_bits, digits);
	}
	SortBuf B;
	int rc;
	if ((rc = B.reserve(n))) return rc;
	if (n) {
		HIP_TRY(hipMemcpyAsync(B.w0[0].p, w0, (size_t)n * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(B.w1[0].p, w1, (size_t)n * 8, hipMemcpyHostToDevice, st));
	}
	if ((rc = device_radix_sort(B, digits, n_digits, st))) return rc;
	if (n) {
		HIP_TRY(hipMemcpyAsync(w0, B.w0[B.cur].p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(w1, B.w1[B.cur].p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(hipStreamSynchronize(st));
	*n_passes = n < 2 ? 0u : n_digits;        // (fewer than two records: device_radix_sort makes no pass)
	return LSQ_OK;
} LSQ_API_CATCH

} // extern "C"
