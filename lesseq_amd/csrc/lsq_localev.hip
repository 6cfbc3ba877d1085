// Local events (step 2 of the pipeline, bin/Events.r) on the device.  The rules each lane evaluates are the script's,
// with its 1-based column i and coordinates pos[1..2N]; the host side is lsq_localev.cpp.
//
//   lsq_le_kernel<false>   one wave per gene (grid-stride): lanes take columns i in chunks of 64, usage = popcounts of a
//                          column's W = ceil(K/64) words, the MXE / AFE / ALE complement test (a ^ b) == the K-bit mask
//                          word by word; per-gene hits of the eight types into a type-major [8][G] array
//   device_scan            one exclusive scan over the [8][G] hits (lsq_scan.hpp): each gene's first slot per type
//   lsq_le_kernel<true>    the same predicates; a lane's rank within its gene = running offset of the earlier chunks +
//                          mbcnt over the chunk's ballot, so records land in the script's order
#include "lsq_device.hpp"
#include "lsq_scan.hpp"
#include "lsq_localev.hpp"

using namespace lsq;

namespace {

struct LeGene {
	unsigned long long pos_off, bit_off;
	int N, K, W, strand;
};
static_assert(sizeof(LeGene) == 32, "LeGene layout");

constexpr int LE_LOOP_TYPES = 5;          // ES RI A5SS A3SS MXE: one per column; AFE ALE T3: one per gene at most

// lsq::le_record on the device
__device__ inline unsigned long long dev_record(unsigned gene, unsigned code) { return (unsigned long long)code << 32 | gene; }

struct GeneView {
	const int *pos;                        // this gene's pos[1..2N] at pos[0..2N)
	const unsigned long long *bits;
	int N, K, W, strand;
	__device__ long long P(int j) const { return (long long)pos[j - 1]; }
	// usage[c] (1-based column): isoforms that hold the column
	__device__ int usage(int c) const {
		const unsigned long long *b = bits + (size_t)(c - 1) * W;
		int u = 0;
		for (int w = 0; w < W; ++w) u += __popcll(b[w]);
		return u;
	}
	// sum(matrix[, a] == matrix[, b]) == 0: the two columns differ in every row
	__device__ bool complement(int a, int b) const {
		const unsigned long long *x = bits + (size_t)(a - 1) * W, *y = bits + (size_t)(b - 1) * W;
		for (int w = 0; w < W; ++w) {
			const int left = K - 64 * w;
			const unsigned long long m = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
			if ((x[w] ^ y[w]) != m) return false;
		}
		return true;
	}
};

template <bool EMIT>
__global__ void __launch_bounds__(256) lsq_le_kernel(const LeGene *genes, unsigned n_genes, const int *pos, const unsigned long long *bits,
                                                     unsigned *hits, const unsigned long long *slot, unsigned long long *rec) {
	const unsigned lane = threadIdx.x & 63u;
	const unsigned waves = gridDim.x * (blockDim.x >> 6);
	for (unsigned g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); g < n_genes; g += waves) {
		const LeGene d = genes[g];
		GeneView v{pos + d.pos_off, bits + d.bit_off, d.N, d.K, d.W, d.strand};
		const int N = d.N, K = d.K;
		const bool plus = d.strand == LE_PLUS, minus = d.strand == LE_MINUS;
		unsigned cnt[LE_LOOP_TYPES] = {0, 0, 0, 0, 0};
		unsigned block_hit[3] = {0, 0, 0};           // AFE ALE T3
		unsigned block_code[3] = {0, 0, 0};
		if (N >= 3) {                                 // Events.r:57
			for (int c0 = 0; c0 < N; c0 += 64) {
				const int i = c0 + (int)lane + 1;
				bool h[LE_LOOP_TYPES] = {false, false, false, false, false};
				// :62-93, i in 2..N-1
				if (i >= 2 && i <= N - 1 && v.usage(i - 1) == K && v.usage(i + 1) == K && K > v.usage(i)) {
					const long long gl = v.P(2 * i - 1) - v.P(2 * i - 2), gr = v.P(2 * i + 1) - v.P(2 * i);
					h[LE_ES] = gl > 0 && gr > 0;
					h[LE_RI] = gl == 0 && gr == 0;
					h[LE_A5SS] = (plus && gl == 0 && gr > 0) || (minus && gl > 0 && gr == 0);
					h[LE_A3SS] = (plus && gl > 0 && gr == 0) || (minus && gl == 0 && gr > 0);
				}
				// :95-107, i in 4..N
				if (i >= 4 && i <= N && v.usage(i - 3) == K && v.usage(i) == K && v.complement(i - 2, i - 1) &&
				    v.P(2 * i - 1) - v.P(2 * i - 2) > 0 && v.P(2 * i - 3) - v.P(2 * i - 4) > 0 && v.P(2 * i - 5) - v.P(2 * i - 6) > 0)
					h[LE_MXE] = true;
#pragma unroll
				for (int t = 0; t < LE_LOOP_TYPES; ++t) {
					const unsigned long long m = __ballot(h[t]);
					if (EMIT && h[t]) {
						const unsigned r = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
						rec[slot[(size_t)t * n_genes + g] + cnt[t] + r] = dev_record(g, (unsigned)i);
					}
					cnt[t] += (unsigned)__popcll(m);
				}
			}
			const int k = 2 * N;
			// :109-124, first-exon block: AFE on +, ALE on -
			if (v.usage(3) == K && v.complement(1, 2) && v.P(3) - v.P(2) > 0 && v.P(5) - v.P(4) > 0) {
				if (plus) { block_hit[0] = 1; block_code[0] = 0; }
				if (minus) { block_hit[1] = 1; block_code[1] = 0; }
			}
			// :126-141, last-exon block: ALE on +, AFE on -
			if (v.usage(N - 2) == K && v.complement(N - 1, N) && v.P(k - 1) - v.P(k - 2) > 0 && v.P(k - 3) - v.P(k - 4) > 0) {
				if (plus) { block_hit[1] = 1; block_code[1] = 1; }
				if (minus) { block_hit[0] = 1; block_code[0] = 1; }
			}
			// :143-156
			if (plus && v.usage(N - 1) == K && K > v.usage(N) && v.P(k - 1) - v.P(k - 2) == 0) { block_hit[2] = 1; block_code[2] = 0; }
			if (minus && v.usage(2) == K && K > v.usage(1) && v.P(3) - v.P(2) == 0) { block_hit[2] = 1; block_code[2] = 1; }
		}
		if (lane != 0) continue;
		if (!EMIT) {
			for (int t = 0; t < LE_LOOP_TYPES; ++t) hits[(size_t)t * n_genes + g] = cnt[t];
			for (int b = 0; b < 3; ++b) hits[(size_t)(LE_AFE + b) * n_genes + g] = block_hit[b];
		} else {
			for (int b = 0; b < 3; ++b)
				if (block_hit[b]) rec[slot[(size_t)(LE_AFE + b) * n_genes + g]] = dev_record(g, block_code[b]);
		}
	}
}

// base[t] = slot[t * G] for t = 0..8 (base[8]: the total)
__global__ void lsq_le_bases_kernel(const unsigned long long *slot, unsigned n_genes, unsigned long long *base) {
	const unsigned t = threadIdx.x;
	if (t <= (unsigned)LE_TYPES) base[t] = slot[(size_t)t * n_genes];
}

} // namespace

extern "C" {

int lsq_le_detect(lsq_ctx *c, const lsq_le_graphs *g, lsq_le_result **out) LSQ_API_TRY {
	if (!c || !g || !out) return fail(LSQ_E_ARG, "null argument");
	*out = nullptr;
	std::unique_ptr<lsq_le_result> r(new lsq_le_result);
	r->g = g;
	const size_t G = g->size();
	if (G == 0) { *out = r.release(); return LSQ_OK; }
	if (G * LE_TYPES >= 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^29 genes");
	std::vector<LeGene> desc(G);
	for (size_t i = 0; i < G; ++i) {
		desc[i].pos_off = g->pos_off[i];
		desc[i].bit_off = g->bit_off[i];
		desc[i].N = g->N[i];
		desc[i].K = g->K[i];
		desc[i].W = (g->K[i] + 63) / 64;
		desc[i].strand = g->strand_code[i];
		// the kernel reads pos[1..2N] and N * W words of a gene of 3 or more columns
		if (g->N[i] >= 3 && (g->pos_off[i + 1] - g->pos_off[i] != 2ull * (uint64_t)g->N[i] ||
		                     g->bit_off[i + 1] - g->bit_off[i] != (uint64_t)g->N[i] * (uint64_t)desc[i].W || g->K[i] < 1))
			return fail(LSQ_E_INTERNAL, "gene %zu: packing does not match its shape", i);
	}
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	const unsigned n = (unsigned)G, n_hits = n * (unsigned)LE_TYPES;
	DevBuf<LeGene> d_genes;
	DevBuf<int> d_pos;
	DevBuf<unsigned long long> d_bits, d_slot, d_base, d_rec;
	DevBuf<unsigned> d_hits;
	ScanScratch S;
	PhaseClock<4> PC;
	int rc;
	if ((rc = PC.make())) return rc;
	HIP_TRY(PC.mark(0, st));
	if ((rc = d_genes.upload(desc.data(), G, st)) || (rc = d_pos.upload(g->pos.data(), g->pos.size(), st)) ||
	    (rc = d_bits.upload((const unsigned long long *)g->bits.data(), g->bits.size(), st)) || (rc = d_hits.alloc(n_hits)) ||
	    (rc = d_slot.alloc((size_t)n_hits + 1)) || (rc = d_base.alloc(LE_TYPES + 1)) || (rc = S.reserve(n_hits))) return rc;
	HIP_TRY(PC.mark(1, st));
	const unsigned blocks = grid_for(c->n_cu, G, 4, 8);
	hipLaunchKernelGGL((lsq_le_kernel<false>), dim3(blocks), dim3(256), 0, st, (const LeGene *)d_genes.p, n, (const int *)d_pos.p,
	                   (const unsigned long long *)d_bits.p, d_hits.p, (const unsigned long long *)nullptr, (unsigned long long *)nullptr);
	if ((rc = device_scan<1, false>(S, d_hits.p, n_hits, d_slot.p, st))) return rc;
	hipLaunchKernelGGL(lsq_le_bases_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long *)d_slot.p, n, d_base.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(PC.mark(2, st));
	unsigned long long base[LE_TYPES + 1];
	HIP_TRY(hipMemcpyAsync(base, d_base.p, sizeof base, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	const unsigned long long total = base[LE_TYPES];
	if (total) {
		if ((rc = d_rec.alloc((size_t)total))) return rc;
		hipLaunchKernelGGL((lsq_le_kernel<true>), dim3(blocks), dim3(256), 0, st, (const LeGene *)d_genes.p, n, (const int *)d_pos.p,
		                   (const unsigned long long *)d_bits.p, (unsigned *)nullptr, (const unsigned long long *)d_slot.p, d_rec.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(PC.mark(3, st));
		std::vector<unsigned long long> all((size_t)total);
		HIP_TRY(hipMemcpyAsync(all.data(), d_rec.p, (size_t)total * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
		HIP_TRY(PC.mark(4, st));
		HIP_TRY(hipStreamSynchronize(st));
		float t[4];
		for (int q = 0; q < 4; ++q) HIP_TRY(PC.ms(q, &t[q]));
		for (int q = 0; q < 4; ++q) r->ms[q] = t[q];
		for (int t = 0; t < LE_TYPES; ++t) r->rec[t].assign(all.begin() + (ptrdiff_t)base[t], all.begin() + (ptrdiff_t)base[t + 1]);
	}
	*out = r.release();
	return LSQ_OK;
} LSQ_API_CATCH

} // extern "C"
