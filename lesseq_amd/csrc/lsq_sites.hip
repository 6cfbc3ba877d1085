// Splice-site usage and read-through per junction of a parsed read file on the device (include/lesseq_hip.h,
// lsq_ss_device): four phases -- junctions (lsq_junc.hip's five passes as they are: the distinct junction rows), index (the rows
// united with the annotated introns and the boundary arrays, made on the host by lsq_sites.cpp's ss_plan, uploaded), through (a
// lane a read: every block a binary search in its chromosome's boundaries and a walk over them; equal ids are combined inside the
// wave, then added to the workgroup's own counters in LDS, or to the global ones where the id has no slot there: lsq_wave.hpp),
// copy-back (the boundaries' counters; the rows are put together on the host).  Every number is an integer and sums commute: no
// result depends on the order in which lanes arrive.
#include "lsq_wave.hpp"
#include "lsq_sites.hpp"

namespace {

constexpr unsigned SS_LDS_SLOTS = 2048;           // 24 KiB of the exon-bin count's 36 (WgCounters takes a power of two): four workgroups a compute unit

struct SsBoundaries {
	const unsigned *chrom_first;                  // n_chroms + 1
	const int *pos;                               // ascending per chromosome, inside (-2^30, 2^30)
	unsigned n_chroms;
};

// A lane a read, a fixed number of workgroups striding over the reads.  A lane walks its read's blocks up to the next boundary
// that one of them runs through -- s + m <= p <= e - m: a block shorter than 2m has none, a longer one's first is found by a
// binary search, the following ones lie behind it -- then the whole wave combines what its lanes found (wave_add_ids) and goes on:
// as many rounds as the wave's busiest read has hits.  m <= 2^32-1, so s + m and e - m are taken in 64 bits; for a block that is
// looked up (e - s >= 2m) both lie between s and e.  The LDS counters are added to the global ones behind the barrier.
__global__ void __launch_bounds__(256) lsq_ss_through_kernel(ParsedReads R, SsBoundaries B, long long m, unsigned long long *through) {
	__shared__ WgCounters<SS_LDS_SLOTS> local;
	local.clear();
	__syncthreads();
	const unsigned lane = threadIdx.x & 63u;
	const unsigned long long stride = (unsigned long long)gridDim.x * 256u;
	// (the wave's first read decides whether the wave has any: the loop is uniform, a lane beyond the last read has no block)
	for (unsigned long long base = (unsigned long long)blockIdx.x * 256u + (threadIdx.x & ~63u); base < R.n_reads; base += stride) {
		const unsigned long long r = base + lane;
		const bool have = r < R.n_reads;
		const unsigned long long b1 = have ? R.blk_off[r + 1] : 0ull;
		unsigned long long k = have ? R.blk_off[r] : 0ull;       // the next block to begin
		unsigned i = 0, i_end = 0;                               // the next boundary of the walk, the end of the chromosome's
		int last = 0;                                            // e - m of the block being walked
		for (;;) {
			unsigned hit = NO_ID;
			while (hit == NO_ID) {
				if (i < i_end && B.pos[i] <= last) hit = i++;
				else if (k < b1) {                                // the next block
					const int s = R.bs[k], e = R.be[k];
					const unsigned ch = R.bc[k];
					++k;
					i = i_end = 0;
					if (ch == NO_CHROM || ch >= B.n_chroms || (long long)e - s < 2 * m) continue;
					const int first = (int)(s + m);
					last = (int)(e - m);
					unsigned lo = B.chrom_first[ch], hi = B.chrom_first[ch + 1u];
					i_end = hi;
					while (lo < hi) {                             // the first boundary at or behind s + m
						const unsigned mid = lo + ((hi - lo) >> 1);
						if (B.pos[mid] < first) lo = mid + 1u; else hi = mid;
					}
					i = lo;
				} else break;                                     // the read is done
			}
			if (!__any(hit != NO_ID)) break;
			wave_add_ids(local, through, hit, lane);
		}
	}
	__syncthreads();
	local.flush(through);
}

} // namespace

int lsq::ss_device_reads(lsq_ctx *c, const lsq_ss_index &ix, const ParsedReads &R, uint32_t min_overhang, lsq_ss_table &t) {
	hipStream_t st = c->stream;
	int rc;
	PhaseClock<3> PC;                             // index, through, copy-back
	if ((rc = PC.make())) return rc;

	// ---- junctions
	lsq_jn_table jt;
	if ((rc = jn_device_reads(c, *ix.J, R, min_overhang, jt))) return rc;

	// ---- index: the rows and the boundaries, on the host; the boundaries uploaded
	HIP_TRY(PC.mark(0, st));
	SsPlan P;
	if ((rc = ss_plan(ix, jt, P))) return rc;
	const size_t nb = P.pos.size(), nc = ix.E.covered.size();
	std::vector<uint64_t> through(nb, 0);
	DevBuf<unsigned> d_first;
	DevBuf<int> d_pos;
	DevBuf<unsigned long long> d_through;
	if ((rc = d_first.upload(P.chrom_first_boundary.data(), nc + 1, st)) || (rc = d_pos.upload(P.pos.data(), nb, st)) || (rc = d_through.alloc(nb))) return rc;
	if (nb) HIP_TRY(hipMemsetAsync(d_through.p, 0, nb * 8, st));

	// ---- through
	HIP_TRY(PC.mark(1, st));
	if (R.n_reads && nb) {
		const SsBoundaries B{d_first.p, d_pos.p, (unsigned)nc};
		hipLaunchKernelGGL(lsq_ss_through_kernel, dim3(stride_grid(c, "LSQ_SS_GRID", R.n_reads)), dim3(256), 0, st, R, B, (long long)ss_through_overhang(min_overhang), d_through.p);
		HIP_TRY(hipGetLastError());
	}

	// ---- copy-back
	HIP_TRY(PC.mark(2, st));
	if (nb) HIP_TRY(hipMemcpyAsync(through.data(), d_through.p, nb * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(PC.mark(3, st));
	HIP_TRY(hipStreamSynchronize(st));
	ss_finish_table(ix, P, through, jt, t);
	t.ms[0] = 0;
	for (float v : jt.ms) t.ms[0] += v;
	for (int k = 0; k < 3; ++k) (void)PC.ms(k, &t.ms[k + 1]);
	return LSQ_OK;
}

// the boundary ids a workgroup of the through count keeps in LDS (tests place their cases around it)
extern "C" int lsq_ss_lds_slots(void) { return (int)SS_LDS_SLOTS; }
