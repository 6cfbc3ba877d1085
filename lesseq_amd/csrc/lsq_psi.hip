// The junction reads per event form of a parsed read file on the device (include/lesseq_hip.h, lsq_ps_device): three
// phases over device arrays -- index upload, count (a lane a read: every pair of neighbouring blocks the junction rule and a binary
// search among its chromosome's informative introns, then a walk over the intron's forms; a read counts once a form and once an
// event by predicates over its earlier pairs alone, no per-lane list; equal ids are combined inside the wave, then added to the
// workgroup's own counters in LDS, or to the global ones where the id has no slot there: lsq_wave.hpp), copy-back (the counters).
// Every number is an integer and sums commute: no result depends on the order in which lanes arrive.  The pair rule, the intron
// search and the once-per-form predicates are lsq_psi_dev.hpp's, which the evidence count (lsq_evidence.hip) shares.
#include "lsq_psi_count.hpp"


int lsq::ps_device_reads(lsq_ctx *c, const lsq_ps_index &ix, const ParsedReads &R, uint32_t min_overhang, lsq_ps_table &t) {
	hipStream_t st = c->stream;
	int rc;
	PhaseClock<PS_PHASES> PC;
	if ((rc = PC.make())) return rc;
	ps_start_table(ix, t);
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks;
	const size_t nf = ix.form_name.size(), ne = ix.event_name.size();

	// ---- index upload
	HIP_TRY(PC.mark(0, st));
	PsDeviceIndex d_ix;
	DevBuf<unsigned long long> d_reads, d_total;
	DevBuf<PsAcc> d_acc;
	DevBuf<unsigned long long> d_lib;                // a stranded index: the library report
	const bool stranded = ix.E.stranded();
	const PsAcc acc0{0, 0, 0, 0, 0, 0};
	PsAcc acc = acc0;
	if ((rc = d_ix.upload(ix, st)) || (rc = d_reads.alloc(nf)) || (rc = d_total.alloc(ne)) || (rc = d_acc.upload(&acc0, 1, st))) return rc;
	if (nf) HIP_TRY(hipMemsetAsync(d_reads.p, 0, nf * 8, st));
	if (ne) HIP_TRY(hipMemsetAsync(d_total.p, 0, ne * 8, st));
	if (stranded) {
		if ((rc = d_lib.alloc(LIB_REPORT))) return rc;
		HIP_TRY(hipMemsetAsync(d_lib.p, 0, LIB_REPORT * 8, st));
	}

	// ---- count
	HIP_TRY(PC.mark(1, st));
	if (R.n_reads) {
		const PsIndex I = d_ix.view(ix);
		const dim3 grid(stride_grid(c, "LSQ_PS_GRID", R.n_reads));
		if (stranded) ps_launch_stranded(grid.x, st, R, I, (unsigned)min_overhang, d_reads.p, d_total.p, d_acc.p,
		                                 route_lib_word(ix.E.library == LSQ_LIBRARY_REVERSE, (unsigned)ix.E.strand_plus, (unsigned)ix.E.strand_minus), d_lib.p);
		else hipLaunchKernelGGL(lsq_ps_count_kernel<false>, grid, dim3(256), 0, st, R, I, (unsigned)min_overhang, d_reads.p, d_total.p, d_acc.p);
		HIP_TRY(hipGetLastError());
	}

	// ---- copy-back
	HIP_TRY(PC.mark(2, st));
	if (nf) HIP_TRY(hipMemcpyAsync(t.reads.data(), d_reads.p, nf * 8, hipMemcpyDeviceToHost, st));
	if (ne) HIP_TRY(hipMemcpyAsync(t.total.data(), d_total.p, ne * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&acc, d_acc.p, sizeof(acc), hipMemcpyDeviceToHost, st));
	if (stranded) HIP_TRY(hipMemcpyAsync(t.lib, d_lib.p, LIB_REPORT * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(PC.mark(3, st));
	HIP_TRY(hipStreamSynchronize(st));
	t.report[2] = acc.occurrences; t.report[3] = acc.dropped; t.report[4] = acc.nochrom; t.report[5] = acc.found; t.report[6] = acc.counted; t.report[7] = acc.multi_event;
	for (int k = 0; k < PS_PHASES; ++k) (void)PC.ms(k, &t.ms[k]);
	return LSQ_OK;
}
