// The junction and exon-body reads per event form of a parsed read file on the device (include/lesseq_hip.h,
// lsq_fe_device): three phases over device arrays -- index upload, count (a lane a read: first its block pairs against the
// informative introns, exactly as the psi count walks them (lsq_psi_dev.hpp); then its blocks against the informative body -- a
// binary search in the chromosome's cells, a walk over them, the overlap test on every region; a read counts once a form and once an
// event by predicates over its pairs and its earlier (block, region) couples alone, no per-lane list; equal ids are combined inside
// the wave, then added to the workgroup's own counters in LDS, or to the global ones where the id has no slot there: lsq_wave.hpp),
// copy-back (the counters).  Every number is an integer and sums commute: no result depends on the order in which lanes arrive.
#include "lsq_evidence_count.hpp"


int lsq::fe_device_reads(lsq_ctx *c, const lsq_fe_index &ix, const ParsedReads &R, uint32_t min_overhang, uint32_t min_body, lsq_fe_table &t) {
	hipStream_t st = c->stream;
	int rc;
	PhaseClock<FE_PHASES> PC;
	if ((rc = PC.make())) return rc;
	fe_start_table(ix, min_overhang, min_body, t);
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks;
	const lsq_ps_index &P = *ix.P;
	const FeGeometry &G = *ix.G;
	const size_t nf = P.form_name.size(), ne = P.event_name.size(), n_tab = ix.E.covered.size(), nr = ix.region_form.size(), n_cells = ix.cell_start.size();

	// ---- index upload
	HIP_TRY(PC.mark(0, st));
	PsDeviceIndex d_ps;
	DevBuf<int> d_rs, d_re, d_cs, d_ce;
	DevBuf<unsigned> d_rf, d_fr, d_fc, d_cf, d_co, d_cr;
	DevBuf<unsigned long long> d_reads, d_total;
	DevBuf<FeAcc> d_acc;
	DevBuf<unsigned long long> d_lib;                // a stranded index: the library report
	const bool stranded = ix.E.stranded();
	const FeAcc acc0{0, 0, 0, 0, 0, 0, 0, 0, 0};
	FeAcc acc = acc0;
	if ((rc = d_ps.upload(P, st)) || (rc = d_rs.upload(G.region_start.data(), nr, st)) || (rc = d_re.upload(G.region_end.data(), nr, st)) ||
	    (rc = d_rf.upload(ix.region_form.data(), nr, st)) || (rc = d_fr.upload(G.form_first_region.data(), nf + 1, st)) || (rc = d_fc.upload(ix.form_chrom.data(), nf, st)) ||
	    (rc = d_cf.upload(ix.chrom_first_cell.data(), n_tab + 1, st)) || (rc = d_cs.upload(ix.cell_start.data(), n_cells, st)) || (rc = d_ce.upload(ix.cell_end.data(), n_cells, st)) ||
	    (rc = d_co.upload(ix.cell_off.data(), n_cells + 1, st)) || (rc = d_cr.upload(ix.cell_regions.data(), ix.cell_regions.size(), st)) ||
	    (rc = d_reads.alloc(nf)) || (rc = d_total.alloc(ne)) || (rc = d_acc.upload(&acc0, 1, st))) return rc;
	if (nf) HIP_TRY(hipMemsetAsync(d_reads.p, 0, nf * 8, st));
	if (ne) HIP_TRY(hipMemsetAsync(d_total.p, 0, ne * 8, st));
	if (stranded) {
		if ((rc = d_lib.alloc(LIB_REPORT))) return rc;
		HIP_TRY(hipMemsetAsync(d_lib.p, 0, LIB_REPORT * 8, st));
	}

	// ---- count
	HIP_TRY(PC.mark(1, st));
	if (R.n_reads) {
		const FeIndex F{d_rs.p, d_re.p, d_rf.p, d_fr.p, d_fc.p, d_cf.p, d_cs.p, d_ce.p, d_co.p, d_cr.p};
		const dim3 grid(stride_grid(c, "LSQ_FE_GRID", R.n_reads));
		if (stranded) fe_launch_stranded(grid.x, st, R, d_ps.view(P), F, (unsigned)min_overhang, (unsigned)min_body, d_reads.p, d_total.p, d_acc.p,
		                                 route_lib_word(ix.E.library == LSQ_LIBRARY_REVERSE, (unsigned)ix.E.strand_plus, (unsigned)ix.E.strand_minus), d_lib.p);
		else hipLaunchKernelGGL(lsq_fe_count_kernel<false>, grid, dim3(256), 0, st, R, d_ps.view(P), F, (unsigned)min_overhang, (unsigned)min_body, d_reads.p, d_total.p, d_acc.p);
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
	t.report[2] = acc.occurrences; t.report[3] = acc.dropped; t.report[4] = acc.nochrom; t.report[5] = acc.found; t.report[6] = acc.skipped; t.report[7] = acc.body_hits;
	t.report[8] = acc.counted; t.report[9] = acc.multi_event; t.report[10] = acc.body_alone;
	for (int k = 0; k < FE_PHASES; ++k) (void)PC.ms(k, &t.ms[k]);
	return LSQ_OK;
}
