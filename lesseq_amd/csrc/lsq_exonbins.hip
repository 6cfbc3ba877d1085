// The reads per exon bin and per gene of a parsed read file on the device (include/lesseq_hip.h, lsq_xb_device): three
// phases over device arrays -- index upload, count (a lane a read: every block a binary search in its chromosome's cells and a
// walk over them; a read counts once a bin and once a gene by predicates alone, no per-lane list; equal ids are combined inside the
// wave, then added to the workgroup's own counters in LDS, or to the global ones where the id has no slot there: lsq_wave.hpp), copy-back (the
// counters).  Every number is an integer and sums commute: no result depends on the order in which lanes arrive.
#include "lsq_exonbins_dev.hpp"


int lsq::xb_device_reads(lsq_ctx *c, const lsq_xb_index &ix, const ParsedReads &R, lsq_xb_table &t) {
	hipStream_t st = c->stream;
	int rc;
	PhaseClock<XB_PHASES> PC;
	if ((rc = PC.make())) return rc;
	xb_start_table(ix, t);
	t.report[0] = R.n_reads; t.report[1] = R.n_blocks;
	// (n_tab: the lookup's tables -- chromosomes, or two a chromosome under a stranded index)
	const size_t nb = ix.bin_gene.size(), ng = ix.gene_name.size(), nc = ix.E.n_table_chroms(), n_tab = ix.E.covered.size(), n_cells = ix.cell_start.size();
	const bool stranded = ix.E.stranded();

	// ---- index upload
	HIP_TRY(PC.mark(0, st));
	DevBuf<int> d_bs, d_be, d_cs, d_ce;
	DevBuf<unsigned> d_bg, d_gf, d_cf, d_co, d_cb;
	DevBuf<unsigned long long> d_reads, d_total;
	DevBuf<XbAcc> d_acc;
	DevBuf<unsigned long long> d_lib;                // a stranded index: the library report
	const XbAcc acc0{0, 0, 0, 0};
	XbAcc acc = acc0;
	if ((rc = d_bs.upload(ix.c_bin_start.data(), nb, st)) || (rc = d_be.upload(ix.c_bin_end.data(), nb, st)) || (rc = d_bg.upload(ix.bin_gene.data(), nb, st)) ||
	    (rc = d_gf.upload(ix.gene_first_bin.data(), ng + 1, st)) || (rc = d_cf.upload(ix.chrom_first_cell.data(), n_tab + 1, st)) ||
	    (rc = d_cs.upload(ix.cell_start.data(), n_cells, st)) || (rc = d_ce.upload(ix.cell_end.data(), n_cells, st)) ||
	    (rc = d_co.upload(ix.cell_off.data(), n_cells + 1, st)) || (rc = d_cb.upload(ix.cell_bins.data(), ix.cell_bins.size(), st)) ||
	    (rc = d_reads.alloc(nb)) || (rc = d_total.alloc(ng)) || (rc = d_acc.upload(&acc0, 1, st))) return rc;
	if (nb) HIP_TRY(hipMemsetAsync(d_reads.p, 0, nb * 8, st));
	if (ng) HIP_TRY(hipMemsetAsync(d_total.p, 0, ng * 8, st));
	if (stranded) {
		if ((rc = d_lib.alloc(LIB_REPORT))) return rc;
		HIP_TRY(hipMemsetAsync(d_lib.p, 0, LIB_REPORT * 8, st));
	}

	// ---- count
	HIP_TRY(PC.mark(1, st));
	if (R.n_reads) {
		const XbIndex I{d_bs.p, d_be.p, d_bg.p, d_gf.p, d_cf.p, d_cs.p, d_ce.p, d_co.p, d_cb.p, (unsigned)nc};
		const dim3 grid(stride_grid(c, "LSQ_XB_GRID", R.n_reads));
		if (stranded) xb_launch_stranded(grid.x, st, R, I, d_reads.p, d_total.p, d_acc.p, route_lib_word(ix.E.library == LSQ_LIBRARY_REVERSE, (unsigned)ix.E.strand_plus, (unsigned)ix.E.strand_minus), d_lib.p);
		else hipLaunchKernelGGL(lsq_xb_count_kernel<false>, grid, dim3(256), 0, st, R, I, d_reads.p, d_total.p, d_acc.p);
		HIP_TRY(hipGetLastError());
	}

	// ---- copy-back
	HIP_TRY(PC.mark(2, st));
	if (nb) HIP_TRY(hipMemcpyAsync(t.reads.data(), d_reads.p, nb * 8, hipMemcpyDeviceToHost, st));
	if (ng) HIP_TRY(hipMemcpyAsync(t.total.data(), d_total.p, ng * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&acc, d_acc.p, sizeof(acc), hipMemcpyDeviceToHost, st));
	if (stranded) HIP_TRY(hipMemcpyAsync(t.lib, d_lib.p, LIB_REPORT * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(PC.mark(3, st));
	HIP_TRY(hipStreamSynchronize(st));
	t.report[2] = acc.bad_blocks; t.report[3] = acc.no_gene; t.report[4] = acc.multi_gene; t.report[5] = acc.bin_hits;
	for (int k = 0; k < XB_PHASES; ++k) (void)PC.ms(k, &t.ms[k]);
	return LSQ_OK;
}
