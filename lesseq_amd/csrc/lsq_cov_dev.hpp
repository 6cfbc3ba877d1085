// The depth rows of a parsed read file as they lie on the device: what lsq_cov.hip, which makes them, and
// lsq_retention.hip, which selects order statistics from them without a copy to the host, share.
#pragma once

#include "lsq_device.hpp"
#include "lsq_cov.hpp"

namespace lsq {

// stretches of one depth > 0: pieces between neighbouring runs of sort records, or the rows joined from them
struct CovPieces { unsigned *chrom; int *start, *end; unsigned *depth; };
struct DevPieces {
	DevBuf<unsigned> chrom, depth;
	DevBuf<int> start, end;
	int alloc(size_t n) { int rc; if ((rc = chrom.alloc(n)) || (rc = start.alloc(n)) || (rc = end.alloc(n)) || (rc = depth.alloc(n))) return rc; return LSQ_OK; }
	CovPieces view() const { return CovPieces{chrom.p, start.p, end.p, depth.p}; }
};

// lsq_cov.hip: coverage's phases extract, sort, reduce and scan, emit over device arrays (R.n_reads <= 2^32).  `rows`: the n_rows
// rows, ascending in (chromosome index, start), left on the device; report: COV_REPORT entries; PC: marks 0 .. 4 are recorded on the
// context's stream (phase k lies between marks k and k + 1), the later ones are the caller's.  The stream has been waited for.
int cov_device_rows(lsq_ctx *c, const ParsedReads &R, int strand, PhaseClock<COV_PHASES> &PC, DevPieces &rows, unsigned &n_rows, uint64_t *report);

} // namespace lsq
