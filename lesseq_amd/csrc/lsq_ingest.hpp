// Where the loader chain (lsq_ingest.hip) and the read files (lsq_readfile.hip) meet; not a public header.
// Needs: lsq_route.hpp.  Gives: the front end a caller hands the chain -- the reads of one file as the routing pass meets them -- and
// the chain itself.
#pragma once
#include <functional>

#include "lsq_route.hpp"

namespace lsq {

constexpr int LSQ_RETRY = 1;                           // a front end's settle(): route the file again (it has changed its own mode)

struct Front {
	unsigned long long n = 0;                 // reads of the pass (text: data lines, skipped ones among them)
	const unsigned *line_no = nullptr;        // per read (device), or null: first_line + index
	unsigned long long first_line = 0;
	unsigned long long in_bytes = 0;          // what the routing pass reads
	const char *stage = "route";              // the routing pass's name in the stage report
	std::function<int(const RouteTables &, const RouteOut &, hipStream_t)> launch;   // runs the routing kernel
	std::function<int(hipStream_t)> settle;   // once the stream has been waited for: the front end's own verdict (the first failing line)
};

RouteTables route_tables(lsq_ctx *c);
unsigned route_lib(const lsq_ctx *c);          // the `lib` word of the stranded routing kernels (lsq_route.hpp); 0 for unstranded events
// Runs the chain over the reads a front end delivers.  The stage report (StageClock, lsq_text.hpp) lists the passes the front end has
// clocked since stages_reset, then the chain's own.
int ingest_device(lsq_ctx *c, int method, Front &F);

} // namespace lsq
