// The tables lsq_events_upload (lsq_device.hip) copies to the device, worked out from compiled events alone: standard C++, no HIP
// header, every function pure -- so that tests/test_upload_tables_host.py can hold them against their definitions on a machine
// without a GPU (lsq_debug_upload_tables, include/lesseq_hip_dev.h).
#pragma once
#include "lsq_internal.hpp"

namespace lsq {

// records the device reads as int2 / uint2 / int4 (lsq_device.hip ties the layouts together)
struct CovRec { int x, y; };                 // a covered region: start, end
struct LocRec { unsigned x, y; };            // a locator entry: lower bounds among the covered starts (.x) and the cluster starts (.y)
struct CluRec { int x, y, z, w; };           // a cluster record: start, end (inclusive, clamped to the bucket's hi), bucket, the bucket's first base

// EM places: events with at most two isoforms and one (method, class) pair per lane first ("lean"), then the others; each
// group padded with 0xFFFFFFFF to whole waves (64 / EM_LANES events) so that a wave runs one loop shape.  Events of host buckets
// (solved on the host) have no place.
struct EmPlacement {
	std::vector<uint32_t> order;             // device event per place
	unsigned small_places = 0, places = 0;   // the lean group's places (the first ones); all places
};
EmPlacement em_placement(const lsq_events &E);

// lsq_results_pack_device: where every class slot, isoform and event of the shard sits in the device arrays, listed in output
// order (the shard is a contiguous run of output-ordered events)
struct PackLists { std::vector<uint32_t> cls, iso, ev; };
PackLists pack_lists(const lsq_events &E);

// G = 1/ARS (common/read.h:331-340), [method][device isoform]; zero where an isoform has no accessible start
std::vector<double> start_weights(const lsq_events &E);

// The loader's tables: per table id (lsq_events::table_of) a RouteChrom; the covered regions (count/count.cpp:244); the clusters
// (spans of the planned events) with the bucket each lies in, cut at the bucket cuts; and the locator grid over both: per
// chromosome bins of 2^shift bases, entry k = lower bounds of the bin's first base among the covered starts (.x) and the cluster
// starts (.y); entries k and k + 1, one 16-byte load, bound a search to a handful of neighbouring records.  loc ends in two zero
// entries (an entry is read as a pair with its successor); cov and clu hold one zero record where they would be empty.
struct RouteHostTables {
	std::vector<RouteChrom> chrom;           // at least one record
	std::vector<CovRec> cov;
	std::vector<CluRec> clu;
	std::vector<LocRec> loc;
	unsigned shift = 10, n_chrom = 0;        // n_chrom: table ids that exist
};
RouteHostTables route_host_tables(const lsq_events &E);

// Per bucket (n_buckets + 1 values each) the first of its bins among all bins, of its groups of the one-block pool (its cells and
// one more group for the reads that start in no cell) and of its groups of the two-block pool (its junction groups, then one a
// cell and one for "no cell": two-block reads that cross no junction of the annotation); the last values are the totals.
struct GroupBases {
	std::vector<unsigned> bin_base, cell_base, jgroup_base;
	size_t n_fine = 0, n_cell_groups = 0, n_junction_groups = 0;
};
GroupBases group_bases(const lsq_events &E);

// gene names in device event order, for span-start ties against named reads: one blob and n_events + 1 offsets into it
struct GeneNames { std::string blob; std::vector<uint32_t> off; };
GeneNames gene_names(const lsq_events &E);

} // namespace lsq
