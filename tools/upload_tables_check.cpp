// The host unit behind lsq_events_upload (csrc/lsq_upload_tables.cpp) under the host sanitizers, as a program of its own: no HIP,
// no Python.  It loads an annotation, compiles the events with their device plan and builds every table; then it builds the
// loader's tables of events made by hand whose first cluster begins LEFT of the chromosome's first bucket cut -- a shape the
// planner never makes (the first cut is the first cluster's start), so only this program reaches the rule that such a stretch
// gets no record.  Two ways to build it.  Against the built library, as tests/test_upload_tables_host.py does on every run of the
// suite (there a dropped rule indexes the buckets four thousand million records out and the program dies):
//   g++ -O1 -std=c++17 -o upload_tables_check tools/upload_tables_check.cpp -Llesseq_amd/_build -llesseq_hip -Wl,-rpath,$PWD/lesseq_amd/_build
// Or from the two host sources alone, under the sanitizers (from lesseq_amd/csrc):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -ffp-contract=off -pthread -o upload_tables_check
//       ../../tools/upload_tables_check.cpp lsq_upload_tables.cpp lsq_annot.cpp
// Either way: upload_tables_check x.interval x.map
#include "../lesseq_amd/csrc/lsq_upload_tables.hpp"

#include <cstdlib>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "upload_tables_check: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

int main(int argc, char **argv) {
	using namespace lsq;
	if (argc != 3) { fprintf(stderr, "usage: upload_tables_check x.interval x.map\n"); return 2; }
	lsq_annotation *a = nullptr;
	CHECK(lsq_annotation_load("LH_GENE_TXT", argv[1], "UCSC_GENE2ISOFORM", argv[2], 0, 1000000, &a) == LSQ_OK);
	for (int n_files = 1; n_files <= 2; ++n_files) {
		const char *types[2] = {"SHORT_READ", "SHORT_READ"};
		const uint64_t lengths[2] = {100, 75};
		lsq_events *E = nullptr;
		CHECK(lsq_events_compile(a, n_files, types, lengths, &E) == LSQ_OK);
		const EmPlacement P = em_placement(*E);
		const PackLists L = pack_lists(*E);
		const std::vector<double> G = start_weights(*E);
		const RouteHostTables T = route_host_tables(*E);
		const GroupBases B = group_bases(*E);
		const GeneNames N = gene_names(*E);
		CHECK(P.places % 16 == 0 && P.small_places <= P.places && P.order.size() == P.places);
		CHECK(L.ev.size() == E->dev2out.size() && L.cls.size() == E->n_cls_total && L.iso.size() == E->n_iso_total);
		CHECK(G.size() == (size_t)n_files * E->n_iso_total);
		CHECK(T.loc.size() >= 2 && T.chrom.size() >= 1 && !T.cov.empty() && !T.clu.empty());
		CHECK(B.bin_base.size() == E->buckets.size() + 1 && B.jgroup_base.back() == B.n_junction_groups);
		CHECK(N.off.back() == N.blob.size());
		printf("%d read file(s): %zu events, %u places (%u lean), %zu covered regions, %zu cluster records, %zu locator entries at shift %u\n", n_files,
		       E->dev2out.size(), P.places, P.small_places, T.cov.size(), T.clu.size(), T.loc.size(), T.shift);
		lsq_events_free(E);
	}
	lsq_annotation_free(a);
	// by hand: one chromosome, buckets cut at 1000 and 2000; clusters [400, 600] (left of the first cut), [900, 1100] (across
	// it), [2500, 2600]
	lsq_events H;
	H.covered.resize(1);
	H.covered[0].s = {400, 900, 2500}; H.covered[0].e = {601, 1101, 2601};
	H.buckets.resize(2);
	H.buckets[0].lo = 1000; H.buckets[0].hi = 1100; H.buckets[1].lo = 2000; H.buckets[1].hi = 2550;
	H.chrom_first_bucket = {0};
	H.cut_lo = {{1000, 2000}};
	H.clu_s = {{400, 900, 2500}}; H.clu_e = {{600, 1100, 2600}};
	const RouteHostTables T = route_host_tables(H);
	CHECK(T.clu.size() == 2);          // nothing for [400, 600], nothing for [900, 999]
	CHECK(T.clu[0].x == 1000 && T.clu[0].y == 1100 && T.clu[0].z == 0 && T.clu[0].w == 1000);
	CHECK(T.clu[1].x == 2500 && T.clu[1].y == 2550 && T.clu[1].z == 1 && T.clu[1].w == 2000);          // (.y clamped to the bucket's hi)
	CHECK(T.chrom[0].clu0 == 0 && T.chrom[0].clu1 == 2 && T.chrom[0].loc_base == 0 && T.shift == 10 && T.chrom[0].loc_nb == 3);
	printf("upload_tables_check: ok\n");
	return 0;
}
