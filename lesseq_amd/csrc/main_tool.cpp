// count / solve / classify executables: the reference's argv, stdout, stderr log and exit
// status (count/count.cpp:88-129, solve/solve.cpp:102-146, classify/classify.cpp:51-79);
// test_as, the differential splicing tests of bin/Test_AS.r (lsq_as.cpp); events, the local events of bin/Events.r
// (lsq_localev.cpp); parseGencode and gencodeIsoformMap, the annotation from a GTF (lsq_gtf.cpp); sam2mrf and bam2mrf, the MRF
// equivalent of an alignment file (lsq_sam.cpp, lsq_bam.cpp); bamcheck, the whole-file check of a BAM file (lsq_cli.cpp);
// junctions, the splice junctions of a read file (lsq_junc.cpp); coverage, its per-base depth (lsq_cov.cpp); exonbins, its reads
// per exon bin and per gene (lsq_exonbins.cpp); psi, its junction reads per event form (lsq_psi.cpp); evidence, its junction and
// exon-body reads per event form (lsq_evidence.cpp); sites, its splice-site usage and read-through per junction (lsq_sites.cpp);
// retention, its depth quartiles and IR ratio per intron (lsq_retention.cpp); libtype, which library type it is (lsq_libtype.cpp).
// The tool is chosen by the program name.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/lesseq_hip.h"

int main(int argc, char **argv) {
	const char *base = strrchr(argv[0], '/');
	base = base ? base + 1 : argv[0];
	const char *tool = strstr(base, "libtype") ? "libtype" : strstr(base, "retention") ? "retention" : strstr(base, "sites") ? "sites" : strstr(base, "evidence") ? "evidence" : strstr(base, "psi") ? "psi" : strstr(base, "exonbins") ? "exonbins" : strstr(base, "coverage") ? "coverage" : strstr(base, "junctions") ? "junctions" : strstr(base, "sam2mrf") ? "sam2mrf" : strstr(base, "bam2mrf") ? "bam2mrf" : strstr(base, "bamcheck") ? "bamcheck" : strstr(base, "parseGencode") ? "parseGencode" : strstr(base, "gencodeIsoformMap") ? "gencodeIsoformMap" : strstr(base, "events") ? "events" : strstr(base, "test_as") ? "test_as" : strstr(base, "solve") ? "solve" : (strstr(base, "classify") ? "classify" : "count");
	return lsq_cli_main(tool, argc, argv);
}
