// The shared BAM headers (lesseq_amd/csrc: lsq_inflate.hpp, lsq_bam_record.hpp, lsq_bam.hpp) as a program of their own, for runs
// under the host sanitizers -- nothing of the library, no GPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I lesseq_amd/csrc tools/bam_decode_check.cpp -o bam_decode_check
//   bam_decode_check inflate FILE EXPECTED     the BGZF blocks of FILE inflated; "ok <bytes>" when the stream equals EXPECTED's bytes
//   bam_decode_check mrf FILE [SKIP MAPQ]      FILE through the whole host path; "ok <records> <reads> <blocks>"
// A file the headers reject prints "<status> <message>" -- the library's status and message for it -- and that is a clean run too:
// exit status 0 whenever the headers gave an answer, 2 for a bad command line or a stream that differs.  tests/test_bam_host.py
// feeds it the good and the corrupt streams of the suite.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "lsq_bam.hpp"

using namespace lsq;

static bool slurp(const char *path, std::vector<unsigned char> &out) {
	std::ifstream f(path, std::ios::binary);
	if (!f) return false;
	out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
	return true;
}

int main(int argc, char **argv) {
	if (argc < 3) { fprintf(stderr, "usage: bam_decode_check inflate FILE EXPECTED | mrf FILE [SKIP MAPQ]\n"); return 2; }
	const std::string mode = argv[1];
	std::vector<unsigned char> file;
	if (!slurp(argv[2], file)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
	// (the bytes in an allocation of their exact size: a read one byte beyond them is the sanitizer's to see)
	std::vector<unsigned char> exact(file.begin(), file.end());
	exact.shrink_to_fit();
	BamError e;
	if (mode == "inflate" && argc == 4) {
		std::vector<unsigned char> want;
		if (!slurp(argv[3], want)) { fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
		std::vector<BgzfBlock> tab;
		uint64_t total = 0;
		if (bgzf_block_table(exact.data(), exact.size(), tab, total, e)) { printf("%d %s\n", e.status, e.text.c_str()); return 0; }
		std::vector<unsigned char> out((size_t)total);
		for (int threads : {1, 4}) {
			std::fill(out.begin(), out.end(), 0);
			if (bgzf_inflate_all(exact.data(), tab, out.data(), threads, e)) { printf("%d %s\n", e.status, e.text.c_str()); return 0; }
			if (out != want) { printf("differs\n"); return 2; }
		}
		printf("ok %llu\n", (unsigned long long)total);
		return 0;
	}
	if (mode == "mrf" && (argc == 3 || argc == 5)) {
		const unsigned skip = argc == 5 ? (unsigned)strtoul(argv[3], nullptr, 0) : SAM_DEFAULT_SKIP_FLAGS, mapq = argc == 5 ? (unsigned)strtoul(argv[4], nullptr, 0) : 0u;
		BamStream S;
		if (bam_open(exact.data(), exact.size(), 2, S, e)) { printf("%d %s\n", e.status, e.text.c_str()); return 0; }
		unsigned long long records = 0, reads = 0, blocks = 0;
		const int st = bam_for_each_record(S, skip, mapq, [&](int64_t, bool, int64_t, int64_t, int64_t, int64_t) { ++blocks; },
		                                   [&](uint64_t, int v) { ++records; reads += v == SAM_READ; return (int)BAM_OK; }, e);
		if (st) { printf("%d %s\n", e.status, e.text.c_str()); return 0; }
		printf("ok %llu %llu %llu\n", records, reads, blocks);
		return 0;
	}
	fprintf(stderr, "usage: bam_decode_check inflate FILE EXPECTED | mrf FILE [SKIP MAPQ]\n");
	return 2;
}
