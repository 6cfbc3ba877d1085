// The shared CRC-32 header (lesseq_amd/csrc/lsq_crc32.hpp) as a program of its own, for runs under the host sanitizers --
// nothing of the library, no GPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I lesseq_amd/csrc tools/bam_crc_check.cpp -o bam_crc_check
//   bam_crc_check FILE...
// Per file one line "<bytes> <whole> <combined> <folded>", the sums as eight hex digits: the bytes in one run; in the 64 slices
// the device pass gives the lanes of a wave (lsq_bam_device.hpp: ceil(bytes / 64) rounded up to 16 each), every slice finalised
// and the 64 joined left to right by crc32_combine; and as the kernel folds them -- raw registers, lane 0 from 0xFFFFFFFF,
// each times crc32_xpow8(bytes behind its slice), xor-ed.  tests/test_bam_crc_host.py holds all three against zlib.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "lsq_crc32.hpp"

using namespace lsq;

int main(int argc, char **argv) {
	if (argc < 2) { fprintf(stderr, "usage: bam_crc_check FILE...\n"); return 2; }
	for (int a = 1; a < argc; ++a) {
		std::ifstream f(argv[a], std::ios::binary);
		if (!f) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
		// (the bytes in an allocation of their exact size: a read one byte beyond them is the sanitizer's to see)
		std::vector<unsigned char> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
		std::vector<unsigned char> exact(file.begin(), file.end());
		exact.shrink_to_fit();
		const uint32_t n = (uint32_t)exact.size();
		const unsigned char *const base = exact.empty() ? reinterpret_cast<const unsigned char *>("") : exact.data();
		if (exact.size() > 65536u) { fprintf(stderr, "%s: more than 65536 bytes\n", argv[a]); return 2; }
		const uint32_t S = (((n + 63u) >> 6) + 15u) & ~15u;
		uint32_t combined = 0, folded = 0;
		for (uint32_t l = 0; l < 64u; ++l) {
			const uint32_t lo = l * S < n ? l * S : n, hi = lo + S < n ? lo + S : n;
			combined = crc32_combine(combined, crc32_bytes(base + lo, hi - lo), hi - lo);
			const uint32_t c = crc32_update(l == 0u ? 0xFFFFFFFFu : 0u, base + lo, hi - lo, crc32_host_tables());
			folded ^= crc32_mulmod(c, crc32_xpow8(n - hi));
		}
		printf("%u %08x %08x %08x\n", (unsigned)n, (unsigned)crc32_bytes(base, n), (unsigned)combined, (unsigned)(folded ^ 0xFFFFFFFFu));
	}
	return 0;
}
