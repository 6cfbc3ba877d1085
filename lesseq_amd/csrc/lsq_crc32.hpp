// The gzip CRC-32 (reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF), one source for the host BAM
// parser (lsq_bam.hpp: bgzf_inflate_all) and the device pass behind the inflate kernel (lsq_bam_device.hpp:
// lsq_bgzf_crc_kernel).  DESIGN.md 4.10.
//
// Two things live here.  The update of a register over a run of bytes, four bytes a step through four tables of 256 words
// (slicing-by-4): the tables are generated, at compile time for the host and into LDS by the kernel, from crc32_table_entry.
// And the arithmetic that lets a run be checksummed in pieces: CRC-32 is linear over GF(2), a register that then meets n zero
// bytes is the register times x^(8n) modulo the polynomial, so the checksum of A followed by B is
//     crc32_combine(crc(A), crc(B), |B|) = crc32_mulmod(crc(A), crc32_xpow8(|B|)) ^ crc(B)
// on finalised values (zlib's crc32_combine identity), and on raw registers alike.  A residue is held as the register holds
// it: bit 31 is the coefficient of x^0.
#pragma once
#include <cstddef>
#include <cstdint>

#include "lsq_mrf_line.hpp"

namespace lsq {

constexpr uint32_t CRC32_POLY = 0xEDB88320u;
constexpr uint32_t CRC32_ONE = 0x80000000u;         // x^0
constexpr unsigned CRC32_TABLE_WORDS = 4u * 256u;   // table k (0..3) at [256 k, 256 k + 256)
constexpr unsigned CRC32_POW_ENTRIES = 17u;         // x^(8 * 2^k), k = 0..16: enough for n <= 65 536, a BGZF block

// the register after byte i and then k zero bytes, from a zero register: entry i of table k
LSQ_HD constexpr uint32_t crc32_table_entry(unsigned i, unsigned k) {
	uint32_t c = i;
	for (unsigned s = 0; s < 8u * (k + 1u); ++s) c = (c >> 1) ^ (CRC32_POLY & (0u - (c & 1u)));
	return c;
}

// a * b modulo the polynomial, both residues and the product in the reflected representation: 32 shift-and-xor steps
LSQ_HD constexpr uint32_t crc32_mulmod(uint32_t a, uint32_t b) {
	uint32_t p = 0;
	for (unsigned s = 0; s < 32u; ++s) {
		p ^= b & (0u - ((a >> (31u - s)) & 1u));
		b = (b >> 1) ^ (CRC32_POLY & (0u - (b & 1u)));
	}
	return p;
}

struct Crc32Tables { uint32_t v[CRC32_TABLE_WORDS]; };
struct Crc32Powers { uint32_t v[CRC32_POW_ENTRIES]; };
constexpr Crc32Tables crc32_make_tables() {
	Crc32Tables T{};
	for (unsigned k = 0; k < 4u; ++k)
		for (unsigned i = 0; i < 256u; ++i) T.v[256u * k + i] = crc32_table_entry(i, k);
	return T;
}
constexpr Crc32Powers crc32_make_powers() {
	Crc32Powers T{};
	T.v[0] = CRC32_ONE >> 8;            // x^8
	for (unsigned k = 1; k < CRC32_POW_ENTRIES; ++k) T.v[k] = crc32_mulmod(T.v[k - 1u], T.v[k - 1u]);
	return T;
}

// x^(8n) modulo the polynomial, n <= 131 071 (the table's 17 bits; a BGZF block needs 65 536): square-and-multiply over the table
LSQ_HD inline uint32_t crc32_xpow8(uint32_t n) {
	static constexpr Crc32Powers T = crc32_make_powers();
	uint32_t p = CRC32_ONE;
	for (unsigned k = 0; k < CRC32_POW_ENTRIES && (n >> k) != 0u; ++k)
		if ((n >> k) & 1u) p = crc32_mulmod(p, T.v[k]);
	return p;
}

LSQ_HD inline uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint32_t len_b) { return crc32_mulmod(crc_a, crc32_xpow8(len_b)) ^ crc_b; }

// The register c over n bytes, no initial value or final xor applied.  `tab`: the four tables (crc32_host_tables(), or the
// kernel's copy in LDS).
LSQ_HD inline uint32_t crc32_step_byte(uint32_t c, unsigned b, const uint32_t *tab) { return tab[(c ^ b) & 0xFFu] ^ (c >> 8); }
LSQ_HD inline uint32_t crc32_step_word(uint32_t c, uint32_t w, const uint32_t *tab) {      // w: four bytes, the first in the low bits
	c ^= w;
	return tab[768u + (c & 0xFFu)] ^ tab[512u + ((c >> 8) & 0xFFu)] ^ tab[256u + ((c >> 16) & 0xFFu)] ^ tab[c >> 24];
}
LSQ_HD inline uint32_t crc32_update(uint32_t c, const unsigned char *p, size_t n, const uint32_t *tab) {
	for (; n >= 4u; p += 4, n -= 4u) c = crc32_step_word(c, (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24), tab);
	for (; n; ++p, --n) c = crc32_step_byte(c, *p, tab);
	return c;
}

// host: the tables, made at compile time; the finalised checksum of n bytes
inline const uint32_t *crc32_host_tables() {
	static constexpr Crc32Tables T = crc32_make_tables();
	return T.v;
}
inline uint32_t crc32_bytes(const unsigned char *p, size_t n) { return crc32_update(0xFFFFFFFFu, p, n, crc32_host_tables()) ^ 0xFFFFFFFFu; }

} // namespace lsq
