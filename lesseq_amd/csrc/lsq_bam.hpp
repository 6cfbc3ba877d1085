// BAM_SINGLE on the host, header only: the BGZF block chain, the inflate of every block with the shared decoder
// (lsq_inflate.hpp; no zlib), the BAM header, and the loop over the records (lsq_bam_record.hpp).  lsq_bam.cpp (parser,
// converter), the device chain's host side (lsq_bam_device.hpp: block table and header) and tools/bam_decode_check.cpp use it;
// it depends on nothing of the library.  DESIGN.md 4.10.
//
// Errors, in the order a file meets them: the block chain (all of it), the deflate streams (first failing block in file order),
// the BAM header, the records (first malformed record in file order).  With `verify` (bam_open, bgzf_inflate_all; off unless a
// caller asks) two checks stand between the deflate streams and the header: every block's CRC32 (lsq_crc32.hpp) against the
// stored one, the first differing block in file order, and the end-of-file marker as the file's last 28 bytes.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "lsq_bam_record.hpp"
#include "lsq_crc32.hpp"
#include "lsq_inflate.hpp"

namespace lsq {

constexpr int BAM_OK = 0, BAM_E_FORMAT = -3, BAM_E_PARSE = -4, BAM_E_RANGE = -5;       // (the values of LSQ_E_FORMAT, LSQ_E_PARSE, LSQ_E_RANGE)
constexpr uint32_t BGZF_MAX_ISIZE = 65536;

struct BamError { int status = BAM_OK; std::string text; };

// one BGZF block: where it begins in the file, its deflate stream, and its bytes' place in the inflated stream
struct BgzfBlock { uint64_t file_off, in_off; uint32_t in_len, isize; uint64_t out_off; };

// A file-level error is a file that is not of the format named: the message ends as the reference's does for a format it does not know.
inline int bam_format_error(BamError &e, const std::string &what, uint64_t file_off) {
	e.status = BAM_E_FORMAT;
	e.text = what + " in the BGZF block at file offset " + std::to_string(file_off) + ": Unknown file format error: BAM_SINGLE";
	return e.status;
}
inline int bam_inflate_error(BamError &e, int inflate_status, uint64_t file_off) {
	return bam_format_error(e, std::string("invalid deflate stream (") + inflate_status_text(inflate_status) + ")", file_off);
}
inline int bam_crc_error(BamError &e, uint32_t stored, uint32_t computed, uint64_t file_off) {
	char what[80];
	snprintf(what, sizeof what, "CRC32 mismatch (stored 0x%08x, computed 0x%08x)", (unsigned)stored, (unsigned)computed);
	return bam_format_error(e, what, file_off);
}
// the empty block that ends a BGZF file: a file cut at a block boundary lacks it
constexpr unsigned char BGZF_EOF_MARKER[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};
inline int bam_check_eof_marker(const unsigned char *b, uint64_t len, BamError &e) {
	if (len >= sizeof BGZF_EOF_MARKER && memcmp(b + len - sizeof BGZF_EOF_MARKER, BGZF_EOF_MARKER, sizeof BGZF_EOF_MARKER) == 0) return BAM_OK;
	return bam_format_error(e, "no end-of-file marker", len);
}
// the CRC32 a block stores: the four bytes behind its deflate stream
inline uint32_t bgzf_stored_crc(const unsigned char *b, const BgzfBlock &B) { return bam_le32(b + B.in_off + B.in_len); }
inline int bam_record_error(BamError &e, uint64_t line_no, uint64_t byte) {
	e.status = BAM_E_PARSE;
	e.text = "#" + std::to_string(line_no) + ":<BAM record at byte " + std::to_string(byte) + " of the inflated stream>";
	return e.status;
}

// The block chain of a file's bytes (BSIZE to BSIZE), with the output offsets as the prefix sum of ISIZE.
inline int bgzf_block_table(const unsigned char *b, uint64_t len, std::vector<BgzfBlock> &tab, uint64_t &total, BamError &e) {
	tab.clear();
	total = 0;
	if (len == 0) return bam_format_error(e, "no BAM magic", 0);
	for (uint64_t o = 0; o < len;) {
		if (len - o < 18u || b[o] != 31u || b[o + 1] != 139u || b[o + 2] != 8u || (b[o + 3] & 4u) == 0u) return bam_format_error(e, "bad gzip magic", o);
		const uint64_t xlen = bam_le16(b + o + 10);
		if (12u + xlen > len - o) return bam_format_error(e, "gzip extra field past the end of the file", o);
		uint64_t bsize = 0;
		for (uint64_t x = 0; x + 4u <= xlen;) {
			const unsigned char *sf = b + o + 12 + x;
			const uint64_t slen = bam_le16(sf + 2);
			if (sf[0] == 66u && sf[1] == 67u && slen == 2u && x + 6u <= xlen) { bsize = (uint64_t)bam_le16(sf + 4) + 1u; break; }
			x += 4u + slen;
		}
		if (bsize == 0) return bam_format_error(e, "no BC subfield", o);
		if (bsize > len - o) return bam_format_error(e, "BSIZE past the end of the file", o);
		if (bsize < 12u + xlen + 8u) return bam_format_error(e, "BSIZE smaller than the block's own header", o);
		const uint32_t isize = bam_le32(b + o + bsize - 4);
		if (isize > BGZF_MAX_ISIZE) return bam_format_error(e, "ISIZE above 65536", o);
		tab.push_back(BgzfBlock{o, o + 12u + xlen, (uint32_t)(bsize - 12u - xlen - 8u), isize, total});
		total += isize;
		o += bsize;
	}
	return BAM_OK;
}

// Every block of the table into out (total bytes), by n_threads threads; the first failing block in file order speaks.  With
// `verify` each thread checksums the blocks it inflated: a deflate error anywhere in the file comes before a CRC32 that differs.
inline int bgzf_inflate_all(const unsigned char *b, const std::vector<BgzfBlock> &tab, unsigned char *out, int n_threads, BamError &e, bool verify = false) {
	std::atomic<uint64_t> first_bad{~0ull}, first_crc{~0ull};
	auto lower = [](std::atomic<uint64_t> &word, uint64_t mine) {
		uint64_t cur = word.load();
		while (mine < cur && !word.compare_exchange_weak(cur, mine)) {}
	};
	auto work = [&](size_t t, size_t T) {
		for (size_t k = t; k < tab.size(); k += T) {
			const int st = inflate_block(b + tab[k].in_off, tab[k].in_len, out + tab[k].out_off, tab[k].isize);
			if (st) lower(first_bad, ((uint64_t)k << 8) | (uint64_t)st);
			else if (verify && crc32_bytes(out + tab[k].out_off, tab[k].isize) != bgzf_stored_crc(b, tab[k])) lower(first_crc, (uint64_t)k);
		}
	};
	const size_t T = (size_t)std::max(1, std::min<int>(n_threads, (int)std::min<size_t>(tab.size() / 16 + 1, 64)));
	if (T == 1) work(0, 1);
	else {
		std::vector<std::thread> th;
		for (size_t t = 0; t < T; ++t) th.emplace_back(work, t, T);
		for (auto &x : th) x.join();
	}
	const uint64_t bad = first_bad.load();
	if (bad != ~0ull) return bam_inflate_error(e, (int)(bad & 0xFFu), tab[(size_t)(bad >> 8)].file_off);
	if (first_crc.load() != ~0ull) {
		const BgzfBlock &B = tab[(size_t)first_crc.load()];
		return bam_crc_error(e, bgzf_stored_crc(b, B), crc32_bytes(out + B.out_off, B.isize), B.file_off);
	}
	return BAM_OK;
}

struct BamHeader {
	uint64_t end = 0;                        // where the first record begins
	uint64_t h_lines = 0;                    // lines of the header text
	std::vector<std::string> ref_names;
	std::vector<unsigned char> ref_walks;    // per reference: can its name be an MRF chromosome
};
constexpr int BAM_HEADER_NEED_MORE = 1;
// The header from the first `avail` bytes of an inflated stream of `total`: BAM_OK, BAM_HEADER_NEED_MORE (avail < total
// and the header runs on), or an error (the header begins in the first block: file offset 0).
inline int bam_parse_header(const unsigned char *s, uint64_t avail, uint64_t total, BamHeader &H, BamError &e) {
	auto more = [&](const char *what) { return avail < total ? BAM_HEADER_NEED_MORE : bam_format_error(e, std::string("the BAM header is cut short (") + what + ")", 0); };
	if (total < 4u || (avail >= 4u && memcmp(s, "BAM\1", 4) != 0)) return bam_format_error(e, "bad BAM magic", 0);
	if (total < 12u) return bam_format_error(e, "the BAM header is cut short (l_text)", 0);
	if (avail < 8u) return more("l_text");
	const uint64_t l_text = bam_le32(s + 4);
	if (l_text > total - 8u) return bam_format_error(e, "the BAM header is cut short (text)", 0);
	if (avail < 12u + l_text) return more("text");
	// the text as a C string: its lines, a last one without '\n' among them
	uint64_t n_text = 0;
	while (n_text < l_text && s[8 + n_text] != 0u) ++n_text;
	H.h_lines = (uint64_t)std::count(s + 8, s + 8 + n_text, (unsigned char)'\n') + (n_text && s[8 + n_text - 1] != '\n' ? 1u : 0u);
	uint64_t p = 8u + l_text;
	const uint64_t n_ref = bam_le32(s + p);
	p += 4;
	if (n_ref > 0x7FFFFFFFull || n_ref * 9u > total - p) return bam_format_error(e, "the BAM header is cut short (references)", 0);
	H.ref_names.clear();
	H.ref_walks.clear();
	for (uint64_t r = 0; r < n_ref; ++r) {
		if (avail - p < 4u) return more("reference name length");
		const uint64_t l_name = bam_le32(s + p);
		if (l_name == 0u || l_name > total - p - 4u || total - p - 4u - l_name < 4u) return bam_format_error(e, "the BAM header is cut short (reference name)", 0);
		if (avail - p - 4u < l_name + 4u) return more("reference name");
		const char *nm = (const char *)s + p + 4;
		const size_t n = strnlen(nm, (size_t)l_name);
		H.ref_names.emplace_back(nm, n);
		H.ref_walks.push_back(bam_ref_name_walks(nm, n) ? 1u : 0u);
		p += 4u + l_name + 4u;
	}
	H.end = p;
	return BAM_OK;
}

// A whole file's bytes: the inflated stream and its header.
struct BamStream { std::vector<unsigned char> bytes; BamHeader H; uint64_t n_blocks = 0; };
inline int bam_open(const unsigned char *file, uint64_t len, int n_threads, BamStream &S, BamError &e, bool verify = false) {
	std::vector<BgzfBlock> tab;
	uint64_t total = 0;
	int st = bgzf_block_table(file, len, tab, total, e);
	if (st) return st;
	S.n_blocks = tab.size();
	S.bytes.assign((size_t)total + 16, 0);
	if ((st = bgzf_inflate_all(file, tab, S.bytes.data(), n_threads, e, verify))) return st;
	if (verify && (st = bam_check_eof_marker(file, len, e))) return st;
	S.bytes.resize((size_t)total);
	return bam_parse_header(S.bytes.data(), total, total, S.H, e);
}

// Every record in file order: on_block(ref_id, minus, start, end, qstart, qend) as bam_split_record calls it, then
// on_record(line_no, verdict) -- SAM_NO_READ or SAM_READ; the first malformed record ends the loop with its error.
template <class OnBlock, class OnRecord>
inline int bam_for_each_record(const BamStream &S, unsigned skip_flags, unsigned min_mapq, OnBlock &&on_block, OnRecord &&on_record, BamError &e, const bool mate_strand = false) {
	const unsigned char *s = S.bytes.data();
	const uint64_t total = S.bytes.size();
	const int64_t n_ref = (int64_t)S.H.ref_names.size();
	uint64_t line_no = S.H.h_lines;
	for (uint64_t p = S.H.end; p < total; p = bam_next_record(s, total, p)) {
		++line_no;
		const int v = bam_split_record(s + p, total - p, n_ref, skip_flags, min_mapq, [&](int64_t r) { return S.H.ref_walks[(size_t)r] != 0u; }, on_block, mate_strand);
		if (v == SAM_MALFORMED) return bam_record_error(e, line_no, p);
		const int st = on_record(line_no, v);
		if (st) return st;
	}
	return BAM_OK;
}

} // namespace lsq
