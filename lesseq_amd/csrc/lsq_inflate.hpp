// A complete DEFLATE (RFC 1951) decoder, shared by the host BAM parser (lsq_bam.cpp) and the device inflate kernel
// (lsq_bam_device.hpp): stored, fixed and dynamic blocks, any number of them per stream.  DESIGN.md 4.10.
//
// It is a template over a source and a sink, as the line splitters are templates over their view:
//   source:  bool next(unsigned &byte)            the next input byte; false behind the last one
//   sink:    int literal(unsigned byte)           one output byte
//            int match(unsigned len, unsigned dist)   len bytes (3..258) copied from dist bytes back (1..32768; may overlap)
//            both return INF_OK or the status that ends the run
// The decoder itself holds no pointer into the input or the output.  A code is decoded from its canonical form -- symbols
// per length and the symbols in code order -- one bit at a time, so nothing is ever indexed by unvalidated input: a bit
// string either reaches a symbol that the code lengths put into the table, or runs out of lengths and is an error.  Lengths
// and distances come from the symbol by arithmetic, not from tables.  Over-subscribed codes are errors; so are incomplete
// ones, but for what zlib lets pass as well -- a code whose longest length is one bit (a single distance used), and a
// distance code without any length (a block of literals only); a bit string outside such a code is an error when it is met.
#pragma once
#include "lsq_mrf_line.hpp"

namespace lsq {

enum InflateStatus {
	INF_OK = 0,
	INF_TRUNCATED = 1,       // the input ends inside the stream
	INF_BLOCK_TYPE = 2,      // block type 3
	INF_STORED_LEN = 3,      // LEN / NLEN of a stored block do not match
	INF_CODE_COUNTS = 4,     // more than 286 literal/length or 30 distance codes; a repeat with nothing before it or past the end
	INF_CODE_OVER = 5,       // an over-subscribed code
	INF_CODE_INCOMPLETE = 6, // an incomplete code
	INF_SYMBOL = 7,          // a bit string no code word begins, or a symbol that names no length or distance
	INF_DISTANCE = 8,        // a distance beyond the bytes produced so far
	INF_OUTPUT_OVER = 9,     // more output than the block's ISIZE
	INF_OUTPUT_UNDER = 10    // less
};
LSQ_HD inline const char *inflate_status_text(int st) {
	switch (st) {
	case INF_TRUNCATED: return "the deflate stream is cut short";
	case INF_BLOCK_TYPE: return "deflate block type 3";
	case INF_STORED_LEN: return "a stored block's LEN and NLEN do not match";
	case INF_CODE_COUNTS: return "bad code length counts";
	case INF_CODE_OVER: return "an over-subscribed code";
	case INF_CODE_INCOMPLETE: return "an incomplete code";
	case INF_SYMBOL: return "an invalid symbol";
	case INF_DISTANCE: return "a distance before the start of the output";
	case INF_OUTPUT_OVER: return "more bytes than ISIZE";
	case INF_OUTPUT_UNDER: return "fewer bytes than ISIZE";
	default: return "ok";
	}
}

// bytes in memory: every read is bounded by n
struct InflateMemSource {
	const unsigned char *p;
	size_t n, at;
	LSQ_HD inline bool next(unsigned &b) { if (at >= n) return false; b = p[at++]; return true; }
};
// bytes to memory: every write is bounded by cap, every distance by the bytes produced
struct InflateMemSink {
	unsigned char *out;
	size_t cap, n;
	LSQ_HD inline int literal(unsigned b) { if (n >= cap) return INF_OUTPUT_OVER; out[n++] = (unsigned char)b; return INF_OK; }
	LSQ_HD inline int match(unsigned len, unsigned dist) {
		if (dist > n) return INF_DISTANCE;
		if (len > cap - n) return INF_OUTPUT_OVER;
		for (unsigned i = 0; i < len; ++i) out[n + i] = out[n - dist + i];
		n += len;
		return INF_OK;
	}
};

constexpr int INF_MAXBITS = 15, INF_MAXLCODES = 286, INF_MAXDCODES = 30, INF_FIXLCODES = 288;

// a code in canonical form: count[l] symbols of length l, symbol[] in code order
struct InflateCode { unsigned short *count, *symbol; };

template <class Source>
struct InflateBits {
	Source &src;
	unsigned buf, cnt;
	LSQ_HD inline bool take(unsigned n, unsigned &v) {      // n <= 16, least significant bit first
		while (cnt < n) {
			unsigned b;
			if (!src.next(b)) return false;
			buf |= b << cnt;
			cnt += 8;
		}
		v = buf & ((1u << n) - 1u);
		buf >>= n;
		cnt -= n;
		return true;
	}
	LSQ_HD inline void to_byte_boundary() { buf >>= (cnt & 7u); cnt &= ~7u; }
};

// the canonical form of n code lengths: INF_OK, INF_CODE_OVER, INF_CODE_INCOMPLETE (the tables are usable either way)
LSQ_HD inline int inflate_construct(InflateCode h, const unsigned short *length, int n) {
	unsigned short offs[INF_MAXBITS + 1];
	for (int l = 0; l <= INF_MAXBITS; ++l) h.count[l] = 0;
	for (int s = 0; s < n; ++s) ++h.count[length[s]];        // (every length is <= 15: a 4-bit field, or the fixed code's)
	if (h.count[0] == n) return INF_OK;                      // no codes at all: complete, and nothing decodes
	int left = 1;
	for (int l = 1; l <= INF_MAXBITS; ++l) {
		left <<= 1;
		left -= (int)h.count[l];
		if (left < 0) return INF_CODE_OVER;
	}
	offs[1] = 0;
	for (int l = 1; l < INF_MAXBITS; ++l) offs[l + 1] = (unsigned short)(offs[l] + h.count[l]);
	for (int s = 0; s < n; ++s) if (length[s] != 0) h.symbol[offs[length[s]]++] = (unsigned short)s;
	return left > 0 ? INF_CODE_INCOMPLETE : INF_OK;
}
// an incomplete code zlib accepts: its longest length is one bit
LSQ_HD inline bool inflate_single_bit_code(InflateCode h) {
	for (int l = 2; l <= INF_MAXBITS; ++l) if (h.count[l]) return false;
	return true;
}

// one symbol: INF_OK, INF_TRUNCATED, INF_SYMBOL.  index + (code - first) < the number of symbols with a length, always.
template <class Source>
LSQ_HD inline int inflate_decode(InflateBits<Source> &B, InflateCode h, unsigned &sym) {
	int code = 0, first = 0, index = 0;
	for (int l = 1; l <= INF_MAXBITS; ++l) {
		unsigned bit;
		if (!B.take(1, bit)) return INF_TRUNCATED;
		code |= (int)bit;
		const int count = h.count[l];
		if (code - count < first) { sym = h.symbol[index + (code - first)]; return INF_OK; }
		index += count;
		first += count;
		first <<= 1;
		code <<= 1;
	}
	return INF_SYMBOL;
}

// the literals, lengths and distances of one block
template <class Source, class Sink>
LSQ_HD inline int inflate_codes(InflateBits<Source> &B, Sink &out, InflateCode lencode, InflateCode distcode) {
	for (;;) {
		unsigned sym, extra;
		int st = inflate_decode(B, lencode, sym);
		if (st) return st;
		if (sym < 256u) { if ((st = out.literal(sym))) return st; continue; }
		if (sym == 256u) return INF_OK;
		if (sym > 285u) return INF_SYMBOL;
		// length: 257..264 -> 3..10; 265..284 -> e = (sym - 261) / 4 extra bits on ((4 + (sym - 261) % 4) << e) + 3; 285 -> 258
		unsigned len;
		if (sym == 285u) len = 258u;
		else if (sym < 265u) len = sym - 254u;
		else {
			const unsigned e = (sym - 261u) >> 2;
			if (!B.take(e, extra)) return INF_TRUNCATED;
			len = ((4u + ((sym - 261u) & 3u)) << e) + 3u + extra;
		}
		if ((st = inflate_decode(B, distcode, sym))) return st;
		if (sym > 29u) return INF_SYMBOL;
		// distance: 0..3 -> 1..4; else e = sym / 2 - 1 extra bits on ((2 + sym % 2) << e) + 1
		unsigned dist;
		if (sym < 4u) dist = sym + 1u;
		else {
			const unsigned e = (sym >> 1) - 1u;
			if (!B.take(e, extra)) return INF_TRUNCATED;
			dist = ((2u + (sym & 1u)) << e) + 1u + extra;
		}
		if ((st = out.match(len, dist))) return st;
	}
}

// The decoder's tables -- two codes in canonical form and the code lengths they are made from -- live in memory the caller
// gives: INF_WORK_SHORTS 16-bit words (the host's stack; the lane's private segment on the device).
constexpr int INF_WORK_SHORTS = 2 * (INF_MAXBITS + 1) + INF_FIXLCODES + (INF_MAXDCODES + 2) + (INF_FIXLCODES + INF_MAXDCODES + 2);

// A whole deflate stream from `src` into `out`.  The caller compares what the sink holds with ISIZE (inflate_block does).
template <class Source, class Sink>
LSQ_HD inline int inflate_stream(Source &src, Sink &out, unsigned short *work) {
	InflateBits<Source> B{src, 0u, 0u};
	unsigned short *lencnt = work, *lensym = lencnt + (INF_MAXBITS + 1), *distcnt = lensym + INF_FIXLCODES, *distsym = distcnt + (INF_MAXBITS + 1);
	unsigned short *lengths = distsym + (INF_MAXDCODES + 2);
	const InflateCode lencode{lencnt, lensym}, distcode{distcnt, distsym};
	unsigned last, type, v;
	do {
		if (!B.take(1, last) || !B.take(2, type)) return INF_TRUNCATED;
		if (type == 0u) {
			B.to_byte_boundary();
			unsigned len, nlen;
			if (!B.take(16, len) || !B.take(16, nlen)) return INF_TRUNCATED;
			if ((len ^ 0xFFFFu) != nlen) return INF_STORED_LEN;
			for (unsigned i = 0; i < len; ++i) {
				if (!B.take(8, v)) return INF_TRUNCATED;
				const int st = out.literal(v);
				if (st) return st;
			}
		} else if (type == 1u) {
			int s = 0;
			for (; s < 144; ++s) lengths[s] = 8;
			for (; s < 256; ++s) lengths[s] = 9;
			for (; s < 280; ++s) lengths[s] = 7;
			for (; s < INF_FIXLCODES; ++s) lengths[s] = 8;
			(void)inflate_construct(lencode, lengths, INF_FIXLCODES);
			for (s = 0; s < 32; ++s) lengths[s] = 5;         // (30 and 31 decode and name no distance: INF_SYMBOL)
			(void)inflate_construct(distcode, lengths, 32);
			const int st = inflate_codes(B, out, lencode, distcode);
			if (st) return st;
		} else if (type == 2u) {
			unsigned nlen, ndist, ncode;
			if (!B.take(5, nlen) || !B.take(5, ndist) || !B.take(4, ncode)) return INF_TRUNCATED;
			nlen += 257u; ndist += 1u; ncode += 4u;
			if (nlen > (unsigned)INF_MAXLCODES || ndist > (unsigned)INF_MAXDCODES) return INF_CODE_COUNTS;
			const unsigned char order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
			unsigned i = 0;
			for (; i < ncode; ++i) { if (!B.take(3, v)) return INF_TRUNCATED; lengths[order[i]] = (unsigned short)v; }
			for (; i < 19u; ++i) lengths[order[i]] = 0;
			int st = inflate_construct(lencode, lengths, 19);
			if (st) return st;                               // the code length code must be complete
			unsigned idx = 0;
			while (idx < nlen + ndist) {
				unsigned sym;
				if ((st = inflate_decode(B, lencode, sym))) return st;
				if (sym < 16u) lengths[idx++] = (unsigned short)sym;
				else {
					unsigned prev = 0, rep;
					if (sym == 16u) {
						if (idx == 0) return INF_CODE_COUNTS;
						prev = lengths[idx - 1];
						if (!B.take(2, v)) return INF_TRUNCATED;
						rep = 3u + v;
					} else if (sym == 17u) { if (!B.take(3, v)) return INF_TRUNCATED; rep = 3u + v; }
					else { if (!B.take(7, v)) return INF_TRUNCATED; rep = 11u + v; }
					if (idx + rep > nlen + ndist) return INF_CODE_COUNTS;
					while (rep--) lengths[idx++] = (unsigned short)prev;
				}
			}
			if (lengths[256] == 0) return INF_SYMBOL;        // no end-of-block code
			st = inflate_construct(lencode, lengths, (int)nlen);
			if (st == INF_CODE_OVER || (st == INF_CODE_INCOMPLETE && !inflate_single_bit_code(lencode))) return st;
			st = inflate_construct(distcode, lengths + nlen, (int)ndist);
			if (st == INF_CODE_OVER || (st == INF_CODE_INCOMPLETE && !inflate_single_bit_code(distcode))) return st;
			if ((st = inflate_codes(B, out, lencode, distcode))) return st;
		} else return INF_BLOCK_TYPE;
	} while (!last);
	return INF_OK;
}

// One BGZF block's deflate stream -- in_len bytes at `in` -- into exactly `isize` bytes at `out`.  Leaves neither range.
LSQ_HD inline int inflate_block(const unsigned char *in, size_t in_len, unsigned char *out, size_t isize) {
	InflateMemSource src{in, in_len, 0};
	InflateMemSink sink{out, isize, 0};
	unsigned short work[INF_WORK_SHORTS];
	const int st = inflate_stream(src, sink, work);
	if (st) return st;
	return sink.n == isize ? INF_OK : INF_OUTPUT_UNDER;
}

} // namespace lsq
