// The SAM_SINGLE line splitter, shared by the host parser and the converter (lsq_sam.cpp) and by the device
// parser (lsq_sam_device.hpp): the one place where the rules of the format are written.
//
// SAM_SINGLE is defined by its MRF equivalent: the file "AlignmentBlocks\n" followed by one line per SAM line that
// ends in '\n' -- '#' for a line that makes no read, the blocks "RNAME:<strand>:<s>:<e>:<qs>:<qe>" joined by ','
// otherwise.  SAM line k (1-based, every line counted) is therefore the read "read-<k>".  Every alignment record is
// a read of its own; mates are not paired.
//
// A line, in this order:
//   begins with '@'                                   no read
//   fewer than six TAB-separated fields               malformed
//   FLAG not [0-9]+ or above 65535                    malformed
//   MAPQ not [0-9]+ or above 255                      malformed
//   FLAG & skip_flags, MAPQ < min_mapq                no read
//   POS not [0-9]+ or above 2^31-1                    malformed
//   CIGAR neither "*" nor ([0-9]+[MIDNSHP=X])+ with
//     every length <= 2^31-1                          malformed
//   RNAME "*", POS 0, CIGAR "*"                       no read
//   RNAME holds ':' or ',' or begins with '#'         no read (such a name cannot be written in MRF -- the line would split
//                                                     elsewhere, or be a comment -- and names no chromosome an MRF run could match)
//   the walk below; a reference end beyond 2^31-1     malformed
//   no block                                          no read
// The walk starts at reference position POS and query position 1 (both 1-based) with an empty open block.  M = X
// extend the open block on reference and query, D on the reference only; N closes the open block and advances the
// reference; I S advance the query; H P do nothing.  A block is delivered when N or the end of the CIGAR closes it
// and only if it covers at least one reference base.  Its query interval runs from the query position at its first
// reference base to the last query base consumed inside it (never read by count or solve).
//
// The splitter is a template over the view of the line, as lsq_mrf_line.hpp is: plain memory with size_t positions
// on the host and in the device's fall-back kernel, an LDS pointer with 32-bit positions in the tile kernel.  Nothing
// behind the CIGAR field is ever looked at, so a view may end anywhere at or behind the CIGAR's last byte.
#pragma once
#include "lsq_mrf_line.hpp"

namespace lsq {

constexpr unsigned SAM_DEFAULT_SKIP_FLAGS = 0x904u;     // unmapped, secondary, supplementary
constexpr unsigned SAM_DEFAULT_MIN_MAPQ = 0u;
constexpr int64_t SAM_POS_MAX = 2147483647ll;           // 2^31 - 1

enum SamVerdict { SAM_NO_READ = 0, SAM_READ = 1, SAM_MALFORMED = 2 };

// [0-9]+ with a value of at most `limit` (<= 2^31-1); any number of leading zeros
template <class V>
LSQ_HD inline bool sam_cast_unsigned(V f, int64_t limit, int64_t &out) {
	typedef typename V::index_type Idx;
	if (f.n == 0) return false;
	int64_t v = 0;
	for (Idx j = 0; j < f.n; ++j) {
		const unsigned d = (unsigned)(unsigned char)f.p[j] - (unsigned)'0';
		if (d > 9) return false;
		v = v * 10 + (int64_t)d;
		if (v > limit) return false;
	}
	out = v;
	return true;
}

enum SamBounds { SAM_BOUNDS_OK = 0, SAM_BOUNDS_SHORT_LINE = 1, SAM_BOUNDS_SHORT_VIEW = 2 };

// The first six TAB-separated fields of a line -- QNAME FLAG RNAME POS MAPQ CIGAR -- in one walk over its bytes: field k is
// [b[k], b[k + 1] - 1).  `whole` says that the view runs to the line's end; a view that is cut short (the device's tile
// kernel sees the head of a line only) must hold the sixth TAB.  SAM_BOUNDS_SHORT_LINE: a whole line of fewer than six fields.
template <class V>
LSQ_HD inline int sam_field_bounds(V l, bool whole, typename V::index_type *b) {
	typedef typename V::index_type Idx;
	unsigned k = 0;
	b[0] = 0;
	for (Idx i = 0; i < l.n; ++i)
		if (l.p[i] == '\t') {
			b[++k] = i + 1;
			if (k == 6u) return SAM_BOUNDS_OK;
		}
	if (!whole) return SAM_BOUNDS_SHORT_VIEW;
	if (k < 5u) return SAM_BOUNDS_SHORT_LINE;
	b[6] = l.n + 1;
	return SAM_BOUNDS_OK;
}

// The walk's block-emitting half, one CIGAR operation at a time: the text splitter below and the binary-record walk
// (lsq_bam_record.hpp) both feed it, so the rules above are written once.  emit(start, end, qstart, qend), 1-based inclusive.
struct SamBlockWalk {
	int64_t ref, bs, q, qs, qe;
	unsigned n_blocks;
	LSQ_HD inline void begin(int64_t pos) { ref = pos; bs = pos; q = 1; qs = 1; qe = 0; n_blocks = 0; }
	// op: one of MIDNSHP=X, len <= 2^31-1.  false: the reference end lies beyond 2^31-1
	template <class Emit>
	LSQ_HD inline bool step(const char op, const int64_t len, Emit &&emit) {
		if (op == 'M' || op == '=' || op == 'X' || op == 'D') {
			if (len > 0) {
				if (ref == bs) { qs = q; qe = q - 1; }
				ref += len;
				if (op != 'D') { q += len; qe = q - 1; }
			}
		} else if (op == 'N') {
			if (ref > bs) { emit(bs, ref - 1, qs, qe); ++n_blocks; }
			ref += len;
			bs = ref;
		} else if (op == 'I' || op == 'S') q += len;
		return ref - 1 <= SAM_POS_MAX;
	}
	template <class Emit>
	LSQ_HD inline void end(Emit &&emit) { if (ref > bs) { emit(bs, ref - 1, qs, qe); ++n_blocks; } }
};

// the record is the second mate of a pair: its fragment came from the strand opposite to the one it aligned to
LSQ_HD inline bool sam_flag_mate2(unsigned flag) { return (flag & 0x1u) != 0u && (flag & 0x80u) != 0u; }

// Calls on_block(rname, minus, start, end, qstart, qend) for every block of the record, in order (1-based inclusive).
// minus: FLAG & 0x10; with mate_strand set (stranded jobs), that XOR sam_flag_mate2 -- the strand the fragment's first mate lies on.
// SAM_MALFORMED may come after blocks have been delivered; SAM_READ only when at least one was.  `b`: sam_field_bounds
// of a line that does not begin with '@'.
template <class V, class OnBlock>
LSQ_HD inline int sam_split_fields(V line, const typename V::index_type *b, unsigned skip_flags, unsigned min_mapq, OnBlock &&on_block, const bool mate_strand = false) {
	typedef typename V::index_type Idx;
	auto field = [&](int k) { return V{line.p + b[k], (Idx)(b[k + 1] - 1 - b[k])}; };
	int64_t flag, mapq, pos;
	if (!sam_cast_unsigned(field(1), 65535, flag)) return SAM_MALFORMED;
	if (!sam_cast_unsigned(field(4), 255, mapq)) return SAM_MALFORMED;
	if (((unsigned)flag & skip_flags) != 0u) return SAM_NO_READ;
	if ((unsigned)mapq < min_mapq) return SAM_NO_READ;
	if (!sam_cast_unsigned(field(3), SAM_POS_MAX, pos)) return SAM_MALFORMED;
	const V rname = field(2), cigar = field(5);
	const bool no_cigar = cigar.n == 1 && cigar.p[0] == '*';
	bool walk = !(rname.n == 1 && rname.p[0] == '*') && pos != 0 && !no_cigar;
	if (rname.n >= 1 && rname.p[0] == '#') walk = false;
	for (Idx j = 0; walk && j < rname.n; ++j) if (rname.p[j] == ':' || rname.p[j] == ',') walk = false;
	if (no_cigar) return SAM_NO_READ;
	if (cigar.n == 0) return SAM_MALFORMED;
	const bool minus = (((unsigned)flag & 0x10u) != 0u) != (mate_strand && sam_flag_mate2((unsigned)flag));
	auto emit = [&](int64_t s, int64_t e, int64_t qs, int64_t qe) { on_block(rname, minus, s, e, qs, qe); };
	SamBlockWalk W;
	W.begin(pos);
	Idx j = 0;
	while (j < cigar.n) {
		Idx k = j;
		while (k < cigar.n && (unsigned)(unsigned char)cigar.p[k] - (unsigned)'0' <= 9u) ++k;
		int64_t len;
		if (k == cigar.n || !sam_cast_unsigned(V{cigar.p + j, (Idx)(k - j)}, SAM_POS_MAX, len)) return SAM_MALFORMED;
		const char op = cigar.p[k];
		j = k + 1;
		const bool on_ref = op == 'M' || op == '=' || op == 'X' || op == 'D';
		if (!on_ref && op != 'N' && op != 'I' && op != 'S' && op != 'H' && op != 'P') return SAM_MALFORMED;
		if (!walk) continue;
		if (!W.step(op, len, emit)) return SAM_MALFORMED;
	}
	if (walk) W.end(emit);
	return W.n_blocks ? SAM_READ : SAM_NO_READ;
}

// a whole line
template <class V, class OnBlock>
LSQ_HD inline int sam_split_line(V line, unsigned skip_flags, unsigned min_mapq, OnBlock &&on_block, const bool mate_strand = false) {
	typename V::index_type b[7];
	if (line.n >= 1 && line.p[0] == '@') return SAM_NO_READ;
	if (sam_field_bounds(line, true, b) != SAM_BOUNDS_OK) return SAM_MALFORMED;
	return sam_split_fields(line, b, skip_flags, min_mapq, on_block, mate_strand);
}

} // namespace lsq
