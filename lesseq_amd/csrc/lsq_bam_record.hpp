// The BAM_SINGLE record walk, shared by the host parser and the converter (lsq_bam.cpp) and by the device chain
// (lsq_bam_device.hpp): the one place where the binary record is taken apart.
//
// BAM_SINGLE is defined by its SAM equivalent: a BAM file means the SAM text `samtools view -h` prints for it -- the lines of the
// header text, then one line per alignment record in file order -- and that text means what lsq_sam_line.hpp says.  Of a record
// only FLAG, RNAME (the name of refID; "*" for -1), POS (pos + 1), MAPQ and CIGAR (the operations; "*" for none) matter.
// Record i (0-based) is the read "read-<h + i + 1>", h the number of lines of the header text (a last line without '\n' counts).
//
// The inflated stream: "BAM\1", l_text, the text, n_ref, per reference (l_name, name with its NUL, l_ref); then records:
//   block_size | refID pos l_read_name mapq bin n_cigar_op flag l_seq next_refID next_pos tlen (32 bytes) | read_name | cigar | ...
// A record, in this order:
//   runs past the end of the stream, block_size < 32, l_read_name == 0,
//   fixed part + name + CIGAR beyond block_size, refID >= n_ref or < -1,
//   a CIGAR operation code above 8                     malformed (structure: nothing else of the record is believed)
//   FLAG & skip_flags, MAPQ < min_mapq                 no read
//   POS outside 0 .. 2^31-1                            malformed (the text "-5" or "2147483648" is no POS)
//   no CIGAR operation ("*")                           no read
//   RNAME "*", POS 0, an RNAME MRF cannot write        no read
//   the walk of lsq_sam_line.hpp (SamBlockWalk, the code the text splitter runs); a reference end beyond 2^31-1   malformed
// A CIGAR of more than 65 535 operations lies in the CG tag and the record holds "<l_seq>S<ref_len>N" in its place: it is read as
// stored, and a soft clip and a skip make no read.
#pragma once
#include "lsq_sam_line.hpp"

namespace lsq {

LSQ_HD inline uint32_t bam_le32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
LSQ_HD inline uint32_t bam_le16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// Where the record behind the one at byte p of a stream of `len` bytes starts (never beyond len, always beyond p): what the
// record-start passes chase.  A record whose block_size field or body runs past the end is the stream's last.
LSQ_HD inline uint64_t bam_next_record(const unsigned char *s, uint64_t len, uint64_t p) {
	if (len - p < 4u) return len;
	const uint64_t nx = p + 4u + (uint64_t)bam_le32(s + p);
	return nx > len ? len : nx;
}

// One record: `r` points at its block_size field, `avail` bytes of the stream lie from there on.  ref_walks(refID) says
// whether the reference's name can be an MRF chromosome (not "*", no ':' or ',', no leading '#').  Calls
// on_block(refID, minus, start, end, qstart, qend) for every block, in order (1-based inclusive).  Verdicts, and mate_strand, as sam_split_fields.
template <class RefWalks, class OnBlock>
LSQ_HD inline int bam_split_record(const unsigned char *r, uint64_t avail, int64_t n_ref, unsigned skip_flags, unsigned min_mapq, RefWalks &&ref_walks, OnBlock &&on_block, const bool mate_strand = false) {
	if (avail < 4u) return SAM_MALFORMED;
	const uint64_t block_size = bam_le32(r);
	if (block_size > avail - 4u || block_size < 32u) return SAM_MALFORMED;
	const unsigned char *f = r + 4;
	const int64_t ref_id = (int32_t)bam_le32(f), pos0 = (int32_t)bam_le32(f + 4);
	const unsigned l_read_name = f[8], mapq = f[9], n_cigar = bam_le16(f + 12), flag = bam_le16(f + 14);
	if (l_read_name == 0u) return SAM_MALFORMED;
	if (32u + (uint64_t)l_read_name + 4u * (uint64_t)n_cigar > block_size) return SAM_MALFORMED;
	if (ref_id >= n_ref || ref_id < -1) return SAM_MALFORMED;
	const unsigned char *cigar = f + 32 + l_read_name;
	for (unsigned k = 0; k < n_cigar; ++k) if ((cigar[4u * k] & 15u) > 8u) return SAM_MALFORMED;
	if ((flag & skip_flags) != 0u) return SAM_NO_READ;
	if (mapq < min_mapq) return SAM_NO_READ;
	const int64_t pos = pos0 + 1;
	if (pos < 0 || pos > SAM_POS_MAX) return SAM_MALFORMED;
	if (n_cigar == 0u) return SAM_NO_READ;
	if (ref_id < 0 || pos == 0 || !ref_walks(ref_id)) return SAM_NO_READ;
	const bool minus = ((flag & 0x10u) != 0u) != (mate_strand && sam_flag_mate2(flag));
	auto emit = [&](int64_t s, int64_t e, int64_t qs, int64_t qe) { on_block(ref_id, minus, s, e, qs, qe); };
	SamBlockWalk W;
	W.begin(pos);
	for (unsigned k = 0; k < n_cigar; ++k) {
		const uint32_t v = bam_le32(cigar + 4u * k);
		const char ops[9] = {'M', 'I', 'D', 'N', 'S', 'H', 'P', '=', 'X'};
		if (!W.step(ops[v & 15u], (int64_t)(v >> 4), emit)) return SAM_MALFORMED;
	}
	W.end(emit);
	return W.n_blocks ? SAM_READ : SAM_NO_READ;
}

// can this reference name be an MRF chromosome (the rule of lsq_sam_line.hpp)
LSQ_HD inline bool bam_ref_name_walks(const char *p, size_t n) {
	if (n == 1 && p[0] == '*') return false;
	if (n >= 1 && p[0] == '#') return false;
	for (size_t j = 0; j < n; ++j) if (p[j] == ':' || p[j] == ',') return false;
	return true;
}

} // namespace lsq
