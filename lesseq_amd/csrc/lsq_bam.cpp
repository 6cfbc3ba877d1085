// BAM_SINGLE on the host: the parser (lsq_bam_parse: the arrays lsq_sam_parse fills for the equivalent SAM text) and the
// converter to the equivalent MRF_SINGLE text (lsq_bam_to_mrf, the bam2mrf executable).  The rules live in lsq_bam_record.hpp
// and lsq_sam_line.hpp, the decoder in lsq_inflate.hpp, the file's structure in lsq_bam.hpp.  No GPU touched, no zlib.
// The _checked entries verify every block's CRC32 and the end-of-file marker (lsq_crc32.hpp) on the way; lsq_bam_check_host is
// the whole-file check without an annotation (the bamcheck executable with --host).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lsq_bam.hpp"
#include "lsq_gtf.hpp"
#include "lsq_internal.hpp"

using namespace lsq;

namespace lsq {

int bam_fail(const BamError &e) { return fail(e.status, "%s", e.text.c_str()); }      // (declared in lsq_internal.hpp: the device chain reports through it too)

// the MRF text that defines what the BAM file means: "AlignmentBlocks", '#' per header line, a line per record
int bam_to_mrf(const char *bytes, size_t len, unsigned skip_flags, unsigned min_mapq, std::string &o, bool verify, int library) {
	BamStream S;
	BamError e;
	if (bam_open((const unsigned char *)bytes, len, host_threads(0), S, e, verify)) return bam_fail(e);
	o = "AlignmentBlocks\n";
	for (uint64_t k = 0; k < S.H.h_lines; ++k) o += "#\n";
	size_t keep = o.size();
	auto put = [&](int64_t v) { char b[24]; o.append(b, (size_t)snprintf(b, sizeof b, "%lld", (long long)v)); };
	const int st = bam_for_each_record(S, skip_flags, min_mapq, [&](int64_t ref, bool minus, int64_t bs, int64_t be, int64_t qs, int64_t qe) {
		if (o.size() > keep) o += ',';
		o += S.H.ref_names[(size_t)ref];
		o += (minus != (library == LSQ_LIBRARY_REVERSE)) ? ":-:" : ":+:";      // (a library given: the transcript strand)
		put(bs); o += ':'; put(be); o += ':'; put(qs); o += ':'; put(qe);
	}, [&](uint64_t, int v) {
		if (v != SAM_READ) { o.resize(keep); o += '#'; }
		o += '\n';
		keep = o.size();
		return BAM_OK;
	}, e, library != LSQ_LIBRARY_UNSTRANDED);
	return st ? bam_fail(e) : LSQ_OK;
}

// a file's bytes, a file that does not open named as the parsers name it
static int bam_read_file(const char *path, std::string &bytes) {
	FILE *f = fopen(path, "rb");
	if (!f) return fail(LSQ_E_IO, "cannot open reads file %s", path);
	fclose(f);
	return read_all(path, bytes) ? LSQ_E_IO : LSQ_OK;
}

static int bam_parse_file(const char *path, lsq_events *E, unsigned skip_flags, unsigned min_mapq, int n_threads, bool verify, lsq_reads **out) {
	if (!path || !E || !out) return fail(LSQ_E_ARG, "null argument");
	std::string bytes;
	if (const int rc = bam_read_file(path, bytes)) return rc;
	BamStream S;
	BamError e;
	if (bam_open((const unsigned char *)bytes.data(), bytes.size(), host_threads(n_threads), S, e, verify)) return bam_fail(e);
	std::string().swap(bytes);
	// chromosome ids: only names the events know can ever pass the containment filter (as lsq_mrf.cpp's parse_chunk)
	const uint16_t NOCHROM = 0xFFFF;
	std::vector<uint16_t> ref_chrom(S.H.ref_names.size(), NOCHROM);
	for (size_t r = 0; r < ref_chrom.size(); ++r) {
		const int id = E->chroms.find(S.H.ref_names[r]);
		if (id >= 0 && (size_t)id < E->n_table_chroms()) ref_chrom[r] = (uint16_t)id;
	}
	int strand_id[2] = {-1, -1};
	const int64_t LIM = (int64_t)1 << 30;
	std::unique_ptr<lsq_reads> R(new lsq_reads);
	R->o_blk_off.push_back(0);
	size_t keep = 0;
	int range = LSQ_OK;
	const int st = bam_for_each_record(S, skip_flags, min_mapq, [&](int64_t ref, bool minus, int64_t start, int64_t end, int64_t, int64_t) {
		int &sid = strand_id[minus ? 1 : 0];
		if (sid < 0) { sid = E->strands.intern(minus ? "-" : "+"); if (sid > 255) { range = LSQ_E_RANGE; sid = 0; } }
		int64_t s0 = start - 1;
		uint16_t cid = ref_chrom[(size_t)ref];
		if (s0 >= LIM || end >= LIM) { cid = NOCHROM; s0 = 0; end = 0; }
		R->o_start.push_back((int32_t)s0); R->o_end.push_back((int32_t)end); R->o_chrom.push_back(cid); R->o_strand.push_back((uint8_t)sid);
	}, [&](uint64_t line_no, int v) {
		if (range) { e.status = range; e.text = "more than 256 distinct strand strings"; return range; }
		if (v != SAM_READ) { R->o_start.resize(keep); R->o_end.resize(keep); R->o_chrom.resize(keep); R->o_strand.resize(keep); return (int)BAM_OK; }
		if (line_no > 0xFFFFFFFFull) { e.status = LSQ_E_RANGE; e.text = "more than 2^32 lines"; return e.status; }
		keep = R->o_start.size();
		R->o_blk_off.push_back(keep);
		R->o_line_no.push_back((uint32_t)line_no);
		return (int)BAM_OK;
	}, e, E->stranded());       // (stranded events: the strand of the fragment's first mate, as lsq_sam_parse writes it)
	if (st) return bam_fail(e);
	R->adopt();
	*out = R.release();
	return LSQ_OK;
}

static int bam_to_mrf_text(const void *bam_bytes, uint64_t len, unsigned skip_flags, unsigned min_mapq, bool verify, char **mrf_text, uint64_t *mrf_len) {
	if ((!bam_bytes && len) || !mrf_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	const int st = bam_to_mrf((const char *)bam_bytes, (size_t)len, skip_flags, min_mapq, o, verify);
	if (st) return st;
	char *p = (char *)malloc(o.size() + 1);
	if (!p) return fail(LSQ_E_INTERNAL, "out of memory");
	memcpy(p, o.data(), o.size());
	p[o.size()] = 0;
	*mrf_text = p;
	if (mrf_len) *mrf_len = o.size();
	return LSQ_OK;
}

} // namespace lsq

extern "C" {

int lsq_bam_parse(const char *path, lsq_events *E, unsigned skip_flags, unsigned min_mapq, int n_threads, lsq_reads **out) LSQ_API_TRY {
	return bam_parse_file(path, E, skip_flags, min_mapq, n_threads, false, out);
} LSQ_API_CATCH
int lsq_bam_parse_checked(const char *path, lsq_events *E, unsigned skip_flags, unsigned min_mapq, int n_threads, lsq_reads **out) LSQ_API_TRY {
	return bam_parse_file(path, E, skip_flags, min_mapq, n_threads, true, out);
} LSQ_API_CATCH

int lsq_bam_to_mrf(const void *bam_bytes, uint64_t len, unsigned skip_flags, unsigned min_mapq, char **mrf_text, uint64_t *mrf_len) LSQ_API_TRY {
	return bam_to_mrf_text(bam_bytes, len, skip_flags, min_mapq, false, mrf_text, mrf_len);
} LSQ_API_CATCH
int lsq_bam_to_mrf_checked(const void *bam_bytes, uint64_t len, unsigned skip_flags, unsigned min_mapq, char **mrf_text, uint64_t *mrf_len) LSQ_API_TRY {
	return bam_to_mrf_text(bam_bytes, len, skip_flags, min_mapq, true, mrf_text, mrf_len);
} LSQ_API_CATCH

int lsq_bam_check_host(const char *path, int n_threads, lsq_bam_report *r) LSQ_API_TRY {
	if (!path || !r) return fail(LSQ_E_ARG, "null argument");
	std::string bytes;
	if (const int rc = bam_read_file(path, bytes)) return rc;
	BamStream S;
	BamError e;
	if (bam_open((const unsigned char *)bytes.data(), bytes.size(), host_threads(n_threads), S, e, true)) return bam_fail(e);
	lsq_bam_report R{};
	R.file_bytes = bytes.size(); R.blocks = S.n_blocks; R.inflated_bytes = S.bytes.size();
	R.header_lines = S.H.h_lines; R.references = S.H.ref_names.size();
	uint64_t nb = 0;
	const int st = bam_for_each_record(S, SAM_DEFAULT_SKIP_FLAGS, SAM_DEFAULT_MIN_MAPQ, [&](int64_t, bool, int64_t, int64_t, int64_t, int64_t) { ++nb; },
	                                   [&](uint64_t, int v) { ++R.records; if (v == SAM_READ) { ++R.reads; R.read_blocks += nb; } nb = 0; return (int)BAM_OK; }, e);
	if (st) return bam_fail(e);
	*r = R;
	return LSQ_OK;
} LSQ_API_CATCH

} // extern "C"
