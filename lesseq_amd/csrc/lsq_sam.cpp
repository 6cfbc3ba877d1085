// SAM_SINGLE on the host: the converter to the equivalent MRF_SINGLE text (lsq_sam_to_mrf, the sam2mrf executable).
// The rules live in lsq_sam_line.hpp; the host parser (lsq_sam_parse) shares lsq_mrf.cpp's driver.  No GPU touched.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lsq_gtf.hpp"
#include "lsq_internal.hpp"
#include "lsq_sam_line.hpp"

using namespace lsq;

namespace {

void put_i64(std::string &o, int64_t v) {
	char b[24];
	const int n = snprintf(b, sizeof b, "%lld", (long long)v);
	o.append(b, (size_t)n);
}

int sam_to_mrf(const char *s, size_t len, unsigned skip_flags, unsigned min_mapq, std::string &o, int library = LSQ_LIBRARY_UNSTRANDED) {
	o = "AlignmentBlocks\n";
	uint64_t no = 0;
	for (size_t p = 0; p < len;) {
		const char *nl = (const char *)memchr(s + p, '\n', len - p);
		if (!nl) break;                    // a last line without '\n' is never seen
		const MrfView line{s + p, (size_t)(nl - (s + p))};
		p += line.n + 1;
		++no;
		const size_t keep = o.size();
		const int v = sam_split_line(line, skip_flags, min_mapq, [&](MrfView rname, bool minus, int64_t bs, int64_t be, int64_t qs, int64_t qe) {
			if (o.size() > keep) o += ',';
			o.append(rname.p, rname.n);
			o += (minus != (library == LSQ_LIBRARY_REVERSE)) ? ":-:" : ":+:";      // (a library given: the transcript strand)
			put_i64(o, bs); o += ':'; put_i64(o, be); o += ':'; put_i64(o, qs); o += ':'; put_i64(o, qe);
		}, library != LSQ_LIBRARY_UNSTRANDED);
		if (v == SAM_MALFORMED) return fail(LSQ_E_PARSE, "#%llu:%.*s", (unsigned long long)no, (int)std::min<size_t>(line.n, 1u << 20), line.p);
		if (v != SAM_READ) { o.resize(keep); o += '#'; }
		o += '\n';
	}
	return LSQ_OK;
}

bool cast_u32(const char *s, unsigned &out) {
	char *end = nullptr;
	errno = 0;
	const unsigned long v = strtoul(s, &end, 0);
	if (errno || end == s || *end || v > 0xFFFFFFFFul || *s == '-') return false;
	out = (unsigned)v;
	return true;
}

} // namespace

namespace lsq {

// sam2mrf [--skip-flags N] [--min-mapq N] [--library forward|reverse] [file]: SAM from standard input (or the file) to the equivalent MRF on standard
// output.  Exit status 0; 1 for a malformed line ("#<k>:<line>" and the lexical-cast line on standard error) or a file
// that does not open; nothing on standard output then.  bam2mrf: the same for a BAM file (lsq_bam.cpp); a file that is no
// BAM file is exit status 1 with its message alone; bam2mrf --verify also checks every block's CRC32 and the end-of-file marker.
// --library: the strand column holds the record's transcript strand in that library, not its alignment strand -- the MRF
// file whose forward-library job is the SAM file's job in the library named.
int run_sam2mrf(bool bam, int argc, const char *const *argv, std::string &out) {
	unsigned skip_flags = SAM_DEFAULT_SKIP_FLAGS, min_mapq = SAM_DEFAULT_MIN_MAPQ;
	const char *path = nullptr;
	bool bad = false, verify = false;
	int library = LSQ_LIBRARY_UNSTRANDED;
	for (int i = 1; i < argc && !bad; ++i) {
		if (bam && strcmp(argv[i], "--verify") == 0) verify = true;
		else if (strcmp(argv[i], "--skip-flags") == 0 && i + 1 < argc) bad = !cast_u32(argv[++i], skip_flags);
		else if (strcmp(argv[i], "--min-mapq") == 0 && i + 1 < argc) bad = !cast_u32(argv[++i], min_mapq);
		else if (strcmp(argv[i], "--library") == 0 && i + 1 < argc) { library = lsq_library_from_name(argv[++i]); bad = library != LSQ_LIBRARY_FORWARD && library != LSQ_LIBRARY_REVERSE; }
		else if (argv[i][0] == '-' && argv[i][1] == '-') bad = true;
		else if (!path) path = argv[i];
		else bad = true;
	}
	if (bad) { cli_log(0, bam ? "Usage:\nbam2mrf [--verify] [--skip-flags N] [--min-mapq N] [--library forward|reverse] [bam_path]      (standard input without a path)" : "Usage:\nsam2mrf [--skip-flags N] [--min-mapq N] [--library forward|reverse] [sam_path]      (standard input without a path)"); return 1; }
	std::string bytes;
	if (read_all(path, bytes)) { cli_log(0, lsq_last_error()); return 1; }
	const int st = bam ? bam_to_mrf(bytes.data(), bytes.size(), skip_flags, min_mapq, out, verify, library) : sam_to_mrf(bytes.data(), bytes.size(), skip_flags, min_mapq, out, library);
	if (st) { out.clear(); cli_log(0, lsq_last_error()); if (st == LSQ_E_PARSE) cli_log(0, LEXICAL_CAST_ERROR); return 1; }
	return 0;
}

} // namespace lsq

extern "C" {

int lsq_sam_to_mrf(const void *sam_bytes, uint64_t len, unsigned skip_flags, unsigned min_mapq, char **mrf_text, uint64_t *mrf_len) LSQ_API_TRY {
	if ((!sam_bytes && len) || !mrf_text) return fail(LSQ_E_ARG, "null argument");
	std::string o;
	const int st = sam_to_mrf((const char *)sam_bytes, (size_t)len, skip_flags, min_mapq, o);
	if (st) return st;
	char *p = (char *)malloc(o.size() + 1);
	if (!p) return fail(LSQ_E_INTERNAL, "out of memory");
	memcpy(p, o.data(), o.size());
	p[o.size()] = 0;
	*mrf_text = p;
	if (mrf_len) *mrf_len = o.size();
	return LSQ_OK;
} LSQ_API_CATCH

} // extern "C"
