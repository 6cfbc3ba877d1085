// GTF annotation parsed on the device: what bin/parseGencode does per byte and per line (the host side --
// sorting the transcripts, formatting, the executables -- is lsq_gtf.cpp).  The text is staged in HBM and its newline tiles
// are counted by the text layer the read parsers use (lsq_text.hip: text_stage_buffer, scan_newlines).
//
//   lsq_gtf_lines_kernel   one workgroup per tile of the newline scan.  The tile and GTF_AHEAD bytes behind it go to LDS with
//                          16-byte loads; the tile's newlines are listed in order (lsq_text.hpp: TextTileNl), so
//                          that line j that STARTS in the tile has the number tile base + j.  A wave takes a line: the 64
//                          lanes look at 64 bytes at a time and ballots find the TABs, the end of the line, the first
//                          "gene_id" / "transcript_id", the ';' around it and the quotes inside -- every branch is the same
//                          for all lanes of a wave, kept and ignored lines never share one.  Bytes outside the LDS window
//                          (a line that runs on past it: any length) come from HBM through the same accessor.  Lane 0
//                          writes the line's record to its slot of a dense array, a flag for kept (`exon`) lines, and
//                          lowers the error word for a bad line.
//   device_scan            over the flags: every kept line's place in file order
//   lsq_gtf_compact_kernel the kept records to their places, (start, end) pairs beside them
//   lsq_gtf_heads_kernel   a lane per kept line: 1 where (gene id, transcript id) differs bytewise from the kept line before
//   device_scan + lsq_gtf_emit_heads_kernel   the run heads, compacted
// Only the run heads (one per transcript, more where a transcript's lines are scattered), the (start, end) pairs and three
// words of status come back; the text does not.
#include "lsq_text.hpp"
#include "lsq_gtf.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace lsq;

namespace {

constexpr unsigned GTF_AHEAD = 2560;            // bytes behind the tile that are staged with it: lines that start in the tile end here, mostly
static_assert(TEXT_TILE % 16u == 0 && GTF_AHEAD % 16u == 0, "the window is staged in 16-byte words");
constexpr unsigned long long GTF_NONE = ~0ull;

struct GtfLds {
	__align__(16) unsigned char text[TEXT_TILE + GTF_AHEAD];
	TextNlLds nl;
};

// the text as a wave reads it: LDS inside the window [w0, w1), HBM elsewhere
struct GtfView {
	const unsigned char *text;
	const unsigned char *lds;
	unsigned long long len, w0, w1;
	__device__ unsigned char at(unsigned long long i) const { return i >= w0 && i < w1 ? lds[i - w0] : text[i]; }
};

__device__ inline unsigned gtf_lane() { return threadIdx.x & 63u; }
__device__ inline unsigned gtf_ctz(unsigned long long m) { return (unsigned)__ffsll((long long)m) - 1u; }

// first position in [from, to) that holds ch, or `to`.  to <= len.
__device__ inline unsigned long long gtf_find_first(const GtfView &V, unsigned char ch, unsigned long long from, unsigned long long to) {
	for (unsigned long long B = from & ~63ull; B < to; B += 64) {
		const unsigned long long i = B + gtf_lane();
		const unsigned long long m = __ballot(i >= from && i < to && V.at(i) == ch);
		if (m) return B + gtf_ctz(m);
	}
	return to;
}
// last position in [from, to) that holds ch, or GTF_NONE
__device__ inline unsigned long long gtf_find_last(const GtfView &V, unsigned char ch, unsigned long long from, unsigned long long to) {
	if (to <= from) return GTF_NONE;
	for (unsigned long long B = (to - 1) & ~63ull;; B -= 64) {
		const unsigned long long i = B + gtf_lane();
		const unsigned long long m = __ballot(i >= from && i < to && V.at(i) == ch);
		if (m) return B + 63u - (unsigned)__clzll((long long)m);
		if (B <= from) break;             // (B is a multiple of 64: B < 64 implies B == 0 <= from)
	}
	return GTF_NONE;
}
// first position p in [from, to - n] with the n bytes of `key` at p, or GTF_NONE (strstr inside the field)
template <unsigned N>
__device__ inline unsigned long long gtf_find_key(const GtfView &V, const char (&key)[N], unsigned long long from, unsigned long long to) {
	constexpr unsigned n = N - 1;
	if (to < from + n) return GTF_NONE;
	const unsigned long long last = to - n;
	for (unsigned long long B = from & ~63ull; B <= last; B += 64) {
		const unsigned long long i = B + gtf_lane();
		bool hit = i >= from && i <= last && V.at(i) == (unsigned char)key[0];
		if (hit) {
			for (unsigned q = 1; q < n; ++q) if (V.at(i + q) != (unsigned char)key[q]) { hit = false; break; }
		}
		const unsigned long long m = __ballot(hit);
		if (m) return B + gtf_ctz(m);
	}
	return GTF_NONE;
}

// C's atoi on the bytes [a, b) (a field: it holds no TAB and no newline): blanks, a sign, digits; strtol's saturation at
// the ends of a 64-bit long, then the low 32 bits.  Every lane walks the same bytes.
__device__ inline int gtf_atoi(const GtfView &V, unsigned long long a, unsigned long long b) {
	while (a < b) { const unsigned char c = V.at(a); if (c == ' ' || (c >= 9 && c <= 13)) ++a; else break; }
	bool neg = false;
	if (a < b) { const unsigned char c = V.at(a); if (c == '-' || c == '+') { neg = c == '-'; ++a; } }
	const unsigned long long limit = neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull;
	unsigned long long acc = 0;
	bool sat = false;
	for (; a < b; ++a) {
		const unsigned d = (unsigned)V.at(a) - '0';
		if (d > 9u) break;
		if (sat || acc > (limit - d) / 10ull) { sat = true; acc = limit; }
		else acc = acc * 10ull + d;
	}
	return (int)(unsigned)(neg ? 0ull - acc : acc);
}

// An attribute of field 9 [fs, fe) as the reference takes it: the field is cut at every ';' (quotes do not protect one);
// the first piece that holds `key` anywhere is the item; its value runs from behind the item's first '"' to its last '"'
// (to the item's end when there is one quote only).  Returns 0, or 1 = no such item, 2 = the item holds no '"' (then
// [v0, v1) is the item).
template <unsigned N>
__device__ inline int gtf_attribute(const GtfView &V, const char (&key)[N], unsigned long long fs, unsigned long long fe, unsigned long long &v0, unsigned long long &v1) {
	const unsigned long long m = gtf_find_key(V, key, fs, fe);
	if (m == GTF_NONE) return 1;
	const unsigned long long before = gtf_find_last(V, ';', fs, m);
	const unsigned long long i0 = before == GTF_NONE ? fs : before + 1, i1 = gtf_find_first(V, ';', m, fe);
	const unsigned long long q0 = gtf_find_first(V, '"', i0, i1);
	if (q0 == i1) { v0 = i0; v1 = i1; return 2; }
	const unsigned long long q1 = gtf_find_last(V, '"', q0 + 1, i1);
	v0 = q0 + 1; v1 = q1 == GTF_NONE ? i1 : q1;
	return 0;
}

struct GtfStatus { unsigned long long err, skipped; };

__device__ inline void gtf_line(const GtfView &V, unsigned long long s, unsigned long long idx, GtfRec *rec, unsigned *keep, GtfStatus *status) {
	const unsigned lane = gtf_lane();
	const unsigned long long len = V.len;
	// the first nine TABs and the end of the line (a newline, or the end of the text)
	unsigned long long tab[9], e = GTF_NONE;
	unsigned ntab = 0;
	if (V.at(s) == '#') { if (lane == 0) atomicAdd(&status->skipped, 1ull); return; }
	for (unsigned long long B = s & ~63ull;; B += 64) {
		const unsigned long long i = B + lane;
		const unsigned char c = i < len ? V.at(i) : (unsigned char)'\n';
		const unsigned long long mnl = __ballot(i >= s && c == '\n');
		unsigned long long mtab = __ballot(i >= s && c == '\t');
		if (mnl) mtab &= (1ull << gtf_ctz(mnl)) - 1ull;
#pragma unroll
		for (unsigned k = 0; k < 9; ++k)
			if (ntab == k && mtab) { tab[k] = B + gtf_ctz(mtab); mtab &= mtab - 1ull; ++ntab; }
		if (mnl) { e = B + gtf_ctz(mnl); break; }
		if (ntab == 9) break;
	}
	// "\r\n" ends a line as "\n" does; a '\r' at the very end of the text stays
	if (e != GTF_NONE && e < len && e > s && V.at(e - 1) == '\r') --e;
	if (e == s) { if (lane == 0) atomicAdd(&status->skipped, 1ull); return; }
	if (ntab < 8) { if (lane == 0) atomicMin(&status->err, idx << 8 | (unsigned long long)GTF_E_SHORT); return; }
	const unsigned long long fs = tab[7] + 1, fe = ntab == 9 ? tab[8] : e;
	unsigned long long g0 = 0, g1 = 0, t0 = 0, t1 = 0;
	int bad = 0;
	const int ga = gtf_attribute(V, "gene_id", fs, fe, g0, g1);
	if (ga) bad = ga == 1 ? GTF_E_NO_GENE : GTF_E_UNQUOTED_GENE;
	else {
		const int ta = gtf_attribute(V, "transcript_id", fs, fe, t0, t1);
		if (ta) { bad = ta == 1 ? GTF_E_NO_TX : GTF_E_UNQUOTED_TX; g0 = t0; g1 = t1; }
	}
	const bool exon = tab[2] - tab[1] == 5 && V.at(tab[1] + 1) == 'e' && V.at(tab[1] + 2) == 'x' && V.at(tab[1] + 3) == 'o' && V.at(tab[1] + 4) == 'n';
	if (bad == 0 && !exon) return;
	GtfRec r;
	r.line_off = s; r.line_no = (unsigned)(idx + 1); r.chrom_len = (unsigned)(tab[0] - s);
	r.strand_off = (unsigned)(tab[5] + 1 - s); r.strand_len = (unsigned)(tab[6] - tab[5] - 1);
	r.gene_off = (unsigned)(g0 - s); r.gene_len = (unsigned)(g1 - g0);
	r.tx_off = (unsigned)(t0 - s); r.tx_len = (unsigned)(t1 - t0);
	r.start = 0; r.end = 0; r.aux = 0; r.pad = 0;
	if (bad == 0) {
		r.start = (int)((unsigned)gtf_atoi(V, tab[2] + 1, tab[3]) - 1u);
		r.end = gtf_atoi(V, tab[3] + 1, tab[4]);
	}
	if (lane == 0) {
		rec[idx] = r;
		if (bad) atomicMin(&status->err, idx << 8 | (unsigned long long)bad);
		else keep[idx] = 1u;
	}
}

__global__ void __launch_bounds__(256) lsq_gtf_lines_kernel(const unsigned char *text, unsigned long long len, const unsigned long long *tile_base,
                                                            GtfRec *rec, unsigned *keep, GtfStatus *status) {
	__shared__ GtfLds L;
	const unsigned long long t0 = (unsigned long long)blockIdx.x * TEXT_TILE;
	// the window: the tile, its newlines found on the way, and GTF_AHEAD bytes behind it, 16 bytes a lane and round (the buffer
	// holds 16 bytes of slack behind the text; t0 is a multiple of 16)
	const unsigned long long w1 = min(len, t0 + TEXT_TILE + GTF_AHEAD);
	TextTileNl N;
	N.load(L.text, text, len, t0);
	for (unsigned off = TEXT_TILE + threadIdx.x * 16u; t0 + off < w1; off += 256u * 16u)
		*reinterpret_cast<uint4 *>(L.text + off) = *reinterpret_cast<const uint4 *>(text + t0 + off);
	N.number(L.nl);                                  // (its barriers also publish L.text)
	const GtfView V{text, L.text, len, t0, w1};
	const unsigned long long base = tile_base[blockIdx.x];      // newlines ahead of the tile: line `base` is the one that holds t0 (or starts at it)
	// the lines that start in the tile: at byte 0 of the text, and behind each of the tile's newlines; a wave takes every fourth
	const unsigned wave = threadIdx.x >> 6;
	if (blockIdx.x == 0 && wave == 0) gtf_line(V, 0ull, 0ull, rec, keep, status);
	for (unsigned rb = 0; rb < N.nt; rb += TEXT_NLCAP) {
		N.round(L.nl, rb);
		const unsigned r_end = min(N.nt, rb + TEXT_NLCAP);
		for (unsigned j = rb + wave; j < r_end; j += 4u) {
			const unsigned long long s = t0 + L.nl.nlpos[j - rb] + 1ull;
			if (s >= len) continue;               // the text ends with this newline
			gtf_line(V, s, base + (unsigned long long)j + 1ull, rec, keep, status);
		}
	}
}

__global__ void __launch_bounds__(256) lsq_gtf_compact_kernel(const GtfRec *rec, const unsigned *keep, const unsigned long long *place, unsigned long long n_lines,
                                                              GtfRec *out, int2 *se) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i >= n_lines || !keep[i]) return;
	const GtfRec r = rec[i];
	out[place[i]] = r;
	se[place[i]] = make_int2(r.start, r.end);
}

__device__ inline bool gtf_same_bytes(const unsigned char *a, const unsigned char *b, unsigned n) {
	for (unsigned q = 0; q < n; ++q) if (a[q] != b[q]) return false;
	return true;
}

// head[k] = 1 where kept line k opens a run of one (gene id, transcript id); 0 behind the kept lines (the scan runs over n_lines)
__global__ void __launch_bounds__(256) lsq_gtf_heads_kernel(const unsigned char *text, const GtfRec *out, const unsigned long long *n_kept_p, unsigned long long n_lines, unsigned *head) {
	const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (k >= n_lines) return;
	unsigned h = 0;
	if (k < *n_kept_p) {
		h = 1;
		if (k > 0) {
			const GtfRec a = out[k], b = out[k - 1];
			if (a.gene_len == b.gene_len && a.tx_len == b.tx_len &&
			    gtf_same_bytes(text + a.line_off + a.gene_off, text + b.line_off + b.gene_off, a.gene_len) &&
			    gtf_same_bytes(text + a.line_off + a.tx_off, text + b.line_off + b.tx_off, a.tx_len)) h = 0;
		}
	}
	head[k] = h;
}

__global__ void __launch_bounds__(256) lsq_gtf_emit_heads_kernel(const GtfRec *out, const unsigned *head, const unsigned long long *place, const unsigned long long *n_kept_p,
                                                                 GtfRec *heads) {
	const unsigned long long k = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (k >= *n_kept_p || !head[k]) return;
	GtfRec r = out[k];
	r.aux = (unsigned)k;
	heads[place[k]] = r;
}

const char *const KIND_TEXT[] = {"", "", "PROBLEM: Expected to find attribute: gene_id", "", "PROBLEM: Expected to find attribute: transcript_id", ""};

int parse_bytes(lsq_ctx *c, const unsigned char *bytes, unsigned long long len, const char *label, lsq_gtf **out) {
	*out = nullptr;
	std::unique_ptr<lsq_gtf> G(new lsq_gtf);
	if (len == 0) { *out = G.release(); return LSQ_OK; }
	HIP_TRY(hipSetDevice(c->device));
	hipStream_t st = c->stream;
	lsq_text T;
	int rc;
	PhaseClock<4> PC;            // marks 2 -> 3, the host's look at the status, are not reported
	if ((rc = PC.make())) return rc;
	if ((rc = text_stage_buffer(c, bytes, len, label, T))) return rc;
	HIP_TRY(PC.mark(0, st));
	if ((rc = scan_newlines(c, T))) return rc;
	HIP_TRY(PC.mark(1, st));
	const unsigned long long n_lines = T.n_nl + 1;                 // lines that may exist (the last one may be empty: the text ends in a newline)
	if (n_lines >= 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "%s: more than 2^32 lines", label);
	const unsigned long long n_tiles = (len + TEXT_TILE - 1) / TEXT_TILE;
	DevBuf<GtfRec> d_rec, d_out, d_heads;
	DevBuf<int2> d_se;
	DevBuf<unsigned> d_keep, d_head;
	DevBuf<unsigned long long> d_kplace, d_hplace;
	DevBuf<GtfStatus> d_status;
	ScanScratch S;
	if ((rc = d_rec.alloc(n_lines)) || (rc = d_out.alloc(n_lines)) || (rc = d_heads.alloc(n_lines)) || (rc = d_se.alloc(n_lines)) || (rc = d_keep.alloc(n_lines)) ||
	    (rc = d_head.alloc(n_lines)) || (rc = d_kplace.alloc(n_lines + 1)) || (rc = d_hplace.alloc(n_lines + 1)) || (rc = d_status.alloc(1)) || (rc = S.reserve(n_lines))) return rc;
	const GtfStatus clean{GTF_NO_ERR, 0};
	HIP_TRY(hipMemcpyAsync(d_status.p, &clean, sizeof clean, hipMemcpyHostToDevice, st));
	HIP_TRY(hipMemsetAsync(d_keep.p, 0, n_lines * sizeof(unsigned), st));
	const unsigned lb = grid_for(n_lines, 256);
	hipLaunchKernelGGL(lsq_gtf_lines_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, (const unsigned char *)T.d_text.p, len, (const unsigned long long *)T.d_tile_base.p,
	                   d_rec.p, d_keep.p, d_status.p);
	if ((rc = device_scan<1, true>(S, d_keep.p, n_lines, d_kplace.p, st))) return rc;
	hipLaunchKernelGGL(lsq_gtf_compact_kernel, dim3(lb), dim3(256), 0, st, (const GtfRec *)d_rec.p, (const unsigned *)d_keep.p, (const unsigned long long *)d_kplace.p, n_lines, d_out.p, d_se.p);
	hipLaunchKernelGGL(lsq_gtf_heads_kernel, dim3(lb), dim3(256), 0, st, (const unsigned char *)T.d_text.p, (const GtfRec *)d_out.p, (const unsigned long long *)(d_kplace.p + n_lines), n_lines, d_head.p);
	if ((rc = device_scan<1, true>(S, d_head.p, n_lines, d_hplace.p, st))) return rc;
	hipLaunchKernelGGL(lsq_gtf_emit_heads_kernel, dim3(lb), dim3(256), 0, st, (const GtfRec *)d_out.p, (const unsigned *)d_head.p, (const unsigned long long *)d_hplace.p,
	                   (const unsigned long long *)(d_kplace.p + n_lines), d_heads.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(PC.mark(2, st));
	GtfStatus status;
	unsigned long long n_kept = 0, n_heads = 0;
	HIP_TRY(hipMemcpyAsync(&status, d_status.p, sizeof status, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&n_kept, d_kplace.p + n_lines, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&n_heads, d_hplace.p + n_lines, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (status.err != GTF_NO_ERR) {
		const unsigned long long idx = status.err >> 8;
		const int kind = (int)(status.err & 0xFF);
		if (kind == GTF_E_SHORT) return fail(LSQ_E_PARSE, "PROBLEM: line %llu has fewer than nine TAB-separated fields", idx + 1);
		if (kind == GTF_E_NO_GENE || kind == GTF_E_NO_TX) return fail(LSQ_E_PARSE, "%s", KIND_TEXT[kind]);
		GtfRec r;
		HIP_TRY(hipMemcpy(&r, d_rec.p + idx, sizeof r, hipMemcpyDeviceToHost));
		const std::string item((const char *)bytes + r.line_off + r.gene_off, r.gene_len);      // sliced out of the host's copy by the device's offsets
		return fail(LSQ_E_PARSE, "PROBLEM: Unexpected token: %s", item.c_str());
	}
	if (n_kept > n_lines || n_heads > n_kept) return fail(LSQ_E_INTERNAL, "%s: %llu kept lines and %llu runs of %llu lines", label, n_kept, n_heads, n_lines);
	HIP_TRY(PC.mark(3, st));
	std::vector<GtfRec> heads((size_t)n_heads);
	std::vector<int32_t> se((size_t)n_kept * 2);
	if (n_kept) {
		HIP_TRY(hipMemcpyAsync(heads.data(), d_heads.p, (size_t)n_heads * sizeof(GtfRec), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(se.data(), d_se.p, (size_t)n_kept * sizeof(int2), hipMemcpyDeviceToHost, st));
	}
	HIP_TRY(PC.mark(4, st));
	HIP_TRY(hipStreamSynchronize(st));
	float t;
	G->ms[0] = T.h2d_ms;
	HIP_TRY(PC.ms(0, &t)); G->ms[1] = t;
	HIP_TRY(PC.ms(1, &t)); G->ms[2] = t;
	HIP_TRY(PC.ms(3, &t)); G->ms[3] = t;
	G->n_lines = T.n_nl + (bytes[len - 1] != '\n' ? 1 : 0);
	G->n_kept = n_kept; G->n_skipped = status.skipped;
	if (status.skipped)
		warn("%s: %llu line(s) that are empty or begin with '#' were skipped (the reference's parseGencode dies on them)", label, status.skipped);
	for (const GtfRec &h : heads)
		if (h.line_off > len || (unsigned long long)h.gene_off + h.gene_len > len - h.line_off || (unsigned long long)h.tx_off + h.tx_len > len - h.line_off ||
		    (unsigned long long)h.strand_off + h.strand_len > len - h.line_off || h.chrom_len > len - h.line_off || h.aux >= n_kept)
			return fail(LSQ_E_INTERNAL, "%s: a record of line %u points outside the text", label, h.line_no);
	if ((rc = gtf_assemble(bytes, heads.data(), heads.size(), se.data(), (size_t)n_kept, G->tx, G->n_genes))) return rc;
	*out = G.release();
	return LSQ_OK;
}

struct Mapped {
	void *p = MAP_FAILED; size_t n = 0; int fd = -1;
	~Mapped() { if (p != MAP_FAILED) munmap(p, n); if (fd >= 0) close(fd); }
};

} // namespace

extern "C" {

int lsq_gtf_parse_text(lsq_ctx *c, const void *bytes, uint64_t len, lsq_gtf **out) LSQ_API_TRY {
	if (!c || !out || (!bytes && len)) return fail(LSQ_E_ARG, "null argument");
	return parse_bytes(c, (const unsigned char *)bytes, len, "GTF text", out);
} LSQ_API_CATCH

int lsq_gtf_parse(lsq_ctx *c, const char *path, lsq_gtf **out) LSQ_API_TRY {
	if (!c || !path || !out) return fail(LSQ_E_ARG, "null argument");
	*out = nullptr;
	Mapped M;
	M.fd = open(path, O_RDONLY);
	if (M.fd < 0) return fail(LSQ_E_IO, "cannot open GTF file %s", path);
	struct stat sb;
	if (fstat(M.fd, &sb) != 0) return fail(LSQ_E_IO, "cannot stat %s", path);
	if (!S_ISREG(sb.st_mode)) {               // a pipe, a terminal: read to the end
		std::string all;
		int rc = read_all(path, all);
		return rc ? rc : parse_bytes(c, (const unsigned char *)all.data(), all.size(), path, out);
	}
	M.n = (size_t)sb.st_size;
	if (M.n == 0) return parse_bytes(c, nullptr, 0, path, out);
	M.p = mmap(nullptr, M.n, PROT_READ, MAP_PRIVATE, M.fd, 0);
	if (M.p == MAP_FAILED) return fail(LSQ_E_IO, "cannot map %s", path);
	madvise(M.p, M.n, MADV_SEQUENTIAL);
	return parse_bytes(c, (const unsigned char *)M.p, M.n, path, out);
} LSQ_API_CATCH

} // extern "C"
