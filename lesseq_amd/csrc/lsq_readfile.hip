// The read files of the loader: the formats the device parses from a file's own bytes (READ_FORMATS), a file of one of them opened
// (ReadSource), and the entry points that take one -- through the chain (lsq_ingest.hip) for count and solve, into the arrays of
// lsq_mrf_parse for tests and tools, or over its records alone (lsq_bam_check).  The parsers themselves are lsq_mrf_device.hpp,
// lsq_sam_device.hpp and lsq_bam_device.hpp; this unit and the chain's meet through lsq_ingest.hpp only.  The tools that take a
// read file against an index's dictionaries (junctions, coverage, exonbins, psi, evidence, sites, retention) enter through table_of_file: their passes
// (lsq_junc.hip, lsq_cov.hip, lsq_exonbins.hip, lsq_psi.hip, lsq_evidence.hip, lsq_sites.hip, lsq_retention.hip) take the device arrays as lsq_readtool.hpp's ParsedReads.
#include <fcntl.h>
#include <unistd.h>

#include "lsq_ingest.hpp"
#include "lsq_mrf_device.hpp"
#include "lsq_sam_device.hpp"
#include "lsq_bam_device.hpp"
#include "lsq_junc.hpp"
#include "lsq_cov.hpp"
#include "lsq_exonbins.hpp"
#include "lsq_sites.hpp"
#include "lsq_retention.hpp"
#include "lsq_psi.hpp"
#include "lsq_evidence.hpp"
#include "lsq_libtype.hpp"

namespace {

// The dictionaries of a parse: the events' chromosome names behind a hash table, the strand table seeded with the strands
// already known.  The events' strand dictionary grows by the strings the file introduces (as it does under lsq_mrf_parse).
struct MrfDictDev {
	DevBuf<unsigned> d_hash, d_id, d_off;
	DevBuf<unsigned long long> d_strand;
	DevBuf<char> d_names;
	size_t n_seed = 0;
	MrfDict D{};
	int build(lsq_ctx *c, hipStream_t st) {
		lsq_events &E = *c->E;
		int rc;
		const size_t nc = E.n_table_chroms();          // (chromosome ids that have tables)
		size_t tab = 2;
		while (tab < 4 * nc) tab <<= 1;
		std::vector<unsigned> h_hash(tab, 0), h_id(tab, 0), h_off(nc + 1, 0);
		std::string h_names;
		for (size_t id = 0; id < nc; ++id) {
			const std::string &nm = E.chroms.names[id];
			const unsigned h = mrf_fnv32(nm.data(), nm.size());
			size_t i = (size_t)(h & (unsigned)(tab - 1));
			while (h_hash[i] != 0) i = (i + 1) & (tab - 1);
			h_hash[i] = h; h_id[i] = (unsigned)id;
			h_names += nm;
			h_off[id + 1] = (unsigned)h_names.size();
		}
		if (E.strands.names.size() > 256) return fail(LSQ_E_RANGE, "more than 256 distinct strand strings");
		n_seed = E.strands.names.size();
		std::vector<unsigned long long> h_strand(256, STRAND_EMPTY);
		for (size_t i = 0; i < n_seed; ++i) {
			const std::string &s = E.strands.names[i];
			h_strand[i] = s.size() <= 7 ? mrf_strand_key(s.data(), s.size()) : STRAND_UNMATCHABLE;
		}
		if ((rc = d_hash.upload(h_hash.data(), tab, st)) || (rc = d_id.upload(h_id.data(), tab, st)) || (rc = d_off.upload(h_off.data(), nc + 1, st)) ||
		    (rc = d_names.upload(h_names.data(), h_names.size(), st)) || (rc = d_strand.upload(h_strand.data(), 256, st))) return rc;
		HIP_TRY(hipStreamSynchronize(st));            // the host vectors go out of scope
		D.chrom_hash = d_hash.p; D.chrom_id = d_id.p; D.name_off = d_off.p; D.names = d_names.p; D.mask = (unsigned)(tab - 1);
		D.n_chrom = (unsigned)nc; D.names_bytes = (unsigned)h_names.size(); D.strand_tab = d_strand.p;
		return LSQ_OK;
	}
	// once the parse kernels have run and the table has been read back: the strings the file introduced join the events' dictionary
	int learn(lsq_ctx *c, const std::vector<unsigned long long> &h_strand) {
		lsq_events &E = *c->E;
		for (size_t i = n_seed; i < 256 && h_strand[i] != STRAND_EMPTY; ++i) {
			const unsigned long long k = h_strand[i];
			std::string s;
			for (unsigned j = 0; j < (unsigned)(k & 0xFF); ++j) s.push_back((char)(k >> (56 - 8 * j)));
			const int id = E.strands.intern(s);
			if (id != (int)i) return fail(LSQ_E_STATE, "strand dictionary changed while a reads file was being parsed");
		}
		n_seed = E.strands.names.size();
		return LSQ_OK;
	}
};

struct DevParsed {
	uint64_t n_reads = 0, n_blocks = 0;
	DevBuf<unsigned long long> blk_off;
	DevBuf<unsigned> line_no;
	DevBuf<int> bs, be;
	DevBuf<unsigned short> bc;
	DevBuf<unsigned char> bst;
	ParsedReads view() const { return ParsedReads{n_reads, n_blocks, blk_off.p, bs.p, be.p, bc.p, bst.p}; }
};

// ---- the read formats: the one place that names them.  Per format: whether a whole file's first line is a header (MRF; every
// line of a SAM file counts: "read-<k>", k from 1), the switch that shortens its line list (tests: the run-over path on a small
// file), the routing stage's name, how a staged file of it is opened (its units counted: lines or records) and how it names a unit
// that fails, its front end for the chain (prepare once; launch the routing kernels, once more with J.all_slow set if the line list
// ran over; record what they handed on), and its count / write launches for the first pass and parse_staged_text
struct ReadSource;
struct ReadFormat {
	const char *name;
	unsigned has_header;
	const char *line_list_env, *stage;
	int (*open)(lsq_ctx *, ReadSource &);
	int (*fail_unit)(const ReadSource &, unsigned long long, hipStream_t);
	int (*prepare)(TextJob &);                               // (prepare and record may be null)
	void (*launch)(const TextJob &, const RouteTables &, const RouteOut &, hipStream_t);
	void (*record)(const TextJob &);
	void (*count)(const TextJob &, hipStream_t, unsigned *);
	void (*write)(const TextJob &, hipStream_t, const unsigned *, const unsigned long long *, const unsigned long long *, const MrfOut &);
};

// One staged file of a format, opened: how many units it holds (data lines, or records) and the number of the first, what the routing
// pass reads of it, the views its format's kernels take (J) and the error words they write -- err[0] the first unit that is
// malformed, err[1] a strand string too long, err[2] too many of them.  The dictionaries are built on request: a walk that routes
// and writes nothing (first_pass under lsq_bam_check) runs without them, and without events.
struct ReadSource {
	const ReadFormat *fmt = nullptr;
	lsq_text *T = nullptr;
	unsigned has_header = 0;
	unsigned long long n_units = 0, first_unit = 0, in_bytes = 0;
	unsigned long long list_cap = 0;          // lines the format's tile kernel may hand on (records: none)
	bool verify = false;                      // a BAM file: the CRC32 pass whatever the context's option says
	BamRecords BR;                            // a file of records: what takes the place of the text's newline tiles
	MrfDictDev DD;
	DevBuf<unsigned long long> d_err;
	TextJob J{};

	int open(lsq_ctx *c, const ReadFormat *f, lsq_text &text, unsigned header, unsigned long long first_line) {
		int rc;
		fmt = f; T = &text; has_header = header; first_unit = first_line;
		if ((rc = ensure_lanes(c)) || (rc = fmt->open(c, *this))) return rc;        // (c->ev1 / c->ev2 are the lanes thread's)
		if (first_unit + n_units > 0xFFFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^32 lines");
		if ((rc = d_err.alloc(4)) || (rc = reset_errors(c->stream))) return rc;
		J.c = c; J.X = MrfText{T->d_text.p, T->len, T->d_tile_base.p, has_header, first_unit, n_units}; J.R = BR.view(); J.err = d_err.p;
		J.n_tiles = (unsigned)((T->len + TEXT_TILE - 1) / TEXT_TILE);
		return LSQ_OK;
	}
	int dictionaries(lsq_ctx *c) {
		const int rc = DD.build(c, c->stream);
		J.D = DD.D;
		return rc;
	}
	int reset_errors(hipStream_t st) {
		static const unsigned long long err0[4] = {MRF_NO_ERR, 0, 0, 0};
		HIP_TRY(hipMemcpyAsync(d_err.p, err0, sizeof(err0), hipMemcpyHostToDevice, st));
		return LSQ_OK;
	}
	int fail_unit(unsigned long long k, hipStream_t st) const { return fmt->fail_unit(*this, k, st); }
	// after the parse kernels have run: waits for the stream; the first failing unit, strand strings out of range, new strands
	int settle(lsq_ctx *c, hipStream_t st) {
		unsigned long long err[4];
		std::vector<unsigned long long> h_strand(256);
		HIP_TRY(hipMemcpyAsync(err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(h_strand.data(), DD.d_strand.p, 256 * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		if (err[0] != MRF_NO_ERR) return fail_unit(err[0], st);
		if (err[1]) return fail(LSQ_E_UNSUPPORTED, "a strand string longer than 7 bytes: outside the device parser's range (lsq_mrf_parse handles it)");
		if (err[2]) return fail(LSQ_E_RANGE, "more than 256 distinct strand strings");
		return DD.learn(c, h_strand);
	}
};

// a text: its newlines counted (once), a unit a terminated line behind the header
int text_open(lsq_ctx *c, ReadSource &S) {
	lsq_text &T = *S.T;
	int rc;
	if (T.len && (rc = scan_newlines(c, T))) return rc;
	const unsigned long long n_nl = T.len ? T.n_nl : 0;
	S.n_units = n_nl >= 1 + S.has_header ? n_nl - S.has_header : 0;       // (header only, or no terminated line at all: no reads)
	S.in_bytes = T.len;
	// what a format's tile kernel hands on: tiles it does not take (MRF: more delimiters than the fast kernel's tables hold), lines
	// it does not settle (another shape than a read's; at most one a tile begins ahead of its window; the rest is whatever the
	// file holds -- when the list runs over, the whole file goes through the format's byte-walking kernel)
	S.list_cap = 1ull << 22;
	if (const char *e = getenv(S.fmt->line_list_env)) { const long long v = atoll(e); if (v >= 0) S.list_cap = (unsigned long long)v; }
	return LSQ_OK;
}
// the text of the failing line, from the file: between the newline that ends the line before it and its own
int text_fail_line(const ReadSource &S, unsigned long long line_no, hipStream_t) {
	const lsq_text &T = *S.T;
	const unsigned long long want = line_no - S.first_unit + S.has_header;      // ordinal of the newline that ends the failing line
	std::string text;
	const int fd = open(T.path.c_str(), O_RDONLY);
	if (fd >= 0) {
		// walk the file's range for the want-th newline (an error path: speed does not matter, bounded memory does)
		std::vector<char> buf(1 << 20);
		unsigned long long seen = 0, pos = 0;
		bool in_line = want == 0, done = false;
		while (!done && pos < T.len) {
			const size_t ask = (size_t)std::min<unsigned long long>(buf.size(), T.len - pos);
			const ssize_t got = pread(fd, buf.data(), ask, (off_t)(T.offset + pos));
			if (got <= 0) break;
			for (ssize_t q = 0; q < got && !done; ++q) {
				if (buf[(size_t)q] == '\n') {
					if (in_line) done = true;
					else if (++seen == want) in_line = true;
				} else if (in_line) text.push_back(buf[(size_t)q]);
			}
			pos += (unsigned long long)got;
		}
		close(fd);
	}
	return fail(LSQ_E_PARSE, "#%llu:%s", line_no, text.c_str());
}
// a BAM file: inflated, its header read, its records found; record i is data line i, behind the header's lines
int bam_open(lsq_ctx *c, ReadSource &S) {
	if (S.has_header || S.first_unit != 1ull) return fail(LSQ_E_ARG, "a %s file is taken whole, not in byte ranges", S.fmt->name);
	const int rc = bam_open_verified(c, *S.T, S.BR, S.verify || c->opt_bam_verify);
	S.n_units = S.BR.n_rec; S.first_unit = S.BR.H.h_lines + 1; S.in_bytes = S.BR.total;
	return rc;
}
int bam_fail_record(const ReadSource &S, unsigned long long line_no, hipStream_t st) { return S.BR.fail_record(line_no, st); }

const ReadFormat READ_FORMATS[] = {
	{"MRF_SINGLE", 1u, "LSQ_MRF_LINE_LIST", "route", text_open, text_fail_line, mrf_prepare, mrf_launch, mrf_record,
	 [](const TextJob &J, hipStream_t st, unsigned *nb) { hipLaunchKernelGGL(lsq_mrf_count_kernel, dim3(J.n_tiles), dim3(256), 0, st, J.X, nb, J.err); },
	 [](const TextJob &J, hipStream_t st, const unsigned *nb, const unsigned long long *rd, const unsigned long long *bk, const MrfOut &O) {
		 hipLaunchKernelGGL(lsq_mrf_write_kernel, dim3(J.n_tiles), dim3(256), 0, st, J.X, nb, rd, bk, J.D, O, J.err); }},
	{"SAM_SINGLE", 0u, "LSQ_SAM_LINE_LIST", "sam_route", text_open, text_fail_line, sam_prepare, sam_launch, sam_record,
	 [](const TextJob &J, hipStream_t st, unsigned *nb) { hipLaunchKernelGGL(lsq_sam_count_kernel, dim3(J.n_tiles), dim3(256), 0, st, J.X, sam_opts(J.c), nb, J.err); },
	 [](const TextJob &J, hipStream_t st, const unsigned *nb, const unsigned long long *rd, const unsigned long long *bk, const MrfOut &O) {
		 hipLaunchKernelGGL(lsq_sam_write_kernel, dim3(J.n_tiles), dim3(256), 0, st, J.X, sam_opts(J.c), nb, rd, bk, J.D, O, J.err, J.c->E->stranded() ? 1u : 0u); }},
	{"BAM_SINGLE", 0u, nullptr, "bam_route", bam_open, bam_fail_record, nullptr, bam_launch, nullptr,
	 [](const TextJob &J, hipStream_t st, unsigned *nb) {
		 hipLaunchKernelGGL(lsq_bam_count_kernel, dim3((unsigned)((J.X.n_lines + 255) / 256)), dim3(256), 0, st, J.R, J.X, sam_opts(J.c), nb, J.err); },
	 [](const TextJob &J, hipStream_t st, const unsigned *nb, const unsigned long long *rd, const unsigned long long *bk, const MrfOut &O) {
		 hipLaunchKernelGGL(lsq_bam_write_kernel, dim3((unsigned)((J.X.n_lines + 255) / 256)), dim3(256), 0, st, J.R, J.X, sam_opts(J.c), nb, rd, bk, J.D, O, J.err, J.c->E->stranded() ? 1u : 0u); }},
};
// the format a caller names (looked up once its file has been opened: the order in which the reference meets a bad file or literal)
int read_format_named(const char *name, const ReadFormat *&fmt) {
	if (!name) return fail(LSQ_E_ARG, "null argument");
	for (const ReadFormat &f : READ_FORMATS) if (strcmp(name, f.name) == 0) { fmt = &f; return LSQ_OK; }
	return fail(LSQ_E_FORMAT, "Unknown file format error: %s", name);
}

// The first pass over an opened file: the blocks of every unit (0 for one that makes no read), the two prefix sums -- which read a
// unit is, where its blocks go -- and their totals; the first malformed unit ends the run here.  Needs the error words alone.
struct FirstPass {
	DevBuf<unsigned> line_nb;
	DevBuf<unsigned long long> rd_idx, bk_off;
	unsigned long long n_reads = 0, n_blocks = 0;
};
int first_pass(ReadSource &S, hipStream_t st, FirstPass &P) {
	const unsigned long long n = S.n_units;
	unsigned long long bad = MRF_NO_ERR;
	ScanScratch SS;
	int rc;
	if ((rc = P.line_nb.alloc(n)) || (rc = P.rd_idx.alloc(n + 1)) || (rc = P.bk_off.alloc(n + 1)) || (rc = SS.reserve(n))) return rc;
	S.fmt->count(S.J, st, P.line_nb.p);
	HIP_TRY(hipGetLastError());
	if ((rc = device_scan<1, true>(SS, P.line_nb.p, n, P.rd_idx.p, st)) || (rc = device_scan<1, false>(SS, P.line_nb.p, n, P.bk_off.p, st))) return rc;
	HIP_TRY(hipMemcpyAsync(&P.n_reads, P.rd_idx.p + n, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&P.n_blocks, P.bk_off.p + n, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&bad, S.d_err.p, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	return bad != MRF_NO_ERR ? S.fail_unit(bad, st) : LSQ_OK;
}

// Parses staged text on the device into the arrays of lsq_mrf_parse (file order): lsq_mrf_parse_device.
int parse_staged_text(lsq_ctx *c, const ReadFormat *fmt, lsq_text &T, DevParsed &out) {
	hipStream_t st = c->stream;
	int rc;
	if ((rc = ensure_lanes(c))) return rc;                 // (c->ev1 / c->ev2 are the lanes thread's)
	out.n_reads = out.n_blocks = 0;
	c->mrf_h2d_ms = T.h2d_ms; c->mrf_parse_ms = 0;
	HIP_TRY(hipEventRecord(c->ev1, st));
	ReadSource S;
	if ((rc = S.open(c, fmt, T, fmt->has_header, 1ull))) return rc;
	if (!S.n_units) {                                      // header only (or no terminated line at all)
		const unsigned long long zero_off = 0;
		if ((rc = out.blk_off.upload(&zero_off, 1, st)) || (rc = out.line_no.alloc(0)) || (rc = out.bs.alloc(0)) || (rc = out.be.alloc(0)) ||
		    (rc = out.bc.alloc(0)) || (rc = out.bst.alloc(0))) return rc;
		HIP_TRY(hipStreamSynchronize(st));
		return LSQ_OK;
	}
	FirstPass P;
	if ((rc = S.dictionaries(c)) || (rc = first_pass(S, st, P))) return rc;
	if ((rc = out.blk_off.alloc(P.n_reads + 1)) || (rc = out.line_no.alloc(P.n_reads)) || (rc = out.bs.alloc(P.n_blocks)) || (rc = out.be.alloc(P.n_blocks)) ||
	    (rc = out.bc.alloc(P.n_blocks)) || (rc = out.bst.alloc(P.n_blocks))) return rc;
	const MrfOut O{out.blk_off.p, out.line_no.p, out.bs.p, out.be.p, out.bc.p, out.bst.p};
	fmt->write(S.J, st, P.line_nb.p, P.rd_idx.p, P.bk_off.p, O);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(c->ev2, st));
	if ((rc = S.settle(c, st))) return rc;
	(void)hipEventElapsedTime(&c->mrf_parse_ms, c->ev1, c->ev2);
	out.n_reads = P.n_reads; out.n_blocks = P.n_blocks;
	return LSQ_OK;
}

// A read file's bytes in HBM through the chain: the file opened, then the format's parse as the chain's routing pass
int ingest_text(lsq_ctx *c, int method, const ReadFormat *fmt, lsq_text &T, unsigned has_header, unsigned long long first_line) {
	hipStream_t st = c->stream;
	int rc;
	c->mrf_h2d_ms = T.h2d_ms; c->mrf_parse_ms = 0;
	stages_reset(c, T.scanned);          // (newlines counted earlier, through lsq_text_lines: that pass is this ingest's)
	ReadSource S;
	if ((rc = S.open(c, fmt, T, has_header, first_line)) || (rc = S.dictionaries(c))) return rc;
	TextJob &J = S.J;
	const unsigned line_cap = (unsigned)std::min<unsigned long long>(S.n_units, S.list_cap) + J.n_tiles + 1u;
	DevBuf<MrfLongLine> d_lines;
	DevBuf<unsigned> d_tiles, d_counts;
	if ((rc = d_lines.alloc(line_cap)) || (rc = d_tiles.alloc(J.n_tiles)) || (rc = d_counts.alloc(4))) return rc;
	HIP_TRY(hipMemsetAsync(d_counts.p, 0, 16, st));          // (a file without lines launches nothing; the verdict below still reads these)
	J.H = MrfHandOff{d_counts.p, d_tiles.p, J.n_tiles, d_lines.p, line_cap};
	if (fmt->prepare && (rc = fmt->prepare(J))) return rc;
	Front F;
	F.n = S.n_units; F.line_no = nullptr; F.first_line = S.first_unit; F.in_bytes = S.in_bytes; F.stage = fmt->stage;
	F.launch = [&](const RouteTables &RT, const RouteOut &O, hipStream_t s) -> int {
		const int r2 = S.reset_errors(s);
		if (r2) return r2;
		HIP_TRY(hipMemsetAsync(d_counts.p, 0, 16, s));
		fmt->launch(J, RT, O, s);
		HIP_TRY(hipGetLastError());
		return LSQ_OK;
	};
	F.settle = [&](hipStream_t s) -> int {
		// the line list ran over (a file of lines of another shape than a read's): once more, every tile through the byte-walking kernel
		HIP_TRY(hipMemcpy(J.counts, d_counts.p, 16, hipMemcpyDeviceToHost));
		if (J.counts[2] && !J.all_slow) { J.all_slow = true; return LSQ_RETRY; }
		if (J.counts[2]) return fail(LSQ_E_INTERNAL, "the device parser's line list ran over");
		if (fmt->record) fmt->record(J);
		return S.settle(c, s);
	};
	c->reads[method].named = false;
	if ((rc = ingest_device(c, method, F))) return rc;
	// (device time of the parse = the passes up to and including the routing pass; the rest of the chain is the ingest)
	for (int k = 0; k < c->ing_n; ++k) {
		c->mrf_parse_ms += c->ing_pass[k].ms;
		if (strcmp(c->ing_pass[k].name, fmt->stage) == 0) break;
	}
	return LSQ_OK;
}

// A read file parsed as lsq_mrf_parse_device parses it, against dictionaries that are not the context's events' (table_of_file:
// an index's chromosomes and strand table): for the length of the call E stands where the context's events do,
// so every parser finds its chromosomes, its strand table and its library type where it always looks -- unstranded, or, under a
// stranded index, a stranded one: the parsers then deliver the strand of a fragment's first mate, as for stranded events.  The text is
// freed once it has been read (its room is the caller's sort's); the context's events, reads and counters are not touched.
int parse_file_against(lsq_ctx *c, lsq_events &E, const char *read_format, const char *path, DevParsed &P) {
	HIP_TRY(hipSetDevice(c->device));
	const ReadFormat *fmt;
	lsq_text T;
	int rc;
	if ((rc = ensure_lanes(c)) || (rc = stage_text_file(c, path, 0, ~0ull, T)) || (rc = read_format_named(read_format, fmt))) return rc;
	struct Stand { lsq_ctx *c; lsq_events *own; ~Stand() { c->E = own; } } stand{c, c->E};
	c->E = &E;
	return parse_staged_text(c, fmt, T, P);
}

// lsq_jn_device, lsq_ss_device, lsq_ir_device, lsq_cov_device, lsq_xb_device, lsq_ps_device, lsq_fe_device behind their argument checks: the file parsed against the index's dictionaries, a
// new table filled from the device arrays by the tool's passes (fill(reads, table)) and handed out
template <class IX, class T, class F>
int table_of_file(lsq_ctx *c, IX *ix, const char *read_format, const char *path, T **out, F fill) {
	DevParsed P;
	const int rc = parse_file_against(c, ix->E, read_format, path, P);
	return rc ? rc : new_table(out, [&](T &t) { return fill(P.view(), t); });
}

} // namespace

extern "C" {

int lsq_reads_upload_mrf(lsq_ctx *c, int method, const char *read_format, const char *path) LSQ_API_TRY {
	if (!c) return fail(LSQ_E_ARG, "null argument");
	if (!c->E) return fail(LSQ_E_STATE, "lsq_events_upload must come first");
	if (method < 0 || method >= c->E->n_methods) return fail(LSQ_E_ARG, "method %d out of range", method);
	HIP_TRY(hipSetDevice(c->device));
	HostStopwatch SW;
	if (!read_format || !path) return fail(LSQ_E_ARG, "null argument");
	const ReadFormat *fmt;
	lsq_text T;
	int rc;
	if ((rc = stage_text_file(c, path, 0, ~0ull, T)) || (rc = read_format_named(read_format, fmt))) return rc;
	rc = ingest_text(c, method, fmt, T, fmt->has_header, 1ull);
	SW.mark("upload_mrf: all");
	return rc;
} LSQ_API_CATCH

int lsq_reads_upload_text(lsq_ctx *c, int method, const char *read_format, lsq_text *t) LSQ_API_TRY {
	const ReadFormat *fmt = nullptr;          // (a whole file of its format: the first line as the format has it; a bad literal is reported below)
	(void)read_format_named(read_format, fmt);
	return lsq_reads_upload_text_at(c, method, read_format, t, fmt ? (int)fmt->has_header : 1, 1);
} LSQ_API_CATCH

int lsq_reads_upload_text_at(lsq_ctx *c, int method, const char *read_format, lsq_text *t, int has_header, uint64_t first_line) LSQ_API_TRY {
	if (!c || !t) return fail(LSQ_E_ARG, "null argument");
	if (!c->E) return fail(LSQ_E_STATE, "lsq_events_upload must come first");
	if (method < 0 || method >= c->E->n_methods) return fail(LSQ_E_ARG, "method %d out of range", method);
	HIP_TRY(hipSetDevice(c->device));
	const ReadFormat *fmt;
	const int rc = read_format_named(read_format, fmt);
	return rc ? rc : ingest_text(c, method, fmt, *t, has_header ? 1u : 0u, first_line);
} LSQ_API_CATCH

int lsq_mrf_parse_device(lsq_ctx *c, const char *read_format, const char *path, lsq_reads **out) LSQ_API_TRY {
	if (!c || !out) return fail(LSQ_E_ARG, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	if (!c->E) return fail(LSQ_E_STATE, "lsq_events_upload must come first");
	if (!read_format || !path) return fail(LSQ_E_ARG, "null argument");
	const ReadFormat *fmt;
	lsq_text T;
	int rc;
	if ((rc = stage_text_file(c, path, 0, ~0ull, T)) || (rc = read_format_named(read_format, fmt))) return rc;
	DevParsed P;
	if ((rc = parse_staged_text(c, fmt, T, P))) return rc;
	std::unique_ptr<lsq_reads> R(new lsq_reads);
	R->o_blk_off.resize(P.n_reads + 1); R->o_line_no.resize(P.n_reads);
	R->o_start.resize(P.n_blocks); R->o_end.resize(P.n_blocks); R->o_chrom.resize(P.n_blocks); R->o_strand.resize(P.n_blocks);
	HIP_TRY(hipMemcpy(R->o_blk_off.data(), P.blk_off.p, (P.n_reads + 1) * 8, hipMemcpyDeviceToHost));
	if (P.n_reads) HIP_TRY(hipMemcpy(R->o_line_no.data(), P.line_no.p, P.n_reads * 4, hipMemcpyDeviceToHost));
	if (P.n_blocks) {
		HIP_TRY(hipMemcpy(R->o_start.data(), P.bs.p, P.n_blocks * 4, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(R->o_end.data(), P.be.p, P.n_blocks * 4, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(R->o_chrom.data(), P.bc.p, P.n_blocks * 2, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(R->o_strand.data(), P.bst.p, P.n_blocks, hipMemcpyDeviceToHost));
	}
	R->adopt();
	*out = R.release();
	return LSQ_OK;
} LSQ_API_CATCH

// developer entry (include/lesseq_hip_dev.h): which of the parse's three kernels the latest MRF text went through
int lsq_debug_last_parse_paths(const lsq_ctx *c, unsigned *tiles_handed, unsigned *lines_listed, unsigned *all_slow) {
	if (!c) return LSQ_E_ARG;
	if (tiles_handed) *tiles_handed = c->parse_tiles_handed;
	if (lines_listed) *lines_listed = c->parse_lines_listed;
	if (all_slow) *all_slow = c->parse_all_slow;
	return LSQ_OK;
}

int lsq_last_mrf_timing(lsq_ctx *c, float *h2d_ms, float *parse_ms) LSQ_API_TRY {
	if (!c) return fail(LSQ_E_ARG, "null context");
	if (h2d_ms) *h2d_ms = c->mrf_h2d_ms;
	if (parse_ms) *parse_ms = c->mrf_parse_ms;
	return LSQ_OK;
} LSQ_API_CATCH
int lsq_last_bam_paths(const lsq_ctx *c, uint64_t *n_blocks, uint64_t *blocks_repaired) {
	if (!c) return LSQ_E_ARG;
	if (n_blocks) *n_blocks = c->bam_blocks;
	if (blocks_repaired) *blocks_repaired = c->bam_blocks_repaired;
	return LSQ_OK;
}
// developer entry (include/lesseq_hip_dev.h): the staging and the inflate kernel of the BAM chain alone
int lsq_debug_bgzf_inflate(lsq_ctx *c, const void *bytes, uint64_t len, void *out, uint64_t cap, uint64_t *n) LSQ_API_TRY {
	if (!c || (!bytes && len) || (!out && cap) || !n) return fail(LSQ_E_ARG, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	if ((rc = ensure_lanes(c))) return rc;
	lsq_text T;
	BamRecords B;
	if ((rc = text_stage_buffer(c, bytes, len, "<bytes>", T)) || (rc = bam_inflate_staged(c, T, (const unsigned char *)bytes, B, 0))) return rc;
	*n = B.total;
	if (B.total > cap) return fail(LSQ_E_RANGE, "the inflated stream holds %llu bytes, the buffer %llu", B.total, (unsigned long long)cap);
	if (B.total) HIP_TRY(hipMemcpy(out, B.d_stream.p, (size_t)B.total, hipMemcpyDeviceToHost));
	return LSQ_OK;
} LSQ_API_CATCH
// developer entry: ... and the CRC32 kernel behind it, its sums returned uncompared
int lsq_debug_bgzf_crc32(lsq_ctx *c, const void *bytes, uint64_t len, uint32_t *crc, uint64_t cap, uint64_t *n) LSQ_API_TRY {
	if (!c || (!bytes && len) || (!crc && cap) || !n) return fail(LSQ_E_ARG, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	int rc;
	if ((rc = ensure_lanes(c))) return rc;
	lsq_text T;
	BamRecords B;
	if ((rc = text_stage_buffer(c, bytes, len, "<bytes>", T)) || (rc = bam_inflate_staged(c, T, (const unsigned char *)bytes, B, 2))) return rc;
	*n = B.tab.size();
	if (B.tab.size() > cap) return fail(LSQ_E_RANGE, "the file holds %llu BGZF blocks, the buffer %llu", (unsigned long long)B.tab.size(), (unsigned long long)cap);
	if (!B.tab.empty()) HIP_TRY(hipMemcpy(crc, B.d_crc.p, B.tab.size() * 4, hipMemcpyDeviceToHost));
	return LSQ_OK;
} LSQ_API_CATCH

// The whole-file check (include/lesseq_hip.h): the file opened as every BAM file is, always verifying, then the first pass of
// lsq_mrf_parse_device over its records.  No events needed: no record is routed, no dictionary built.
int lsq_bam_check(lsq_ctx *c, const char *path, lsq_bam_report *r) LSQ_API_TRY {
	if (!c || !path || !r) return fail(LSQ_E_ARG, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	const ReadFormat *fmt;
	lsq_text T;
	ReadSource S;
	FirstPass P;
	int rc;
	S.verify = true;
	if ((rc = ensure_lanes(c)) || (rc = stage_text_file(c, path, 0, ~0ull, T)) || (rc = read_format_named("BAM_SINGLE", fmt)) || (rc = S.open(c, fmt, T, 0u, 1ull))) return rc;
	if (S.n_units && (rc = first_pass(S, c->stream, P))) return rc;
	lsq_bam_report R{};
	R.file_bytes = T.len; R.blocks = S.BR.tab.size(); R.inflated_bytes = S.BR.total;
	R.header_lines = S.BR.H.h_lines; R.references = S.BR.H.ref_names.size();
	R.records = S.BR.n_rec; R.blocks_repaired = c->bam_blocks_repaired;
	R.reads = P.n_reads; R.read_blocks = P.n_blocks;
	*r = R;
	return LSQ_OK;
} LSQ_API_CATCH

// The splice junctions of a read file (include/lesseq_hip.h): the device arrays handed to lsq_junc.hip
int lsq_jn_device(lsq_ctx *c, lsq_jn_index *ix, const char *read_format, const char *path, uint32_t min_overhang, lsq_jn_table **out) LSQ_API_TRY {
	if (!c || !ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	if (min_overhang < 1) return fail(LSQ_E_ARG, "min_overhang must be at least 1");
	return table_of_file(c, ix, read_format, path, out, [&](const ParsedReads &R, lsq_jn_table &t) {
		const int rc = jn_device_reads(c, *ix, R, min_overhang, t);
		if (!rc) jn_finish_table(*ix, t);
		return rc;
	});
} LSQ_API_CATCH

// Splice-site usage and read-through per junction of a read file (include/lesseq_hip.h): the device arrays handed to lsq_sites.hip
int lsq_ss_device(lsq_ctx *c, lsq_ss_index *ix, const char *read_format, const char *path, uint32_t min_overhang, lsq_ss_table **out) LSQ_API_TRY {
	if (!c || !ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	return table_of_file(c, ix, read_format, path, out, [&](const ParsedReads &R, lsq_ss_table &t) { return ss_device_reads(c, *ix, R, min_overhang, t); });
} LSQ_API_CATCH

// Intron retention of a read file (include/lesseq_hip.h): the device arrays handed to lsq_retention.hip
int lsq_ir_device(lsq_ctx *c, lsq_ir_index *ix, const char *read_format, const char *path, uint32_t min_overhang, lsq_ir_table **out) LSQ_API_TRY {
	if (!c || !ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	return table_of_file(c, ix, read_format, path, out, [&](const ParsedReads &R, lsq_ir_table &t) { return ir_device_reads(c, *ix, R, min_overhang, t); });
} LSQ_API_CATCH

// The per-base depth of a read file (include/lesseq_hip.h): the device arrays handed to lsq_cov.hip
int lsq_cov_device(lsq_ctx *c, lsq_cov_index *ix, const char *read_format, const char *path, int strand, uint32_t min_depth, lsq_cov_table **out) LSQ_API_TRY {
	if (!c || !ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	if (!cov_strand_ok(strand)) return fail(LSQ_E_ARG, "strand must be 0, '+' or '-'");
	return table_of_file(c, ix, read_format, path, out, [&](const ParsedReads &R, lsq_cov_table &t) {
		t.min_depth = min_depth;
		const int rc = cov_device_reads(c, *ix, R, strand, min_depth, t);
		if (!rc) cov_finish_table(*ix, t);
		return rc;
	});
} LSQ_API_CATCH

// The reads per exon bin and per gene of a read file (include/lesseq_hip.h): the device arrays handed to lsq_exonbins.hip
int lsq_xb_device(lsq_ctx *c, lsq_xb_index *ix, const char *read_format, const char *path, lsq_xb_table **out) LSQ_API_TRY {
	if (!c || !ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	return table_of_file(c, ix, read_format, path, out, [&](const ParsedReads &R, lsq_xb_table &t) { return xb_device_reads(c, *ix, R, t); });
} LSQ_API_CATCH

// The junction reads per event form of a read file (include/lesseq_hip.h): the device arrays handed to lsq_psi.hip
int lsq_ps_device(lsq_ctx *c, lsq_ps_index *ix, const char *read_format, const char *path, uint32_t min_overhang, lsq_ps_table **out) LSQ_API_TRY {
	if (!c || !ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	if (min_overhang < 1) return fail(LSQ_E_ARG, "min_overhang must be at least 1");
	return table_of_file(c, ix, read_format, path, out, [&](const ParsedReads &R, lsq_ps_table &t) { return ps_device_reads(c, *ix, R, min_overhang, t); });
} LSQ_API_CATCH

// The junction and exon-body reads per event form of a read file (include/lesseq_hip.h): the device arrays handed to lsq_evidence.hip
int lsq_fe_device(lsq_ctx *c, lsq_fe_index *ix, const char *read_format, const char *path, uint32_t min_overhang, uint32_t min_body, lsq_fe_table **out) LSQ_API_TRY {
	if (!c || !ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	if (min_overhang < 1) return fail(LSQ_E_ARG, "min_overhang must be at least 1");
	if (min_body < 1) return fail(LSQ_E_ARG, "min_body must be at least 1");
	return table_of_file(c, ix, read_format, path, out, [&](const ParsedReads &R, lsq_fe_table &t) { return fe_device_reads(c, *ix, R, min_overhang, min_body, t); });
} LSQ_API_CATCH

// Which library type a read file is (include/lesseq_hip.h): the device arrays handed to lsq_libtype.hip
int lsq_lt_device(lsq_ctx *c, lsq_lt_index *ix, const char *read_format, const char *path, lsq_lt_table **out) LSQ_API_TRY {
	if (!c || !ix || !read_format || !path || !out) return fail(LSQ_E_ARG, "null argument");
	return table_of_file(c, ix, read_format, path, out, [&](const ParsedReads &R, lsq_lt_table &t) { return lt_device_reads(c, *ix, R, t); });
} LSQ_API_CATCH

int lsq_last_sam_paths(const lsq_ctx *c, uint32_t *lines_listed, uint32_t *all_slow) {
	if (!c) return LSQ_E_ARG;
	if (lines_listed) *lines_listed = c->sam_lines_listed;
	if (all_slow) *all_slow = c->sam_all_slow;
	return LSQ_OK;
}

} // extern "C"

// lsq_internal.hpp: whether the device parses files of this format from their own bytes (the executables ask before they stage one)
bool lsq::device_read_format(const char *name) {
	for (const ReadFormat &f : READ_FORMATS) if (strcmp(name, f.name) == 0) return true;
	return false;
}
