// SAM_SINGLE parsed on the device; not a public header.
// Needs: lsq_mrf_device.hpp (the tile's LDS, the dictionary look-ups, the byte tests; through it lsq_route.hpp, lsq_text.hpp and
// lsq_readjob.hpp), lsq_sam_line.hpp (the shared splitter).  Gives: the routing kernels and the format's front end for the loader chain
// (sam_prepare, sam_launch, sam_record), the count / write kernels of lsq_mrf_parse_device, and the record filters (SamOpts, sam_opts)
// the BAM parser shares.
//
// The text lies in HBM as lsq_text.hip staged it and its newline-count pass has numbered its tiles (lsq_text.hpp), as for MRF.  What differs is the shape of a line: a record with SEQ and QUAL is 200-400 bytes of which only the
// first six fields, 40-90 bytes, are ever read, so a 7 680-byte tile holds about 25 lines.  Hence another form than MRF's:
//   - a line belongs to the tile in which it STARTS (MRF: ends), so that its head is in the tile or the 512 bytes staged
//     behind it and never in the tile before;
//   - the newline scan is byte-parallel in registers, 16 bytes a lane, every lane of the workgroup (the bulk of the bytes
//     -- SEQ, QUAL, tags -- is touched by that scan only, once);
//   - a lane a line then walks the line's HEAD only: the six field bounds from the TABs of its 8-byte words
//     (sam_field_bounds_lds), then FLAG, MAPQ, POS, RNAME and CIGAR byte by byte (sam_split_fields, the code the host parser
//     runs); neighbouring lines go to different waves of the workgroup.
// A head the tile kernel does not hold -- longer than SAM_HEAD_MAX bytes, or running past the staged window -- is not
// settled there: the line goes on a list and lsq_sam_route_lines_kernel runs the same splitter over the bytes in HBM (a CIGAR
// of hundreds of operations, a very long RNAME or QNAME).  Should that list run over, every tile goes through the tile kernel
// once more in its byte-walking form (HBM views for every line).
//   lsq_sam_route_kernel<false>   every tile: heads in LDS; lists what it does not hold
//   lsq_sam_route_kernel<true>    every tile, every line over HBM bytes (list run over; LSQ_SAM_SLOW)
//   lsq_sam_route_lines_kernel    the listed lines
//   lsq_sam_count_kernel / lsq_sam_write_kernel   the same walk for lsq_mrf_parse_device("SAM_SINGLE"): blocks per line,
//                                 then the parsed arrays, around two prefix sums
// The format's front end (sam_launch, at the end of this file) launches the route kernels; READ_FORMATS (lsq_readfile.hip) the other two.
// Line numbers: the ordinal of the newline ahead of a line (tile base + place in the tile) is the line's 0-based number;
// "read-<k>" counts every line from 1, so has_header = 0 and first_line = 1 for a whole file.
#pragma once
#include "lsq_mrf_device.hpp"
#include "lsq_sam_line.hpp"

namespace {

constexpr unsigned SAM_TAIL = MRF_LB;               // bytes behind the tile that are staged with it
constexpr unsigned SAM_HEAD_MAX = 256;              // bytes of a line (through the CIGAR field) the tile kernel walks at most
static_assert(SAM_HEAD_MAX <= SAM_TAIL, "a head that starts in the tile's last byte lies in the staged window");

struct SamOpts { unsigned skip_flags, min_mapq; };

// The lines that START in this workgroup's tile: fn(i, start, n, whole) once per data line by the lane that owns it -- i its
// 0-based index among the data lines, start its first byte in the tile, n its bytes inside the staged window (the tile
// and SAM_TAIL bytes behind it, S.text), whole: the window holds the line's end.  Lines without a '\n' are never seen.
template <class Fn>
__device__ inline void sam_tile_lines(MrfTileLds &S, const unsigned tile, const MrfText &X, Fn &&fn) {
	const unsigned tid = threadIdx.x;
	const unsigned long long t0 = (unsigned long long)tile * TEXT_TILE;
	TextTileNl N;
	N.load(S.text, X.text, X.len, t0);
	// the bytes behind the tile and the first newline among them (wave 0)
	if (tid < 64u) {
		unsigned first = 0xFFFFu;
		if (tid < SAM_TAIL / 16u) {
			unsigned valid = 0;
			const uint4 v = text_load16(X.text, X.len, t0 + TEXT_TILE + tid * 16ull, valid);
			*reinterpret_cast<uint4 *>(&S.text[TEXT_TILE + tid * 16u]) = v;
			const unsigned b = text_newline_bits16(v, valid);
			if (b) first = TEXT_TILE + tid * 16u + ((unsigned)__ffs((int)b) - 1u);
		}
		for (unsigned d = 1; d < 64u; d <<= 1) first = min(first, (unsigned)__shfl_xor((int)first, (int)d));
		if (tid == 0) S.first_start = first == 0xFFFFu ? -1ll : (long long)first;
	}
	// a line starts at the tile's first byte when the byte ahead of it is a newline (or there is none)
	const bool lead = t0 == 0 || X.text[t0 - 1] == '\n';
	N.number(S.nl);                                                 // (its barriers also publish S.text and S.first_start)
	const unsigned nt = N.nt;
	const unsigned long long g0 = X.tile_base[tile];                // newlines ahead of the tile = the number of a line that starts at its first byte
	const unsigned win = (unsigned)min((unsigned long long)(TEXT_TILE + SAM_TAIL), X.len - t0);       // bytes of the window that are text
	// line v of the tile: v = 0 starts at the tile's first byte (if `lead`), v = j + 1 behind the tile's newline j
	for (unsigned rb = 0; rb <= nt; rb += TEXT_NLCAP) {
		N.round(S.nl, rb);
		const unsigned v_end = min(nt + 1u, rb + TEXT_NLCAP);
		// (neighbouring lines go to different waves: a tile of records holds ~25 lines, and one wave walking them all while three
		// wait is what a lane a line in thread order comes to)
		for (unsigned v = rb + (tid & 63u) * 4u + (tid >> 6); v < v_end; v += 256u) {
			unsigned start;
			if (v == 0) { if (!lead) continue; start = 0; }
			else start = (v - 1u >= rb ? (unsigned)S.nl.nlpos[v - 1u - rb] : S.nl.carry) + 1u;
			if (start >= TEXT_TILE) continue;                      // (the tile's last byte is a newline: the line behind it is the next tile's)
			const unsigned long long g = g0 + v;
			if ((X.has_header && g == 0) || g - X.has_header >= X.n_lines) continue;        // the header; a last line without '\n'
			bool whole = true;
			unsigned end;
			if (v < nt) end = S.nl.nlpos[v - rb];
			else if (S.first_start >= 0) end = (unsigned)S.first_start;
			else { end = win; whole = false; }
			fn(g - X.has_header, start, end - start, whole);
		}
	}
}

// lsq::sam_field_bounds over a head in the staged window, eight bytes a step instead of one: the TABs of an aligned 8-byte
// word by the exact zero-byte test on word ^ 0x0909..., bytes ahead of the head and behind it masked off.  Same result as
// the shared walk on MrfLdsView{text + start, n} (the tests hold the two together through the host parser).
__device__ inline int sam_field_bounds_lds(const unsigned char *text, const unsigned start, const unsigned n, const bool whole, unsigned *b) {
	unsigned k = 0;
	b[0] = 0;
	const unsigned end = start + n;
	for (unsigned a = start & ~7u; a < end; a += 8u) {
		const uint2 w = *reinterpret_cast<const uint2 *>(text + a);
		unsigned m = fp_pack4(fp_eq_bytes(w.x, 0x09090909u)) | (fp_pack4(fp_eq_bytes(w.y, 0x09090909u)) << 4);
		if (a < start) m &= 0xFFu << (start - a);
		if (a + 8u > end) m &= (1u << (end - a)) - 1u;
		while (m) {
			const unsigned j = (unsigned)__ffs((int)m) - 1u; m &= m - 1u;
			b[++k] = a + j - start + 1u;
			if (k == 6u) return lsq::SAM_BOUNDS_OK;
		}
	}
	if (!whole) return lsq::SAM_BOUNDS_SHORT_VIEW;
	if (k < 5u) return lsq::SAM_BOUNDS_SHORT_LINE;
	b[6] = n + 1u;
	return lsq::SAM_BOUNDS_OK;
}

// a line whose bytes lie in HBM from `start` on: its view up to the newline (there is one: lines without are never seen)
__device__ inline lsq::MrfView sam_hbm_line(const MrfText &X, const unsigned long long start) {
	unsigned long long e = start;
	while (e < X.len && X.text[e] != '\n') ++e;
	return lsq::MrfView{reinterpret_cast<const char *>(X.text) + start, (size_t)(e - start)};
}

// one record through the containment filter and the merge, as mrf_route_line does for an MRF line
// (STRANDED, lsq_route.hpp: the splitter hands over the strand of the fragment's first mate; the library turns that into t)
// (the stranded form's two arguments -- the `lib` word and the kernel's tally -- are a parameter pack, empty in the unstranded form, as
// the kernels' own: with them in its signature the unstranded helper lay beyond the inliner's threshold, and the byte-walking kernel
// called sam_route_whole_line where it had held it)
template <bool STRANDED, class V, class... Lib>
__device__ inline void sam_route_fields(const MrfText &X, const SamOpts Q, const MrfDict &D, const unsigned long long *lds_strand, const RouteTables &T, const RouteChrom *chroms,
                                        const RouteOut &O, unsigned long long *err, const unsigned long long i, const V line, const typename V::index_type *b, Lib... lib_arg) {
	const unsigned lib = route_helper_lib(lib_arg...);
	const long long LIM = 1ll << 30;
	ReadAcc A;
	ReadBig B;
	A.init();
	LocProbe P;
	P.chrom = -1; P.bin = 0;
	unsigned cid = MRF_NOCHROM, sid = 0, t = 0;
	bool looked = false;
	const int verdict = lsq::sam_split_fields(line, b, Q.skip_flags, Q.min_mapq, [&](const V chr, const bool minus, const int64_t start, const int64_t end, int64_t, int64_t) {
		if (!looked) {
			// (one RNAME and one strand a record)
			looked = true;
			cid = mrf_chrom_lookup(D, chr);
			if constexpr (STRANDED) { t = route_transcript(lib, minus ? 1u : 0u); if (cid != MRF_NOCHROM) cid = route_table(cid, t); }
			const char sc = (STRANDED ? t != 0u : minus) ? '-' : '+';
			sid = mrf_strand_slot(lds_strand, D.strand_tab, lsq::MrfView{&sc, 1}, err);
		}
		const long long s0 = start - 1, e0 = end;
		if (cid >= T.n_chrom || e0 >= LIM || s0 >= LIM) return;
		if (!route_covered(T, chroms[cid], (int)cid, (int)s0, (int)e0, P)) return;
		A.add(B, cid, sid, (int)s0, (int)e0);
	}, STRANDED);
	if (verdict == lsq::SAM_MALFORMED) { atomicMin(&err[0], X.first_line + i); O.key[i] = ROUTE_KEY_DROPPED; return; }
	if (verdict != lsq::SAM_READ) { O.key[i] = ROUTE_KEY_DROPPED; return; }
	if constexpr (STRANDED) route_tally_arg(lib_arg...)->note(t, A.kept());
	A.finish(B, T, chroms, P, O, (unsigned)i);
}
template <bool STRANDED, class V, class... Lib>
__device__ inline void sam_route_whole_line(const MrfText &X, const SamOpts Q, const MrfDict &D, const unsigned long long *lds_strand, const RouteTables &T, const RouteChrom *chroms,
                                            const RouteOut &O, unsigned long long *err, const unsigned long long i, const V line, Lib... lib_arg) {
	typename V::index_type b[7];
	if (line.n >= 1 && line.p[0] == '@') { O.key[i] = ROUTE_KEY_DROPPED; return; }
	if (lsq::sam_field_bounds(line, true, b) != lsq::SAM_BOUNDS_OK) { atomicMin(&err[0], X.first_line + i); O.key[i] = ROUTE_KEY_DROPPED; return; }
	sam_route_fields<STRANDED>(X, Q, D, lds_strand, T, chroms, O, err, i, line, b, lib_arg...);
}

// Waves a SIMD the compiler is asked to leave room for in the tile kernel.  Left alone (0) it takes 181 registers -- two
// workgroups a compute unit -- and the walk, a chain of LDS and L2 round trips per line, waits: 15.3 ms for 10 M records (2.56 GB);
// held to 128 registers (4) 8.4 ms; to 80 (6, with 336 bytes a lane in the private segment) 7.1 ms (same box, tools/sam_bench.py).
#ifndef LSQ_SAM_WAVES
#define LSQ_SAM_WAVES 6
#endif
#if LSQ_SAM_WAVES
#define LSQ_SAM_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(LSQ_SAM_WAVES)))
#else
#define LSQ_SAM_WAVES_ATTR
#endif

template <bool ALL_HBM, bool STRANDED, class... Lib>
__global__ void __launch_bounds__(256) LSQ_SAM_WAVES_ATTR lsq_sam_route_kernel(MrfText X, SamOpts Q, MrfDict G, RouteTables T, RouteOut O, unsigned long long *err, MrfHandOff H, unsigned n_tiles, Lib... lib_arg) {
	const unsigned lib = route_lib_arg(lib_arg...);
	__shared__ MrfTileLds S;
	LibTally L;
	L.init();
	const MrfDict D = mrf_stage_dict(S, G);
	const RouteChrom *chroms = route_stage_chroms(T, S.chrom);
	const mrf_lds_cptr lds_text = (mrf_lds_cptr)(const char *)S.text;
	for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		const unsigned long long t0 = (unsigned long long)tile * TEXT_TILE;
		sam_tile_lines(S, tile, X, [&](const unsigned long long i, const unsigned start, const unsigned n, const bool whole) {
			if constexpr (ALL_HBM) {
				if constexpr (STRANDED) [[clang::always_inline]] sam_route_whole_line<true>(X, Q, D, S.strand, T, chroms, O, err, i, sam_hbm_line(X, t0 + start), lib, &L);
				// (held here, as it was before the helper had a stranded sibling: left to itself the inliner now calls it from this kernel)
				else [[clang::always_inline]] sam_route_whole_line<false>(X, Q, D, S.strand, T, chroms, O, err, i, sam_hbm_line(X, t0 + start));
			}
			else {
				if (n >= 1u && lds_text[start] == '@') { O.key[i] = ROUTE_KEY_DROPPED; return; }
				const MrfLdsView head{lds_text + start, n < SAM_HEAD_MAX ? n : SAM_HEAD_MAX};
				unsigned b[7];
				const int fb = sam_field_bounds_lds(S.text, start, head.n, whole && n <= SAM_HEAD_MAX, b);
				if (fb == lsq::SAM_BOUNDS_SHORT_VIEW) {
					// not a head this kernel holds: the shared splitter takes the line from HBM
					const unsigned at = atomicAdd(&H.counts[1], 1u);
					if (at < H.line_cap) H.lines[at] = MrfLongLine{i, t0 + start, ~0ull}; else H.counts[2] = 1u;
				}
				else if (fb == lsq::SAM_BOUNDS_SHORT_LINE) { atomicMin(&err[0], X.first_line + i); O.key[i] = ROUTE_KEY_DROPPED; }
				else if constexpr (STRANDED) sam_route_fields<true>(X, Q, D, S.strand, T, chroms, O, err, i, head, b, lib, &L);
				else sam_route_fields<false>(X, Q, D, S.strand, T, chroms, O, err, i, head, b);
			}
		});
		__syncthreads();
	}
	if constexpr (STRANDED) L.flush(O);
}

// the listed lines, one lane each, straight from HBM
template <bool STRANDED, class... Lib>
__global__ void __launch_bounds__(256) lsq_sam_route_lines_kernel(MrfText X, SamOpts Q, MrfDict G, RouteTables T, RouteOut O, unsigned long long *err, MrfHandOff H, Lib... lib_arg) {
	const unsigned lib = route_lib_arg(lib_arg...);
	const unsigned n = min(H.counts[1], H.line_cap);
	LibTally LT;
	LT.init();
	for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
		const MrfLongLine L = H.lines[t];
		if constexpr (STRANDED) sam_route_whole_line<true>(X, Q, G, nullptr, T, T.chrom, O, err, L.i, sam_hbm_line(X, L.start), lib, &LT);
		else sam_route_whole_line<false>(X, Q, G, nullptr, T, T.chrom, O, err, L.i, sam_hbm_line(X, L.start));
	}
	if constexpr (STRANDED) LT.flush(O);
}

// ---- lsq_mrf_parse_device("SAM_SINGLE"): pass 1, blocks per data line (0 for lines that make no read), first malformed line
__global__ void __launch_bounds__(256) lsq_sam_count_kernel(MrfText X, SamOpts Q, unsigned *line_nb, unsigned long long *err) {
	__shared__ MrfTileLds S;
	const unsigned long long t0 = (unsigned long long)blockIdx.x * TEXT_TILE;
	sam_tile_lines(S, blockIdx.x, X, [&](const unsigned long long i, const unsigned start, unsigned, bool) {
		unsigned nb = 0;
		const int verdict = lsq::sam_split_line(sam_hbm_line(X, t0 + start), Q.skip_flags, Q.min_mapq, [&](lsq::MrfView, bool, int64_t, int64_t, int64_t, int64_t) { ++nb; });
		if (verdict == lsq::SAM_MALFORMED) atomicMin(&err[0], X.first_line + i);
		line_nb[i] = verdict == lsq::SAM_READ ? nb : 0u;
	});
}

// pass 2: every read's blocks to their place (as lsq_mrf_write_kernel)
// (mate_strand: stranded events -- the strand written is that of the fragment's first mate, as lsq_sam_parse writes it)
__global__ void __launch_bounds__(256) lsq_sam_write_kernel(MrfText X, SamOpts Q, const unsigned *line_nb, const unsigned long long *rd_idx, const unsigned long long *bk_off,
                                                            MrfDict G, MrfOut O, unsigned long long *err, unsigned mate_strand) {
	__shared__ MrfTileLds S;
	const MrfDict D = mrf_stage_dict(S, G);
	const long long LIM = 1ll << 30;
	const unsigned long long t0 = (unsigned long long)blockIdx.x * TEXT_TILE;
	sam_tile_lines(S, blockIdx.x, X, [&](const unsigned long long i, const unsigned start, unsigned, bool) {
		const unsigned nb = line_nb[i];
		const unsigned long long r = rd_idx[i], o = bk_off[i];
		if (i + 1 == X.n_lines) O.blk_off[r + (nb ? 1u : 0u)] = o + nb;
		if (!nb) return;
		O.blk_off[r] = o;
		O.line_no[r] = (unsigned)(X.first_line + i);
		unsigned long long w = o;
		(void)lsq::sam_split_line(sam_hbm_line(X, t0 + start), Q.skip_flags, Q.min_mapq, [&](lsq::MrfView chr, bool minus, int64_t bstart, int64_t bend, int64_t, int64_t) {
			unsigned cid = mrf_chrom_lookup(D, chr);
			const char sc = minus ? '-' : '+';
			const unsigned sid = mrf_strand_slot(S.strand, D.strand_tab, lsq::MrfView{&sc, 1}, err);
			long long s0 = bstart - 1, e0 = bend;
			if (e0 >= LIM || s0 >= LIM) { cid = MRF_NOCHROM; s0 = 0; e0 = 0; }
			O.blk_start[w] = (int)s0; O.blk_end[w] = (int)e0;
			O.blk_chrom[w] = (unsigned short)cid; O.blk_strand[w] = (unsigned char)sid;
			++w;
		}, mate_strand != 0u);
	});
}

// ---- the front end (READ_FORMATS, lsq_readfile.hip)
static SamOpts sam_opts(const lsq_ctx *c) { return SamOpts{c->opt_sam_skip_flags, c->opt_sam_min_mapq}; }
static int sam_prepare(TextJob &J) {
	J.all_slow = getenv("LSQ_SAM_SLOW") != nullptr;       // (LSQ_SAM_SLOW: the tests run the byte-walking form over whole files with it)
	return LSQ_OK;
}
static void sam_launch(const TextJob &J, const RouteTables &RT, const RouteOut &O, hipStream_t s) {
	const SamOpts Q = sam_opts(J.c);
	// a workgroup a tile, as the MRF kernel is launched; the listed lines behind it
	const unsigned lib = lsq::route_lib(J.c);
	const dim3 lines_grid(std::min(J.H.line_cap / 256u + 1u, 1024u));
	if (!J.n_tiles) return;
	if (J.c->E->stranded()) {
		if (J.all_slow) hipLaunchKernelGGL((lsq_sam_route_kernel<true, true, unsigned>), dim3(J.n_tiles), dim3(256), 0, s, J.X, Q, J.D, RT, O, J.err, J.H, J.n_tiles, lib);
		else {
			hipLaunchKernelGGL((lsq_sam_route_kernel<false, true, unsigned>), dim3(J.n_tiles), dim3(256), 0, s, J.X, Q, J.D, RT, O, J.err, J.H, J.n_tiles, lib);
			hipLaunchKernelGGL((lsq_sam_route_lines_kernel<true, unsigned>), lines_grid, dim3(256), 0, s, J.X, Q, J.D, RT, O, J.err, J.H, lib);
		}
	} else if (J.all_slow) hipLaunchKernelGGL((lsq_sam_route_kernel<true, false>), dim3(J.n_tiles), dim3(256), 0, s, J.X, Q, J.D, RT, O, J.err, J.H, J.n_tiles);
	else {
		hipLaunchKernelGGL((lsq_sam_route_kernel<false, false>), dim3(J.n_tiles), dim3(256), 0, s, J.X, Q, J.D, RT, O, J.err, J.H, J.n_tiles);
		hipLaunchKernelGGL(lsq_sam_route_lines_kernel<false>, lines_grid, dim3(256), 0, s, J.X, Q, J.D, RT, O, J.err, J.H);
	}
}
static void sam_record(const TextJob &J) { J.c->sam_lines_listed = J.all_slow ? 0u : J.counts[1]; J.c->sam_all_slow = J.all_slow ? 1u : 0u; }

} // namespace
