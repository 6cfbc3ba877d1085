// MRF_SINGLE parsed on the device; not a public header.
// Needs: lsq_route.hpp (the routing pass's tables and the merge of a read's blocks), lsq_text.hpp (a text's newline tiles), lsq_mrf_line.hpp
// (the shared splitter), lsq_readjob.hpp (the kernels' parameter structs).  Gives: the three routing kernels and the format's front end
// for the loader chain (mrf_prepare, mrf_launch, mrf_record), the count / write kernels of lsq_mrf_parse_device, and the dictionary code
// (chromosome and strand look-ups) the SAM and BAM parsers share.
//
// The text lies in HBM as lsq_text.hip staged it, its newlines counted per tile (lsq_text.hpp).  A workgroup of the parse owns
// the lines that END in its tile and sees the tile and the 512 bytes before it.  The newline ordinal of a line (tile base from
// the prefix sum over the tile counts + its place in the tile) is its line number: the header and "read-<n>" fall out as in
// the reference (count/count.cpp:283,286,293-295).
//
// The parse IS the routing pass of the loader chain (lsq_ingest.hip: ingest_device): per line, every block goes through the containment
// filter and the merge as it is split off, and nothing but the routed read leaves the kernel -- no parsed array exists in HBM
// either.  Three kernels, launched by the format's front end (mrf_launch, at the end of this file):
//   lsq_mrf_route_fast_kernel   every tile: delimiter tables from byte-parallel zero-byte tests, lines walk table entries,
//                               a lane a block does the coordinates (eight-digit sums), the chromosome and strand (64-bit
//                               keys), the filter; settles every line of a read's usual shape and lists the others
//   lsq_mrf_route_kernel        the byte-walking form: the tile in LDS, a lane a line runs the SHARED SPLITTER
//                               (lsq_mrf_line.hpp -- the code the host parser runs) over LDS bytes; takes the tiles the fast
//                               kernel hands on, or whole files where that one does not apply
//   lsq_mrf_route_lines_kernel  the listed lines (another shape than a read's; began ahead of their tile's window): a lane
//                               a line, the shared splitter over the bytes in HBM
// lsq_mrf_parse_device (tests, tools) still wants the parsed arrays: the byte-walking tile walk run twice, counting
// (lsq_mrf_count_kernel) and writing (lsq_mrf_write_kernel) around two prefix sums.
//   - the first line is the header (count.cpp:283); a last line without '\n' is never seen (:285)
//   - '#' lines and the literal "AlignmentBlocks" consume a line number only (:288)
//   - a field that fails the cast stops the run: the FIRST such line in file order is reported
//   - chromosome names resolve against the events' chromosomes (64-bit keys of names up to seven bytes in LDS; a hash table
//     with byte-wise verification for the byte-walking kernels); strand strings against a 256-slot table seeded with the
//     strands already known, grown with atomicCAS (strings of at most 7 bytes; longer ones give LSQ_E_UNSUPPORTED -- use
//     lsq_mrf_parse)
// The SAM parser (lsq_sam_device.hpp) resolves chromosomes and strands with the dictionary code here.
#pragma once
#include "lsq_route.hpp"
#include "lsq_text.hpp"
#include "lsq_mrf_line.hpp"
#include "lsq_readjob.hpp"

namespace {      // (the device code of the unit that includes it: internal linkage)

constexpr unsigned MRF_LB = 512;                    // bytes ahead of the tile that are staged with it: a window of 8 KiB (tiles of 7 680 bytes) or 4 KiB (3 584)
constexpr unsigned long long MRF_NO_ERR = ~0ull;
constexpr unsigned long long STRAND_EMPTY = ~0ull;
constexpr unsigned long long STRAND_UNMATCHABLE = ~0ull - 1;
constexpr unsigned MRF_NOCHROM = 0xFFFFu;
constexpr unsigned MRF_DICT_LDS_SLOTS = 256;        // chromosome hash tables up to this size are staged in LDS (<= 64 chromosomes)
constexpr unsigned MRF_DICT_LDS_NAMES = 1024;

typedef const __attribute__((address_space(3))) char *mrf_lds_cptr;
typedef lsq::MrfViewT<mrf_lds_cptr, unsigned> MrfLdsView;

struct MrfTileLds {
	__align__(16) unsigned char text[MRF_LB + TEXT_TILE + 16];
	TextNlLds nl;
	long long first_start;                  // first byte of the first line that ends in the tile
	// the dictionaries, when they are small
	unsigned long long strand[256];
	unsigned d_hash[MRF_DICT_LDS_SLOTS], d_id[MRF_DICT_LDS_SLOTS], d_off[MRF_DICT_LDS_SLOTS / 4 + 1];
	char d_names[MRF_DICT_LDS_NAMES];
	__align__(16) RouteChrom chrom[ROUTE_CHROM_LDS];      // the routing pass's chromosome records (lsq_mrf_route_kernel)
};

// The lines that end in this workgroup's tile: fn(i, view) is called once per data line -- i its 0-based index among the
// data lines (with a header: the lines after the first), view the line's bytes without the newline -- by the lane that
// owns it.  view is an LDS view, or a plain one for a line that began more than MRF_LB bytes ahead of the tile.
template <bool DEFER, class Fn>
__device__ inline void mrf_tile_lines(MrfTileLds &S, const unsigned tile, const unsigned char *text, const unsigned long long len, const unsigned long long *tile_base,
                                      const unsigned has_header, MrfLongLine *long_lines, unsigned *n_long, const unsigned long_cap, unsigned *long_over, Fn &&fn) {
	const unsigned tid = threadIdx.x;
	const unsigned long long t0 = (unsigned long long)tile * TEXT_TILE;
	TextTileNl N;
	N.load(&S.text[MRF_LB], text, len, t0);
	if (tid < MRF_LB / 16u && t0 >= MRF_LB)
		*reinterpret_cast<uint4 *>(&S.text[tid * 16u]) = *reinterpret_cast<const uint4 *>(text + (t0 - MRF_LB) + tid * 16ull);
	N.number(S.nl);
	const unsigned nt = N.nt;
	if (nt == 0) return;                      // (uniform: every lane holds the same total)
	// the first line that ends here began after the last newline ahead of the tile
	if (tid < 64u) {
		long long found = -1;
		if (t0 > 0) {
			for (unsigned long long k = 0;; ++k) {
				const long long pos = (long long)t0 - 1 - (long long)(k * 64ull + tid);
				const bool hit = pos >= 0 && text[pos] == '\n';
				const unsigned long long m = __ballot(hit);
				if (m) { found = (long long)t0 - 1 - (long long)(k * 64ull + (unsigned)(__ffsll((long long)m) - 1)); break; }
				if ((long long)t0 - 1 - (long long)(k * 64ull + 63ull) <= 0) break;
			}
		}
		if (tid == 0) S.first_start = found + 1;
	}
	const unsigned long long g0 = tile_base[tile];
	const mrf_lds_cptr lds_text = (mrf_lds_cptr)(const char *)S.text;
	for (unsigned rb = 0; rb < nt; rb += TEXT_NLCAP) {
		N.round(S.nl, rb);                     // (its barrier also publishes S.first_start)
		const unsigned r_end = min(nt, rb + TEXT_NLCAP);
		for (unsigned j = rb + tid; j < r_end; j += 256u) {
			const unsigned long long g = g0 + j;                 // the newline's ordinal in the text = the 0-based number of the line it ends
			if (has_header && g == 0) continue;
			const int end_rel = (int)S.nl.nlpos[j - rb];
			long long start_rel;
			if (j == 0) start_rel = S.first_start - (long long)t0;
			else if (j > rb) start_rel = (long long)S.nl.nlpos[j - 1 - rb] + 1;
			else start_rel = (long long)S.nl.carry + 1;
			const unsigned long long i = g - has_header;
			if (start_rel >= -(long long)MRF_LB) fn(i, MrfLdsView{lds_text + (MRF_LB + (int)start_rel), (unsigned)(end_rel - (int)start_rel)});
			else if constexpr (DEFER) {
				const unsigned at = atomicAdd(n_long, 1u);
				if (at < long_cap) long_lines[at] = MrfLongLine{i, (unsigned long long)((long long)t0 + start_rel), (unsigned long long)((long long)end_rel - start_rel)}; else *long_over = 1u;
			}
			else fn(i, lsq::MrfView{reinterpret_cast<const char *>(text) + (t0 + start_rel), (size_t)((long long)end_rel - start_rel)});
		}
	}
}

// the dictionaries into LDS when they fit; returns the view the lookups use
__device__ inline MrfDict mrf_stage_dict(MrfTileLds &S, const MrfDict &G) {
	S.strand[threadIdx.x & 255u] = __hip_atomic_load(&G.strand_tab[threadIdx.x & 255u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	MrfDict D = G;
	if (G.mask < MRF_DICT_LDS_SLOTS && G.names_bytes <= MRF_DICT_LDS_NAMES && G.n_chrom <= MRF_DICT_LDS_SLOTS / 4) {
		for (unsigned i = threadIdx.x; i <= G.mask; i += 256u) { S.d_hash[i] = G.chrom_hash[i]; S.d_id[i] = G.chrom_id[i]; }
		for (unsigned i = threadIdx.x; i <= G.n_chrom; i += 256u) S.d_off[i] = G.name_off[i];
		for (unsigned i = threadIdx.x; i < G.names_bytes; i += 256u) S.d_names[i] = G.names[i];
		D.chrom_hash = S.d_hash; D.chrom_id = S.d_id; D.name_off = S.d_off; D.names = S.d_names;
	}
	__syncthreads();
	return D;
}

LSQ_HD inline unsigned mrf_fnv32(const char *p, size_t n) {
	unsigned h = 2166136261u;
	for (size_t j = 0; j < n; ++j) { h ^= (unsigned char)p[j]; h *= 16777619u; }
	return h ? h : 1u;
}

template <class V>
__device__ inline unsigned mrf_chrom_lookup(const MrfDict &D, V s) {
	typedef typename V::index_type Idx;
	unsigned h = 2166136261u;
	for (Idx j = 0; j < s.n; ++j) { h ^= (unsigned char)s.p[j]; h *= 16777619u; }
	if (h == 0) h = 1;
	for (unsigned i = h & D.mask;; i = (i + 1u) & D.mask) {
		const unsigned t = D.chrom_hash[i];
		if (t == 0) return MRF_NOCHROM;
		if (t != h) continue;
		const unsigned id = D.chrom_id[i];
		const unsigned a = D.name_off[id], b = D.name_off[id + 1];
		if ((Idx)(b - a) != s.n) continue;
		bool same = true;
		for (Idx j = 0; j < s.n; ++j) same = same && D.names[a + j] == s.p[j];
		if (same) return id;
	}
}

// strand strings of <= 7 bytes as one order-preserving 64-bit key (bytes big-endian, length last)
LSQ_HD inline unsigned long long mrf_strand_key(const char *p, size_t n) {
	unsigned long long k = (unsigned long long)n;
	for (size_t j = 0; j < n; ++j) k |= (unsigned long long)(unsigned char)p[j] << (56 - 8 * j);
	return k;
}

// the slot of a strand string: the workgroup's LDS copy of the table first (the strands every file has are there from the
// start), the table itself -- and a place in it for a new string -- otherwise
template <class V>
__device__ inline unsigned mrf_strand_slot(const unsigned long long *lds_tab, unsigned long long *tab, V s, unsigned long long *err) {
	if (s.n > 7) { atomicMax(&err[1], 1ull); return 0; }
	unsigned long long key = (unsigned long long)s.n;
	for (unsigned j = 0; j < (unsigned)s.n; ++j) key |= (unsigned long long)(unsigned char)s.p[j] << (56 - 8 * j);
	if (lds_tab) for (unsigned i = 0; i < 256; ++i) {
		const unsigned long long cur = lds_tab[i];
		if (cur == key) return i;
		if (cur == STRAND_EMPTY) break;
	}
	for (unsigned i = 0; i < 256; ++i) {
		const unsigned long long cur = __hip_atomic_load(&tab[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == key) return i;
		if (cur == STRAND_EMPTY) {
			const unsigned long long prev = atomicCAS(&tab[i], STRAND_EMPTY, key);
			if (prev == STRAND_EMPTY || prev == key) return i;
		}
	}
	atomicMax(&err[2], 1ull);
	return 0;
}

// ---- the parse that feeds the load-time filter (the product path): per line, every block through the covered regions and
// the merge as it is split off; the routed read to key[i] / rec[i], i the data line's index
// t of an MRF strand column: exactly "+" or "-" (lsq_route.hpp)
template <class V>
__device__ inline unsigned mrf_transcript(const unsigned lib, const V strand) {
	if (strand.n != 1 || (strand.p[0] != '+' && strand.p[0] != '-')) return ROUTE_NO_STRAND;
	return route_transcript(lib, strand.p[0] == '-' ? 1u : 0u);
}
// (STRANDED: the read's transcript strand is that of its first block's strand column; every block of it goes by that one)
template <bool STRANDED, class V>
__device__ inline void mrf_route_line(const MrfText &X, const MrfDict &D, const unsigned long long *lds_strand, const RouteTables &T, const RouteChrom *chroms, const RouteOut &O,
                                      unsigned long long *err, const unsigned long long i, const V line, const unsigned lib, LibTally &L) {
	const long long LIM = 1ll << 30;
	if (lsq::mrf_line_is_skipped(line)) { O.key[i] = ROUTE_KEY_DROPPED; return; }
	ReadAcc A;
	ReadBig B;
	A.init();
	LocProbe P;
	P.chrom = -1; P.bin = 0;
	unsigned t = 3u;                        // (STRANDED; 3: no block seen yet)
	const bool ok = lsq::mrf_split_line(line, [&](const V chr, const V strand, const int64_t start, const int64_t end) {
		unsigned cid = mrf_chrom_lookup(D, chr);
		const long long s0 = start - 1, e0 = end;
		if constexpr (STRANDED) {
			if (t == 3u) t = mrf_transcript(lib, strand);
			if (t >= ROUTE_NO_STRAND || cid == MRF_NOCHROM) return;
			cid = route_table(cid, t);
		}
		if (cid >= T.n_chrom || s0 <= -LIM || e0 >= LIM || s0 >= LIM || e0 <= -LIM) return;
		if (!route_covered(T, chroms[cid], (int)cid, (int)s0, (int)e0, P)) return;
		if constexpr (STRANDED) { const char tc = t ? '-' : '+'; A.add(B, cid, mrf_strand_slot(lds_strand, D.strand_tab, lsq::MrfView{&tc, 1}, err), (int)s0, (int)e0); }
		else A.add(B, cid, mrf_strand_slot(lds_strand, D.strand_tab, strand, err), (int)s0, (int)e0);
	});
	if (!ok) { atomicMin(&err[0], X.first_line + i); O.key[i] = ROUTE_KEY_DROPPED; return; }
	if constexpr (STRANDED) { if (t != 3u) L.note(t, A.kept()); }
	A.finish(B, T, chroms, P, O, (unsigned)i);
}

template <bool STRANDED, class... Lib>
__global__ void __launch_bounds__(256) lsq_mrf_route_kernel(MrfText X, MrfDict G, RouteTables T, RouteOut O, unsigned long long *err, MrfHandOff H, unsigned n_tiles, unsigned listed, Lib... lib_arg) {
	const unsigned lib = route_lib_arg(lib_arg...);
	__shared__ MrfTileLds S;
	const MrfDict D = mrf_stage_dict(S, G);
	const RouteChrom *chroms = route_stage_chroms(T, S.chrom);
	const unsigned n = listed ? min(H.counts[0], H.tile_cap) : n_tiles;
	LibTally L;
	L.init();
	for (unsigned t = blockIdx.x; t < n; t += gridDim.x) {
		const unsigned tile = listed ? H.tiles[t] : t;
		mrf_tile_lines<true>(S, tile, X.text, X.len, X.tile_base, X.has_header, H.lines, H.counts + 1, H.line_cap, H.counts + 2, [&](const unsigned long long i, const MrfLdsView line) {
			mrf_route_line<STRANDED>(X, D, S.strand, T, chroms, O, err, i, line, lib, L);
		});
		__syncthreads();
	}
	if constexpr (STRANDED) L.flush(O);
}
// listed lines, one lane each, straight from HBM.  A line listed without its start (n = ~0: it began ahead of a tile's
// window) is walked back to the newline before it first.
template <bool STRANDED, class... Lib>
__global__ void __launch_bounds__(256) lsq_mrf_route_lines_kernel(MrfText X, MrfDict G, RouteTables T, RouteOut O, unsigned long long *err, MrfHandOff H, Lib... lib_arg) {
	const unsigned lib = route_lib_arg(lib_arg...);
	const unsigned n = min(H.counts[1], H.line_cap);
	LibTally LT;
	LT.init();
	for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
		MrfLongLine L = H.lines[t];
		if (L.n == ~0ull) {
			// L.start: the line's newline
			unsigned long long a = L.start;
			while (a > 0 && X.text[a - 1] != '\n') --a;
			L.n = L.start - a; L.start = a;
		}
		mrf_route_line<STRANDED>(X, G, nullptr, T, T.chrom, O, err, L.i, lsq::MrfView{reinterpret_cast<const char *>(X.text) + L.start, (size_t)L.n}, lib, LT);
	}
	if constexpr (STRANDED) LT.flush(O);
}

// ---- the fast kernel.  A workgroup takes a window of 8 KiB of text -- a tile of 7 680 bytes and the 512 ahead of it -- 32
// bytes a lane, in registers: three exact zero-byte tests (word ^ 0x0A.., ^ 0x3A.., ^ 0x2C..) give every lane the newlines,
// colons and commas among its bytes as bit masks; one prefix sum over the lanes' counts numbers them; the lanes write the
// window's delimiters, in text order, into an LDS table (position | kind) and, per newline, the index of its entry.  Then one
// lane per line that ends in the tile walks its entries instead of its bytes.  A block whose next four delimiters are colons
// is exactly what the reference's find / substr walk (count/count.cpp:297-326) takes it for: chr = [block start, colon 1),
// strand, start, end = the stretches between the colons, the next block behind the first comma after colon 4 (colons in
// between -- the query fields -- are passed over).  The two coordinates are at most nine decimal digits (what
// lexical_cast<long> takes without a sign, and no overflow possible): eight bytes that END at the delimiter, bytes ahead of
// the field replaced by '0', summed pairwise (1 x 10 + 1, 2 x 100 + 2, 4 x 10000 + 4 digits) -- and a ninth digit.  The
// chromosome (at most seven bytes) is looked up by its bytes as one 64-bit key in an LDS table, the strand likewise.
// Whatever does not fit this shape -- fewer than four colons before the next comma or the line's end, a sign or a stray
// byte in a coordinate, ten digits, a chromosome or strand of eight bytes or more, a line that starts ahead of the window
// -- is not decided here: the line goes on a list and lsq_mrf_route_lines_kernel runs the shared splitter on it.
// Waves a SIMD the compiler is asked to leave room for.  Left alone it takes 156 registers (three waves) and the kernel, a chain of
// LDS and L2 round trips per line, waits: 10.1 ms per C3 file; held to 128 (four waves, with spills) 13.5; asked for five or more
// it settles at 75 registers -- six waves, what the 23 KB of LDS tables allow -- with the per-line state it cannot keep in registers
// in the private segment (L1-resident): 6.4 ms (same box, tools/ingest_bench.py).
#ifndef LSQ_FAST_WAVES
#define LSQ_FAST_WAVES 6
#endif
#if LSQ_FAST_WAVES
#define LSQ_FAST_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(LSQ_FAST_WAVES)))
#else
#define LSQ_FAST_WAVES_ATTR
#endif
constexpr unsigned FP_WIN = MRF_LB + TEXT_TILE;          // 8 192
constexpr unsigned FP_PAD = 16;                          // bytes of LDS ahead of the window (a coordinate's eight bytes may begin there)
constexpr unsigned FP_LANE = FP_WIN / 256;               // window bytes a lane takes: 32 or 16
constexpr unsigned FP_DCAP = FP_WIN * 5 / 16, FP_NCAP = FP_WIN / 8;       // delimiters / newlines a window may hold (8 KiB of reads: ~1 500 / ~220)
constexpr unsigned FP_BCAP = FP_WIN >= 8192 ? 384 : 256;                        // blocks of one round of 256 lines (reads: ~310); a line whose blocks find no room goes to the list
constexpr unsigned FP_STRANDS = 32;                      // strand keys kept in LDS (the table's first slots: the strands every file has)
constexpr unsigned FP_KIND_SHIFT = 13;                   // entry: position in the window | kind << 13 (0 colon, 1 comma, 2 newline)
constexpr unsigned FP_DICT = 256;

struct MrfFastDict {
	const unsigned long long *ckey;       // FP_DICT slots: the chromosome's bytes as a key (mrf_strand_key), 0 = empty
	const unsigned short *cid;
	unsigned usable;                       // every chromosome name has a slot (names of eight bytes and more have none: their lines go to the list)
};
__host__ __device__ inline unsigned mrf_key_slot(unsigned long long k) {
	unsigned x = (unsigned)k ^ (unsigned)(k >> 32);
	x ^= x >> 16; x ^= x >> 8;
	return x & (FP_DICT - 1u);
}

struct MrfFastLds {
	__align__(16) unsigned char text[FP_PAD + FP_WIN + 16];
	__align__(8) unsigned short delim[FP_DCAP + 8];
	unsigned short nl_dord[FP_NCAP];
	unsigned scan4[4];
	unsigned nl_ahead;                      // newlines in the 512 bytes ahead of the tile
	unsigned n_blk;                         // blocks listed in this round
	__align__(16) uint4 blk[FP_BCAP];       // a block: its five field bounds on the way in, what became of it on the way out
	__align__(8) unsigned long long strand[FP_STRANDS];
	unsigned long long ckey[FP_DICT];
	unsigned short cid[FP_DICT];
	__align__(16) RouteChrom chrom[ROUTE_CHROM_LDS];
};

// 0x80 in every byte of w that equals c
__device__ inline unsigned fp_eq_bytes(const unsigned w, const unsigned c4) {
	const unsigned x = w ^ c4;
	return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
__device__ inline unsigned fp_pack4(const unsigned z) { return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u); }

// the decimal number in the eight bytes of `w` (first byte lowest), the last `len` of them digits (1 <= len <= 8): bytes ahead of the
// field count as '0'.  false when a byte of the field is no digit.
__device__ inline bool fp_number8(const unsigned long long w, const unsigned len, unsigned &out) {
	unsigned lo = (unsigned)w, hi = (unsigned)(w >> 32);                     // lo: the four bytes ahead, hi: the last four
	const unsigned keep_hi = len >= 4u ? 0xFFFFFFFFu : 0xFFFFFFFFu << (8u * (4u - len));
	const unsigned keep_lo = len >= 8u ? 0xFFFFFFFFu : (len > 4u ? 0xFFFFFFFFu << (8u * (8u - len)) : 0u);
	hi = (hi & keep_hi) | (0x30303030u & ~keep_hi);
	lo = (lo & keep_lo) | (0x30303030u & ~keep_lo);
	// every byte of the eight in '0'..'9': on the low seven bits of each byte, + 0x46 must not reach the top bit (<= '9') and + 0x50 must (>= '0')
	const unsigned lo7 = lo & 0x7F7F7F7Fu, hi7 = hi & 0x7F7F7F7Fu;
	const bool digits = ((lo | hi) & 0x80808080u) == 0u && (((lo7 + 0x46464646u) | (hi7 + 0x46464646u)) & 0x80808080u) == 0u &&
	                    (((lo7 + 0x50505050u) & (hi7 + 0x50505050u)) & 0x80808080u) == 0x80808080u;
	unsigned a = lo - 0x30303030u, b = hi - 0x30303030u;       // (no borrow between bytes when they are digits; otherwise the result is not used)
	// first byte = most significant digit: pairs, then fours
	a = (a * 10u + (a >> 8)) & 0x00FF00FFu; b = (b * 10u + (b >> 8)) & 0x00FF00FFu;
	a = (__umul24(a & 0xFFFFu, 100u) + (a >> 16)); b = (__umul24(b & 0xFFFFu, 100u) + (b >> 16));
	out = __umul24(a, 10000u) + b;
	return digits;
}

// (STRANDED, lsq_route.hpp: step (2) filters a block against the tables of its own strand column's t and notes t for the blocks it
// passes over; step (3) takes the read's t from its first block, and a line whose blocks disagree goes to the list, where
// mrf_route_line settles it)
template <bool STRANDED, class... Lib>
__global__ void __launch_bounds__(256) LSQ_FAST_WAVES_ATTR lsq_mrf_route_fast_kernel(MrfText X, MrfDict G, MrfFastDict FD, RouteTables T, RouteOut O, unsigned long long *err, MrfHandOff H, unsigned n_tiles, Lib... lib_arg) {
	const unsigned lib = route_lib_arg(lib_arg...);
	__shared__ MrfFastLds S;
	const unsigned tid = threadIdx.x;
	LibTally L;
	L.init();
	// ---- the dictionaries
	if (tid < FP_STRANDS) S.strand[tid] = __hip_atomic_load(&G.strand_tab[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	S.ckey[tid] = FD.ckey[tid]; S.cid[tid] = FD.cid[tid];
	for (unsigned q = tid; q < 2u * T.n_chrom; q += 256u) reinterpret_cast<uint4 *>(S.chrom)[q] = reinterpret_cast<const uint4 *>(T.chrom)[q];
	const mrf_lds_cptr text = (mrf_lds_cptr)(const char *)S.text + FP_PAD;      // window byte 0
	const unsigned POS = (1u << FP_KIND_SHIFT) - 1u;
	auto defer = [&](const unsigned long long i, const unsigned long long start, const unsigned long long n) {
		const unsigned at = atomicAdd(&H.counts[1], 1u);
		if (at < H.line_cap) H.lines[at] = MrfLongLine{i, start, n}; else H.counts[2] = 1u;
	};
	// a workgroup stays for many tiles (the dictionaries above are staged once: 4 KB per workgroup beside 8 KB of text per tile otherwise)
	for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
	const unsigned long long t0 = (unsigned long long)tile * TEXT_TILE;
	__syncthreads();                          // (the tile before is done with the tables below)
	// ---- the window: FP_LANE bytes a lane, in text order (window byte FP_LANE x lane); bytes ahead of the text or behind it count as none
	unsigned w[FP_LANE / 4];
	unsigned valid = 0;                       // bytes of the lane's that are text
	{
		const long long at = (long long)t0 - (long long)MRF_LB + (long long)FP_LANE * tid;
		uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
		if (at >= 0 && (unsigned long long)at < X.len) {
			v0 = *reinterpret_cast<const uint4 *>(X.text + at);
			if (FP_LANE > 16 && (unsigned long long)at + 16u < X.len) v1 = *reinterpret_cast<const uint4 *>(X.text + at + 16);
			valid = (unsigned)min((unsigned long long)FP_LANE, X.len - (unsigned long long)at);
		}
		*reinterpret_cast<uint4 *>(&S.text[FP_PAD + FP_LANE * tid]) = v0;
		w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w;
		if constexpr (FP_LANE > 16) {
			*reinterpret_cast<uint4 *>(&S.text[FP_PAD + FP_LANE * tid + 16u]) = v1;
			w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
		}
	}
	unsigned m_nl = 0, m_colon = 0, m_comma = 0;
#pragma unroll
	for (int q = 0; q < (int)(FP_LANE / 4); ++q) {
		m_nl |= fp_pack4(fp_eq_bytes(w[q], 0x0A0A0A0Au)) << (4 * q);
		m_colon |= fp_pack4(fp_eq_bytes(w[q], 0x3A3A3A3Au)) << (4 * q);
		m_comma |= fp_pack4(fp_eq_bytes(w[q], 0x2C2C2C2Cu)) << (4 * q);
	}
	const unsigned live = valid >= 32u ? 0xFFFFFFFFu : ((1u << valid) - 1u);            // (valid <= FP_LANE)
	m_nl &= live; m_colon &= live; m_comma &= live;
	const unsigned m_any = m_nl | m_colon | m_comma;
	unsigned total;
	const unsigned ex = scan_block_excl32(((unsigned)__popc(m_any) << 16) | (unsigned)__popc(m_nl), S.scan4, total);
	const unsigned n_delim = total >> 16, n_nl = total & 0xFFFFu;
	if (tid == MRF_LB / FP_LANE) S.nl_ahead = ex & 0xFFFFu;          // (the first lane of the tile proper: what lies ahead of it is the 512 bytes)
	if (n_delim > FP_DCAP || n_nl > FP_NCAP) {
		// more delimiters than the tables hold: the tile goes to the kernel that walks bytes
		if (tid == 0) { const unsigned at = atomicAdd(&H.counts[0], 1u); if (at < H.tile_cap) H.tiles[at] = tile; }
		continue;
	}
	{
		// (one loop over the lane's delimiters of all kinds: a loop per dword, without the packing, ran as long as the busiest
		// lane of every dword in turn -- measured 6.1 -> 6.9 ms)
		unsigned b = m_any, od = ex >> 16, on = ex & 0xFFFFu;
		while (b) {
			const unsigned j = (unsigned)__ffs((int)b) - 1u; b &= b - 1u;
			const unsigned kind = ((m_nl >> j) & 1u) * 2u + ((m_comma >> j) & 1u);
			S.delim[od] = (unsigned short)((FP_LANE * tid + j) | (kind << FP_KIND_SHIFT));
			if (kind == 2u) S.nl_dord[on++] = (unsigned short)od;
			++od;
		}
	}
	__syncthreads();
	const unsigned nl_ahead = S.nl_ahead;
	if (n_nl == nl_ahead) continue;               // no line ends in the tile
	const unsigned long long g0 = X.tile_base[tile];
	// Rounds of 256 lines, three passes each.  (1) A lane a LINE walks the line's entries: every block must show four colons (or
	// three and the line's end) -- otherwise the line goes to the list -- and is written to S.blk with its five field bounds.
	// (2) A lane a BLOCK: the two coordinates, the chromosome, the containment filter, the strand -- the expensive part, on every
	// lane of the wave whatever the lines' block counts are (a lane a line ran this loop twice for every wave that held one
	// two-block read: a quarter of the lanes busy in the second turn).  (3) A lane a line again: its blocks' outcomes in order
	// into the merge, then the bucket of the first merged base, key and blocks out.
	for (unsigned m0 = nl_ahead; m0 < n_nl; m0 += 256u) {
		if (tid == 0) S.n_blk = 0;
		__syncthreads();
		const unsigned m = m0 + tid;
		// ---- (1)
		bool live = m < n_nl, odd = false, dropped = false;
		unsigned long long i = 0;
		unsigned dS = 0, start = 0, eol = 0, nb = 0, first = 0;
		const unsigned long long w0 = t0 - MRF_LB;                 // (window byte 0 in the text; wraps below zero for tile 0, whose window bytes < 512 hold nothing)
		if (live) {
			const unsigned long long g = g0 + (m - nl_ahead);        // the newline's ordinal in the text = the 0-based number of the line it ends
			if (X.has_header && g == 0) live = false;
			i = g - X.has_header;
		}
		if (live) {
			const unsigned dE = S.nl_dord[m];
			eol = S.delim[dE] & POS;
			if (m == 0) {
				if (t0 != 0) { defer(i, w0 + eol, ~0ull); live = false; }  // began ahead of the window
				else { dS = 0; start = MRF_LB; }
			} else { const unsigned dp = S.nl_dord[m - 1]; dS = dp + 1u; start = (S.delim[dp] & POS) + 1u; }
		}
		if (live) {
			if (eol > start && text[start] == '#') dropped = true;       // a comment line takes a line number only (count.cpp:288)
			else {
				// the walk: the line's blocks counted, the first two kept in registers (a read has one or two; a line of more is walked once
				// more to list the rest -- a second walk for every line cost 0.5 ms of the 6.4 on C3)
				uint4 b0 = make_uint4(0, 0, 0, 0), b1 = b0;
				unsigned d = dS, cpos = start;
				for (;;) {
					unsigned long long e4;
					__builtin_memcpy(&e4, &S.delim[d], 8);
					// four colons -- or three and the line's end: a block without query fields, whose end field runs to the end of the line
					// (count.cpp:313-316 with find() == npos) and after which nothing follows
					const bool to_eol = (e4 & 0xE000600060006000ull) == 0x4000000000000000ull;
					if ((e4 & 0x6000600060006000ull) != 0ull && !to_eol) { odd = true; break; }
					const uint4 bd = make_uint4(cpos | (((unsigned)e4 & POS) << 16), ((unsigned)(e4 >> 16) & POS) | (((unsigned)(e4 >> 32) & POS) << 16), (unsigned)(e4 >> 48) & POS, 0u);
					if (nb == 0u) b0 = bd; else if (nb == 1u) b1 = bd;
					++nb;
					if (to_eol) break;
					unsigned dn = d + 4u, kind;
					while ((kind = S.delim[dn] >> FP_KIND_SHIFT) == 0u) ++dn;      // the next block, if any: behind the first comma after colon 4
					if (kind != 1u) break;
					cpos = (S.delim[dn] & POS) + 1u; d = dn + 1u;
				}
				if (!odd) {
					first = atomicAdd(&S.n_blk, nb);
					if (first + nb > FP_BCAP) {                     // no room in this round's list: the shared splitter takes the line
						odd = true;
						for (unsigned q = first; q < FP_BCAP; ++q) S.blk[q] = make_uint4(0u, 0u, 0u, 3u);      // (its places below the list's end hold nothing)
					}
				}
				if (!odd) {
					S.blk[first] = b0;
					if (nb > 1u) S.blk[first + 1u] = b1;
					if (nb > 2u) {
						unsigned q = first;
						cpos = start; d = dS;
						for (;;) {
							unsigned long long e4;
							__builtin_memcpy(&e4, &S.delim[d], 8);
							const bool to_eol = (e4 & 0xE000600060006000ull) == 0x4000000000000000ull;
							if (q >= first + 2u) S.blk[q] = make_uint4(cpos | (((unsigned)e4 & POS) << 16), ((unsigned)(e4 >> 16) & POS) | (((unsigned)(e4 >> 32) & POS) << 16), (unsigned)(e4 >> 48) & POS, 0u);
							++q;
							if (to_eol) break;
							unsigned dn = d + 4u, kind;
							while ((kind = S.delim[dn] >> FP_KIND_SHIFT) == 0u) ++dn;
							if (kind != 1u) break;
							cpos = (S.delim[dn] & POS) + 1u; d = dn + 1u;
						}
					}
				}
			}
			if (odd) { defer(i, w0 + start, eol - start); live = false; }
		}
		__syncthreads();
		// ---- (2)
		const unsigned n_blk = min(S.n_blk, FP_BCAP);          // (lines beyond the list's room listed nothing)
		for (unsigned q = tid; q < n_blk; q += 256u) {
			const uint4 bd = S.blk[q];
			if (bd.w == 3u) continue;
			const unsigned cpos = bd.x & 0xFFFFu, p1 = bd.x >> 16, p2 = bd.y & 0xFFFFu, p3 = bd.y >> 16, p4 = bd.z;
			const unsigned l_chr = p1 - cpos, l_str = p2 - p1 - 1u, l_s = p3 - p2 - 1u, l_e = p4 - p3 - 1u;
			uint4 out = make_uint4(0u, 0u, 0u, 2u);              // .w: 0 kept (.x chromosome | strand << 16, .y / .z the block), 1 passed over, 2 not the usual shape
			if (!(l_chr > 7u || l_str > 7u || l_s - 1u > 8u || l_e - 1u > 8u)) {
				// the coordinates: the eight bytes that end at the delimiter, and the byte ahead of them
				unsigned long long ws, we, wc, wt;
				__builtin_memcpy(&ws, &S.text[FP_PAD + p3 - 8u], 8);
				__builtin_memcpy(&we, &S.text[FP_PAD + p4 - 8u], 8);
				__builtin_memcpy(&wc, &S.text[FP_PAD + cpos], 8);
				__builtin_memcpy(&wt, &S.text[FP_PAD + p1 + 1u], 8);
				const unsigned s9 = (unsigned)(unsigned char)text[(int)p3 - 9] - (unsigned)'0', e9 = (unsigned)(unsigned char)text[(int)p4 - 9] - (unsigned)'0';
				unsigned vs, ve;
				const bool good_s = fp_number8(ws, min(l_s, 8u), vs), good_e = fp_number8(we, min(l_e, 8u), ve);
				bool good = good_s && good_e;
				if (l_s == 9u) { good = good && s9 <= 9u; vs += s9 * 100000000u; }
				if (l_e == 9u) { good = good && e9 <= 9u; ve += e9 * 100000000u; }
				if (good) {
					out.w = 1u;
					unsigned tb = 0u;
					if constexpr (STRANDED) {
						const unsigned char c0 = (unsigned char)wt;
						tb = l_str == 1u && (c0 == '+' || c0 == '-') ? route_transcript(lib, c0 == '-' ? 1u : 0u) : ROUTE_NO_STRAND;
						out.x = tb;
					}
					if (l_chr != 0u && tb < ROUTE_NO_STRAND) {
						const unsigned long long kb = wc & ((1ull << (8u * l_chr)) - 1ull);
						const unsigned long long key = ((unsigned long long)__builtin_bswap32((unsigned)kb) << 32) | (unsigned long long)__builtin_bswap32((unsigned)(kb >> 32)) | (unsigned long long)l_chr;
						unsigned cid = MRF_NOCHROM;
						for (unsigned sl = mrf_key_slot(key);; sl = (sl + 1u) & (FP_DICT - 1u)) {
							const unsigned long long k = S.ckey[sl];
							if (k == key) { cid = S.cid[sl]; break; }
							if (k == 0ull) break;
						}
						const int s0 = (int)vs - 1, e0 = (int)ve;
						LocProbe P;
						P.chrom = -1; P.bin = 0;
						if constexpr (STRANDED) { if (cid != MRF_NOCHROM) cid = route_table(cid, tb); }
						if (cid < T.n_chrom && route_covered(T, S.chrom[cid], (int)cid, s0, e0, P)) {
							const unsigned long long sb = wt & ((1ull << (8u * l_str)) - 1ull);
							unsigned long long tkey = ((unsigned long long)__builtin_bswap32((unsigned)sb) << 32) | (unsigned long long)__builtin_bswap32((unsigned)(sb >> 32)) | (unsigned long long)l_str;
							if constexpr (STRANDED) tkey = ((unsigned long long)(tb ? '-' : '+') << 56) | 1ull;       // (the read carries t's string)
							unsigned sid = 256u;
							for (unsigned z = 0; z < FP_STRANDS; ++z) { const unsigned long long cur = S.strand[z]; if (cur == tkey) { sid = z; break; } if (cur == STRAND_EMPTY) break; }
							if constexpr (STRANDED) { if (sid == 256u) { const char tc = tb ? '-' : '+'; sid = mrf_strand_slot(nullptr, G.strand_tab, lsq::MrfView{&tc, 1}, err); } }
							else if (sid == 256u) sid = mrf_strand_slot(nullptr, G.strand_tab, MrfLdsView{text + (p1 + 1u), l_str}, err);
							out = make_uint4(cid | (sid << 16), (unsigned)s0, (unsigned)e0, 0u);
						}
					}
				}
			}
			S.blk[q] = out;
		}
		__syncthreads();
		// ---- (3)
		if (live) {
			if (dropped) O.key[i] = ROUTE_KEY_DROPPED;
			else {
				ReadAcc A;
				ReadBig B;
				A.init();
				unsigned t = ROUTE_NO_STRAND;
				for (unsigned q = 0; q < nb; ++q) {
					const uint4 r = S.blk[first + q];
					if (r.w == 2u) { odd = true; break; }
					if constexpr (STRANDED) {
						// (a kept block's table id is odd for t = minus; a block passed over holds t itself)
						const unsigned tq = r.w == 0u ? (r.x & 1u) : r.x;
						if (q == 0u) t = tq;
						else if (tq != t) { odd = true; break; }
					}
					if (r.w == 0u) A.add(B, r.x & 0xFFFFu, r.x >> 16, (int)r.y, (int)r.z);
				}
				if (odd) defer(i, w0 + start, eol - start);
				else {
					LocProbe P;
					P.chrom = -1; P.bin = 0;
					if constexpr (STRANDED) L.note(t, A.kept());
					A.finish(B, T, S.chrom, P, O, (unsigned)i);
				}
			}
		}
	}
	}
	if constexpr (STRANDED) L.flush(O);
}

// ---- the same walk for lsq_mrf_parse_device: pass 1, blocks per data line (0 for skipped lines), first failing line
__global__ void __launch_bounds__(256) lsq_mrf_count_kernel(MrfText X, unsigned *line_nb, unsigned long long *err) {
	__shared__ MrfTileLds S;
	mrf_tile_lines<false>(S, blockIdx.x, X.text, X.len, X.tile_base, X.has_header, nullptr, nullptr, 0u, nullptr, [&](const unsigned long long i, auto line) {
		unsigned nb = 0;
		if (!lsq::mrf_line_is_skipped(line)) {
			const bool ok = lsq::mrf_split_line(line, [&](auto, auto, int64_t, int64_t) { ++nb; });
			if (!ok) { atomicMin(&err[0], X.first_line + i); nb = 0; }
		}
		line_nb[i] = nb;
	});
}

// pass 2: every read's blocks to their place (rd_idx / bk_off: exclusive prefix sums of "has blocks" / of the block counts over the data lines)
__global__ void __launch_bounds__(256) lsq_mrf_write_kernel(MrfText X, const unsigned *line_nb, const unsigned long long *rd_idx, const unsigned long long *bk_off,
                                                            MrfDict G, MrfOut O, unsigned long long *err) {
	__shared__ MrfTileLds S;
	const MrfDict D = mrf_stage_dict(S, G);
	const long long LIM = 1ll << 30;
	mrf_tile_lines<false>(S, blockIdx.x, X.text, X.len, X.tile_base, X.has_header, nullptr, nullptr, 0u, nullptr, [&](const unsigned long long i, auto line) {
		const unsigned nb = line_nb[i];
		const unsigned long long r = rd_idx[i], o = bk_off[i];
		if (i + 1 == X.n_lines) O.blk_off[r + (nb ? 1u : 0u)] = o + nb;
		if (!nb) return;
		O.blk_off[r] = o;
		O.line_no[r] = (unsigned)(X.first_line + i);
		unsigned long long w = o;
		(void)lsq::mrf_split_line(line, [&](auto chr, auto strand, int64_t start, int64_t end) {
			unsigned cid = mrf_chrom_lookup(D, chr);
			const unsigned sid = mrf_strand_slot(S.strand, D.strand_tab, strand, err);
			long long s0 = start - 1, e0 = end;
			if (s0 <= -LIM || e0 >= LIM || s0 >= LIM || e0 <= -LIM) { cid = MRF_NOCHROM; s0 = 0; e0 = 0; }
			O.blk_start[w] = (int)s0; O.blk_end[w] = (int)e0;
			O.blk_chrom[w] = (unsigned short)cid; O.blk_strand[w] = (unsigned char)sid;
			++w;
		});
	});
}

// ---- the front end (READ_FORMATS, lsq_readfile.hip): the fast kernel's dictionary, the routing launches, what they handed on
static int mrf_prepare(TextJob &J) {
	hipStream_t st = J.c->stream;
	int rc;
	// the chromosomes' names as 64-bit keys (names of at most seven bytes; a longer one has no slot and its lines go to the list)
	const lsq_events &E = *J.c->E;
	const size_t nc = E.n_table_chroms();          // (chromosome ids that have tables)
	std::vector<unsigned long long> ck(FP_DICT, 0);
	std::vector<unsigned short> ci(FP_DICT, 0);
	const bool usable = E.covered.size() <= ROUTE_CHROM_LDS && getenv("LSQ_MRF_SLOW") == nullptr;       // (the fast kernel keeps every table's record in LDS; LSQ_MRF_SLOW: the tests run the byte-walking kernel over whole files with it)
	for (size_t id = 0; usable && id < nc; ++id) {
		const std::string &nm = E.chroms.names[id];
		if (nm.empty() || nm.size() > 7) continue;
		const unsigned long long key = mrf_strand_key(nm.data(), nm.size());
		unsigned sl = mrf_key_slot(key);
		while (ck[sl] != 0) sl = (sl + 1u) & (FP_DICT - 1u);
		ck[sl] = key; ci[sl] = (unsigned short)id;
	}
	if ((rc = J.tab64.upload(ck.data(), FP_DICT, st)) || (rc = J.tab16.upload(ci.data(), FP_DICT, st))) return rc;
	HIP_TRY(hipStreamSynchronize(st));
	J.all_slow = !usable;
	return LSQ_OK;
}
static void mrf_launch(const TextJob &J, const RouteTables &RT, const RouteOut &O, hipStream_t s) {
	const unsigned n_cu = (unsigned)J.c->n_cu, side_grid = std::min(std::max(J.n_tiles, 1u), 4u * n_cu);
	// a workgroup a tile: the kernel can also run as a grid of resident workgroups that stay for many tiles (LSQ_FAST_GRID workgroups a
	// compute unit; developer aid) -- measured slower on C3: 7.4 ms at 6, 7.0 at 12, 6.7 at 24 against 6.1 with a workgroup a tile
	unsigned fast_grid = std::max(J.n_tiles, 1u);
	if (const char *e = getenv("LSQ_FAST_GRID")) { const int v = atoi(e); if (v > 0) fast_grid = (unsigned)v * n_cu; }
	const MrfFastDict FD{J.tab64.p, J.tab16.p, 1u};        // (usable, or J.all_slow is set)
	const unsigned lib = lsq::route_lib(J.c);
	const dim3 lines_grid(std::min(J.H.line_cap / 256u + 1u, 1024u));
	if (J.c->E->stranded()) {
		if (!J.all_slow) {
			hipLaunchKernelGGL((lsq_mrf_route_fast_kernel<true, unsigned>), dim3(std::min(J.n_tiles, fast_grid)), dim3(256), 0, s, J.X, J.D, FD, RT, O, J.err, J.H, J.n_tiles, lib);
			hipLaunchKernelGGL((lsq_mrf_route_kernel<true, unsigned>), dim3(std::min(side_grid, 256u)), dim3(256), 0, s, J.X, J.D, RT, O, J.err, J.H, J.n_tiles, 1u, lib);
		} else hipLaunchKernelGGL((lsq_mrf_route_kernel<true, unsigned>), dim3(J.n_tiles), dim3(256), 0, s, J.X, J.D, RT, O, J.err, J.H, J.n_tiles, 0u, lib);
		hipLaunchKernelGGL((lsq_mrf_route_lines_kernel<true, unsigned>), lines_grid, dim3(256), 0, s, J.X, J.D, RT, O, J.err, J.H, lib);
		return;
	}
	if (!J.all_slow) {
		hipLaunchKernelGGL(lsq_mrf_route_fast_kernel<false>, dim3(std::min(J.n_tiles, fast_grid)), dim3(256), 0, s, J.X, J.D, FD, RT, O, J.err, J.H, J.n_tiles);
		hipLaunchKernelGGL(lsq_mrf_route_kernel<false>, dim3(std::min(side_grid, 256u)), dim3(256), 0, s, J.X, J.D, RT, O, J.err, J.H, J.n_tiles, 1u);
	} else hipLaunchKernelGGL(lsq_mrf_route_kernel<false>, dim3(J.n_tiles), dim3(256), 0, s, J.X, J.D, RT, O, J.err, J.H, J.n_tiles, 0u);
	hipLaunchKernelGGL(lsq_mrf_route_lines_kernel<false>, lines_grid, dim3(256), 0, s, J.X, J.D, RT, O, J.err, J.H);
}
static void mrf_record(const TextJob &J) {
	J.c->parse_tiles_handed = J.all_slow ? 0u : J.counts[0]; J.c->parse_lines_listed = J.counts[1]; J.c->parse_all_slow = J.all_slow ? 1u : 0u;
}

} // namespace
