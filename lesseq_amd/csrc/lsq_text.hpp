// Text staged in HBM, as the device parsers (lsq_mrf_device.hpp, lsq_sam_device.hpp, lsq_gtf.hip) see it; not a public header.
//
// lsq_text.hip puts a text into HBM as it is, with 16 bytes of slack behind it, and counts the newlines of every tile of
// TEXT_TILE bytes (16 bytes per lane, the exact zero-byte test on word ^ 0x0A0A0A0A); a prefix sum over the tile counts
// (lsq_text::d_tile_base) tells a workgroup of a parser how many newlines lie ahead of its tile.  Its place among the tile's
// own newlines then gives every newline its ordinal in the text: the number of the line it ends, or of the line it starts.
// A parser's workgroup takes a tile through TextTileNl below; which lines of the tile are its own (those that end in it, or
// those that start in it), what it stages around the tile and how it walks a line is the parser's business.
#pragma once
#include <chrono>
#include <functional>

#include "lsq_device.hpp"
#include "lsq_scan.hpp"

namespace lsq {
// lsq_text.hip: a file's bytes [byte_begin, byte_end), or bytes in host memory, staged in HBM; the newline tiles of a staged text
// (T.d_tile_base, T.n_nl), counted once; the copy pipeline through the context's pinned buffers, fed by fill(dst, offset, bytes)
constexpr size_t PIN_SLICE = 32ull << 20;
int stage_text_file(lsq_ctx *c, const char *path, unsigned long long byte_begin, unsigned long long byte_end, lsq_text &T);
int text_stage_buffer(lsq_ctx *c, const void *bytes, unsigned long long len, const char *label, lsq_text &T);
int scan_newlines(lsq_ctx *c, lsq_text &T);
typedef std::function<bool(unsigned char *, size_t, size_t)> SliceFill;
int pinned_pipeline(lsq_ctx *c, unsigned char *d_dst, size_t len, const SliceFill &fill, const char *what);

// developer aid: LSQ_CLI_TIMING=1 prints host-side seconds of the loader's steps on stderr
struct HostStopwatch {
	bool on = getenv("LSQ_CLI_TIMING") != nullptr;
	std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
	void mark(const char *what) {
		if (!on) return;
		const auto n = std::chrono::steady_clock::now();
		fprintf(stderr, "[timing]     %-32s %.3f s\n", what, std::chrono::duration<double>(n - t).count());
		t = n;
	}
};

// Device time of the loader's passes (lsq_last_ingest_stages): events around each pass's launches.  The context lists the passes
// of the latest ingest (lsq_ctx::ing_pass) in the order in which they were first named; naming one again -- a route that runs a
// second time -- overwrites its entry.  An entry keeps its pair of events: they are made once and used again by whatever pass comes
// to stand there.
inline IngestPass *stage_entry(lsq_ctx *c, const char *name) {
	for (int k = 0; k < c->ing_n; ++k) if (strcmp(c->ing_pass[k].name, name) == 0) return &c->ing_pass[k];
	if (c->ing_n == LSQ_INGEST_PASS_MAX) return nullptr;
	IngestPass &p = c->ing_pass[c->ing_n++];
	p.name = name; p.bytes = 0; p.ms = 0; p.clocked = false;
	return &p;
}
// a new ingest begins: the list is empty again -- but for the newline count, if the text at hand was counted before the ingest took it
inline void stages_reset(lsq_ctx *c, bool keep_newline_count) {
	int n = 0;
	for (int k = 0; keep_newline_count && k < c->ing_n && !n; ++k)
		if (strcmp(c->ing_pass[k].name, "newline_count") == 0) { std::swap(c->ing_pass[0], c->ing_pass[k]); n = 1; }
	c->ing_n = n; c->ing_reported = 0;
}
struct StageClock {
	IngestPass *p; hipStream_t st;
	StageClock(lsq_ctx *c, hipStream_t st_, const char *name) : p(stage_entry(c, name)), st(st_) {
		if (!p) return;
		for (hipEvent_t &e : p->ev) if (!e) (void)hipEventCreate(&e);
		if (p->ev[0]) (void)hipEventRecord(p->ev[0], st);
	}
	void end(unsigned long long bytes) {
		if (!p) return;
		if (p->ev[1]) (void)hipEventRecord(p->ev[1], st);
		p->bytes = bytes; p->clocked = true;
	}
};
} // namespace lsq

#ifndef LSQ_MRF_TILE
#define LSQ_MRF_TILE 7680
#endif
constexpr unsigned TEXT_TILE = LSQ_MRF_TILE;        // text bytes per workgroup
static_assert(TEXT_TILE == 7680 || TEXT_TILE == 3584, "with the 512 bytes MRF's fast kernel sees ahead of a tile: a window of 256 lanes x 32 or x 16 bytes");
constexpr unsigned TEXT_TILE_Q = (TEXT_TILE + 4095) / 4096;    // 16-byte words a lane of 256 takes
constexpr unsigned TEXT_NLCAP = 1024;               // newline positions held at a time (a tile of shorter lines takes several rounds)

// bit j set iff byte j of the 16 bytes is '\n'; only the first `valid` bytes count
__device__ inline unsigned text_newline_bits16(const uint4 v, unsigned valid) {
	const unsigned w[4] = {v.x, v.y, v.z, v.w};
	unsigned bits = 0;
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const unsigned x = w[q] ^ 0x0A0A0A0Au;
		const unsigned z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;   // 0x80 in every zero byte
		bits |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
	}
	return valid >= 16u ? bits : (bits & ((1u << valid) - 1u));
}
// the 16 bytes at `at` of a text of `len` bytes (the buffer holds 16 bytes of slack behind the text) and how many of them are text
__device__ inline uint4 text_load16(const unsigned char *text, unsigned long long len, unsigned long long at, unsigned &valid) {
	if (at >= len) { valid = 0; return make_uint4(0, 0, 0, 0); }
	valid = (unsigned)min(16ull, len - at);
	return *reinterpret_cast<const uint4 *>(text + at);
}

// what the newline list of a tile takes of a workgroup's LDS
struct TextNlLds {
	unsigned short nlpos[TEXT_NLCAP];       // the round's newlines: byte offsets in the tile
	unsigned scan4[4];
	unsigned carry;                         // last newline of the previous round
};

// The newlines of one tile, listed by the 256 lanes of a workgroup.  A lane keeps the newlines of its own 16-byte words as
// bit masks and, after number(), their ordinals in the tile; round() then lists TEXT_NLCAP of them at a time in L.nlpos.
struct TextTileNl {
	unsigned bits[TEXT_TILE_Q], ord[TEXT_TILE_Q];
	unsigned nt;                            // newlines of the tile (the same on every lane)
	// the tile that begins at byte t0 of the text into lds_tile (TEXT_TILE bytes, 16-byte aligned): bytes behind the text are zero
	__device__ inline void load(unsigned char *lds_tile, const unsigned char *text, const unsigned long long len, const unsigned long long t0) {
#pragma unroll
		for (unsigned q = 0; q < TEXT_TILE_Q; ++q) {
			unsigned valid = 0;
			const unsigned off = q * 4096u + threadIdx.x * 16u;
			const uint4 v = off < TEXT_TILE ? text_load16(text, len, t0 + off, valid) : make_uint4(0, 0, 0, 0);
			if (off < TEXT_TILE) *reinterpret_cast<uint4 *>(&lds_tile[off]) = v;
			bits[q] = text_newline_bits16(v, valid);
		}
	}
	// ordinals of the newlines: the lanes' first words cover bytes 0..4095 of the tile, their second words the rest.  (Two barriers
	// a word: whatever the workgroup wrote to LDS before this call is visible to all of it afterwards.)
	__device__ inline void number(TextNlLds &L) {
		nt = 0;
#pragma unroll
		for (unsigned q = 0; q < TEXT_TILE_Q; ++q) {
			unsigned total;
			ord[q] = nt + scan_block_excl32((unsigned)__popc(bits[q]), L.scan4, total);
			nt += total;
		}
	}
	// newlines rb .. rb + TEXT_NLCAP - 1 of the tile: newline j to L.nlpos[j - rb]; L.carry = newline rb - 1.  Called by the whole
	// workgroup, for rb = 0, TEXT_NLCAP, ... in turn; L.nlpos holds the round until the next call.
	__device__ inline void round(TextNlLds &L, const unsigned rb) const {
		if (rb) {
			__syncthreads();                  // (the round before has been walked)
			if (threadIdx.x == 0) L.carry = L.nlpos[TEXT_NLCAP - 1];
			__syncthreads();
		}
#pragma unroll
		for (unsigned q = 0; q < TEXT_TILE_Q; ++q) {
			unsigned b = bits[q], o = ord[q];
			while (b) {
				const unsigned j = (unsigned)__ffs((int)b) - 1u; b &= b - 1u;
				if (o >= rb && o < rb + TEXT_NLCAP) L.nlpos[o - rb] = (unsigned short)(q * 4096u + threadIdx.x * 16u + j);
				++o;
			}
		}
		__syncthreads();
	}
};
