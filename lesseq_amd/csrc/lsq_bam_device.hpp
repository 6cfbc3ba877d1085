// BAM_SINGLE on the device; not a public header.  DESIGN.md 4.10.
// Needs: lsq_sam_device.hpp (the record filters; through it the dictionary look-ups, lsq_route.hpp, lsq_text.hpp -- StageClock -- and
// lsq_readjob.hpp), lsq_bam.hpp (block chain, header, the shared decoder and record walk).  Gives: a staged file opened -- inflated,
// verified on request, its header read and its records found (BamRecords, bam_open_verified) -- the routing kernel and its launch for
// the loader chain (bam_launch), the count / write kernels of lsq_mrf_parse_device.
//
// The file's bytes lie in HBM as lsq_text.hip staged them.  What takes the place of the text and its newline tiles:
//   block table      host: the BGZF chain (BSIZE to BSIZE) over a mapping of the file -- compressed offset, deflate length, ISIZE,
//                    output offset (prefix sum of ISIZE); the compressed bytes and the inflated stream must fit in HBM together
//   bgzf_inflate     lsq_bgzf_inflate_kernel: a lane a BGZF block runs the shared decoder (lsq_inflate.hpp) from the block's
//                    deflate bytes into its ISIZE bytes of the inflated stream; a failing block's status to an error
//                    word, the first in file order wins
//   bgzf_crc32       only with the context option "bam_verify" (and always under lsq_bam_check): lsq_bgzf_crc_kernel, a wave a BGZF
//                    block -- every lane the CRC-32 (lsq_crc32.hpp) of its slice of the block's inflated bytes, folded across the
//                    wave; the first block in file order whose sum is not the stored one to an error word; then the host looks
//                    at the file's last 28 bytes for the end-of-file marker
//   header           host: l_text, the text, n_ref and the names read back -> h and the refID -> chromosome id table
//   bam_record_starts   a record belongs to the block in which it starts.  The stream is contiguous, so only where the first
//                    record of each block begins is unknown: proposed at the block's first byte (the header's end for the block
//                    that holds it) -- what htslib writes -- every block is walked by a lane of its own (lsq_bam_starts_kernel:
//                    records, and where the record behind its last one begins); lsq_bam_verify_kernel counts the blocks whose
//                    entry is not where their predecessor's walk came out.  With block 0 exact, none is a proof that every entry
//                    is right.  Otherwise lsq_bam_repair_kernel goes through the blocks in file order, one workgroup, and walks
//                    again -- staged in LDS -- each block whose entry was wrong: correct for any file.  Then a prefix sum of the
//                    record counts and lsq_bam_offsets_kernel: the same walk, writing every record's offset.
//   bam_route        lsq_bam_route_kernel: a lane a record -- the fixed part and the CIGAR operations through bam_split_record
//                    (lsq_bam_record.hpp: the walk SAM runs), route_covered and ReadAcc::add / finish exactly as the SAM kernels
//   lsq_bam_count_kernel / lsq_bam_write_kernel   the same walk for lsq_mrf_parse_device("BAM_SINGLE")
// Record i of the file is data line i of the chain: first_line = h + 1, no header line.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "lsq_sam_device.hpp"
#include "lsq_bam.hpp"

namespace {

constexpr unsigned BAM_REF_NO_READ = 0xFFFFFFFFu;      // a reference whose name MRF cannot write: its records make no read

// The deflate bytes of a block, read as aligned 8-byte words of the staged file (its buffer is aligned and holds 16 bytes of
// slack behind the file): the word may reach beyond the block, the bytes handed out never do.
struct InflateWordSource {
	const unsigned char *base;
	unsigned long long at, end, w;
	__device__ inline InflateWordSource(const unsigned char *b, unsigned long long first, unsigned long long n) : base(b), at(first), end(first + n), w(0) {
		if (n) w = *reinterpret_cast<const unsigned long long *>(base + (at & ~7ull));
	}
	__device__ inline bool next(unsigned &b) {
		if (at >= end) return false;
		b = (unsigned)(w >> (8u * (unsigned)(at & 7ull))) & 0xFFu;
		++at;
		if ((at & 7ull) == 0 && at < end) w = *reinterpret_cast<const unsigned long long *>(base + at);
		return true;
	}
};

// ---- inflate: a lane a BGZF block; the decoder's tables in the lane's private segment (the form that was measured: DESIGN.md 4.10)
__global__ void __launch_bounds__(64) lsq_bgzf_inflate_kernel(const unsigned char *in, const lsq::BgzfBlock *tab, unsigned nb, unsigned char *out, unsigned long long *err) {
	unsigned short work[lsq::INF_WORK_SHORTS];
	const unsigned b = blockIdx.x * 64u + threadIdx.x;
	if (b >= nb) return;
	const lsq::BgzfBlock B = tab[b];
	InflateWordSource src(in, B.in_off, B.in_len);
	lsq::InflateMemSink sink{out + B.out_off, B.isize, 0};
	int st = lsq::inflate_stream(src, sink, work);
	if (!st && sink.n != B.isize) st = lsq::INF_OUTPUT_UNDER;
	if (st) atomicMin(&err[0], ((unsigned long long)b << 8) | (unsigned long long)st);
}

// ---- CRC-32: a wave a BGZF block.  Lane l owns the bytes [l S, (l + 1) S) of the block's ISIZE, S = ceil(ISIZE / 64) rounded up
// to 16 (at most 1 KiB), and runs the register over them -- from 0xFFFFFFFF in lane 0, from zero elsewhere -- four bytes a step
// through the four tables in LDS.  CRC-32 is linear over GF(2): what a lane's register would be after the bytes behind its
// slice is the register times x^(8 * those bytes) modulo the polynomial, and the block's register is the xor of the 64.  A block's
// place in the stream is a prefix sum of ISIZEs, so of any alignment: a lane takes the bytes up to the first 16-byte boundary
// one at a time, then aligned 16-byte words, then the tail; S is a multiple of 16, so the lanes of a wave share the split.
// crc[b] = the computed sum; with `compare`, the first block in file order whose stored sum (the four bytes behind its deflate
// stream in the staged file) differs goes to err[0].
constexpr unsigned BGZF_CRC_WAVES = 4;           // waves (blocks of the file at a time) per workgroup
__global__ void __launch_bounds__(64 * BGZF_CRC_WAVES) lsq_bgzf_crc_kernel(const unsigned char *in, const lsq::BgzfBlock *tab, unsigned nb, const unsigned char *stream, unsigned *crc,
                                                                            unsigned compare, unsigned long long *err) {
	__shared__ unsigned table[lsq::CRC32_TABLE_WORDS];
	for (unsigned i = threadIdx.x; i < lsq::CRC32_TABLE_WORDS; i += 64u * BGZF_CRC_WAVES) table[i] = lsq::crc32_table_entry(i & 255u, i >> 8);
	__syncthreads();
	const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (unsigned long long b = (unsigned long long)blockIdx.x * BGZF_CRC_WAVES + wave; b < nb; b += (unsigned long long)gridDim.x * BGZF_CRC_WAVES) {
		const lsq::BgzfBlock B = tab[b];
		const unsigned isize = B.isize;                                  // (<= 65 536: the block table refuses more)
		const unsigned S = (((isize + 63u) >> 6) + 15u) & ~15u;
		const unsigned lo = min(lane * S, isize), hi = min(lo + S, isize);
		const unsigned char *p = stream + B.out_off + lo, *const end = stream + B.out_off + hi;
		unsigned c = lane == 0u ? 0xFFFFFFFFu : 0u;
		for (; p < end && ((unsigned long long)p & 15ull) != 0ull; ++p) c = lsq::crc32_step_byte(c, *p, table);
		for (; end - p >= 16; p += 16) {
			const uint4 w = *reinterpret_cast<const uint4 *>(p);
			c = lsq::crc32_step_word(c, w.x, table);
			c = lsq::crc32_step_word(c, w.y, table);
			c = lsq::crc32_step_word(c, w.z, table);
			c = lsq::crc32_step_word(c, w.w, table);
		}
		for (; p < end; ++p) c = lsq::crc32_step_byte(c, *p, table);
		if (c != 0u && hi < isize) c = lsq::crc32_mulmod(c, lsq::crc32_xpow8(isize - hi));
#pragma unroll
		for (unsigned m = 1; m < 64u; m <<= 1) c ^= (unsigned)__shfl_xor((int)c, (int)m, 64);
		if (lane == 0u) {
			c ^= 0xFFFFFFFFu;
			crc[b] = c;
			const unsigned char *q = in + B.in_off + B.in_len;
			const unsigned stored = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
			if (compare && stored != c) atomicMin(&err[0], b);
		}
	}
}

// ---- record starts
struct BamStarts {
	const lsq::BgzfBlock *tab;
	unsigned nb;
	const unsigned char *s;
	unsigned long long len, hdr_end;
	unsigned long long *start, *next;        // per block: where its first record begins; where the record behind its last one does
	unsigned *cnt;                           // per block: records that start in it
};

__global__ void __launch_bounds__(256) lsq_bam_starts_kernel(BamStarts A) {
	const unsigned b = blockIdx.x * 256u + threadIdx.x;
	if (b >= A.nb) return;
	const unsigned long long o = A.tab[b].out_off, end = o + A.tab[b].isize;
	const unsigned long long p0 = o > A.hdr_end ? o : A.hdr_end;
	unsigned long long p = p0;
	unsigned n = 0;
	while (p < end) { ++n; p = lsq::bam_next_record(A.s, A.len, p); }
	A.start[b] = p0; A.next[b] = p; A.cnt[b] = n;
}

__global__ void __launch_bounds__(256) lsq_bam_verify_kernel(BamStarts A, unsigned long long *misc) {
	const unsigned b = blockIdx.x * 256u + threadIdx.x + 1u;
	if (b < A.nb && A.next[b - 1u] != A.start[b]) atomicAdd(&misc[0], 1ull);
}

// One workgroup, the blocks in file order.  What the block before came out at is carried in LDS; a block whose entry is
// another is staged in LDS from its true entry on and chased there by one lane.  misc[1]: blocks walked again.
constexpr unsigned BAM_REPAIR_LDS = lsq::BGZF_MAX_ISIZE + 32u;
__global__ void __launch_bounds__(256) lsq_bam_repair_kernel(BamStarts A, unsigned long long *misc) {
	extern __shared__ __align__(16) unsigned char bam_lds[];
	unsigned long long *s_prev = reinterpret_cast<unsigned long long *>(bam_lds);
	unsigned char *blk = bam_lds + 16;
	if (threadIdx.x == 0) *s_prev = A.next[0];
	__syncthreads();
	unsigned long long repaired = 0;
	for (unsigned b = 1; b < A.nb; ++b) {
		const unsigned long long prev = *s_prev, st = A.start[b];
		__syncthreads();
		if (st == prev) {
			if (threadIdx.x == 0) *s_prev = A.next[b];
			__syncthreads();
			continue;
		}
		// (prev >= the block's first byte: the walk before came out at or behind the end of its own block)
		const unsigned long long o = A.tab[b].out_off, end = o + A.tab[b].isize;
		unsigned long long hi = end + 4ull < A.len ? end + 4ull : A.len;
		if (hi < prev) hi = prev;
		const unsigned n_stage = (unsigned)min(hi - prev, (unsigned long long)(lsq::BGZF_MAX_ISIZE + 4u));
		for (unsigned q = threadIdx.x; q < n_stage; q += 256u) blk[q] = A.s[prev + q];
		__syncthreads();
		if (threadIdx.x == 0) {
			unsigned long long p = prev;
			unsigned n = 0;
			while (p < end) {
				++n;
				// (p < end <= prev + 65536 and p + 4 <= hi unless the stream ends inside the field: the field lies in what was staged)
				if (A.len - p < 4ull || (p - prev) + 4ull > (unsigned long long)n_stage) { p = A.len; break; }
				const unsigned long long nx = p + 4ull + (unsigned long long)lsq::bam_le32(blk + (unsigned)(p - prev));
				p = nx > A.len ? A.len : nx;
			}
			A.start[b] = prev; A.next[b] = p; A.cnt[b] = n;
			*s_prev = p;
			++repaired;
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) misc[1] = repaired;
}

__global__ void __launch_bounds__(256) lsq_bam_offsets_kernel(BamStarts A, const unsigned long long *base, unsigned long long *rec_off) {
	const unsigned b = blockIdx.x * 256u + threadIdx.x;
	if (b >= A.nb) return;
	const unsigned long long end = A.tab[b].out_off + A.tab[b].isize;
	unsigned long long w = base[b];
	const unsigned long long w_end = base[b + 1u];       // (= w + cnt[b]: the walk below is the one that counted)
	for (unsigned long long p = A.start[b]; p < end && w < w_end; p = lsq::bam_next_record(A.s, A.len, p)) rec_off[w++] = p;
}

// ---- routing: a lane a record
#ifndef LSQ_BAM_WAVES
#define LSQ_BAM_WAVES 6
#endif
// (STRANDED: as the SAM kernels, lsq_sam_device.hpp)
template <bool STRANDED, class... Lib>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LSQ_BAM_WAVES))) lsq_bam_route_kernel(BamView R, MrfText X, SamOpts Q, MrfDict G, RouteTables T, RouteOut O, unsigned long long *err, Lib... lib_arg) {
	const unsigned lib = route_lib_arg(lib_arg...);
	__shared__ RouteChrom chrom_lds[ROUTE_CHROM_LDS];
	__shared__ unsigned long long strand_lds[256];
	strand_lds[threadIdx.x & 255u] = __hip_atomic_load(&G.strand_tab[threadIdx.x & 255u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	const RouteChrom *chroms = route_stage_chroms(T, chrom_lds);
	__syncthreads();
	const long long LIM = 1ll << 30;
	const unsigned long long gsz = (unsigned long long)gridDim.x * blockDim.x;
	LibTally L;
	L.init();
	for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < X.n_lines; i += gsz) {
		const unsigned long long p = R.rec_off[i];
		ReadAcc A;
		ReadBig B;
		A.init();
		LocProbe P;
		P.chrom = -1; P.bin = 0;
		unsigned cid = MRF_NOCHROM, sid = 0, t = 0;
		bool looked = false;
		const int verdict = lsq::bam_split_record(R.s + p, R.len - p, R.n_ref, Q.skip_flags, Q.min_mapq, [&](const int64_t ref) { return R.ref_cid[ref] != BAM_REF_NO_READ; },
		                                          [&](const int64_t ref, const bool minus, const int64_t start, const int64_t end, int64_t, int64_t) {
			if (!looked) {
				// (one reference and one strand a record)
				looked = true;
				cid = R.ref_cid[ref];
				if constexpr (STRANDED) { t = route_transcript(lib, minus ? 1u : 0u); if (cid != MRF_NOCHROM) cid = route_table(cid, t); }
				const char sc = (STRANDED ? t != 0u : minus) ? '-' : '+';
				sid = mrf_strand_slot(strand_lds, G.strand_tab, lsq::MrfView{&sc, 1}, err);
			}
			const long long s0 = start - 1, e0 = end;
			if (cid >= T.n_chrom || e0 >= LIM || s0 >= LIM) return;
			if (!route_covered(T, chroms[cid], (int)cid, (int)s0, (int)e0, P)) return;
			A.add(B, cid, sid, (int)s0, (int)e0);
		}, STRANDED);
		if (verdict == lsq::SAM_MALFORMED) { atomicMin(&err[0], X.first_line + i); O.key[i] = ROUTE_KEY_DROPPED; continue; }
		if (verdict != lsq::SAM_READ) { O.key[i] = ROUTE_KEY_DROPPED; continue; }
		if constexpr (STRANDED) L.note(t, A.kept());
		A.finish(B, T, chroms, P, O, (unsigned)i);
	}
	if constexpr (STRANDED) L.flush(O);
}

// ---- lsq_mrf_parse_device("BAM_SINGLE"): pass 1, blocks per record (0 for records that make no read), first malformed record
__global__ void __launch_bounds__(256) lsq_bam_count_kernel(BamView R, MrfText X, SamOpts Q, unsigned *line_nb, unsigned long long *err) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i >= X.n_lines) return;
	const unsigned long long p = R.rec_off[i];
	unsigned nb = 0;
	const int verdict = lsq::bam_split_record(R.s + p, R.len - p, R.n_ref, Q.skip_flags, Q.min_mapq, [&](const int64_t ref) { return R.ref_cid[ref] != BAM_REF_NO_READ; },
	                                          [&](int64_t, bool, int64_t, int64_t, int64_t, int64_t) { ++nb; });
	if (verdict == lsq::SAM_MALFORMED) atomicMin(&err[0], X.first_line + i);
	line_nb[i] = verdict == lsq::SAM_READ ? nb : 0u;
}

// pass 2: every read's blocks to their place (as lsq_sam_write_kernel)
__global__ void __launch_bounds__(256) lsq_bam_write_kernel(BamView R, MrfText X, SamOpts Q, const unsigned *line_nb, const unsigned long long *rd_idx, const unsigned long long *bk_off,
                                                            MrfDict G, MrfOut O, unsigned long long *err, unsigned mate_strand) {
	const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
	if (i >= X.n_lines) return;
	const long long LIM = 1ll << 30;
	const unsigned nb = line_nb[i];
	const unsigned long long r = rd_idx[i], o = bk_off[i];
	if (i + 1 == X.n_lines) O.blk_off[r + (nb ? 1u : 0u)] = o + nb;
	if (!nb) return;
	O.blk_off[r] = o;
	O.line_no[r] = (unsigned)(X.first_line + i);
	unsigned long long w = o;
	const unsigned long long p = R.rec_off[i];
	(void)lsq::bam_split_record(R.s + p, R.len - p, R.n_ref, Q.skip_flags, Q.min_mapq, [&](const int64_t ref) { return R.ref_cid[ref] != BAM_REF_NO_READ; },
	                            [&](const int64_t ref, bool minus, int64_t bstart, int64_t bend, int64_t, int64_t) {
		unsigned cid = R.ref_cid[ref];
		const char sc = minus ? '-' : '+';
		const unsigned sid = mrf_strand_slot(nullptr, G.strand_tab, lsq::MrfView{&sc, 1}, err);
		long long s0 = bstart - 1, e0 = bend;
		if (e0 >= LIM || s0 >= LIM) { cid = MRF_NOCHROM; s0 = 0; e0 = 0; }
		O.blk_start[w] = (int)s0; O.blk_end[w] = (int)e0;
		O.blk_chrom[w] = (unsigned short)cid; O.blk_strand[w] = (unsigned char)sid;
		++w;
	}, mate_strand != 0u);
}

// ---- the host side of the chain: a staged file inflated, its header read, its records found
struct BamRecords {
	std::vector<lsq::BgzfBlock> tab;
	unsigned long long total = 0, n_rec = 0;
	lsq::BamHeader H;
	DevBuf<unsigned char> d_stream;
	DevBuf<lsq::BgzfBlock> d_tab;
	DevBuf<unsigned> d_ref_cid;
	DevBuf<unsigned long long> d_rec_off;
	DevBuf<unsigned> d_crc;                  // per block: the CRC-32 the device computed (only when the file was verified)
	BamView view() const { return BamView{d_stream.p, total, d_rec_off.p, d_ref_cid.p, (long long)H.ref_names.size()}; }
	// the first malformed record of the latest pass, as the host parser names it
	int fail_record(unsigned long long line_no, hipStream_t st) const {
		unsigned long long at = 0;
		const unsigned long long i = line_no - (H.h_lines + 1);
		if (i < n_rec) { HIP_TRY(hipMemcpyAsync(&at, d_rec_off.p + i, 8, hipMemcpyDeviceToHost, st)); HIP_TRY(hipStreamSynchronize(st)); }
		lsq::BamError e;
		lsq::bam_record_error(e, line_no, at);
		return fail(e.status, "%s", e.text.c_str());
	}
};

using lsq::bam_fail;

// the block table over the file's bytes in host memory, and every block through the inflate kernel; verify: 1 -- every block
// through the CRC-32 kernel behind it, compared with the stored sum, then the end-of-file marker; 2 -- the sums computed, nothing
// compared (lsq_debug_bgzf_crc32)
static int bam_inflate_staged(lsq_ctx *c, const lsq_text &T, const unsigned char *host_bytes, BamRecords &B, int verify) {
	hipStream_t st = c->stream;
	int rc;
	lsq::BamError e;
	uint64_t total = 0;
	if (lsq::bgzf_block_table(host_bytes, T.len, B.tab, total, e)) return bam_fail(e);
	B.total = total;
	if (B.tab.size() > 0x7FFFFFFFull) return fail(LSQ_E_RANGE, "more than 2^31 BGZF blocks");
	size_t mem_free = 0, mem_total = 0;
	HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
	const unsigned long long want = B.total + 16ull + B.tab.size() * (sizeof(lsq::BgzfBlock) + 32ull) + (64ull << 20);
	if (want > mem_free) return fail(LSQ_E_RANGE, "%s: the inflated stream (%llu bytes) beside the %llu compressed bytes does not fit the device's free memory (%llu bytes)",
	                                 T.path.c_str(), B.total, T.len, (unsigned long long)mem_free);
	DevBuf<unsigned long long> d_err;
	const unsigned long long no_err = ~0ull;
	if ((rc = B.d_stream.alloc((size_t)B.total + 16)) || (rc = B.d_tab.upload(B.tab.data(), B.tab.size(), st)) || (rc = d_err.upload(&no_err, 1, st))) return rc;
	const unsigned nb = (unsigned)B.tab.size();
	{
		StageClock k(c, st, "bgzf_inflate");
		hipLaunchKernelGGL(lsq_bgzf_inflate_kernel, dim3((nb + 63u) / 64u), dim3(64), 0, st, (const unsigned char *)T.d_text.p, (const lsq::BgzfBlock *)B.d_tab.p, nb, B.d_stream.p, d_err.p);
		HIP_TRY(hipGetLastError());
		k.end(T.len + B.total);
	}
	unsigned long long bad = 0;
	HIP_TRY(hipMemcpyAsync(&bad, d_err.p, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (bad != no_err) { lsq::bam_inflate_error(e, (int)(bad & 0xFFu), B.tab[(size_t)(bad >> 8)].file_off); return bam_fail(e); }
	if (!verify) return LSQ_OK;
	if ((rc = B.d_crc.alloc(nb))) return rc;
	{
		// (the error word still holds "none": the inflate left it alone)
		StageClock k(c, st, "bgzf_crc32");
		const unsigned grid = (unsigned)std::min<unsigned long long>(((unsigned long long)nb + BGZF_CRC_WAVES - 1) / BGZF_CRC_WAVES, (unsigned long long)c->n_cu * 16);
		hipLaunchKernelGGL(lsq_bgzf_crc_kernel, dim3(grid), dim3(64 * BGZF_CRC_WAVES), 0, st, (const unsigned char *)T.d_text.p, (const lsq::BgzfBlock *)B.d_tab.p, nb, (const unsigned char *)B.d_stream.p,
		                   B.d_crc.p, verify == 1 ? 1u : 0u, d_err.p);
		HIP_TRY(hipGetLastError());
		k.end(B.total + 8ull * nb);
	}
	HIP_TRY(hipMemcpyAsync(&bad, d_err.p, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (verify != 1) return LSQ_OK;
	if (bad != no_err) {
		unsigned computed = 0;
		HIP_TRY(hipMemcpy(&computed, B.d_crc.p + bad, 4, hipMemcpyDeviceToHost));
		lsq::bam_crc_error(e, lsq::bgzf_stored_crc(host_bytes, B.tab[(size_t)bad]), computed, B.tab[(size_t)bad].file_off);
		return bam_fail(e);
	}
	if (lsq::bam_check_eof_marker(host_bytes, T.len, e)) return bam_fail(e);
	return LSQ_OK;
}

// a mapping of the staged bytes of T's file (the block chain is walked over it)
struct BamFileMap {
	int fd = -1; void *map = MAP_FAILED; size_t len = 0;
	~BamFileMap() { if (map != MAP_FAILED) munmap(map, len); if (fd >= 0) close(fd); }
	int open_text(const lsq_text &T, const unsigned char *&bytes) {
		fd = open(T.path.c_str(), O_RDONLY);
		struct stat sb;
		if (fd < 0 || fstat(fd, &sb) != 0) return fail(LSQ_E_IO, "cannot open reads file %s", T.path.c_str());
		len = (size_t)sb.st_size;
		if ((unsigned long long)len < T.offset + T.len) return fail(LSQ_E_IO, "%s has changed since it was staged", T.path.c_str());
		bytes = nullptr;
		if (len == 0) return LSQ_OK;
		if ((map = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0)) == MAP_FAILED) return fail(LSQ_E_IO, "cannot map %s", T.path.c_str());
		bytes = (const unsigned char *)map + T.offset;
		return LSQ_OK;
	}
};

// What BAM_SINGLE's ReadFormat::open runs: the staged file to an inflated stream with its records' offsets.  (lsq_bam_check runs it on a
// context without events: no chromosome is known then, and every reference is one the events do not cover.)
static int bam_open_verified(lsq_ctx *c, lsq_text &T, BamRecords &B, bool verify) {
	hipStream_t st = c->stream;
	int rc;
	lsq_events *E = c->E;
	{
		BamFileMap M;
		const unsigned char *bytes = nullptr;
		if ((rc = M.open_text(T, bytes)) || (rc = bam_inflate_staged(c, T, bytes, B, verify ? 1 : 0))) return rc;
	}
	// the header, from a prefix of the stream that grows until it holds it
	lsq::BamError e;
	{
		std::vector<unsigned char> head;
		for (unsigned long long have = std::min<unsigned long long>(B.total, 1ull << 16);; have = std::min<unsigned long long>(B.total, have * 4ull)) {
			head.resize((size_t)have);
			if (have) HIP_TRY(hipMemcpy(head.data(), B.d_stream.p, (size_t)have, hipMemcpyDeviceToHost));
			const int hs = lsq::bam_parse_header(head.data(), have, B.total, B.H, e);
			if (hs == lsq::BAM_HEADER_NEED_MORE) continue;
			if (hs) return bam_fail(e);
			break;
		}
	}
	std::vector<unsigned> ref_cid(B.H.ref_names.size());
	for (size_t r = 0; r < ref_cid.size(); ++r) {
		const int id = E ? E->chroms.find(B.H.ref_names[r]) : -1;
		ref_cid[r] = !B.H.ref_walks[r] ? BAM_REF_NO_READ : (id < 0 || (size_t)id >= E->n_table_chroms()) ? MRF_NOCHROM : (unsigned)id;
	}
	// record starts
	const unsigned nb = (unsigned)B.tab.size();
	DevBuf<unsigned long long> d_start, d_next, d_base, d_misc;
	DevBuf<unsigned> d_cnt;
	ScanScratch SS;
	const unsigned long long zero2[2] = {0, 0};
	if ((rc = B.d_ref_cid.upload(ref_cid.data(), ref_cid.size(), st)) || (rc = d_start.alloc(nb)) || (rc = d_next.alloc(nb)) || (rc = d_cnt.alloc(nb)) || (rc = d_base.alloc((size_t)nb + 1)) ||
	    (rc = d_misc.upload(zero2, 2, st)) || (rc = SS.reserve(nb))) return rc;
	const BamStarts A{B.d_tab.p, nb, B.d_stream.p, B.total, B.H.end, d_start.p, d_next.p, d_cnt.p};
	StageClock k(c, st, "bam_record_starts");
	unsigned long long misc[2] = {0, 0};
	hipLaunchKernelGGL(lsq_bam_starts_kernel, dim3(nb / 256u + 1u), dim3(256), 0, st, A);
	hipLaunchKernelGGL(lsq_bam_verify_kernel, dim3(nb / 256u + 1u), dim3(256), 0, st, A, d_misc.p);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(misc, d_misc.p, 16, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (misc[0]) {
		HIP_TRY(hipFuncSetAttribute((const void *)lsq_bam_repair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BAM_REPAIR_LDS));
		hipLaunchKernelGGL(lsq_bam_repair_kernel, dim3(1), dim3(256), BAM_REPAIR_LDS, st, A, d_misc.p);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(misc, d_misc.p, 16, hipMemcpyDeviceToHost, st));
	}
	if ((rc = device_scan<1>(SS, d_cnt.p, nb, d_base.p, st))) return rc;
	HIP_TRY(hipMemcpyAsync(&B.n_rec, d_base.p + nb, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if ((rc = B.d_rec_off.alloc((size_t)B.n_rec))) return rc;
	hipLaunchKernelGGL(lsq_bam_offsets_kernel, dim3(nb / 256u + 1u), dim3(256), 0, st, A, (const unsigned long long *)d_base.p, B.d_rec_off.p);
	HIP_TRY(hipGetLastError());
	k.end(B.total / 8 + 8ull * B.n_rec + 28ull * nb);
	HIP_TRY(hipStreamSynchronize(st));            // (the walk's arrays go out of scope)
	c->bam_blocks = nb; c->bam_blocks_repaired = misc[1];
	return LSQ_OK;
}

static void bam_launch(const TextJob &J, const RouteTables &RT, const RouteOut &O, hipStream_t s) {
	if (!J.X.n_lines) return;
	const unsigned grid = (unsigned)std::min<unsigned long long>((J.X.n_lines + 255) / 256, (unsigned long long)J.c->n_cu * 16);
	if (J.c->E->stranded()) hipLaunchKernelGGL((lsq_bam_route_kernel<true, unsigned>), dim3(grid), dim3(256), 0, s, J.R, J.X, sam_opts(J.c), J.D, RT, O, J.err, lsq::route_lib(J.c));
	else hipLaunchKernelGGL(lsq_bam_route_kernel<false>, dim3(grid), dim3(256), 0, s, J.R, J.X, sam_opts(J.c), J.D, RT, O, J.err);
}

} // namespace
