// The staged-text layer of the device parsers: a file, a byte range of one, or bytes in host memory into HBM as they are (lsq_text,
// lsq_device.hpp), the pinned-buffer copy pipeline behind it, and the newline counts of the text's tiles (lsq_text.hpp: what a
// parser's workgroup does with a tile).  The read files (lsq_readfile.hip) and the GTF parser (lsq_gtf.hip) stage through here.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>

#include "lsq_text.hpp"

namespace {

// newlines per tile
__global__ void __launch_bounds__(256) lsq_mrf_newline_count_kernel(const unsigned char *text, unsigned long long len, unsigned *tile_cnt) {
	__shared__ unsigned lds4[4];
	const unsigned long long t0 = (unsigned long long)blockIdx.x * TEXT_TILE;
	unsigned n = 0;
#pragma unroll
	for (unsigned q = 0; q < TEXT_TILE_Q; ++q) {
		unsigned valid = 0;
		const unsigned off = q * 4096u + threadIdx.x * 16u;
		const uint4 v = off < TEXT_TILE ? text_load16(text, len, t0 + off, valid) : make_uint4(0, 0, 0, 0);
		n += (unsigned)__popc(text_newline_bits16(v, valid));
	}
	unsigned total;
	(void)scan_block_excl32(n, lds4, total);
	if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

int ensure_pinned_buffers(lsq_ctx *c) {
	if (c->pin_buf[0] && c->pin_buf[1] && c->pin_ev[0] && c->pin_ev[1]) return LSQ_OK;
	const bool ok = hipHostMalloc((void **)&c->pin_buf[0], PIN_SLICE, hipHostMallocDefault) == hipSuccess &&
	                hipHostMalloc((void **)&c->pin_buf[1], PIN_SLICE, hipHostMallocDefault) == hipSuccess &&
	                hipEventCreateWithFlags(&c->pin_ev[0], hipEventDisableTiming) == hipSuccess &&
	                hipEventCreateWithFlags(&c->pin_ev[1], hipEventDisableTiming) == hipSuccess;
	if (!ok) {
		(void)hipGetLastError();
		for (int q = 0; q < 2; ++q) { if (c->pin_buf[q]) (void)hipHostFree(c->pin_buf[q]); if (c->pin_ev[q]) (void)hipEventDestroy(c->pin_ev[q]); c->pin_buf[q] = nullptr; c->pin_ev[q] = nullptr; }
		return fail(LSQ_E_INTERNAL, "no pinned host buffers");
	}
	return LSQ_OK;
}

// The one copy path of a staged text, 16 bytes of slack behind it.  Small texts are copied as they lie in host memory; texts of a
// gigabyte and more go through pinned_pipeline and are never mapped (no page-table build-up and tear-down for gigabytes of mapping).
// A source offers its bytes both ways: fill(dst, off, n), a stretch of the text into a pinned buffer (several threads at once),
// and memory(m), the whole text as host memory the runtime copies from (made when it is asked for).
int stage_text(lsq_ctx *c, const char *label, unsigned long long offset, unsigned long long len, const SliceFill &fill, const std::function<int(const unsigned char *&)> &memory, lsq_text &T) {
	hipStream_t st = c->stream;
	T.path = label; T.len = len; T.offset = offset; T.h2d_ms = 0; T.scanned = false; T.n_nl = 0;
	if (len == 0) return LSQ_OK;
	int rc;
	if ((rc = T.d_text.alloc(len + 16))) return rc;
	unsigned long long pinned_min = 1ull << 30;           // below a gigabyte making the pinned buffers (once per context) costs more than they save
	if (const char *e = getenv("LSQ_PINNED_COPY_MIN")) { const long long v = atoll(e); if (v >= 0) pinned_min = (unsigned long long)v; }   // tests
	bool pinned = len >= pinned_min && len >= 2 * PIN_SLICE;
	HIP_TRY(hipEventRecord(c->evt0, st));
	if (pinned && ensure_pinned_buffers(c) != LSQ_OK) pinned = false;
	if (pinned) {
		if ((rc = pinned_pipeline(c, T.d_text.p, (size_t)len, fill, label))) return rc;
	} else {
		const unsigned char *m = nullptr;
		if ((rc = memory(m))) return rc;
		for (size_t off = 0; off < len && rc == LSQ_OK; off += PIN_SLICE) {
			const size_t nby = std::min<size_t>(PIN_SLICE, len - off);
			if (hipMemcpyAsync(T.d_text.p + off, m + off, nby, hipMemcpyHostToDevice, st) != hipSuccess) rc = fail(LSQ_E_DEVICE, "hipMemcpyAsync failed in the text copy");
		}
		if (hipStreamSynchronize(st) != hipSuccess && rc == LSQ_OK) rc = fail(LSQ_E_DEVICE, "text copy failed");
		if (rc) return rc;
	}
	HIP_TRY(hipEventRecord(c->evt1, st));
	HIP_TRY(hipEventSynchronize(c->evt1));
	(void)hipEventElapsedTime(&T.h2d_ms, c->evt0, c->evt1);
	return LSQ_OK;
}

} // namespace

namespace lsq {

// Host memory (or a file) to HBM through the context's two pinned 32 MiB buffers, made once per context: a few worker threads fill
// their shares of one, while the DMA engine drains the other.  38-53 GB/s, against 18-20 GB/s of the runtime's own staging of pageable
// memory on its first pass over it (it pins the pages it is given: what a first copy of fresh arrays or of a fresh mapping pays for).
int pinned_pipeline(lsq_ctx *c, unsigned char *d_dst, const size_t len, const SliceFill &fill, const char *what) {
	if (len == 0) return LSQ_OK;
	int rc = ensure_pinned_buffers(c);
	if (rc) return rc;
	hipStream_t st = c->stream;
	unsigned char *const *pin = c->pin_buf;
	int rc_copy = LSQ_OK;
	int T = std::max(1, std::min(16, host_threads(0)));
	if (const char *e = getenv("LSQ_COPY_THREADS")) { const int v = atoi(e); if (v > 0 && v <= 64) T = v; }      // developer aid
	const long n_slices = (long)((len + PIN_SLICE - 1) / PIN_SLICE);
	std::atomic<long> go{-1}, filled{0};
	std::atomic<int> io_error{0};
	std::atomic<bool> give_up{false};         // set on every way out of this function: a worker that still waits for its slice leaves
	ThreadGroup workers;                      // (joined on every way out, after give_up is set: declared first, destroyed last)
	struct GiveUp { std::atomic<bool> &f; ~GiveUp() { f.store(true, std::memory_order_release); } } give_up_on_exit{give_up};
	for (int t = 0; t < T; ++t) workers.spawn([&, t] {
		for (long sl = 0; sl < n_slices; ++sl) {
			while (go.load(std::memory_order_acquire) < sl) { if (give_up.load(std::memory_order_acquire)) return; std::this_thread::yield(); }
			const size_t off = (size_t)sl * PIN_SLICE, nby = std::min<size_t>(PIN_SLICE, len - off);
			const size_t a = nby * (size_t)t / (size_t)T, b = nby * (size_t)(t + 1) / (size_t)T;
			if (b > a && !fill(pin[sl & 1] + a, off + a, b - a)) io_error.store(1);
			filled.fetch_add(1, std::memory_order_release);
		}
	});
	for (long sl = 0; sl < n_slices; ++sl) {
		const int k = (int)(sl & 1);
		if (sl >= 2 && rc_copy == LSQ_OK && hipEventSynchronize(c->pin_ev[k]) != hipSuccess) rc_copy = fail(LSQ_E_DEVICE, "hipEventSynchronize failed in the copy of %s", what);
		go.store(sl, std::memory_order_release);
		while (filled.load(std::memory_order_acquire) < (long)T * (sl + 1)) std::this_thread::yield();
		const size_t off = (size_t)sl * PIN_SLICE, nby = std::min<size_t>(PIN_SLICE, len - off);
		if (rc_copy == LSQ_OK && (hipMemcpyAsync(d_dst + off, pin[k], nby, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(c->pin_ev[k], st) != hipSuccess))
			rc_copy = fail(LSQ_E_DEVICE, "hipMemcpyAsync failed in the copy of %s", what);
	}
	workers.join();
	if (hipStreamSynchronize(st) != hipSuccess && rc_copy == LSQ_OK) rc_copy = fail(LSQ_E_DEVICE, "the copy of %s failed", what);
	if (workers.failed() && rc_copy == LSQ_OK) rc_copy = fail(LSQ_E_INTERNAL, "a helper thread failed: %s", workers.error().c_str());
	if (io_error.load() && rc_copy == LSQ_OK) rc_copy = fail(LSQ_E_IO, "cannot read %s", what);
	return rc_copy;
}

int stage_text_file(lsq_ctx *c, const char *path, unsigned long long byte_begin, unsigned long long byte_end, lsq_text &T) {
	HostStopwatch SW;
	struct File { int fd; void *map; size_t len; ~File() { if (map != MAP_FAILED) munmap(map, len); if (fd >= 0) close(fd); } } F{open(path, O_RDONLY), MAP_FAILED, 0};
	const int fd = F.fd;
	if (fd < 0) return fail(LSQ_E_IO, "cannot open reads file %s", path);
	struct stat sb;
	if (fstat(fd, &sb) != 0) return fail(LSQ_E_IO, "cannot stat %s", path);
	const unsigned long long file_len = (unsigned long long)sb.st_size;
	byte_end = std::min(byte_end, file_len);
	byte_begin = std::min(byte_begin, byte_end);                     // the bytes [byte_begin, byte_end) of the file
	// the file as a source: pread() by the pipeline's workers, or a mapping of the file
	// (tried: the workers copying out of a mapping of the file instead -- 55 GB/s against 40-46, but the mapping's tear-down
	// costs 70 ms on one thread and more when the workers share it; and 24 / 32 workers on a box's 16 cores: slower)
	const int rc = stage_text(c, path, byte_begin, byte_end - byte_begin, [&](unsigned char *dst, size_t off, size_t n) {
		for (size_t a = 0; a < n;) {
			const ssize_t got = pread(fd, dst + a, n - a, (off_t)(byte_begin + off + a));
			if (got <= 0) return false;
			a += (size_t)got;
		}
		return true;
	}, [&](const unsigned char *&m) -> int {
		F.len = (size_t)file_len;
		if ((F.map = mmap(nullptr, F.len, PROT_READ, MAP_PRIVATE, fd, 0)) == MAP_FAILED) return fail(LSQ_E_IO, "cannot map %s", path);
		madvise(F.map, F.len, MADV_SEQUENTIAL);
		m = (const unsigned char *)F.map + byte_begin;
		return LSQ_OK;
	}, T);
	if (rc == LSQ_OK && T.len) SW.mark("text: open and copy to HBM");
	return rc;
}

int text_stage_buffer(lsq_ctx *c, const void *bytes, unsigned long long len, const char *label, lsq_text &T) {
	const unsigned char *src = (const unsigned char *)bytes;       // an array, standard input read to its end, somebody's mapping
	return stage_text(c, label, 0, len, [src](unsigned char *dst, size_t off, size_t n) { memcpy(dst, src + off, n); return true; },
	                  [src](const unsigned char *&m) { m = src; return (int)LSQ_OK; }, T);
}

int scan_newlines(lsq_ctx *c, lsq_text &T) {
	if (T.scanned) return LSQ_OK;
	hipStream_t st = c->stream;
	int rc;
	const unsigned long long len = T.len;
	T.n_nl = 0;
	if (len) {
		const unsigned long long n_tiles = (len + TEXT_TILE - 1) / TEXT_TILE;
		if (n_tiles > 0x7FFFFFFFull) return fail(LSQ_E_RANGE, "reads file larger than 16 TiB");
		DevBuf<unsigned> d_tile_cnt;
		ScanScratch SS;
		if ((rc = d_tile_cnt.alloc(n_tiles)) || (rc = T.d_tile_base.alloc(n_tiles + 1)) || (rc = SS.reserve(n_tiles))) return rc;
		StageClock k(c, st, "newline_count");
		hipLaunchKernelGGL(lsq_mrf_newline_count_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, T.d_text.p, len, d_tile_cnt.p);
		HIP_TRY(hipGetLastError());
		if ((rc = device_scan<1>(SS, d_tile_cnt.p, n_tiles, T.d_tile_base.p, st))) return rc;
		k.end(len + 12ull * n_tiles);
		HIP_TRY(hipMemcpyAsync(&T.n_nl, T.d_tile_base.p + n_tiles, 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
	}
	T.scanned = true;
	return LSQ_OK;
}

} // namespace lsq

extern "C" {

int lsq_text_stage_range(lsq_ctx *c, const char *path, uint64_t byte_begin, uint64_t byte_end, lsq_text **out) LSQ_API_TRY {
	if (!c || !path || !out) return fail(LSQ_E_ARG, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	std::unique_ptr<lsq_text> T(new lsq_text);
	int rc = stage_text_file(c, path, byte_begin, byte_end, *T);
	if (rc) return rc;
	*out = T.release();
	return LSQ_OK;
} LSQ_API_CATCH
int lsq_text_stage(lsq_ctx *c, const char *path, lsq_text **out) { return lsq_text_stage_range(c, path, 0, ~0ull, out); }

int lsq_text_lines(lsq_ctx *c, lsq_text *t, uint64_t *n_newlines) LSQ_API_TRY {
	if (!c || !t || !n_newlines) return fail(LSQ_E_ARG, "null argument");
	HIP_TRY(hipSetDevice(c->device));
	int rc = t->len ? scan_newlines(c, *t) : LSQ_OK;
	if (rc) return rc;
	*n_newlines = t->len ? t->n_nl : 0;
	return LSQ_OK;
} LSQ_API_CATCH
void lsq_text_free(lsq_text *t) { delete t; }

} // extern "C"
