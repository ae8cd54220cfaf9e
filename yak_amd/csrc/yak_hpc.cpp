/*
 * yak_hpc.cpp -- homopolymer compression of a base image (include/yak_amd.h): the device-level exports yakamd_hpc_dev and
 * yakamd_hpc_packed_dev, the same function on the host (yakamd_hpc_host), and yk_hpc_compact(), which the engine's feeds, the multi-GPU rounds
 * and yak_qv() run in front of their own kernels when the table lives in compressed space.
 */
#include "engine_int.h"
#include "hpc_host.h"

/* The compaction of kern_hpc.inc on `st`: count, scan, scatter, and with n_seq > 0 (ASCII input only) the sequence remap.  valid == 0: `in` is the
 * ASCII image of n bytes; valid != 0: the packed image of n bases.  Returns the length of the compressed image in `out` (room for n rounded up to
 * 16), or -1 after fail(); the stream is idle when it returns.  The tile counts and their scan live in pool memory of the current device */
int64_t yk_hpc_compact(const void *in, const u32 *valid, int64_t n, void *out, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                       uint64_t *d_seq_off_out, uint32_t *d_seq_len_out, hipStream_t st)
{
	if (n < 0 || n_seq < 0) return fail("hpc: bad n or n_seq");
	if (((uintptr_t)in & 15) != 0 || ((uintptr_t)out & 15) != 0 || ((uintptr_t)valid & 3) != 0) return fail("hpc: the images must be 16-byte aligned");
	if (n_seq > 0 && (valid || !d_seq_off || !d_seq_len || !d_seq_off_out || !d_seq_len_out)) return fail("hpc: the sequence arrays go with an ASCII image and their outputs");
	if (n == 0) {                                              /* nothing to launch for the image: every sequence is empty and starts at 0 */
		if (n_seq > 0) { HIPCK(hipMemsetAsync(d_seq_off_out, 0, (size_t)n_seq * 8, st)); HIPCK(hipMemsetAsync(d_seq_len_out, 0, (size_t)n_seq * 4, st)); HIPCK(hipStreamSynchronize(st)); }
		return 0;
	}
	const int64_t nt = yk_hpc_tiles(valid != 0, n);
	if (nt >> 31) return fail("hpc: an image of %ld positions has too many tiles for one launch", (long)n);
	DevBuf<u32> tcnt; DevBuf<u64> toff;
	if (tcnt.alloc((size_t)nt) || toff.alloc((size_t)nt + 1)) return -1;
	yk_launch_hpc_count(in, valid, n, tcnt, st);
	yk_launch_te_scan(tcnt, nt, 1, toff, st);
	yk_launch_hpc_scatter(in, valid, n, toff, (uint8_t*)out, st);
	if (n_seq > 0) yk_launch_hpc_remap((const uint8_t*)in, n, toff, (const u64*)d_seq_off, d_seq_len, n_seq, (u64*)d_seq_off_out, d_seq_len_out, st);
	HIPCK(hipGetLastError());
	u64 n_out = 0;
	HIPCK(hipMemcpyAsync(&n_out, toff.get() + nt, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	if (n_out > (u64)n) return fail("hpc: %llu positions kept of %ld", (unsigned long long)n_out, (long)n);
	return (int64_t)n_out;
}

extern "C" int64_t yakamd_hpc_dev(const void *d_bases, int64_t n_bytes, void *d_out, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                                  uint64_t *d_seq_off_out, uint32_t *d_seq_len_out, void *stream)
{
	if (n_seq > (int64_t)0xfffffffe) return fail("hpc: bad n_seq");
	if (yakamd_device_count() < 1) return fail("no gfx950 GPU visible: the compaction has no CPU fallback (yakamd_hpc_host is the host function)");
	return yk_hpc_compact(d_bases, 0, n_bytes, d_out, d_seq_off, d_seq_len, n_seq, d_seq_off_out, d_seq_len_out, (hipStream_t)stream);
}

extern "C" int64_t yakamd_hpc_packed_dev(const void *d_codes, const void *d_valid, int64_t n_bases, void *d_out, void *stream)
{
	if (!d_valid) return fail("hpc: packed image without a validity mask");
	if (yakamd_device_count() < 1) return fail("no gfx950 GPU visible: the compaction has no CPU fallback (yakamd_hpc_host is the host function)");
	return yk_hpc_compact(d_codes, (const u32*)d_valid, n_bases, d_out, 0, 0, 0, 0, 0, (hipStream_t)stream);
}

extern "C" int64_t yakamd_hpc_host(const void *ascii, int64_t n_bytes, void *out)
{
	if (n_bytes < 0 || (n_bytes > 0 && (!ascii || !out))) return fail("hpc: bad arguments");
	return yk_hpc_host(seq_nt4_table, (const uint8_t*)ascii, n_bytes, (uint8_t*)out);
}
