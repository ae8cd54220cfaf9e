/*
 * lookup_dev.cpp -- the device-level exports of the lookup-only commands (include/yak_amd.h): the table lookups of yak qv, triobin, trioeval,
 * chkerr and sexchr with their per-record reductions, and yak inspect's join.  Each checks what it is given, launches its kernels
 * (kern_launch.inc) on device buffers of the caller and synchronises; the commands themselves are in yak_lookup.cpp and yak_inspect.cpp.
 */
#include <limits.h>
#include "engine_int.h"

/* ---- the lookups (yak qv, triobin, trioeval, chkerr, sexchr) ---- */
/* the context a lookup export works on, or 0 after fail().  The kernel reads one whole table image: a table that is none (yk_image_state) is
 * refused first */
static yakamd_ctx *lookup_ctx(yak_ch_t *h, const char *what, int k_max, const char *k_msg)
{
	const ImageState s = yk_image_state(h);
	yakamd_ctx *c = s.c;
	if (s.sharded) fail("%s: " YK_MSG_SHARDED, what);
	else if (!c) fail("not an engine table");
	else if (c->in_pass) fail("lookup during an open pass");
	else if (c->k < 1 || c->k > k_max) fail("%s: %s", what, k_msg);
	else return c;
	return 0;
}

/* what the lookup exports share after lookup_ctx(): `launch` starts the export's kernel over the base image on c->st */
template <class Launch> static int lookup_dev(yakamd_ctx *c, const void *d_bases, Launch launch)
{
	if (((uintptr_t)d_bases & 15) != 0) return fail("device base image must be 16-byte aligned");
	HIPCK(hipSetDevice(c->dev));
	launch();
	HIPCK(hipGetLastError());
	HIPCK(hipStreamSynchronize(c->st));
	return 0;
}

/* the sizes a reduce export is given */
static int check_counts(const char *what, int64_t n_seq, int64_t n_bytes)
{
	return n_seq < 0 || n_seq > (int64_t)0xfffffffe || n_bytes < 0 ? fail("%s: bad n_seq or n_bytes", what) : 0;
}

extern "C" int yakamd_lookup_dev(yak_ch_t *h, const void *d_bases, int64_t n_bytes, void *d_out_u16)
{
	yakamd_ctx *c = lookup_ctx(h, "lookup", 31, "k must be below 32 (reference qv.c:44)");
	return c ? lookup_dev(c, d_bases, [&]() { yk_launch_lookup((const uint8_t*)d_bases, n_bytes, c->k, img_view(c), d_out_u16, 2, c->st); }) : -1;
}

extern "C" int yakamd_qv_reduce_dev(yak_ch_t *h, const void *d_t_u16, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                                    int min_len, double min_frac, uint32_t *d_tot, uint32_t *d_non0, uint64_t *d_hist1024)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c) return fail("not an engine table");
	HIPCK(hipSetDevice(c->dev));
	yk_launch_qv_reduce((const unsigned short*)d_t_u16, (const u64*)d_seq_off, d_seq_len, n_seq, min_len, min_frac, d_tot, d_non0, (u64*)d_hist1024, c->st);
	HIPCK(hipStreamSynchronize(c->st));
	return 0;
}

extern "C" int yakamd_triobin_lookup_dev(yak_ch_t *h, const void *d_bases, int64_t n_bytes, void *d_flag_u8)
{
	yakamd_ctx *c = lookup_ctx(h, "triobin lookup", 63, "k must be in [1, 63]");
	if (!c || lookup_dev(c, d_bases, [&]() { yk_launch_lookup((const uint8_t*)d_bases, n_bytes, c->k, img_view(c), d_flag_u8, 1, c->st); })) return -1;
	if (n_bytes > 0 && yk_tb_over_seen(c->st))
		return fail("triobin lookup: a count above 15 in the table -- it was not loaded with yak_ch_restore_core(..., YAK_LOAD_TRIOBIN1 / 2, ...)");
	return 0;
}

extern "C" int yakamd_triobin_reduce_dev(int k, const void *d_flag_u8, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                                         int32_t *d_cnt_i32x19, void *stream)
{
	if (k < 1 || k >= 64) return fail("triobin reduce: k must be in [1, 63]");
	yk_launch_tb_reduce((const uint8_t*)d_flag_u8, (const u64*)d_seq_off, d_seq_len, n_seq, k, (int*)d_cnt_i32x19, (hipStream_t)stream);
	HIPCK(hipGetLastError());
	HIPCK(hipStreamSynchronize((hipStream_t)stream));
	return 0;
}

/* ---- yak inspect's join (kern_inspect.inc) ---- */
/* the engines behind a table: its own, or one per rank of a table sharded over prefix ranges (also for yakamd_inspect_tables, which takes the
 * .yak body of each rank's sub-tables) */
int yk_inspect_engines(const yak_ch_t *h, std::vector<yakamd_ctx*> *out)
{
	const yak_ch_ext *e = (const yak_ch_ext*)h;
	out->clear();
	if (!h || e->magic != EXT_MAGIC) return fail("not an engine table");
	if (e->n_sub > 1) for (int r = 0; r < e->n_sub; ++r) out->push_back(ctx_of(e->sub[r]));
	else out->push_back(e->ctx);
	for (yakamd_ctx *c : *out) {
		if (!c) return fail("not an engine table");
		if (c->dev != (*out)[0]->dev) return fail("inspect: the table is spread over several devices (device %d and %d); count it on one", (*out)[0]->dev, c->dev);
		if (c->in_pass) return fail("inspect during an open pass");
	}
	return 0;
}

extern "C" int yakamd_inspect_dev(yak_ch_t *b, int k, int pre_a, int sub_lo, int sub_hi, const void *d_keys, int64_t n_keys,
                                  const uint64_t *d_sub_off, int headers, int ref_probe, uint64_t *d_joint, void *stream)
{
	if (pre_a < YAK_COUNTER_BITS || pre_a > 30) return fail("inspect: pre %d of the first table is outside [10, 30]", pre_a);
	if (sub_lo < 0 || sub_hi < sub_lo || sub_hi > 1 << pre_a) return fail("inspect: sub-tables [%d, %d) of %d", sub_lo, sub_hi, 1 << pre_a);
	if (n_keys < 0 || (n_keys > 0 && sub_hi == sub_lo)) return fail("inspect: %ld keys in no sub-table", (long)n_keys);
	if (k < 1 || k >= 64) return fail("inspect: k must be in [1, 63]");
	if (((uintptr_t)d_keys & 7) != 0) return fail("inspect: the keys must be 8-byte aligned");
	const hipStream_t st = (hipStream_t)stream;
	if (!b) {                                                  /* one table: c1 = 0 */
		if (yakamd_device_count() < 1) return fail("no gfx950 GPU visible: the join has no CPU fallback");
		ImgView none;
		memset(&none, 0, sizeof(none));
		if (yk_launch_inspect((const u64*)d_keys, (const u64*)d_sub_off, (u64)n_keys, sub_hi - sub_lo, sub_lo, headers != 0, pre_a, 0, none, 0, 0,
		                      0, (u64*)d_joint, st)) return fail("inspect: the join did not launch");
		HIPCK(hipStreamSynchronize(st));
		return 0;
	}
	std::vector<yakamd_ctx*> eng;
	if (yk_inspect_engines(b, &eng)) return -1;
	if (b->k != k) return fail("inspect: the tables have different k (%d and %d)", k, b->k);
	if (!ref_probe && k >= 32 && b->pre != pre_a)
		return fail("inspect: at k >= 32 a stored key holds hash bits [pre, pre + 54): the tables must have the same pre (%d and %d)", pre_a, b->pre);
	HIPCK(hipSetDevice(eng[0]->dev));
	for (yakamd_ctx *c : eng)                                  /* every key is probed by the one rank that owns its sub-table of B */
		if (yk_launch_inspect((const u64*)d_keys, (const u64*)d_sub_off, (u64)n_keys, sub_hi - sub_lo, sub_lo, headers != 0, pre_a, 1, img_view(c),
		                      c->plo, c->phi, ref_probe != 0, (u64*)d_joint, st)) return fail("inspect: the join did not launch");
	HIPCK(hipStreamSynchronize(st));
	return 0;
}

/* trioeval's scratch (kern_trioeval.inc): kept from one call to the next, grown when a call needs more, on the device of the last call */
namespace {
struct TeScratch {
	std::mutex mu;
	int dev = -1;
	GrowBuf tcnt, toff, st, en, kcnt, koff, list;
	u64 *host = 0;                                     /* pinned: the two totals read back */
	void on(int d) { if (d == dev) return; for (GrowBuf *b : { &tcnt, &toff, &st, &en, &kcnt, &koff, &list }) b->drop(); dev = d; }
};
TeScratch &g_te = *new TeScratch;                       /* never deleted: its buffers must not be freed once the HIP runtime has shut down at exit */
}

/* the ordered list of kept runs over bytes [0, n_bytes) of `flag` (kern_trioeval.inc): low = 0 trioeval's typed runs, with its per-record counters
 * into cnt6 when cnt6 != 0; low = 1 chkerr's runs of low k-mers.  d_streaks: as yakamd_trioeval_reduce_dev's */
static int te_streaks(const char *what, int low, int k, int min_n, const uint8_t *flag, const uint64_t *d_seq_off, int64_t n_seq, int64_t n_bytes,
                      int32_t *cnt6, void **d_streaks, int64_t *n_streaks, hipStream_t st)
{
	std::lock_guard<std::mutex> lk(g_te.mu);
	int dev = 0;
	HIPCK(hipGetDevice(&dev));
	g_te.on(dev);
	TeScratch &s = g_te;
	const int64_t nt = yk_te_tiles(n_bytes);
	if (!s.tcnt.fit((size_t)nt * 8) || !s.toff.fit((size_t)(nt + 1) * 16)) return fail("%s: out of device memory", what);
	if (!s.host) HIPCK(hipHostMalloc((void**)&s.host, 16));
	yk_launch_te_runs(flag, n_bytes, (u32*)s.tcnt.p, 0, 0, 0, 0, st, low);
	yk_launch_te_scan((const u32*)s.tcnt.p, nt, 2, (u64*)s.toff.p, st);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpyAsync(s.host, (const u64*)s.toff.p + nt, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	const u64 n_runs = s.host[0];
	void *list = 0;
	s.host[1] = 0;
	if (n_runs > 0) {                                  /* the list is sized by the runs: the number kept stays on the device until the end */
		if (!s.st.fit(n_runs * 8) || !s.en.fit(n_runs * 8)) return fail("%s: out of device memory for %llu runs", what, (unsigned long long)n_runs);
		const int64_t nb = yk_te_keep_blocks((int64_t)n_runs);
		if (!s.kcnt.fit((size_t)nb * 4) || !s.koff.fit((size_t)(nb + 1) * 8)) return fail("%s: out of device memory", what);
		if (d_streaks) { if (hipMalloc(&list, n_runs * 16) != hipSuccess) return fail("%s: out of device memory for %llu runs", what, (unsigned long long)n_runs); }
		else if (!s.list.fit(n_runs * 16)) return fail("%s: out of device memory", what);
		else list = s.list.p;
		yk_launch_te_runs(flag, n_bytes, 0, (const u64*)s.toff.p, (u64*)s.st.p, (u64*)s.en.p, 1, st, low);
		yk_launch_te_keep((const u64*)s.st.p, (const u64*)s.en.p, flag, (int64_t)n_runs, min_n, (u32*)s.kcnt.p, 0, (const u64*)d_seq_off, n_seq, 0, 0, st, low);
		yk_launch_te_scan((const u32*)s.kcnt.p, nb, 1, (u64*)s.koff.p, st);
		yk_launch_te_keep((const u64*)s.st.p, (const u64*)s.en.p, flag, (int64_t)n_runs, min_n, 0, (const u64*)s.koff.p, (const u64*)d_seq_off, n_seq, list, 1, st, low);
		if (cnt6) yk_launch_te_seq(list, (const u64*)s.koff.p + nb, (int64_t)n_runs, k, (int*)cnt6, st);
		const hipError_t e = hipGetLastError();
		if (e == hipSuccess) (void)hipMemcpyAsync(s.host + 1, (const u64*)s.koff.p + nb, 8, hipMemcpyDeviceToHost, st);
	}
	const hipError_t e = hipGetLastError(), e2 = hipStreamSynchronize(st);
	const u64 n_keep = s.host[1];
	if (e != hipSuccess || e2 != hipSuccess) {
		if (d_streaks) (void)hipFree(list);
		return fail("%s: %s", what, hipGetErrorString(e != hipSuccess ? e : e2));
	}
	if (d_streaks && n_keep == 0) { (void)hipFree(list); list = 0; }
	if (d_streaks) *d_streaks = list;
	if (n_streaks) *n_streaks = (int64_t)n_keep;
	return 0;
}

extern "C" int yakamd_trioeval_reduce_dev(int k, int min_n, const void *d_flag_u8, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                                          int64_t n_bytes, int32_t *d_cnt_i32x6, void **d_streaks, int64_t *n_streaks, void *stream)
{
	(void)d_seq_len;                                   /* the records are told apart by their separators; off[] places a streak */
	if (d_streaks) *d_streaks = 0;
	if (n_streaks) *n_streaks = 0;
	if (k < 1 || k >= 64) return fail("trioeval reduce: k must be in [1, 63]");
	if (check_counts("trioeval reduce", n_seq, n_bytes)) return -1;
	const hipStream_t st = (hipStream_t)stream;
	if (n_seq > 0) HIPCK(hipMemsetAsync(d_cnt_i32x6, 0, (size_t)n_seq * 24, st));
	if (n_seq == 0 || n_bytes == 0) { HIPCK(hipStreamSynchronize(st)); return 0; }
	return te_streaks("trioeval reduce", 0, k, min_n, (const uint8_t*)d_flag_u8, d_seq_off, n_seq, n_bytes, d_cnt_i32x6, d_streaks, n_streaks, st);
}

/* ---- yak chkerr and yak sexchr ---- */
extern "C" int yakamd_chkerr_lookup_dev(yak_ch_t *h, const void *d_bases, int64_t n_bytes, int min_cnt, void *d_low_u8)
{
	yakamd_ctx *c = lookup_ctx(h, "chkerr lookup", 63, "k must be in [1, 63]");
	return c ? lookup_dev(c, d_bases, [&]() { yk_launch_ce_lookup((const uint8_t*)d_bases, n_bytes, c->k, img_view(c), (uint8_t*)d_low_u8, min_cnt, c->st); }) : -1;
}

extern "C" int yakamd_chkerr_streaks_dev(int min_streak, const void *d_low_u8, const uint64_t *d_seq_off, int64_t n_seq, int64_t n_bytes,
                                         void **d_streaks, int64_t *n_streaks, void *stream)
{
	if (d_streaks) *d_streaks = 0;
	if (n_streaks) *n_streaks = 0;
	if (check_counts("chkerr streaks", n_seq, n_bytes)) return -1;
	const hipStream_t st = (hipStream_t)stream;
	if (n_seq == 0 || n_bytes == 0) { HIPCK(hipStreamSynchronize(st)); return 0; }
	/* chkerr.c:63-64 prints a streak when e - s > min_streak: keep e - s >= min_streak + 1, saturated; a negative min_streak keeps every run */
	const int min_n = min_streak < 0 ? 0 : min_streak >= INT_MAX - 1 ? INT_MAX : min_streak + 1;
	return te_streaks("chkerr streaks", 1, 1, min_n, (const uint8_t*)d_low_u8, d_seq_off, n_seq, n_bytes, 0, d_streaks, n_streaks, st);
}

/* ---- yak-amd cover (kern_cover.inc) ---- */
extern "C" int yakamd_cover_dev(int k, int lo, int hi, const void *d_cnt_u16, int64_t n_bytes, const uint64_t *d_seq_off, const uint32_t *d_seq_len,
                                int64_t n_seq, const void *d_bases, int mask, void *d_cov_u8, void *d_masked, yakamd_cov_t *d_tally, void *stream)
{
	if (k < 1 || k >= 32) return fail("cover: k must be below 32 (reference qv.c:44)");
	if (lo < 0 || hi < lo || hi > 1023) return fail("cover: the counts [%d, %d] are not inside [0, 1023]", lo, hi);
	if (mask < 0 || mask > 2) return fail("cover: mask %d is none of 0 (none), 1 (soft), 2 (hard)", mask);
	if (check_counts("cover", n_seq, n_bytes)) return -1;
	if (n_bytes > 0 && (!d_cnt_u16 || !d_cov_u8)) return fail("cover: no count array or no cover array");
	if (mask != 0 && (!d_bases || !d_masked)) return fail("cover: mask %d without a base image or without room for the masked one", mask);
	if (n_seq > 0 && (!d_seq_off || !d_seq_len || !d_tally)) return fail("cover: %ld sequences without their offsets, lengths or tallies", (long)n_seq);
	if ((((uintptr_t)d_cnt_u16 | (uintptr_t)d_cov_u8 | (mask ? (uintptr_t)d_bases | (uintptr_t)d_masked : 0)) & 15) != 0 || ((uintptr_t)d_seq_off & 7) != 0
	    || (((uintptr_t)d_seq_len | (uintptr_t)d_tally) & 3) != 0)
		return fail("cover: the counts, the cover and the images must be 16-byte aligned, the offsets 8-byte, the lengths and tallies 4-byte");
	if (n_bytes == 0 && n_seq == 0) return 0;
	const hipStream_t st = (hipStream_t)stream;
	if (n_seq > 0) HIPCK(hipMemsetAsync(d_tally, 0, (size_t)n_seq * sizeof(yakamd_cov_t), st));
	if (n_bytes > 0) {
		CvArgs a;
		a.t = (const unsigned short*)d_cnt_u16; a.n = n_bytes;
		a.seq_off = (const u64*)d_seq_off; a.seq_len = d_seq_len; a.n_seq = n_seq;
		a.bases = (const uint8_t*)d_bases; a.cov = (uint8_t*)d_cov_u8; a.masked = (uint8_t*)d_masked; a.tally = (u32*)d_tally;
		a.k = k; a.lo = (u32)lo; a.hi = (u32)hi;
		yk_launch_cover(a, mask, st);
		HIPCK(hipGetLastError());
	}
	HIPCK(hipStreamSynchronize(st));
	return 0;
}

/* ---- yak-amd depth (kern_depth.inc) ---- */
namespace {
struct DpScratch {                                     /* kept from one call to the next, on the device of the last call */
	std::mutex mu;
	int dev = -1;
	GrowBuf list, tbase, hist, ctr;
	u64 *host = 0;                                     /* pinned: the words read back */
	void on(int d) { if (d == dev) return; for (GrowBuf *b : { &list, &tbase, &hist, &ctr }) b->drop(); dev = d; }
};
DpScratch &g_dp = *new DpScratch;                       /* never deleted, as g_te */
const u32 DP_LONG_DEFAULT = 2048;                       /* positions from which a window goes through the histogram kernels */
const u32 DP_GROUP = 16384;                             /* long windows whose histograms are held at once: 128 MiB */
}

int64_t yk_depth_batch_max(void)
{
	const int64_t b = yk_knob("YAKAMD_DEPTH_BATCH", (int64_t)1 << 24);
	return b < 1 ? 1 : b > ((int64_t)1 << 24) ? (int64_t)1 << 24 : b;
}

/* windows [g0, g0 + n_win) of the call's numbering into d_win[0 .. n_win): one batch, n_win <= yk_depth_batch_max().  Asynchronous on `st` but for
 * the read-back of the long windows' number */
int yk_depth_batch(int k, int64_t w, const void *d_cnt_u16, const uint64_t *d_seq_off, const uint32_t *d_seq_len, const uint64_t *d_win_off,
                   int64_t n_seq, int64_t n_bytes, uint64_t g0, uint32_t n_win, void *d_win, hipStream_t st)
{
	if (n_win == 0) return 0;
	std::lock_guard<std::mutex> lk(g_dp.mu);
	int dev = 0;
	HIPCK(hipGetDevice(&dev));
	g_dp.on(dev);
	DpScratch &s = g_dp;
	const int64_t knob = yk_knob("YAKAMD_DEPTH_LONG", DP_LONG_DEFAULT);
	const u32 T = (u32)(knob < 0 ? 0 : knob > (1 << 20) ? 1 << 20 : knob);
	/* long windows are disjoint slices of more than T positions each; with w <= T there is none */
	const u64 most = w > 0 && (u64)w <= T ? 0 : std::min<u64>(n_win, (u64)n_bytes / ((u64)T + 1));
	if (!s.host) HIPCK(hipHostMalloc((void**)&s.host, 16));
	if (!s.ctr.fit(8) || !s.list.fit(most * 4 + 4) || !s.tbase.fit(most * 8 + 8)) return fail("depth reduce: out of device memory");
	DpArgs a;
	a.cnt = (const unsigned short*)d_cnt_u16; a.seq_off = (const u64*)d_seq_off; a.seq_len = d_seq_len; a.win_off = (const u64*)d_win_off;
	a.n_seq = n_seq; a.n_bytes = n_bytes; a.w = (u64)w; a.k = k;
	HIPCK(hipMemsetAsync(s.ctr.p, 0, 8, st));
	yk_launch_dp_short(a, g0, n_win, T, d_win, (u32*)s.list.p, (u64*)s.tbase.p, (u32)most, (u64*)s.ctr.p, st);
	HIPCK(hipGetLastError());
	if (most == 0) return 0;
	HIPCK(hipMemcpyAsync(s.host, s.ctr.p, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	const u64 n_long = s.host[0] >> 40, n_tiles = s.host[0] & ((1ull << 40) - 1);
	if (n_long > most) return fail("depth reduce: the sequences overlap (%llu windows of more than %u positions in %ld)", (unsigned long long)n_long, T, (long)n_bytes);
	for (u64 slot0 = 0; slot0 < n_long; slot0 += DP_GROUP) {   /* a group's tiles are [its first slot's base, the next group's) */
		const u32 ns = (u32)std::min<u64>(DP_GROUP, n_long - slot0);
		u64 t0 = 0, t1 = n_tiles;
		if (slot0 > 0) { HIPCK(hipMemcpyAsync(s.host, (const u64*)s.tbase.p + slot0, 8, hipMemcpyDeviceToHost, st)); }
		if (slot0 + ns < n_long) { HIPCK(hipMemcpyAsync(s.host + 1, (const u64*)s.tbase.p + slot0 + ns, 8, hipMemcpyDeviceToHost, st)); }
		if (slot0 > 0 || slot0 + ns < n_long) {
			HIPCK(hipStreamSynchronize(st));
			if (slot0 > 0) t0 = s.host[0];
			if (slot0 + ns < n_long) t1 = s.host[1];
		}
		if (t1 < t0 || t1 > n_tiles) return fail("depth reduce: bad tile ranges");
		if (!s.hist.fit((size_t)ns * 8192)) return fail("depth reduce: out of device memory");
		HIPCK(hipMemsetAsync(s.hist.p, 0, (size_t)ns * 8192, st));
		yk_launch_dp_long(a, g0, (const u32*)s.list.p, (const u64*)s.tbase.p, (u32)slot0, ns, t0, t1 - t0, (u64*)s.hist.p, st);
		yk_launch_dp_finish((const u64*)s.hist.p, (const u32*)s.list.p, (u32)slot0, ns, d_win, st);
		HIPCK(hipGetLastError());
	}
	return 0;
}

static int depth_args(const char *what, int k, int64_t w, const void *d_cnt_u16, const void *d_win)
{
	if (k < 1 || k >= 32) return fail("%s: k must be below 32 (reference qv.c:44)", what);
	if (w < 0) return fail("%s: a window of %ld k-mer starts", what, (long)w);
	if (((uintptr_t)d_cnt_u16 & 15) != 0 || ((uintptr_t)d_win & 7) != 0) return fail("%s: the counts must be 16-byte and the windows 8-byte aligned", what);
	return 0;
}

extern "C" int yakamd_depth_reduce_dev(int k, int64_t w, const void *d_cnt_u16, const uint64_t *d_seq_off, const uint32_t *d_seq_len,
                                       const uint64_t *d_win_off, int64_t n_seq, int64_t n_bytes, yakamd_win_t *d_win, void *stream)
{
	if (depth_args("depth reduce", k, w, d_cnt_u16, d_win) || check_counts("depth reduce", n_seq, n_bytes)) return -1;
	const hipStream_t st = (hipStream_t)stream;
	uint64_t n_win = 0;
	if (n_seq > 0) HIPCK(hipMemcpyAsync(&n_win, d_win_off + n_seq, 8, hipMemcpyDeviceToHost, st));
	HIPCK(hipStreamSynchronize(st));
	if (n_win < (uint64_t)n_seq || (w == 0 && n_win != (uint64_t)n_seq)) return fail("depth reduce: %llu windows for %ld sequences", (unsigned long long)n_win, (long)n_seq);
	const uint64_t batch = (uint64_t)yk_depth_batch_max();
	for (uint64_t g0 = 0; g0 < n_win; g0 += batch)
		if (yk_depth_batch(k, w, d_cnt_u16, d_seq_off, d_seq_len, d_win_off, n_seq, n_bytes, g0, (uint32_t)std::min<uint64_t>(batch, n_win - g0), d_win + g0, st)) return -1;
	HIPCK(hipStreamSynchronize(st));
	return 0;
}

extern "C" int yakamd_sexchr_reduce_dev(const void *d_flag_u8, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq, int64_t n_bytes,
                                        uint64_t *d_cnt_u64x4, void *stream)
{
	if (check_counts("sexchr reduce", n_seq, n_bytes)) return -1;
	const hipStream_t st = (hipStream_t)stream;
	if (n_seq > 0) HIPCK(hipMemsetAsync(d_cnt_u64x4, 0, (size_t)n_seq * 32, st));
	yk_launch_sc_reduce((const uint8_t*)d_flag_u8, n_bytes, (const u64*)d_seq_off, d_seq_len, n_seq, (u64*)d_cnt_u64x4, st);
	HIPCK(hipGetLastError());
	HIPCK(hipStreamSynchronize(st));
	return 0;
}
