/* kern_launch.inc -- part of kernels.hip (one translation unit, included in this order): launch wrappers (extern "C", declared in yk_device.h) */
#include <atomic>
#include "count_plan.h"                  /* the two LDS size formulas of the count-existing kernels */
/* The dynamic-LDS limit of kernel K (hipFuncSetAttribute) belongs to the device that was current when it was set, so a process that drives several
 * GPUs sets it once on each: lds_limit<K>(bytes), before a launch of K that asks for more than 64 KiB, sets it once per kernel and device.  false: the
 * runtime refused (the error stays for the caller to clear or to find; the next call asks again) -- what that means is the caller's to say */
template <auto K> static bool lds_limit(int bytes)
{
	static std::atomic<unsigned> done{0};                             /* bit d: set on device d */
	int d = 0; (void)hipGetDevice(&d);
	if (done.load(std::memory_order_acquire) >> (d & 31) & 1) return true;
	if (hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
	done.fetch_or(1u << (d & 31), std::memory_order_release);
	return true;
}
extern "C" {

/* k-mers ENDING at positions [pos0, n) of `bases` (bytes before pos0 are read as left context);
 * emitted position = index in `bases` - t_sub */
void yk_launch_extract(const uint8_t *bases, int64_t pos0, int64_t n, int64_t t_sub, int k, int pre, int plo, int phi,
                       u64 *out_hash, u32 *out_t, u64 *cursor, hipStream_t st)
{
	if (n <= pos0) return;
	const u64 tiles = ((u64)(n - pos0) + XT_TILE - 1) / XT_TILE;
	YK_LAUNCH(k_extract, dim3((unsigned)tiles), dim3(XT_THREADS), 0, st, bases, pos0, n, t_sub, k, pre, plo, phi, out_hash, out_t, cursor);
}

/* ASCII image -> the packed image of yakamd_feed_packed_dev: 32 bases per lane, two code words and one validity word */
__global__ __launch_bounds__(256)
void k_pack(const uint8_t *__restrict__ a, int64_t n, u32 *__restrict__ codes, u32 *__restrict__ valid)
{
	const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x, p0 = w * 32;
	if (p0 >= n) return;
	u32 c0 = 0, c1 = 0, v = 0;
	for (int j = 0; j < 32; ++j) {
		const int64_t p = p0 + j;
		const u32 c = p < n ? d_nt4[a[p]] : 4u;
		if (c < 4) { v |= 1u << j; if (j < 16) c0 |= c << (2 * j); else c1 |= c << (2 * (j - 16)); }
	}
	codes[2 * w] = c0; codes[2 * w + 1] = c1; valid[w] = v;
}
void yk_launch_pack(const uint8_t *a, int64_t n, u32 *codes, u32 *valid, hipStream_t st)
{
	if (n > 0) YK_LAUNCH(k_pack, dim3((unsigned)((n + 32 * 256 - 1) / (32 * 256))), dim3(256), 0, st, a, n, codes, valid);
}

/* partitioning extraction: a histogram sweep, the scan of its rows, the scatter of the records of format `fmt`; bstart[1 << nb_bits] (device) = the record count */
void yk_launch_xpart(const uint8_t *bases, int64_t pos0, int64_t n, int64_t t_sub, int k, int pre, int plo, int phi,
                     int nb_bits, u32 *rows, u64 *partial, u64 *bstart, void *out, RecFmt fmt, hipStream_t st, const u32 *valid)
{
	if (n <= pos0) return;
	const int n_blk = yk_xpart_blocks(n - pos0);
	const size_t lds = sizeof(u32) << nb_bits;
	const int lds_max = 160 * 1024 - 4096;
	auto histogram = [&]() {                                          /* (the tagged records' own sweep also counts the rounds that reach a bucket) */
		YK_LAUNCH(k_xpart<0>, dim3(n_blk), dim3(XT_THREADS), lds, st, bases, pos0, n, t_sub, k, pre, plo, phi, nb_bits, rows, (Rec*)out, valid);
		launch_part_scan(rows, n_blk, nb_bits, partial, bstart, st);
	};
	switch (fmt) {
	case YK_FMT_TAGGED: {                                             /* needs nb_bits <= 10, k < 32 (the caller checks) */
		const size_t wlds = wc_lds_bytes<8, XW_CAP_S, false>(1 << nb_bits, 1024);
		lds_limit<k_xpart_wcs<true>>(lds_max);
		static bool said = false;
		if (!said && getenv("YAKAMD_VERBOSE") && atoi(getenv("YAKAMD_VERBOSE")) > 1) {
			int nb = 0; said = true;
			hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)k_xpart_wcs<true>, 1024, wlds);
			fprintf(stderr, "[yak_amd] k_xpart_wcs: %zu B of dynamic LDS, %d workgroups per CU\n", wlds, nb);
		}
		const bool k31 = k == 31;                                     /* yak's default k: the variants with the constant folded in */
		if (k31) YK_LAUNCH((k_xpart<3, 31>), dim3(n_blk), dim3(XT_THREADS), 3 * lds, st, bases, pos0, n, t_sub, k, pre, plo, phi, nb_bits, rows, (Rec*)out, valid);
		else YK_LAUNCH(k_xpart<3>, dim3(n_blk), dim3(XT_THREADS), 3 * lds, st, bases, pos0, n, t_sub, k, pre, plo, phi, nb_bits, rows, (Rec*)out, valid);
		launch_part_scan(rows, n_blk, nb_bits, partial, bstart, st, true);
		if (k31) {
			lds_limit<k_xpart_wcs<true, 31>>(lds_max);
			YK_LAUNCH((k_xpart_wcs<true, 31>), dim3(n_blk), dim3(1024), wlds, st, bases, pos0, n, k, pre, plo, phi, nb_bits, (const u32*)rows, (u64*)out, 0, valid);
		}
		else YK_LAUNCH(k_xpart_wcs<true>, dim3(n_blk), dim3(1024), wlds, st, bases, pos0, n, k, pre, plo, phi, nb_bits, (const u32*)rows, (u64*)out, 0, valid);
		return;
	}
	case YK_FMT_POS:                                                  /* the write-combining scatter; the plain one serves prefixes beyond 10 bits */
		histogram();
		if (nb_bits <= 10) {
			lds_limit<k_xpart_wc<1>>(lds_max);
			YK_LAUNCH(k_xpart_wc<1>, dim3(n_blk), dim3(XW_NT), (wc_lds_bytes<4, XW_CAP_T, true>(1 << nb_bits, XW_NT)), st,
			          bases, pos0, n, t_sub, k, pre, plo, phi, nb_bits, (const u32*)rows, (const u64*)bstart, out, valid);
		}
		else YK_LAUNCH(k_xpart<1>, dim3(n_blk), dim3(XT_THREADS), lds, st, bases, pos0, n, t_sub, k, pre, plo, phi, nb_bits, rows, (Rec*)out, valid);
		return;
	case YK_FMT_HASH:
	case YK_FMT_HASH_RNG:                                             /* the range tag is the round-stable scatter's alone (the caller checked k and nb_bits) */
		histogram();
		if (nb_bits <= 10 && k < 32) {                                /* round-stable: 7 slots per stack, two workgroups per CU */
			lds_limit<k_xpart_wcs<false>>(lds_max);
			YK_LAUNCH(k_xpart_wcs<false>, dim3(n_blk), dim3(1024), (wc_lds_bytes<8, XW_CAP_S, false>(1 << nb_bits, 1024)), st,
			          bases, pos0, n, k, pre, plo, phi, nb_bits, (const u32*)rows, (u64*)out, fmt == YK_FMT_HASH_RNG, valid);
		} else if (nb_bits <= 10) {
			lds_limit<k_xpart_wc<2>>(lds_max);
			YK_LAUNCH(k_xpart_wc<2>, dim3(n_blk), dim3(XW_NT), (wc_lds_bytes<8, XW_CAP_H, false>(1 << nb_bits, XW_NT)), st,
			          bases, pos0, n, t_sub, k, pre, plo, phi, nb_bits, (const u32*)rows, (const u64*)bstart, out, valid);
		}
		else YK_LAUNCH(k_xpart<2>, dim3(n_blk), dim3(XT_THREADS), lds, st, bases, pos0, n, t_sub, k, pre, plo, phi, nb_bits, rows, (Rec*)out, valid);
		return;
	}
}

int yk_part_groups(void) { return PS_G; }
int yk_xpart_blocks(int64_t n_pos) { return (int)(((u64)n_pos + (u64)XP_T * XT_TILE - 1) / ((u64)XP_T * XT_TILE)); }
int yk_rpart_blocks(int64_t n_rec) { return (int)(((u64)n_rec + RP_CHUNK - 1) / RP_CHUNK); }

void yk_launch_rpart(const u64 *in_hash, const u32 *in_t, int64_t n, int pre, int plo, int phi,
                     int nb_bits, u32 *rows, u64 *partial, u64 *bstart, Rec *out, hipStream_t st)
{
	if (n <= 0) return;
	const int n_blk = yk_rpart_blocks(n);
	const size_t lds = sizeof(u32) << nb_bits;
	YK_LAUNCH(k_rpart<0>, dim3(n_blk), dim3(256), lds, st, in_hash, in_t, n, pre, plo, phi, nb_bits, rows, out);
	launch_part_scan(rows, n_blk, nb_bits, partial, bstart, st);
	YK_LAUNCH(k_rpart<1>, dim3(n_blk), dim3(256), lds, st, in_hash, in_t, n, pre, plo, phi, nb_bits, rows, out);
}

void yk_replay_prof(u64 *out8) { (void)hipMemcpyFromSymbol(out8, HIP_SYMBOL(d_rp_prof), 64); u64 z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(d_rp_prof), z, 64); }
void yk_par_counters(u32 *ok, u32 *fail)
{
	(void)hipDeviceSynchronize();
	(void)hipMemcpyFromSymbol(ok, HIP_SYMBOL(d_par_ok), 4);
	(void)hipMemcpyFromSymbol(fail, HIP_SYMBOL(d_par_fail), 4);
}

int yk_bad_hash_seen(hipStream_t st)
{
	u32 v = 0;
	(void)hipStreamSynchronize(st);
	(void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(d_bad_hash), 4);
	return (int)v;
}

void yk_launch_acc_init(AccSlot *s, u64 n, hipStream_t st)
{
	YK_LAUNCH(k_acc_init, dim3(grid_for(n)), dim3(256), 0, st, s, n);
}

void yk_launch_acc_insert(const Rec *rec, int64_t n, u64 t0, AccTab tab, ImgView img,
                          int img_nonempty, int bloom_mode, u64 *newlist, u64 *counters, hipStream_t st)
{
	if (n <= 0) return;
	YK_LAUNCH(k_acc_insert, dim3(grid_for((u64)n)), dim3(256), 0, st, rec, n, t0, tab, img, img_nonempty, bloom_mode, newlist, counters);
}

void yk_launch_acc_rehash(AccTab oldt, AccTab newt, hipStream_t st)
{
	YK_LAUNCH(k_acc_rehash, dim3(grid_for(oldt.mask + 1)), dim3(256), 0, st, oldt, newt);
}

void yk_launch_img_count(const Rec *rec, int64_t n, ImgView img, hipStream_t st)
{
	if (n <= 0) return;
	YK_LAUNCH(k_img_count, dim3(grid_for((u64)n)), dim3(256), 0, st, rec, n, img);
}

/* LDS needed by k_img_count_lds for a sub-table of `cap` slots holding `count` keys */
size_t yk_img_count_lds_bytes(u32 cap, u32 count) { return yk_plan_img_count_lds_bytes(cap, count); }

/* YK_FMT_POS or YK_FMT_HASH records, grouped by sub-table (bstart) */
int yk_launch_img_count_lds(const void *rec, RecFmt fmt, const u64 *bstart, ImgView img, int plo, int phi, size_t lds, u64 *compact, u32 stride, hipStream_t st)
{
	if (!lds_limit<k_img_count_lds<1>>(160 * 1024 - 256) || !lds_limit<k_img_count_lds<2>>(160 * 1024 - 256)) { (void)hipGetLastError(); return -1; }
	if (fmt != YK_FMT_POS) YK_LAUNCH(k_img_count_lds<1>, dim3(phi - plo), dim3(1024), lds, st, (const u64*)rec, bstart, img, plo, compact, stride);
	else YK_LAUNCH(k_img_count_lds<2>, dim3(phi - plo), dim3(1024), lds, st, (const u64*)rec, bstart, img, plo, compact, stride);
	return 0;
}

void yk_launch_img_count_h(const u64 *hash, int64_t n, ImgView img, hipStream_t st)
{
	if (n <= 0) return;
	YK_LAUNCH(k_img_count_h, dim3(grid_for((u64)n)), dim3(256), 0, st, hash, n, img);
}

void yk_launch_img_inc(ImgView img, u64 hash, u64 *out2, hipStream_t st) { YK_LAUNCH(k_img_inc, dim3(1), dim3(1), 0, st, img, hash, out2); }

void yk_launch_img_fold(ImgView img, u64 n_slots, hipStream_t st)
{
	if (n_slots) YK_LAUNCH(k_img_fold, dim3(grid_for(n_slots)), dim3(256), 0, st, img, n_slots);
}

void yk_launch_img_clear(ImgView img, u64 n_slots, hipStream_t st, int bump)
{
	if (n_slots) YK_LAUNCH(k_img_clear, dim3(grid_for(n_slots)), dim3(256), 0, st, img, n_slots, bump);
}

void yk_launch_img_hist(ImgView img, u64 n_slots, u64 *hist, hipStream_t st)
{
	if (n_slots) YK_LAUNCH(k_img_hist, dim3(grid_for(n_slots)), dim3(256), 0, st, img, n_slots, (unsigned long long*)hist);
}

void yk_launch_img_setcnt(ImgView img, u64 n_slots, u32 cnt, hipStream_t st)
{
	if (n_slots) YK_LAUNCH(k_img_setcnt, dim3(grid_for(n_slots)), dim3(256), 0, st, img, n_slots, cnt);
}

void yk_launch_lastput(const Rec *rec, int64_t n, u64 t0, u64 t_from, AccTab tab, ImgView img,
                       int img_nonempty, int bloom_mode, const u32 *only_missing, u64 *lp_batch, hipStream_t st)
{
	if (n <= 0) return;
	YK_LAUNCH(k_lastput, dim3(grid_for((u64)n)), dim3(256), 0, st, rec, n, t0, t_from, tab, img, img_nonempty, bloom_mode, only_missing, lp_batch);
}

void yk_launch_lastput_merge(u64 *lastput, const u64 *lp_batch, u32 *missing, u32 *n_missing, int P, int plo, int phi, hipStream_t st)
{
	YK_LAUNCH(k_lastput_merge, dim3((P + 255) / 256), dim3(256), 0, st, lastput, lp_batch, missing, n_missing, P, plo, phi);
}

void yk_launch_bf_test(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, u64 *miss, hipStream_t st)
{
	if (n_new) YK_LAUNCH(k_bf_test, dim3(grid_for(n_new)), dim3(256), 0, st, tab, newlist, n_new, bf, miss);
}

void yk_launch_bf_set(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, const u64 *miss,
                      u32 *multi, int multi_bits, u64 *counters, hipStream_t st)
{
	if (n_new) YK_LAUNCH(k_bf_set, dim3(grid_for(n_new)), dim3(256), 0, st, tab, newlist, n_new, bf, miss, multi, multi_bits, counters);
}

void yk_launch_bf_check(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, const u64 *miss,
                        const u32 *multi, int multi_bits, u64 *cand, u64 *counters, hipStream_t st)
{
	if (n_new) YK_LAUNCH(k_bf_check, dim3(grid_for(n_new)), dim3(256), 0, st, tab, newlist, n_new, bf, miss, multi, multi_bits, cand, counters);
}

void yk_launch_bf_mapfill(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, const u64 *miss,
                          const u32 *multi, int multi_bits, u64 *map, int map_bits, hipStream_t st)
{
	if (n_new) YK_LAUNCH(k_bf_mapfill, dim3(grid_for(n_new)), dim3(256), 0, st, tab, newlist, n_new, bf, miss, multi, multi_bits, map, map_bits);
}

void yk_launch_bf_resolve(AccTab tab, const u64 *newlist, const u64 *cand, u64 n_cand, BloomView bf,
                          const u64 *miss, const u64 *map, int map_bits, hipStream_t st)
{
	if (n_cand) YK_LAUNCH(k_bf_resolve, dim3(grid_for(n_cand)), dim3(256), 0, st, tab, newlist, cand, n_cand, bf, miss, map, map_bits);
}

void yk_launch_select_count(AccTab tab, int bloom_mode, int P, u32 *seg_cnt, hipStream_t st)
{
	(void)P;
	YK_LAUNCH(k_select_count, dim3((unsigned)((tab.mask + SEL_CHUNK) / SEL_CHUNK)), dim3(256), 0, st, tab, bloom_mode, seg_cnt);
}

void yk_launch_select_scatter(AccTab tab, int bloom_mode, int P, const u64 *seg_off, u32 *seg_cur,
                              u64 *rec_kc, u64 *rec_t, hipStream_t st)
{
	(void)P;
	YK_LAUNCH(k_select_scatter, dim3((unsigned)((tab.mask + SEL_CHUNK) / SEL_CHUNK)), dim3(256), 0, st, tab, bloom_mode, seg_off, seg_cur, rec_kc, rec_t);
}

void yk_launch_seg_sort_pass(const u64 *seg_off, int P, const u64 *src_kc, const u64 *src_t,
                             u64 *dst_kc, u64 *dst_t, int shift, u32 *dig_hist, int n_dig, hipStream_t st)
{
	YK_LAUNCH((k_seg_sort_pass<8, 256>), dim3(P), dim3(256), 0, st, seg_off, (const u32*)0, src_kc, src_t, dst_kc, dst_t, shift, dig_hist, n_dig);
}

void yk_launch_replay(const ReplayTask *tasks, int n_tasks, int n_threads, const u64 *old_keys, const u32 *old_used,
                      u64 *new_keys, u32 *new_used, u32 *scr_used, u32 *scr_owner, u64 *scr_par,
                      const u64 *rec_kc, const u64 *rec_t, const u64 *lastput,
                      u32 *out_bits, u32 *out_count, u32 lds_words, hipStream_t st)
{
	lds_limit<k_replay>(160 * 1024 - 1024);
	if (lds_words < 2 * RP_LDS_WORDS) lds_words = 2 * RP_LDS_WORDS;
	YK_LAUNCH(k_replay, dim3(n_tasks), dim3(n_threads), (size_t)lds_words * 4, st, tasks, old_keys, old_used, new_keys, new_used,
	                   scr_used, scr_owner, scr_par, rec_kc, rec_t, lastput, out_bits, out_count, lds_words);
}

/* rng != 0: SHR_RG workgroups per sub-table; seg_cnt then holds P x SHR_RG counts (yk_shrink_shares) and the scatter takes them as rng_cnt */
int yk_shrink_shares(void) { return SHR_RG; }
void yk_launch_shrink_count(ImgView img, int P, int cmin, int cmax, int which, ImgView other, u32 *seg_cnt, hipStream_t st, int rng)
{
	YK_LAUNCH(k_shrink_count, dim3(P, rng ? SHR_RG : 1), dim3(256), 0, st, img, cmin, cmax, which, other, seg_cnt);
}

void yk_launch_shrink_scatter(ImgView img, int P, int cmin, int cmax, int which, ImgView other, const u64 *seg_off, u64 *rec_kc, hipStream_t st, const u32 *rng_cnt)
{
	YK_LAUNCH(k_shrink_scatter, dim3(P, rng_cnt ? SHR_RG : 1), dim3(256), 0, st, img, cmin, cmax, which, other, seg_off, rec_kc, rng_cnt);
}

void yk_launch_put_u64(const u64 *pos, const u64 *val, u32 n, u64 *out, hipStream_t st)
{
	if (n) YK_LAUNCH(k_put_u64, dim3((n + 255) / 256), dim3(256), 0, st, pos, val, n, out);
}

void yk_launch_resize(const ResizeTask *tasks, int P, const u64 *old_keys, const u32 *old_used, u64 *new_keys, u32 *new_used, u32 *scr_used, hipStream_t st)
{
	YK_LAUNCH(k_resize, dim3(P), dim3(256), 0, st, tasks, old_keys, old_used, new_keys, new_used, scr_used);
}

void yk_launch_keys_to_hashes(const u64 *kc, const u64 *seg_off, int P, int pre, u64 *hash, u32 *t, hipStream_t st, unsigned short *cnt)
{
	YK_LAUNCH(k_keys_to_hashes, dim3(P), dim3(256), 0, st, kc, seg_off, pre, hash, t, cnt);
}

/* yakamd_ch_sum's count step over a listing of n {hash, count} entries; *missing is raised when a listed key of [plo, phi) is not in the image */
void yk_launch_img_add_counts(const u64 *hash, const unsigned short *cnt, u64 n, ImgView img, int plo, int phi, u32 *missing, hipStream_t st)
{
	if (n == 0) return;
	const int tab = img.pre <= 12;
	const size_t lds = tab ? (size_t)8 << img.pre : 0;
	const dim3 grid(grid_for(n, AC_THREADS * AC_U)), block(AC_THREADS);
	if (img.k < 32) YK_LAUNCH(k_img_add_counts<false>, grid, block, lds, st, hash, cnt, n, img, plo, phi, tab, missing);
	else YK_LAUNCH(k_img_add_counts<true>, grid, block, lds, st, hash, cnt, n, img, plo, phi, tab, missing);
}

/* one sweep of the sort by insertion time (k_part2<.., TS>): {key, time} pairs in and out, bin = (time >> fp.ssh) mod 2^fp.s2_bits */
void yk_launch_part2_ts(const Chunk2 *chunks, int n_chunks, const u32 *chunk_first, const u64 *bbase, FastParams fp, int P,
                        u32 *rows2, u64 *sbstart, Rec *out, hipStream_t st)
{
	const size_t lds = sizeof(u32) << fp.s2_bits;
	lds_limit<k_part2<1, true>>(160 * 1024 - 256);
	lds_limit<k_part2_wc<true>>(160 * 1024 - 256);
	if (n_chunks) YK_LAUNCH((k_part2<0, true>), dim3(n_chunks), dim3(256), lds, st, chunks, fp, rows2, bbase, out);
	YK_LAUNCH(k_part2_scan, dim3(P), dim3(256), 0, st, chunk_first, bbase, fp.s2_bits, rows2, sbstart, P, 1);
	if (n_chunks && fp.s2_bits <= 13 && fp.s2_bits >= 4) {
		const size_t l2 = wc_lds_bytes<4, WC_CAP, true>(fp.s2_bits < 11 ? 1 << fp.s2_bits : WC_SEG, WC_NT);
		YK_LAUNCH((k_part2_wc<true>), dim3(n_chunks), dim3(WC_NT), l2, st, chunks, fp, (const u32*)rows2, (const u64*)sbstart, bbase, out);
	} else if (n_chunks) YK_LAUNCH((k_part2<1, true>), dim3(n_chunks), dim3(1024), lds, st, chunks, fp, rows2, bbase, out);
}
size_t yk_ts_rank_lds(int ws, u32 *cap_out)
{
	const size_t nW = ws > 6 ? (size_t)1 << (ws - 5) : 2;
	*cap_out = 256 * TSR_R;                                       /* what the lanes' registers hold: 32 KB of stage; with the bitmap of up to 2^15 times, four workgroups per CU */
	if (const long e = yk_knob("YAKAMD_TS_CAP", 0)) *cap_out = (u32)std::min<long>(256 * TSR_R, std::max<long>(16, e));   /* tests: a small stage sends bins through the window loop */
	return 8 * nW + 16 * (size_t)*cap_out;
}
/* bins of 2^w times, 2^j of them per workgroup step (n_bins is a multiple of 2^j) */
int yk_launch_ts_rank(const u64 *binstart, const Rec *in, int w, int j, u32 bin_lo, u32 n_bins, u64 *out_kc, u64 *out_t, u32 *fail, hipStream_t st)
{
	u32 cap = 0;
	const size_t lds = yk_ts_rank_lds(w + j, &cap);
	if (!lds_limit<k_ts_rank>(100 * 1024)) { (void)hipGetLastError(); return -1; }
	if (lds > 100 * 1024 || (n_bins & ((1u << j) - 1))) return -1;
	const u32 n_super = n_bins >> j;
	const u32 grid = std::min<u32>(n_super, 256 * 4 * 16);        /* a few steps per workgroup, handed out as slots free up */
	if (grid) YK_LAUNCH(k_ts_rank, dim3(grid), dim3(256), lds, st, binstart, in, w, j, bin_lo, n_super, out_kc, out_t, fail, cap);
	return 0;
}
void yk_launch_kt_split(const Rec *in, u64 n, u64 *out_kc, u64 *out_t, hipStream_t st)
{
	const u32 grid = (u32)std::min<u64>((n + 255) / 256, 256 * 8 * 8);
	if (grid) YK_LAUNCH(k_kt_split, dim3(grid), dim3(256), 0, st, in, n, out_kc, out_t);
}

void yk_launch_part2(const Chunk2 *chunks, int n_chunks, const u32 *chunk_first, const u64 *bbase, FastParams fp, int P,
                     u32 *rows2, u64 *sbstart, Rec *out, hipStream_t st)
{
	const size_t lds = sizeof(u32) << fp.s2_bits;
	const int nt = 1024;
	lds_limit<k_part2<1, false>>(160 * 1024 - 256);
	if (n_chunks) YK_LAUNCH((k_part2<0>), dim3(n_chunks), dim3(256), lds, st, chunks, fp, rows2, bbase, out);
	YK_LAUNCH(k_part2_scan, dim3(P), dim3(256), 0, st, chunk_first, bbase, fp.s2_bits, rows2, sbstart, P, 1);
	const int wc = (int)yk_knob("YAKAMD_P2_WC", 1);
	if (n_chunks && wc && fp.rec8_out && fp.s2_bits <= 13 && fp.s2_bits >= 4) {
		if (!lds_limit<k_part2_wc8<false>>(WC_SEG * WC8_CAP * 8 + WC_SEG * 8 + WC_NT * 4 + 16)) (void)hipGetLastError();   /* the kernel has 6.5 KB of static LDS besides */
		const size_t seg = fp.s2_bits < 11 ? (size_t)1 << fp.s2_bits : WC_SEG;
		if (fp.rec8_in && seg <= 1024 && yk_knob("YAKAMD_P2_CAP7", 1) != 0) {   /* <= 76 KB with the ring: two workgroups per CU */
			if (!lds_limit<k_part2_wc8<false, 7>>(1024 * 7 * 8 + 1024 * 8 + WC_NT * 4 + 16)) (void)hipGetLastError();
			YK_LAUNCH((k_part2_wc8<false, 7>), dim3(n_chunks), dim3(WC_NT), seg * 7 * 8 + seg * 8 + WC_NT * 4 + 16, st, chunks, fp, (const u32*)rows2, (const u64*)sbstart, bbase, (u64*)out);
		}
		else if (fp.rec8_in) YK_LAUNCH((k_part2_wc8<false>), dim3(n_chunks), dim3(WC_NT), seg * WC8_CAP * 8 + seg * 8 + WC_NT * 4 + 16, st, chunks, fp, (const u32*)rows2, (const u64*)sbstart, bbase, (u64*)out);
		else {                                                      /* the second sweep of a two-sweep partition: {hash, rank} records in */
			if (!lds_limit<k_part2_wc8r>(WC_SEG * WC8_CAP * 8 + WC_SEG * 8 + WC_NT * 4 + 16)) (void)hipGetLastError();
			YK_LAUNCH(k_part2_wc8r, dim3(n_chunks), dim3(WC_NT), seg * WC8_CAP * 8 + seg * 8 + WC_NT * 4 + 16, st, chunks, fp, (const u32*)rows2, bbase, (u64*)out);
		}
	} else if (n_chunks && wc && fp.rec8_in && fp.s2_bits <= 13 && fp.s2_bits >= 4) {
		/* tagged records in, {hash, rank} records out (the first sweep of a two-sweep partition; ranks beyond their field): the ring kernel with 16-byte stacks */
		if (!lds_limit<k_part2_wc8<true>>(160 * 1024 - 8192)) (void)hipGetLastError();
		const size_t l2 = wc_lds_bytes<4, WC_CAP, true>(fp.s2_bits < 11 ? 1 << fp.s2_bits : WC_SEG, WC_NT);
		YK_LAUNCH((k_part2_wc8<true>), dim3(n_chunks), dim3(WC_NT), l2, st, chunks, fp, (const u32*)rows2, (const u64*)sbstart, bbase, (u64*)out);
	} else if (n_chunks && wc && fp.s2_bits <= 13 && fp.s2_bits >= 4) {
		lds_limit<k_part2_wc<false>>(160 * 1024 - 256);
		const size_t l2 = wc_lds_bytes<4, WC_CAP, true>(fp.s2_bits < 11 ? 1 << fp.s2_bits : WC_SEG, WC_NT);
		YK_LAUNCH((k_part2_wc<false>), dim3(n_chunks), dim3(WC_NT), l2, st, chunks, fp, (const u32*)rows2, (const u64*)sbstart, bbase, out);
	} else if (n_chunks) YK_LAUNCH((k_part2<1>), dim3(n_chunks), dim3(nt), lds, st, chunks, fp, rows2, bbase, out);
}

int yk_rng_log(void)                      /* log2 slots per range; the env knob lets tests split small tables */
{
	const int v = (int)yk_knob("YAKAMD_RNG_LOG", RNG_LOG);
	return v < 5 ? 5 : v > RNG_LOG ? RNG_LOG : v;
}
int yk_hpart2_chunk(void) { return 131072; }

void yk_launch_hpart2(const Chunk2 *chunks, int n_chunks, const u32 *chunk_first, const u64 *bbase, ImgView img, int rb, int P,
                      u32 *rows2, u64 *sbstart, u64 *out, hipStream_t st)
{
	const int S2 = 1 << rb;
	lds_limit<k_hpart2<1>>(160 * 1024 - 256);
	if (n_chunks) YK_LAUNCH(k_hpart2<0>, dim3(n_chunks), dim3(WC_NT), sizeof(u32) * S2, st, chunks, img, rb, yk_rng_log(), rows2, (const u64*)sbstart, out);
	YK_LAUNCH(k_part2_scan, dim3(P), dim3(256), 0, st, chunk_first, bbase, rb, rows2, sbstart, P, 0);
	if (n_chunks) YK_LAUNCH(k_hpart2<1>, dim3(n_chunks), dim3(WC_NT), (wc_lds_bytes<8, XW_CAP_H, false>(S2, WC_NT)), st,
	                                 chunks, img, rb, yk_rng_log(), rows2, (const u64*)sbstart, out);
}

int yk_launch_img_count_rng(const u64 *rec, int cross, const u64 *sbstart, ImgView img, int plo, int phi, int rb, u32 max_len,
                            u64 *list, u32 *list_n, u32 list_cap, hipStream_t st)
{
	if (!lds_limit<k_img_count_rng<0>>(160 * 1024 - 256) || !lds_limit<k_img_count_rng<1>>(160 * 1024 - 256)) { (void)hipGetLastError(); return -1; }
	const size_t lds = (size_t)((max_len + 31) / 32) * 4 + (size_t)(max_len + 1) / 2 * 4 + 16;
	const dim3 grid((unsigned)(phi - plo) << rb), blk(1024);
	if (cross) YK_LAUNCH(k_img_count_rng<1>, grid, blk, lds, st, rec, sbstart, img, plo, rb, yk_rng_log(), list, list_n, list_cap);
	else YK_LAUNCH(k_img_count_rng<0>, grid, blk, lds, st, rec, sbstart, img, plo, rb, yk_rng_log(), list, list_n, list_cap);
	return 0;
}

void yk_launch_lds_count_ovf(FastParams fp, const u64 *sbstart, const Rec *rec,
                             u32 *bloom32, ImgView img, LcOut O, const u32 *ovf_list, u32 n_ovf, const u64 *scr_off,
                             u64 *scr, hipStream_t st)
{
	if (n_ovf) YK_LAUNCH(k_lds_count_ovf, dim3(n_ovf), dim3(256), 0, st, fp, sbstart, rec, bloom32, img,
	                              O, ovf_list, scr_off, scr);
}

size_t yk_count_own_lds(u32 range_len, u32 kmax) { return yk_plan_count_own_lds(range_len, kmax); }   /* (count_plan.h) */

/* records of any RecFmt, grouped by sub-table (bstart).  The format gives the kernel its two arguments: W, the record's stride in words, and ytag, how the
 * record's one word is read -- 0 the hash, 1 the range-tagged hash, 2 the tagged level-1 record */
int yk_launch_img_count_own(const void *rec, RecFmt fmt, int cross, const u64 *bstart, ImgView img, int plo, int phi, int rb, int rng_log, u32 kmax,
                            size_t lds, u64 *list, u32 *list_n, u32 list_cap, hipStream_t st)
{
	const int lds_max = 160 * 1024 - 256;
	if (!lds_limit<k_img_count_own<1, 0>>(lds_max) || !lds_limit<k_img_count_own<1, 1>>(lds_max) || !lds_limit<k_img_count_own<2, 0>>(lds_max) ||
	    !lds_limit<k_img_count_own<2, 1>>(lds_max)) { (void)hipGetLastError(); return -1; }
	const int ytag = fmt == YK_FMT_HASH_RNG ? 1 : fmt == YK_FMT_TAGGED ? 2 : 0;
	const int n_p = phi - plo;
	const dim3 grid((unsigned)((n_p + 7) / 8 * 8) << rb), blk(1024);
#define YK_OWN(Wv, Cv) YK_LAUNCH((k_img_count_own<Wv, Cv>), grid, blk, lds, st, (const u64*)rec, bstart, img, plo, n_p, rb, rng_log, kmax, list, list_n, list_cap, ytag)
	if (fmt != YK_FMT_POS) { if (cross) YK_OWN(1, 1); else YK_OWN(1, 0); }
	else { if (cross) YK_OWN(2, 1); else YK_OWN(2, 0); }
#undef YK_OWN
	return 0;
}

/* ---- replay2 launchers (grids: x = blocks per sub-table, y = sub-table) ---- */
void yk_r2_binit(const R2Tab *tabs, const R2Act *acts, int P, u32 bmax, u32 *OCC, u32 *USED, hipStream_t st)
{
	const u64 W = (2ull << bmax) / 32 + 1;                        /* bitmap words of the largest new table */
	YK_LAUNCH(k_r2_binit, dim3((unsigned)std::min<u64>((W + 1023) / 1024, 256), P), dim3(256), 0, st, tabs, acts, OCC, USED);
}
void yk_r2_dsmall(const R2Tab *tabs, const R2Act *acts, int P, u64 *K0, u64 *K1, u32 *TAG, u32 *OCC, u32 *USED, u32 *Fcur, u32 *Gcur, u32 *fail, hipStream_t st)
{
	const int defer = 1;                                          /* (0: the prefix lane follows every chain to its end -- the older, slower rule) */
	YK_LAUNCH(k_r2_dsmall, dim3(P), dim3(256), 0, st, tabs, acts, K0, K1, TAG, OCC, USED, Fcur, Gcur, fail, (u32)yk_r2_small_f(), defer);
}
int yk_r2_small_f(void)                                            /* YAKAMD_R2_SMALL_F: test / tuning knob, a power of two in [16, 4096] */
{
	int v = (int)yk_knob("YAKAMD_R2_SMALL_F", 16);   /* the fused rounds (k_r2_double) take over right behind the literal prefix: their chunk routine places a round's runs side by side where k_r2_dsmall walks them lane by lane */
	if (v < 16) v = 16;
	if (v > 4096) v = 4096;
	while (v & (v - 1)) v &= v - 1;
	return v;
}
/* the rounds of a doubling step from k_r2_dsmall's end (Fin) on in one launch (k_r2_double): n_dbl = sub-tables that double in this step */
int yk_r2_double(const R2Tab *tabs, const R2Act *acts, int P, int n_dbl, u64 *K0, u64 *K1, u32 *TAG, u32 *OCC, u32 *USED, const u32 *Fin, u32 *Fout, u32 *fail, hipStream_t st)
{
	/* many sub-tables: four workgroups per CU (all 1024 sub-tables of a default table resident at once); few, large ones (a shard of
	 * a multi-GPU job): 16 waves each.  YAKAMD_R2_DBL = 10 * waves + walks side by side (tests / tuning) */
	const int knob = (int)yk_knob("YAKAMD_R2_DBL", 51);              /* measured at a 1 Gb assembly: 5 waves 125.1 / 125.4 / 126.2 ms (1 / 2 / 4 walks side by side), 6 waves 130.4 / 128.3 / 129.1 */
	const int nw = n_dbl <= 256 ? 16 : knob / 10 == 6 ? 6 : 5, il = knob % 10 == 2 ? 2 : knob % 10 == 4 ? 4 : 1;
	static u64 *d_prof = 0;
	static const bool prof = getenv("YAKAMD_VERBOSE") && atoi(getenv("YAKAMD_VERBOSE")) > 1;
	if (prof && !d_prof) { hipMalloc((void**)&d_prof, 16 * 8); }
	if (prof) hipMemsetAsync(d_prof, 0, 16 * 8, st);
#define YK_DBL(NWv, PRv, ILv) YK_LAUNCH((k_r2_double<NWv, PRv, ILv>), dim3(P), dim3(64 * NWv), 0, st, tabs, acts, K0, K1, TAG, (const u32*)OCC, USED, (const u32*)Fin, Fout, fail, d_prof)
#define YK_DBL_IL(NWv, PRv) do { if (il == 1) YK_DBL(NWv, PRv, 1); else if (il == 4) YK_DBL(NWv, PRv, 4); else YK_DBL(NWv, PRv, 2); } while (0)
	if (nw >= 16) { if (prof) YK_DBL(16, true, 1); else YK_DBL(16, false, 1); }
	else if (nw == 5) { if (prof) YK_DBL(5, true, 1); else YK_DBL_IL(5, false); }
	else { if (prof) YK_DBL(6, true, 1); else YK_DBL_IL(6, false); }
#undef YK_DBL_IL
#undef YK_DBL
	if (prof) {
		u64 h[16];
		hipMemcpyAsync(h, d_prof, sizeof(h), hipMemcpyDeviceToHost, st);
		hipStreamSynchronize(st);
		if (h[8]) fprintf(stderr, "[yak_amd] k_r2_double<%d> 100 MHz ticks per wave (%llu waves): stage %llu, window+scans %llu, probing %llu, write-back %llu, medium runs %llu, round total %llu, barrier %llu, big runs %llu\n",
		                  nw, (unsigned long long)h[8], (unsigned long long)(h[0] / h[8]), (unsigned long long)(h[1] / h[8]), (unsigned long long)(h[2] / h[8]), (unsigned long long)(h[3] / h[8]),
		                  (unsigned long long)(h[4] / h[8]), (unsigned long long)(h[5] / h[8]), (unsigned long long)(h[6] / h[8]), (unsigned long long)(h[7] / h[8]));
	}
	return 0;
}
int yk_r2_seg_log(void) { const int v = (int)yk_knob("YAKAMD_R2_SEG_LOG", R2_SEG_LOG); return v < 10 ? 10 : v > R2_SEG_LOG ? R2_SEG_LOG : v; }   /* the knob lets tests split small tables */
int yk_r2_head(void) { const u32 seg = 1u << yk_r2_seg_log(); return (int)(seg / 2 < R2_HEAD ? seg / 2 : R2_HEAD); }
void yk_r2_place(const R2Tab *tabs, const R2Act *acts, int P, int p0, int np, u32 bmax, u64 *K0, u64 *K1, const u64 *kc, u64 *pk, u32 *pr, u32 *seg_start,
                 u32 *head, u64 *spill, u32 *spill_n, u32 spill_cap, u32 *fail, u32 *img_u, const u32 *USED, u32 *pcnt, int G, hipStream_t st)
{
	lds_limit<k_r2_place>(64 * 1024 + 8192 + 256);
	const u32 SL = (u32)yk_r2_seg_log(), HD = (u32)yk_r2_head();
	const u32 nseg = bmax > SL ? 1u << (bmax - SL) : 1, L = bmax > SL ? 1u << SL : 1u << bmax;
	hipMemsetAsync(spill_n, 0, 4, st);
	if (nseg > 1 && G > 1 && pcnt) {                              /* few sub-tables place: G workgroups each */
		YK_LAUNCH(k_r2_ppart_cnt, dim3(G, P), dim3(1024), 0, st, tabs, acts, kc, pcnt, SL);
		YK_LAUNCH(k_r2_ppart_scan, dim3(P), dim3(1024), 0, st, acts, pcnt, seg_start, SL, (u32)G);
		YK_LAUNCH(k_r2_ppart_scat, dim3(G, P), dim3(1024), 0, st, tabs, acts, kc, pk, pr, (const u32*)pcnt, SL);
	} else if (nseg > 1) YK_LAUNCH(k_r2_ppart, dim3(P), dim3(1024), 0, st, tabs, acts, kc, pk, pr, seg_start, SL);
	const int pt = 1024;
	YK_LAUNCH(k_r2_place, dim3(nseg, np), dim3(pt), (size_t)L * 4 + (pt / 64) * 512, st, tabs, acts, K0, K1, kc, (const u64*)pk, (const u32*)pr, (const u32*)seg_start, head, spill, spill_n, spill_cap, fail, SL, HD, img_u, (u32)p0, USED);
	if (nseg > 1) {
		YK_LAUNCH(k_r2_spill, dim3(64), dim3(256), 0, st, acts, (const u64*)spill, (const u32*)spill_n, spill_cap, head, fail, HD);
			YK_LAUNCH(k_r2_headfill, dim3(nseg, np), dim3(256), 0, st, tabs, acts, K0, K1, kc, (const u32*)head, SL, HD, img_u, (u32)p0);
		}
}
void yk_r2_load(const R2Tab *tabs, const R2Load *ld, int P, u32 bmax, const u64 *src1, const u64 *src2, u64 *K0, u64 *K1, u32 *USED, hipStream_t st)
{
	const u64 n = 1ull << bmax;
	YK_LAUNCH(k_r2_load, dim3((unsigned)std::min<u64>((n + 1023) / 1024, 4096), P), dim3(256), 0, st, tabs, ld, src1, src2, K0, K1, USED);
}
void yk_r2_trail(const u64 *lastput, const u64 *rec_t, const u64 *rec_off, const u32 *m, int P, u32 *out, hipStream_t st)
{
	YK_LAUNCH(k_r2_trail, dim3((P + 255) / 256), dim3(256), 0, st, lastput, rec_t, rec_off, m, P, out);
}
void yk_r2_publish(const R2Tab *tabs, const R2Pub *pub, int P, u32 bmax, const u64 *K0, const u64 *K1, u64 *nk, u32 *nu, hipStream_t st)
{
	const u64 n = 1ull << bmax;
	YK_LAUNCH(k_r2_publish, dim3((unsigned)std::min<u64>((n + 1023) / 1024, 4096), P), dim3(256), 0, st, tabs, pub, K0, K1, nk, nu);
}

int yk_lc2_ok(FastParams fp)
{
	const int on = (int)yk_knob("YAKAMD_LC2", 1);          /* 0: the older three-tier kernels (tests) */
	if (!on || fp.n_hash > 32) return 0;
	if (fp.bloom_mode) { const int lb = fp.nb - 9 - fp.s2_bits; if (lb < 0 || lb > (fp.bf_nowb ? 8 : 7)) return 0; }   /* a staged range holds 128 blocks; without a stage (bf_nowb) the table gives a block >= 4 home slots */
	return 1;
}
int yk_lc2_per_sb(int bloom_mode)       /* mean records per sub-bucket the counting kernel is built for (engine_slice.cpp sizes the level-2 partition by it) */
{
	if (bloom_mode) return 1800;
	return yk_knob("YAKAMD_LC2", 1) != 0 && yk_knob("YAKAMD_LC2_CAPB", 11) >= 11 ? 1200 : 600;
}

void yk_launch_lc2(FastParams fp, const u64 *sbstart, const Rec *rec, u32 *bloom32, ImgView img, LcOut O, u64 *counters, u32 *ovf_list, hipStream_t st)
{
	const unsigned n_sb = (unsigned)(fp.phi - fp.plo) << fp.s2_bits;
	/* 5 workgroups of 32 KB LDS are resident per CU; the grid is 64 times that, each workgroup walking every gridDim-th sub-bucket (~25 of 2 M): the
	 * dispatcher hands a new one to whichever slot frees first.  Measured on 10 M reads: 1280 workgroups 15.4 ms, 10240 14.2, 81920 13.4, 655360 13.8,
	 * one per sub-bucket 15.0 (30 M reads: 48.9 -> 39.3 ms) */
	const int wgs = (int)yk_knob("YAKAMD_LC2_WGS", 256 * 5 * 64);
	const unsigned grid = n_sb < (unsigned)wgs ? n_sb : (unsigned)wgs;
	if (grid) {
#define YK_LC2X(B, I, Pf, R8, S, C) YK_LAUNCH((k_lc2<B, I, Pf, R8, S, C>), dim3(grid), dim3(256), 0, st, fp, sbstart, rec, bloom32, img, O, counters, ovf_list, n_sb)
#define YK_LC2(B, I, Pf) do { if constexpr (!B) { if (cap11) { if (fp.rec8_out) YK_LC2X(false, I, Pf, true, false, 11); else YK_LC2X(false, I, Pf, false, false, 11); } \
                                                  else if (fp.rec8_out) YK_LC2X(false, I, Pf, true, false, 10); else YK_LC2X(false, I, Pf, false, false, 10); } \
                              else { if (fp.rec8_out) YK_LC2X(true, I, Pf, true, true, 10); else YK_LC2X(true, I, Pf, false, true, 10); } } while (0)
		const bool cap11 = yk_lc2_per_sb(0) == 1200;                  /* no filter: the 2048-slot table (engine_slice.cpp made the sub-buckets for it) */
		/* an untouched filter whose bits nobody reads (engine_slice.cpp: one-slice pass into an empty table, records kept): no stage in LDS */
		const bool nostage = fp.bloom_mode && fp.bf_nowb && fp.bf_virgin && !fp.img_nonempty && fp.rec8_out && yk_knob("YAKAMD_LC2_NOSTAGE", 1) != 0;
		const int v = (fp.bloom_mode ? 4 : 0) | (fp.img_nonempty ? 2 : 0) | ((fp.dbg & 128) ? 1 : 0);
		if (nostage) {
			if (fp.dbg & 128) YK_LC2X(true, false, true, true, false, 10);
			else if (yk_knob("YAKAMD_LC2_W6", 1)) YK_LAUNCH((k_lc2<true, false, false, true, false, 10, 6>), dim3(grid), dim3(256), 0, st, fp, sbstart, rec, bloom32, img, O, counters, ovf_list, n_sb);
			else YK_LC2X(true, false, false, true, false, 10);
		}
		else switch (v) {
		case 0: YK_LC2(false, false, false); break;
		case 1: YK_LC2(false, false, true); break;
		case 2: YK_LC2(false, true, false); break;
		case 3: YK_LC2(false, true, true); break;
		case 4: YK_LC2(true, false, false); break;
		case 5: YK_LC2(true, false, true); break;
		case 6: YK_LC2(true, true, false); break;
		default: YK_LC2(true, true, true); break;
		}
#undef YK_LC2
#undef YK_LC2X
	}
	if (grid && (fp.dbg & 128)) {
		u64 h[8];
		hipStreamSynchronize(st);
		hipMemcpyFromSymbol(h, HIP_SYMBOL(d_lc2_prof), sizeof(h));
		if (h[4]) fprintf(stderr, "[yak_amd] k_lc2 clocks per sub-bucket (lane 0, mean over %llu): A %llu, gate %llu, set+select %llu, write-back+clean %llu; inside A: wait for the records %llu, lane 0's puts %llu\n", (unsigned long long)h[4],
		                  (unsigned long long)(h[0] / h[4]), (unsigned long long)(h[1] / h[4]), (unsigned long long)(h[2] / h[4]), (unsigned long long)(h[3] / h[4]), (unsigned long long)(h[5] / h[4]), (unsigned long long)(h[6] / h[4]));
		for (int i = 0; i < 8; ++i) h[i] = 0;
		hipMemcpyToSymbol(HIP_SYMBOL(d_lc2_prof), h, sizeof(h));
	}
}

void yk_launch_lc_sum(const u32 *nsel, int s2_bits, int plo, int phi, u32 *seg_cnt, hipStream_t st)
{
	YK_LAUNCH(k_lc_sum, dim3(phi - plo), dim3(256), 0, st, nsel, s2_bits, plo, seg_cnt);
}

void yk_launch_bf_rebuild(FastParams fp, const u64 *sbstart, const Rec *rec, u32 *bloom32, hipStream_t st)
{
	const u32 n_sb = (u32)(fp.phi - fp.plo) << fp.s2_bits;
	const u32 grid = std::min<u32>(n_sb, 256 * 8 * 16);
	if (grid) YK_LAUNCH(k_bf_rebuild, dim3(grid), dim3(256), 0, st, fp, sbstart, rec, bloom32, n_sb);
}
void yk_launch_lc_sum3(LcOut O, int s2_bits, int plo, int phi, u64 t_pass0, u32 *seg_cnt, u64 *lastput, u32 *ndist_p, hipStream_t st)
{
	YK_LAUNCH(k_lc_sum3, dim3(phi - plo), dim3(256), 0, st, O, s2_bits, plo, t_pass0, seg_cnt, lastput, ndist_p);
}
void yk_launch_lc_gather(LcOut O, const u64 *sbstart, const u64 *key_off, int s2_bits, int plo, int phi, u64 *out_kc, u64 *out_T, Rec *out_kt, u32 *out_c2, hipStream_t st)
{
	const u32 n_sb = (u32)(phi - plo) << s2_bits;
	const u32 grid = (u32)std::min<u64>(((u64)n_sb + 255) / 256, 256 * 8 * 16);
	if (grid) YK_LAUNCH(k_lc_gather, dim3(grid), dim3(256), 0, st, O, sbstart, key_off, (u32)plo << s2_bits, n_sb, out_kc, out_T, out_kt, out_c2);
}
void yk_launch_lc_compact(LcOut O, const u64 *sbstart, int s2_bits, int plo, int phi, u64 t_pass0, const u64 *seg_base,
                          u64 *out_kc, u64 *out_T, u64 *lastput, u32 *ndist_p, Rec *out_kt, u32 *out_c2, hipStream_t st)
{
	YK_LAUNCH(k_lc_compact, dim3(phi - plo), dim3(256), 0, st, O, sbstart, s2_bits, plo, t_pass0, seg_base, out_kc, out_T, lastput, ndist_p, out_kt, out_c2);
}

void yk_launch_seg_sort_pass2(const u64 *seg_base, const u32 *seg_cnt, int P, const u64 *src_kc, const u64 *src_t,
                              u64 *dst_kc, u64 *dst_t, int shift, u32 *dig_hist, int n_dig, hipStream_t st, int big)
{
	/* long segments (an assembly: ~1 M keys per sub-table): 1024 threads per sub-table */
	if (big) YK_LAUNCH((k_seg_sort_pass<8, 1024>), dim3(P), dim3(1024), 0, st, seg_base, seg_cnt, src_kc, src_t, dst_kc, dst_t, shift, dig_hist, n_dig);
	else YK_LAUNCH((k_seg_sort_pass<8, 256>), dim3(P), dim3(256), 0, st, seg_base, seg_cnt, src_kc, src_t, dst_kc, dst_t, shift, dig_hist, n_dig);
}
void yk_launch_cnt2(FastParams fp, const u64 *sbstart, const Rec *rec, const u64 *key_off, const u64 *key_kc, const u64 *seg_base, u32 *key_cnt, ImgView img, u64 n_keys, u32 *used_delta, hipStream_t st)
{
	const u32 n_sb = (u32)(fp.phi - fp.plo) << fp.s2_bits;
	/* eight workgroups of 256 threads per CU are the wave slots (the big table's LDS allows six); the grid is far larger, for the same reason as
	 * k_lc2's: 2048 workgroups 8.1 ms (count + apply), 8192 6.9, 65536 6.6, 262144 6.5 */
	const int wgs = (int)yk_knob("YAKAMD_CNT2_WGS", 256 * 1024);
	const int small_max = (int)yk_knob("YAKAMD_CNT2_SMALL", 128);   /* mean keys per sub-bucket up to which the small LDS table is used (a fuller sub-bucket falls back to table lookups: exact, slow) */
	const dim3 grid(std::min<u32>(n_sb, (u32)std::max(1, wgs)));
	if (n_sb && small_max >= 0 && n_keys / n_sb <= (u64)small_max) YK_LAUNCH((k_cnt2<512, 320>), grid, dim3(256), 0, st, fp, sbstart, rec, key_off, key_kc, img, n_sb, key_cnt, used_delta);
	else YK_LAUNCH((k_cnt2<2048, 1280>), grid, dim3(256), 0, st, fp, sbstart, rec, key_off, key_kc, img, n_sb, key_cnt, used_delta);
	yk_launch_cnt2_apply(fp, key_kc, key_cnt, seg_base, img, st);
}
void yk_launch_cnt2_apply(FastParams fp, const u64 *key_kc, const u32 *key_cnt, const u64 *seg_base, ImgView img, hipStream_t st, int fix)
{
	const int n_p = fp.phi - fp.plo;
	const int per = std::max(1, 8192 / std::max(1, n_p));                  /* ~8 K workgroups in all */
	YK_LAUNCH(k_cnt2_apply, dim3(per, n_p), dim3(256), 0, st, key_kc, key_cnt, seg_base, fp.plo, fp.pre, img, fix);
}
void yk_launch_nsel_scan(const u32 *nsel, int s2_bits, int plo, int phi, int P, const u64 *seg_base, u64 *key_off, hipStream_t st)
{
	YK_LAUNCH(k_nsel_scan, dim3(P), dim3(256), 0, st, nsel, s2_bits, plo, phi, P, seg_base, key_off);
}

static int cu_count()                                             /* the compute units of the current device, for the persistent grids below; 256 if it does not tell */
{
	int dev = 0, n_cu = 0;
	return hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n_cu >= 1 ? n_cu : 256;
}

/* yak inspect's join (kern_inspect.inc): one persistent grid over the n keys, as many workgroups as the LDS lets share a CU (the 64 KiB corner
 * histogram, B's sub-table directory and A's offsets: 80 KiB at pre 10, two per CU), never fewer than n / 2^31 (a corner bin is a u32) */
int yk_launch_inspect(const u64 *keys, const u64 *off, u64 n, int n_sub, int sub_lo, int hdr, int pre_a, int has_b, ImgView img, int blo, int bhi,
                      int ref, u64 *J, hipStream_t st)
{
	if (n == 0) return 0;
	InArgs a;
	a.keys = keys; a.off = off; a.n = n; a.J = J; a.n_sub = n_sub; a.sub_lo = sub_lo; a.hdr = hdr; a.pre_a = pre_a;
	a.blo = blo; a.bhi = bhi; a.ref = ref;
	a.tab_b = has_b && img.pre <= 12;
	a.tab_a = n_sub <= 4096;
	const size_t lds = IN_CORNER_BYTES + (a.tab_b ? (size_t)8 << img.pre : 0) + (a.tab_a ? (size_t)8 * n_sub : 0);
	const int n_cu = cu_count();
	const u64 per_cu = std::max<u64>(1, std::min<u64>(4, (u64)(160 * 1024) / lds));
	const u64 steps = (n + IN_THREADS * IN_U - 1) / (IN_THREADS * IN_U);
	const u64 grid = std::max<u64>(std::min<u64>((u64)n_cu * per_cu, steps), (n >> 31) + 1);
	const bool lng = img.k >= 32;
	lds_limit<k_inspect<false, false>>(160 * 1024);
	lds_limit<k_inspect<true, false>>(160 * 1024);
	lds_limit<k_inspect<true, true>>(160 * 1024);
	if (!has_b) YK_LAUNCH((k_inspect<false, false>), dim3((unsigned)grid), dim3(IN_THREADS), lds, st, a, img);
	else if (lng) YK_LAUNCH((k_inspect<true, true>), dim3((unsigned)grid), dim3(IN_THREADS), lds, st, a, img);
	else YK_LAUNCH((k_inspect<true, false>), dim3((unsigned)grid), dim3(IN_THREADS), lds, st, a, img);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* `yak-amd depth` (kern_depth.inc).  short: the n_win windows from g0 on, out[i] = window g0 + i; the long ones (more than T positions) go to
 * long_list / tile_base (long_cap entries) and are counted, with their tiles, in *counter (zeroed by the caller).  long: the tiles [tile0, tile0 +
 * n_tiles) of the slots [slot0, slot0 + n_slots) into hist (1024 zeroed u64 bins per slot); finish: those slots' windows from their bins */
int yk_dp_run(void) { return DP_RUN; }
void yk_launch_dp_short(DpArgs a, u64 g0, u32 n_win, u32 T, void *out, u32 *long_list, u64 *tile_base, u32 long_cap, u64 *counter, hipStream_t st)
{
	if (n_win == 0) return;
	const u64 want = ((u64)n_win + DP_THREADS / WAVE - 1) / (DP_THREADS / WAVE);
	YK_LAUNCH(k_dp_short, dim3((unsigned)std::min<u64>(want, 65536)), dim3(DP_THREADS), 0, st, a, g0, n_win, T, (DpOut*)out, long_list, tile_base,
	                   long_cap, (unsigned long long*)counter);
}
void yk_launch_dp_long(DpArgs a, u64 g0, const u32 *long_list, const u64 *tile_base, u32 slot0, u32 n_slots, u64 tile0, u64 n_tiles, u64 *hist, hipStream_t st)
{
	if (n_tiles) YK_LAUNCH(k_dp_long, dim3((unsigned)n_tiles), dim3(DP_THREADS), 0, st, a, g0, long_list, tile_base, slot0, n_slots, tile0,
	                                (unsigned long long*)hist);
}
void yk_launch_dp_finish(const u64 *hist, const u32 *long_list, u32 slot0, u32 n_slots, void *out, hipStream_t st)
{
	if (n_slots == 0) return;
	const u32 want = (n_slots + DP_THREADS / WAVE - 1) / (DP_THREADS / WAVE);
	YK_LAUNCH(k_dp_finish, dim3(std::min<u32>(want, 65536)), dim3(DP_THREADS), 0, st, (const unsigned long long*)hist, long_list, slot0, n_slots, (DpOut*)out);
}

/* `yak-amd hetmers` (kern_hetmer.inc): one persistent grid over the n staged keys of sub-tables [sub_lo, sub_lo + n_sub), probing the whole image.
 * mode 0: the group tallies and J (LDS: the 64 KiB corner, the directory while pre <= 12, the offsets while n_sub <= 4096 -- 80 KiB at pre 10, two
 * workgroups per CU); mode 1: the pairs per tile into tile_cnt; mode 2: the records at tile_off.  The three modes run the same grid -- the one
 * mode 0's LDS allows -- so a key is taken by the same workgroup and step in each.  0, or -1 if the launch failed */
u64 yk_hetmer_tiles(u64 n) { return (n + HM_THREADS - 1) / HM_THREADS; }
int yk_launch_hetmer(int mode, const u64 *keys, const u64 *off, u64 n, int n_sub, int sub_lo, int min_cnt, ImgView img, u64 *J, u64 *group,
                     u32 *tile_cnt, const u64 *tile_off, void *list, hipStream_t st)
{
	if (n == 0) return 0;
	if (img.k < 1 || img.k > 31 || !(img.k & 1) || mode < 0 || mode > 2 || (yk_hetmer_tiles(n) >> 31)) return -1;
	HmArgs a;
	a.img = keys; a.off = off; a.n = n; a.J = J; a.group = group; a.tile_cnt = tile_cnt; a.tile_off = tile_off; a.list = (u64*)list;
	a.n_sub = n_sub; a.sub_lo = sub_lo; a.k = img.k; a.min_cnt = min_cnt;
	a.tab = img.pre <= 12;
	a.tab_off = n_sub <= 4096;
	const size_t lds = (mode == 0 ? HM_CORNER_BYTES : 0) + (a.tab ? (size_t)8 << img.pre : 0) + (a.tab_off ? (size_t)8 * n_sub : 0);
	const int n_cu = cu_count();
	const u64 per_cu = std::max<u64>(1, std::min<u64>(4, (u64)(160 * 1024) / (lds + (mode == 0 ? 0 : HM_CORNER_BYTES))));
	const u64 grid = std::max<u64>(std::min<u64>((u64)n_cu * per_cu, yk_hetmer_tiles(n)), (n >> 31) + 1);
	/* 128 KiB is the most a launch asks for (the corner, 32 KiB of directory at pre 12, 32 KiB of offsets); COUNT and WRITE hold 32 bytes of static
	 * LDS besides, so the whole 160 KiB cannot be asked for as dynamic */
	if (!lds_limit<k_hetmer<HM_TALLY>>(128 * 1024) || !lds_limit<k_hetmer<HM_COUNT>>(128 * 1024) || !lds_limit<k_hetmer<HM_WRITE>>(128 * 1024)) return -1;
	if (mode == 0) YK_LAUNCH((k_hetmer<HM_TALLY>), dim3((unsigned)grid), dim3(HM_THREADS), lds, st, a, img);
	else if (mode == 1) YK_LAUNCH((k_hetmer<HM_COUNT>), dim3((unsigned)grid), dim3(HM_THREADS), lds, st, a, img);
	else YK_LAUNCH((k_hetmer<HM_WRITE>), dim3((unsigned)grid), dim3(HM_THREADS), lds, st, a, img);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* `yak-amd unitigs` (kern_graph.inc).  The grids are persistent ones over the tiles [t_lo, t_hi) of the arena; the LDS is the sub-table directory
 * while pre <= 12 (32 KiB at the most).  what 0: the edge bytes and the degree tallies, `inflight` (4, or 8) probes requested together; 1: the rank
 * directory, one workgroup per sub-table; 2: tally[25] += linked sides; 3: the records of the tiles' keys.  grid_want > 0: that many workgroups
 * instead of four per CU (a test switch: no result depends on it).  0, or -1 if the launch failed */
u64 yk_graph_tile(void) { return GR_THREADS; }
int yk_launch_graph(int what, int inflight, int grid_want, const u64 *tile0, const u64 *key0, uint8_t *edges, u32 *wrank, u64 *tally, u64 t_lo, u64 t_hi, u64 n_slots,
                    int P, int min_cnt, void *out, u64 out_key0, u64 out_n, ImgView img, hipStream_t st)
{
	if (img.k < 1 || img.k > 31 || !(img.k & 1) || what < 0 || what > 3 || t_hi < t_lo || P != 1 << img.pre) return -1;
	GrArgs a;
	a.tile0 = tile0; a.key0 = key0; a.edges = edges; a.wrank = wrank; a.tally = tally; a.out = (u64*)out; a.out_key0 = out_key0; a.out_n = out_n;
	a.t_lo = t_lo; a.t_hi = t_hi; a.n_slots = n_slots; a.P = P; a.k = img.k; a.min_cnt = min_cnt;
	a.tab = img.pre <= 12;
	if (what == 1) {
		YK_LAUNCH(k_graph_rank, dim3((unsigned)P), dim3(256), 0, st, a, img);
		return hipGetLastError() == hipSuccess ? 0 : -1;
	}
	if (t_hi == t_lo) return 0;
	const size_t lds = a.tab ? (size_t)8 << img.pre : 0;
	const int n_cu = cu_count();
	const u64 grid = std::max<u64>(std::min<u64>(grid_want > 0 ? (u64)grid_want : (u64)n_cu * 4, t_hi - t_lo), 1);
	if (what == 0 && inflight == 8) YK_LAUNCH((k_graph_edges<8>), dim3((unsigned)grid), dim3(GR_THREADS), lds, st, a, img);
	else if (what == 0) YK_LAUNCH((k_graph_edges<4>), dim3((unsigned)grid), dim3(GR_THREADS), lds, st, a, img);
	else if (what == 2) YK_LAUNCH((k_graph_link<GR_COUNT>), dim3((unsigned)grid), dim3(GR_THREADS), lds, st, a, img);
	else YK_LAUNCH((k_graph_link<GR_EMIT>), dim3((unsigned)grid), dim3(GR_THREADS), lds, st, a, img);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* homopolymer compression (kern_hpc.inc).  valid == 0: `in` is the ASCII image; valid != 0: the packed one (code words at `in`).  Tiles of
 * yk_hpc_tile(packed) positions; tcnt = yk_hpc_tiles() words, toff = their exclusive scan (yk_launch_te_scan), one word more */
int64_t yk_hpc_tile(int packed) { return (int64_t)HP_THREADS * (packed ? (int)HpPacked::PER : (int)HpAscii::PER); }
int64_t yk_hpc_tiles(int packed, int64_t n) { return (n + yk_hpc_tile(packed) - 1) / yk_hpc_tile(packed); }
void yk_launch_hpc_count(const void *in, const u32 *valid, int64_t n, u32 *tcnt, hipStream_t st)
{
	const int64_t nt = yk_hpc_tiles(valid != 0, n);
	if (nt <= 0) return;
	if (valid) YK_LAUNCH(k_hpc_count<HpPacked>, dim3((unsigned)nt), dim3(HP_THREADS), 0, st, HpPacked{ (const u32*)in, valid }, n, tcnt);
	else YK_LAUNCH(k_hpc_count<HpAscii>, dim3((unsigned)nt), dim3(HP_THREADS), 0, st, HpAscii{ (const uint8_t*)in }, n, tcnt);
}
void yk_launch_hpc_scatter(const void *in, const u32 *valid, int64_t n, const u64 *toff, uint8_t *out, hipStream_t st)
{
	const int64_t nt = yk_hpc_tiles(valid != 0, n);
	if (nt <= 0) return;
	if (valid) YK_LAUNCH(k_hpc_scatter<HpPacked>, dim3((unsigned)nt), dim3(HP_THREADS), 0, st, HpPacked{ (const u32*)in, valid }, n, toff, nt, out);
	else YK_LAUNCH(k_hpc_scatter<HpAscii>, dim3((unsigned)nt), dim3(HP_THREADS), 0, st, HpAscii{ (const uint8_t*)in }, n, toff, nt, out);
}
/* one wave per sequence; toff = the scan of the ASCII form's tiles */
void yk_launch_hpc_remap(const uint8_t *a, int64_t n, const u64 *toff, const u64 *off, const u32 *len, int64_t n_seq, u64 *off_out, u32 *len_out, hipStream_t st)
{
	if (n_seq <= 0) return;
	const int64_t nb = (n_seq + HP_THREADS / WAVE - 1) / (HP_THREADS / WAVE);
	YK_LAUNCH(k_hpc_remap, dim3((unsigned)nb), dim3(HP_THREADS), 0, st, HpAscii{ a }, n, toff, off, len, n_seq, off_out, len_out);
}

} /* extern "C" */
