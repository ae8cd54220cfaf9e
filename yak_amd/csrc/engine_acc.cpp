/* engine_acc.cpp -- the accumulator ("general") path of a create pass: acc_records takes a batch (accumulator insert, bloom gate, last put-calls),
 * acc_finish lays the pass's new keys out at its end (select, the stable sort passes by insertion time, the layout replay).  The exclusive-ownership
 * path, which keeps its batches and counts them as slices, is in engine_slice.cpp. */
#include "engine_int.h"
#include "seg_sort_tile.h"

/* make room for `incoming` more distinct keys at a load factor <= 0.6 */
static int acc_reserve(yakamd_ctx *c, u64 incoming)
{
	PassBufs &ps = c->pass;
	const u64 need = ps.acc_count + incoming;
	int want = std::max(c->pre + 2, ceil_log2_u64((u64)(need / 0.6) + 1));
	if (want < 12) want = 12;
	if (ps.acc.s && ps.acc.bits >= want) return 0;
	AccTab nt;
	DevBuf<AccSlot> mem;
	nt.bits = want; nt.pre = c->pre; nt.mask = (1ull << want) - 1;
	if (mem.alloc((size_t)1 << want)) return -1;
	nt.s = mem;
	yk_launch_acc_init(nt.s, 1ull << want, c->st);
	if (ps.acc.s) {
		yk_launch_acc_rehash(ps.acc, nt, c->st);
		HIPCK(hipStreamSynchronize(c->st));
	}
	ps.acc_mem = std::move(mem);                               /* (frees the old table) */
	ps.acc = nt;
	return 0;
}

/* bloom gate over the keys first seen in the batch just inserted (kernels.hip K2) */
static int bloom_phases(yakamd_ctx *c, u64 n_new)
{
	if (n_new == 0) return 0;
	const BloomView bf = bloom_view(c);
	u64 h_cnt[YKC_N];
	EvTimer tm(c->st);
	HIPCK(hipMemsetAsync(c->d_counters + YKC_ANYMULTI, 0, 3 * 8, c->st));   /* ANYMULTI, NCAND, NMARKED */
	yk_launch_bf_test(c->pass.acc, c->pass.newlist, n_new, bf, c->pass.miss, c->st);
	yk_launch_bf_set(c->pass.acc, c->pass.newlist, n_new, bf, c->pass.miss, c->d_multi, c->multi_bits, c->d_counters, c->st);
	HIPCK(hipMemcpyAsync(h_cnt, c->d_counters, sizeof(h_cnt), hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	if (h_cnt[YKC_ANYMULTI]) {
		yk_launch_bf_check(c->pass.acc, c->pass.newlist, n_new, bf, c->pass.miss, c->d_multi, c->multi_bits, c->pass.cand, c->d_counters, c->st);
		HIPCK(hipMemcpyAsync(h_cnt, c->d_counters, sizeof(h_cnt), hipMemcpyDeviceToHost, c->st));
		HIPCK(hipStreamSynchronize(c->st));
		const u64 n_cand = h_cnt[YKC_NCAND], n_marked = h_cnt[YKC_NMARKED];
		if (n_cand) {
			const int map_bits = std::max(10, ceil_log2_u64(2 * n_marked + 2));
			DevBuf<u64> d_map;
			if (d_map.alloc((size_t)2 << map_bits)) return -1;
			HIPCK(hipMemsetAsync(d_map, 0, (size_t)16 << map_bits, c->st));
			yk_launch_bf_mapfill(c->pass.acc, c->pass.newlist, n_new, bf, c->pass.miss, c->d_multi, c->multi_bits, d_map, map_bits, c->st);
			yk_launch_bf_resolve(c->pass.acc, c->pass.newlist, c->pass.cand, n_cand, bf, c->pass.miss, d_map, map_bits, c->st);
			HIPCK(hipStreamSynchronize(c->st));
			c->st_cur.n_bloom_candidates += (int64_t)n_cand;
		}
		HIPCK(hipMemsetAsync(c->d_multi, 0, (size_t)1 << (c->multi_bits - 3), c->st));
	}
	c->st_cur.ms_bloom += tm.stop();
	return 0;
}

/* per sub-table time of the last put-call of this batch (see k_lastput) */
static int lastput_phase(yakamd_ctx *c, const Rec *d_rec, int64_t n_rec, u64 t0, u64 batch_lo, u64 batch_hi, int img_nonempty)
{
	const int64_t tail = env_i64("YAKAMD_LASTPUT_TAIL", 4 << 20);
	const u64 t_from = (batch_hi - batch_lo > (u64)tail) ? batch_hi - (u64)tail : batch_lo;
	const ImgView img = img_view(c);
	u32 n_missing = 0;
	HIPCK(hipMemsetAsync(c->d_lpbatch, 0, c->P * 8, c->st));
	HIPCK(hipMemsetAsync(c->d_missing, 0, ((c->P + 31) / 32) * 4, c->st));
	HIPCK(hipMemsetAsync(c->d_nmissing, 0, 4, c->st));
	yk_launch_lastput(d_rec, n_rec, t0, t_from, c->pass.acc, img, img_nonempty, c->bloom_mode, 0, c->d_lpbatch, c->st);
	yk_launch_lastput_merge(c->d_lastput, c->d_lpbatch, c->d_missing, c->d_nmissing, c->P, c->plo, c->phi, c->st);
	if (t_from > batch_lo) {
		HIPCK(hipMemcpyAsync(&n_missing, c->d_nmissing, 4, hipMemcpyDeviceToHost, c->st));
		HIPCK(hipStreamSynchronize(c->st));
		if (n_missing) {    /* the tail did not reach every sub-table: scan the whole batch for those */
			yk_launch_lastput(d_rec, n_rec, t0, batch_lo, c->pass.acc, img, img_nonempty, c->bloom_mode, c->d_missing, c->d_lpbatch, c->st);
			HIPCK(hipMemsetAsync(c->d_nmissing, 0, 4, c->st));
			yk_launch_lastput_merge(c->d_lastput, c->d_lpbatch, c->d_missing, c->d_nmissing, c->P, c->plo, c->phi, c->st);
		}
	}
	return 0;
}

/* the bloom gate's lists for a batch of n records: the three grow together, the old ones freed before the first new one is asked for */
static int new_reserve(yakamd_ctx *c, int64_t n)
{
	PassBufs &ps = c->pass;
	if (!c->bloom_mode || (size_t)n <= ps.newlist.cap()) return 0;
	ps.newlist.reset(); ps.miss.reset(); ps.cand.reset();
	return ps.newlist.reserve((size_t)n) || ps.miss.reserve((size_t)n * bloom_view(c).mw) || ps.cand.reserve((size_t)n) ? -1 : 0;
}

int acc_records(yakamd_ctx *c, const Rec *rec, int64_t n_rec, u64 t0, u64 batch_lo, u64 batch_hi)
{
	ImgView img = img_view(c);
	const int img_nonempty = c->img_keys_total > 0;
	if (img_nonempty) { if (delta_ensure(c)) return -1; c->delta_dirty = true; img = img_view(c); }   /* the view above was taken before the delta array existed: k_acc_insert adds to img.delta */
	if (c->bloom_mode && bloom_materialise(c)) return -1;
	if (acc_reserve(c, (u64)n_rec) || new_reserve(c, n_rec)) return -1;
	u64 h_cnt[YKC_N];
	{
		EvTimer tm(c->st);
		yk_launch_acc_insert(rec, n_rec, t0, c->pass.acc, img, img_nonempty, c->bloom_mode,
		                     c->bloom_mode ? c->pass.newlist : 0, c->d_counters, c->st);
		insert_ms(c, tm);
	}
	HIPCK(hipMemcpyAsync(h_cnt, c->d_counters, sizeof(h_cnt), hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	const u64 n_new = h_cnt[YKC_NEW];
	c->pass.acc_count += n_new;
	HIPCK(hipMemsetAsync(c->d_counters + YKC_NEW, 0, 8, c->st));
	if (c->bloom_mode && bloom_phases(c, n_new)) return -1;
	return lastput_phase(c, rec, n_rec, t0, batch_lo, batch_hi, img_nonempty);
}

int acc_finish(yakamd_ctx *c, int64_t *n_ins)
{
	const int P = c->P;
	if (c->fast && fast_abandon(c)) return -1;          /* cannot happen today; keeps the invariant explicit */
	const u64 before = c->keys_at_begin;                 /* slices counted earlier in this pass included */
	if (c->img_keys_total && c->d_delta) yk_launch_img_fold(img_view(c), c->n_slots, c->st);   /* put-calls that hit existing keys */
	std::vector<u32> m(P, 0);
	std::vector<u64> seg_off(P + 1, 0);
	DevBuf<u64> kc[2], tt[2], d_segoff; DevBuf<u32> d_segcur, d_segcnt;
	if (d_segcnt.alloc(P) || d_segcur.alloc(P) || d_segoff.alloc(P + 1)) return -1;
	HIPCK(hipMemsetAsync(d_segcnt, 0, P * 4, c->st));
	HIPCK(hipMemsetAsync(d_segcur, 0, P * 4, c->st));
	int cur = 0;
	if (c->pass.acc.s) {
		{
			EvTimer tm(c->st);
			yk_launch_select_count(c->pass.acc, c->bloom_mode, P, d_segcnt, c->st);
			HIPCK(hipMemcpyAsync(m.data(), d_segcnt, P * 4, hipMemcpyDeviceToHost, c->st));
			HIPCK(hipStreamSynchronize(c->st));
			for (int p = 0; p < P; ++p) seg_off[p + 1] = seg_off[p] + m[p];
			const u64 tot = seg_off[P];
			if (kc[0].alloc(tot) || kc[1].alloc(tot) || tt[0].alloc(tot) || tt[1].alloc(tot)) return -1;
			HIPCK(hipMemcpyAsync(d_segoff, seg_off.data(), (P + 1) * 8, hipMemcpyHostToDevice, c->st));
			yk_launch_select_scatter(c->pass.acc, c->bloom_mode, P, d_segoff, d_segcur, kc[0], tt[0], c->st);
			c->st_cur.ms_select += tm.stop();
		}
		c->pass.acc_mem.reset(); c->pass.acc.s = 0;        /* the accumulator is no longer needed */
		{
			EvTimer tm(c->st);
			const int tbits = std::max(1, ceil_log2_u64(c->t_end + 1)), n_dig = sst_n_digits(tbits);
			DevBuf<u32> dig_hist;                          /* every digit's histogram, counted by the first pass */
			if (n_dig > 1 && dig_hist.alloc((size_t)P * n_dig * SST_NBIN)) return -1;
			for (int shift = 0; shift < tbits; shift += 8) {
				yk_launch_seg_sort_pass(d_segoff, P, kc[cur], tt[cur], kc[cur ^ 1], tt[cur ^ 1], shift, dig_hist, n_dig, c->st);
				cur ^= 1;
			}
			c->st_cur.ms_sort += tm.stop();
		}
	} else {
		HIPCK(hipMemcpyAsync(d_segoff, seg_off.data(), (P + 1) * 8, hipMemcpyHostToDevice, c->st));
		if (kc[0].alloc(1) || tt[0].alloc(1)) return -1;
	}
	{
		EvTimer tm(c->st);
		if (yk_run_replay(c, m, kc[cur], tt[cur], c->d_lastput, 0, false)) return -1;
		c->st_cur.ms_replay += tm.stop();
	}
	*n_ins = (int64_t)(c->img_keys_total - before);
	c->st_cur.n_distinct_seen = (int64_t)c->pass.acc_count;
	c->st_cur.n_new_keys = *n_ins;
	return 0;
}
