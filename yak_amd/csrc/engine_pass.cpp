/* engine_pass.cpp -- a counting pass of the engine: yakamd_pass_begin and yakamd_pass_end, every yakamd_feed_* and yakamd_partition_* entry
 * point, the accumulator path of a create pass (consume_records: accumulator insert, bloom gate, last put-calls) and the count-existing paths
 * (key-owning ranges, slot ranges, LDS ranks, device atomics; yakamd_count_*, yakamd_count_retained).  The exclusive-ownership path of a create
 * pass, which keeps its batches and counts them as slices, is in engine_slice.cpp. */
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

extern "C" int yakamd_pass_begin(yak_ch_t *h, int create_new)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c) return fail("not an engine table");
	if (c->in_pass) return fail("pass already open");
	HIPCK(hipSetDevice(c->dev));
	(void)hipGetLastError();                                   /* whatever other users of the runtime left behind is not this pass's (see yakamd_pass_end) */
	c->create_new = create_new;
	c->delta_dirty = false;
	if (!create_new && delta_ensure(c)) return -1;
	if (create_new) { retained_drop(c); c->retain_broken = false; }
	c->n_slices = 0;
	c->bloom_mode = create_new && c->has_bloom && !c->gate_off;
	c->in_pass = true;
	c->t_end = 0;
	c->st_cur = {};
	HIPCK(hipMemsetAsync(c->d_counters, 0, YKC_N * 8, c->st));
	HIPCK(hipMemsetAsync(c->d_lastput, 0, c->P * 8, c->st));
	c->st_cur.ms_total = now_ms();
	/* exclusive-ownership LDS counting needs level-1 buckets == sub-tables and 2-bit k-mers */
	c->fast = create_new && env_i64("YAKAMD_FAST", 1) != 0 && c->nb_bits == c->pre && (!c->has_bloom || c->nb <= 42);
	c->pass.kept_bytes = 0; c->t_pass0_set = false; c->ms_part2 = c->ms_lds = 0; c->keys_at_begin = c->img_keys_total;
	if (c->fast) {
		size_t fr = 0, tot = 0;
		HIPCK(hipMemGetInfo(&fr, &tot));
		c->fast_budget = (u64)env_i64("YAKAMD_FAST_BUDGET", (int64_t)((fr + yk_pool_cached_bytes()) / 4));
	}
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

/* the level-1 partition's scratch: room for a launch of n_blk blocks */
static int part_reserve(yakamd_ctx *c, int n_blk)
{
	const size_t NB = (size_t)1 << c->nb_bits;
	if (!c->d_partial && (c->d_partial.alloc(NB * yk_part_groups()) || c->d_bstart.alloc(NB + 1))) return -1;
	return c->rows.reserve(NB * (size_t)n_blk);
}

/* the bloom gate's lists for a batch of n records: the three grow together, the old ones freed before the first new one is asked for */
static int new_reserve(yakamd_ctx *c, int64_t n)
{
	PassBufs &ps = c->pass;
	if (!c->bloom_mode || (size_t)n <= ps.newlist.cap()) return 0;
	ps.newlist.reset(); ps.miss.reset(); ps.cand.reset();
	return ps.newlist.reserve((size_t)n) || ps.miss.reserve((size_t)n * bloom_view(c).mw) || ps.cand.reserve((size_t)n) ? -1 : 0;
}

/* LDS bytes of the exclusive-ownership pass-2 counter for the current table image (0: not eligible) */
static size_t count_lds_bytes(yakamd_ctx *c)
{
	size_t lds = 0;
	if (c->nb_bits != c->pre || env_i64("YAKAMD_COUNT_LDS", 1) == 0) return 0;
	for (int p = c->plo; p < c->phi; ++p)
		if (c->h_bits[p] != YK_NOCAP) lds = std::max(lds, yk_img_count_lds_bytes(1u << c->h_bits[p], c->h_count[p]));
	return lds > 150 * 1024 ? 0 : lds;
}

/* count-existing pass, records = 8-byte hashes grouped by prefix (d_bstart), tables beyond the LDS
 * kernel: level-2 partition by home-slot range (k_hpart2) + one workgroup per range (k_img_count_rng).
 * Returns 0 done, -1 error, 1 not applicable (caller falls back to the device-atomics kernel). */
static int count_by_ranges(yakamd_ctx *c, const void *d_hash, int64_t n_rec, const u64 *d_bstart)
{
	const int P = c->P;
	u32 bmax = 0;
	for (int p = c->plo; p < c->phi; ++p) if (c->h_bits[p] != YK_NOCAP) bmax = std::max(bmax, c->h_bits[p]);
	const int rb = (int)bmax > yk_rng_log() ? (int)bmax - yk_rng_log() : 0;
	if (bmax == 0 || rb > 8) return 1;
	const size_t NB = (size_t)1 << c->nb_bits, S2 = (size_t)1 << rb, n_sb = (size_t)P << rb;
	std::vector<u64> bst(NB + 1);
	HIPCK(hipMemcpyAsync(bst.data(), d_bstart, (NB + 1) * 8, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	ChunkTable t;
	chunk_runs(t, d_hash, yk_rec_bytes(YK_FMT_HASH), bst.data(), P, (u64)yk_hpart2_chunk());
	std::vector<u64> bbase(P + 1, 0);
	for (int p = 0; p < P; ++p) bbase[p + 1] = bbase[p] + (bst[p + 1] - bst[p]);
	DevBuf<u64> d_bbase, d_sbstart, d_h2, d_list; DevBuf<u32> d_rows2, d_ln;
	const u32 list_cap = (u32)std::min<int64_t>(env_i64("YAKAMD_XLIST_CAP", 1 << 22), 1 << 22);   /* the knob is for tests */
	if (t.upload(c->st) || d_bbase.alloc(P + 1) || d_rows2.alloc((t.h.size() + 1) * S2) ||
	    d_sbstart.alloc(n_sb + 1) || d_h2.alloc((size_t)n_rec) || d_list.alloc((size_t)1 << 22) || d_ln.alloc(2)) return -1;
	HIPCK(hipMemcpyAsync(d_bbase, bbase.data(), (P + 1) * 8, hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemsetAsync(d_ln, 0, 8, c->st));
	const ImgView img = img_view(c);
	yk_launch_hpart2(t.d, (int)t.h.size(), t.d_first, d_bbase, img, rb, P, d_rows2, d_sbstart, d_h2, c->st);
	const u32 max_len = bmax > (u32)yk_rng_log() ? 1u << yk_rng_log() : 1u << bmax;
	int r = 0;
	if (yk_launch_img_count_rng(d_h2, 0, d_sbstart, img, c->plo, c->phi, rb, max_len, d_list, d_ln, list_cap, c->st)) r = fail("range count kernel could not be configured");
	u32 xn[2] = { 0, 0 };
	if (!r) {
		HIPCK(hipMemcpyAsync(xn, d_ln, 8, hipMemcpyDeviceToHost, c->st));
		HIPCK(hipStreamSynchronize(c->st));
		if (xn[1]) yk_event(YKE_RNG_SWEEPS);
		if (xn[1]) yk_launch_img_count_rng(d_h2, 1, d_sbstart, img, c->plo, c->phi, rb, max_len, d_list, d_ln, list_cap, c->st);   /* list too small: second sweep */
		else if (xn[0]) yk_launch_img_count_h(d_list, (int64_t)xn[0], img, c->st);
		if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] range count: 2^%d ranges per sub-table, %u boundary-crossing instances%s\n", rb, xn[0], xn[1] ? " (list overflow: second sweep)" : "");
		HIPCK(hipStreamSynchronize(c->st));
	}
	return r;
}

/* count-existing pass, records grouped by prefix: one workgroup per slot range with the range's keys in LDS
 * (k_img_count_own).  Returns 0 done, -1 error, 1 not applicable. */
/* the ranges of k_img_count_own for the table as it stands: 1 = not applicable, 0 = go (rb == -1: no sub-table has a slot) */
static int count_own_plan(yakamd_ctx *c, int *rng_log_out, int *rb_out, u32 *kmax_out)
{
	if (env_i64("YAKAMD_COUNT_OWN", 1) == 0 || c->nb_bits != c->pre) return 1;
	const size_t budget = (size_t)env_i64("YAKAMD_OWN_LDS", 156000);     /* one workgroup per CU with as few ranges as possible: every range re-reads the sub-table's records (measured: 8 ranges x 1 WG/CU 16.9 ms, 16 ranges x 2 WG/CU 24.8 ms) */
	u32 bmax = 0;
	for (int p = c->plo; p < c->phi; ++p) if (c->h_bits[p] != YK_NOCAP) bmax = std::max(bmax, c->h_bits[p]);
	*rng_log_out = 0; *rb_out = -1; *kmax_out = 0;
	if (bmax == 0) return 0;                                         /* no sub-table has a slot: nothing can be found */
	int rng_log = -1; u32 kmax = 0;
	for (int rl = (int)bmax; rl >= 5 && rng_log < 0; --rl) {
		u32 km = 1;
		for (int p = c->plo; p < c->phi; ++p) {
			if (c->h_bits[p] == YK_NOCAP) continue;
			const int rbp = (int)c->h_bits[p] > rl ? (int)c->h_bits[p] - rl : 0;
			const u32 e = (c->h_count[p] + (1u << rbp) - 1) >> rbp;
			km = std::max(km, rbp ? e + e / 8 + 192 : c->h_count[p]);   /* a range's share of the keys + 12 % + 6 sigma at small counts */
		}
		if (yk_count_own_lds(1u << rl, km) <= budget) { rng_log = rl; kmax = km; }
	}
	const int rb = rng_log < 0 ? 99 : (int)bmax - rng_log;
	if (rb > (int)env_i64("YAKAMD_OWN_MAXRB", 4)) return 1;        /* every range's workgroup streams the whole sub-table: too redundant beyond 16 ranges */
	*rng_log_out = rng_log; *rb_out = rb; *kmax_out = kmax;
	return 0;
}

/* records that only k_img_count_own reads: the range-tagged hashes the extraction made for it, the tagged level-1 records of the pass before */
static bool own_count_only(RecFmt fmt) { return fmt == YK_FMT_HASH_RNG || fmt == YK_FMT_TAGGED; }
static int count_own(yakamd_ctx *c, const void *d_rec, RecFmt fmt, const u64 *d_bstart)
{
	int rng_log, rb; u32 kmax;
	const int pl = count_own_plan(c, &rng_log, &rb, &kmax);
	if (pl) return own_count_only(fmt) ? fail("the table changed between the extraction and the count of a pass") : 1;
	if (rb < 0) return 0;
	DevBuf<u32> d_ln; DevBuf<u64> d_list;
	const u32 list_cap = (u32)std::min<int64_t>(env_i64("YAKAMD_XLIST_CAP", 1 << 22), 1 << 22);   /* the knob is for tests */
	if (d_list.alloc((size_t)1 << 22) || d_ln.alloc(2)) return -1;
	int r = 0;
	const ImgView img = img_view(c);
	const size_t lds = yk_count_own_lds(1u << rng_log, kmax);
	if (hipMemsetAsync(d_ln, 0, 8, c->st) != hipSuccess) r = fail("memset");
	if (!r && yk_launch_img_count_own(d_rec, fmt, 0, d_bstart, img, c->plo, c->phi, rb, rng_log, kmax, lds, d_list, d_ln, list_cap, c->st)) r = fail("key-owning count kernel could not be configured");
	u32 xn[2] = { 0, 0 };
	if (!r && (hipMemcpyAsync(xn, d_ln, 8, hipMemcpyDeviceToHost, c->st) != hipSuccess || hipStreamSynchronize(c->st) != hipSuccess)) r = fail("key-owning count kernel failed: %s", hipGetErrorString(hipGetLastError()));
	if (!r) {
		if (xn[1]) yk_event(YKE_OWN_SWEEPS);
		if (xn[1]) yk_launch_img_count_own(d_rec, fmt, 1, d_bstart, img, c->plo, c->phi, rb, rng_log, kmax, lds, d_list, d_ln, list_cap, c->st);   /* list too small: second sweep */
		else if (xn[0]) yk_launch_img_count_h(d_list, (int64_t)xn[0], img, c->st);
		if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] key-owning count: 2^%d slots per range (up to 2^%d ranges per sub-table), %u keys of LDS room, %zu B of LDS, %u boundary-crossing instances%s\n",
		                                          rng_log, rb, kmax, lds, xn[0], xn[1] ? " (list overflow: second sweep)" : "");
		if (hipStreamSynchronize(c->st) != hipSuccess) r = fail("count sweep failed");
	}
	return r;
}

int consume_records(yakamd_ctx *c, const void *d_rec, RecFmt fmt, int64_t n_rec, u64 t0, u64 batch_lo, u64 batch_hi, const u64 *d_bstart)
{
	if (n_rec <= 0) return 0;
	ImgView img = img_view(c);
	c->st_cur.n_instances += n_rec;
	if (batch_hi > c->t_end) c->t_end = batch_hi;
	if (!c->create_new) {
		c->delta_dirty = true;
		yk_image_touched(c);
		EvTimer tm(c->st);
		/* records grouped by sub-table and every sub-table small enough for LDS rank counters:
		 * exclusive-ownership counting, no global atomics */
		if (d_bstart) {
			const int r = count_own(c, d_rec, fmt, d_bstart);
			if (r <= 0 || own_count_only(fmt)) {
				insert_ms(c, tm);
				return r;
			}
		}
		const size_t lds = d_bstart ? count_lds_bytes(c) : 0;
		if (!lds && d_bstart && fmt == YK_FMT_HASH && c->nb_bits == c->pre && env_i64("YAKAMD_COUNT_RNG", 1) != 0) {
			/* sub-tables too large for one workgroup's LDS: split each one's hashes by home-slot range first */
			const int r = count_by_ranges(c, d_rec, n_rec, d_bstart);
			if (r <= 0) {                                        /* done (0) or failed (-1); 1 = not applicable */
				insert_ms(c, tm);
				return r;
			}
		}
		DevBuf<u64> d_ck; u32 ck_stride = 1;
		if (lds) {
			for (int p = c->plo; p < c->phi; ++p) ck_stride = std::max(ck_stride, c->h_count[p]);
			if (d_ck.alloc((size_t)(c->phi - c->plo) * ck_stride)) return -1;
		}
		const bool lds_done = lds && yk_launch_img_count_lds(d_rec, fmt, d_bstart, img, c->plo, c->phi, lds, d_ck, ck_stride, c->st) == 0;
		if (d_ck) { HIPCK(hipStreamSynchronize(c->st)); d_ck.reset(); }
		if (!lds_done) {
			if (fmt == YK_FMT_HASH) yk_launch_img_count_h((const u64*)d_rec, n_rec, img, c->st);
			else yk_launch_img_count((const Rec*)d_rec, n_rec, img, c->st);
		}
		insert_ms(c, tm);
		return 0;
	}
	const Rec *rec = (const Rec*)d_rec;                        /* a create pass: {hash, position} records */
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

/* a base image on the device (ASCII, or packed with d_valid) into the open pass, a batch at a time */
static int feed_image(yak_ch_t *h, const void *d_bases, const u32 *d_valid, int64_t n_bytes, uint64_t t0)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	if (c->k >= 64 || c->k < 1) return fail("k must be in [1, 63]");
	if (((uintptr_t)d_bases & 15) != 0) return fail("device base image must be 16-byte aligned");
	HIPCK(hipSetDevice(c->dev));
	if (c->hpc && n_bytes > 0) {
		/* a table in homopolymer-compressed space: the image is compacted, ASCII or packed, into the pass's buffer and the feed goes
		 * on with that.  t0 stays the feed's position in the uncompressed stream: a compressed position is no larger than the original one, so the
		 * feeds keep their order, and only the order of stream positions matters */
		DevVec<uint8_t> &hpc = c->pass.hpc;
		if ((size_t)n_bytes > hpc.cap() && hpc.reserve((size_t)(((n_bytes + (n_bytes >> 3) + 4096) + 15) & ~(int64_t)15))) return -1;
		const int64_t n_out = yk_hpc_compact(d_bases, d_valid, n_bytes, hpc, 0, 0, 0, 0, 0, c->st);
		if (n_out < 0) return -1;
		d_bases = hpc.get(); d_valid = 0; n_bytes = n_out;
	}
	int64_t batch = env_i64("YAKAMD_BATCH", (int64_t)1 << 31);
	batch = std::min<int64_t>((int64_t)1 << 31, std::max<int64_t>(4096, batch & ~(int64_t)4095));   /* run starts are 31-bit (tagged records: bit 31 is the toggle) */
	RecFmt consumed = c->create_new ? YK_FMT_POS : YK_FMT_HASH;   /* of a batch that is consumed at once: counting existing keys needs no stream positions */
	if (!c->create_new && c->k < 32 && c->nb_bits <= 10 && env_i64("YAKAMD_YTAG", 1) != 0) {   /* the key-owning count will run: its range test is prepared by the extraction */
		int rl, rb; u32 km;
		if (count_own_plan(c, &rl, &rb, &km) == 0 && rb >= 0) consumed = YK_FMT_HASH_RNG;
	}
	/* a kept batch: tagged 8-byte records (half the partition traffic) when the hash leaves room for the tag, (hash >> pre) < 2^52 */
	const RecFmt kept = yk_tagged_fits(c->k, c->pre) && c->nb_bits == c->pre && !c->or_mode ? YK_FMT_TAGGED : YK_FMT_POS;
	const int64_t bmax = std::min(batch, (n_bytes + 4095) & ~(int64_t)4095);
	if ((!c->fast && c->pass.rec.reserve((size_t)bmax)) || part_reserve(c, yk_xpart_blocks(bmax))) return -1;   /* the fast path keeps every batch in a buffer of its own */
	for (int64_t pos = 0; pos < n_bytes; pos += batch) {
		const int64_t end = std::min(n_bytes, pos + batch);
		u64 n_rec = 0;
		void *out = c->pass.rec.get();
		if (c->fast) {                                   /* the batch stays resident until pass_end */
			if (fast_admit(c, kept, t0 + (u64)pos, (u64)(end - pos), (u64)(end - pos), &out)) return -1;
			if (!c->fast) { if (c->pass.rec.reserve((size_t)bmax)) return -1; out = c->pass.rec.get(); }   /* the pass has just left the fast path */
		}
		const RecFmt fmt = c->fast ? kept : consumed;
		{
			EvTimer tm(c->st);
			yk_launch_xpart((const uint8_t*)d_bases, pos, end, pos, c->k, c->pre, c->plo, c->phi, c->nb_bits,
			                c->rows, c->d_partial, c->d_bstart, out, fmt, c->st, d_valid);
			HIPCK(hipMemcpyAsync(&n_rec, c->d_bstart + ((size_t)1 << c->nb_bits), 8, hipMemcpyDeviceToHost, c->st));
			c->st_cur.ms_extract += tm.stop();
		}
		if (c->fast) { if (fast_keep(c, n_rec)) return -1; if (t0 + (u64)end > c->t_end) c->t_end = t0 + (u64)end; continue; }
		if (consume_records(c, out, fmt, (int64_t)n_rec, t0 + (u64)pos, t0 + (u64)pos, t0 + (u64)end, c->d_bstart)) return -1;
	}
	return 0;
}

extern "C" int yakamd_feed_bases_dev(yak_ch_t *h, const void *d_bases, int64_t n_bytes, uint64_t t0) { return feed_image(h, d_bases, 0, n_bytes, t0); }
/* the same stream at 0.375 bytes per base: 2-bit codes, 16 bases per 32-bit word (base j at bits 2 (j % 16)), and a validity bit
 * per base (bit j % 32 of word j / 32; 0 = N, any other non-ACGT byte or a record separator).  Position j of the stream is base j */
extern "C" int yakamd_feed_packed_dev(yak_ch_t *h, const void *d_codes, const void *d_valid, int64_t n_bases, uint64_t t0)
{
	if (!d_valid) return fail("packed feed without a validity mask");
	if (((uintptr_t)d_valid & 3) != 0) return fail("validity mask must be 4-byte aligned");
	return feed_image(h, d_codes, (const u32*)d_valid, n_bases, t0);
}
extern "C" int yakamd_pack_bases_dev(const void *d_ascii, int64_t n, void *d_codes, void *d_valid, void *stream)
{
	yk_launch_pack((const uint8_t*)d_ascii, n, (u32*)d_codes, (u32*)d_valid, (hipStream_t)stream);
	return hipGetLastError() == hipSuccess ? 0 : fail("pack kernel launch failed");
}

/* the staging buffer of the host feeds: room for n bytes */
static int stage_reserve(yakamd_ctx *c, int64_t n)
{
	return (size_t)n <= c->stage.cap() ? 0 : c->stage.reserve((size_t)(n + (n >> 3) + 4096));
}

extern "C" int yakamd_feed_bases_host(yak_ch_t *h, const void *h_bases, int64_t n_bytes, uint64_t t0)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	HIPCK(hipSetDevice(c->dev));
	if (stage_reserve(c, n_bytes)) return -1;
	HIPCK(hipMemcpyAsync(c->stage, h_bases, (size_t)n_bytes, hipMemcpyHostToDevice, c->st));
	return yakamd_feed_bases_dev(h, c->stage, n_bytes, t0);
}

/* the packed image made on the host (yakamd_pack_bases_host: the code words, then -- 16-byte aligned -- the validity words): one copy of
 * 0.375 bytes per base over the bus, then the packed feed */
extern "C" int64_t yakamd_packed_bytes(int64_t n_bases) { const int64_t nw = (n_bases + 31) / 32; return ((nw * 8 + 15) & ~(int64_t)15) + nw * 4; }
extern "C" int yakamd_feed_packed_host(yak_ch_t *h, const void *h_packed, int64_t n_bases, uint64_t t0)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	if (n_bases <= 0) return 0;
	HIPCK(hipSetDevice(c->dev));
	const int64_t need = yakamd_packed_bytes(n_bases), valid_at = need - (n_bases + 31) / 32 * 4;
	if (stage_reserve(c, need)) return -1;
	HIPCK(hipMemcpyAsync(c->stage, h_packed, (size_t)need, hipMemcpyHostToDevice, c->st));
	return yakamd_feed_packed_dev(h, c->stage, c->stage + valid_at, n_bases, t0);
}

/* packed pieces of the stream, each a whole number of 32-position words (its code words and its validity words apart), laid one behind the
 * other on the device -- two copies per piece -- and fed as one image: what yak_count() does with the segments its parser threads packed */
extern "C" int yakamd_feed_packed_pieces_host(yak_ch_t *h, int n_pieces, const void *const *codes, const void *const *valid, const int64_t *n_words, uint64_t t0)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	int64_t nw = 0;
	for (int i = 0; i < n_pieces; ++i) { if (n_words[i] < 0) return fail("packed piece of negative length"); nw += n_words[i]; }
	if (nw == 0) return 0;
	HIPCK(hipSetDevice(c->dev));
	const int64_t n_bases = nw * 32, need = yakamd_packed_bytes(n_bases), valid_at = need - nw * 4;
	if (stage_reserve(c, need)) return -1;
	int64_t w = 0;
	for (int i = 0; i < n_pieces; ++i) {
		if (n_words[i] == 0) continue;
		HIPCK(hipMemcpyAsync(c->stage + w * 8, codes[i], (size_t)n_words[i] * 8, hipMemcpyHostToDevice, c->st));
		HIPCK(hipMemcpyAsync(c->stage + valid_at + w * 4, valid[i], (size_t)n_words[i] * 4, hipMemcpyHostToDevice, c->st));
		w += n_words[i];
	}
	return yakamd_feed_packed_dev(h, c->stage, c->stage + valid_at, n_bases, t0);
}

extern "C" int yakamd_feed_hashed_dev(yak_ch_t *h, const void *d_hash, const void *d_t, int64_t n, uint64_t t0, uint64_t t_span)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	HIPCK(hipSetDevice(c->dev));
	/* group the records by sub-table prefix first (same locality as the extraction path) */
	if (n <= 0) return 0;
	if (c->pass.rec.reserve((size_t)n) || part_reserve(c, yk_rpart_blocks(n))) return -1;
	u64 n_rec = 0;
	void *out = c->pass.rec.get();
	if (c->fast && fast_admit(c, YK_FMT_POS, t0, t_span, (u64)n, &out)) return -1;
	yk_launch_rpart((const u64*)d_hash, (const u32*)d_t, n, c->pre, c->plo, c->phi, c->nb_bits,
	                c->rows, c->d_partial, c->d_bstart, (Rec*)out, c->st);
	HIPCK(hipMemcpyAsync(&n_rec, c->d_bstart + ((size_t)1 << c->nb_bits), 8, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	if (c->fast) { if (t0 + t_span > c->t_end) c->t_end = t0 + t_span; return fast_keep(c, n_rec); }
	return consume_records(c, out, YK_FMT_POS, (int64_t)n_rec, t0, t0, t0 + t_span, c->d_bstart);
}

static int64_t partition_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_out, RecFmt fmt, uint64_t *h_bstart)
{
	if (k < 1 || k > 63 || pre < 3 || pre > 13) { fail("partition: unsupported k / pre"); return -1; }
	if (((uintptr_t)d_bases & 15) != 0 || n_bytes >= ((int64_t)1 << 32)) { fail("partition: base image must be 16-byte aligned and < 4 GiB"); return -1; }
	const size_t NB = (size_t)1 << pre;
	if (n_bytes <= 0) { memset(h_bstart, 0, (NB + 1) * 8); return 0; }   /* no chunk: nothing is launched (yk_launch_xpart would leave d_bstart as the pool handed it out) */
	const int n_blk = yk_xpart_blocks(n_bytes);
	DevBuf<u64> d_bstart, d_partial; DevBuf<u32> d_rows;
	if (d_rows.alloc(NB * (size_t)n_blk) || d_partial.alloc(NB * yk_part_groups()) || d_bstart.alloc(NB + 1)) return -1;
	/* on a stream of its own, not the null stream (which waits for, and holds up, every other stream of the device): a multi-GPU job partitions the
	 * chunks of its next round while the owners' streams take in the round before */
	int dev = 0;
	(void)hipGetDevice(&dev);
	hipStream_t ps = yk_stream_get(dev);
	yk_launch_xpart((const uint8_t*)d_bases, 0, n_bytes, 0, k, pre, 0, 1 << pre, pre, d_rows, d_partial, d_bstart, d_out, fmt, ps);
	hipError_t e = hipMemcpyAsync(h_bstart, d_bstart, (NB + 1) * 8, hipMemcpyDeviceToHost, ps);
	if (e == hipSuccess) e = hipStreamSynchronize(ps);
	yk_stream_put(dev, ps);
	if (e != hipSuccess) { fail("partition: %s", hipGetErrorString(e)); return -1; }
	return (int64_t)h_bstart[NB];
}

extern "C" int64_t yakamd_partition_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_rec_out, uint64_t *h_bstart)
{
	return partition_dev(k, pre, d_bases, n_bytes, d_rec_out, YK_FMT_POS, h_bstart);
}

/* the same partition as 8-byte tagged records (yk_device.h YK_R8_*: half the exchange payload of a sharded pass); for
 * yakamd_feed_partitioned_tagged_dev on the owner.  yakamd_tagged_ok says whether k / pre allow the format */
extern "C" int yakamd_tagged_ok(int k, int pre) { return k >= 1 && pre >= 3 && yk_tagged_fits(k, pre); }   /* (k and pre as partition_dev takes them) */
extern "C" int64_t yakamd_partition_tagged_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_rec8_out, uint64_t *h_bstart)
{
	if (!yakamd_tagged_ok(k, pre)) { fail("partition: tagged records need k < 32, 2k - pre <= 52, pre <= 10"); return -1; }
	if (n_bytes > ((int64_t)1 << 31)) { fail("partition: at most 2^31 stream positions per call with tagged records (31-bit run starts)"); return -1; }
	return partition_dev(k, pre, d_bases, n_bytes, d_rec8_out, YK_FMT_TAGGED, h_bstart);
}

extern "C" int64_t yakamd_partition_hashes_dev(int k, int pre, const void *d_bases, int64_t n_bytes, void *d_hash_out, uint64_t *h_bstart)
{
	return partition_dev(k, pre, d_bases, n_bytes, d_hash_out, YK_FMT_HASH, h_bstart);
}

static int feed_partitioned(yak_ch_t *h, const void *d_rec, RecFmt fmt, int64_t n, const uint64_t *h_bstart, uint64_t t0, uint64_t t_span, bool borrow)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("feed outside a pass");
	if (c->nb_bits != c->pre) return fail("feed_partitioned needs pre <= 13");
	HIPCK(hipSetDevice(c->dev));
	if (n <= 0) return 0;
	const size_t NB = (size_t)1 << c->nb_bits;
	if (c->fast) {
		void *out = 0;
		if (fmt == YK_FMT_TAGGED && !(yakamd_tagged_ok(c->k, c->pre) && !c->or_mode)) return fail("tagged records do not fit this table (k, pre)");
		if (fast_admit(c, fmt, t0, t_span, (u64)n, &out, borrow ? d_rec : 0)) return -1;
		if (c->fast) {                                       /* admitted: already grouped by prefix; keep a private copy unless lent */
			if (!borrow) HIPCK(hipMemcpyAsync(out, d_rec, (size_t)n * yk_rec_bytes(fmt), hipMemcpyDeviceToDevice, c->st));
			Kept &k = c->pass.kept.back();
			k.bstart.assign(h_bstart, h_bstart + NB + 1);
			k.n = (u64)n;
			c->st_cur.n_instances += n;
			if (t0 + t_span > c->t_end) c->t_end = t0 + t_span;
			return 0;
		}
	}
	if (fmt == YK_FMT_TAGGED) return fail("tagged records need the exclusive-ownership path (the pass left it: input beyond the device budget, or YAKAMD_FAST=0)");
	return consume_records(c, d_rec, fmt, n, t0, t0, t0 + t_span);   /* general path / pass 2: consume in place */
}

extern "C" int yakamd_feed_partitioned_dev(yak_ch_t *h, const void *d_rec, int64_t n, const uint64_t *h_bstart, uint64_t t0, uint64_t t_span)
{
	return feed_partitioned(h, d_rec, YK_FMT_POS, n, h_bstart, t0, t_span, false);
}

extern "C" int yakamd_feed_partitioned_lent_dev(yak_ch_t *h, const void *d_rec, int64_t n, const uint64_t *h_bstart, uint64_t t0, uint64_t t_span)
{
	return feed_partitioned(h, d_rec, YK_FMT_POS, n, h_bstart, t0, t_span, true);
}

/* 1 while the open pass of h runs on the exclusive-ownership path (the only one that takes tagged records) */
extern "C" int yakamd_pass_fast(yak_ch_t *h) { yakamd_ctx *c = ctx_of(h); return c && c->in_pass && c->fast && !c->or_mode; }

extern "C" int yakamd_feed_partitioned_tagged_dev(yak_ch_t *h, const void *d_rec8, int64_t n, const uint64_t *h_bstart, uint64_t t0, uint64_t t_span, int lent)
{
	return feed_partitioned(h, d_rec8, YK_FMT_TAGGED, n, h_bstart, t0, t_span, lent != 0);
}

extern "C" int yakamd_count_partitioned_dev(yak_ch_t *h, const void *d_hash_u64, int64_t n, const uint64_t *h_bstart)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass || c->create_new) return fail("count_partitioned needs an open create_new = 0 pass");
	if (c->nb_bits != c->pre) return fail("count_partitioned needs pre <= 13");
	HIPCK(hipSetDevice(c->dev));
	if (n <= 0) return 0;
	const size_t NB = (size_t)1 << c->nb_bits;
	if (part_reserve(c, 1)) return -1;
	HIPCK(hipMemcpyAsync(c->d_bstart, h_bstart, (NB + 1) * 8, hipMemcpyHostToDevice, c->st));
	const int r = consume_records(c, d_hash_u64, YK_FMT_HASH, n, 0, 0, 0, c->d_bstart);
	HIPCK(hipStreamSynchronize(c->st));                       /* h_bstart may be a temporary of the caller */
	return r;
}

extern "C" int yakamd_count_hashes_dev(yak_ch_t *h, const void *d_hash_u64, int64_t n)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass || c->create_new) return fail("count_hashes needs an open create_new = 0 pass");
	HIPCK(hipSetDevice(c->dev));
	if (n <= 0) return 0;
	c->delta_dirty = true;
	yk_image_touched(c);
	EvTimer tm(c->st);
	yk_launch_img_count_h((const u64*)d_hash_u64, n, img_view(c), c->st);
	insert_ms(c, tm);
	c->st_cur.n_instances += n;
	return 0;
}

/* ---- the count pass over the input of the pass before (reference main.c:53-57: both passes read the same file) ---- */
extern "C" int yakamd_retain_input(yak_ch_t *h, int on)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c) return fail("not an engine table");
	if (c->in_pass) return fail("yakamd_retain_input inside a pass");
	HIPCK(hipSetDevice(c->dev));
	c->retain_on = on != 0;
	if (!on) retained_drop(c);
	return 0;
}

extern "C" int64_t yakamd_retained_instances(yak_ch_t *h)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || c->retain_broken) return 0;
	u64 n = c->ret.l2.valid ? c->ret.l2.n_total : 0;
	for (auto &r : c->ret.l1) n += r.n;
	return (int64_t)n;
}

/* inside an open create_new = 0 pass: count every instance of the retained records (k_img_count_own reads the tagged level-1 records
 * as they are).  0 = counted, the records are released; 1 = nothing usable was retained (the caller feeds the input again); -1 = error */
extern "C" int yakamd_count_retained(yak_ch_t *h)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass || c->create_new) return fail("yakamd_count_retained needs an open create_new = 0 pass");
	HIPCK(hipSetDevice(c->dev));
	const Ret2 &l2 = c->ret.l2;
	if (l2.valid && !c->retain_broken && l2.kc2) {
		/* k_lc2 counted every instance of every key it selected while it owned the sub-bucket: all that is left is to add those counts.
		 * Behind a yak_ch_clear that has not run yet, on a key list that is the whole image as the pass before left it (Ret2.whole_image), "clear, then
		 * add c2" needs no probe per key: that pass counted every instance but the first, which the filter took, so c2 == min(c1 + 1, 1023) for every
		 * key but the few the filter let through at once (k_lc2: fpk).  One sweep raises every count by one (k_img_clear's bump) and takes the pending
		 * clear's place; k_cnt2_apply reads its lists and probes only the keys whose c2 is something else.  YAKAMD_PASS2_BUMP=0 (a test switch):
		 * clear, then add */
		const bool bump = c->clear_pending && l2.whole_image && env_i64("YAKAMD_PASS2_BUMP", 1) != 0;
		const ImgView img = bump ? img_view_pending(c) : img_view(c);
		EvTimer tm(c->st);
		if (bump) {
			c->clear_pending = false;
			yk_launch_img_clear(img, c->n_slots, c->st, 1);
		}
		yk_launch_cnt2_apply(l2.fp, l2.kkc, l2.kc2, l2.segbase, img, c->st, bump);
		const double ms = insert_ms(c, tm);
		const bool bad = hipGetLastError() != hipSuccess;
		c->st_cur.n_instances += (int64_t)l2.n_total;
		c->st_cur.pass2_path = 1; yk_event(YKE_PASS2_FUSED);
		if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] count pass: the counts of the pass before applied (%llu keys, %.2f ms%s)\n", (unsigned long long)l2.n_keys, ms, bump ? "; with the pending clear, in one sweep" : "");
		retained_drop(c);
		return bad ? fail("applying the counts of the pass before failed") : 0;
	}
	if (l2.valid && !c->retain_broken) {
		DevBuf<u32> d_kcnt;
		if (d_kcnt.alloc(l2.n_keys)) return -1;
		HIPCK(hipMemsetAsync(c->d_nmissing, 0, 4, c->st));          /* (a spare word of the context: "some instance went through the pending counts") */
		EvTimer tm(c->st);
		yk_launch_cnt2(l2.fp, l2.sbstart, l2.r2, l2.koff, l2.kkc, l2.segbase, d_kcnt, img_view(c), l2.n_keys, c->d_nmissing, c->st);
		u32 used = 1;
		(void)hipMemcpyAsync(&used, c->d_nmissing, 4, hipMemcpyDeviceToHost, c->st);
		const double ms = insert_ms(c, tm);
		if (used) c->delta_dirty = true;
		d_kcnt.reset();
		const bool bad = hipGetLastError() != hipSuccess;
		c->st_cur.n_instances += (int64_t)l2.n_total;
		c->st_cur.pass2_path = 2; yk_event(YKE_PASS2_RECOUNT);
		if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] count pass: k_cnt2 over the retained sub-bucket records (%llu keys, %.2f ms)\n", (unsigned long long)l2.n_keys, ms);
		retained_drop(c);
		return bad ? fail("the count over the retained sub-bucket records failed") : 0;
	}
	if (c->ret.l1.empty() || c->retain_broken) { yk_event(YKE_PASS2_NONE); retained_drop(c); return 1; }
	{
		int rl, rb; u32 km;
		if (count_own_plan(c, &rl, &rb, &km) != 0) { yk_event(YKE_PASS2_NONE); retained_drop(c); return 1; }   /* tables beyond the key-owning count kernel: the general count path wants plain hashes */
	}
	const size_t NB = (size_t)1 << c->nb_bits;
	if (part_reserve(c, 1)) return -1;
	int r = 0;
	for (auto &b : c->ret.l1) {
		if (r) break;
		if (hipMemcpyAsync(c->d_bstart, b.bstart.data(), (NB + 1) * 8, hipMemcpyHostToDevice, c->st) != hipSuccess) { r = fail("memcpy"); break; }
		r = consume_records(c, b.rec.get(), YK_FMT_TAGGED, (int64_t)b.n, 0, 0, 0, c->d_bstart);
		if (!r && hipStreamSynchronize(c->st) != hipSuccess) r = fail("count of the retained records failed");
	}
	retained_drop(c);
	if (!r) { c->st_cur.pass2_path = 3; yk_event(YKE_PASS2_PREFIX); }
	return r ? -1 : 0;
}

/* ---- the hashes of a base image (the device-level exports of the lookup commands are in lookup_dev.cpp) ---- */
extern "C" int64_t yakamd_extract_dev(int k, const void *d_bases, int64_t n_bytes, void *d_hash, void *d_t,
                                      int pre, int plo, int phi, void *stream)
{
	if (k >= 64 || k < 1) { fail("extract: unsupported k"); return -1; }
	u64 *d_cur = 0, n = 0;
	hipStream_t st = (hipStream_t)stream;
	if (hipMalloc((void**)&d_cur, 8) != hipSuccess) { fail("hipMalloc"); return -1; }
	hipMemsetAsync(d_cur, 0, 8, st);
	yk_launch_extract((const uint8_t*)d_bases, 0, n_bytes, 0, k, pre, plo, phi, (u64*)d_hash, (u32*)d_t, d_cur, st);
	hipMemcpyAsync(&n, d_cur, 8, hipMemcpyDeviceToHost, st);
	hipStreamSynchronize(st);
	hipFree(d_cur);
	return (int64_t)n;
}

/* the end of a pass: pending counts folded in, or the new keys of a create pass laid out */
static int64_t pass_end_body(yakamd_ctx *c)
{
	HIPCK(hipSetDevice(c->dev));
	const int P = c->P;
	int64_t n_ins = 0;
	if (c->k >= 32 && yk_bad_hash_seen(c->st)) { pass_free(c); return fail("a 64-bit k-mer hash equals the empty-slot pattern: unsupported input for k >= 32"); }
	if (!c->create_new) {
		if (c->d_delta && c->delta_dirty) yk_launch_img_fold(img_view(c), c->n_slots, c->st);   /* (k_cnt2_apply writes its counts straight into the keys) */
		HIPCK(hipStreamSynchronize(c->st));
		c->d_delta.reset();
		c->host_valid = false;
		retained_drop(c);                                        /* used or not: the next pass is another input's */
	} else if (c->or_mode && !(c->fast && !c->pass.acc.s)) {
		pass_free(c);
		return fail("flag-mode loads need the exclusive-ownership path (prefix length <= 13, input within the device budget)");
	} else if (c->fast && !c->pass.acc.s) {
		if (fast_finish(c, true)) return -1;
		n_ins = (int64_t)(c->img_keys_total - c->keys_at_begin);   /* earlier slices of the pass included */
		c->st_cur.n_new_keys = n_ins;
	} else {
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
		n_ins = (int64_t)(c->img_keys_total - before);
		c->st_cur.n_distinct_seen = (int64_t)c->pass.acc_count;
		c->st_cur.n_new_keys = n_ins;
	}
	pass_free(c);
	c->st_cur.ms_total = now_ms() - c->st_cur.ms_total;
	c->st_last = c->st_cur;
	return n_ins;
}

extern "C" int64_t yakamd_pass_end(yak_ch_t *h)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass) return fail("no pass open");
	int64_t r = pass_end_body(c);
	if (r >= 0) {                                              /* a launch that was refused (bad configuration) reports nothing by itself */
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) r = fail("a HIP call of this pass was refused: %s", hipGetErrorString(e));
	}
	if (r < 0) pass_free(c);                                 /* a failed pass is closed too: the table stays usable (the pass's k-mers are lost, the error is reported) */
	return r;
}
