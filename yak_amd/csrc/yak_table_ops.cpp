/*
 * yak_table_ops.cpp -- the operations of include/yak.h on two tables: yak_ch_subtract / yak_ch_isec (keep_by_membership), yak_ch_merge and
 * yakamd_ch_sum (put_listed).  Either operand may be sharded over prefix ranges (yak_count() shards by itself: several GPUs, or an
 * unfiltered count of a large plain file taken in sweeps); every sub-table belongs to exactly one shard of each operand, and the
 * reference's operations are per sub-table (kt_for over 1 << pre, htab.c:246-347), so they are carried out shard by shard.
 */
#include "yak_host.h"
#include "yak_file.h"

/* an unsharded copy of `h` on device `dev`, by way of its .yak image (same keys and counts; the slot layout is the restored one, which
 * membership tests do not look at).  Only for the second operand of subtract / isec when it is sharded or lives on another device */
static yak_ch_t *unsharded_copy(const yak_ch_t *h, int dev)
{
	uint8_t *img = 0;
	const int64_t sz = yakamd_dump_mem((yak_ch_t*)h, &img);
	if (sz < 0) return 0;
	YakSrc src = YakSrc::memory(img, (size_t)sz);
	YakHeader hd;
	std::vector<uint32_t> caps, sizes;
	std::vector<uint64_t> keys;
	const bool ok = yak_read_header(src, &hd) == YAK_OK && (int)hd.pre == h->pre && yak_read_all(src, h->pre, caps, sizes, keys) == YAK_OK;
	free(img);
	if (!ok) return 0;
	yk_ctx_next_device(dev);
	yak_ch_t *c = yak_ch_init(h->k, h->pre, 0, 0);
	if (c && yk_ctx_load(shard_ctx(c), caps.data(), sizes.data(), keys.data()) != 0) { yak_ch_destroy(c); c = 0; }
	return c;
}

/* reference htab.c:287-316 / 318-347: keep the k-mers of h0 that are absent from (which = 1) / present in (2) h1 */
static void keep_by_membership(yak_ch_t *h0, const yak_ch_t *h1, int which, const char *fn_name)
{
	if (h0->k != h1->k || h0->pre != h1->pre) { fprintf(stderr, "[E::%s] tables of different k / prefix length\n", fn_name); return; }
	std::map<int, yak_ch_t*> copy_on;                             /* device -> unsharded copy of h1 made for it */
	bool ok = true;
	for (yak_ch_t *s0 : shards_of(h0)) {
		yakamd_ctx *c0 = shard_ctx(s0);
		const int dev = yk_ctx_device(c0);
		const yak_ch_t *other = h1;
		if (YK_MULTI((const yak_ch_ext*)h1) || yk_ctx_device(shard_ctx((yak_ch_t*)h1)) != dev) {
			if (!copy_on.count(dev)) copy_on[dev] = unsharded_copy(h1, dev);
			other = copy_on[dev];
			if (!other) { ok = false; break; }
		}
		unsigned long long tot = 0;
		if ((which == 1 ? yk_ctx_subtract(c0, shard_ctx((yak_ch_t*)other), &tot) : yk_ctx_isec(c0, shard_ctx((yak_ch_t*)other), &tot)) != 0) { ok = false; break; }
		s0->tot = tot;
	}
	for (auto &kv : copy_on) if (kv.second) yak_ch_destroy(kv.second);
	set_tot(h0);
	if (!ok) fprintf(stderr, "[E::%s] %s\n", fn_name, *yakamd_last_error() ? yakamd_last_error() : "the second table could not be brought to the device of the first");
}

/* What yak_ch_merge and yakamd_ch_sum share.  One counting pass per shard of h0 puts every k-mer of h1 with min <= count <= hi into it, sub-table
 * by sub-table in h1's slot order: the list positions are the stream times; a shard of h0 takes the lists of the shards of h1 that overlap its
 * range one after the other (the feed keeps the k-mers of its own prefix range).  sum: the lists carry the counts, are kept until the pass has
 * ended and then add them (yk_ctx_add_counts).  h1 is only read.  false after a message in yakamd_last_error() */
static bool put_listed(yak_ch_t *h0, const yak_ch_t *h1, int min, int hi, int pre_resize, bool sum)
{
	bool ok = true;
	for (yak_ch_t *s0 : shards_of(h0)) {
		if (!ok) break;
		yakamd_ctx *c0 = shard_ctx(s0);
		int lo0, hi0;
		yk_ctx_range(c0, &lo0, &hi0);
		std::vector<yak_ch_t*> from;
		for (yak_ch_t *s1 : shards_of(h1)) { int lo1, hi1; yk_ctx_range(shard_ctx(s1), &lo1, &hi1); if (std::max(lo0, lo1) < std::min(hi0, hi1)) from.push_back(s1); }
		if (pre_resize) for (yak_ch_t *s1 : from) ok = ok && yk_ctx_merge_presize(c0, shard_ctx(s1)) == 0;
		if (!ok) break;
		/* sum: a list and its counts as c0's device reaches them, owned until the pass has ended and they were added (staged: a copy made with
		 * yakamd_dev_alloc on c0's device; else the listing's own pool buffers) */
		struct Held {
			u64 *hash; unsigned short *cnt; u64 n; bool staged;
			Held(u64 *h, unsigned short *c, u64 n_, bool st) : hash(h), cnt(c), n(n_), staged(st) {}
			Held(Held &&o) : hash(o.hash), cnt(o.cnt), n(o.n), staged(o.staged) { o.hash = 0; o.cnt = 0; }
			Held(const Held&) = delete;
			Held &operator=(const Held&) = delete;
			~Held() { if (staged) { yakamd_dev_free(hash); yakamd_dev_free(cnt); } else { yk_pool_release(hash); yk_pool_release(cnt); } }
		};
		std::vector<Held> held;
		yk_ctx_gate(c0, false);
		ok = yakamd_pass_begin(s0, 1) == 0;
		uint64_t t0 = 0;
		for (yak_ch_t *s1 : from) {
			u64 *d_hash = 0, n = 0; u32 *d_t = 0; unsigned short *d_cnt = 0;
			ok = ok && hipSetDevice(yk_ctx_device(shard_ctx(s1))) == hipSuccess && yk_ctx_list_hashes(shard_ctx(s1), min, hi, &d_hash, &d_t, &n, sum ? &d_cnt : 0) == 0;
			const int dv0 = yk_ctx_device(c0), dv1 = yk_ctx_device(shard_ctx(s1));
			if (ok && n && dv0 != dv1) {
				/* the list lies on s1's device and the feed's kernels run on c0's: peer access (enabled here: nothing else in this process may have
				 * done it), or a staged copy on c0's device when the two cannot reach each other */
				int can = 0;
				ok = hipSetDevice(dv0) == hipSuccess;
				if (ok && hipDeviceCanAccessPeer(&can, dv0, dv1) == hipSuccess && can) {
					const hipError_t pe = hipDeviceEnablePeerAccess(dv1, 0);
					if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) can = 0;
					(void)hipGetLastError();
				}
				if (ok && !can) {
					u64 *h2 = (u64*)yakamd_dev_alloc(n * 8); u32 *t2 = (u32*)yakamd_dev_alloc(n * 4);
					Held copy(h2, sum && h2 && t2 ? (unsigned short*)yakamd_dev_alloc(n * 2) : 0, n, true);   /* frees h2 (and the counts) when it goes */
					ok = h2 && t2 && hipMemcpyPeer(h2, dv0, d_hash, dv1, n * 8) == hipSuccess && hipMemcpyPeer(t2, dv0, d_t, dv1, n * 4) == hipSuccess;
					if (ok && sum) ok = copy.cnt && hipMemcpyPeer(copy.cnt, dv0, d_cnt, dv1, n * 2) == hipSuccess;
					if (ok) ok = yakamd_feed_hashed_dev(s0, h2, t2, (int64_t)n, t0, n) == 0;
					if (ok) ok = hipStreamSynchronize(yk_ctx_stream(c0)) == hipSuccess;
					yakamd_dev_free(t2);
					if (sum) held.push_back(std::move(copy));
					t0 += n;
					yk_pool_release(d_hash); yk_pool_release(d_t); yk_pool_release(d_cnt);
					continue;
				}
			}
			if (ok && n) ok = yakamd_feed_hashed_dev(s0, d_hash, d_t, (int64_t)n, t0, n) == 0;
			t0 += n;
			yk_pool_release(d_t);
			if (sum) held.emplace_back(d_hash, d_cnt, n, false);
			else yk_pool_release(d_hash);
		}
		if (yakamd_pass_end(s0) < 0) ok = false;                 /* closes the pass whatever the feeds did */
		yk_ctx_gate(c0, true);
		for (const Held &l : held) ok = ok && yk_ctx_add_counts(c0, l.hash, l.cnt, l.n) == 0;   /* every listed key is in s0 now, one above its old count */
		if (ok) s0->tot = yk_ctx_keys_total(c0);                /* htab.c:284: tot = sum of the sub-table sizes */
	}
	set_tot(h0);
	return ok;
}

extern "C" {

void yak_ch_subtract(yak_ch_t *h0, const yak_ch_t *h1, int n_thread) { (void)n_thread; keep_by_membership(h0, h1, 1, __func__); }
void yak_ch_isec(yak_ch_t *h0, const yak_ch_t *h1, int n_thread) { (void)n_thread; keep_by_membership(h0, h1, 2, __func__); }

/* reference htab.c:246-285: every k-mer of h1 with min <= count <= max is put into h0 (its count in
 * h0 goes up by one, saturating; new k-mers start at 1), sub-table by sub-table in h1's slot order;
 * h1 is destroyed. */
void yak_ch_merge(yak_ch_t *h0, yak_ch_t *h1, int min, int max, int n_thread, int pre_resize)
{
	(void)n_thread;
	const int hi = (max >= min && max <= YAK_MAX_COUNT) ? max : YAK_MAX_COUNT;
	bool ok = h0->k == h1->k && h0->pre == h1->pre;
	if (!ok) { fprintf(stderr, "[E::yak_ch_merge] tables of different k / prefix length\n"); set_tot(h0); }
	else ok = put_listed(h0, h1, min, hi, pre_resize, false);
	if (!ok) fprintf(stderr, "[E::yak_ch_merge] %s\n", yakamd_last_error());
	yak_ch_destroy(h1);                                          /* htab.c:283: h1 is consumed whatever happened */
}

/* include/yak_amd.h: h0 += h1, count by count.  Everything that can be refused is refused before h0 is touched */
int yakamd_ch_sum(yak_ch_t *h0, const yak_ch_t *h1, int pre_resize)
{
	const yak_ch_ext *e0 = (const yak_ch_ext*)h0, *e1 = (const yak_ch_ext*)h1;
	if (!h0 || !h1 || e0->magic != EXT_MAGIC || e1->magic != EXT_MAGIC) return yk_set_error("yakamd_ch_sum: not an engine table");
	if (h0 == h1) return yk_set_error("yakamd_ch_sum: the two tables are the same one");
	if (h0->k != h1->k || h0->pre != h1->pre) return yk_set_error("yakamd_ch_sum: tables of different k / prefix length (k %d and %d, pre %d and %d)", h0->k, h1->k, h0->pre, h1->pre);
	for (const yak_ch_t *h : { (const yak_ch_t*)h0, h1 })
		for (yak_ch_t *s : shards_of(h))
			if (!s || ((yak_ch_ext*)s)->magic != EXT_MAGIC || !shard_ctx(s)) return yk_set_error("yakamd_ch_sum: not an engine table");
			else if (yk_ctx_in_pass(shard_ctx(s))) return yk_set_error("yakamd_ch_sum during an open pass");
	return put_listed(h0, h1, 1, YAK_MAX_COUNT, pre_resize, true) ? 0 : -1;
}

} /* extern "C" */
