/*
 * yak_api.cpp -- the drop-in C surface (include/yak.h) on top of the HBM-resident engine.
 *
 * Every function keeps the reference's name, argument meaning, return convention and messages
 * (reference file:line cited per function): the table's life cycle, insert_list, the operations on
 * two tables (subtract / isec, merge / sum), dump and restore.  Host work here is orchestration only;
 * all counting, bloom gating, table layout, clearing and shrinking run in the HIP kernels of
 * kernels.hip.  yak_count() is in yak_count.cpp, the input reader in yak_reader.cpp, qv's solver in
 * yak_qv_solve.cpp.
 */
#include "yak_host.h"
#include <unistd.h>

extern "C" {

int yak_verbose = 3;                                         /* reference sys.c:5 */

unsigned char seq_nt4_table[256] = {                         /* reference misc.c:4-21 */
#define R4(v) v, v, v, v
#define R16(v) R4(v), R4(v), R4(v), R4(v)
	0, 1, 2, 3, R4(4), R4(4), R4(4),
	R16(4), R16(4), R16(4),
	4, 0, 4, 1, 4, 4, 4, 2, R4(4), R4(4),
	4, 4, 4, 4, 3, 3, 4, 4, R4(4), R4(4),
	4, 0, 4, 1, 4, 4, 4, 2, R4(4), R4(4),
	4, 4, 4, 4, 3, 3, 4, 4, R4(4), R4(4),
	R16(4), R16(4), R16(4), R16(4), R16(4), R16(4), R16(4), R16(4)
#undef R16
#undef R4
};

} /* extern "C" */
static double yk_realtime0 = -1;
double yk_realtime(void)                                     /* (C++ linkage, as yak_host.h declares them) */
{
	struct timeval tp;
	gettimeofday(&tp, 0);
	const double t = tp.tv_sec + tp.tv_usec * 1e-6;
	if (yk_realtime0 < 0) yk_realtime0 = t;
	return t - yk_realtime0;
}
double yk_cputime(void)
{
	struct rusage r;
	getrusage(RUSAGE_SELF, &r);
	return r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec);
}
extern "C" {

void yak_copt_init(yak_copt_t *o)                            /* reference misc.c:23-32 */
{
	memset(o, 0, sizeof(*o));
	o->bf_shift = 0; o->bf_n_hash = 4; o->k = 31; o->pre = 10; o->n_thread = 4;
	o->chunk_size = 10000000;
}

/* ---- stand-alone host bloom filter: API completeness only (reference bbf.c); the counting path
 * keeps its filters in HBM and never calls these ---- */
yak_bf_t *yak_bf_init(int n_shift, int n_hashes)
{
	if (n_shift + YAK_BLK_SHIFT > 64 || n_shift < YAK_BLK_SHIFT) return 0;
	yak_bf_t *b = (yak_bf_t*)calloc(1, sizeof(*b));
	void *p = 0;
	b->n_shift = n_shift; b->n_hashes = n_hashes;
	if (posix_memalign(&p, 64, (size_t)1 << (n_shift - 3)) != 0) { free(b); return 0; }
	memset(p, 0, (size_t)1 << (n_shift - 3));
	b->b = (uint8_t*)p;
	return b;
}

void yak_bf_destroy(yak_bf_t *b) { if (b) { free(b->b); free(b); } }

int yak_bf_insert(yak_bf_t *b, uint64_t hash)
{
	const int lgblk = b->n_shift - YAK_BLK_SHIFT;
	uint8_t *blk = b->b + ((hash & ((1ULL << lgblk) - 1)) << 6);
	int z = (int)(hash >> lgblk) & YAK_BLK_MASK, step = (int)(hash >> b->n_shift) & YAK_BLK_MASK, hits = 0;
	if ((step & 31) == 0) step = (step + 1) & YAK_BLK_MASK;
	for (int i = 0; i < b->n_hashes; ++i, z = (z + step) & YAK_BLK_MASK) {
		hits += blk[z >> 3] >> (z & 7) & 1;
		blk[z >> 3] |= (uint8_t)(1 << (z & 7));
	}
	return hits;
}

/* ---- table life cycle (reference htab.c:13-49) ---- */
yak_ch_t *yak_ch_init(int k, int pre, int n_hash, int n_shift)
{
	if (pre < YAK_COUNTER_BITS) return 0;
	yakamd_ctx *ctx = yk_ctx_create(k, pre, n_hash, n_shift);
	if (!ctx) return 0;                                      /* no GPU: fail, never count on the CPU */
	yak_ch_ext *e = (yak_ch_ext*)calloc(1, sizeof(*e));
	e->ctx = ctx; e->magic = EXT_MAGIC;
	yak_ch_t *h = &e->pub;
	h->k = k; h->pre = pre;
	h->h = (yak_ch1_t*)calloc((size_t)1 << pre, sizeof(yak_ch1_t));
	if (n_hash > 0 && n_shift > pre) {
		h->n_hash = n_hash; h->n_shift = n_shift;
		if (n_shift - pre >= YAK_BLK_SHIFT && n_shift - pre + YAK_BLK_SHIFT <= 64) {
			/* descriptors only: the bits live in HBM (b == NULL on the host side) */
			yak_bf_t *bf = (yak_bf_t*)calloc((size_t)1 << pre, sizeof(yak_bf_t));
			for (int i = 0; i < 1 << pre; ++i) { bf[i].n_shift = n_shift - pre; bf[i].n_hashes = n_hash; h->h[i].b = &bf[i]; }
		}
	}
	yk_ctx_sync_host(ctx, h);
	return h;
}

int multi_refuse(const yak_ch_t *h, const char *what)
{
	if (!YK_MULTI((const yak_ch_ext*)h)) return 0;
	fprintf(stderr, "[E::%s] " YK_MSG_SHARDED " (several GPUs, or a large unfiltered count taken in sweeps: YAKAMD_GPUS / YAKAMD_AUTO_SWEEP_GB)\n", what);
	return 1;
}

void yak_ch_destroy_bf(yak_ch_t *h)
{
	yak_ch_ext *e = (yak_ch_ext*)h;
	if (YK_MULTI(e)) { for (int r = 0; r < e->n_sub; ++r) yak_ch_destroy_bf(e->sub[r]); for (int i = 0; i < 1 << h->pre; ++i) h->h[i].b = 0; return; }
	if (h->h[0].b) free(h->h[0].b);                          /* one block of descriptors */
	for (int i = 0; i < 1 << h->pre; ++i) h->h[i].b = 0;
	yk_ctx_destroy_bf(e->ctx);
}

void yak_ch_destroy(yak_ch_t *h)
{
	if (h == 0) return;
	yak_ch_ext *e = (yak_ch_ext*)h;
	if (YK_MULTI(e)) { for (int r = 0; r < e->n_sub; ++r) yak_ch_destroy(e->sub[r]); free(e->sub); free(h->h); free(e); return; }
	yak_ch_destroy_bf(h);
	yk_ctx_destroy(e->ctx);
	free(h->h); free(e);
}

/* ---- reference htab.c:51-78.  The list is one bucket of hashed k-mers sharing a prefix; list
 * order is stream order.  Runs as a one-batch device pass. ---- */
int yak_ch_insert_list(yak_ch_t *h, int create_new, int n, const uint64_t *a)
{
	yak_ch_ext *e = (yak_ch_ext*)h;
	if (n <= 0) return 0;
	if (YK_MULTI(e)) return yak_ch_insert_list(e->sub[(a[0] & ((1ULL << h->pre) - 1)) * e->n_sub >> h->pre], create_new, n, a);   /* the owner of the list's prefix */
	const uint64_t pm = (1ULL << h->pre) - 1;
	std::vector<uint64_t> hv; std::vector<uint32_t> tv;
	hv.reserve(n); tv.reserve(n);
	for (int j = 0; j < n; ++j)
		if ((a[j] & pm) == (a[0] & pm)) { hv.push_back(a[j]); tv.push_back((uint32_t)j); }   /* htab.c:61 */
	/* the reference's callers run this from kt_for workers, one sub-table each (count.c:129-143); here a call
	 * is a whole-table device pass, so concurrent callers take turns.  Failures are reported, never silent. */
	struct Lock { yakamd_ctx *c; Lock(yakamd_ctx *c_) : c(c_) { yk_ctx_lock(c); } ~Lock() { yk_ctx_unlock(c); } } lock(e->ctx);
	const size_t nb = hv.size() * 8, need = ((nb + 15) & ~(size_t)15) + hv.size() * 4;
	uint8_t *d = (uint8_t*)yk_ctx_scratch(e->ctx, need);
	int64_t n_ins = -1;
	bool ok = d != 0 && hipSetDevice(yk_ctx_device(e->ctx)) == hipSuccess;
	uint64_t *d_h = (uint64_t*)d; uint32_t *d_t = (uint32_t*)(d + ((nb + 15) & ~(size_t)15));
	ok = ok && hipMemcpy(d_h, hv.data(), nb, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_t, tv.data(), tv.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
	if (ok) {
		const uint64_t t0 = yk_ctx_list_time(e->ctx, (uint64_t)n);
		ok = yakamd_pass_begin(h, create_new) == 0;
		if (ok) {
			ok = yakamd_feed_hashed_dev(h, d_h, d_t, (int64_t)hv.size(), t0, (uint64_t)n) == 0;
			n_ins = yakamd_pass_end(h);                          /* closes the pass whatever the feed did */
			ok = ok && n_ins >= 0;
		}
	}
	if (!ok) { fprintf(stderr, "[E::%s] %s\n", __func__, *yakamd_last_error() ? yakamd_last_error() : "device buffer allocation or copy failed"); return -1; }
	return (int)n_ins;
}

static inline uint32_t ht_cap(const yak_ht_t *g) { return g->keys ? 1U << g->bits : 0U; }

static uint32_t ht_get(const yak_ht_t *g, uint64_t key)      /* khashl.h:137-150 on the host mirror */
{
	if (g->keys == 0) return 0;
	const uint32_t n = 1U << g->bits, mask = n - 1;
	uint32_t i = (uint32_t)((uint32_t)(key >> YAK_COUNTER_BITS) * 2654435769U) >> (32 - g->bits), first = i;
	while ((g->used[i >> 5] >> (i & 31) & 1) && g->keys[i] >> YAK_COUNTER_BITS != key >> YAK_COUNTER_BITS) {
		i = (i + 1) & mask;
		if (i == first) return n;
	}
	return (g->used[i >> 5] >> (i & 31) & 1) ? i : n;
}

int yak_ch_get(const yak_ch_t *h, uint64_t x)                /* reference htab.c:93-100 */
{
	yak_ch_ext *e = (yak_ch_ext*)h;
	if (YK_MULTI(e)) return yak_ch_get(e->sub[(x & ((1ULL << h->pre) - 1)) * e->n_sub >> h->pre], x);
	if (yk_ctx_sync_host(e->ctx, (yak_ch_t*)h)) return -1;
	const yak_ht_t *g = h->h[x & ((1ULL << h->pre) - 1)].h;
	const uint32_t i = ht_get(g, x >> h->pre << YAK_COUNTER_BITS);
	return i == ht_cap(g) ? -1 : (int)(g->keys[i] & YAK_MAX_COUNT);
}

int yak_ch_inc(yak_ch_t *h, uint64_t x)                      /* reference htab.c:80-91 */
{
	if (YK_MULTI((yak_ch_ext*)h)) { yak_ch_ext *e = (yak_ch_ext*)h; return yak_ch_inc(e->sub[(x & ((1ULL << h->pre) - 1)) * e->n_sub >> h->pre], x); }
	int c = -1;                                              /* one single-lane kernel on the table image; a valid host mirror is patched in place */
	yakamd_ctx *ctx = ((yak_ch_ext*)h)->ctx;
	struct Lock { yakamd_ctx *c; Lock(yakamd_ctx *c_) : c(c_) { yk_ctx_lock(c); } ~Lock() { yk_ctx_unlock(c); } } lock(ctx);   /* shares the stream and the counters with yak_ch_insert_list */
	if (yk_ctx_inc(ctx, x, &c) != 0) { fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error()); return -1; }
	return c;
}

void yak_ch_clear(yak_ch_t *h, int n_thread)                 /* reference htab.c:127-130 */
{
	(void)n_thread;
	if (YK_MULTI((yak_ch_ext*)h)) { yak_ch_ext *e = (yak_ch_ext*)h; for (int r = 0; r < e->n_sub; ++r) yak_ch_clear(e->sub[r], n_thread); return; }
	yk_ctx_clear(((yak_ch_ext*)h)->ctx);
}

void yak_ch_shrink(yak_ch_t *h, int min, int max, int n_thread) /* reference htab.c:199-208 */
{
	(void)n_thread;
	if (YK_MULTI((yak_ch_ext*)h)) {                           /* every GPU shrinks its own sub-tables, side by side */
		yak_ch_ext *e = (yak_ch_ext*)h;
		std::vector<std::thread> th;
		for (int r = 0; r < e->n_sub; ++r) th.emplace_back([=]() { yak_ch_shrink(e->sub[r], min, max, n_thread); });
		for (auto &t : th) t.join();
		multi_tot(h);
		return;
	}
	unsigned long long tot = 0;
	const int hi = (max >= min && max <= YAK_MAX_COUNT) ? max : YAK_MAX_COUNT;
	if (yk_ctx_shrink(((yak_ch_ext*)h)->ctx, min, hi, &tot) == 0) h->tot = tot;
}

/* reference htab.c:102-110: resize every sub-table filled to less than a third */
void yak_ch_tighten(yak_ch_t *h)
{
	if (YK_MULTI((yak_ch_ext*)h)) { yak_ch_ext *e = (yak_ch_ext*)h; for (int r = 0; r < e->n_sub; ++r) yak_ch_tighten(e->sub[r]); return; }
	if (yk_ctx_tighten(((yak_ch_ext*)h)->ctx)) fprintf(stderr, "[E::yak_ch_tighten] %s\n", yakamd_last_error());
}

/* ---- operations on two tables.  Either operand may be sharded over prefix ranges (yak_count() shards by itself: several GPUs, or an
 * unfiltered count of a large plain file taken in sweeps); every sub-table belongs to exactly one shard of each operand, and the
 * reference's operations are per sub-table (kt_for over 1 << pre, htab.c:246-347), so they are carried out shard by shard. ---- */
int64_t yakamd_dump_mem(yak_ch_t *h, uint8_t **out);
int64_t yakamd_dump_range_mem(yak_ch_t *h, int lo, int hi, uint8_t **out);
static std::vector<yak_ch_t*> shards_of(const yak_ch_t *h)
{
	const yak_ch_ext *e = (const yak_ch_ext*)h;
	return YK_MULTI(e) ? std::vector<yak_ch_t*>(e->sub, e->sub + e->n_sub) : std::vector<yak_ch_t*>(1, (yak_ch_t*)h);
}
static inline yakamd_ctx *shard_ctx(yak_ch_t *s) { return ((yak_ch_ext*)s)->ctx; }
static void set_tot(yak_ch_t *h) { if (YK_MULTI((yak_ch_ext*)h)) multi_tot(h); }

static bool parse_yak_image(const uint8_t *img, size_t sz, uint32_t hdr[3], std::vector<uint32_t> &caps, std::vector<uint32_t> &sizes, std::vector<uint64_t> &keys)
{
	if (sz < 16 || memcmp(img, YAK_MAGIC, 4) != 0) return false;
	memcpy(hdr, img + 4, 12);
	const int P = 1 << hdr[1];
	caps.assign(P, 0); sizes.assign(P, 0); keys.clear();
	size_t off = 16;
	for (int p = 0; p < P; ++p) {
		if (off + 8 > sz) return false;
		uint32_t u[2]; memcpy(u, img + off, 8); off += 8;
		if (off + (size_t)8 * u[1] > sz) return false;
		caps[p] = u[0]; sizes[p] = u[1];
		const size_t at = keys.size();
		keys.resize(at + u[1]);
		if (u[1]) memcpy(&keys[at], img + off, (size_t)8 * u[1]);
		off += (size_t)8 * u[1];
	}
	return true;
}

/* an unsharded copy of `h` on device `dev`, by way of its .yak image (same keys and counts; the slot layout is the restored one, which
 * membership tests do not look at).  Only for the second operand of subtract / isec when it is sharded or lives on another device */
static yak_ch_t *unsharded_copy(const yak_ch_t *h, int dev)
{
	uint8_t *img = 0;
	const int64_t sz = yakamd_dump_mem((yak_ch_t*)h, &img);
	if (sz < 0) return 0;
	uint32_t hdr[3];
	std::vector<uint32_t> caps, sizes;
	std::vector<uint64_t> keys;
	const bool ok = parse_yak_image(img, (size_t)sz, hdr, caps, sizes, keys);
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

void yak_ch_subtract(yak_ch_t *h0, const yak_ch_t *h1, int n_thread) { (void)n_thread; keep_by_membership(h0, h1, 1, __func__); }
void yak_ch_isec(yak_ch_t *h0, const yak_ch_t *h1, int n_thread) { (void)n_thread; keep_by_membership(h0, h1, 2, __func__); }

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

void yak_ch_hist(const yak_ch_t *h, int64_t cnt[YAK_N_COUNTS], int n_thread) /* reference htab.c:156-169 */
{
	(void)n_thread;
	memset(cnt, 0, YAK_N_COUNTS * sizeof(int64_t));
	if (YK_MULTI((const yak_ch_ext*)h)) {
		const yak_ch_ext *e = (const yak_ch_ext*)h;
		std::vector<int64_t> part(YAK_N_COUNTS);
		for (int r = 0; r < e->n_sub; ++r) { yak_ch_hist(e->sub[r], part.data(), n_thread); for (int i = 0; i < YAK_N_COUNTS; ++i) cnt[i] += part[i]; }
		return;
	}
	if (yk_ctx_hist(((yak_ch_ext*)h)->ctx, cnt)) fprintf(stderr, "[E::yak_ch_hist] %s\n", yakamd_last_error());
}

void yak_ch_setcnt(yak_ch_t *h, int cnt, int n_thread)        /* reference htab.c:219-235: every stored k-mer gets count `cnt` */
{
	(void)n_thread;
	if (YK_MULTI((yak_ch_ext*)h)) { yak_ch_ext *e = (yak_ch_ext*)h; for (int r = 0; r < e->n_sub; ++r) yak_ch_setcnt(e->sub[r], cnt, n_thread); return; }
	if (yk_ctx_setcnt(((yak_ch_ext*)h)->ctx, cnt)) fprintf(stderr, "[E::yak_ch_setcnt] %s\n", yakamd_last_error());
}

yak_knt_t *yak_ch_getseq(const yak_ch_t *h, int w, uint32_t *n) /* reference htab.c:353-367 */
{
	assert(h->k < 32 && w < 1 << h->pre);
	if (YK_MULTI((const yak_ch_ext*)h)) { const yak_ch_ext *e = (const yak_ch_ext*)h; return yak_ch_getseq(e->sub[(uint64_t)w * e->n_sub >> h->pre], w, n); }
	*n = 0;
	if (yk_ctx_sync_host(((yak_ch_ext*)h)->ctx, (yak_ch_t*)h)) return 0;
	const yak_ht_t *g = h->h[w].h;
	const uint64_t mask = (1ULL << h->k * 2) - 1;
	yak_knt_t *a = (yak_knt_t*)calloc(g->count ? g->count : 1, sizeof(*a));
	uint32_t j = 0;
	for (uint32_t i = 0, cap = ht_cap(g); i < cap; ++i)
		if (g->used[i >> 5] >> (i & 31) & 1) {
			a[j].x = yk_hash64_inv(g->keys[i] >> YAK_COUNTER_BITS << h->pre | (uint64_t)w, mask);
			a[j++].c = (int)(g->keys[i] & YAK_MAX_COUNT);
		}
	*n = g->count;
	return a;
}

/* ---- .yak serialisation (reference htab.c:373-394): header, then per sub-table capacity, size and
 * the keys in ascending slot order.  Every shard puts the bytes of its own sub-tables together on its device
 * (StagedRange); they come back in one copy (yakamd_dump_mem), or go to the file in 8 MiB pieces through a
 * few page-locked buffers that writer threads pwrite() while the next pieces are on the bus (yak_ch_dump) ---- */
struct DumpSink {
	uint8_t *mem; int fd;                                      /* one of the two */
	bool put(int dev, hipStream_t st, const uint8_t *d_src, size_t bytes, size_t off);
};
bool DumpSink::put(int dev, hipStream_t st, const uint8_t *d_src, size_t bytes, size_t off)
{
	if (bytes == 0) return true;
	if (hipSetDevice(dev) != hipSuccess) return false;            /* the events below are recorded on `st`: they must be this device's */
	if (mem) return hipMemcpyAsync(mem + off, d_src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
	enum { NB = 6, W = 3 };
	const size_t CH = (size_t)8 << 20, n_ch = (bytes + CH - 1) / CH;
	static std::mutex mu;                                         /* the staging buffers are the process's: one dump at a time uses them */
	static void *stage[NB] = { 0 };
	std::lock_guard<std::mutex> lk(mu);
	for (int i = 0; i < NB; ++i) if (!stage[i] && hipHostMalloc(&stage[i], CH, hipHostMallocPortable) != hipSuccess) { stage[i] = 0; return false; }
	hipEvent_t ev[NB];
	for (int i = 0; i < NB; ++i) if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) { while (i-- > 0) (void)hipEventDestroy(ev[i]); return false; }
	std::vector<int> issued_v(n_ch, 0), written_v(n_ch, 0);
	volatile int *issued = issued_v.data(), *written = written_v.data();
	bool good = true;
	std::vector<std::thread> th;
	for (int w = 0; w < W; ++w) th.emplace_back([&, w]() {
		(void)hipSetDevice(dev);
		for (size_t j = (size_t)w; j < n_ch; j += W) {
			while (!__atomic_load_n(&issued[j], __ATOMIC_ACQUIRE)) std::this_thread::yield();
			bool ok = __atomic_load_n(&issued[j], __ATOMIC_ACQUIRE) == 1 && hipEventSynchronize(ev[j % NB]) == hipSuccess;
			const size_t n = std::min(CH, bytes - j * CH);
			for (size_t done = 0; ok && done < n; ) {
				const ssize_t r = ::pwrite(fd, (const char*)stage[j % NB] + done, n - done, (off_t)(off + j * CH + done));
				if (r <= 0) ok = false; else done += (size_t)r;
			}
			if (!ok) __atomic_store_n(&good, false, __ATOMIC_RELAXED);
			__atomic_store_n(&written[j], 1, __ATOMIC_RELEASE);
		}
	});
	for (size_t i = 0; i < n_ch; ++i) {
		if (i >= NB) while (!__atomic_load_n(&written[i - NB], __ATOMIC_ACQUIRE)) std::this_thread::yield();
		const size_t n = std::min(CH, bytes - i * CH);
		const bool ok = hipMemcpyAsync(stage[i % NB], d_src + i * CH, n, hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(ev[i % NB], st) == hipSuccess;
		__atomic_store_n(&issued[i], ok ? 1 : 2, __ATOMIC_RELEASE);
	}
	for (auto &t : th) t.join();
	(void)hipStreamSynchronize(st);
	for (int i = 0; i < NB; ++i) (void)hipEventDestroy(ev[i]);
	return good;
}

/* the bytes of sub-tables [lo, hi) -- {capacity, size, keys in slot order} each -- through `sink`, behind the 16-byte header when `head` is set (the whole
 * table then: the .yak image), every shard staging the part it owns; their number, or -1.  sink == 0: the number alone */
static int64_t dump_through(yak_ch_t *h, int lo, int hi, bool head, DumpSink *sink)
{
	yak_ch_ext *e = (yak_ch_ext*)h;
	const int P = 1 << h->pre, n_sub = YK_MULTI(e) ? e->n_sub : 1;
	if (lo < 0 || hi > P || lo >= hi) return -1;
	struct Part { yak_ch_t *hs; int a, b; };
	std::vector<Part> part;
	size_t sz = (head ? 16 : 0) + (size_t)8 * (hi - lo), off = 0;
	uint32_t cap, cnt;
	for (int r = 0; r < n_sub; ++r) {
		const Part pt = { YK_MULTI(e) ? e->sub[r] : h, std::max(lo, (int)(((int64_t)r << h->pre) / n_sub)), std::min(hi, (int)(((int64_t)(r + 1) << h->pre) / n_sub)) };
		for (int p = pt.a; p < pt.b; ++p) { if (yakamd_subtable(pt.hs, p, &cap, &cnt) != 0) return -1; sz += (size_t)8 * cnt; }
		if (pt.a < pt.b) part.push_back(pt);
	}
	if (!sink) return (int64_t)sz;
	if (head) {
		uint8_t hd[16];
		const uint32_t t[3] = { (uint32_t)h->k, (uint32_t)h->pre, YAK_COUNTER_BITS };
		memcpy(hd, YAK_MAGIC, 4); memcpy(hd + 4, t, 12);
		if (sink->mem) memcpy(sink->mem, hd, 16);
		else if (::pwrite(sink->fd, hd, 16, 0) != 16) return -1;
		off = 16;
	}
	for (const Part &pt : part) {
		yakamd_ctx *c = ((yak_ch_ext*)pt.hs)->ctx;
		StagedRange s;                                               /* (the image goes back when the shard is written) */
		if (s.stage(c, pt.a, pt.b) != 0 || off + (size_t)s.n_words * 8 > sz || !sink->put(yk_ctx_device(c), yk_ctx_stream(c), (const uint8_t*)s.d_img, (size_t)s.n_words * 8, off)) return -1;
		off += (size_t)s.n_words * 8;
	}
	return off == sz ? (int64_t)sz : -1;
}

/* to memory: the whole image (yakamd_dump_mem), or the bytes of sub-tables [lo, hi) alone, no header: what one rank of a prefix-sharded job owns of
 * the .yak file (tests and bench.py compare a rank's share with the oracle's without serialising the whole table) */
static int64_t dump_to_mem(yak_ch_t *h, int lo, int hi, bool head, uint8_t **out)
{
	*out = 0;
	const int64_t sz = dump_through(h, lo, hi, head, 0);
	if (sz < 0) return -1;
	DumpSink sink; sink.mem = (uint8_t*)malloc((size_t)sz); sink.fd = -1;
	if (!sink.mem) return -1;
	if (dump_through(h, lo, hi, head, &sink) != sz) { free(sink.mem); return -1; }
	*out = sink.mem;
	return sz;
}
int64_t yakamd_dump_mem(yak_ch_t *h, uint8_t **out) { return dump_to_mem(h, 0, 1 << h->pre, true, out); }
int64_t yakamd_dump_range_mem(yak_ch_t *h, int lo, int hi, uint8_t **out) { return dump_to_mem(h, lo, hi, false, out); }

int yak_ch_dump(const yak_ch_t *h, const char *fn)
{
	struct stat sb;
	const bool to_stdout = strcmp(fn, "-") == 0;
	if (to_stdout || (stat(fn, &sb) == 0 && !S_ISREG(sb.st_mode))) {   /* a pipe (or any name that is no regular file) takes the image in one piece */
		FILE *fp = to_stdout ? stdout : fopen(fn, "wb");
		if (fp == 0) return -1;
		uint8_t *buf = 0;
		const int64_t sz = yakamd_dump_mem((yak_ch_t*)h, &buf);
		if (sz < 0) { if (!to_stdout) fclose(fp); return -1; }
		const bool ok = fwrite(buf, 1, (size_t)sz, fp) == (size_t)sz;
		free(buf);
		if ((to_stdout ? fflush(fp) : fclose(fp)) != 0 || !ok) return -1;
	} else {
		const double t0 = yk_realtime();
		DumpSink sink; sink.mem = 0;
		/* fopen(fn, "wb"), htab.c:377 -- except that a file that is there is cut to the new size AFTER it was written over: its pages are reused
		 * instead of being given back and asked for again (0.05 s instead of 0.12 s for 420 MB) */
		sink.fd = ::open(fn, O_WRONLY | O_CREAT, 0666);
		if (sink.fd < 0) return -1;
		const int64_t sz = dump_through((yak_ch_t*)h, 0, 1 << h->pre, true, &sink);
		const bool cut = sz >= 0 && ::ftruncate(sink.fd, (off_t)sz) == 0;
		if (sz < 0) (void)::ftruncate(sink.fd, 0);                  /* a dump that failed midway leaves an empty file, not a header in front of old bytes (fopen "wb", htab.c:377, never keeps any) */
		if (::close(sink.fd) != 0 || !cut) return -1;
		if (getenv("YAKAMD_VERBOSE")) fprintf(stderr, "[yak_amd] dump: %.1f MB in %.3f s\n", sz / 1e6, yk_realtime() - t0);
	}
	fprintf(stderr, "[M::%s] dumpped the hash table to file '%s'.\n", __func__, fn);
	return 0;
}

/* reference htab.c:396-481 (mode YAK_LOAD_ALL): every sub-table is pre-sized to the saved
 * capacity and the keys are put back in file order -- the same staged FCFS replay as shrink */
/* reads a .yak file (htab.c:413-433): header checks, then per sub-table capacity, size and keys */
static bool read_yak(const char *fn, uint32_t hdr[3], std::vector<uint32_t> &caps, std::vector<uint32_t> &sizes, std::vector<uint64_t> &keys)
{
	FILE *fp = fopen(fn, "rb");
	char magic[4];
	if (fp == 0) return false;
	if (fread(magic, 1, 4, fp) != 4) { fclose(fp); return false; }
	if (strncmp(magic, YAK_MAGIC, 4) != 0) { fprintf(stderr, "ERROR: wrong file magic.\n"); fclose(fp); return false; }
	if (fread(hdr, 4, 3, fp) != 3) { fclose(fp); return false; }
	if (hdr[2] != YAK_COUNTER_BITS) {
		fprintf(stderr, "ERROR: saved counter bits: %d; compile-time counter bits: %d\n", hdr[2], YAK_COUNTER_BITS);
		fclose(fp); return false;
	}
	if (hdr[1] < YAK_COUNTER_BITS || hdr[1] > 24) { fclose(fp); return false; }
	const int P = 1 << hdr[1];
	caps.assign(P, 0); sizes.assign(P, 0); keys.clear();
	for (int p = 0; p < P; ++p) {
		uint32_t u[2];
		if (fread(u, 4, 2, fp) != 2) break;
		/* a capacity is 0 or a power of two <= 2^31 (khashl.h:155-158), and it holds its keys at <= 75 % load after the
		 * resize-before-put rule: anything else is a corrupt file */
		if (u[0] > (1u << 31) || (u[0] & (u[0] - 1)) != 0 || u[1] > u[0]) { fprintf(stderr, "ERROR: corrupt sub-table header in '%s' (capacity %u, size %u)\n", fn, u[0], u[1]); fclose(fp); return false; }
		caps[p] = u[0]; sizes[p] = u[1];
		const size_t at = keys.size();
		keys.resize(at + u[1]);
		if (u[1] && fread(&keys[at], 8, u[1], fp) != u[1]) break;
	}
	fclose(fp);
	return true;
}

/* reference htab.c:396-476.  YAK_LOAD_ALL builds the table from the file; the flag modes (trio binning
 * 2 / 3 with min_cnt, mid_cnt; sex chromosomes 4 / 5 / 6) put every selected key with a flag in its low
 * bits, ORing the flag into keys already present -- one counting pass on the device whose records
 * carry the flag in the low 4 bits of their list position. */
yak_ch_t *yak_ch_restore_core(yak_ch_t *ch0, const char *fn, int mode, ...)
{
	int min_cnt = 0, mid_cnt = 0;
	va_list ap;
	va_start(ap, mode);
	if (mode == YAK_LOAD_TRIOBIN1 || mode == YAK_LOAD_TRIOBIN2) { min_cnt = va_arg(ap, int); mid_cnt = va_arg(ap, int); }
	va_end(ap);
	if (mode < YAK_LOAD_ALL || mode > YAK_LOAD_SEXCHR3) return 0;
	if (ch0 == 0 && (mode == YAK_LOAD_TRIOBIN2 || mode == YAK_LOAD_SEXCHR2 || mode == YAK_LOAD_SEXCHR3)) return 0;   /* htab.c:413-420 */
	uint32_t hdr[3];
	std::vector<uint32_t> caps, sizes;
	std::vector<uint64_t> keys;
	if (!read_yak(fn, hdr, caps, sizes, keys)) return 0;
	if (mode == YAK_LOAD_ALL && ch0 == 0) {
		yak_ch_t *h = yak_ch_init((int)hdr[0], (int)hdr[1], 0, 0);
		if (h == 0) return 0;
		if (yk_ctx_load(((yak_ch_ext*)h)->ctx, caps.data(), sizes.data(), keys.data()) != 0) { yak_ch_destroy(h); return 0; }
		fprintf(stderr, "[M::%s] inserted %ld k-mers, of which %ld are new\n", __func__, (long)keys.size(), (long)keys.size());
		return h;
	}
	/* every other case puts the selected keys, in file order, into a table that may already hold some of them
	 * (htab.c:441-470): a flag mode ORs a flag into keys already present, YAK_LOAD_ALL leaves them alone, and a
	 * new key keeps the flag / its saved count.  That is a counting pass whose records carry the payload in the low
	 * bits of their list position (4 bits for a flag, 10 for a count), run in as many passes as the 32-bit
	 * position field needs: a pass meets the keys of the earlier ones as existing state, exactly as the
	 * reference's sequential puts do. */
	if (ch0 && multi_refuse(ch0, __func__)) return 0;           /* a load into a table sharded over prefix ranges: not carried out shard by shard (yet) */
	yak_ch_t *h = ch0 ? ch0 : yak_ch_init((int)hdr[0], (int)hdr[1], 0, 0);
	if (h == 0) return 0;
	assert((int)hdr[0] == h->k && (int)hdr[1] == h->pre);       /* htab.c:437 */
	yakamd_ctx *c = ((yak_ch_ext*)h)->ctx;
	const int P = 1 << h->pre;
	const uint64_t mask = (1ULL << YAK_COUNTER_BITS) - 1;
	const int pbits = mode == YAK_LOAD_ALL ? YAK_COUNTER_BITS : 4;
	size_t per_pass = ((size_t)1 << (32 - pbits)) - 16;
	if (yk_knob("YAKAMD_LOAD_SLICE", 0) > 0) per_pass = std::min<size_t>(per_pass, (size_t)yk_knob("YAKAMD_LOAD_SLICE", 0));   /* tests */
	std::vector<uint64_t> hashes;
	std::vector<uint32_t> times;
	long n_tot = 0, n_new = 0;
	bool ok = yk_ctx_resize_to(c, caps.data()) == 0;             /* htab.c:441 */
	void *d_h = 0, *d_t = 0;
	auto flush = [&]() {
		const size_t n = hashes.size();
		if (n == 0 || !ok) return;
		if (!d_h) { d_h = yakamd_dev_alloc(std::min(per_pass, keys.size()) * 8); d_t = yakamd_dev_alloc(std::min(per_pass, keys.size()) * 4); }
		ok = d_h && d_t && yakamd_memcpy_h2d(d_h, hashes.data(), n * 8) == 0 && yakamd_memcpy_h2d(d_t, times.data(), n * 4) == 0;
		if (ok) {
			yk_ctx_gate(c, false); yk_ctx_or_mode(c, mode == YAK_LOAD_ALL ? 2 : 1);
			ok = yakamd_pass_begin(h, 1) == 0;
			if (ok) {
				ok = yakamd_feed_hashed_dev(h, d_h, d_t, (int64_t)n, 0, (uint64_t)n << pbits) == 0;
				const int64_t r = yakamd_pass_end(h);
				ok = ok && r >= 0;
				if (ok) n_new += (long)r;
			}
			yk_ctx_gate(c, true); yk_ctx_or_mode(c, 0);
		}
		n_tot += (long)n;
		hashes.clear(); times.clear();
	};
	size_t at = 0;
	for (int p = 0; p < P && ok; ++p)
		for (uint32_t j = 0; j < sizes[p] && ok; ++j, ++at) {
			const uint64_t key = keys[at];
			int x;
			if (mode == YAK_LOAD_ALL) x = (int)(key & mask);
			else if (mode == YAK_LOAD_TRIOBIN1 || mode == YAK_LOAD_TRIOBIN2) {
				const int cnt = (int)(key & mask), shift = mode == YAK_LOAD_TRIOBIN1 ? 0 : 2;
				x = cnt >= mid_cnt ? 2 << shift : cnt >= min_cnt ? 1 << shift : -1;
			} else x = 1 << (mode - YAK_LOAD_SEXCHR1);
			if (x < 0) continue;
			hashes.push_back((key >> YAK_COUNTER_BITS) << h->pre | (uint64_t)p);
			times.push_back((uint32_t)(hashes.size() - 1) << pbits | (uint32_t)x);
			if (hashes.size() >= per_pass) flush();
		}
	flush();
	yakamd_dev_free(d_h); yakamd_dev_free(d_t);
	if (!ok) { fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error()); if (!ch0) yak_ch_destroy(h); return 0; }
	fprintf(stderr, "[M::%s] inserted %ld k-mers, of which %ld are new\n", __func__, n_tot, n_new);
	return h;
}

yak_ch_t *yak_ch_restore(const char *fn) { return yak_ch_restore_core(0, fn, YAK_LOAD_ALL); }   /* reference htab.c:478 */

} /* extern "C" */
