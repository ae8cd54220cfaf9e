/*
 * yak_api.cpp -- the drop-in C surface (include/yak.h) on top of the HBM-resident engine.
 *
 * Every function keeps the reference's name, argument meaning, return convention and messages
 * (reference file:line cited per function).  Here: the globals, the host bloom filter, the table's
 * life cycle and the calls on one table (insert_list, get, inc, clear, shrink, tighten, hist, setcnt,
 * getseq).  The operations on two tables (subtract / isec, merge / sum) are in yak_table_ops.cpp, dump
 * and restore in yak_file.cpp.  Host work here is orchestration only; all counting, bloom gating, table
 * layout, clearing and shrinking run in the HIP kernels of kernels.hip.  yak_count() is in yak_count.cpp,
 * the input reader in yak_reader.cpp, qv's solver in yak_qv_solve.cpp.
 */
#include "yak_host.h"

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
	if (YK_MULTI(e)) for (yak_ch_t *s : shards_of(h)) yak_ch_destroy_bf(s);
	else { if (h->h[0].b) free(h->h[0].b); yk_ctx_destroy_bf(e->ctx); }   /* one block of descriptors */
	for (int i = 0; i < 1 << h->pre; ++i) h->h[i].b = 0;
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
	const uint64_t pm = (1ULL << h->pre) - 1;
	if (YK_MULTI(e)) return yak_ch_insert_list(e->sub[yk_shard_owner(h->pre, e->n_sub, a[0] & pm)], create_new, n, a);   /* the owner of the list's prefix */
	std::vector<uint64_t> hv; std::vector<uint32_t> tv;
	hv.reserve(n); tv.reserve(n);
	for (int j = 0; j < n; ++j)
		if ((a[j] & pm) == (a[0] & pm)) { hv.push_back(a[j]); tv.push_back((uint32_t)j); }   /* htab.c:61 */
	/* the reference's callers run this from kt_for workers, one sub-table each (count.c:129-143); here a call
	 * is a whole-table device pass, so concurrent callers take turns.  Failures are reported, never silent. */
	CtxLock lock(e->ctx);
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
	const uint64_t w = x & ((1ULL << h->pre) - 1);
	if (YK_MULTI(e)) return yak_ch_get(e->sub[yk_shard_owner(h->pre, e->n_sub, w)], x);
	if (yk_ctx_sync_host(e->ctx, (yak_ch_t*)h)) return -1;
	const yak_ht_t *g = h->h[w].h;
	const uint32_t i = ht_get(g, x >> h->pre << YAK_COUNTER_BITS);
	return i == ht_cap(g) ? -1 : (int)(g->keys[i] & YAK_MAX_COUNT);
}

int yak_ch_inc(yak_ch_t *h, uint64_t x)                      /* reference htab.c:80-91 */
{
	yak_ch_ext *e = (yak_ch_ext*)h;
	if (YK_MULTI(e)) return yak_ch_inc(e->sub[yk_shard_owner(h->pre, e->n_sub, x & ((1ULL << h->pre) - 1))], x);
	int c = -1;                                              /* one single-lane kernel on the table image; a valid host mirror is patched in place */
	CtxLock lock(e->ctx);                                    /* shares the stream and the counters with yak_ch_insert_list */
	if (yk_ctx_inc(e->ctx, x, &c) != 0) { fprintf(stderr, "[E::%s] %s\n", __func__, yakamd_last_error()); return -1; }
	return c;
}

void yak_ch_clear(yak_ch_t *h, int n_thread)                 /* reference htab.c:127-130 */
{
	(void)n_thread;
	for (yak_ch_t *s : shards_of(h)) yk_ctx_clear(shard_ctx(s));
}

void yak_ch_shrink(yak_ch_t *h, int min, int max, int n_thread) /* reference htab.c:199-208 */
{
	(void)n_thread;
	if (YK_MULTI((yak_ch_ext*)h)) {                           /* every GPU shrinks its own sub-tables, side by side */
		std::vector<std::thread> th;
		for (yak_ch_t *s : shards_of(h)) th.emplace_back([=]() { yak_ch_shrink(s, min, max, n_thread); });
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
	for (yak_ch_t *s : shards_of(h))
		if (yk_ctx_tighten(shard_ctx(s))) fprintf(stderr, "[E::yak_ch_tighten] %s\n", yakamd_last_error());
}

void yak_ch_hist(const yak_ch_t *h, int64_t cnt[YAK_N_COUNTS], int n_thread) /* reference htab.c:156-169 */
{
	(void)n_thread;
	memset(cnt, 0, YAK_N_COUNTS * sizeof(int64_t));
	std::vector<int64_t> part(YAK_N_COUNTS);
	for (yak_ch_t *s : shards_of(h)) {
		std::fill(part.begin(), part.end(), 0);
		if (yk_ctx_hist(shard_ctx(s), part.data())) fprintf(stderr, "[E::yak_ch_hist] %s\n", yakamd_last_error());
		for (int i = 0; i < YAK_N_COUNTS; ++i) cnt[i] += part[i];
	}
}

void yak_ch_setcnt(yak_ch_t *h, int cnt, int n_thread)        /* reference htab.c:219-235: every stored k-mer gets count `cnt` */
{
	(void)n_thread;
	for (yak_ch_t *s : shards_of(h))
		if (yk_ctx_setcnt(shard_ctx(s), cnt)) fprintf(stderr, "[E::yak_ch_setcnt] %s\n", yakamd_last_error());
}

yak_knt_t *yak_ch_getseq(const yak_ch_t *h, int w, uint32_t *n) /* reference htab.c:353-367 */
{
	assert(h->k < 32 && w < 1 << h->pre);
	if (YK_MULTI((const yak_ch_ext*)h)) { const yak_ch_ext *e = (const yak_ch_ext*)h; return yak_ch_getseq(e->sub[yk_shard_owner(h->pre, e->n_sub, (uint64_t)w)], w, n); }
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

} /* extern "C" */
