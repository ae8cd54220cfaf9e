/*
 * engine_ctx.cpp -- the context of a table in the MI355X counting engine behind yak.h: error text, device count, the stream and event cache,
 * context create and destroy, shard and HPC settings, the host mirror, the scratch buffer and the one-line accessors.  The passes are in
 * engine_pass.cpp (with engine_acc.cpp and engine_count.cpp), the count of a slice in engine_slice.cpp, whole-table operations in engine_table.cpp.
 *
 * State model.  The authoritative copy of a counting table lives in HBM as an exact image of the
 * reference's 1<<pre khashl sets (one arena of 64-bit slots + one "used" bitmap, reference
 * khashl.h:104-109 / htab.c:9-11) together with the blocked bloom filters (bbf.c).  The slot arrays
 * reachable from the caller-visible yak_ch_t are a host mirror that is refreshed on demand
 * (yak_ch_dump, yak_ch_get, ...).  There is NO CPU counting path: without a usable GPU every
 * entry point fails loudly.
 *
 * A counting pass (reference count.c:147-166) is: pass_begin, feed..., pass_end.  For
 * create_new = 1 the pass accumulates, per distinct hashed k-mer, its count and the stream times
 * of its first and second occurrence (kernels.hip K1/K3), applies the order-exact bloom gate
 * (K2), and pass_end turns that into the reference's slot layout (select -> sort -> K5 replay).
 *
 * Ownership.  Every device buffer of a context is a DevBuf / DevVec member of yakamd_ctx (engine_int.h, dev_buf.h) and goes with it; the two
 * groups that go earlier are sub-structs, reset as a whole: what a pass holds (pass_free) and the retained input (retained_drop).  Every pool
 * free happens with the context's device current: yk_ctx_destroy selects it before the members are destroyed.
 */
#include "engine_int.h"
#include <atomic>

static thread_local char g_err[512] = "";

extern "C" const char *yakamd_last_error(void) { return g_err; }
int yk_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); fprintf(stderr, "[E::yak_amd] %s\n", g_err); return -1; }

extern "C" int yakamd_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	int ok = 0;
	for (int i = 0; i < n; ++i) {
		hipDeviceProp_t pr;
		if (hipGetDeviceProperties(&pr, i) == hipSuccess && strncmp(pr.gcnArchName, "gfx950", 6) == 0) ++ok;
	}
	return ok;
}

extern "C" yakamd_ctx *yakamd_ctx_of(yak_ch_t *h) { return ctx_of(h); }

BloomView bloom_view(yakamd_ctx *c)
{
	BloomView b;
	b.bits32 = c->d_bf; b.nb = c->nb; b.n_hash = c->n_hash;
	const int nd = c->n_hash < 512 ? c->n_hash : 512;
	b.mw = (nd + 63) / 64; if (b.mw < 1) b.mw = 1;
	return b;
}

/* give a never-written bloom array its zeros (paths that read-modify-write it in place) */
int bloom_materialise(yakamd_ctx *c)
{
	if (c->d_bf && c->bf_virgin) {
		HIPCK(hipMemsetAsync(c->d_bf, 0, c->bf_words * 4, c->st));
		c->bf_virgin = false;
	}
	return 0;
}

/* install a fresh, empty image: every sub-table has capacity 0 but owns 32 arena slots */
static int img_reset_empty(yakamd_ctx *c)
{
	const int P = c->P;
	c->d_keys.reset(); c->d_used.reset(); c->d_delta.reset();
	c->n_slots = (u64)P * 32;
	if (c->d_keys.alloc(c->n_slots) || c->d_used.alloc(c->n_slots / 32)) return -1;   /* d_delta: see delta_ensure */
	HIPCK(hipMemsetAsync(c->d_keys, 0xff, c->n_slots * 8, c->st));
	HIPCK(hipMemsetAsync(c->d_used, 0, c->n_slots / 8, c->st));
	c->h_bits.assign(P, YK_NOCAP); c->h_count.assign(P, 0); c->h_off.resize(P);
	for (int p = 0; p < P; ++p) c->h_off[p] = (u64)p * 32;
	HIPCK(hipMemcpyAsync(c->d_bits, c->h_bits.data(), P * 4, hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemcpyAsync(c->d_off, c->h_off.data(), P * 8, hipMemcpyHostToDevice, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	c->img_keys_total = 0;
	c->host_valid = false;
	return 0;
}

/* the per-slot pending increments (4 bytes per slot of the arena: 8.6 GB beside a 2 Gb assembly's table) exist only while a pass can add to the
 * counts of stored keys -- a count-existing pass, or puts of the accumulator path on a table that holds keys -- and are folded in and released when
 * that pass ends */
int delta_ensure(yakamd_ctx *c)
{
	if (c->d_delta) return 0;
	if (c->d_delta.alloc(c->n_slots)) return -1;
	HIPCK(hipMemsetAsync(c->d_delta, 0, c->n_slots * 4, c->st));
	return 0;
}

/* events and streams are kept and handed out again: creating and destroying them costs a runtime call each (a millisecond per stream with the
 * ROCm 7.2 runtime), and a counting job of 60 ms opens a table per step and times a dozen stages */
struct HipCache {
	std::mutex mu;
	std::vector<hipEvent_t> ev[16];
	std::vector<hipStream_t> st[16];
};
static HipCache g_hc;
hipEvent_t yk_ev_get()
{
	int d = 0; (void)hipGetDevice(&d); d &= 15;
	{ std::lock_guard<std::mutex> lk(g_hc.mu); if (!g_hc.ev[d].empty()) { hipEvent_t e = g_hc.ev[d].back(); g_hc.ev[d].pop_back(); return e; } }
	hipEvent_t e = 0; (void)hipEventCreate(&e); return e;
}
void yk_ev_put(hipEvent_t e) { int d = 0; (void)hipGetDevice(&d); d &= 15; std::lock_guard<std::mutex> lk(g_hc.mu); g_hc.ev[d].push_back(e); }
hipStream_t yk_stream_get(int dev)
{
	{ std::lock_guard<std::mutex> lk(g_hc.mu); auto &v = g_hc.st[dev & 15]; if (!v.empty()) { hipStream_t x = v.back(); v.pop_back(); return x; } }
	hipStream_t x = 0;
	return hipStreamCreate(&x) == hipSuccess ? x : 0;
}
void yk_stream_put(int dev, hipStream_t x) { (void)hipStreamSynchronize(x); std::lock_guard<std::mutex> lk(g_hc.mu); g_hc.st[dev & 15].push_back(x); }

static thread_local int g_next_device = -1;          /* device of the next context created on this thread (multi-GPU tables) */
void yk_ctx_next_device(int dev) { g_next_device = dev; }

yakamd_ctx *yk_ctx_create(int k, int pre, int n_hash, int n_shift)
{
	if (yakamd_device_count() < 1) { fail("no gfx950 GPU visible: the counting engine has no CPU fallback"); return 0; }
	yakamd_ctx *c = new yakamd_ctx();
	c->k = k; c->pre = pre; c->P = 1 << pre; c->phi = c->P;
	c->nb_bits = (int)std::min<int64_t>(pre, env_i64("YAKAMD_PART_BITS", 13));
	if (c->nb_bits < 3) c->nb_bits = 3;
	if (c->nb_bits > 13) c->nb_bits = 13;
	c->dev = (int)env_i64("YAKAMD_DEVICE", 0);
	{
		const char *lr = getenv("LOCAL_RANK");
		int nd = 0;
		if (!getenv("YAKAMD_DEVICE") && lr && hipGetDeviceCount(&nd) == hipSuccess && nd > 0) c->dev = atoi(lr) % nd;
	}
	if (g_next_device >= 0) { c->dev = g_next_device; g_next_device = -1; }
	c->st.dev = c->dev;
	if (hipSetDevice(c->dev) != hipSuccess || (c->st.s = yk_stream_get(c->dev)) == 0) { fail("cannot open device %d", c->dev); delete c; return 0; }
	if (n_hash > 0 && n_shift > pre) {                       /* reference htab.c:23-27 */
		c->n_hash = n_hash; c->bf_shift = n_shift; c->nb = n_shift - pre;
		c->has_bloom = c->nb >= 9 && c->nb + 9 <= 64;        /* yak_bf_init returns NULL otherwise (bbf.c:9) */
	}
	if (c->d_bits.alloc(c->P) || c->d_off.alloc(c->P) || c->d_counters.alloc(YKC_N) ||
	    c->d_lastput.alloc(c->P) || c->d_lpbatch.alloc(c->P) || c->d_missing.alloc((c->P + 31) / 32 + 1) ||
	    c->d_nmissing.alloc(1) || img_reset_empty(c)) { yk_ctx_destroy(c); return 0; }
	if (c->has_bloom) {
		c->bf_words = (size_t)c->P << (c->nb - 5);
		if (c->d_bf.alloc(c->bf_words)) { yk_ctx_destroy(c); return 0; }
		c->bf_virgin = true;               /* zero-filled lazily: the first counting pass writes every block anyway */
		c->multi_bits = (int)env_i64("YAKAMD_MULTI_BITS", 30);
		if (c->multi_bits < 10) c->multi_bits = 10;
		if (c->d_multi.alloc((size_t)1 << (c->multi_bits - 5))) { yk_ctx_destroy(c); return 0; }
		hipMemsetAsync(c->d_multi, 0, (size_t)1 << (c->multi_bits - 3), c->st);
		hipStreamSynchronize(c->st);
	}
	return c;
}

/* a filter whose write-back was skipped becomes real before the records it can be rebuilt from go away */
static void bloom_undefer(yakamd_ctx *c)
{
	if (!c->bf_deferred) return;
	c->bf_deferred = false;
	const Ret2 &r = c->ret.l2;
	if (!c->d_bf || !r.valid) return;
	(void)hipMemsetAsync(c->d_bf, 0, c->bf_words * 4, c->st);
	yk_launch_bf_rebuild(r.fp, r.sbstart, r.r2, c->d_bf, c->st);
	(void)hipStreamSynchronize(c->st);
	if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] the filter of the last pass rebuilt from its retained records (its write-back had been skipped)\n");
}

void retained_drop(yakamd_ctx *c)
{
	bloom_undefer(c);
	c->ret = RetainedInput();
	c->src_set = false;
}

void pass_free(yakamd_ctx *c)
{
	c->pass = PassBufs();
	c->in_pass = false;
}

/* the members free what the context holds, with its device current; a deferred filter is not rebuilt (nobody will read it) */
void yk_ctx_destroy(yakamd_ctx *c)
{
	if (!c) return;
	hipSetDevice(c->dev);
	delete c;
}

int yk_ctx_destroy_bf(yakamd_ctx *c)
{
	hipSetDevice(c->dev);
	c->d_bf.reset(); c->d_multi.reset();
	c->has_bloom = false; c->bf_deferred = false;
	return 0;
}

extern "C" int yakamd_set_shard(yak_ch_t *h, int lo, int hi)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || lo < 0 || hi > c->P || lo >= hi) return fail("bad shard range");
	if (c->in_pass) return fail("shard change inside a pass");
	if (c->has_bloom && !c->bf_virgin && (lo != c->plo || hi != c->phi))
		return fail("the shard cannot move once its bloom filters have been written (only the shard's part is initialised)");
	c->plo = lo; c->phi = hi;
	return 0;
}

/* the table's space.  The mark is the table's, not the file's: dump and restore do not carry it */
extern "C" int yakamd_ch_set_hpc(yak_ch_t *h, int on)
{
	const yak_ch_ext *e = (const yak_ch_ext*)h;
	if (!h || e->magic != EXT_MAGIC) return fail("not an engine table");
	if (e->n_sub > 1) {                                        /* sharded over ranks: every shard, or none */
		for (int r = 0; r < e->n_sub; ++r) { yakamd_ctx *c = ctx_of(e->sub[r]); if (!c) return fail("not an engine table"); if (c->in_pass) return fail("yakamd_ch_set_hpc inside an open pass"); }
		for (int r = 0; r < e->n_sub; ++r) ctx_of(e->sub[r])->hpc = on != 0;
		return 0;
	}
	yakamd_ctx *c = e->ctx;
	if (!c) return fail("not an engine table");
	if (c->in_pass) return fail("yakamd_ch_set_hpc inside an open pass");
	c->hpc = on != 0;
	return 0;
}
extern "C" int yakamd_ch_hpc(const yak_ch_t *h)
{
	const yak_ch_ext *e = (const yak_ch_ext*)h;
	if (!h || e->magic != EXT_MAGIC) return 0;
	const yakamd_ctx *c = e->n_sub > 1 ? ctx_of(e->sub[0]) : e->ctx;
	return c && c->hpc;
}

/* yak_count(): the file whose records are retained (device, inode, size, mtime) and its sequence count, for the log line */
void yk_ctx_set_source(yakamd_ctx *c, const uint64_t id[4], int64_t n_seq) { memcpy(c->src_id, id, 32); c->src_id[4] = (u64)n_seq; c->src_set = true; }
/* (The retained key lists name the keys pass 1 put into the table.  Nothing can add a key between the two passes without a create_new pass -- which
 * drops what is retained (yakamd_pass_begin) -- and yak_ch_inc / setcnt / clear only touch counts; keys removed in between (shrink, subtract) are
 * simply not found by the count) */
bool yk_ctx_same_source(yakamd_ctx *c, const uint64_t id[4], int64_t *n_seq)
{
	if (!c->src_set || (c->ret.l1.empty() && !c->ret.l2.valid) || c->retain_broken || memcmp(c->src_id, id, 32) != 0) return false;
	*n_seq = (int64_t)c->src_id[4];
	return true;
}

extern "C" void yakamd_debug_counters(uint32_t *out4)
{
	out4[0] = out4[1] = 0;
	yk_par_counters(&out4[0], &out4[1]);
	{   /* the tally's events count what has been added since the call before */
		static std::atomic<uint32_t> seen_ok{0}, seen_fail{0};
		yk_event(YKE_PAR_OK, (uint32_t)(out4[0] - seen_ok.exchange(out4[0])));
		yk_event(YKE_PAR_FAIL, (uint32_t)(out4[1] - seen_fail.exchange(out4[1])));
	}
	yk_replay_counters(&out4[2], &out4[3]);
}

/* small runtime services for callers that hold no HIP runtime of their own (bench.py's single-GPU mode, the tests): page-locked host memory and
 * "everything queued on the current device is done" */
extern "C" void *yakamd_host_alloc(size_t bytes) { void *p = 0; return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : 0; }
extern "C" void yakamd_host_free(void *p) { if (p) (void)hipHostFree(p); }
extern "C" int yakamd_device_sync(void) { return hipDeviceSynchronize() == hipSuccess ? 0 : fail("hipDeviceSynchronize: %s", hipGetErrorString(hipGetLastError())); }
extern "C" int yakamd_mem_info(size_t *free_bytes, size_t *total_bytes) { return hipMemGetInfo(free_bytes, total_bytes) == hipSuccess ? 0 : -1; }
extern "C" void *yakamd_dev_alloc(size_t bytes) { void *p = 0; return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess ? p : 0; }
extern "C" void yakamd_dev_free(void *p) { if (p) (void)hipFree(p); }
extern "C" int yakamd_memcpy_h2d(void *d, const void *s, size_t n) { return hipMemcpy(d, s, n, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1; }
extern "C" int yakamd_memcpy_d2h(void *d, const void *s, size_t n) { return hipMemcpy(d, s, n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1; }

extern "C" int yakamd_get_stats(yak_ch_t *h, yakamd_stats_t *st)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c) return -1;
	*st = c->st_last;
	return 0;
}

int yk_ctx_in_pass(yakamd_ctx *c) { return c->in_pass; }

void yk_ctx_gate(yakamd_ctx *c, bool on) { c->gate_off = !on; }
void yk_ctx_or_mode(yakamd_ctx *c, int mode) { c->or_mode = mode; }

u64 yk_ctx_keys_total(yakamd_ctx *c) { return c->img_keys_total; }
void yk_ctx_range(yakamd_ctx *c, int *lo, int *hi) { *lo = c->plo; *hi = c->phi; }

/* ------------------------------------------------------------------------------------------
 * host mirror
 * ------------------------------------------------------------------------------------------ */
struct yak_ht_t { uint32_t bits, count; uint32_t *used; uint64_t *keys; };   /* same shape as khashl.h:104-109 */

static std::atomic<int64_t> g_host_syncs{0};
extern "C" int64_t yakamd_host_syncs(void) { return g_host_syncs.load(); }

int yk_ctx_sync_host(yakamd_ctx *c, yak_ch_t *h)
{
	/* yak_ch_get() is called concurrently by the reference's kt_for workers (qv.c:59, triobin.c): the
	 * first callers serialise on the refresh, later ones only read the flag */
	if (__atomic_load_n(&c->host_valid, __ATOMIC_ACQUIRE)) return 0;
	static std::mutex mu;
	std::lock_guard<std::mutex> lk(mu);
	if (c->host_valid) return 0;
	HIPCK(hipSetDevice(c->dev));
	if (yk_image_settle(c)) return -1;
	++g_host_syncs;
	if (c->hm_slots < c->n_slots) {
		c->hm_keys.reset(); c->hm_used.reset(); c->hm_slots = 0;
		void *hk = 0, *hu = 0;
		HIPCK(hipHostMalloc(&hk, c->n_slots * 8));
		c->hm_keys.reset((u64*)hk);
		HIPCK(hipHostMalloc(&hu, c->n_slots / 8));
		c->hm_used.reset((u32*)hu);
		c->hm_slots = c->n_slots;
	}
	HIPCK(hipMemcpyAsync(c->hm_keys.get(), c->d_keys, c->n_slots * 8, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipMemcpyAsync(c->hm_used.get(), c->d_used, c->n_slots / 8, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	if (!c->hts) c->hts.reset((yak_ht_t*)calloc(c->P, sizeof(yak_ht_t)));
	for (int p = 0; p < c->P; ++p) {
		yak_ht_t *g = &c->hts[p];
		const bool has = c->h_bits[p] != YK_NOCAP;
		g->bits = has ? c->h_bits[p] : 0;
		g->count = c->h_count[p];
		g->keys = has ? (uint64_t*)(c->hm_keys.get() + c->h_off[p]) : 0;
		g->used = c->hm_used.get() + c->h_off[p] / 32;
		if (h) h->h[p].h = g;
	}
	__atomic_store_n(&c->host_valid, true, __ATOMIC_RELEASE);
	return 0;
}

extern "C" int yakamd_sync_host(yak_ch_t *h)
{
	yakamd_ctx *c = ctx_of(h);
	return c ? yk_ctx_sync_host(c, h) : fail("not an engine table");
}

extern "C" int yakamd_subtable(yak_ch_t *h, int i, uint32_t *capacity, uint32_t *size)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || i < 0 || i >= c->P) return -1;
	*capacity = c->h_bits[i] == YK_NOCAP ? 0 : 1u << c->h_bits[i];
	*size = c->h_count[i];
	return 0;
}

u64 yk_ctx_list_time(yakamd_ctx *c, u64 n) { const u64 t = c->list_t; c->list_t += n; return t; }
void yk_ctx_lock(yakamd_ctx *c) { c->api_mu.lock(); }
void yk_ctx_unlock(yakamd_ctx *c) { c->api_mu.unlock(); }

/* a device buffer of at least `bytes` that lives as long as the context (small repeated calls: yak_ch_insert_list) */
void *yk_ctx_scratch(yakamd_ctx *c, size_t bytes)
{
	if (bytes <= c->scratch.cap()) return c->scratch.get();
	if (hipSetDevice(c->dev) != hipSuccess) return 0;
	return c->scratch.reserve(std::max<size_t>(bytes + bytes / 2, 1 << 16)) ? 0 : c->scratch.get();
}

int yk_ctx_device(yakamd_ctx *c) { return c->dev; }
hipStream_t yk_ctx_stream(yakamd_ctx *c) { return c->st; }
const yak_ht_t *yk_ctx_ht(yakamd_ctx *c, int p) { return c->hts ? &c->hts[p] : 0; }
