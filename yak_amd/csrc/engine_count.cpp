/* engine_count.cpp -- counting into the keys a table already holds (a create_new = 0 pass).  count_records takes a batch by the one plan of
 * count_plan.h: key-owning ranges, home-slot ranges, LDS ranks or device atomics; yakamd_count_hashes_dev / yakamd_count_partitioned_dev feed it
 * bare hashes, and yakamd_count_retained counts the input of the pass before without reading it again. */
#include "engine_int.h"
#include "count_plan.h"

/* the plan's settings: the one place that reads them */
static CountKnobs count_knobs()
{
	CountKnobs kn;
	kn.own = env_i64("YAKAMD_COUNT_OWN", 1) != 0;
	kn.own_lds = (size_t)env_i64("YAKAMD_OWN_LDS", 156000);
	kn.own_maxrb = (int)env_i64("YAKAMD_OWN_MAXRB", 4);
	kn.lds_ranks = env_i64("YAKAMD_COUNT_LDS", 1) != 0;
	kn.ranges = env_i64("YAKAMD_COUNT_RNG", 1) != 0;
	kn.rng_log = yk_rng_log();                                   /* YAKAMD_RNG_LOG, as the kernels' launch wrappers read it */
	kn.ytag = env_i64("YAKAMD_YTAG", 1) != 0;
	return kn;
}
static CountTable count_table(const yakamd_ctx *c) { return CountTable{ c->nb_bits, c->pre, c->k, c->plo, c->phi, c->h_bits.data(), c->h_count.data() }; }
static CountPlan plan_of(const yakamd_ctx *c, RecFmt fmt, bool grouped) { return count_plan(count_table(c), count_knobs(), fmt, grouped); }
RecFmt count_pass_fmt(const yakamd_ctx *c) { return count_consumed_fmt(count_table(c), count_knobs()); }

/* The overflow list of the two-sweep count kernels (k_img_count_own, k_img_count_rng).  Sweep 0 counts what its workgroups own and lists the
 * instances whose key lies beyond their range: n[0] of them, n[1] != 0 when the list ran out of room.  Then either a second sweep counts every
 * boundary-crossing instance itself, or k_img_count_h counts the listed ones */
struct XList {
	DevBuf<u64> list; DevBuf<u32> n; u32 cap = 0;
	int alloc(hipStream_t st)
	{
		cap = (u32)std::min<int64_t>(env_i64("YAKAMD_XLIST_CAP", 1 << 22), 1 << 22);   /* the knob is for tests */
		if (list.alloc((size_t)1 << 22) || n.alloc(2)) return -1;
		HIPCK(hipMemsetAsync(n, 0, 8, st));
		return 0;
	}
	/* sweep(cross) launches the kernel, != 0: it could not be configured (`refusal` says so); `what` opens the verbose line */
	template <class Sweep> int run(yakamd_ctx *c, const ImgView &img, Sweep sweep, YkEvent event, const char *refusal, const char *what)
	{
		if (sweep(0)) return fail("%s", refusal);
		u32 xn[2] = { 0, 0 };
		HIPCK(hipMemcpyAsync(xn, n, 8, hipMemcpyDeviceToHost, c->st));
		HIPCK(hipStreamSynchronize(c->st));
		if (xn[1]) { yk_event(event); sweep(1); }                /* list too small: second sweep */
		else if (xn[0]) yk_launch_img_count_h(list, (int64_t)xn[0], img, c->st);
		if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] %s, %u boundary-crossing instances%s\n", what, xn[0], xn[1] ? " (list overflow: second sweep)" : "");
		HIPCK(hipStreamSynchronize(c->st));
		return 0;
	}
};

/* records = 8-byte hashes grouped by prefix (d_bstart), tables beyond the LDS kernel: level-2 partition by home-slot range (k_hpart2) + one
 * workgroup per range (k_img_count_rng) */
static int count_by_ranges(yakamd_ctx *c, const CountPlan &pl, const void *d_hash, int64_t n_rec, const u64 *d_bstart)
{
	const int P = c->P, rb = pl.rb;
	const size_t NB = (size_t)1 << c->nb_bits, S2 = (size_t)1 << rb, n_sb = (size_t)P << rb;
	std::vector<u64> bst(NB + 1);
	HIPCK(hipMemcpyAsync(bst.data(), d_bstart, (NB + 1) * 8, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	ChunkTable t;
	chunk_runs(t, d_hash, yk_rec_bytes(YK_FMT_HASH), bst.data(), P, (u64)yk_hpart2_chunk());
	std::vector<u64> bbase(P + 1, 0);
	for (int p = 0; p < P; ++p) bbase[p + 1] = bbase[p] + (bst[p + 1] - bst[p]);
	DevBuf<u64> d_bbase, d_sbstart, d_h2; DevBuf<u32> d_rows2; XList x;
	if (t.upload(c->st) || d_bbase.alloc(P + 1) || d_rows2.alloc((t.h.size() + 1) * S2) ||
	    d_sbstart.alloc(n_sb + 1) || d_h2.alloc((size_t)n_rec) || x.alloc(c->st)) return -1;
	HIPCK(hipMemcpyAsync(d_bbase, bbase.data(), (P + 1) * 8, hipMemcpyHostToDevice, c->st));
	const ImgView img = img_view(c);
	yk_launch_hpart2(t.d, (int)t.h.size(), t.d_first, d_bbase, img, rb, P, d_rows2, d_sbstart, d_h2, c->st);
	char what[64];
	snprintf(what, sizeof(what), "range count: 2^%d ranges per sub-table", rb);
	return x.run(c, img, [&](int cross) { return yk_launch_img_count_rng(d_h2, cross, d_sbstart, img, c->plo, c->phi, rb, pl.max_len, x.list, x.n, x.cap, c->st); },
	             YKE_RNG_SWEEPS, "range count kernel could not be configured", what);
}

/* records grouped by prefix: one workgroup per slot range with the range's keys in LDS (k_img_count_own) */
static int count_own(yakamd_ctx *c, const CountPlan &pl, const void *d_rec, RecFmt fmt, const u64 *d_bstart)
{
	XList x;
	if (x.alloc(c->st)) return -1;
	const ImgView img = img_view(c);
	char what[192];
	snprintf(what, sizeof(what), "key-owning count: 2^%d slots per range (up to 2^%d ranges per sub-table), %u keys of LDS room, %zu B of LDS", pl.rng_log, pl.rb, pl.kmax, pl.lds);
	return x.run(c, img, [&](int cross) { return yk_launch_img_count_own(d_rec, fmt, cross, d_bstart, img, c->plo, c->phi, pl.rb, pl.rng_log, pl.kmax, pl.lds, x.list, x.n, x.cap, c->st); },
	             YKE_OWN_SWEEPS, "key-owning count kernel could not be configured", what);
}

/* every sub-table small enough for LDS rank counters: exclusive-ownership counting, no global atomics (k_img_count_lds).  1: the launch wrapper
 * could not be configured at run time, the caller counts with device atomics */
static int count_lds_ranks(yakamd_ctx *c, const CountPlan &pl, const void *d_rec, RecFmt fmt, const u64 *d_bstart)
{
	DevBuf<u64> d_ck;
	if (d_ck.alloc((size_t)(c->phi - c->plo) * pl.ck_stride)) return -1;
	const int r = yk_launch_img_count_lds(d_rec, fmt, d_bstart, img_view(c), c->plo, c->phi, pl.lds, d_ck, pl.ck_stride, c->st);
	HIPCK(hipStreamSynchronize(c->st));
	return r ? 1 : 0;
}

int count_records(yakamd_ctx *c, const void *d_rec, RecFmt fmt, int64_t n_rec, const u64 *d_bstart)
{
	const ImgView img = img_view(c);
	c->delta_dirty = true;
	yk_image_touched(c);
	EvTimer tm(c->st);
	const CountPlan pl = plan_of(c, fmt, d_bstart != 0);
	int r = 0;
	switch (pl.path) {
	case YK_COUNT_NOTHING: break;
	case YK_COUNT_REFUSED: r = fail("the table changed between the extraction and the count of a pass"); break;
	case YK_COUNT_OWN: r = count_own(c, pl, d_rec, fmt, d_bstart); break;
	case YK_COUNT_RANGES: r = count_by_ranges(c, pl, d_rec, n_rec, d_bstart); break;
	case YK_COUNT_LDS:
		r = count_lds_ranks(c, pl, d_rec, fmt, d_bstart);
		if (r != 1) break;
		r = 0;
		[[fallthrough]];
	case YK_COUNT_ATOMICS:
		if (fmt == YK_FMT_HASH) yk_launch_img_count_h((const u64*)d_rec, n_rec, img, c->st);
		else yk_launch_img_count((const Rec*)d_rec, n_rec, img, c->st);
	}
	insert_ms(c, tm);
	return r;
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

/* the end of a path of yakamd_count_retained that counted: the pass's statistics and events, the records released.  n_inst: instances the path
 * counted beyond what consume_records has booked; text: the verbose line; failed: what to report when a launch of the path was refused (0: the
 * path has checked its own calls) */
static int retained_done(yakamd_ctx *c, int path, YkEvent event, u64 n_inst, const char *text, const char *failed)
{
	const bool bad = failed && hipGetLastError() != hipSuccess;
	c->st_cur.n_instances += (int64_t)n_inst;
	c->st_cur.pass2_path = path; yk_event(event);
	if (text && env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] count pass: %s\n", text);
	retained_drop(c);
	return bad ? fail("%s", failed) : 0;
}

/* inside an open create_new = 0 pass: count every instance of the retained records (k_img_count_own reads the tagged level-1 records
 * as they are).  0 = counted, the records are released; 1 = nothing usable was retained (the caller feeds the input again); -1 = error */
extern "C" int yakamd_count_retained(yak_ch_t *h)
{
	yakamd_ctx *c = ctx_of(h);
	if (!c || !c->in_pass || c->create_new) return fail("yakamd_count_retained needs an open create_new = 0 pass");
	HIPCK(hipSetDevice(c->dev));
	const Ret2 &l2 = c->ret.l2;
	char text[160];
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
		snprintf(text, sizeof(text), "the counts of the pass before applied (%llu keys, %.2f ms%s)", (unsigned long long)l2.n_keys, ms, bump ? "; with the pending clear, in one sweep" : "");
		return retained_done(c, 1, YKE_PASS2_FUSED, l2.n_total, text, "applying the counts of the pass before failed");
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
		snprintf(text, sizeof(text), "k_cnt2 over the retained sub-bucket records (%llu keys, %.2f ms)", (unsigned long long)l2.n_keys, ms);
		return retained_done(c, 2, YKE_PASS2_RECOUNT, l2.n_total, text, "the count over the retained sub-bucket records failed");
	}
	/* the level-1 records, grouped by prefix.  Tables beyond the key-owning count kernel: the general count path wants plain hashes */
	if (c->ret.l1.empty() || c->retain_broken || plan_of(c, YK_FMT_TAGGED, true).path == YK_COUNT_REFUSED) { yk_event(YKE_PASS2_NONE); retained_drop(c); return 1; }
	const size_t NB = (size_t)1 << c->nb_bits;
	if (part_reserve(c, 1)) return -1;
	int r = 0;
	for (auto &b : c->ret.l1) {
		if (r) break;
		if (hipMemcpyAsync(c->d_bstart, b.bstart.data(), (NB + 1) * 8, hipMemcpyHostToDevice, c->st) != hipSuccess) { r = fail("memcpy"); break; }
		r = consume_records(c, b.rec.get(), YK_FMT_TAGGED, (int64_t)b.n, 0, 0, 0, c->d_bstart);
		if (!r && hipStreamSynchronize(c->st) != hipSuccess) r = fail("count of the retained records failed");
	}
	if (r) { retained_drop(c); return -1; }
	return retained_done(c, 3, YKE_PASS2_PREFIX, 0, 0, 0);
}
