/* engine_slice.cpp -- the exclusive-ownership path of a create pass: the batches of a pass are kept (fast_admit, fast_keep) and counted together
 * as a slice (fast_finish: its stages below, handing each other a Slice) at the end of the pass, or earlier when the budget says so
 * (fast_flush_slice); a pass that cannot stay on the path hands what it kept to the accumulator path of engine_acc.cpp (fast_abandon). */
#include "engine_int.h"
#include "seg_sort_tile.h"

/* the runs [start[q], start[q + 1]) of buckets q < n_buckets, records of `stride` bytes from `base`, cut into items of at most `len` records */
void chunk_runs(ChunkTable &t, const void *base, size_t stride, const u64 *start, size_t n_buckets, u64 len)
{
	t.h.clear();
	t.first.assign(n_buckets + 1, 0);
	for (size_t q = 0; q < n_buckets; ++q) {
		t.first[q] = (u32)t.h.size();
		for (u64 o = start[q]; o < start[q + 1]; o += len) {
			Chunk2 ch = {};
			ch.rec = (const Rec*)((const char*)base + o * stride); ch.n = (u32)std::min<u64>(len, start[q + 1] - o); ch.bucket = (u32)q;
			t.h.push_back(ch);
		}
		if (t.h.size() > t.first[q]) t.h.back().spare = 1;
	}
	t.first[n_buckets] = (u32)t.h.size();
}

/* ---- pass_end of the fast path (fast_finish): plan -> level-2 partition (the retain decision between its sweeps) -> exclusive LDS counting
 * (+ bloom gate) -> gather of the selected keys -> per sub-table sort by insertion time -> exact layout replay ---- */

/* what the stages of fast_finish hand each other: every device buffer stays here until a stage frees it or hands it to the context */
struct Slice {
	FastParams fp;
	u64 n_total = 0, sort_tmax = 0, budget = 0;
	RecFmt fmt_in = YK_FMT_POS; int s2 = 0, s2a = 0, s2b = 0;   /* fmt_in: of every kept batch, YK_FMT_POS or YK_FMT_TAGGED */
	bool three = false, nowb_plan = false, keep2 = false;
	size_t n_sb = 0;
	DevBuf<u64> sbstart; DevBuf<u32> segcur, ovf2; DevBuf<Rec> r2;   /* the level-2 partition: the sub-buckets' starts and records */
	int r2_alloc() { return r2.alloc(fp.rec8_out ? (n_total + 1) / 2 : n_total); }   /* (level 2's own 8-byte records: FastParams.rec8_out) */
	DevBuf<u64> lo_kc, lo_T; DevBuf<u32> lo_nsel, lo_lp, lo_nd; DevBuf<unsigned short> lo_c2;   /* k_lc2's output (LcOut) */
	DevBuf<u32> ndist;
	std::vector<u32> m; std::vector<u64> ro; u64 n_sel = 0;        /* the gather: keys per sub-table (m), their offsets (ro) */
	DevBuf<u64> segbase, koff; DevBuf<u32> kc2;
	/* the sort: {key, time} pairs as gathered (kt), keys and times in two buffer pairs, the current one cur */
	int tbits = 0, ts_b = 0, ts_w = 0, ts_j = 0; bool tsort = false;
	DevBuf<u64> kc[2], tt[2]; int cur = 0;
	DevBuf<Rec> kt; DevBuf<u32> tsfail;
	bool laps; double lap_t;   /* YAKAMD_VERBOSE > 1: wall-clock laps of the stages (each behind a stream synchronise: allocation stalls show up where they happen) */

	Slice() : laps(env_i64("YAKAMD_VERBOSE", 0) > 1), lap_t(now_ms()) {}
	LcOut lo() const { LcOut o; o.kc = lo_kc; o.T = lo_T; o.nsel = lo_nsel; o.lp = lo_lp; o.nd = lo_nd; o.c2 = lo_c2; return o; }
	void lap(yakamd_ctx *c, const char *what)
	{
		if (!laps) return;
		(void)hipStreamSynchronize(c->st);
		const double t = now_ms();
		size_t fr = 0, tt_ = 0;
		(void)hipMemGetInfo(&fr, &tt_);
		fprintf(stderr, "[yak_amd] slice stage %-28s %9.2f ms   (device memory in use %.1f GB, of it idle in the pool %.1f GB)\n", what, t - lap_t, (double)(tt_ - fr) / 1e9, (double)yk_pool_cached_bytes() / 1e9);
		lap_t = now_ms();
	}
};

/* the plan of the slice: sub-buckets per sub-table (s2, in one or two sweeps), the filter-less plan (nowb_plan), the FastParams they imply */
static int slice_plan(yakamd_ctx *c, Slice &s, bool last)
{
	const int P = c->P;
	for (auto &k : c->pass.kept) s.n_total += k.n;
	s.fmt_in = c->pass.kept.empty() ? YK_FMT_POS : c->pass.kept.front().fmt;
	s.sort_tmax = c->t_end;
	FastParams &fp = s.fp;
	fp.pre = c->pre; fp.k = c->k; fp.bloom_mode = c->bloom_mode; fp.nb = c->nb; fp.n_hash = c->n_hash;
	fp.img_nonempty = c->img_keys_total > 0; fp.plo = c->plo; fp.phi = c->phi; fp.t_pass0 = c->t_pass0;
	fp.dbg = (int)env_i64("YAKAMD_DBG", 0);
	fp.or_mode = c->or_mode;
	fp.bf_nowb = 0;
	const u64 n_total = s.n_total;
	/* mean sub-bucket <= ~600 instances: even if all are distinct the 1024-slot LDS table holds them.  With a filter the input is reads with
	 * coverage (a filtered count of all-distinct k-mers keeps nothing): three times as many instances per sub-bucket still leave the distinct
	 * k-mers far below the table's 624 (30 x coverage: ~100 distinct per 560 instances), and 2048 sub-buckets per sub-table are what the
	 * level-2 scatter takes in one sweep -- 30 M reads: 13 -> 11 bits, its partition 124 -> ~40 ms.  A sub-bucket that does overflow goes to
	 * the tiers behind k_lc2, as always */
	const u64 per_sb = (u64)yk_lc2_per_sb(c->bloom_mode);         /* 1800 with a filter; without one 1200 (k_lc2's 2048-slot table) or 600 (the older tiers) */
	/* the largest stream of one sub-table in this slice: decides whether the level-2 records take 8 bytes (below), which the plan needs */
	u64 np_max = 0;
	for (int p = 0; p < P; ++p) { u64 np = 0; for (auto &k : c->pass.kept) np += k.bstart[p + 1] - k.bstart[p]; np_max = std::max(np_max, np); }
	/* Known before the partition: will every record of this pass stay on the device for the count pass over the same input (keep2 below) while
	 * the filter is still untouched?  Then nobody reads the filter's bits before the records can rebuild them (bf_nowb), k_lc2 needs no stage of
	 * the filter in LDS, and a sub-bucket may own 256 blocks instead of 128: half as many, twice as large */
	const int64_t cap_gb = env_i64("YAKAMD_RETAIN_GB", -1);   /* the budget of the records kept for that pass (slice_retain): else an eighth of the device */
	size_t fr = 0, tot = 0;
	s.budget = cap_gb >= 0 ? (u64)cap_gb << 30 : hipMemGetInfo(&fr, &tot) == hipSuccess ? tot / 8 : 0;
	bool &nowb_plan = s.nowb_plan;
	nowb_plan = c->bloom_mode && c->bf_virgin && last && c->n_slices == 0 && c->img_keys_total == 0 && c->retain_on && !c->retain_broken && s.fmt_in == YK_FMT_TAGGED &&
	            !c->or_mode && c->ret.l1.empty() && c->ret.l1_bytes + n_total * yk_rec_bytes(YK_FMT_TAGGED) <= s.budget && c->n_hash <= 32 &&
	            env_i64("YAKAMD_RETAIN2", 1) != 0 && env_i64("YAKAMD_BF_DEFER", 1) != 0 && env_i64("YAKAMD_LC2", 1) != 0 && env_i64("YAKAMD_LC2_NOSTAGE", 1) != 0;
	for (auto &k : c->pass.kept) nowb_plan = nowb_plan && k.own;
	/* one sweep of the level-2 scatter takes up to 2^11 sub-buckets (2^13 in sweeps over the chunk); beyond that -- the share of an N-GPU job's rank:
	 * 128 sub-tables of 69 M instances each -- the partition takes two sweeps (p3): the high bits first into {hash, rank} records, then 2^p3_low
	 * sub-buckets inside every group.  2^18 sub-buckets per sub-table bound the per-sub-bucket arrays */
	const int p3_min = (int)env_i64("YAKAMD_P3_MIN", 13), p3_low = (int)std::min<int64_t>(11, std::max<int64_t>(1, env_i64("YAKAMD_P3_LOW", 11)));
	int &s2 = s.s2, &s2a = s.s2a, &s2b = s.s2b;
	bool &three = s.three;
	for (int attempt = 0; attempt < 2; ++attempt) {
		const int lb_max = nowb_plan ? 8 : 7;                      /* log2 blocks a sub-bucket may own: k_lc2 stages at most 128; without a stage its table gives every block >= 4 home slots */
		s2 = n_total ? ceil_log2_u64((n_total / (u64)(c->phi - c->plo) + per_sb - 1) / per_sb) : 0;
		if (c->bloom_mode && s2 < c->nb - 9 - lb_max && n_total / (u64)(c->phi - c->plo) > 600) s2 = c->nb - 9 - lb_max;
		s2 = (int)env_i64("YAKAMD_S2_BITS", s2);
		if (s2 > 18) s2 = 18;
		if (s2 < 0) s2 = 0;
		if (c->bloom_mode) {
			if (s2 > c->nb - 9) s2 = c->nb - 9;              /* a sub-bucket owns whole 512-bit blocks ... */
			if (s2 < c->nb - 9 - 20) s2 = c->nb - 9 - 20;    /* ... and at most 2^20 of them (sort-key packing) */
		}
		three = s2 > p3_min;
		if (!three && s2 > 13) s2 = 13;
		s2a = three ? std::min(11, std::max(std::min(4, s2 - 1), s2 - p3_low)) : 0; s2b = s2 - s2a;   /* the first sweep keeps >= 16 groups: the write-combining scatter wants >= 4 bits */
		/* the plan without a filter stage falls when the pass cannot keep its level-2 records after all (16-byte records are not kept; ranges beyond 256 blocks
		 * go to the tier behind k_lc2).  s2 was sized for 256 blocks per sub-bucket then: it is chosen again for the 128 a stage holds (the
		 * first choice stayed, k_lc2 refused the 256-block ranges and the whole pass went through the global-scratch tier) */
		if (nowb_plan && c->bloom_mode && (YK_R8_TAG_BITS + s2 >= 64 || np_max >= (1ull << (YK_R8_TAG_BITS + s2)) || env_i64("YAKAMD_REC8_OUT", 1) == 0 || c->nb - 9 - s2 > 8 || c->nb - 9 - s2 < 0)) { nowb_plan = false; continue; }
		break;
	}
	if (three && s2b > 13) return fail("level-2 partition: 2^%d sub-buckets per sub-table cannot be split into two sweeps", s2);
	fp.s2_bits = s2; fp.s2_tot = s2;
	fp.sw = c->bloom_mode ? c->nb - 9 : s2; fp.ssh = fp.sw - s2;
	fp.bf_virgin = 0;
	fp.rec8_in = s.fmt_in == YK_FMT_TAGGED; fp.tb = YK_R8_TAG_BITS + s2;
	fp.rec8_out = 0;                                         /* set below, once the largest sub-table stream is known */
	if (c->bloom_mode) {
		FastParams probe = fp;                                    /* will k_lc2 run (yk_lc2_ok, asked again by slice_count)?  The tier behind it works on the filter in memory and needs real zeros */
		probe.bf_nowb = nowb_plan;
		if (c->bf_virgin && yk_lc2_ok(probe)) fp.bf_virgin = 1;   /* LDS-staged ranges: skip the read, write every block of the shard (yakamd_set_shard refuses to move the shard afterwards) */
		else if (bloom_materialise(c)) return -1;
		c->bf_virgin = false;
	}
	s.n_sb = (size_t)P << s2;
	if (s.fmt_in == YK_FMT_TAGGED) {
		if (np_max >= (1ull << 32)) return fail("more than 2^32 k-mer instances of one sub-table in one slice");
		fp.rec8_out = np_max < (1ull << fp.tb) && env_i64("YAKAMD_REC8_OUT", 1) != 0;   /* the rank must fit below the hash bits; else 16-byte records {hash, rank} */
		fp.t_pass0 = 0;                                       /* times are ranks inside the sub-table's stream of this slice */
		s.sort_tmax = np_max;
	}
	return 0;
}

/* the level-1 records stay for the count pass over the same input when the caller asked for that and they fit the budget: all of the pass's
 * records, or none.  The kept batches are released or handed to c->ret.l1 */
static void slice_retain(yakamd_ctx *c, Slice &s, bool last)
{
	bool keep = c->retain_on && !c->retain_broken && s.fmt_in == YK_FMT_TAGGED && c->bloom_mode && !c->or_mode && c->ret.l1_bytes + s.n_total * yk_rec_bytes(YK_FMT_TAGGED) <= s.budget;
	for (auto &k : c->pass.kept) keep = keep && k.own;
	/* the whole pass in this one slice, into an empty table: the level-2 records and the sub-buckets' key lists serve the count pass better (k_cnt2) */
	s.keep2 = keep && last && c->n_slices == 0 && c->img_keys_total == 0 && s.fp.rec8_out && c->ret.l1.empty() && env_i64("YAKAMD_RETAIN2", 1) != 0;
	if (s.keep2) keep = false;
	if (c->retain_on && !keep && !s.keep2 && !c->pass.kept.empty()) { c->retain_broken = true; retained_drop(c); }
	for (auto &k : c->pass.kept)
		if (keep && k.n) { Retained r; r.rec = std::move(k.own); r.n = k.n; r.bstart.swap(k.bstart); c->ret.l1.push_back(std::move(r)); c->ret.l1_bytes += k.n * yk_rec_bytes(YK_FMT_TAGGED); }
	c->pass.kept.clear(); c->pass.kept_bytes = 0;
}

/* the level-2 partition in one or two sweeps; the retain decision runs behind the first, which reads the level-1 records */
static int slice_partition(yakamd_ctx *c, Slice &s, bool last)
{
	const int P = c->P;
	const FastParams &fp = s.fp;
	const int s2_first = s.three ? s.s2a : s.s2;                 /* bits of the sweep that reads the level-1 records */
	const u64 ch2 = std::max<u64>((u64)env_i64("YAKAMD_CH2", YK_CH2), (u64)32 << s2_first);    /* keep >= 32 records per sub-bucket run */
	/* chunk table: runs of one sub-table's records, grouped by sub-table; each batch's runs cut on their own */
	ChunkTable t;
	t.first.assign(P + 1, 0);
	std::vector<u64> bbase(P + 1, 0);
	for (int p = 0; p < P; ++p) {
		t.first[p] = (u32)t.h.size();
		u64 np = 0;
		for (auto &k : c->pass.kept) {
			const u64 a = k.bstart[p], b = k.bstart[p + 1];
			for (u64 o = a; o < b; o += ch2) {
				Chunk2 ch;
				ch.rec = (const Rec*)((const char*)k.d_rec + o * yk_rec_bytes(s.fmt_in)); ch.spare = 0;
				ch.n = (u32)std::min<u64>(ch2, b - o); ch.bucket = (u32)p;
				ch.tbase = s.fmt_in == YK_FMT_TAGGED ? (u32)np : (u32)(k.t0 - c->t_pass0); ch.fmt = (u32)s.fmt_in;   /* tagged: ranks continue from the earlier batches of this sub-table */
				ch.before = (u32)(o - a); ch.after = (u32)(b - (o + ch.n));
				t.h.push_back(ch);
			}
			np += b - a;
		}
		bbase[p + 1] = bbase[p] + np;
		if (t.h.size() > t.first[p]) t.h.back().spare = 1;          /* last chunk of its sub-table */
	}
	t.first[P] = (u32)t.h.size();
	DevBuf<u64> d_bbase, d_sba; DevBuf<u32> d_rows2; DevBuf<Rec> d_ra;
	if (t.upload(c->st) || d_bbase.alloc(P + 1) || d_rows2.alloc(t.h.size() << s2_first) || s.sbstart.alloc(s.n_sb + 1) || s.segcur.alloc(P) || s.ovf2.alloc(s.n_sb)) return -1;
	if (s.three ? (d_ra.alloc(s.n_total) || d_sba.alloc(((size_t)P << s.s2a) + 1)) : s.r2_alloc()) return -1;
	HIPCK(hipMemcpyAsync(d_bbase, bbase.data(), (P + 1) * 8, hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemsetAsync(c->d_counters + YKC_NOVF2, 0, 8, c->st));
	std::vector<u64> h_sba;
	{
		EvTimer tm(c->st);
		if (!s.three) yk_launch_part2(t.d, (int)t.h.size(), t.d_first, d_bbase, fp, P, d_rows2, s.sbstart, s.r2, c->st);
		else {
			/* first sweep: the high s2a bits of the sub-bucket, {hash, rank} records out (the rank no longer fits beside the hash while only
			 * s2a of its bits are implied by the place) */
			FastParams fa = fp;
			fa.s2_bits = s.s2a; fa.ssh = fp.sw - s.s2a; fa.rec8_out = 0;
			yk_launch_part2(t.d, (int)t.h.size(), t.d_first, d_bbase, fa, P, d_rows2, d_sba, d_ra, c->st);
			h_sba.resize(((size_t)P << s.s2a) + 1);
			HIPCK(hipMemcpyAsync(h_sba.data(), d_sba, h_sba.size() * 8, hipMemcpyDeviceToHost, c->st));
		}
		c->ms_part2 = tm.stop();
		c->st_cur.ms_extract += c->ms_part2; c->st_cur.ms_part2 += c->ms_part2;
	}
	s.lap(c, "level-2 partition (first sweep)");
	slice_retain(c, s, last);
	t.reset(); d_rows2.reset(); d_bbase.reset();
	if (s.three) {
		/* second sweep: every group of the first is a bucket of its own (sub-table << s2a | group); its 2^s2b sub-buckets take the group's place in
		 * the final numbering sub-table << s2 | sub-bucket, so the offsets of the first sweep are the bucket bases of the second */
		const size_t PB = (size_t)P << s.s2a, S2B = (size_t)1 << s.s2b;
		chunk_runs(t, d_ra, sizeof(Rec), h_sba.data(), PB, std::max<u64>((u64)env_i64("YAKAMD_CH2", YK_CH2), (u64)32 << s.s2b));
		FastParams fb = fp;
		fb.s2_bits = s.s2b; fb.rec8_in = 0;                          /* routes by the low s2b bits, packs with all of them (s2_tot) */
		if (t.upload(c->st) || d_rows2.alloc(t.h.size() * S2B) || s.r2_alloc()) return -1;
		EvTimer tm(c->st);
		yk_launch_part2(t.d, (int)t.h.size(), t.d_first, d_sba, fb, (int)PB, d_rows2, s.sbstart, s.r2, c->st);
		const double ms = tm.stop();                                /* (the host vectors above outlive the copies) */
		c->ms_part2 += ms; c->st_cur.ms_extract += ms; c->st_cur.ms_part2 += ms;
		t.reset(); d_rows2.reset(); d_ra.reset(); d_sba.reset();
		if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] level-2 partition in two sweeps: 2^%d groups, then 2^%d sub-buckets each (%llu records, %.2f ms)\n", s.s2a, s.s2b, (unsigned long long)s.n_total, c->ms_part2);
	}
	s.lap(c, "release / second sweep");
	return 0;
}

/* the count: k_lc2 owns every sub-bucket in LDS and selects its new keys; the sub-buckets it passes on go to the same algorithm on tables in
 * global scratch, a group of them at a time */
static int slice_count(yakamd_ctx *c, Slice &s)
{
	const int P = c->P;
	FastParams &fp = s.fp;
	const size_t n_sb = s.n_sb;
	/* the keys a sub-bucket selects are written over the front of its own record range in lo.kc / lo.T */
	/* 8-byte level-2 records that nobody keeps: the keys go over the records themselves (a workgroup has read all of its sub-bucket's records
	 * before it writes its first key, and nobody else reads them) -- 8 bytes per record less at the peak of a slice (a cfg3 rank: 71 GB) */
	const bool kc_inplace = fp.rec8_out && !s.keep2;
	if (kc_inplace) s.lo_kc = DevBuf<u64>((u64*)s.r2.release());
	else if (s.lo_kc.alloc(s.n_total)) return -1;
	if (s.lo_T.alloc(s.n_total) || s.lo_nsel.alloc(n_sb) || s.lo_lp.alloc(n_sb) || s.lo_nd.alloc(n_sb) || s.ndist.alloc(P)) return -1;
	const Rec *lc_rec_in = kc_inplace ? (const Rec*)s.lo_kc.get() : s.r2.get();
	/* the count pass over these same records (keep2) gets its counts from the counting kernels, next to the keys they select: every instance of a
	 * key lies in its sub-bucket, which they own outright (k_cnt2 would read all the records again to count what they had in LDS).  Without the
	 * room for them the count pass recounts (k_cnt2) */
	if (s.keep2 && env_i64("YAKAMD_CNT2_FUSED", 1) != 0) s.lo_c2 = DevBuf<unsigned short>((unsigned short*)yk_pool_alloc(s.n_total * 2, false));
	if (c->plo > 0 || c->phi < P) {                              /* sub-buckets outside the shard are never visited */
		HIPCK(hipMemsetAsync(s.lo_nsel, 0, n_sb * 4, c->st)); HIPCK(hipMemsetAsync(s.lo_lp, 0, n_sb * 4, c->st)); HIPCK(hipMemsetAsync(s.lo_nd, 0, n_sb * 4, c->st));
	}
	HIPCK(hipMemsetAsync(s.ndist, 0, P * 4, c->st));
	HIPCK(hipMemsetAsync(s.segcur, 0, P * 4, c->st));
	u64 h_cnt[YKC_N];
	/* every record of the pass stays on the device (keep2) and the filter has never been written: the 2^bf_shift bits are not written at all --
	 * yak_ch_destroy_bf usually comes next (main.c:55); whatever reads the filter first rebuilds it (bloom_undefer).  nowb_plan said so before the
	 * partition (sub-buckets of up to 256 blocks, no stage in LDS); with the stage (a plan that was off) the bits are kept in LDS and dropped */
	fp.bf_nowb = s.keep2 && fp.bf_virgin && env_i64("YAKAMD_BF_DEFER", 1) != 0 && env_i64("YAKAMD_LC2", 1) != 0 && c->n_hash <= 32;
	if (s.nowb_plan && !fp.bf_nowb) {
		/* the two predicates (nowb_plan before the partition, keep2 behind it) disagree: the sub-buckets own up to 256 filter blocks, which only the
		 * kernel without a stage takes.  Not a reason to fail the pass: the filter gets its real zeros and the tier behind k_lc2 counts on it in memory */
		if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] a pass planned without a filter stage does not keep its records after all: filter materialised, sub-buckets to the global-scratch tier\n");
		if (fp.bf_virgin) { if (c->d_bf) HIPCK(hipMemsetAsync(c->d_bf, 0, c->bf_words * 4, c->st)); fp.bf_virgin = 0; }   /* (c->bf_virgin is off already: bloom_materialise would do nothing) */
	}
	const bool lc2 = yk_lc2_ok(fp) != 0;
	if (!lc2) fp.bf_nowb = 0;
	{
		EvTimer tm(c->st);
		if (lc2) yk_launch_lc2(fp, s.sbstart, lc_rec_in, c->d_bf, img_view(c), s.lo(), c->d_counters, s.ovf2, c->st);
		c->ms_lds = insert_ms(c, tm);
	}
	HIPCK(hipMemcpyAsync(h_cnt, c->d_counters, sizeof(h_cnt), hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	if (!lc2) {
		/* k_lc2 does not run this pass (n_hash > 32, sub-buckets that own more filter blocks than it stages, YAKAMD_LC2=0): every sub-bucket of the shard
		 * goes to the tier behind it */
		const u32 first = (u32)c->plo << s.s2, n_all = (u32)(c->phi - c->plo) << s.s2;
		std::vector<u32> all(n_all);
		for (u32 i = 0; i < n_all; ++i) all[i] = first + i;
		HIPCK(hipMemcpy(s.ovf2, all.data(), (size_t)n_all * 4, hipMemcpyHostToDevice));
		h_cnt[YKC_NOVF2] = n_all;
	}
	if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] %s: %.2f ms, %llu of %zu sub-buckets passed on\n", lc2 ? "k_lc2" : "k_lc2 not run", c->ms_lds, (unsigned long long)h_cnt[YKC_NOVF2], n_sb);
	yk_event(YKE_LC2_PASSED_ON, h_cnt[YKC_NOVF2]);
	if (h_cnt[YKC_NOVF2]) {     /* the same algorithm on tables in global scratch */
		const u32 n_ovf = (u32)h_cnt[YKC_NOVF2];
		std::vector<u32> ovf(n_ovf);
		std::vector<u64> sbs(n_sb + 1), off(n_ovf);
		HIPCK(hipMemcpy(ovf.data(), s.ovf2, n_ovf * 4, hipMemcpyDeviceToHost));
		HIPCK(hipMemcpy(sbs.data(), s.sbstart, (n_sb + 1) * 8, hipMemcpyDeviceToHost));
		/* scratch tables of 40 B per slot (5 u64), in groups of sub-buckets that stay within a quarter of the free memory */
		size_t fr = 0, tot = 0;
		if (hipMemGetInfo(&fr, &tot) != hipSuccess) return fail("hipMemGetInfo failed");
		const u64 max_words = (u64)env_i64("YAKAMD_OVF_SCRATCH_WORDS", (int64_t)(std::max<u64>(fr / 4, (u64)1 << 28) / 8));
		DevBuf<u64> scroff;
		if (scroff.alloc(n_ovf)) return -1;
		for (u32 i0 = 0; i0 < n_ovf;) {
			u64 words = 0;
			u32 i1 = i0;
			for (; i1 < n_ovf; ++i1) {
				const u64 n = sbs[ovf[i1] + 1] - sbs[ovf[i1]];
				u64 cap = 4096; while (cap < 2 * n) cap <<= 1;
				if (i1 > i0 && words + 5 * cap > max_words) break;
				off[i1] = words; words += 5 * cap;
			}
			DevBuf<u64> scr;
			if (scr.alloc(words)) return -1;
			HIPCK(hipMemcpyAsync(scroff + i0, off.data() + i0, (size_t)(i1 - i0) * 8, hipMemcpyHostToDevice, c->st));
			EvTimer tm(c->st);
			yk_event(YKE_OVF_GROUPS); if (i0) yk_event(YKE_OVF_MORE_GROUPS);
			yk_launch_lds_count_ovf(fp, s.sbstart, lc_rec_in, c->d_bf, img_view(c), s.lo(), s.ovf2 + i0, i1 - i0, scroff + i0, scr, c->st);
			c->st_cur.ms_insert += tm.stop();
			HIPCK(hipStreamSynchronize(c->st));
			scr.reset();
			i0 = i1;
		}
	}
	return 0;
}

/* gather the fragments: keys per sub-table, then one contiguous list each, and the plan of the sort by insertion time; with keep2 the list and its
 * sub-bucket offsets go to c->ret.l2 */
static int slice_gather(yakamd_ctx *c, Slice &s)
{
	const int P = c->P;
	const FastParams &fp = s.fp;
	const int s2 = s.s2;
	const LcOut lo = s.lo();
	s.m.assign(P, 0);
	s.ro.assign(P + 1, 0);
	/* many sub-buckets per sub-table, or few sub-tables: the gather spread over the whole chip (k_lc_sum3 / k_nsel_scan / k_lc_gather) */
	const bool flat = env_i64("YAKAMD_LC_FLAT", (s2 > 11 || c->phi - c->plo < 512) ? 1 : 0) != 0;
	if (flat) yk_launch_lc_sum3(lo, s2, c->plo, c->phi, fp.t_pass0, s.segcur, c->d_lastput, s.ndist, c->st);
	else yk_launch_lc_sum(lo.nsel, s2, c->plo, c->phi, s.segcur, c->st);
	HIPCK(hipMemcpyAsync(s.m.data(), s.segcur, P * 4, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	for (int p = 0; p < P; ++p) s.ro[p + 1] = s.ro[p] + s.m[p];
	const u64 n_sel = s.n_sel = s.ro[P];
	/* The sort by insertion time T.  Times are unique inside a sub-table and < 2^tbits, so the order needs no comparisons: one partition sweep by
	 * the top ts_b bits of T (the level-2 partition's kernels on {key, T} pairs), then every bin ranks its keys with a bitmap of its 2^ts_w possible
	 * times (k_ts_rank).  ts_w = 11 wherever that leaves at most 2^13 bins: a bin then never holds more keys than the ranking kernel's registers and
	 * stage (the times of first occurrences are dense at the start of a stream of reads and sparse later), and the kernel takes 2^ts_j sparse
	 * neighbours in one step (~1000 keys).  Times beyond 32 bits or bins wider than 2^18 times take the stable 8-bit passes as before */
	s.tbits = std::max(1, ceil_log2_u64(s.sort_tmax + 1));
	u32 m_max = 0;
	for (int p = 0; p < P; ++p) m_max = std::max(m_max, s.m[p]);
	s.ts_b = std::min(13, std::max(0, s.tbits - 11));
	s.ts_b = (int)std::min<int64_t>(13, std::max<int64_t>(0, env_i64("YAKAMD_TS_BITS", s.ts_b)));
	s.ts_w = std::max(5, s.tbits - s.ts_b);
	while (s.ts_j < s.ts_b && s.ts_w + s.ts_j < 15 && ((u64)m_max >> (s.ts_b - s.ts_j - 1)) <= 256) ++s.ts_j;   /* a mean of 256: the head of a stream of reads is several times denser */
	s.ts_j = (int)std::min<int64_t>(s.ts_b, std::max<int64_t>(0, env_i64("YAKAMD_TS_JOIN", s.ts_j)));
	/* short lists in many sub-tables (a filtered count of reads: ~50 K keys per sub-table) are done sooner by three launches of the stable pass */
	s.tsort = env_i64("YAKAMD_TSORT", (m_max >= 100000 || c->phi - c->plo < 512) ? 1 : 0) != 0 && s.tbits <= 32 && s.ts_w + s.ts_j <= 18 && n_sel > 0;
	if (s.kc[0].alloc(n_sel) || s.tt[0].alloc(n_sel) || s.segbase.alloc(P + 1)) return -1;
	if (s.tsort && (s.kt.alloc(n_sel) || s.tsfail.alloc(1))) return -1;
	HIPCK(hipMemcpyAsync(s.segbase, s.ro.data(), (P + 1) * 8, hipMemcpyHostToDevice, c->st));
	if (lo.c2) s.kc2 = DevBuf<u32>((u32*)yk_pool_alloc(std::max<u64>(n_sel, 1) * 4, false));   /* the count pass's counts, in the order of the gathered list (ret.l2.kkc) */
	{
		EvTimer tm(c->st);
		if (flat) {
			if (s.koff.alloc(s.n_sb + 1)) return -1;
			yk_launch_nsel_scan(lo.nsel, s2, c->plo, c->phi, P, s.segbase, s.koff, c->st);
			yk_launch_lc_gather(lo, s.sbstart, s.koff, s2, c->plo, c->phi, s.kc[0], s.tt[0], s.kt, s.kc2, c->st);
		} else yk_launch_lc_compact(lo, s.sbstart, s2, c->plo, c->phi, fp.t_pass0, s.segbase, s.kc[0], s.tt[0], c->d_lastput, s.ndist, s.kt, s.kc2, c->st);
		c->st_cur.ms_select += tm.stop();
	}
	{
		std::vector<u32> nd(P);
		HIPCK(hipMemcpy(nd.data(), s.ndist, P * 4, hipMemcpyDeviceToHost));
		u64 tot_d = 0;
		for (int p = 0; p < P; ++p) tot_d += nd[p];
		c->st_cur.n_distinct_seen += (int64_t)tot_d;
	}
	if (!s.keep2) return 0;
	/* the gathered list is grouped by sub-bucket (k_lc_compact walks them in order): a copy of it + the first key of every sub-bucket */
	Ret2 &l2 = c->ret.l2;
	if ((!s.koff && l2.koff.alloc(s.n_sb + 1)) || l2.kkc.alloc(n_sel) || l2.segbase.alloc(P + 1)) {
		if (fp.bf_nowb) {                                         /* the records go after all: the filter they stood for is written now */
			FastParams fr = fp;
			fr.bf_nowb = 0;
			HIPCK(hipMemsetAsync(c->d_bf, 0, c->bf_words * 4, c->st));
			yk_launch_bf_rebuild(fr, s.sbstart, l2.r2, c->d_bf, c->st);
			HIPCK(hipStreamSynchronize(c->st));
		}
		retained_drop(c); c->retain_broken = true; s.keep2 = false;
		return 0;
	}
	if (s.koff) l2.koff = std::move(s.koff);                   /* the flat gather has them already */
	else yk_launch_nsel_scan(lo.nsel, s2, c->plo, c->phi, P, s.segbase, l2.koff, c->st);
	if (s.kt) yk_launch_kt_split(s.kt, n_sel, l2.kkc, 0, c->st);
	else HIPCK(hipMemcpyAsync(l2.kkc, s.kc[0], n_sel * 8, hipMemcpyDeviceToDevice, c->st));
	l2.sbstart = std::move(s.sbstart);
	HIPCK(hipMemcpyAsync(l2.segbase, s.segbase, (P + 1) * 8, hipMemcpyDeviceToDevice, c->st));
	l2.kc2 = std::move(s.kc2);
	l2.n_keys = n_sel;
	l2.valid = true;
	c->bf_deferred = fp.bf_nowb != 0;
	return 0;
}

/* the sort by insertion time: bitmap ranks, or the stable radix passes where they are refused; the result is kc[cur] / tt[cur] */
static int slice_sort(yakamd_ctx *c, Slice &s)
{
	const int P = c->P;
	const u64 n_sel = s.n_sel;
	bool sorted = false;
	if (s.tsort) {
		EvTimer tm(c->st);
		HIPCK(hipMemsetAsync(s.tsfail, 0, 4, c->st));
		const Rec *rank_in = s.kt;
		const u64 *rank_start = s.segbase;                        /* ts_b == 0: a sub-table is its one bin */
		DevBuf<Rec> kt2; DevBuf<u64> binstart;
		if (s.ts_b > 0) {
			ChunkTable t;
			chunk_runs(t, s.kt, sizeof(Rec), s.ro.data(), P, std::max<u64>((u64)env_i64("YAKAMD_CH2", YK_CH2), (u64)32 << s.ts_b));
			DevBuf<u32> rows;
			if (t.upload(c->st) || rows.alloc(t.h.size() << s.ts_b) || binstart.alloc(((size_t)P << s.ts_b) + 1) || kt2.alloc(n_sel)) return -1;
			FastParams ft = s.fp;
			ft.s2_bits = s.ts_b; ft.ssh = s.ts_w; ft.rec8_in = 0; ft.rec8_out = 0;
			yk_launch_part2_ts(t.d, (int)t.h.size(), t.d_first, s.segbase, ft, P, rows, binstart, kt2, c->st);
			HIPCK(hipStreamSynchronize(c->st));                  /* the host tables above go out of scope */
			rank_in = kt2; rank_start = binstart;
			s.kt.reset();                                           /* the pairs as gathered: no longer needed (a refused ranking re-splits the partitioned ones: same keys per sub-table) */
		}
		u32 h_fail = 1;
		if (yk_launch_ts_rank(rank_start, rank_in, s.ts_w, s.ts_j, (u32)c->plo << s.ts_b, (u32)(c->phi - c->plo) << s.ts_b, s.kc[0], s.tt[0], s.tsfail, c->st) == 0) {
			HIPCK(hipMemcpyAsync(&h_fail, s.tsfail, 4, hipMemcpyDeviceToHost, c->st));
			HIPCK(hipStreamSynchronize(c->st));
		}
		sorted = h_fail == 0;
		if (!sorted) yk_event(YKE_RANK_REFUSED);
		if (!sorted) {                                            /* a time seen twice, or the kernel could not be configured: the stable passes on the gathered pairs */
			if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] sort by bitmap ranks refused: stable radix passes instead\n");
			yk_launch_kt_split(rank_in, n_sel, s.kc[0], s.tt[0], c->st);
		}
		kt2.reset(); binstart.reset();
		c->st_cur.ms_sort += tm.stop();
	}
	s.kt.reset();
	if (!sorted) {
		/* the first pass counts every digit's histogram in its one sweep over the times, the later ones take theirs from dig_hist */
		const int n_dig = sst_n_digits(s.tbits);
		DevBuf<u32> dig_hist;
		if (s.kc[1].alloc(n_sel) || s.tt[1].alloc(n_sel) || (n_dig > 1 && dig_hist.alloc((size_t)P * n_dig * SST_NBIN))) return -1;
		EvTimer tm(c->st);
		const int sort_big = n_sel / (u64)std::max(1, c->phi - c->plo) >= 30000;
		for (int shift = 0; shift < s.tbits; shift += 8) {
			yk_launch_seg_sort_pass2(s.segbase, s.segcur, P, s.kc[s.cur], s.tt[s.cur], s.kc[s.cur ^ 1], s.tt[s.cur ^ 1], shift, dig_hist, n_dig, c->st, sort_big);
			s.cur ^= 1;
		}
		c->st_cur.ms_sort += tm.stop();
	}
	return 0;
}

int fast_finish(yakamd_ctx *c, bool last)
{
	Slice s;
	yk_event(YKE_SLICES);
	if (slice_plan(c, s, last) || slice_partition(c, s, last) || slice_count(c, s)) return -1;
	s.lap(c, "insert (k_lc2 + tiers)");
	if (s.keep2) { Ret2 &l2 = c->ret.l2; l2.r2 = std::move(s.r2); l2.n_total = s.n_total; l2.fp = s.fp; l2.fp.bf_nowb = 0; }
	s.r2.reset(); s.ovf2.reset();
	if (slice_gather(c, s)) return -1;
	s.lo_kc.reset(); s.lo_T.reset(); s.lo_nsel.reset(); s.lo_lp.reset(); s.lo_nd.reset(); s.lo_c2.reset();
	s.kc2.reset(); s.sbstart.reset(); s.ndist.reset(); s.koff.reset();
	s.lap(c, "gather of the selected keys");
	if (slice_sort(c, s)) return -1;
	s.kc[s.cur ^ 1].reset(); s.tt[s.cur ^ 1].reset();           /* the sort's other buffer pair: 16 bytes per key the layout stage can use */
	s.lap(c, "sort by insertion time");
	{
		EvTimer tm(c->st);
		s.ro.resize(c->P);
		if (yk_run_replay(c, s.m, s.kc[s.cur], s.tt[s.cur], c->d_lastput, 0, false, &s.ro)) return -1;
		c->st_cur.ms_replay += tm.stop();
	}
	s.lap(c, "exact layout");
	/* the retained key list is the image: the pass began on an empty one and this is its only slice (keep2 says both; no k_lc2 instance met a table),
	 * it kept the counts of the count pass, and every listed key went in once -- the count pass may then raise all counts in one sweep
	 * (yakamd_count_retained).  The mark falls with the first change of keys or counts that is not a clear (yk_image_touched: the layout just above too) */
	Ret2 &l2 = c->ret.l2;
	l2.whole_image = s.keep2 && l2.valid && l2.kc2 && last && c->n_slices == 0 && c->keys_at_begin == 0 && !s.fp.img_nonempty && !c->retain_broken &&
	                 l2.n_keys == c->img_keys_total;
	return 0;
}

/* leave the fast path: push every kept batch through the accumulator path, in stream order */
int fast_abandon(yakamd_ctx *c)
{
	for (auto &k : c->pass.kept) if (k.fmt != YK_FMT_POS) return fail("a batch was fed out of stream order after tagged 8-byte batches were kept: feed in order, or set YAKAMD_REC8=0");
	c->fast = false;
	yk_event(YKE_FAST_ABANDONED);
	c->retain_broken = true; retained_drop(c);                 /* the pass leaves the path whose records can be kept */
	int r = 0;
	for (auto &k : c->pass.kept) {
		if (!r) r = consume_records(c, k.d_rec, k.fmt, (int64_t)k.n, k.t0, k.t0, k.t0 + k.span);
		k.own.reset();
	}
	c->pass.kept.clear(); c->pass.kept_bytes = 0;
	return r;
}

static int fast_flush_slice(yakamd_ctx *c)
{
	if (fast_finish(c)) return -1;
	++c->n_slices; yk_event(YKE_EARLY_SLICES);
	HIPCK(hipMemsetAsync(c->d_lastput, 0, c->P * 8, c->st));      /* the put-calls of the slice are accounted for */
	HIPCK(hipMemsetAsync(c->d_counters, 0, YKC_N * 8, c->st));
	if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] slice of the pass counted early (budget / 2^32-position limit): %llu keys in the table\n", (unsigned long long)c->img_keys_total);
	return 0;
}

/* may this batch (n_pos stream positions starting at time t) stay on the fast path?  If so,
 * allocate its level-1 output buffers */
int fast_admit(yakamd_ctx *c, RecFmt fmt, u64 t, u64 n_pos, u64 n_cap, void **out, const void *borrowed)
{
	if (!c->t_pass0_set) { c->t_pass0 = t; c->t_pass0_set = true; }
	/* what a kept record costs against the budget (a quarter of the free memory): its 16 bytes, or for an 8-byte tagged record 12 -- the count of
	 * the slice holds 24-32 bytes per record at its peak (level-2 records, 8 or 16 bytes when the ranks outgrow their field, + 16 of key / time
	 * output), so that a slice admitted by records x 12 <= free / 4 peaks at two thirds of the free memory.  (Tagged slices used to be cut by the
	 * 2^32-position limit long before memory mattered; a rank of an 8-GPU job feeds 9 G records.)  A borrowed buffer is the caller's memory */
	const u64 tagged_peak_share = 4;                            /* what a tagged record is charged beyond its own bytes, for its part in that peak */
	const bool tagged = fmt == YK_FMT_TAGGED;
	const u64 cost = borrowed ? 0 : n_cap * (yk_rec_bytes(fmt) + (tagged ? tagged_peak_share : 0));
	/* {hash, position} records hold 32-bit positions relative to the slice; tagged records hold no position at all (their times are ranks inside a
	 * sub-table's stream, checked when the slice is counted), so a slice of them may span more than 2^32 stream positions */
	const bool span_ok = tagged || t + n_pos - c->t_pass0 < 0xfffffff0ull;
	bool fits = t >= c->t_pass0 && span_ok && c->pass.kept_bytes + cost <= c->fast_budget;
	if (fits && !c->pass.kept.empty()) {
		/* the count of a slice cuts a sub-table into at most 2^13 sub-buckets, each meant to hold what one workgroup's LDS table takes (fast_finish):
		 * a slice stops growing where its sub-tables would outgrow that.  Unsharded that is > 5 G records; an 8-GPU rank (an eighth of the
		 * sub-tables, 9 G records of 600 M reads) reaches it every ~700 M records -- the 2^32-position limit used to cut there by accident */
		u64 kept_n = 0;
		for (auto &k : c->pass.kept) kept_n += k.n;
		const u64 per_sb = (u64)yk_lc2_per_sb(c->bloom_mode);
		if (kept_n + n_cap > (u64)(c->phi - c->plo) * (u64)env_i64("YAKAMD_SLICE_SB", env_i64("YAKAMD_P3_MIN", 13) < 18 ? (int64_t)1 << 18 : 8192) * per_sb) fits = false;
	}
	if (!c->pass.kept.empty() && c->pass.kept.back().fmt != fmt) fits = false;   /* tagged records carry ranks, Rec records stream positions: never in one slice */
	/* (a chunk that continues a sequence cut by the caller starts k - 1 positions before the end of the previous one, yak_multi.cpp take_piece:
	 * its first k - 1 positions complete no k-mer, so it is still "behind" everything kept) */
	if (!fits && !c->pass.kept.empty() && t + (u64)(c->k - 1) >= c->t_end && (tagged || n_pos < 0xfffffff0ull) && cost <= c->fast_budget && !c->pass.acc.s) {
		/* the kept batches are a complete prefix of the stream: count them now, exactly as if the pass
		 * ended here (table, filter and counts carry over; the next slice meets them as existing state --
		 * what the reference does chunk after chunk), and start a new slice with times relative to t */
		if (fast_flush_slice(c)) return -1;
		c->t_pass0 = t;
		fits = true;
	}
	if (!fits) { if (fast_abandon(c)) return -1; return 0; }
	Kept k;
	k.t0 = t; k.span = n_pos; k.fmt = fmt;
	if (!borrowed && k.own.alloc(yk_rec_units(fmt, (size_t)n_cap))) return -1;
	*out = k.own.get(); k.d_rec = borrowed ? borrowed : k.own.get();
	c->pass.kept_bytes += cost;
	c->pass.kept.push_back(std::move(k));
	return 0;
}

int fast_keep(yakamd_ctx *c, u64 n_rec)
{
	Kept &k = c->pass.kept.back();
	const size_t NB = (size_t)1 << c->nb_bits;
	k.bstart.resize(NB + 1);
	HIPCK(hipMemcpyAsync(k.bstart.data(), c->d_bstart, (NB + 1) * 8, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	k.n = n_rec;
	c->st_cur.n_instances += (int64_t)n_rec;
	return 0;
}
