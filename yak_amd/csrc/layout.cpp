/*
 * layout.cpp -- the exact-layout stage of a pass: the streaming replay of large sub-tables (kern_replay2.inc) as a sequence of stages over the host
 * plan of replay_plan.h (capacities after the new keys, khashl.h:197-221; the doubling / placement schedule; the arenas), and the one-workgroup-per-table
 * replay of small tables (k_replay).  Cut out of the engine's passes (now engine_pass.cpp, engine_acc.cpp, engine_slice.cpp) in round 6.
 */
#include "engine_int.h"

/* ------------------------------------------------------------------------------------------
 * layout planning + replay
 * ------------------------------------------------------------------------------------------ */

/* launch parameters of k_replay for a set of tasks (shared by the two replay drivers) */
static void legacy_replay_launch(yakamd_ctx *c, const std::vector<ReplayTask> &tasks, const ReplayTask *d_tasks, u64 *nk, u32 *nu, u32 *su, u32 *so, u64 *sp,
                                 const u64 *d_rec_kc, const u64 *d_rec_t, const u64 *d_lastput, u32 *d_ob, u32 *d_oc)
{
	const int P = c->P, n_active = c->phi - c->plo;               /* few, large sub-tables (a shard of a multi-GPU job): more lanes per sub-table */
	/* owner ranks of the placement stages in LDS: 32-bit up to lds_words slots, 16-bit up to twice that */
	u32 cap_top = 0;
	for (int p = 0; p < P; ++p) if (tasks[p].m) cap_top = std::max(cap_top, 1u << tasks[p].cap_max_bits);
	u32 lds_words = std::min<u32>(cap_top, (u32)env_i64("YAKAMD_REPLAY_LDS", 16384));   /* 64 KB: two workgroups per CU (measured 18.5 ms against 20.5 with 128 KB); 0: owner ranks in global scratch */
	int n_thr = n_active <= 256 ? 1024 : n_active <= 512 ? 512 : 256;
	if (lds_words * 4 >= 96 * 1024) n_thr = 1024; else if (lds_words * 4 >= 48 * 1024) n_thr = std::max(n_thr, 512);
	n_thr = (int)env_i64("YAKAMD_REPLAY_THREADS", n_thr);
	yk_launch_replay(d_tasks, P, n_thr, c->d_keys, c->d_used, nk, nu, su, so, sp, d_rec_kc, d_rec_t, d_lastput, d_ob, d_oc, lds_words, c->st);
}

int yk_image_commit(yakamd_ctx *c, DevBuf<u64> &&keys, DevBuf<u32> &&used, u64 tot, const std::vector<u64> &new_off)
{
	c->d_keys = std::move(keys); c->d_used = std::move(used); c->d_delta.reset();   /* (each frees the old image's first) */
	yk_image_touched(c);
	c->n_slots = tot;
	c->h_off = new_off;
	HIPCK(hipMemcpyAsync(c->d_bits, c->h_bits.data(), c->P * 4, hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemcpyAsync(c->d_off, c->h_off.data(), c->P * 8, hipMemcpyHostToDevice, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	c->img_keys_total = 0;
	for (int p = 0; p < c->P; ++p) c->img_keys_total += c->h_count[p];
	c->host_valid = false;
	return 0;
}

static u32 g_r2_used = 0, g_r2_refused = 0;        /* debug counters: replays done by the streaming kernels / handed back to k_replay */

/* What the stages of a streaming replay hand each other: the host plan (replay_plan.h) and every device buffer of the stage, owned here and given back
 * to the pool when the replay ends, last member first (the order in which the pool sees them is part of its reuse pattern) */
struct Replay2 {
	yakamd_ctx *c;
	const u64 *d_rec_kc, *d_rec_t, *d_lastput;
	ReplayPlan pl;
	std::vector<u64> lp_host;                                    /* the last put-call per sub-table, as far as k_replay may act on it */
	std::vector<u32> ob, oc;                                     /* what k_replay left: log2 slots and keys per sub-table */
	u64 *nk = 0; u32 *nu = 0;                                    /* k_replay's arena: nk_al / nu_al, addressed from slot pl.nk_lo on */
	u32 spill_cap = 0;
	int ppG = 1;
	bool prof = false; double tl = 0;
	DevBuf<R2Pub> d_pub; DevBuf<R2Load> d_ld; DevBuf<R2Act> d_acts; DevBuf<R2Tab> d_tabs; DevBuf<ReplayTask> d_tasks;
	DevBuf<u32> misc, Fc, head, segst, pr, pcnt, USED, OCC, TAG, d_oc, d_ob, so, su;
	DevBuf<u64> spill, pk, K1, K0, sp, d_lp2, d_ro;
	DevBuf<u32> d_trail, d_m;
	DevBuf<u32> img_u, nu_al; DevBuf<u64> nk_al;                  /* img_u: the image's bitmap when a work buffer becomes the image */

	u32 *d_fail() const { return misc; }                         /* a kernel refused: read once, after the last step */
	u32 *d_nspill() const { return misc + 1; }
	void lap(const char *what, size_t k, u32 bits)
	{
		if (!prof) return;
		hipStreamSynchronize(c->st);
		const double t1 = now_ms();
		fprintf(stderr, "[yak_amd] replay2 step %zu (2^%u): %s %.3f ms\n", k, bits, what, t1 - tl);
		tl = t1;
	}
};

/* classify; read back which sub-tables end with a put-call on an existing key (device data: the last put-call and the time of the last new key per
 * sub-table); schedule */
static int r2_plan(Replay2 &s, const ReplayIn &in)
{
	yakamd_ctx *c = s.c; const int P = in.P;
	const u32 SB = (u32)std::min<int64_t>(20, std::max<int64_t>(5, env_i64("YAKAMD_R2_SMALL_BITS", 13)));
	if (!s.pl.classify(in, SB, (u32)env_i64("YAKAMD_DBG", 0))) return 1;
	std::vector<u32> trail(P, 0);
	s.lp_host.assign(P, 0);
	if (s.d_lastput) {
		if (s.d_m.alloc(P) || s.d_trail.alloc(P) || s.d_ro.alloc(P) || s.d_lp2.alloc(P)) return -1;
		HIPCK(hipMemcpyAsync(s.d_m, in.m, P * 4, hipMemcpyHostToDevice, c->st));
		HIPCK(hipMemcpyAsync(s.d_ro, s.pl.rec_off.data(), P * 8, hipMemcpyHostToDevice, c->st));
		yk_r2_trail(s.d_lastput, s.d_rec_t, s.d_ro, s.d_m, P, s.d_trail, c->st);
		HIPCK(hipMemcpyAsync(trail.data(), s.d_trail, P * 4, hipMemcpyDeviceToHost, c->st));
		HIPCK(hipMemcpyAsync(s.lp_host.data(), s.d_lastput, P * 8, hipMemcpyDeviceToHost, c->st));
		HIPCK(hipStreamSynchronize(c->st));
	}
	const int r = s.pl.schedule(trail.data(), yk_r2_seg_log());
	return r < 0 ? fail("%s", s.pl.err) : r;
}

/* the empty pattern (no key, no "used" bit) on the arena regions of the sub-tables that are not large: a run of them is contiguous in the arena */
static int clear_small_runs(const ReplayPlan &pl, u64 *keys, u32 *used, hipStream_t st)
{
	for (int p = 0; p < pl.P;) {
		if (pl.large[p]) { ++p; continue; }
		int q = p;
		while (q < pl.P && !pl.large[q]) ++q;
		const u64 a = pl.new_off[p], b = q < pl.P ? pl.new_off[q] : pl.tot;
		HIPCK(hipMemsetAsync(keys + a, 0xff, (b - a) * 8, st));
		HIPCK(hipMemsetAsync(used + a / 32, 0, (b - a) / 32 * 4, st));
		p = q;
	}
	return 0;
}

/* k_replay: the small sub-tables into the final arena, the first part of the large ones into the side arena behind it */
static int r2_small_part(Replay2 &s)
{
	yakamd_ctx *c = s.c; const ReplayPlan &pl = s.pl; const int P = pl.P;
	const u64 tot = pl.tot, tot_ext = pl.tot_ext, scr_lo = pl.scr_lo, scr_n = tot_ext - scr_lo, nk_lo = pl.nk_lo;
	const bool par = env_i64("YAKAMD_PAR_REPLAY", 1) != 0;
	if ((par && s.sp.alloc(2 * scr_n)) || s.nk_al.alloc(tot_ext - nk_lo) || s.nu_al.alloc((tot_ext - nk_lo) / 32 + 1) || s.su.alloc(scr_n / 32 + 1) || s.so.alloc(scr_n) ||
	    s.d_tasks.alloc(P) || s.d_ob.alloc(P) || s.d_oc.alloc(P)) return -1;
	u64 *const nk = s.nk = s.nk_al - nk_lo; u32 *const nu = s.nu = s.nu_al - nk_lo / 32;
	if (pl.only_side) {
		/* k_r2_publish writes every slot and every bitmap word of a large sub-table: only the side arena and the (empty, 32-slot) regions of
		 * the other sub-tables need the empty pattern -- not 8 bytes per slot of the whole arena (1 Gb assembly: 2.9 ms).  In place, the side
		 * arena is all there is of nk / nu: the other regions are cleared in the buffer that becomes the image, after the last step */
		HIPCK(hipMemsetAsync(nk + tot, 0xff, (tot_ext - tot) * 8, c->st));
		HIPCK(hipMemsetAsync(nu + tot / 32, 0, ((tot_ext - tot) / 32 + 1) * 4, c->st));
		if (!pl.inplace && clear_small_runs(pl, nk, nu, c->st)) return -1;
	} else {
		HIPCK(hipMemsetAsync(nk, 0xff, tot_ext * 8, c->st));
		HIPCK(hipMemsetAsync(nu, 0, (tot_ext / 32 + 1) * 4, c->st));
	}
	/* the trailing put-call of a large sub-table is the schedule's business; and no put-call can have hit a sub-table that holds nothing (only_side:
	 * all the others): never let a stray time grow it */
	for (int p = 0; p < P; ++p) if (pl.large[p] || pl.only_side) s.lp_host[p] = 0;
	HIPCK(hipMemcpyAsync(s.d_tasks, pl.tasks.data(), P * sizeof(ReplayTask), hipMemcpyHostToDevice, c->st));
	if (s.d_lastput) HIPCK(hipMemcpyAsync(s.d_lp2, s.lp_host.data(), P * 8, hipMemcpyHostToDevice, c->st));
	legacy_replay_launch(c, pl.tasks, s.d_tasks, nk, nu, s.su - scr_lo / 32, s.so - scr_lo, s.sp ? s.sp - 2 * scr_lo : 0, s.d_rec_kc, s.d_rec_t, s.d_lastput ? s.d_lp2.get() : 0, s.d_ob, s.d_oc);
	s.ob.resize(P); s.oc.resize(P);
	HIPCK(hipMemcpyAsync(s.ob.data(), s.d_ob, P * 4, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipMemcpyAsync(s.oc.data(), s.d_oc, P * 4, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	s.sp.reset(); s.su.reset(); s.so.reset();
	for (int p = 0; p < P; ++p)
		if (pl.large[p] && pl.ld[p].from_src == 1 && (s.ob[p] != pl.bitsS[p] || s.oc[p] != pl.cntS[p]))
			return fail("replay: sub-table %d left k_replay with 2^%u slots / %u keys, the schedule says 2^%u / %u", p, s.ob[p], s.oc[p], pl.bitsS[p], pl.cntS[p]);
	return 0;
}

/* the work buffers of the large sub-tables, the plan's parameter blocks, and the tables k_replay or the old image hold into the buffers */
static int r2_buffers(Replay2 &s)
{
	yakamd_ctx *c = s.c; const ReplayPlan &pl = s.pl; const int P = pl.P;
	const u64 tot2 = pl.tot2, nseg_tot = pl.nseg_tot;
	if (pl.inplace && s.img_u.alloc(pl.tot / 32 + 1)) return -1;
	s.spill_cap = (u32)std::min<u64>(1u << 28, std::max<u64>(1u << 20, tot2 / 16));   /* also the list of long runs of a doubling round */
	if (s.K0.alloc(tot2) || s.K1.alloc(tot2) || s.TAG.alloc(tot2 / 2 + 1) || s.OCC.alloc(tot2 / 16 + (size_t)P + 64) || s.USED.alloc(tot2 / 32 + 64) || s.d_tabs.alloc(P) || s.d_acts.alloc(pl.acts.size()) || s.d_ld.alloc(P) || s.d_pub.alloc(P) ||
	    s.pk.alloc(pl.n_keys) || s.pr.alloc(pl.n_keys) || s.segst.alloc(nseg_tot + 1) || s.head.alloc((size_t)nseg_tot * yk_r2_head()) || s.spill.alloc(s.spill_cap) || s.Fc.alloc(4 * (size_t)P) || s.misc.alloc(4)) return -1;
	/* few large sub-tables (a shard): the keys of a stage are grouped by G workgroups per sub-table instead of one (YAKAMD_R2_PPART_G: tests) */
	s.ppG = (int)std::min<int64_t>(16, std::max<int64_t>(1, env_i64("YAKAMD_R2_PPART_G", pl.n_large <= 512 ? 1024 / std::max<u32>(1, pl.n_large) : 1)));
	if ((size_t)P * s.ppG > (64u << 10)) s.ppG = 1;              /* (the counters are indexed by sub-table: 4 KB per sub-table and share) */
	if (s.ppG > 1 && s.pcnt.alloc((size_t)P * s.ppG * 1024)) return -1;
	HIPCK(hipMemcpyAsync(s.d_tabs, pl.tabs.data(), P * sizeof(R2Tab), hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemcpyAsync(s.d_acts, pl.acts.data(), pl.acts.size() * sizeof(R2Act), hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemcpyAsync(s.d_ld, pl.ld.data(), P * sizeof(R2Load), hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemcpyAsync(s.d_pub, pl.pub.data(), P * sizeof(R2Pub), hipMemcpyHostToDevice, c->st));
	HIPCK(hipMemsetAsync(s.misc, 0, 16, c->st));
	yk_r2_load(s.d_tabs, s.d_ld, P, pl.bmaxS, s.nk, c->d_keys, s.K0, s.K1, s.USED, c->st);
	s.prof = env_i64("YAKAMD_VERBOSE", 0) > 1;
	s.tl = now_ms();
	s.lap("k_replay part + load", 0, pl.bmaxS);
	return 0;
}

/* all large sub-tables advance together, step by step: a doubling, or a placement of the next keys up to the growth threshold */
static void r2_steps(Replay2 &s)
{
	yakamd_ctx *c = s.c; const ReplayPlan &pl = s.pl; const int P = pl.P;
	for (size_t k = 0; k < pl.n_steps; ++k) {
		u32 bd = 0, bp = 0; int n_dbl = 0;
		int p_lo = P, p_hi = 0;                                      /* the sub-tables that place in this step: a shard's are a contiguous range of the P */
		for (int p = 0; p < P; ++p) {
			const R2Act &a = pl.acts[k * P + p];
			if (a.kind == 2) { ++n_dbl; bd = std::max(bd, a.bits); }
			else if (a.kind == 1) { bp = std::max(bp, a.bits); p_lo = std::min(p_lo, p); p_hi = p + 1; }
		}
		const R2Act *da = s.d_acts + k * P;
		if (n_dbl) {
			yk_r2_binit(s.d_tabs, da, P, bd, s.OCC, s.USED, c->st);
			s.lap("binit", k, bd);
			yk_r2_dsmall(s.d_tabs, da, P, s.K0, s.K1, s.TAG, s.OCC, s.USED, s.Fc, s.Fc + 2 * P, s.d_fail(), c->st);
			s.lap("dsmall", k, bd);
			/* the rounds from there on in one launch: a workgroup per sub-table walks its rounds behind workgroup barriers.  A sub-table that does
			 * not reach its end raises `fail` (read once, after the last step: whatever the later steps then do is thrown away with the buffers) */
			yk_r2_double(s.d_tabs, da, P, n_dbl, s.K0, s.K1, s.TAG, s.OCC, s.USED, s.Fc, s.Fc + P, s.d_fail(), c->st);
			s.lap("double (fused rounds)", k, bd);
		}
		if (p_hi) { yk_r2_place(s.d_tabs, da, P, p_lo, p_hi - p_lo, bp, s.K0, s.K1, s.d_rec_kc, s.pk, s.pr, s.segst, s.head, s.spill, s.d_nspill(), s.spill_cap, s.d_fail(), s.img_u, s.USED, s.pcnt, s.ppG, c->st); s.lap("place", k, bp); }
	}
}

/* the final tables into the image; the kernels' verdict; the context takes the image over */
static int r2_publish_commit(Replay2 &s)
{
	yakamd_ctx *c = s.c; ReplayPlan &pl = s.pl; const int P = pl.P;
	DevBuf<u64> &A = pl.img_is1 ? s.K1 : s.K0;                   /* the buffer that becomes the image (inplace) */
	if (pl.inplace) {
		if (clear_small_runs(pl, A, s.img_u, c->st)) return -1;   /* the regions of the sub-tables that hold nothing */
		for (int p = 0; p < P; ++p) { pl.pub[p].new_off = pl.tabs[p].off; if (!pl.pub_needed[p]) pl.pub[p].bits = YK_NOCAP; }
		HIPCK(hipMemcpyAsync(s.d_pub, pl.pub.data(), P * sizeof(R2Pub), hipMemcpyHostToDevice, c->st));
		yk_r2_publish(s.d_tabs, s.d_pub, P, pl.bmaxF, s.K0, s.K1, A, s.img_u, c->st);   /* a table already in A only gets its bitmap */
	} else yk_r2_publish(s.d_tabs, s.d_pub, P, pl.bmaxF, s.K0, s.K1, s.nk, s.nu, c->st);
	s.lap("publish", pl.n_steps, pl.bmaxF);
	u32 h_fail = 0;
	HIPCK(hipMemcpyAsync(&h_fail, s.d_fail(), 4, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	if (h_fail) {
		if (env_i64("YAKAMD_VERBOSE", 0)) fprintf(stderr, "[yak_amd] streaming replay refused (code %u): falling back to k_replay\n", h_fail);
		++g_r2_refused; yk_event(YKE_R2_REFUSED);
		return 1;
	}
	++g_r2_used; yk_event(YKE_R2_USED);
	for (int p = 0; p < P; ++p) {
		c->h_bits[p] = pl.large[p] ? pl.bitsF[p] : s.ob[p];
		c->h_count[p] = pl.large[p] ? pl.cntF[p] : s.oc[p];
	}
	if (pl.inplace) return yk_image_commit(c, std::move(A), std::move(s.img_u), pl.tot, pl.new_off);
	return yk_image_commit(c, std::move(s.nk_al), std::move(s.nu_al), pl.tot, pl.new_off);
}

/* Layout replay with the large sub-tables on the streaming kernels (kernels.hip "replay2").  A sub-table whose
 * final capacity stays within 2^SB slots is replayed by k_replay as before.  A larger one is brought to 2^SB slots
 * by k_replay (everything in LDS there), then all of them advance together, step by step: a placement of the next
 * keys up to the growth threshold, or a doubling.  The schedule is khashl's (khashl.h:202: grow BEFORE the put once
 * count >= 0.75 capacity; a trailing put-call on an existing key can still double) and is simulated on the host
 * (replay_plan.h); the kernels only move keys.  Returns 0 done, -1 error, 1 not applicable / refused (caller: k_replay). */
static int run_replay_v2(yakamd_ctx *c, const ReplayIn &in, const u64 *d_rec_kc, const u64 *d_rec_t, const u64 *d_lastput)
{
	if (env_i64("YAKAMD_REPLAY2", 1) == 0 || in.P > 65536) return 1;
	Replay2 s;
	s.c = c; s.d_rec_kc = d_rec_kc; s.d_rec_t = d_rec_t; s.d_lastput = d_lastput;
	int r;
	if ((r = r2_plan(s, in)) != 0) return r;
	if ((r = r2_small_part(s)) != 0) return r;
	if ((r = r2_buffers(s)) != 0) return r;
	r2_steps(s);
	return r2_publish_commit(s);
}

/* rebuild the image from per-sub-table ordered record lists.  rec_t/lastput may be NULL (shrink) */
int yk_run_replay(yakamd_ctx *c, const std::vector<u32> &m, const u64 *d_rec_kc, const u64 *d_rec_t,
                  const u64 *d_lastput, const std::vector<u32> *init_bits, bool from_empty, const std::vector<u64> *rec_off)
{
	const int P = c->P;
	if (yk_image_settle(c)) return -1;                           /* k_replay and k_r2_load read the old image's keys as they are (c->d_keys) */
	const ReplayIn in = { P, c->h_bits.data(), c->h_count.data(), c->h_off.data(), m.data(), init_bits ? init_bits->data() : 0, rec_off ? rec_off->data() : 0, from_empty, d_lastput != 0 };
	{
		const int r2 = run_replay_v2(c, in, d_rec_kc, d_rec_t, d_lastput);
		if (r2 <= 0) return r2;
	}
	ReplayPlan pl;                                               /* k_replay alone: every sub-table in the final arena */
	pl.classify(in, ReplayPlan::SB_NONE, (u32)env_i64("YAKAMD_DBG", 0));
	const u64 tot = pl.tot;
	DevBuf<u32> nu; DevBuf<u64> nk; DevBuf<u32> d_oc, d_ob; DevBuf<ReplayTask> d_tasks; DevBuf<u64> sp; DevBuf<u32> so, su;   /* nk / nu are handed to the context on success */
	const bool par = env_i64("YAKAMD_PAR_REPLAY", 1) != 0;
	if ((par && sp.alloc(2 * tot)) || nk.alloc(tot) || nu.alloc(tot / 32) || su.alloc(tot / 32) || so.alloc(tot) ||
	    d_tasks.alloc(P) || d_ob.alloc(P) || d_oc.alloc(P)) return -1;
	HIPCK(hipMemsetAsync(nk, 0xff, tot * 8, c->st));
	HIPCK(hipMemsetAsync(nu, 0, tot / 8, c->st));
	HIPCK(hipMemcpyAsync(d_tasks, pl.tasks.data(), P * sizeof(ReplayTask), hipMemcpyHostToDevice, c->st));
	legacy_replay_launch(c, pl.tasks, d_tasks, nk, nu, su, so, sp, d_rec_kc, d_rec_t, d_lastput, d_ob, d_oc);
	if (env_i64("YAKAMD_DBG", 0) & 32) {
		HIPCK(hipStreamSynchronize(c->st));
		u64 pr[8]; yk_replay_prof(pr);
		fprintf(stderr, "[yak_amd] replay block 0 (100 MHz ticks): double<32K %llu, double>=32K %llu, place<32K %llu, place>=32K %llu, publish %llu | par doubling: setup+base %llu, rounds %llu, verify+commit %llu\n",
		        (unsigned long long)pr[0], (unsigned long long)pr[1], (unsigned long long)pr[2], (unsigned long long)pr[3], (unsigned long long)pr[4],
		        (unsigned long long)pr[5], (unsigned long long)pr[6], (unsigned long long)pr[7]);
	}
	HIPCK(hipMemcpyAsync(c->h_bits.data(), d_ob, P * 4, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipMemcpyAsync(c->h_count.data(), d_oc, P * 4, hipMemcpyDeviceToHost, c->st));
	HIPCK(hipStreamSynchronize(c->st));
	return yk_image_commit(c, std::move(nk), std::move(nu), tot, pl.new_off);
}

void yk_replay_counters(u32 *used, u32 *refused) { *used = g_r2_used; *refused = g_r2_refused; }
