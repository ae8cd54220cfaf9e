/* replay_plan.h -- the host plan of the exact-layout stage (layout.cpp; DESIGN.md section 4, "Streaming replay"): the parameter blocks its kernels
 * read, khashl's growth schedule, and everything the stage decides before a kernel runs -- which sub-tables go to the streaming kernels, their
 * doubling / placement actions, the arena mode and every offset into the arenas.  Plain C++: no HIP, no device, no library state, so that
 * tests/tools/replay_plan_check.cpp can hold it to a put-by-put model of khashl on the CPU. */
#ifndef YK_REPLAY_PLAN_H
#define YK_REPLAY_PLAN_H
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

typedef unsigned long long u64;
typedef unsigned int u32;

#define YK_NOCAP   0xFFFFFFFFu               /* sub-table without a slot array (kh_capacity == 0) */

/* parameters of one replay task (one sub-table) */
struct ReplayTask {
	u32 old_bits, old_count;
	u64 old_off;        /* slot offset in the old arena */
	u64 new_off;        /* slot offset in the new arena (multiple of 32) */
	u64 rec_off;        /* first record of this sub-table's sorted new keys */
	u32 m;              /* number of new keys */
	u32 init_bits;      /* pre-sized empty table (shrink), YK_NOCAP otherwise */
	u32 cap_max_bits;   /* room reserved in the new arena */
	u32 dbg;
};

/* replay2 (layout replay of large sub-tables, kern_replay2.inc) */
struct R2Tab { u64 off, rec_off; };
struct R2Act { u32 kind, bits, i0, batch, src, seg0, pad0, pad1; };
struct R2Load { u64 src_off; u32 bits, from_src, dst, pad; };
struct R2Pub { u64 new_off; u32 bits, src; };

/* One step of khashl's growth (khashl.h:197-221) on a table of `cap` slots and `cnt` keys with `rem` > 0 keys still to put: the table grows BEFORE a
 * put once cnt >= 0.75 cap.  Either it doubles now (yk_grow_cap), or the next `batch` > 0 keys are put at this capacity */
struct GrowStep { bool grow; u64 batch; };
static inline GrowStep yk_grow_step(u64 cap, u64 cnt, u64 rem)
{
	const u64 thr = (cap >> 1) + (cap >> 2);
	if (cnt >= thr) return GrowStep{ true, 0 };
	return GrowStep{ false, std::min(rem, thr - cnt) };
}
static inline u64 yk_grow_cap(u64 cap) { return cap ? cap << 1 : 4; }
static inline u32 yk_cap_bits(u64 cap) { u32 b = 0; while ((1ull << b) < cap) ++b; return cap ? b : YK_NOCAP; }

/* capacity after `m` new keys on a table of (cap, cnt), plus one possible trailing doubling (a put-call on an existing key can still grow the table) */
static inline u32 yk_plan_cap(u32 cap, u32 cnt, u32 m, bool may_trail)
{
	u64 n = cap, c = cnt, rem = m;
	while (rem > 0) {
		const GrowStep g = yk_grow_step(n, c, rem);
		if (g.grow) { n = yk_grow_cap(n); continue; }
		c += g.batch; rem -= g.batch;
	}
	if (may_trail && yk_grow_step(n, c, 1).grow) n = yk_grow_cap(n);
	return (u32)n;
}

/* what classify() is told about the P sub-tables: the old image (bits YK_NOCAP = no slot array; ignored with from_empty), m[p] new keys each, sorted
 * by put time from record rec_off[p] on (rec_off == 0: one behind the other), init_bits (0, or per sub-table the pre-sized empty table of a shrink) */
struct ReplayIn {
	int P;
	const u32 *old_bits, *old_count; const u64 *old_off;
	const u32 *m, *init_bits; const u64 *rec_off;
	bool from_empty, has_lastput;
};

struct ReplayPlan {
	enum { SB_NONE = 32 };               /* classify(): no sub-table is large (every capacity fits 32 bits) */
	int P = 0; u32 SB = 0;
	/* classify(): the final arena -- sub-table p has max(32, capm[p]) slots at new_off[p], tot in all -- k_replay's tasks on it, and the sub-tables that
	 * outgrow 2^SB slots (`large`: the streaming kernels') */
	std::vector<ReplayTask> tasks;
	std::vector<u64> rec_off, new_off;
	std::vector<u32> m, cap0, cnt0, capm;
	std::vector<char> large;
	u64 tot = 0; u32 n_large = 0;
	/* schedule(), per large sub-table: k_replay puts the first m1 keys and leaves (bitsS, cntS); the actions acts[k * P + p], k < n_act[p], lead to
	 * (bitsF, cntF); seg0 = its first placement segment */
	std::vector<u32> m1, bitsS, cntS, bitsF, cntF, seg0, n_act;
	std::vector<R2Act> acts; size_t n_steps = 0;
	std::vector<R2Tab> tabs; std::vector<R2Load> ld; std::vector<R2Pub> pub;
	std::vector<char> pub_needed;        /* 0: the last step's kernels already wrote the sub-table's "used" bits (R2Act.pad0) */
	/* the arena mode.  only_side: k_replay works in the side arena [tot, tot_ext) alone, its scratch is addressed from scr_lo = tot on.  inplace: on top
	 * of that the two work buffers are laid out like the arena and buffer img_is1 BECOMES the image; nk / nu hold the side arena only (nk_lo = tot) */
	bool only_side = false, inplace = false, img_is1 = false;
	u64 tot_ext = 0, scr_lo = 0, nk_lo = 0, tot2 = 0, nseg_tot = 0, n_keys = 0;
	u32 bmaxS = 0, bmaxF = 0;
	char err[160] = { 0 };               /* the text of schedule()'s -1 */

	u64 side_slots() const { return std::max<u64>(32, 1ull << SB); }   /* a large sub-table's room in the side arena */

	/* Runs before any device work.  Returns whether any sub-table is large */
	bool classify(const ReplayIn &in, u32 sb, u32 dbg)
	{
		P = in.P; SB = sb;
		tasks.resize(P); rec_off.resize(P); new_off.resize(P); m.assign(in.m, in.m + P); cap0.resize(P); cnt0.resize(P); capm.resize(P); large.assign(P, 0);
		tot = 0; n_large = 0;
		u64 rec = 0;
		for (int p = 0; p < P; ++p) {
			ReplayTask &t = tasks[p];
			t.old_bits = in.from_empty ? YK_NOCAP : in.old_bits[p];
			t.old_count = cnt0[p] = in.from_empty ? 0 : in.old_count[p];
			t.old_off = in.old_off[p];
			t.rec_off = rec_off[p] = in.rec_off ? in.rec_off[p] : rec; rec += m[p];
			t.m = m[p];
			t.init_bits = in.init_bits ? in.init_bits[p] : YK_NOCAP;
			cap0[p] = t.old_bits == YK_NOCAP ? 0 : 1u << t.old_bits;
			if (cap0[p] == 0 && t.init_bits != YK_NOCAP) cap0[p] = 1u << t.init_bits;
			capm[p] = yk_plan_cap(cap0[p], cnt0[p], m[p], in.has_lastput);
			t.cap_max_bits = capm[p] ? yk_cap_bits(capm[p]) : 0;
			t.dbg = dbg;
			t.new_off = new_off[p] = tot; tot += std::max<u64>(32, capm[p]);
			large[p] = capm[p] > (1ull << SB);
			n_large += large[p];
		}
		return n_large != 0;
	}

	/* trail[p] != 0 (trail == 0: none): a put-call on an existing key follows sub-table p's last new key, and doubles the table if it is due.  The
	 * tasks of the large sub-tables become their k_replay part, in the side arena.  0; 1: not applicable (a sub-table of more than 1024 placement
	 * segments of 2^SEGLOG slots); -1: `err` */
	int schedule(const u32 *trail, int SEGLOG)
	{
		const u64 SMALLCAP = 1ull << SB;
		m1.assign(P, 0); bitsS.assign(P, YK_NOCAP); cntS.assign(P, 0); bitsF.assign(P, YK_NOCAP); cntF.assign(P, 0); seg0.assign(P, 0); n_act.assign(P, 0);
		tabs.resize(P); ld.resize(P); pub.resize(P); pub_needed.assign(P, 1);
		acts.clear(); n_steps = 0; nseg_tot = 0; n_keys = 0; bmaxS = bmaxF = 0; tot2 = 0;
		u64 side = tot;
		for (int p = 0; p < P; ++p) {
			n_keys = std::max(n_keys, rec_off[p] + m[p]);
			tabs[p].off = tot2; tabs[p].rec_off = rec_off[p];
			ld[p] = R2Load{ 0, YK_NOCAP, 0, 0, 0 };
			pub[p] = R2Pub{ new_off[p], YK_NOCAP, 0 };
			if (!large[p]) continue;
			u64 cap = cap0[p], cnt = cnt0[p], rem = m[p];
			const bool beyond = cap0[p] > SMALLCAP;                   /* already out of k_replay's reach: loaded straight from the old image */
			while (!beyond && rem > 0) {                               /* the part k_replay does: up to a full table of SMALLCAP slots */
				const GrowStep g = yk_grow_step(cap, cnt, rem);
				if (g.grow) { if (cap >= SMALLCAP) break; cap = yk_grow_cap(cap); continue; }
				cnt += g.batch; rem -= g.batch;
			}
			m1[p] = (u32)(m[p] - rem); bitsS[p] = yk_cap_bits(cap); cntS[p] = (u32)cnt;
			seg0[p] = (u32)nseg_tot;
			u32 src = 0, k = 0;                                        /* the doublings alternate between the two work buffers */
			for (bool more = true; more;) {
				const GrowStep g = yk_grow_step(cap, cnt, std::max<u64>(rem, 1));
				if (rem == 0) { if (!(trail && trail[p] && g.grow)) break; more = false; }   /* the trailing doubling */
				if (acts.size() < (size_t)(k + 1) * P) acts.resize((size_t)(k + 1) * P);   /* (a sub-table without an action in a step: zeros) */
				R2Act &a = acts[(size_t)k++ * P + p];
				a.bits = yk_cap_bits(cap); a.src = src; a.seg0 = seg0[p];
				if (g.grow) { a.kind = 2; cap = yk_grow_cap(cap); src ^= 1; }
				else { a.kind = 1; a.i0 = (u32)(m[p] - rem); a.batch = (u32)g.batch; cnt += g.batch; rem -= g.batch; }
			}
			n_act[p] = k; n_steps = std::max<size_t>(n_steps, k);
			bitsF[p] = yk_cap_bits(cap); cntF[p] = (u32)cnt;
			if ((1ull << bitsF[p]) > capm[p]) return error("replay schedule exceeds the planned capacity");
			tot2 += 1ull << bitsF[p];
			nseg_tot += (bitsF[p] > (u32)SEGLOG ? 1ull << (bitsF[p] - SEGLOG) : 1) + 1;
			bmaxF = std::max(bmaxF, bitsF[p]); bmaxS = std::max(bmaxS, bitsS[p]);
			ReplayTask &t = tasks[p];
			ld[p].bits = bitsS[p];
			if (beyond) {
				const bool old = t.old_bits != YK_NOCAP;
				ld[p].from_src = old ? 2 : 0; ld[p].src_off = old ? t.old_off : 0;
				t.old_bits = YK_NOCAP; t.old_count = 0; t.m = 0; t.init_bits = YK_NOCAP; t.cap_max_bits = 0;
			} else {
				ld[p].from_src = 1; ld[p].src_off = side;
				t.m = m1[p]; t.cap_max_bits = SB;
			}
			t.new_off = side; side += side_slots();
			pub[p].bits = bitsF[p]; pub[p].src = src;
		}
		acts.resize(std::max<size_t>(1, n_steps) * P);
		for (int p = 0; p < P; ++p) if (large[p] && (int)bitsF[p] - SEGLOG > 10) return 1;
		tot_ext = tot + (u64)n_large * side_slots();
		/* k_replay's scratch arrays (ranks, second bitmap, doubling lists: 28 bytes per slot) are indexed by arena offsets.  When every sub-table it
		 * touches is a large one -- an assembly, any pass of a big count -- it only works in the side arena behind the final one, so the arrays
		 * cover that alone and are addressed from `tot` on: at 2 G keys they were 85 GB that nothing touched, more than the pool could keep, and the
		 * hipMalloc / hipFree of them cost 5 s per pass (the kernels of the whole layout stage: 0.28 s) */
		only_side = true;
		for (int p = 0; p < P; ++p) if (!large[p] && (m[p] || cap0[p])) only_side = false;
		scr_lo = only_side ? tot : 0;
		if (only_side) {
			/* the scratch pointers handed to k_replay are shifted by scr_lo: that is only sound while the kernel touches no scratch below `tot`,
			 * i.e. while every task outside the side arena is an empty one, and while bitmap words of the two arenas do not straddle */
			if (tot % 32 != 0) return error("replay: arena size %llu is not a multiple of 32", tot);
			for (int p = 0; p < P; ++p)
				if (!large[p] && (tasks[p].m != 0 || tasks[p].old_count != 0 || cap0[p] != 0)) return error("replay: sub-table %d is not empty but lies outside the side arena", p);
		}
		/* Every sub-table that holds anything is a large one and ends at the capacity the arena reserves for it (no trailing doubling left out): the
		 * two buffers the doublings alternate between are then laid out exactly like the arena, and whichever holds most of the final tables BECOMES the
		 * table image -- the others' tables are copied over, nothing else is (the copy of every slot into a third array was 12 ms and 34 GB beside a
		 * 2 Gb assembly).  k_replay's side arena is then all that `nk` / `nu` hold; they are addressed from `tot` on like its scratch */
		inplace = only_side;
		for (int p = 0; p < P && inplace; ++p) if (large[p] && (1ull << bitsF[p]) != std::max<u64>(32, capm[p])) inplace = false;
		nk_lo = inplace ? tot : 0;
		img_is1 = false;
		if (!inplace) return 0;
		/* the buffer that becomes the image, known before anything runs: a sub-table that ends there with a placement gets its "used" bits from that
		 * step's kernels (R2Act.pad0) and needs no pass of k_r2_publish */
		u64 in1 = 0, in0 = 0;
		for (int p = 0; p < P; ++p) if (large[p]) (pub[p].src ? in1 : in0) += 1ull << bitsF[p];
		img_is1 = in1 > in0;
		for (int p = 0; p < P; ++p) {
			tabs[p].off = new_off[p];                                 /* the buffers are arenas */
			if (!large[p] || n_act[p] == 0) continue;
			R2Act &last = acts[(size_t)(n_act[p] - 1) * P + p];
			if (last.kind != 1 || (pub[p].src != 0) != img_is1) continue;
			last.pad0 = 1; pub_needed[p] = 0;
		}
		tot2 = tot;
		return 0;
	}

private:
	int error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(err, sizeof err, fmt, ap); va_end(ap); return -1; }
};
#endif
