/* replay_plan_check.cpp -- the host plan of the layout replay (yak_amd/csrc/replay_plan.h: which sub-tables go to the streaming kernels, their doubling /
 * placement schedule, the arena mode and every offset the kernels are handed) against a literal put-by-put model of khashl's growth, as a program of its
 * own so that the plan runs on the CPU, and under the sanitizers:
 *     g++ -std=c++17 -O1 -Wall tests/tools/replay_plan_check.cpp -o /tmp/replay_plan_check && /tmp/replay_plan_check
 *     g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/tools/replay_plan_check.cpp -o /tmp/replay_plan_check && /tmp/replay_plan_check
 * The model, per new key: while count >= (cap >> 1) + (cap >> 2) the table doubles (none: 4 slots); then count++.  After the last key one more doubling
 * iff a put-call on an existing key follows (`trail`) and the threshold is reached.
 * Prints "ok" and returns 0 when every case keeps every invariant; a plan that does not come to an end is stopped by alarm(). */
#include <signal.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include <set>
#include <vector>
#include "../../yak_amd/csrc/replay_plan.h"

static const int P = 4;
static int n_bad = 0, n_cases = 0, n_mode[3];                /* cases seen as mixed, side-arena-only, in place */
static char what[256];                                       /* the running case, for the report */

#define CHECK(cond) do { if (!(cond)) { if (++n_bad <= 20) fprintf(stderr, "FAILED %s: %s (line %d)\n", what, #cond, __LINE__); return; } } while (0)

static u64 thr_of(u64 cap) { return (cap >> 1) + (cap >> 2); }
static u32 lg(u64 cap) { u32 b = 0; while ((1ull << b) < cap) ++b; return b; }

struct Model { std::vector<u64> cap_of; u64 cap, cnt; };    /* the capacity each key is put at; the end state */
static Model model(u64 cap, u64 cnt, u32 m, bool trail)
{
	Model r;
	for (u32 i = 0; i < m; ++i) {
		while (cnt >= thr_of(cap)) cap = cap ? cap << 1 : 4;
		r.cap_of.push_back(cap); ++cnt;
	}
	if (trail && cnt >= thr_of(cap)) cap = cap ? cap << 1 : 4;
	r.cap = cap; r.cnt = cnt;
	return r;
}

struct Sub { u32 cap0, cnt0, m; bool by_init, trail; };      /* by_init: cap0 comes from init_bits (a pre-sized empty table), not from the old image */

/* expect: 0 a plan; 1 "not applicable" (the segment limit) */
static void run_case(u32 SB, const Sub *sub, bool from_empty, bool has_lastput, bool given_rec_off, int SEGLOG, int expect)
{
	++n_cases;
	const u64 SMALL = 1ull << SB, SIDE = std::max<u64>(32, SMALL);
	u32 ob[P], oc[P], ib[P], m[P], trail[P]; u64 oo[P], ro[P];
	bool any_init = false;
	for (int p = 0; p < P; ++p) {
		const Sub &s = sub[p];
		const bool from_old = !s.by_init && !from_empty && s.cap0;
		ob[p] = from_old ? lg(s.cap0) : from_empty ? 7 : YK_NOCAP;   /* from_empty: the old image is to be ignored, whatever it says */
		oc[p] = from_old ? s.cnt0 : from_empty ? 9 : 0;
		oo[p] = 1000 + 64 * p;
		ib[p] = s.by_init && s.cap0 ? lg(s.cap0) : YK_NOCAP;
		any_init = any_init || s.by_init;
		m[p] = s.m; trail[p] = has_lastput && s.trail;
		ro[p] = 5000 - 1000 * p;                                  /* any order will do when the offsets are given */
	}
	const ReplayIn in = { P, ob, oc, oo, m, any_init ? ib : 0, given_rec_off ? ro : 0, from_empty, has_lastput };
	ReplayPlan pl;
	const bool any = pl.classify(in, SB, 77);
	/* what the model says of every sub-table */
	Model md[P]; u64 cap0[P], cnt0[P], capm[P]; bool large[P]; u32 n_large = 0;
	u64 tot = 0, rec = 0, n_keys = 0;
	for (int p = 0; p < P; ++p) {
		cap0[p] = (sub[p].by_init || !from_empty) ? sub[p].cap0 : 0;
		cnt0[p] = (sub[p].by_init || from_empty) ? 0 : sub[p].cnt0;
		capm[p] = model(cap0[p], cnt0[p], m[p], has_lastput).cap;   /* the arena reserves the trailing doubling wherever one may come */
		md[p] = model(cap0[p], cnt0[p], m[p], trail[p] != 0);
		large[p] = capm[p] > SMALL; n_large += large[p];
		const ReplayTask &t = pl.tasks[p];
		CHECK(pl.capm[p] == capm[p] && pl.large[p] == (char)large[p] && pl.cap0[p] == cap0[p] && pl.cnt0[p] == cnt0[p]);
		CHECK(pl.new_off[p] == tot && tot % 32 == 0);
		CHECK(t.old_bits == (from_empty ? YK_NOCAP : ob[p]) && t.old_count == cnt0[p] && t.old_off == oo[p] && t.init_bits == ib[p] && t.dbg == 77);
		CHECK(t.rec_off == (given_rec_off ? ro[p] : rec) && pl.rec_off[p] == t.rec_off && t.m == m[p] && t.new_off == tot);
		CHECK(t.cap_max_bits == (capm[p] ? lg(capm[p]) : 0));
		tot += std::max<u64>(32, capm[p]); rec += m[p];
		n_keys = std::max<u64>(n_keys, t.rec_off + m[p]);
	}
	CHECK(pl.tot == tot && pl.n_large == n_large && any == (n_large != 0));
	if (!any) return;
	const std::vector<ReplayTask> tasks0 = pl.tasks;
	const int r = pl.schedule(has_lastput ? trail : 0, SEGLOG);
	CHECK(r == expect);
	if (r) return;
	bool only_side = true, inplace = true;
	for (int p = 0; p < P; ++p) {
		if (!large[p] && (m[p] || cap0[p])) only_side = false;
		if (large[p] && md[p].cap != std::max<u64>(32, capm[p])) inplace = false;
	}
	inplace = inplace && only_side;
	CHECK(pl.only_side == only_side && pl.inplace == inplace);
	++n_mode[inplace ? 2 : only_side ? 1 : 0];
	CHECK(pl.tot_ext == tot + n_large * SIDE && pl.scr_lo == (only_side ? tot : 0) && pl.nk_lo == (inplace ? tot : 0) && pl.n_keys == n_keys);
	CHECK(pl.acts.size() == std::max<size_t>(1, pl.n_steps) * P);
	u64 side = tot, sum2 = 0, nseg = 0, in_buf[2] = { 0, 0 };
	size_t n_steps = 0; u32 bmaxS = 0, bmaxF = 0, src_end[P];
	for (int p = 0; p < P; ++p) {
		const ReplayTask &t = pl.tasks[p];
		CHECK(pl.tabs[p].rec_off == tasks0[p].rec_off && pl.tabs[p].off == (inplace ? pl.new_off[p] : sum2));
		if (!large[p]) {
			for (size_t k = 0; k < pl.n_steps; ++k) CHECK(pl.acts[k * P + p].kind == 0 && pl.acts[k * P + p].pad0 == 0);
			CHECK(pl.n_act[p] == 0 && pl.ld[p].bits == YK_NOCAP && pl.pub[p].bits == YK_NOCAP && pl.pub[p].new_off == pl.new_off[p]);
			CHECK(memcmp(&t, &tasks0[p], sizeof t) == 0);
			continue;
		}
		/* the k_replay part: the first m1 keys, into the side arena */
		const bool beyond = cap0[p] > SMALL;
		const u32 m1 = pl.m1[p];
		const Model ms = model(cap0[p], cnt0[p], m1, false);
		CHECK(m1 <= m[p] && ms.cap == 1ull << pl.bitsS[p] && ms.cnt == pl.cntS[p]);
		CHECK(beyond ? m1 == 0 : pl.bitsS[p] <= SB);
		CHECK(beyond || m1 == m[p] || (ms.cap == SMALL && ms.cnt >= thr_of(SMALL)));   /* k_replay stops at a full table of 2^SB slots, not before */
		CHECK(t.new_off == side && t.rec_off == tasks0[p].rec_off && t.old_off == oo[p] && t.dbg == 77);
		if (beyond) {
			const bool old = !from_empty && ob[p] != YK_NOCAP;
			CHECK(t.m == 0 && t.old_bits == YK_NOCAP && t.old_count == 0 && t.init_bits == YK_NOCAP && t.cap_max_bits == 0);
			CHECK(pl.ld[p].from_src == (old ? 2u : 0u) && pl.ld[p].src_off == (old ? oo[p] : 0));
		} else {
			CHECK(t.m == m1 && t.cap_max_bits == SB && t.old_bits == tasks0[p].old_bits && t.old_count == cnt0[p] && t.init_bits == ib[p]);
			CHECK(pl.ld[p].from_src == 1 && pl.ld[p].src_off == side);
		}
		CHECK(pl.ld[p].bits == pl.bitsS[p] && pl.ld[p].dst == 0 && pl.ld[p].pad == 0);
		side += SIDE;
		/* the actions: placements tile [m1, m), each key at the model's capacity; src flips at a doubling and nowhere else */
		u32 next = m1, src = 0; u64 cap = ms.cap;
		CHECK(pl.seg0[p] == nseg);
		for (u32 k = 0; k < pl.n_steps; ++k) {
			const R2Act &a = pl.acts[(size_t)k * P + p];
			if (k >= pl.n_act[p]) { CHECK(a.kind == 0 && a.pad0 == 0); continue; }
			CHECK((a.kind == 1 || a.kind == 2) && a.src == src && a.seg0 == nseg && a.bits == lg(cap) && a.pad1 == 0);
			if (a.kind == 2) { CHECK(a.i0 == 0 && a.batch == 0 && a.pad0 == 0); cap <<= 1; src ^= 1; continue; }
			CHECK(a.i0 == next && a.batch > 0 && (u64)next + a.batch <= m[p]);
			for (u32 i = next; i < next + a.batch; ++i) CHECK(md[p].cap_of[i] == cap);
			next += a.batch;
		}
		CHECK(next == m[p] && cap == md[p].cap);
		CHECK(1ull << pl.bitsF[p] == md[p].cap && pl.cntF[p] == md[p].cnt && md[p].cap <= capm[p]);
		CHECK(pl.pub[p].bits == pl.bitsF[p] && pl.pub[p].src == src && pl.pub[p].new_off == pl.new_off[p]);
		src_end[p] = src; in_buf[src] += md[p].cap;
		sum2 += md[p].cap;
		nseg += (pl.bitsF[p] > (u32)SEGLOG ? 1ull << (pl.bitsF[p] - SEGLOG) : 1) + 1;
		n_steps = std::max<size_t>(n_steps, pl.n_act[p]);
		bmaxS = std::max(bmaxS, pl.bitsS[p]); bmaxF = std::max(bmaxF, pl.bitsF[p]);
	}
	CHECK(pl.n_steps == n_steps && pl.nseg_tot == nseg && pl.bmaxS == bmaxS && pl.bmaxF == bmaxF && pl.tot2 == (inplace ? tot : sum2));
	/* the buffer that becomes the image holds the larger slot total; a sub-table that ends there with a placement has its bitmap written by that step */
	CHECK(pl.img_is1 == (inplace && in_buf[1] > in_buf[0]));
	for (int p = 0; p < P; ++p) {
		if (!large[p]) { CHECK(pl.pub_needed[p] == 1); continue; }
		bool pad = false;
		for (u32 k = 0; k < pl.n_act[p]; ++k) {
			const R2Act &a = pl.acts[(size_t)k * P + p];
			const bool want = inplace && k + 1 == pl.n_act[p] && a.kind == 1 && (src_end[p] != 0) == pl.img_is1;
			CHECK(a.pad0 == (want ? 1u : 0u));
			pad = pad || want;
		}
		CHECK(pl.pub_needed[p] == (pad ? 0 : 1));
	}
}

static void on_alarm(int) { static const char msg[] = "FAILED: the plan does not come to an end\n"; if (write(2, msg, sizeof msg - 1)) {} _exit(1); }

int main(void)
{
	signal(SIGALRM, on_alarm);
	alarm(120);
	const Sub none = { 0, 0, 0, false, false };
	for (u32 SB = 5; SB <= 6; ++SB) {
		std::vector<u32> caps(1, 0);
		for (u32 c = 4; c <= (4u << SB); c <<= 1) caps.push_back(c);
		for (u32 cap0 : caps) for (int ci = 0; ci < 3; ++ci) {
			const u32 thr = (u32)thr_of(cap0), cnt0 = ci == 0 ? 0 : ci == 1 ? thr - 1 : thr;
			if (ci && (cap0 == 0 || (ci == 1 && cnt0 == 0))) continue;
			std::set<u32> ms;
			for (u32 i = 0; i <= 60; ++i) ms.insert(i);
			for (u64 c = 4; thr_of(c) <= 400; c <<= 1) for (int d = -1; d <= 1; ++d) { const long long v = (long long)thr_of(c) + d - cnt0; if (v >= 0) ms.insert((u32)v); }
			ms.insert(400);
			for (u32 m : ms) for (int tr = 0; tr < 3; ++tr) for (int how = 0; how < 3; ++how) {
				if (how && cnt0) continue;                           /* a table from init_bits is an empty one */
				const bool has_lp = tr != 0, from_empty = how == 2;
				const Sub v = { cap0, cnt0, m, how != 0, tr == 2 };
				const Sub small = { 4, 1, 2, false, true }, big = { 4u << SB, 3u << SB, 5, false, true }, grown = { 0, 0, 100, false, false };
				snprintf(what, sizeof what, "SB %u cap0 %u cnt0 %u m %u trail %d init/from_empty %d", SB, cap0, cnt0, m, tr, how);
				const Sub alone[P] = { none, v, none, v }, mixed[P] = { small, v, none, big }, two[P] = { v, none, grown, none };
				run_case(SB, alone, from_empty, has_lp, false, 3, 0);
				run_case(SB, mixed, from_empty, has_lp, true, 4, 0);
				run_case(SB, two, from_empty, has_lp, false, 2, 0);
			}
		}
	}
	if (!n_mode[0] || !n_mode[1] || !n_mode[2]) { fprintf(stderr, "FAILED: arena modes seen: mixed %d, side arena only %d, in place %d\n", n_mode[0], n_mode[1], n_mode[2]); ++n_bad; }
	{	/* more than 1024 placement segments in a sub-table: not applicable, and 1024 still is */
		const Sub at = { 0, 0, 767, false, false }, over = { 0, 0, 769, false, false };
		const Sub a[P] = { none, at, none, none }, b[P] = { none, at, over, none };
		snprintf(what, sizeof what, "the segment limit");
		run_case(5, a, false, false, false, 0, 0);
		run_case(5, b, false, false, false, 0, 1);
	}
	{	/* SB_NONE: nothing is large, whatever its size */
		const u32 nb[P] = { YK_NOCAP, 3, YK_NOCAP, 20 }, nc[P] = { 0, 5, 0, 700000 }, nm[P] = { 1000, 0, 0, 90000 }; const u64 no[P] = { 0, 32, 64, 96 };
		const ReplayIn in = { P, nb, nc, no, nm, 0, 0, false, true };
		ReplayPlan pl;
		if (pl.classify(in, ReplayPlan::SB_NONE, 0) || pl.n_large || pl.capm[0] != 2048 || pl.capm[3] != 2u << 20 || pl.tot != 2048 + 32 + 32 + (2u << 20)) { fprintf(stderr, "FAILED: SB_NONE\n"); ++n_bad; }
	}
	if (n_bad) { fprintf(stderr, "%d of %d cases failed\n", n_bad, n_cases); return 1; }
	puts("ok");
	return 0;
}
