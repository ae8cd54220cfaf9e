/* count_plan_check.cpp -- the plan of a count into existing keys (yak_amd/csrc/count_plan.h) against the cascade of engine_pass.cpp it replaced,
 * restated here as it stood: consume_records' count half with count_own, count_own_plan, count_lds_bytes and the conditions of count_by_ranges, in
 * their order, the refusal of the records that only the key-owning kernel reads, feed_image's choice of the consumed format, yakamd_count_retained's
 * test, and the two LDS size formulas of kern_launch.inc.  A few thousand random tables and settings, and hand cases at every limit; a program of
 * its own (tests/test_count_plan.py builds it with the address and undefined-behaviour sanitizers); prints `ok`. */
#include <stdio.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../yak_amd/csrc/count_plan.h"

static int g_bad = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { if (g_bad < 20) fprintf(stderr, "%s:%d: %s does not hold (case %d)\n", __FILE__, __LINE__, #x, g_case); ++g_bad; } } while (0)

/* ---- the old code: the context's fields it read, the settings it read through env_i64 / yk_rng_log, and what it then did ---- */
struct Ctx { int nb_bits, pre, k, plo, phi; std::vector<u32> h_bits, h_count; };
struct Env { int64_t COUNT_OWN, OWN_LDS, OWN_MAXRB, COUNT_LDS, COUNT_RNG, YTAG; int rng_log; };   /* rng_log: yk_rng_log(), YAKAMD_RNG_LOG clamped to 5..16 */
enum Did { NOTHING, OWN, RANGES, LDS, ATOMICS, FAILED };
struct Outcome { Did did; int rng_log, rb; u32 kmax, max_len, ck_stride; size_t lds; };

static size_t old_img_count_lds_bytes(u32 cap, u32 count) { return (size_t)((cap + 31) / 32) * 8 + (size_t)(count + 1) / 2 * 4 + 16; }
static size_t old_count_own_lds(u32 range_len, u32 kmax) { const u32 nw = (range_len + 31) / 32; return (size_t)2 * ((nw + 1) & ~1u) * 4 + (size_t)kmax * 8 + (size_t)(((kmax + 1) / 2 + 1) & ~1u) * 4 + 16 * 128 * 8 + 16; }

static size_t old_count_lds_bytes(const Ctx *c, const Env &env)
{
	size_t lds = 0;
	if (c->nb_bits != c->pre || env.COUNT_LDS == 0) return 0;
	for (int p = c->plo; p < c->phi; ++p)
		if (c->h_bits[p] != YK_NOCAP) lds = std::max(lds, old_img_count_lds_bytes(1u << c->h_bits[p], c->h_count[p]));
	return lds > 150 * 1024 ? 0 : lds;
}

/* 1 = not applicable, 0 = go (rb == -1: no sub-table has a slot) */
static int old_count_own_plan(const Ctx *c, const Env &env, int *rng_log_out, int *rb_out, u32 *kmax_out)
{
	if (env.COUNT_OWN == 0 || c->nb_bits != c->pre) return 1;
	const size_t budget = (size_t)env.OWN_LDS;
	u32 bmax = 0;
	for (int p = c->plo; p < c->phi; ++p) if (c->h_bits[p] != YK_NOCAP) bmax = std::max(bmax, c->h_bits[p]);
	*rng_log_out = 0; *rb_out = -1; *kmax_out = 0;
	if (bmax == 0) return 0;
	int rng_log = -1; u32 kmax = 0;
	for (int rl = (int)bmax; rl >= 5 && rng_log < 0; --rl) {
		u32 km = 1;
		for (int p = c->plo; p < c->phi; ++p) {
			if (c->h_bits[p] == YK_NOCAP) continue;
			const int rbp = (int)c->h_bits[p] > rl ? (int)c->h_bits[p] - rl : 0;
			const u32 e = (c->h_count[p] + (1u << rbp) - 1) >> rbp;
			km = std::max(km, rbp ? e + e / 8 + 192 : c->h_count[p]);
		}
		if (old_count_own_lds(1u << rl, km) <= budget) { rng_log = rl; kmax = km; }
	}
	const int rb = rng_log < 0 ? 99 : (int)bmax - rng_log;
	if (rb > (int)env.OWN_MAXRB) return 1;
	*rng_log_out = rng_log; *rb_out = rb; *kmax_out = kmax;
	return 0;
}

static bool old_own_count_only(RecFmt fmt) { return fmt == YK_FMT_HASH_RNG || fmt == YK_FMT_TAGGED; }

/* count_own: 0 done, -1 error, 1 not applicable */
static int old_count_own(const Ctx *c, const Env &env, RecFmt fmt, Outcome *o)
{
	int rng_log, rb; u32 kmax;
	const int pl = old_count_own_plan(c, env, &rng_log, &rb, &kmax);
	if (pl) { if (old_own_count_only(fmt)) { o->did = FAILED; return -1; } return 1; }   /* fail("the table changed between the extraction and the count of a pass") */
	if (rb < 0) { o->did = NOTHING; return 0; }
	o->did = OWN; o->rng_log = rng_log; o->rb = rb; o->kmax = kmax; o->lds = old_count_own_lds(1u << rng_log, kmax);   /* yk_launch_img_count_own(...) */
	return 0;
}

/* count_by_ranges: 0 done, 1 not applicable */
static int old_count_by_ranges(const Ctx *c, const Env &env, Outcome *o)
{
	u32 bmax = 0;
	for (int p = c->plo; p < c->phi; ++p) if (c->h_bits[p] != YK_NOCAP) bmax = std::max(bmax, c->h_bits[p]);
	const int rb = (int)bmax > env.rng_log ? (int)bmax - env.rng_log : 0;
	if (bmax == 0 || rb > 8) return 1;
	const u32 max_len = bmax > (u32)env.rng_log ? 1u << env.rng_log : 1u << bmax;
	o->did = RANGES; o->rb = rb; o->max_len = max_len;                          /* yk_launch_hpart2(... rb ...), yk_launch_img_count_rng(... rb, max_len ...) */
	return 0;
}

/* consume_records, !c->create_new, n_rec > 0 */
static Outcome old_consume_records(const Ctx *c, const Env &env, RecFmt fmt, bool d_bstart)
{
	Outcome o = { ATOMICS, 0, 0, 0, 0, 1, 0 };
	if (d_bstart) {
		const int r = old_count_own(c, env, fmt, &o);
		if (r <= 0 || old_own_count_only(fmt)) return o;
	}
	const size_t lds = d_bstart ? old_count_lds_bytes(c, env) : 0;
	if (!lds && d_bstart && fmt == YK_FMT_HASH && c->nb_bits == c->pre && env.COUNT_RNG != 0) {
		const int r = old_count_by_ranges(c, env, &o);
		if (r <= 0) return o;
	}
	u32 ck_stride = 1;
	if (lds) {
		for (int p = c->plo; p < c->phi; ++p) ck_stride = std::max(ck_stride, c->h_count[p]);
		o.did = LDS; o.lds = lds; o.ck_stride = ck_stride;                     /* yk_launch_img_count_lds(... lds, d_ck, ck_stride ...) */
		return o;
	}
	return o;                                                                  /* k_img_count_h / k_img_count */
}

/* feed_image: the format of a batch a count pass consumes at once */
static RecFmt old_consumed(const Ctx *c, const Env &env)
{
	RecFmt consumed = YK_FMT_HASH;
	if (c->k < 32 && c->nb_bits <= 10 && env.YTAG != 0) {
		int rl, rb; u32 km;
		if (old_count_own_plan(c, env, &rl, &rb, &km) == 0 && rb >= 0) consumed = YK_FMT_HASH_RNG;
	}
	return consumed;
}

/* ---- one case ---- */
static const RecFmt FMTS[4] = { YK_FMT_POS, YK_FMT_TAGGED, YK_FMT_HASH, YK_FMT_HASH_RNG };
static int g_seen[6];

static CountKnobs knobs_of(const Env &env)
{
	CountKnobs kn;
	kn.own = env.COUNT_OWN != 0; kn.lds_ranks = env.COUNT_LDS != 0; kn.ranges = env.COUNT_RNG != 0; kn.ytag = env.YTAG != 0;
	kn.own_lds = (size_t)env.OWN_LDS; kn.own_maxrb = (int)env.OWN_MAXRB; kn.rng_log = env.rng_log;
	return kn;
}
static CountPlan plan_of(const Ctx &c, const Env &env, RecFmt fmt, bool grouped)
{
	const CountTable t = { c.nb_bits, c.pre, c.k, c.plo, c.phi, c.h_bits.data(), c.h_count.data() };
	return count_plan(t, knobs_of(env), fmt, grouped);
}

static void one_case(const Ctx &c, const Env &env)
{
	++g_case;
	const CountTable t = { c.nb_bits, c.pre, c.k, c.plo, c.phi, c.h_bits.data(), c.h_count.data() };
	for (int f = 0; f < 4; ++f)
		for (int grouped = 0; grouped < 2; ++grouped) {
			const Outcome o = old_consume_records(&c, env, FMTS[f], grouped != 0);
			const CountPlan pl = plan_of(c, env, FMTS[f], grouped != 0);
			++g_seen[pl.path];
			switch (o.did) {
			case NOTHING: CHECK(pl.path == YK_COUNT_NOTHING); break;
			case FAILED: CHECK(pl.path == YK_COUNT_REFUSED); break;
			case OWN: CHECK(pl.path == YK_COUNT_OWN && pl.rng_log == o.rng_log && pl.rb == o.rb && pl.kmax == o.kmax && pl.lds == o.lds); break;
			case RANGES: CHECK(pl.path == YK_COUNT_RANGES && pl.rb == o.rb && pl.max_len == o.max_len); break;
			case LDS: CHECK(pl.path == YK_COUNT_LDS && pl.lds == o.lds && pl.ck_stride == o.ck_stride); break;
			case ATOMICS: CHECK(pl.path == YK_COUNT_ATOMICS); break;
			}
		}
	CHECK(count_consumed_fmt(t, knobs_of(env)) == old_consumed(&c, env));
	/* yakamd_count_retained: "count_own_plan(c, ...) != 0 -> nothing usable was retained" */
	int rl, rb; u32 km;
	CHECK((plan_of(c, env, YK_FMT_TAGGED, true).path == YK_COUNT_REFUSED) == (old_count_own_plan(&c, env, &rl, &rb, &km) != 0));
}

/* ---- the cases ---- */
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static Ctx table(int pre, u32 bits, u32 count)                                   /* every sub-table alike, level-1 buckets == sub-tables */
{
	Ctx c = { pre, pre, 31, 0, 1 << pre, std::vector<u32>((size_t)1 << pre, bits), std::vector<u32>((size_t)1 << pre, count) };
	return c;
}
static const Env DEFAULTS = { 1, 156000, 4, 1, 1, 1, 16 };

int main()
{
	/* the formulas, over the sizes the kernels are given */
	for (u32 b = 0; b <= 22; ++b)
		for (int i = 0; i < 200; ++i) {
			const u32 cap = 1u << b, n = (u32)(rnd() % (cap + 1));
			CHECK(yk_plan_img_count_lds_bytes(cap, n) == old_img_count_lds_bytes(cap, n));
			CHECK(yk_plan_count_own_lds(cap, n) == old_count_own_lds(cap, n));
		}

	/* hand cases: the equality with the old code, and what each must come to */
	{   /* no sub-table has a slot: the key-owning path ends it without a launch; without that path the atomics kernel is launched as before */
		Ctx c = table(4, YK_NOCAP, 0);
		Env env = DEFAULTS;
		one_case(c, env);
		CHECK(plan_of(c, env, YK_FMT_HASH, true).path == YK_COUNT_NOTHING && plan_of(c, env, YK_FMT_TAGGED, true).path == YK_COUNT_NOTHING);
		CHECK(plan_of(c, env, YK_FMT_HASH, false).path == YK_COUNT_ATOMICS);
		CHECK(count_consumed_fmt(CountTable{ c.nb_bits, c.pre, c.k, c.plo, c.phi, c.h_bits.data(), c.h_count.data() }, knobs_of(env)) == YK_FMT_HASH);
		env.COUNT_OWN = 0;
		one_case(c, env);
		CHECK(plan_of(c, env, YK_FMT_HASH, true).path == YK_COUNT_ATOMICS && plan_of(c, env, YK_FMT_POS, true).path == YK_COUNT_ATOMICS);
		CHECK(plan_of(c, env, YK_FMT_TAGGED, true).path == YK_COUNT_REFUSED);
	}
	{   /* one sub-table of 4 slots among empties: no range of 32 slots, so LDS ranks; the records of the key-owning kernel alone are refused */
		Ctx c = table(5, YK_NOCAP, 0);
		c.h_bits[11] = 2; c.h_count[11] = 3;
		one_case(c, DEFAULTS);
		const CountPlan pl = plan_of(c, DEFAULTS, YK_FMT_HASH, true);
		CHECK(pl.path == YK_COUNT_LDS && pl.lds == 8 + 8 + 16 && pl.ck_stride == 3);
		CHECK(plan_of(c, DEFAULTS, YK_FMT_HASH_RNG, true).path == YK_COUNT_REFUSED);
		Ctx shard = c;                                                         /* ... and a shard that does not hold it sees an empty table */
		shard.plo = 12;
		one_case(shard, DEFAULTS);
		CHECK(plan_of(shard, DEFAULTS, YK_FMT_HASH, true).path == YK_COUNT_NOTHING);
	}
	for (int rng_log : { 5, 10 }) {   /* the largest sub-table at 2^8 and at 2^9 home-slot ranges */
		Env env = DEFAULTS;
		env.COUNT_OWN = 0; env.COUNT_LDS = 0; env.rng_log = rng_log;
		Ctx c = table(3, 6, 40);
		c.h_bits[5] = (u32)rng_log + 8; c.h_count[5] = 3u << (rng_log + 6);
		one_case(c, env);
		const CountPlan pl = plan_of(c, env, YK_FMT_HASH, true);
		CHECK(pl.path == YK_COUNT_RANGES && pl.rb == 8 && pl.max_len == 1u << rng_log);
		CHECK(plan_of(c, env, YK_FMT_POS, true).path == YK_COUNT_ATOMICS);      /* the ranges take hashes alone */
		c.h_bits[5] = (u32)rng_log + 9;
		one_case(c, env);
		CHECK(plan_of(c, env, YK_FMT_HASH, true).path == YK_COUNT_ATOMICS);
	}
	{   /* LDS ranks at their limit: 2^18 slots are 65536 bytes of bitmap and ranks, 44024 keys 88048 bytes of counters, + 16 = 150 KiB */
		Env env = DEFAULTS;
		env.COUNT_OWN = 0;
		Ctx c = table(3, 18, 1000);
		c.h_count[2] = 44024;
		one_case(c, env);
		CountPlan pl = plan_of(c, env, YK_FMT_HASH, true);
		CHECK(pl.path == YK_COUNT_LDS && pl.lds == 150 * 1024 && pl.ck_stride == 44024);
		c.h_count[2] = 44025;
		one_case(c, env);
		pl = plan_of(c, env, YK_FMT_HASH, true);
		CHECK(pl.path == YK_COUNT_RANGES && pl.rb == 2 && pl.max_len == 1u << 16);
		CHECK(plan_of(c, env, YK_FMT_POS, true).path == YK_COUNT_ATOMICS);
	}
	{   /* key-owning ranges at the limit of ranges per sub-table: 700 keys in 1024 slots and 18700 bytes leave ranges of 32 slots (22 keys a range,
	     * + 2 + 192 = 216 keys of room: 16 + 1728 + 432 + 16400 = 18576 bytes; ranges of 64 slots need 241 keys of room, 18832 bytes), 2^5 of them */
		Env env = DEFAULTS;
		env.OWN_LDS = 18700; env.OWN_MAXRB = 5;
		Ctx c = table(4, 10, 700);
		one_case(c, env);
		const CountPlan pl = plan_of(c, env, YK_FMT_TAGGED, true);
		CHECK(pl.path == YK_COUNT_OWN && pl.rng_log == 5 && pl.rb == 5 && pl.kmax == 216 && pl.lds == 18576);
		CHECK(count_consumed_fmt(CountTable{ c.nb_bits, c.pre, c.k, c.plo, c.phi, c.h_bits.data(), c.h_count.data() }, knobs_of(env)) == YK_FMT_HASH_RNG);
		env.OWN_MAXRB = 4;
		one_case(c, env);
		CHECK(plan_of(c, env, YK_FMT_TAGGED, true).path == YK_COUNT_REFUSED && plan_of(c, env, YK_FMT_HASH, true).path == YK_COUNT_LDS);
		CHECK(count_consumed_fmt(CountTable{ c.nb_bits, c.pre, c.k, c.plo, c.phi, c.h_bits.data(), c.h_count.data() }, knobs_of(env)) == YK_FMT_HASH);
	}
	{   /* tagged records with the key-owning path switched off */
		Env env = DEFAULTS;
		env.COUNT_OWN = 0;
		Ctx c = table(6, 9, 300);
		one_case(c, env);
		CHECK(plan_of(c, env, YK_FMT_TAGGED, true).path == YK_COUNT_REFUSED);
	}

	/* random tables and settings */
	static const int64_t OWN_LDS[7] = { 18500, 18700, 19500, 21000, 24000, 30000, 156000 };   /* the budgets of the GPU tests' matrices */
	static const int RNG_LOGS[5] = { 5, 6, 7, 10, 16 };
	static const int KS[6] = { 15, 21, 31, 32, 40, 63 };
	for (int rep = 0; rep < 4000; ++rep) {
		Ctx c;
		c.pre = 3 + (int)(rnd() % 8);                                          /* P = 8 .. 1024: with few sub-tables the shard bounds bite */
		c.nb_bits = c.pre;
		if (rnd() % 4 == 0) do c.nb_bits = 3 + (int)(rnd() % 11); while (c.nb_bits == c.pre);
		c.k = KS[rnd() % 6];
		const int P = 1 << c.pre;
		c.plo = 0; c.phi = P;
		if (rnd() % 2) { c.plo = (int)(rnd() % (uint64_t)P); c.phi = c.plo + 1 + (int)(rnd() % (uint64_t)(P - c.plo)); }
		const u32 top = 2 + (u32)(rnd() % 21);                                 /* sub-tables of 2^2 .. 2^top slots, top <= 22 */
		const int empties = (int)(rnd() % 4);                                  /* none, a quarter, half, all but a few */
		c.h_bits.assign(P, YK_NOCAP); c.h_count.assign(P, 0);
		for (int p = 0; p < P; ++p) {
			if (empties == 3 ? rnd() % 16 != 0 : (int)(rnd() % 4) < empties) continue;
			c.h_bits[p] = 2 + (u32)(rnd() % (top - 1));
			const u32 cap = 1u << c.h_bits[p];
			c.h_count[p] = (u32)(rnd() % (cap * 3 / 4 + 1));
			if (rnd() % 8 == 0) c.h_count[p] = cap * 3 / 4;
		}
		Env env;
		env.COUNT_OWN = rnd() % 4 != 0; env.COUNT_LDS = rnd() % 4 != 0; env.COUNT_RNG = rnd() % 4 != 0; env.YTAG = rnd() % 4 != 0;
		env.OWN_LDS = OWN_LDS[rnd() % 7];
		env.OWN_MAXRB = rnd() % 2 ? 4 : 12;
		env.rng_log = RNG_LOGS[rnd() % 5];
		one_case(c, env);
	}
	for (int p = 0; p < 6; ++p) CHECK(g_seen[p] > 100);                            /* the cases reach every path, often */
	if (g_bad) { fprintf(stderr, "%d checks failed over %d cases\n", g_bad, g_case); return 1; }
	printf("ok\n");
	return 0;
}
