/* count_plan.h -- how a batch of records is counted into the keys a table already holds (a create_new = 0 pass; engine_count.cpp; DESIGN.md section
 * 27): which of the four paths takes it, and with which parameters, is arithmetic on the table's sub-table sizes, the record format and a few
 * settings.  Plain C++: no HIP, no library state, so that tests/tools/count_plan_check.cpp can hold it to the cascade it replaced without a device.
 * The one decision has three askers -- the extraction (which format a count pass consumes), the count of a batch, and the count over the retained
 * records of the pass before (whether the key-owning kernel can read them at all) -- and all three ask count_plan().
 * The order of the choice, first match wins:
 *   1. records grouped by sub-table, level-1 buckets == sub-tables, key-owning on: no sub-table has a slot -> nothing to do; else the largest slot
 *      range (>= 32 slots) whose bitmap and share of the keys fit the LDS budget, if that cuts the largest sub-table into at most 2^own_maxrb ranges
 *      -> key-owning ranges (k_img_count_own);
 *   2. YK_FMT_HASH_RNG and YK_FMT_TAGGED records, grouped, that 1 did not take -> refused: only k_img_count_own reads them;
 *   3. grouped, buckets == sub-tables, LDS ranks on, and every sub-table's bitmap and 16-bit counters within 150 KiB -> LDS ranks (k_img_count_lds);
 *   4. grouped YK_FMT_HASH, buckets == sub-tables, ranges on, some sub-table has a slot, at most 2^8 ranges of 2^rng_log slots in the largest
 *      -> home-slot ranges (k_hpart2 + k_img_count_rng);
 *   5. device atomics (k_img_count_h, k_img_count).  Records that are not grouped come here at once. */
#ifndef YK_COUNT_PLAN_H
#define YK_COUNT_PLAN_H
#include <stddef.h>
#include <algorithm>
#include "replay_plan.h"                 /* u32 / u64, YK_NOCAP */
#include "rec_fmt.h"

/* LDS needed by k_img_count_lds for a sub-table of `cap` slots holding `count` keys */
static inline size_t yk_plan_img_count_lds_bytes(u32 cap, u32 count) { return (size_t)((cap + 31) / 32) * 8 + (size_t)(count + 1) / 2 * 4 + 16; }
/* ... by k_img_count_own for a range of range_len slots with room for kmax keys: bitmap, ranks, keys, counters, 16 wave queues */
static inline size_t yk_plan_count_own_lds(u32 range_len, u32 kmax) { const u32 nw = (range_len + 31) / 32; return (size_t)2 * ((nw + 1) & ~1u) * 4 + (size_t)kmax * 8 + (size_t)(((kmax + 1) / 2 + 1) & ~1u) * 4 + 16 * 128 * 8 + 16; }

/* the table as the choice sees it: sub-tables [plo, phi) of the shard, h_bits[p] = log2 capacity or YK_NOCAP, h_count[p] keys */
struct CountTable { int nb_bits, pre, k, plo, phi; const u32 *h_bits, *h_count; };
/* the settings, filled once by the caller (engine_count.cpp count_knobs: the YAKAMD_* names and their defaults) */
struct CountKnobs {
	bool own, lds_ranks, ranges, ytag;   /* YAKAMD_COUNT_OWN, _COUNT_LDS, _COUNT_RNG, _YTAG */
	size_t own_lds;                      /* YAKAMD_OWN_LDS: one workgroup per CU with as few ranges as possible: every range re-reads the sub-table's records (measured: 8 ranges x 1 WG/CU 16.9 ms, 16 ranges x 2 WG/CU 24.8 ms) */
	int own_maxrb;                       /* YAKAMD_OWN_MAXRB: every range's workgroup streams the whole sub-table: too redundant beyond 16 ranges */
	int rng_log;                         /* yk_rng_log(): log2 slots per range of the home-slot ranges */
};

enum CountPath { YK_COUNT_NOTHING, YK_COUNT_OWN, YK_COUNT_RANGES, YK_COUNT_LDS, YK_COUNT_ATOMICS, YK_COUNT_REFUSED };
struct CountPlan {
	CountPath path;
	int rng_log, rb;                     /* key-owning: 2^rng_log slots per range, up to 2^rb ranges per sub-table; ranges: 2^rb ranges per sub-table */
	u32 kmax;                            /* key-owning: keys of LDS room per range */
	u32 max_len;                         /* ranges: slots of the longest range */
	u32 ck_stride;                       /* LDS ranks: the compact-key scratch per sub-table */
	size_t lds;                          /* key-owning, LDS ranks: dynamic LDS bytes of a workgroup */
};

static inline CountPlan count_plan(const CountTable &t, const CountKnobs &kn, RecFmt fmt, bool grouped)
{
	CountPlan pl = { YK_COUNT_ATOMICS, 0, 0, 0, 0, 1, 0 };
	if (!grouped) return pl;
	const bool by_sub_table = t.nb_bits == t.pre;
	u32 bmax = 0;
	for (int p = t.plo; p < t.phi; ++p) if (t.h_bits[p] != YK_NOCAP) bmax = std::max(bmax, t.h_bits[p]);
	if (kn.own && by_sub_table) {
		if (bmax == 0) { pl.path = YK_COUNT_NOTHING; return pl; }   /* no sub-table has a slot: nothing can be found */
		int rng_log = -1; u32 kmax = 0;
		for (int rl = (int)bmax; rl >= 5 && rng_log < 0; --rl) {
			u32 km = 1;
			for (int p = t.plo; p < t.phi; ++p) {
				if (t.h_bits[p] == YK_NOCAP) continue;
				const int rbp = (int)t.h_bits[p] > rl ? (int)t.h_bits[p] - rl : 0;
				const u32 e = (t.h_count[p] + (1u << rbp) - 1) >> rbp;
				km = std::max(km, rbp ? e + e / 8 + 192 : t.h_count[p]);   /* a range's share of the keys + 12 % + 6 sigma at small counts */
			}
			if (yk_plan_count_own_lds(1u << rl, km) <= kn.own_lds) { rng_log = rl; kmax = km; }
		}
		if (rng_log >= 0 && (int)bmax - rng_log <= kn.own_maxrb) {
			pl.path = YK_COUNT_OWN; pl.rng_log = rng_log; pl.rb = (int)bmax - rng_log; pl.kmax = kmax; pl.lds = yk_plan_count_own_lds(1u << rng_log, kmax);
			return pl;
		}
	}
	if (fmt == YK_FMT_HASH_RNG || fmt == YK_FMT_TAGGED) { pl.path = YK_COUNT_REFUSED; return pl; }
	if (by_sub_table && kn.lds_ranks) {
		size_t lds = 0;
		for (int p = t.plo; p < t.phi; ++p)
			if (t.h_bits[p] != YK_NOCAP) lds = std::max(lds, yk_plan_img_count_lds_bytes(1u << t.h_bits[p], t.h_count[p]));
		if (lds && lds <= 150 * 1024) {
			pl.path = YK_COUNT_LDS; pl.lds = lds;
			for (int p = t.plo; p < t.phi; ++p) pl.ck_stride = std::max(pl.ck_stride, t.h_count[p]);
			return pl;
		}
	}
	const int rb = (int)bmax > kn.rng_log ? (int)bmax - kn.rng_log : 0;
	if (fmt == YK_FMT_HASH && by_sub_table && kn.ranges && bmax != 0 && rb <= 8) {
		/* sub-tables too large for one workgroup's LDS: each one's hashes are split by home-slot range first */
		pl.path = YK_COUNT_RANGES; pl.rb = rb; pl.max_len = 1u << std::min((int)bmax, kn.rng_log);
	}
	return pl;
}

/* the format a count pass's extraction writes for a batch that is consumed at once: counting existing keys needs no stream positions, and where the
 * key-owning count will run, its range test is prepared by the extraction (k < 32 and at most 10 prefix bits: k_xpart_wcs) */
static inline RecFmt count_consumed_fmt(const CountTable &t, const CountKnobs &kn)
{
	return t.k < 32 && t.nb_bits <= 10 && kn.ytag && count_plan(t, kn, YK_FMT_HASH, true).path == YK_COUNT_OWN ? YK_FMT_HASH_RNG : YK_FMT_HASH;
}
#endif
