/* table_ranges_check.cpp -- the range rule of yak_amd/csrc/table_ranges.h against the three loops it replaced, restated here as they stood (the
 * het-mer walk's hm_ranges, the loop of yakamd_print, the loop of yakamd_unitigs), and against the properties of the rule itself, over random
 * size vectors.  A program of its own (tests/test_table_ranges.py builds it with the address and undefined-behaviour sanitizers); prints `ok`.
 *
 * The budgets the old loops were given: hm_ranges and the unitigs loop got theirs through hm_batch / gr_batch, which raise a value below 1 to 1, so
 * that is how they are called here.  The print loop got `room` as it came, and room = 0 (a batch_bytes below one line) is the one place where the
 * rule differs from it on purpose: at 0 the old loop cut in front of every sub-table once the range held a key, the rule counts 0 as 1 and lets a
 * range of one key take the empty sub-tables behind it.  So at room 0 the print shape is held to the old loop at room 1, and for the old loop at
 * room 0 itself the properties are checked that the listing depends on: it tiles the piece, in order. */
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include <algorithm>
#include "../../yak_amd/csrc/table_ranges.h"

typedef unsigned long long u64;

static int g_bad = 0;
#define CHECK(x) do { if (!(x)) { if (g_bad < 20) fprintf(stderr, "%s:%d: %s does not hold (case %d)\n", __FILE__, __LINE__, #x, g_case); ++g_bad; } } while (0)
static int g_case = 0;

/* ---- the old loops ---- */
struct Range { int lo, hi; std::vector<u64> off; u64 n() const { return off.back(); } };

/* yak_hetmer.cpp, hm_ranges(c, batch): c->P is P, c->h_count is h_count */
static std::vector<Range> old_hetmer(int P, const std::vector<uint32_t> &h_count, int64_t batch)
{
	std::vector<Range> out;
	Range r;
	r.lo = 0; r.off.assign(1, 0);
	for (int p = 0; p < P; ++p) {
		const u64 size = h_count[p];
		if (p > r.lo && r.n() + size > (u64)batch) {
			r.hi = p;
			if (r.n()) out.push_back(r);
			r.lo = p; r.off.assign(1, 0);
		}
		r.off.push_back(r.n() + size);
	}
	r.hi = P;
	if (r.n()) out.push_back(r);
	return out;
}

/* yak_print.cpp, yakamd_print: one piece [p_lo, p_hi); yakamd_subtable(p.s, w, &cap, &size) is size = h_count[w] */
struct Piece { int lo, hi; };
static std::vector<Piece> old_print(int p_lo, int p_hi, const std::vector<uint32_t> &h_count, u64 room, u64 *most_out)
{
	std::vector<Piece> ranges;
	u64 most = 0;
	{
		int lo = p_lo;
		u64 n = 0;
		for (int w = p_lo; w < p_hi; ++w) {
			uint32_t size = h_count[w];
			if (w > lo && n + size > room) { ranges.push_back(Piece{ lo, w }); most = std::max(most, n); lo = w; n = 0; }
			n += size;
		}
		ranges.push_back(Piece{ lo, p_hi });
		most = std::max(most, n);
	}
	*most_out = most;
	return ranges;
}

/* yak_graph.cpp, yakamd_unitigs: key0[p] = the keys of the sub-tables before p; the ranges that reach the record kernel */
struct Pulled { int lo, hi; u64 n; };
static std::vector<Pulled> old_unitigs(int P, const std::vector<u64> &key0, int64_t batch)
{
	std::vector<Pulled> out;
	for (int lo = 0; lo < P; ) {
		int hi = lo + 1;
		while (hi < P && key0[hi + 1] - key0[lo] <= (u64)batch) ++hi;
		const u64 n = key0[hi] - key0[lo];
		if (n) out.push_back(Pulled{ lo, hi, n });
		lo = hi;
	}
	return out;
}

/* ---- the rule's own properties, for the result that keeps empty ranges ---- */
static void properties(const std::vector<TableRange> &rs, int lo, int hi, const std::vector<uint32_t> &size, int64_t budget)
{
	const u64 room = budget < 1 ? 1 : (u64)budget;
	CHECK(!rs.empty() && rs.front().lo == lo && rs.back().hi == hi);   /* they tile [lo, hi) in order */
	for (size_t i = 0; i < rs.size(); ++i) {
		const TableRange &r = rs[i];
		CHECK(r.hi > r.lo);                                        /* one sub-table at the least */
		if (i + 1 < rs.size()) CHECK(rs[i + 1].lo == r.hi);
		CHECK(r.off.size() == (size_t)(r.hi - r.lo) + 1 && r.off[0] == 0);
		for (int p = r.lo; p < r.hi && (size_t)(p - r.lo + 1) < r.off.size(); ++p) CHECK(r.off[p - r.lo + 1] == r.off[p - r.lo] + size[p]);   /* the scan of the sizes */
		if (r.hi - r.lo > 1) CHECK(r.n() <= room);                 /* more than one sub-table: within the budget */
		if (r.hi < hi) CHECK(r.n() + size[r.hi] > room);           /* the next one would not have fitted */
	}
}

static bool same(const TableRange &a, const TableRange &b) { return a.lo == b.lo && a.hi == b.hi && a.off == b.off; }

/* ---- the cases ---- */
static u64 g_rng = 0x9e3779b97f4a7c15ull;
static u64 rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static void one_case(int P, const std::vector<uint32_t> &size, int64_t budget)
{
	++g_case;
	auto sz = [&](int p) { return (u64)size[p]; };
	const int64_t clamped = budget < 1 ? 1 : budget;                 /* hm_batch(), gr_batch() */
	std::vector<u64> key0(P + 1, 0);
	for (int p = 0; p < P; ++p) key0[p + 1] = key0[p] + size[p];

	/* the whole table, empty ranges kept: the properties; without them: the same ranges but the empty ones */
	const std::vector<TableRange> all = table_ranges(0, P, sz, budget, true), full = table_ranges(0, P, sz, budget, false);
	properties(all, 0, P, size, budget);
	size_t j = 0;
	for (const TableRange &r : all)
		if (r.n()) { CHECK(j < full.size() && same(full[j], r)); ++j; }
	CHECK(j == full.size());

	/* the het-mer walk */
	const std::vector<Range> hm = old_hetmer(P, size, clamped);
	CHECK(hm.size() == full.size());
	for (size_t i = 0; i < hm.size() && i < full.size(); ++i) CHECK(hm[i].lo == full[i].lo && hm[i].hi == full[i].hi && hm[i].off == full[i].off);

	/* the unitigs walk */
	const std::vector<Pulled> ug = old_unitigs(P, key0, clamped);
	CHECK(ug.size() == full.size());
	for (size_t i = 0; i < ug.size() && i < full.size(); ++i) CHECK(ug[i].lo == full[i].lo && ug[i].hi == full[i].hi && ug[i].n == full[i].n() && key0[ug[i].lo] + full[i].n() == key0[ug[i].hi]);

	/* print: the table as one piece, and as three pieces cut at random (the shards of a table: a piece starts where it starts, not at 0) */
	int cut[4] = { 0, (int)(rnd() % (u64)(P + 1)), (int)(rnd() % (u64)(P + 1)), P };
	std::sort(cut, cut + 4);
	const int whole[2] = { 0, P };
	for (int shape = 0; shape < 2; ++shape) {
		const int *at = shape ? cut : whole, n_pc = shape ? 3 : 1;
		for (int i = 0; i < n_pc; ++i) {
			const int lo = at[i], hi = at[i + 1];
			if (lo == hi) continue;                                /* (no such piece: pieces_of leaves it out) */
			const std::vector<TableRange> got = table_ranges(lo, hi, sz, budget, true);
			properties(got, lo, hi, size, budget);
			u64 most = 0, most_got = 0;
			const std::vector<Piece> want = old_print(lo, hi, size, (u64)clamped, &most);
			CHECK(want.size() == got.size());
			for (size_t q = 0; q < want.size() && q < got.size(); ++q) { CHECK(want[q].lo == got[q].lo && want[q].hi == got[q].hi); most_got = std::max(most_got, got[q].n()); }
			CHECK(most == most_got);
			if (budget < 1) {                                      /* room 0 as the old loop took it: a tiling in order all the same */
				const std::vector<Piece> zero = old_print(lo, hi, size, 0, &most);
				CHECK(zero.front().lo == lo && zero.back().hi == hi);
				for (size_t q = 0; q < zero.size(); ++q) CHECK(zero[q].hi > zero[q].lo && (q + 1 == zero.size() || zero[q + 1].lo == zero[q].hi));
			}
		}
	}
}

/* ---- the shards of a table: yk_shard_owner and yk_shard_span against the two expressions yak_api.cpp had, (x & pm) * n_sub >> pre in insert_list,
 * get, inc and getseq, (r << pre) / n_sub in dump_through, for every n_sub that divides 1 << pre ---- */
static void shards()
{
	for (int pre = 10; pre <= 14; ++pre)
		for (int n_sub = 1; n_sub <= 1 << pre; n_sub <<= 1) {
			g_case = -(pre * 100000 + n_sub);
			const uint64_t pm = (1ULL << pre) - 1;
			int next = 0;
			for (int r = 0; r < n_sub; ++r) {
				const ShardSpan s = yk_shard_span(pre, n_sub, r);
				CHECK(s.lo == next && s.hi > s.lo);                   /* the spans tile [0, 1 << pre) in order */
				CHECK(s.lo == (int)(((int64_t)r << pre) / n_sub) && s.hi == (int)(((int64_t)(r + 1) << pre) / n_sub));
				for (int p = s.lo; p < s.hi; ++p) CHECK(yk_shard_owner(pre, n_sub, (uint64_t)p) == r);   /* owner(p) == r exactly on span(r): the spans are disjoint */
				next = s.hi;
			}
			CHECK(next == 1 << pre);
			for (int p = 0; p < 1 << pre; ++p) {
				const uint64_t x = rnd() << pre | (uint64_t)p;         /* a hash with prefix p */
				CHECK(yk_shard_owner(pre, n_sub, x & pm) == (int)((x & ((1ULL << pre) - 1)) * n_sub >> pre));
				CHECK(yk_shard_owner(pre, n_sub, (uint64_t)p) == (int)((uint64_t)p * n_sub >> pre));   /* getseq's */
			}
		}
}

int main()
{
	int n_vec = 0;
	for (int rep = 0; rep < 48; ++rep)
		for (int P = 1; P <= 64; ++P) {
			std::vector<uint32_t> size(P);
			const int mode = (int)(rnd() % 6);
			static const uint32_t tops[6] = { 2, 10, 1000, 100000, 0xffffffffu, 3 };
			const uint32_t top = tops[mode];
			const int zeros = (int)(rnd() % 4);                     /* 0: none on purpose; 1: half; 2: nine in ten; 3: runs at both ends */
			const int head = zeros == 3 ? (int)(rnd() % (u64)(P + 1)) : 0, tail = zeros == 3 ? (int)(rnd() % (u64)(P + 1)) : 0;
			u64 sum = 0;
			for (int p = 0; p < P; ++p) {
				uint32_t s = (uint32_t)(rnd() % ((u64)top + 1));
				if ((zeros == 1 && rnd() % 2) || (zeros == 2 && rnd() % 10) || (zeros == 3 && (p < head || p >= P - tail))) s = 0;
				size[p] = s; sum += s;
			}
			const u64 big = *std::max_element(size.begin(), size.end());
			const int64_t budgets[] = { 0, 1, (int64_t)sum, (int64_t)sum + 1, -5, (int64_t)(big / 2), (int64_t)big - 1, (int64_t)big, (int64_t)(rnd() % (sum + 2)),
			                            (int64_t)(rnd() % (2 * big + 2)), (int64_t)1 << 62 };   /* below the largest size: single sub-tables above the budget */
			for (int64_t b : budgets) one_case(P, size, b);
			++n_vec;
		}
	/* all sub-tables empty */
	for (int P = 1; P <= 64; P += 9) { one_case(P, std::vector<uint32_t>(P, 0), 0); one_case(P, std::vector<uint32_t>(P, 0), 7); ++n_vec; }
	/* no sub-table at all: no range */
	CHECK(table_ranges(3, 3, [](int) { return (u64)1; }, 5, true).empty());
	shards();
	if (g_bad) { fprintf(stderr, "%d checks failed over %d size vectors\n", g_bad, n_vec); return 1; }
	printf("ok\n");
	return 0;
}
