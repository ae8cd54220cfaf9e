/* table_ranges.h -- the range rule of the commands that walk a table's stored keys (print, hetmers, unitigs): sub-tables [lo, hi) cut into ranges
 * of whole sub-tables, each as many as a budget of keys allows and one at the least, so a sub-table larger than the budget is a range of its own.
 * Host C++ alone: tests/tools/table_ranges_check.cpp holds it against the three loops it replaced. */
#ifndef YK_TABLE_RANGES_H
#define YK_TABLE_RANGES_H
#include <stdint.h>
#include <vector>

/* sub-tables [lo, hi) and off[j] = the keys of the range before sub-table lo + j (hi - lo + 1 entries) */
typedef unsigned long long tr_u64;                            /* (the engine's u64) */
struct TableRange { int lo, hi; std::vector<tr_u64> off; tr_u64 n() const { return off.back(); } };

/* the ranges of [lo, hi) in order; size(p) = the keys of sub-table p.  A budget below 1 counts as 1.  keep_empty: a range without keys is listed
 * too, so that the ranges tile [lo, hi); otherwise it is left out */
template <class Size> std::vector<TableRange> table_ranges(int lo, int hi, Size size, int64_t budget, bool keep_empty)
{
	const tr_u64 room = budget < 1 ? 1 : (tr_u64)budget;
	std::vector<TableRange> out;
	TableRange r{ lo, lo, std::vector<tr_u64>(1, 0) };
	auto close = [&](int p) { r.hi = p; if (keep_empty || r.n()) out.push_back(r); r.lo = p; r.off.assign(1, 0); };
	for (int p = lo; p < hi; ++p) {
		const tr_u64 s = size(p);
		if (p > r.lo && r.n() + s > room) close(p);
		r.off.push_back(r.n() + s);
	}
	if (lo < hi) close(hi);
	return out;
}

/* A table sharded over n_sub owners: owner r holds the prefixes [r P / n_sub, (r + 1) P / n_sub), P = 1 << pre.  Precondition: n_sub divides P
 * (so it is a power of two; yak_multi.cpp deals the prefixes out so and refuses any other number) -- the span's bounds are then exact and the owner
 * of a prefix is the one whose span holds it; with another n_sub the two would round differently */
static inline int yk_shard_owner(int pre, int n_sub, uint64_t prefix) { return (int)(prefix * (uint64_t)n_sub >> pre); }
struct ShardSpan { int lo, hi; };
static inline ShardSpan yk_shard_span(int pre, int n_sub, int r) { return ShardSpan{ (int)(((int64_t)r << pre) / n_sub), (int)(((int64_t)(r + 1) << pre) / n_sub) }; }
#endif
