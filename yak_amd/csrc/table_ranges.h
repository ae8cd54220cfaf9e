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
#endif
