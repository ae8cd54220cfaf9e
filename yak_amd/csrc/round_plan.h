/* round_plan.h -- the exchange plan of one multi-GPU round (yak_multi.cpp; DESIGN.md section 6, "The round plan"): once every slot has grouped the
 * records of its chunk by prefix, who sends what to whom, at which offsets and in which posting order, and what every rank feeds, is arithmetic on
 * the prefix starts.  Plain C++: no HIP, no RCCL, no library state, so that tests/tools/round_plan_check.cpp can hold it to the loops it replaced
 * and to what a grouped send / recv requires, without a device.
 * Rank d owns prefixes [d P / N, (d + 1) P / N) and is hosted by slot slot_of[d]; bst[s][p] = where the records of prefix p start in slot s's send
 * buffer (in records of W words; bst[s][P] = their number).  Receive layout of a slot: for each rank it hosts (rank order), the slices of the other
 * slots' chunks (slot order). */
#ifndef YK_ROUND_PLAN_H
#define YK_ROUND_PLAN_H
#include <stdint.h>
#include <algorithm>
#include <vector>

/* one slice on the wire: rank `rank`'s share of slot src's chunk, cnt words from word send_off of src's send buffer to word recv_off of dst's receive buffer */
struct RoundXfer { int src, dst, rank; uint64_t send_off, recv_off, cnt; };
/* one slice a rank feeds: its share of slot `slot`'s chunk -- cnt records at word `off` of its own slot's send buffer (own: the slice of the slot's
 * own chunk is fed where the partition left it) or receive buffer; ob[p] = where prefix p starts in the slice (p clamped to the rank's range) */
struct RoundSlice { int slot; bool own; uint64_t off, cnt; std::vector<uint64_t> ob; };

struct ExchangePlan {
	std::vector<std::vector<uint64_t> > bst;                     /* [slot][P + 1]: the input, filled by the partition */
	std::vector<std::vector<uint64_t> > roff;                    /* [rank][slot]: where rank d's slice of chunk s lies in its slot's receive buffer (records) */
	std::vector<uint64_t> recv;                                  /* [slot]: records the slot receives */
	std::vector<RoundXfer> xfer;                                 /* in posting order: slot-major, then rank; empty slices and a slot's own are not sent */
	std::vector<std::vector<RoundSlice> > feed;                  /* [rank]: in chunk order = stream order; empty slices left out */

	void build(int N, int P, int S, const std::vector<int> &slot_of, int W)
	{
		roff.assign(N, std::vector<uint64_t>(S, 0));
		recv.assign(S, 0);
		feed.assign(N, std::vector<RoundSlice>());
		xfer.clear();
		for (int d = 0; d < N; ++d)
			for (int s = 0; s < S; ++s) {
				const int lo = d * (P / N), hi = (d + 1) * (P / N), sd = slot_of[d];
				const uint64_t cnt = bst[s][hi] - bst[s][lo];
				if (s != sd) { roff[d][s] = recv[sd]; recv[sd] += cnt; }
				if (cnt == 0) continue;
				if (s != sd) xfer.push_back(RoundXfer{ s, sd, d, bst[s][lo] * W, roff[d][s] * W, cnt * W });
				feed[d].push_back(RoundSlice{ s, s == sd, (s == sd ? bst[s][lo] : roff[d][s]) * W, cnt, std::vector<uint64_t>(P + 1) });
				for (int p = 0; p <= P; ++p) feed[d].back().ob[p] = bst[s][p < lo ? lo : p > hi ? hi : p] - bst[s][lo];
			}
		std::stable_sort(xfer.begin(), xfer.end(), [](const RoundXfer &a, const RoundXfer &b) { return a.src < b.src; });   /* rank-major so far */
	}
};
#endif
