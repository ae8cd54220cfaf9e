/* round_plan_check.cpp -- the exchange plan of a multi-GPU round (yak_amd/csrc/round_plan.h) against the four loops of yak_multi.cpp it replaced,
 * restated here as they stood (round_exchange's offset pass, its peer_copies, its grouped send / recv loop, round_feed), and against what the plan
 * must guarantee by itself: receive buffers tiled without overlap, every (sender, receiver) pair's sends and receives with the same counts in the
 * same order (a grouped send / recv hangs on anything else), every rank fed its prefix range of every chunk in chunk order.  Random cases; a
 * program of its own (tests/test_round_plan.py builds it with the address and undefined-behaviour sanitizers); prints `ok`. */
#include <stdio.h>
#include <stdint.h>
#include <algorithm>
#include <map>
#include <vector>
#include "../../yak_amd/csrc/round_plan.h"

typedef std::vector<std::vector<uint64_t> > Mat;

static int g_bad = 0, g_case = 0;
#define CHECK(x) do { if (!(x)) { if (g_bad < 20) fprintf(stderr, "%s:%d: %s does not hold (case %d)\n", __FILE__, __LINE__, #x, g_case); ++g_bad; } } while (0)

/* ---- the old loops: what they computed and the calls they made, in order ---- */
struct Copy { int to_slot, from_slot; uint64_t recv_word, send_word, bytes; };              /* hipMemcpyPeerAsync(d_recv[to] + recv_word, ..., d_send[from] + send_word, ..., bytes, st[to]) */
struct Call { bool send; int on_slot, peer; uint64_t word, cnt; };                            /* ncclSend(d_send[on] + word, cnt, peer, comm[on]) / ncclRecv(d_recv[on] + word, cnt, peer, comm[on]) */
struct Feed { int rank, slot; bool from_send; uint64_t word, cnt; std::vector<uint64_t> ob; };   /* feed(sub[rank], (from_send ? d_send[slot] : d_recv[slot_of[rank]]) + word, cnt, ob, t0[slot], fill[slot]) */

/* round_exchange, the offset pass */
static void old_offsets(int N, int P, int S, const std::vector<int> &slot_of, const Mat &bst, Mat *roff, std::vector<uint64_t> *used)
{
	roff->assign(N, std::vector<uint64_t>(S, 0));
	used->assign(S, 0);
	for (int d = 0; d < N; ++d) {
		const int lo = d * (P / N), hi = (d + 1) * (P / N), sd = slot_of[d];
		for (int s = 0; s < S; ++s) { if (s == sd) continue; (*roff)[d][s] = (*used)[sd]; (*used)[sd] += bst[s][hi] - bst[s][lo]; }
	}
}

/* round_exchange, peer_copies */
static std::vector<Copy> old_peer_copies(int N, int P, int S, const std::vector<int> &slot_of, int W, const Mat &bst, const Mat &roff)
{
	std::vector<Copy> out;
	for (int s = 0; s < S; ++s)
		for (int d = 0; d < N; ++d) {
			const int lo = d * (P / N), hi = (d + 1) * (P / N), sd = slot_of[d];
			const uint64_t cnt = (bst[s][hi] - bst[s][lo]) * W;
			if (cnt == 0 || s == sd) continue;
			out.push_back(Copy{ sd, s, roff[d][s] * W, bst[s][lo] * W, cnt * 8 });
		}
	return out;
}

/* round_exchange, between GroupStart and GroupEnd */
static std::vector<Call> old_group(int N, int P, int S, const std::vector<int> &slot_of, int W, const Mat &bst, const Mat &roff)
{
	std::vector<Call> out;
	for (int s = 0; s < S; ++s)
		for (int d = 0; d < N; ++d) {
			const int lo = d * (P / N), hi = (d + 1) * (P / N), sd = slot_of[d];
			const uint64_t cnt = (bst[s][hi] - bst[s][lo]) * W;
			if (cnt == 0 || s == sd) continue;
			out.push_back(Call{ true, s, sd, bst[s][lo] * W, cnt });
			out.push_back(Call{ false, sd, s, roff[d][s] * W, cnt });
		}
	return out;
}

/* round_feed: the threads of the slots each take their ranks in rank order; per rank the calls are in this order */
static std::vector<Feed> old_feed(int N, int P, int S, const std::vector<int> &slot_of, int W, const Mat &bst, const Mat &roff)
{
	std::vector<Feed> out;
	for (int sd = 0; sd < S; ++sd) for (int d = 0; d < N; ++d) if (slot_of[d] == sd) {
		const int lo = d * (P / N), hi = (d + 1) * (P / N);
		std::vector<uint64_t> ob(P + 1);
		for (int s = 0; s < S; ++s) {
			const uint64_t cnt = bst[s][hi] - bst[s][lo];
			if (cnt == 0) continue;
			for (int p = 0; p <= P; ++p) { const int q = p < lo ? lo : p > hi ? hi : p; ob[p] = bst[s][q] - bst[s][lo]; }
			if (s == sd) out.push_back(Feed{ d, s, true, bst[s][lo] * W, cnt, ob });
			else out.push_back(Feed{ d, s, false, roff[d][s] * W, cnt, ob });
		}
	}
	return out;
}

/* ---- one case ---- */
static void one_case(int N, int P, int S, const std::vector<int> &slot_of, int W, const Mat &bst)
{
	++g_case;
	ExchangePlan X;
	X.bst = bst;
	X.build(N, P, S, slot_of, W);
	CHECK(X.bst == bst);                                           /* the input is only read */

	/* against the old loops */
	Mat roff; std::vector<uint64_t> used;
	old_offsets(N, P, S, slot_of, bst, &roff, &used);
	CHECK(X.roff == roff && X.recv == used);
	const std::vector<Copy> copies = old_peer_copies(N, P, S, slot_of, W, bst, roff);
	const std::vector<Call> calls = old_group(N, P, S, slot_of, W, bst, roff);
	CHECK(copies.size() == X.xfer.size() && calls.size() == 2 * X.xfer.size());
	for (size_t i = 0; i < X.xfer.size() && i < copies.size() && 2 * i + 1 < calls.size(); ++i) {
		const RoundXfer &t = X.xfer[i];
		const Copy &c = copies[i];
		CHECK(c.to_slot == t.dst && c.from_slot == t.src && c.recv_word == t.recv_off && c.send_word == t.send_off && c.bytes == t.cnt * 8);
		const Call &sn = calls[2 * i], &rc = calls[2 * i + 1];
		CHECK(sn.send && sn.on_slot == t.src && sn.peer == t.dst && sn.word == t.send_off && sn.cnt == t.cnt);
		CHECK(!rc.send && rc.on_slot == t.dst && rc.peer == t.src && rc.word == t.recv_off && rc.cnt == t.cnt);
		CHECK(t.rank >= 0 && t.rank < N && slot_of[t.rank] == t.dst);
	}
	const std::vector<Feed> feeds = old_feed(N, P, S, slot_of, W, bst, roff);
	CHECK((int)X.feed.size() == N);
	size_t at = 0;
	for (int sd = 0; sd < S; ++sd) for (int d = 0; d < N && d < (int)X.feed.size(); ++d) if (slot_of[d] == sd)
		for (const RoundSlice &f : X.feed[d]) {
			CHECK(at < feeds.size());
			if (at >= feeds.size()) break;
			const Feed &o = feeds[at++];
			CHECK(o.rank == d && o.slot == f.slot && o.from_send == f.own && o.word == f.off && o.cnt == f.cnt && o.ob == f.ob);
		}
	CHECK(at == feeds.size());

	/* the plan's own properties */
	/* a receive buffer: its slices are disjoint and fill [0, recv) */
	for (int s = 0; s < S; ++s) {
		std::vector<std::pair<uint64_t, uint64_t> > iv;
		for (const RoundXfer &t : X.xfer) if (t.dst == s) iv.push_back(std::make_pair(t.recv_off, t.cnt));
		std::sort(iv.begin(), iv.end());
		uint64_t end = 0;
		for (size_t i = 0; i < iv.size(); ++i) { CHECK(iv[i].first == end && iv[i].second > 0); end = iv[i].first + iv[i].second; }
		CHECK(end == X.recv[s] * W);
	}
	/* a send stays inside the sender's records, and what leaves a slot for a rank is that rank's prefix range of the chunk */
	for (const RoundXfer &t : X.xfer) {
		const int lo = t.rank * (P / N), hi = (t.rank + 1) * (P / N);
		CHECK(t.src != t.dst && t.send_off == bst[t.src][lo] * W && t.send_off + t.cnt == bst[t.src][hi] * W && bst[t.src][hi] <= bst[t.src][P]);
	}
	/* every (sender, receiver) pair: the sends the sender posts and the receives the receiver posts carry the same counts in the same order.  Both
	 * are posted walking the one list, so the posting order of either side is the list's order restricted to the pair */
	std::map<std::pair<int, int>, std::vector<uint64_t> > sent, received;
	for (const Call &c : calls) (c.send ? sent[std::make_pair(c.on_slot, c.peer)] : received[std::make_pair(c.peer, c.on_slot)]).push_back(c.cnt);
	CHECK(sent == received);
	std::map<std::pair<int, int>, std::vector<uint64_t> > planned;
	for (const RoundXfer &t : X.xfer) planned[std::make_pair(t.src, t.dst)].push_back(t.cnt);
	CHECK(planned == sent);
	/* a rank's feed list: chunk order, exactly its prefix range of every chunk, found where the exchange put it */
	for (int d = 0; d < N && d < (int)X.feed.size(); ++d) {
		const int lo = d * (P / N), hi = (d + 1) * (P / N), sd = slot_of[d];
		size_t i = 0;
		for (int s = 0; s < S; ++s) {
			const uint64_t cnt = bst[s][hi] - bst[s][lo];
			if (cnt == 0) continue;                                /* an empty slice is not fed */
			CHECK(i < X.feed[d].size());
			if (i >= X.feed[d].size()) break;
			const RoundSlice &f = X.feed[d][i++];
			CHECK(f.slot == s && f.cnt == cnt && f.own == (s == sd));
			if (f.own) CHECK(f.off == bst[s][lo] * W);
			else {
				bool found = false;
				for (const RoundXfer &t : X.xfer) if (t.src == s && t.dst == sd && t.rank == d) { found = true; CHECK(t.recv_off == f.off && t.cnt == f.cnt * W); }
				CHECK(found);
			}
			CHECK((int)f.ob.size() == P + 1 && f.ob[0] == 0 && f.ob[P] == f.cnt);
			for (int p = 0; p < P && p + 1 < (int)f.ob.size(); ++p) {
				CHECK(f.ob[p] <= f.ob[p + 1]);
				if (p >= lo && p < hi) CHECK(f.ob[p + 1] - f.ob[p] == bst[s][p + 1] - bst[s][p]);   /* the prefixes of the range keep their sizes */
				else CHECK(f.ob[p + 1] == f.ob[p]);                                                 /* the others are empty */
			}
		}
		CHECK(i == X.feed[d].size());
	}
}

/* ---- the cases ---- */
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

int main()
{
	static const int Ns[5] = { 1, 2, 3, 4, 8 };
	int n_cases = 0;
	for (int rep = 0; rep < 700; ++rep)
		for (int ni = 0; ni < 5; ++ni) {
			const int N = Ns[ni];
			const int P = N * (1 + (int)(rnd() % (uint64_t)(64 / N)));            /* a multiple of N up to 64 */
			const int W = 1 + (int)(rnd() % 2);
			/* slots: one per rank; all ranks on one; ranks dealt to 1 .. N slots in order of first appearance (as multi_open numbers the devices) */
			std::vector<int> slot_of(N, 0);
			int S = 1;
			const int how = (int)(rnd() % 3);
			if (how == 0) { for (int r = 0; r < N; ++r) slot_of[r] = r; S = N; }
			else if (how == 2) {
				S = 0;
				const int most = 1 + (int)(rnd() % (uint64_t)N);
				for (int r = 0; r < N; ++r) { const int s = (int)(rnd() % (uint64_t)most); slot_of[r] = s < S ? s : S++; }
			}
			/* prefix sizes per slot: sparse, dense, an empty chunk, one prefix holding everything */
			Mat bst(S, std::vector<uint64_t>(P + 1, 0));
			for (int s = 0; s < S; ++s) {
				const int shape = (int)(rnd() % 5);
				const int all_in = (int)(rnd() % (uint64_t)P);
				for (int p = 0; p < P; ++p) {
					uint64_t n = 0;
					if (shape == 0) n = rnd() % 1000;
					else if (shape == 1) n = rnd() % 4 ? 0 : rnd() % 50;           /* three prefixes in four are empty */
					else if (shape == 2) n = 0;                                    /* an empty chunk */
					else if (shape == 3) n = p == all_in ? 1 + rnd() % 100000 : 0; /* one prefix holds everything */
					else n = rnd() % 3;
					bst[s][p + 1] = bst[s][p] + n;
				}
			}
			one_case(N, P, S, slot_of, W, bst);
			++n_cases;
		}
	if (g_bad) { fprintf(stderr, "%d checks failed over %d cases\n", g_bad, n_cases); return 1; }
	printf("ok\n");
	return 0;
}
