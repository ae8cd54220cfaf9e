/* unitig_walk.h -- the host walk of `yak-amd unitigs`: from the records yakamd_graph_nodes_dev() writes, one per stored key in
 * listing order, to the unitigs in their defined order and orientation, and to the command's two texts.  No HIP in here, like replay_plan.h and
 * hpc_host.h: tests/tools/unitig_walk_check.cpp builds it with the host compiler and the sanitizers.
 *
 * A record is a node iff its count is at least min_cnt.  link[s] of a node is the listing index of the node its side s (0 = R, 1 = L) is linked to,
 * shifted left by one, | the side t of that node which faces back; UG_NONE without a link.  A traversal state is (v, d): d = 0 reads v as stored and
 * leaves through R, d = 1 reads revcomp(v) and leaves through L; along the link (u, t) it enters (u, t ^ 1) and appends the last base of u as read.
 *   open unitigs   first, ascending by the listing index of their start node: the end node with the smaller index, read away from its unlinked side;
 *                  a node without a link is read as stored.  n_threads threads take the start nodes of an index range each -- a thread follows
 *                  the links from every end node to the other end and keeps the chain if that end's index is larger -- and the ranges' results
 *                  follow each other in index order
 *   cycles         afterwards, over the bitmap of the nodes the open unitigs took: ascending by their smallest index, from that node as stored,
 *                  through R; a unitig of n nodes has n + k - 1 bases, so a cycle repeats its first k - 1 bases at its end
 * Every node is followed at most three times: linear in their number.  Links that lead out of the array, into a key that is no node or round in
 * circles where an end was promised are reported, not followed. */
#ifndef YK_UNITIG_WALK_H
#define YK_UNITIG_WALK_H
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include <algorithm>

#define UG_NONE (~(uint64_t)0)

struct ug_node_t { uint64_t x, link[2]; uint32_t count, edges; };         /* yakamd_gnode_t, include/yak_amd.h */

struct ug_unitig_t { uint64_t at, n_node, kc; int cycle; };               /* its n_node + k - 1 bases start at seq[at] of its part */
struct ug_part_t { std::string seq; std::vector<ug_unitig_t> u; std::string err; };
/* the parts in output order: one per thread's index range, then the cycles */
struct ug_result_t { std::vector<ug_part_t> parts; int k; };

static inline uint64_t ug_revcomp(uint64_t x, int k)
{
	uint64_t r = 0;
	for (int j = 0; j < k; ++j) { r = r << 2 | (3 - (x & 3)); x >>= 2; }
	return r;
}

struct ug_walker_t {
	const ug_node_t *nd;
	uint64_t n;
	int k;
	uint32_t min_cnt;
	std::unique_ptr<std::atomic<uint64_t>[]> seen;

	bool node(uint64_t i) const { return i < n && nd[i].count >= min_cnt; }
	void mark(uint64_t i) { seen[i >> 6].fetch_or((uint64_t)1 << (i & 63), std::memory_order_relaxed); }
	bool marked(uint64_t i) const { return seen[i >> 6].load(std::memory_order_relaxed) >> (i & 63) & 1; }
	static char base_of(uint64_t x, int d, int k) { return "ACGT"[d == 0 ? x & 3 : 3 - (x >> 2 * (k - 1) & 3)]; }

	/* the chain from state (v, d) on: to its end (*end = the last node; false if a link is broken or the chain does not end within n steps), or with
	 * `part` its bases, counts and marks as well; stop = the node a cycle ends in front of (UG_NONE for an open chain) */
	bool follow(uint64_t v, int d, uint64_t stop, uint64_t *end, ug_part_t *part)
	{
		ug_unitig_t u = { 0, 1, 0, stop != UG_NONE };
		if (part) {
			u.at = part->seq.size(); u.kc = nd[v].count;
			const uint64_t s = d == 0 ? nd[v].x : ug_revcomp(nd[v].x, k);
			for (int j = k - 1; j >= 0; --j) part->seq.push_back("ACGT"[s >> 2 * j & 3]);
			mark(v);
		}
		for (uint64_t steps = 0; ; ++steps) {
			const uint64_t lk = nd[v].link[d];
			if (lk == UG_NONE) break;
			const uint64_t w = lk >> 1;
			if (!node(w) || steps >= n) return false;
			d = (int)(lk & 1) ^ 1;
			v = w;
			if (v == stop) { if (d != 0) return false; break; }
			if (part) { ++u.n_node; u.kc += nd[v].count; part->seq.push_back(base_of(nd[v].x, d, k)); mark(v); }
		}
		if (stop != UG_NONE && v != stop) return false;
		if (end) *end = v;
		if (part) part->u.push_back(u);
		return true;
	}

	void open_range(uint64_t lo, uint64_t hi, ug_part_t *part)
	{
		char msg[96];
		for (uint64_t i = lo; i < hi && part->err.empty(); ++i) {
			if (!node(i)) continue;
			const bool r = nd[i].link[0] != UG_NONE, l = nd[i].link[1] != UG_NONE;
			if (r && l) continue;
			const int d = r ? 0 : l ? 1 : 0;                        /* away from the unlinked side; as stored without a link */
			uint64_t end = i;
			bool ok = follow(i, d, UG_NONE, &end, 0);
			if (ok && end < i) continue;                             /* the other end starts this one */
			ok = ok && (end > i || (!r && !l)) && follow(i, d, UG_NONE, 0, part);
			if (!ok) { snprintf(msg, sizeof msg, "the links from key %llu do not lead to another end node", (unsigned long long)i); part->err = msg; }
		}
	}

	void cycles(ug_part_t *part)
	{
		char msg[96];
		for (uint64_t i = 0; i < n && part->err.empty(); ++i) {
			if (!node(i) || marked(i)) continue;
			if (nd[i].link[0] == UG_NONE || nd[i].link[1] == UG_NONE || !follow(i, 0, i, 0, part)) {
				snprintf(msg, sizeof msg, "the links from key %llu do not come back to it", (unsigned long long)i);
				part->err = msg;
			}
		}
	}
};

/* the unitigs of n records; 0, or -1 with *err set */
static inline int ug_walk(const ug_node_t *nd, uint64_t n, int k, uint32_t min_cnt, int n_threads, ug_result_t *out, std::string *err)
{
	ug_walker_t w;
	w.nd = nd; w.n = n; w.k = k; w.min_cnt = min_cnt;
	const uint64_t n_w = (n + 63) / 64 + 1;
	w.seen.reset(new std::atomic<uint64_t>[n_w]);
	for (uint64_t i = 0; i < n_w; ++i) w.seen[i].store(0, std::memory_order_relaxed);
	if (n_threads < 1) n_threads = 1;
	if ((uint64_t)n_threads > n / 4096 + 1) n_threads = (int)(n / 4096 + 1);
	out->k = k;
	out->parts.assign((size_t)n_threads + 1, ug_part_t());
	std::vector<std::thread> th;
	for (int t = 1; t < n_threads; ++t)
		th.emplace_back([&w, out, t, n, n_threads]() { w.open_range(n * t / n_threads, n * (t + 1) / n_threads, &out->parts[t]); });
	w.open_range(0, n / n_threads, &out->parts[0]);
	for (std::thread &t : th) t.join();
	for (int t = 0; t < n_threads; ++t) if (!out->parts[t].err.empty()) { *err = out->parts[t].err; return -1; }
	w.cycles(&out->parts[n_threads]);
	if (!out->parts[n_threads].err.empty()) { *err = out->parts[n_threads].err; return -1; }
	return 0;
}

/* the FASTA of the command, part by part: `put` takes a piece of text and returns false when it cannot be written */
template <class Put> static inline bool ug_fasta(const ug_result_t &r, Put put)
{
	std::string text;
	char head[160];
	uint64_t j = 0;
	for (const ug_part_t &p : r.parts) {
		for (const ug_unitig_t &u : p.u) {
			const uint64_t len = u.n_node + (uint64_t)r.k - 1;
			text.append(head, (size_t)snprintf(head, sizeof head, ">u%llu\tLN:i:%llu\tKC:i:%llu\tkm:f:%.1f\tCL:i:%d\n", (unsigned long long)j++,
			                                   (unsigned long long)len, (unsigned long long)u.kc, (double)u.kc / (double)u.n_node, u.cycle));
			text.append(p.seq, u.at, len).push_back('\n');
			if (text.size() >= (size_t)1 << 22) { if (!put(text)) return false; text.clear(); }
		}
	}
	return text.empty() || put(text);
}

/* the U line of the command's -s form: open unitigs, cycles, bases, the longest, and the N50 -- the largest L such that the unitigs of at least L
 * bases hold half of all bases or more; 0 without a unitig */
static inline std::string ug_stat_line(const ug_result_t &r)
{
	std::vector<uint64_t> len;
	uint64_t n_open = 0, n_cycle = 0, sum = 0, n50 = 0;
	for (const ug_part_t &p : r.parts)
		for (const ug_unitig_t &u : p.u) { len.push_back(u.n_node + (uint64_t)r.k - 1); sum += len.back(); if (u.cycle) ++n_cycle; else ++n_open; }
	std::sort(len.begin(), len.end(), [](uint64_t a, uint64_t b) { return a > b; });
	uint64_t acc = 0;
	for (uint64_t l : len) { acc += l; if (2 * acc >= sum) { n50 = l; break; } }
	char line[160];
	snprintf(line, sizeof line, "U\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)n_open, (unsigned long long)n_cycle, (unsigned long long)sum,
	         (unsigned long long)(len.empty() ? 0 : len[0]), (unsigned long long)n50);
	return line;
}
#endif
