/* uwalk_host.h -- the host's share of the device walk, HIP-free like uwalk_step.h: the cycles, which the ranking leaves
 * unfinished and whose records alone come to the host, compacted in listing order; the tallies of the descriptors; and the command's two texts made
 * from the descriptors and the bases.  walk.hip and tests/tools/uwalk_model_check.cpp share it. */
#ifndef YK_UWALK_HOST_H
#define YK_UWALK_HOST_H
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>
#include "uwalk_step.h"

/* what the host makes of the cycles: a map entry per compacted record, and the descriptors and bases that follow those of the open unitigs */
struct uwh_cycles_t { std::vector<uw_map_t> map; std::vector<uw_desc_t> desc; std::string bases; };

/* rec[i] is the record of listing index idx[i], idx ascending, all of them nodes on cycles.  The cycles ascending by their smallest index, each
 * from that node as stored through R; j0 and off0 are the number and the bases of the open unitigs in front.  0, or -1 with *err set */
static inline int uwh_cycles(const uw_node_t *rec, const uint64_t *idx, uint64_t nc, int k, uint64_t j0, uint64_t off0, uwh_cycles_t *out, std::string *err)
{
	char msg[96];
	std::vector<char> seen((size_t)nc, 0);
	out->map.assign((size_t)nc, uw_map_t{ UW_NONE, 0 });
	for (uint64_t i = 0; i < nc; ++i) {
		if (seen[i]) continue;
		uw_desc_t u = { off0 + out->bases.size(), 0, 0, idx[i] << 1 | 1 };
		uint64_t cur = i;
		int d = 0;
		bool ok = true;
		for (;;) {
			seen[cur] = 1;
			out->map[cur] = uw_map_t{ j0 + out->desc.size(), u.n_node << 1 | (uint64_t)d };
			u.kc += rec[cur].count;
			if (u.n_node == 0) for (int b = 0; b < k; ++b) out->bases.push_back(uw_base_at(rec[cur].x, d, k, b));
			else out->bases.push_back(uw_last_base(rec[cur].x, d, k));
			++u.n_node;
			const uint64_t lk = rec[cur].link[d];
			if (lk == UW_NONE) { ok = false; break; }
			const uint64_t to = lk >> 1;
			d = (int)(lk & 1) ^ 1;
			if (to == idx[i]) { ok = d == 0; break; }
			const uint64_t *at = std::lower_bound(idx, idx + nc, to);
			if (at == idx + nc || *at != to || seen[at - idx]) { ok = false; break; }
			cur = (uint64_t)(at - idx);
		}
		if (!ok) {
			snprintf(msg, sizeof msg, "the links from key %llu do not come back to it", (unsigned long long)idx[i]);
			*err = msg;
			return -1;
		}
		out->desc.push_back(u);
	}
	return 0;
}

/* the tallies of the U line from the descriptors: bases in all, the longest, and the N50 -- the largest L such that the unitigs of at least L bases
 * hold half of all bases or more; 0 without a unitig */
static inline void uwh_lengths(const uw_desc_t *desc, uint64_t n, int k, uint64_t *sum_len, uint64_t *max_len, uint64_t *n50)
{
	std::vector<uint64_t> len((size_t)n);
	uint64_t sum = 0, acc = 0;
	for (uint64_t j = 0; j < n; ++j) { len[j] = desc[j].n_node + (uint64_t)k - 1; sum += len[j]; }
	std::sort(len.begin(), len.end(), [](uint64_t a, uint64_t b) { return a > b; });
	*sum_len = sum; *max_len = n ? len[0] : 0; *n50 = 0;
	for (uint64_t l : len) { acc += l; if (2 * acc >= sum) { *n50 = l; break; } }
}

static inline std::string uwh_u_line(uint64_t n_open, uint64_t n_cycle, uint64_t sum_len, uint64_t max_len, uint64_t n50)
{
	char line[160];
	snprintf(line, sizeof line, "U\t%llu\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)n_open, (unsigned long long)n_cycle, (unsigned long long)sum_len,
	         (unsigned long long)max_len, (unsigned long long)n50);
	return line;
}

/* the FASTA of the command from the descriptors and the bases: `put` takes a piece of text and returns false when it cannot be written */
template <class Put> static inline bool uwh_fasta(const uw_desc_t *desc, uint64_t n, const char *bases, int k, Put put)
{
	std::string text;
	char head[160];
	for (uint64_t j = 0; j < n; ++j) {
		const uw_desc_t &u = desc[j];
		const uint64_t len = u.n_node + (uint64_t)k - 1;
		text.append(head, (size_t)snprintf(head, sizeof head, ">u%llu\tLN:i:%llu\tKC:i:%llu\tkm:f:%.1f\tCL:i:%d\n", (unsigned long long)j, (unsigned long long)len,
		                                   (unsigned long long)u.kc, (double)u.kc / (double)u.n_node, (int)(u.first & 1)));
		text.append(bases + u.off, (size_t)len).push_back('\n');
		if (text.size() >= (size_t)1 << 22) { if (!put(text)) return false; text.clear(); }
	}
	return text.empty() || put(text);
}
#endif
