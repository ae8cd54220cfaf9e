/* bubble_text.h -- the two texts of `yak-amd bubbles` (include/yak_amd_bubble.h) made on the host, HIP-free like
 * bubble_step.h: the B lines from the records, the descriptors and the bases, and the -s form, which is the -s text of `unitigs -G`
 * (../gfa/gfa_text.h) and one line more.  bubble.hip and tests/tools/bubble_model_check.cpp share it. */
#ifndef YK_BUBBLE_TEXT_H
#define YK_BUBBLE_TEXT_H
#include <stdio.h>
#include <string>
#include "../gfa/gfa_text.h"
#include "bubble_step.h"

/* yakamd_bubstat_t */
struct bbt_stats_t { uint64_t n_bubble, n_type[3], n_tip, tip_nodes, max_arm_nodes, n_fork; };

/* `B n_bubble n_S n_E n_I n_fork n_tip tip_nodes max_arm_nodes` */
static inline std::string bbt_stats_line(const bbt_stats_t &s)
{
	const uint64_t v[8] = { s.n_bubble, s.n_type[BB_S], s.n_type[BB_E], s.n_type[BB_I], s.n_fork, s.n_tip, s.tip_nodes, s.max_arm_nodes };
	std::string out = "B";
	for (int i = 0; i < 8; ++i) { out += '\t'; gft_decimal(out, v[i]); }
	out += '\n';
	return out;
}

/* `u<j><+|->` behind a tab */
static inline void bbt_end(std::string &text, uint64_t e)
{
	text += "\tu"; gft_decimal(text, e >> 1);
	text += e & 1 ? '-' : '+';
}

/* the header and a line per record.  `put` takes a piece of text and returns false when it cannot be written; false as well for a record whose
 * ends name no unitig, whose type is none of the three or whose arms do not lie inside the n_bases bases as the record states them */
template <class Put> static inline bool bbt_bubbles(const bb_rec_t *rec, uint64_t n_rec, const bb_desc_t *desc, uint64_t n_unitig, const char *bases, uint64_t n_bases,
                                                    int k, int min_cnt, Put put)
{
	char line[64];
	std::string text(line, (size_t)snprintf(line, sizeof line, "#bubbles\tk=%d\tmin_cnt=%d\n", k, min_cnt));
	for (uint64_t i = 0; i < n_rec; ++i) {
		const bb_rec_t &r = rec[i];
		if (r.src >> 1 >= n_unitig || r.sink >> 1 >= n_unitig || r.type > BB_I) return false;
		text += "B\t"; gft_decimal(text, i);
		bbt_end(text, r.src); bbt_end(text, r.arm[0]); bbt_end(text, r.arm[1]); bbt_end(text, r.sink);
		text += '\t'; text += "SEI"[r.type];
		text += '\t'; gft_decimal(text, r.n_node[0]);
		text += '\t'; gft_decimal(text, r.n_node[1]);
		text += '\t';
		if (r.hd == BB_NONE) text += '.'; else gft_decimal(text, r.hd);
		text += '\t'; gft_decimal(text, r.kc[0]);
		text += '\t'; gft_decimal(text, r.kc[1]);
		for (int a = 0; a < 2; ++a) {                              /* the allele: A[k - 1 : n_node] of the oriented string */
			uint64_t off, len;
			if (bb_arm(desc, n_unitig, n_bases, r.arm[a], r.n_node[a], k, &off, &len) != 0) return false;
			text += '\t';
			if (r.n_node[a] < (uint64_t)k) { text += '*'; continue; }
			for (uint64_t p = (uint64_t)(k - 1); p < r.n_node[a]; ++p) {
				const int b = bb_base(bases, off, len, (int)(r.arm[a] & 1), p);
				if (b < 0) return false;
				text += "ACGT"[b];
			}
		}
		text += '\n';
		if (text.size() >= (size_t)1 << 22) { if (!put(text)) return false; text.clear(); }
	}
	return text.empty() || put(text);
}
#endif
