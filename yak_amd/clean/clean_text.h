/* clean_text.h -- the report of `yak-amd clean` (include/yak_amd_clean.h) made on the host, HIP-free like clean_step.h: the
 * first line, an R line per round, a T or P line per removed unitig, the C line.  clean.hip and tests/tools/clean_model_check.cpp share it. */
#ifndef YK_CLEAN_TEXT_H
#define YK_CLEAN_TEXT_H
#include <stdio.h>
#include <string>
#include "../bubble/bubble_text.h"
#include "clean_step.h"

/* yakamd_cleanround_t */
struct clt_round_t { uint64_t n_key, n_unitig, n_link, n_bubble, n_tip, tip_nodes, n_pop, pop_nodes, removed; };

/* `#clean k=<k> min_cnt=<c> tip_nodes=<T> pop_pct=<P>` */
static inline std::string clt_head(int k, int min_cnt, int tip_nodes, int pop_pct)
{
	char line[128];
	return std::string(line, (size_t)snprintf(line, sizeof line, "#clean\tk=%d\tmin_cnt=%d\ttip_nodes=%d\tpop_pct=%d\n", k, min_cnt, tip_nodes, pop_pct));
}

/* `R <r> <n_key> <n_unitig> <n_link> <n_bubble> <tips> <tip_nodes> <pops> <pop_nodes> <removed>` */
static inline std::string clt_round(uint64_t r, const clt_round_t &s)
{
	const uint64_t v[10] = { r, s.n_key, s.n_unitig, s.n_link, s.n_bubble, s.n_tip, s.tip_nodes, s.n_pop, s.pop_nodes, s.removed };
	std::string out = "R";
	for (int i = 0; i < 10; ++i) { out += '\t'; gft_decimal(out, v[i]); }
	out += '\n';
	return out;
}

/* `T <r> u<j> <n_node> <kc> u<anchor><+|->` / `P <r> u<j> <n_node> <kc> u<winner><+|->` per record.  false for a record whose why is neither, or
 * for a piece that `put` could not write */
template <class Put> static inline bool clt_records(uint64_t r, const cl_rec_t *rec, uint64_t n_rec, Put put)
{
	std::string text;
	for (uint64_t i = 0; i < n_rec; ++i) {
		const cl_rec_t &c = rec[i];
		if (c.why != CL_TIP && c.why != CL_POP) return false;
		text += c.why == CL_TIP ? "T\t" : "P\t"; gft_decimal(text, r);
		text += "\tu"; gft_decimal(text, c.unitig);
		text += '\t'; gft_decimal(text, c.n_node);
		text += '\t'; gft_decimal(text, c.kc);
		bbt_end(text, c.other);
		text += '\n';
		if (text.size() >= (size_t)1 << 22) { if (!put(text)) return false; text.clear(); }
	}
	return text.empty() || put(text);
}

/* `C <rounds> <n_key_in> <n_key_after_shrink> <n_key_out>` */
static inline std::string clt_last(uint64_t rounds, uint64_t n_in, uint64_t n_shrunk, uint64_t n_out)
{
	const uint64_t v[4] = { rounds, n_in, n_shrunk, n_out };
	std::string out = "C";
	for (int i = 0; i < 4; ++i) { out += '\t'; gft_decimal(out, v[i]); }
	out += '\n';
	return out;
}
#endif
