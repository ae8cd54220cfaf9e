/* gfa_text.h -- the two texts of `yak-amd unitigs -G` (include/yak_amd_gfa.h) made on the host, HIP-free like gfa_step.h: the
 * GFA from the descriptors, the bases and the links, and the -s form from the tallies.  gfa.hip and tests/tools/gfa_model_check.cpp share it. */
#ifndef YK_GFA_TEXT_H
#define YK_GFA_TEXT_H
#include <stdio.h>
#include <string>
#include "gfa_step.h"

/* what the -s text states: the options, the graph's tallies (yakamd_gstat_t) and the walk's (yakamd_uwstat_t) */
struct gft_tallies_t { int k, min_cnt; uint64_t n_key, n_node, n_arc, n_linked_side, deg[5][5], n_open, n_cycle, sum_len, max_len, n50; };
/* filled from the two; templates, so that this header needs neither declaration */
template<class Graph, class Walk>
static inline gft_tallies_t gft_tallies(int k, int min_cnt, const Graph &gs, const Walk &us)
{
	gft_tallies_t t;
	t.k = k; t.min_cnt = min_cnt;
	t.n_key = gs.n_key; t.n_node = gs.n_node; t.n_arc = gs.n_arc; t.n_linked_side = gs.n_linked_side;
	for (int l = 0; l < 5; ++l) for (int r = 0; r < 5; ++r) t.deg[l][r] = gs.deg[l][r];
	t.n_open = us.n_open; t.n_cycle = us.n_cycle; t.sum_len = us.sum_len; t.max_len = us.max_len; t.n50 = us.n50;
	return t;
}

/* the text of `unitigs -s` restated line by line, then `G n_link end_deg[0] .. end_deg[4]` */
static inline std::string gft_stats(const gft_tallies_t &t, uint64_t n_link, const uint64_t end_deg[5])
{
	typedef unsigned long long ull;
	char line[200];
	std::string out;
	out.append(line, (size_t)snprintf(line, sizeof line, "#unitigs\tk=%d\tmin_cnt=%d\n", t.k, t.min_cnt));
	out.append(line, (size_t)snprintf(line, sizeof line, "N\t%llu\t%llu\t%llu\t%llu\n", (ull)t.n_key, (ull)t.n_node, (ull)t.n_arc, (ull)t.n_linked_side));
	for (int l = 0; l < 5; ++l)
		for (int r = 0; r < 5; ++r)
			if (t.deg[l][r]) out.append(line, (size_t)snprintf(line, sizeof line, "D\t%d\t%d\t%llu\n", l, r, (ull)t.deg[l][r]));
	out.append(line, (size_t)snprintf(line, sizeof line, "U\t%llu\t%llu\t%llu\t%llu\t%llu\n", (ull)t.n_open, (ull)t.n_cycle, (ull)t.sum_len, (ull)t.max_len, (ull)t.n50));
	out.append(line, (size_t)snprintf(line, sizeof line, "G\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", (ull)n_link, (ull)end_deg[0], (ull)end_deg[1], (ull)end_deg[2],
	                                  (ull)end_deg[3], (ull)end_deg[4]));
	return out;
}

/* v in decimal behind text: the lines by the million are put together without snprintf (km:f: keeps it, for its rounding) */
static inline void gft_decimal(std::string &text, uint64_t v)
{
	char buf[20];
	int n = 20;
	do { buf[--n] = (char)('0' + v % 10); v /= 10; } while (v);
	text.append(buf + n, (size_t)(20 - n));
}

/* GFA 1: the header, a segment per unitig, a link per record.  `put` takes a piece of text and returns false when it cannot be written; false as
 * well for a descriptor outside the n_bases bases or a link that names no unitig */
template <class Put> static inline bool gft_gfa(const gf_desc_t *desc, uint64_t n, const char *bases, uint64_t n_bases, const gf_link_t *links, uint64_t n_link, int k, Put put)
{
	std::string text = "H\tVN:Z:1.0\n", overlap = "\t";
	char buf[64];
	gft_decimal(overlap, (uint64_t)(k - 1));
	overlap += "M\n";
	for (uint64_t j = 0; j < n; ++j) {
		const gf_desc_t &u = desc[j];
		if (u.n_node < 1 || u.off > n_bases || u.n_node > n_bases - u.off || (uint64_t)(k - 1) > n_bases - u.off - u.n_node) return false;
		const uint64_t len = u.n_node + (uint64_t)k - 1;
		text += "S\tu"; gft_decimal(text, j);
		text += '\t'; text.append(bases + u.off, (size_t)len);
		text += "\tLN:i:"; gft_decimal(text, len);
		text += "\tKC:i:"; gft_decimal(text, u.kc);
		text.append(buf, (size_t)snprintf(buf, sizeof buf, "\tkm:f:%.1f", (double)u.kc / (double)u.n_node));
		text += u.first & 1 ? "\tcl:i:1\n" : "\tcl:i:0\n";
		if (text.size() >= (size_t)1 << 22) { if (!put(text)) return false; text.clear(); }
	}
	for (uint64_t i = 0; i < n_link; ++i) {
		const gf_link_t &l = links[i];
		if (l.from >> 1 >= n || l.to >> 1 >= n) return false;
		text += "L\tu"; gft_decimal(text, l.from >> 1);
		text += l.from & 1 ? "\t-\tu" : "\t+\tu"; gft_decimal(text, l.to >> 1);
		text += l.to & 1 ? "\t-" : "\t+";
		text += overlap;
		if (text.size() >= (size_t)1 << 22) { if (!put(text)) return false; text.clear(); }
	}
	return text.empty() || put(text);
}
#endif
