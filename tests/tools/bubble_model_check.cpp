/* bubble_model_check.cpp -- the simple bubbles of `yak-amd bubbles` (yak_amd/bubble/bubble_step.h, bubble_text.h) as a sequential program of its own,
 * for the host compiler and its sanitizers: bubble_model_check <file> text|stats|records reads the file tests/bubble_util.py model_file() writes
 * (64-bit words: k, min_cnt, the numbers of unitigs, bases and links, the graph's tallies, the U line's numbers, end_deg; the descriptors, the links;
 * then the bases) and does what the kernels of yak_amd/bubble/bubble.hip do, link by link, end by end and bubble by bubble, with the very functions
 * they call: the first link of every end, the count, the exclusive scan, the emit at the ranks, the classification position by position.  It
 * prints the B lines, the -s text, or the records as their ten words with a last line `T n_bubble n_S n_E n_I n_fork n_tip tip_nodes
 * max_arm_nodes`.  Exit 1 after a message when the file cannot be read, the list of links does not fit, or an arm does not fit the bases. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../yak_amd/bubble/bubble_text.h"

static int fail(const char *what) { fprintf(stderr, "bubble: %s\n", what); return 1; }

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: bubble_model_check <file> text|stats|records\n"); return 2; }
	FILE *fp = fopen(argv[1], "rb");
	uint64_t head[44];
	if (!fp || fread(head, 8, 44, fp) != 44) return fail("cannot read the file");
	const int k = (int)head[0];
	const uint64_t n_u = head[2], n_bases = head[3], n_link = head[4], n_end = 2 * n_u;
	gft_tallies_t t;
	t.k = k; t.min_cnt = (int)head[1];
	t.n_key = head[5]; t.n_node = head[6]; t.n_arc = head[7]; t.n_linked_side = head[8];
	for (int i = 0; i < 25; ++i) t.deg[i / 5][i % 5] = head[9 + i];
	t.n_open = head[34]; t.n_cycle = head[35]; t.sum_len = head[36]; t.max_len = head[37]; t.n50 = head[38];
	const uint64_t *end_deg = head + 39;
	if (k < 3 || k > 31 || !(k & 1)) return fail("k must be odd and in [3, 31]");
	std::vector<bb_desc_t> desc((size_t)n_u);
	std::vector<bb_link_t> links((size_t)n_link);                       /* exactly n_link and n_bases: a read past them is the sanitizer's */
	std::vector<char> bases((size_t)n_bases);
	if (n_u && fread(desc.data(), sizeof(bb_desc_t), (size_t)n_u, fp) != n_u) return fail("the file is short");
	if (n_link && fread(links.data(), sizeof(bb_link_t), (size_t)n_link, fp) != n_link) return fail("the file is short");
	if (n_bases && fread(bases.data(), 1, (size_t)n_bases, fp) != n_bases) return fail("the file is short");
	fclose(fp);

	/* the first link of every end */
	std::vector<bb_run_t> runs((size_t)n_end, bb_run_t{ BB_NONE, BB_NONE });
	for (uint64_t i = 0; i < n_link; ++i) {
		uint64_t e = 0;
		bb_run_t run;
		const int r = bb_first(links.data(), n_link, i, n_end, &e, &run);
		if (r < 0) return fail("the list of links does not fit: it is not sorted, names an end outside the unitigs or gives an end more than 4 links");
		if (r == 1) runs[(size_t)e] = run;
	}

	/* count, scan, emit */
	bbt_stats_t st;
	memset(&st, 0, sizeof st);
	std::vector<uint64_t> cnt((size_t)n_end + 1, 0);
	uint64_t bad = 0;
	for (uint64_t e = 0; e < n_end; ++e) {
		bb_rec_t r;
		unsigned flags;
		uint64_t tn;
		const int is = bb_find(desc.data(), n_u, runs.data(), links.data(), n_link, e, k, &r, &flags, &tn, &bad);
		cnt[(size_t)e] = (uint64_t)is;
		if (flags & BB_FORK) ++st.n_fork;
		if (flags & BB_TIP) ++st.n_tip;
		st.tip_nodes += tn;
		if (is) for (int a = 0; a < 2; ++a) if (r.n_node[a] > st.max_arm_nodes) st.max_arm_nodes = r.n_node[a];
	}
	if (bad) return fail("the links do not fit the unitigs");
	uint64_t n_bubble = 0;
	for (uint64_t e = 0; e <= n_end; ++e) { const uint64_t v = cnt[(size_t)e]; cnt[(size_t)e] = n_bubble; n_bubble += v; }
	bb_rec_t none;
	memset(&none, 0xff, sizeof none);
	std::vector<bb_rec_t> rec((size_t)n_bubble, none);
	for (uint64_t e = 0; e < n_end; ++e) {
		bb_rec_t r;
		unsigned flags;
		uint64_t tn;
		if (!bb_find(desc.data(), n_u, runs.data(), links.data(), n_link, e, k, &r, &flags, &tn, &bad)) continue;
		if (cnt[(size_t)e] >= n_bubble || cnt[(size_t)e] + 1 != cnt[(size_t)e + 1]) return fail("the emit does not repeat the count");
		r.hd = r.type = BB_NONE;
		rec[(size_t)cnt[(size_t)e]] = r;
	}

	/* classify: position by position, as the lanes of a wave do */
	for (bb_rec_t &r : rec) {
		r.type = bb_type(r.n_node[0], r.n_node[1], k);
		r.hd = BB_NONE;
		if (r.type != BB_I) {
			uint64_t off[2], len = 0, len2 = 0;
			if (bb_arm(desc.data(), n_u, n_bases, r.arm[0], r.n_node[0], k, &off[0], &len) != 0 || bb_arm(desc.data(), n_u, n_bases, r.arm[1], r.n_node[1], k, &off[1], &len2) != 0)
				return fail("an arm does not fit the bases");
			r.hd = 0;
			for (uint64_t p = 0; p < len; ++p) {
				const int m = bb_mismatch(bases.data(), off, len, r.arm, p);
				if (m < 0) return fail("an arm holds a byte that is none of ACGT");
				r.hd += (uint64_t)m;
			}
		}
		++st.n_type[r.type];
	}
	st.n_bubble = n_bubble;

	typedef unsigned long long ull;
	if (strcmp(argv[2], "stats") == 0) fputs((gft_stats(t, n_link, end_deg) + bbt_stats_line(st)).c_str(), stdout);
	else if (strcmp(argv[2], "records") == 0) {
		for (const bb_rec_t &r : rec)
			printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (ull)r.src, (ull)r.sink, (ull)r.arm[0], (ull)r.arm[1], (ull)r.n_node[0], (ull)r.n_node[1], (ull)r.kc[0],
			       (ull)r.kc[1], (ull)r.hd, (ull)r.type);
		printf("T %llu %llu %llu %llu %llu %llu %llu %llu\n", (ull)st.n_bubble, (ull)st.n_type[0], (ull)st.n_type[1], (ull)st.n_type[2], (ull)st.n_fork, (ull)st.n_tip,
		       (ull)st.tip_nodes, (ull)st.max_arm_nodes);
	} else if (!bbt_bubbles(rec.data(), n_bubble, desc.data(), n_u, bases.data(), n_bases, k, t.min_cnt, [](const std::string &s) { return fwrite(s.data(), 1, s.size(), stdout) == s.size(); }))
		return fail("the text cannot be written");
	return fflush(stdout) == 0 ? 0 : 1;
}
