/* phase_text.h -- the text of `yak-amd bubbles -r -p` (include/yak_amd_phase.h) made on the host, HIP-free like phase_step.h:
 * the header, the H lines from the nodes, the K lines from the blocks, the E lines from the edges and the pairs, and the T line; the A lines are
 * those of ../allele/allele_text.h.  phase.hip and tools/phase_model_check.cpp share it. */
#ifndef YK_PHASE_TEXT_H
#define YK_PHASE_TEXT_H
#include <algorithm>
#include "../allele/allele_text.h"
#include "phase_step.h"

struct pht_total_t { uint64_t n_seq, len, path, step, obs, full, vote; };
/* what the T line takes from the solve */
struct pht_solve_t { uint64_t n_pair, n_het, n_edge, n_forest, n_block, n_single; };

/* `#phase k=<k> min_cnt=<c> min_sup=<m> min_link=<e>` */
static inline void pht_head(std::string &text, int k, int min_cnt, int min_sup, int min_link)
{
	char line[128];
	text.append(line, (size_t)snprintf(line, sizeof line, "#phase\tk=%d\tmin_cnt=%d\tmin_sup=%d\tmin_link=%d\n", k, min_cnt, min_sup, min_link));
}

static inline void pht_line(std::string &text, char tag, const uint64_t *v, int n, const char *last)
{
	text += tag;
	for (int x = 0; x < n; ++x) { text += '\t'; gft_decimal(text, v[x]); }
	if (last) { text += '\t'; text += last; }
	text += '\n';
}

/* `H i block <0|1>` per het bubble, i ascending */
static inline void pht_nodes(std::string &text, const ph_node_t *node, uint64_t n_bubble)
{
	for (uint64_t i = 0; i < n_bubble; ++i) {
		if (node[i].block == PH_NONE) continue;
		const uint64_t v[3] = { i, node[i].block, node[i].flags & 1u };
		pht_line(text, 'H', v, 3, 0);
	}
}

/* `K block n_bubble n_edge n_disc w_sum w_disc` per block of two or more, as the records stand (ascending); *n_disc = the discordant edges of all
 * blocks, *max_block is raised to the largest n_bubble; the lines are appended only if `write` */
static inline void pht_blocks(std::string &text, const ph_block_t *blk, uint64_t n_block, bool write, uint64_t *n_disc, uint64_t *max_block)
{
	for (uint64_t b = 0; b < n_block; ++b) {
		const uint64_t v[6] = { blk[b].block, blk[b].n_bubble, blk[b].n_edge, blk[b].n_disc, blk[b].w_sum, blk[b].w_disc };
		*n_disc += v[3];
		if (v[1] > *max_block) *max_block = v[1];
		if (write) pht_line(text, 'K', v, 6, 0);
	}
}

/* `E i j cis trans <forest|conc|disc>` per edge, sorted by (i, j) here: both lists are put in that order.  false for an edge without its pair */
static inline bool pht_edges(std::string &text, std::vector<ph_edge_t> &edge, std::vector<ph_pair_t> &pair)
{
	std::sort(edge.begin(), edge.end(), [](const ph_edge_t &a, const ph_edge_t &b) { return a.i != b.i ? a.i < b.i : a.j < b.j; });
	std::sort(pair.begin(), pair.end(), [](const ph_pair_t &a, const ph_pair_t &b) { return a.i != b.i ? a.i < b.i : a.j < b.j; });
	size_t p = 0;
	for (const ph_edge_t &e : edge) {
		while (p < pair.size() && (pair[p].i != e.i ? pair[p].i < e.i : pair[p].j < e.j)) ++p;
		if (p == pair.size() || pair[p].i != e.i || pair[p].j != e.j) return false;
		const uint64_t v[4] = { e.i, e.j, pair[p].cis, pair[p].trans };
		pht_line(text, 'E', v, 4, e.flags & PH_FOREST ? "forest" : e.flags & PH_DISC ? "disc" : "conc");
	}
	return true;
}

/* `T n_seq sum_len n_path n_step n_obs n_full n_vote n_pair n_bubble n_het n_edge n_forest n_disc n_block n_single max_block`; a het bubble alone
 * is a block of one */
static inline void pht_tail(std::string &text, const pht_total_t &t, uint64_t n_bubble, const pht_solve_t &s, uint64_t n_disc, uint64_t max_block)
{
	if (s.n_single && max_block < 1) max_block = 1;
	const uint64_t v[16] = { t.n_seq, t.len, t.path, t.step, t.obs, t.full, t.vote, s.n_pair, n_bubble, s.n_het, s.n_edge, s.n_forest, n_disc, s.n_block, s.n_single, max_block };
	pht_line(text, 'T', v, 16, 0);
}
#endif
