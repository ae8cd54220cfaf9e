/* allele_text.h -- the text of `yak-amd bubbles -r` (include/yak_amd_allele.h) made on the host, HIP-free like allele_step.h:
 * the header, the F lines of a chunk from its observation records, the A lines from the bubble records and the support, and the T line.  allele.hip
 * and tools/allele_model_check.cpp share it. */
#ifndef YK_ALLELE_TEXT_H
#define YK_ALLELE_TEXT_H
#include <stdio.h>
#include <string>
#include <vector>
#include "../bubble/bubble_text.h"
#include "allele_step.h"

struct alt_total_t { uint64_t n_seq, len, path, step, obs, full, frag; };

/* `#alleles k=<k> min_cnt=<c> min_sup=<m>` */
static inline void alt_head(std::string &text, int k, int min_cnt, int min_sup)
{
	char line[96];
	text.append(line, (size_t)snprintf(line, sizeof line, "#alleles\tk=%d\tmin_cnt=%d\tmin_sup=%d\n", k, min_cnt, min_sup));
}

/* the F lines of a chunk: per sequence with min_frag full observations or more `F name n i:<1|2><+|-> ...`, the full observations in the order of
 * the records, which is read order.  The records are in image order, so those of a sequence are one run.  The lines are counted in tot->frag and
 * appended only if `write`.  false for a record that names no sequence of the chunk or no bubble, or for records out of order */
static inline bool alt_fragments(std::string &text, const std::vector<std::string> &name, const al_obs_t *obs, uint64_t n_obs, uint64_t n_bubble, uint64_t min_frag,
                                 bool write, alt_total_t *tot)
{
	std::string line;
	for (uint64_t r = 0; r < n_obs;) {
		const uint32_t seq = obs[r].seq;
		if (seq >= name.size() || (r && obs[r - 1].seq > seq)) return false;
		uint64_t n = 0;
		line.clear();
		for (; r < n_obs && obs[r].seq == seq; ++r) {
			const al_obs_t &o = obs[r];
			if (o.bubble >= n_bubble) return false;
			if (!(o.flags & AL_FULL)) continue;
			++n;
			line += '\t'; gft_decimal(line, o.bubble);
			line += ':'; line += o.flags & AL_A ? '2' : '1';
			line += o.flags & AL_REV ? '-' : '+';
		}
		if (n < min_frag) continue;
		++tot->frag;
		if (!write) continue;
		text += "F\t"; text += name[seq];
		text += '\t'; gft_decimal(text, n);
		text += line; text += '\n';
	}
	return true;
}

/* an A line per bubble, `A i u<a1><+|-> u<a2><+|-> full1 full2 part1 part2 <het|hom1|hom2|none>`, and the calls counted in n_call[4]; the lines
 * are appended only if `write` */
static inline void alt_alleles(std::string &text, const bb_rec_t *rec, const al_sup_t *sup, uint64_t n_bubble, uint64_t min_sup, bool write, uint64_t n_call[4])
{
	static const char *const CALL[4] = { "het", "hom1", "hom2", "none" };
	for (uint64_t i = 0; i < n_bubble; ++i) {
		const int c = al_call(&sup[i], min_sup);
		++n_call[c];
		if (!write) continue;
		text += "A\t"; gft_decimal(text, i);
		bbt_end(text, rec[i].arm[0]); bbt_end(text, rec[i].arm[1]);
		const uint64_t v[4] = { sup[i].full[0], sup[i].full[1], sup[i].part[0], sup[i].part[1] };
		for (int x = 0; x < 4; ++x) { text += '\t'; gft_decimal(text, v[x]); }
		text += '\t'; text += CALL[c]; text += '\n';
	}
}

/* `T n_seq sum_len n_path n_step n_obs n_full n_frag n_bubble n_het n_hom1 n_hom2 n_none` */
static inline void alt_tail(std::string &text, const alt_total_t &t, uint64_t n_bubble, const uint64_t n_call[4])
{
	const uint64_t v[12] = { t.n_seq, t.len, t.path, t.step, t.obs, t.full, t.frag, n_bubble, n_call[0], n_call[1], n_call[2], n_call[3] };
	text += 'T';
	for (int x = 0; x < 12; ++x) { text += '\t'; gft_decimal(text, v[x]); }
	text += '\n';
}
#endif
