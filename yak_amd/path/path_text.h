/* path_text.h -- the two texts of `yak-amd paths` (include/yak_amd_path.h) made on the host, HIP-free like path_step.h: the GAF
 * lines from a chunk's path records and steps, and the -s form from its tallies; a chunk's sequences are their names and, beside them, their
 * lengths.  path.hip and tests/tools/path_model_check.cpp share it. */
#ifndef YK_PATH_TEXT_H
#define YK_PATH_TEXT_H
#include <stdio.h>
#include <string>
#include <vector>
#include "path_step.h"

struct pxt_total_t { uint64_t n_seq, len, kmer, hit, path, step; };

static inline void pxt_decimal(std::string &text, uint64_t v)
{
	char buf[20];
	int n = 20;
	do { buf[--n] = (char)('0' + v % 10); v /= 10; } while (v);
	text.append(buf + n, (size_t)(20 - n));
}

/* one GAF line per path of the chunk with qe - qs >= min_len, appended to text: name len qs qe + <path> plen ps pe nm nm 255.  n_node[j] = the nodes
 * of unitig j.  false for a record that names no sequence of the chunk, no step of the list or no unitig */
static inline bool pxt_gaf(std::string &text, const std::vector<std::string> &name, const uint32_t *len, const px_path_t *paths, uint64_t n_path, const uint64_t *steps, uint64_t n_step,
                           const uint32_t *n_node, uint64_t n_unitig, int k, int min_len)
{
	for (uint64_t r = 0; r < n_path; ++r) {
		const px_path_t &p = paths[r];
		if (p.seq >= name.size() || p.qe < p.qs || p.step_off > n_step || p.n_step > n_step - p.step_off || p.n_step < 1) return false;
		const uint64_t span = p.qe - p.qs;
		if (span < (uint64_t)(min_len > 0 ? min_len : 0)) continue;
		text += name[p.seq]; text += '\t'; pxt_decimal(text, len[p.seq]);
		text += '\t'; pxt_decimal(text, p.qs);
		text += '\t'; pxt_decimal(text, p.qe);
		text += "\t+\t";
		uint64_t plen = (uint64_t)(k - 1);
		for (uint64_t x = 0; x < p.n_step; ++x) {
			const uint64_t st = steps[p.step_off + x], j = st >> 1;
			if (j >= n_unitig) return false;
			plen += n_node[j];
			text += st & 1 ? "<u" : ">u";
			pxt_decimal(text, j);
		}
		text += '\t'; pxt_decimal(text, plen);
		text += '\t'; pxt_decimal(text, p.ps);
		text += '\t'; pxt_decimal(text, p.ps + span);
		text += '\t'; pxt_decimal(text, span);
		text += '\t'; pxt_decimal(text, span);
		text += "\t255\n";
	}
	return true;
}

static inline void pxt_stats_head(std::string &text, int k, int min_cnt)
{
	char line[80];
	text.append(line, (size_t)snprintf(line, sizeof line, "#paths\tk=%d\tmin_cnt=%d\n", k, min_cnt));
}
/* an S line per sequence of the chunk, added to the totals */
static inline void pxt_stats(std::string &text, const std::vector<std::string> &name, const uint32_t *len, const px_tally_t *tally, pxt_total_t *tot)
{
	for (size_t s = 0; s < name.size(); ++s) {
		const px_tally_t &t = tally[s];
		text += "S\t"; text += name[s];
		text += '\t'; pxt_decimal(text, len[s]);
		text += '\t'; pxt_decimal(text, t.n_kmer);
		text += '\t'; pxt_decimal(text, t.n_hit);
		text += '\t'; pxt_decimal(text, t.n_path);
		text += '\t'; pxt_decimal(text, t.n_step);
		text += '\n';
		++tot->n_seq; tot->len += len[s]; tot->kmer += t.n_kmer; tot->hit += t.n_hit; tot->path += t.n_path; tot->step += t.n_step;
	}
}
static inline void pxt_stats_tail(std::string &text, const pxt_total_t &t)
{
	text += "T";
	const uint64_t v[6] = { t.n_seq, t.len, t.kmer, t.hit, t.path, t.step };
	for (int x = 0; x < 6; ++x) { text += '\t'; pxt_decimal(text, v[x]); }
	text += '\n';
}
#endif
