/* allele_model_check.cpp -- `yak-amd bubbles -r` above the paths (yak_amd/allele/allele_step.h, allele_text.h) as a sequential program of its own, for
 * the host compiler and its sanitizers: allele_model_check <model file> text|records|damage-arm|damage-dup|damage-step|damage-range|damage-last
 * [threads] reads the file tests/allele_util.py model_file() writes -- 64-bit words: k, min_cnt, min_sup, min_frag, fragments, stats_only, the
 * numbers of unitigs, bubbles and chunks; the bubble records (ten words each); then per chunk the numbers of its sequences, their bases, its paths
 * and its steps, the path records (32 bytes each), the steps, the bytes of the names and the names, each followed by a newline, padded to eight
 * bytes -- and does what the kernels of yak_amd/allele/allele.hip do, workgroup by workgroup of `threads` [256] and thread by thread, with the very
 * functions they call: the claims of the arms, the paths of a workgroup's first and last step, the decision per step, the exclusive sum, the record
 * at its rank and the support.  It prints the text of the command, or the records (`O seq bubble flags path` per observation, `N n_obs n_full` per
 * chunk, `S full1 full2 part1 part2` per bubble last).  The damage modes spoil the input first -- an arm outside the unitigs, a unitig claimed by
 * two arms, a step outside the unitigs, a path one step too long (the first: the next does not follow it; the last: it leaves the steps).  Exit 1
 * after a message when the file cannot be read or does not fit: never a read outside. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../yak_amd/allele/allele_text.h"

static int fail(const char *what) { fprintf(stderr, "allele: %s\n", what); return 1; }

struct Chunk {
	uint64_t n_seq, len;
	std::vector<al_path_t> paths;
	std::vector<uint64_t> steps;
	std::vector<std::string> name;
};

static bool words(FILE *fp, uint64_t *w, size_t n) { return fread(w, 8, n, fp) == n; }

int main(int argc, char **argv)
{
	if (argc != 3 && argc != 4) { fprintf(stderr, "usage: allele_model_check <model file> text|records|damage-arm|damage-dup|damage-step|damage-range|damage-last [threads]\n"); return 2; }
	const char *mode = argv[2];
	const uint64_t threads = argc == 4 ? strtoull(argv[3], 0, 10) : 256;
	if (threads < 2) return fail("a workgroup has two threads or more");
	FILE *fp = fopen(argv[1], "rb");
	uint64_t head[9];
	if (!fp || !words(fp, head, 9)) return fail("cannot read the file");
	const int k = (int)head[0], min_cnt = (int)head[1], min_sup = (int)head[2];
	const uint64_t min_frag = head[3], n_u = head[6], n_b = head[7], n_chunk = head[8];
	const bool fragments = head[4] != 0, stats_only = head[5] != 0;
	if (n_u >= (uint64_t)1 << 31 || n_b >= (uint64_t)1 << 31 || n_chunk > 1 << 20 || min_sup < 1 || min_frag < 1) return fail("the numbers of the file do not fit");
	std::vector<bb_rec_t> rec((size_t)n_b);
	if (n_b && fread(rec.data(), sizeof(bb_rec_t), (size_t)n_b, fp) != n_b) return fail("the file is short");
	std::vector<Chunk> chunks((size_t)n_chunk);
	for (Chunk &c : chunks) {
		uint64_t h[4], nb = 0;
		if (!words(fp, h, 4) || h[0] > 1 << 24 || h[2] > 1 << 24 || h[3] > 1 << 24) return fail("the file is short");
		c.n_seq = h[0]; c.len = h[1];
		c.paths.resize((size_t)h[2]); c.steps.resize((size_t)h[3]);
		if (h[2] && fread(c.paths.data(), sizeof(al_path_t), (size_t)h[2], fp) != h[2]) return fail("the file is short");
		if (h[3] && !words(fp, c.steps.data(), (size_t)h[3])) return fail("the file is short");
		if (!words(fp, &nb, 1) || nb > 1 << 28) return fail("the file is short");
		std::string all((size_t)((nb + 7) / 8 * 8), '\0');
		if (nb && fread(&all[0], 1, all.size(), fp) != all.size()) return fail("the file is short");
		for (size_t at = 0; at < (size_t)nb;) {
			const size_t nl = all.find('\n', at);
			if (nl == std::string::npos || nl >= (size_t)nb) return fail("a name without its end");
			c.name.push_back(all.substr(at, nl - at));
			at = nl + 1;
		}
		if (c.name.size() != c.n_seq) return fail("the names are not those of the sequences");
	}
	fclose(fp);

	/* the damage */
	Chunk *first = 0;
	for (Chunk &c : chunks) if (!first && !c.steps.empty() && !c.paths.empty()) first = &c;
	if (strncmp(mode, "damage-", 7) == 0) {
		if (!n_b || !first) return fail("nothing to damage");
		if (strcmp(mode, "damage-arm") == 0) rec[0].arm[0] = n_u << 1;
		else if (strcmp(mode, "damage-dup") == 0) rec[n_b - 1].arm[1] = rec[0].arm[0] ^ 1;
		else if (strcmp(mode, "damage-step") == 0) first->steps[first->steps.size() / 2] = n_u << 1 | 1;
		else if (strcmp(mode, "damage-range") == 0) ++first->paths[0].n_step;
		else if (strcmp(mode, "damage-last") == 0) ++first->paths.back().n_step;
		else return fail("the mode is none of text, records, damage-arm, damage-dup, damage-step, damage-range, damage-last");
	} else if (strcmp(mode, "text") != 0 && strcmp(mode, "records") != 0) return fail("the mode is none of text, records, damage-arm, damage-dup, damage-step, damage-range, damage-last");
	const bool records = strcmp(mode, "records") == 0;

	/* the arm map: k_al_index */
	std::vector<uint32_t> arm_of((size_t)n_u, AL_NONE);
	const auto cas32 = [](uint32_t *p, uint32_t expected, uint32_t desired) { const uint32_t old = *p; if (old == expected) *p = desired; return old; };
	uint64_t bad_arm = 0, dup_arm = 0;
	for (uint64_t i = 0; i < n_b; ++i)
		for (unsigned a = 0; a < 2; ++a) {
			const int r = al_claim(rec[i].arm[a], i, a, n_u, arm_of.data(), cas32);
			bad_arm += r == AL_BAD_ARM; dup_arm += r == AL_DUP_ARM;
		}
	if (bad_arm) return fail("arms of the bubbles name none of the unitigs of the walk");
	if (dup_arm) return fail("arms of the bubbles name a unitig that another arm holds");

	std::vector<al_sup_t> sup((size_t)n_b, al_sup_t{ { 0, 0 }, { 0, 0 } });
	std::string text, rtext;
	char line[96];
	alt_total_t tot = { 0, 0, 0, 0, 0, 0, 0 };
	alt_head(text, k, min_cnt, min_sup);
	for (Chunk &c : chunks) {
		tot.n_seq += c.n_seq; tot.len += c.len;
		const uint64_t n_path = c.paths.size(), n_step = c.steps.size();
		tot.path += n_path; tot.step += n_step;
		if (n_step == 0) { if (records) rtext += "N 0 0\n"; continue; }
		if (n_path < 1 || n_path > n_step) return fail("steps without a path, or more paths than steps");
		if (n_b == 0) { if (records) rtext += "N 0 0\n"; continue; }        /* no arm: nothing is looked at */
		/* k_al_find<COUNT>, the exclusive sum, k_al_find<EMIT> */
		std::vector<uint64_t> cnt((size_t)n_step, 0);
		std::vector<al_obs_t> obs;
		uint64_t n_obs = 0, n_full = 0, bad = 0;
		for (int pass = 0; pass < 2; ++pass) {
			for (uint64_t t0 = 0; t0 < n_step; t0 += threads) {
				const uint64_t last = t0 + threads - 1 < n_step ? t0 + threads - 1 : n_step - 1;
				const uint64_t lo = al_path_of(c.paths.data(), 0, n_path - 1, t0), hi = al_path_of(c.paths.data(), 0, n_path - 1, last);
				for (uint64_t t = t0; t <= last; ++t) {
					al_obs_t o;
					const int is = al_find(c.paths.data(), lo, hi, c.steps.data(), n_step, t, n_u, arm_of.data(), rec.data(), &o, &bad);
					if (pass == 0) {
						cnt[(size_t)t] = (uint64_t)is;
						n_obs += (uint64_t)is; n_full += is && (o.flags & AL_FULL);
					} else if (is) {
						const uint64_t at = cnt[(size_t)t];
						if (at >= n_obs) { ++bad; continue; }
						obs[(size_t)at] = o;
						uint64_t *w = o.flags & AL_FULL ? sup[o.bubble].full : sup[o.bubble].part;
						++w[o.flags & AL_A];
					}
				}
			}
			if (bad) return fail("steps do not fit: the range of a path does not follow the path before it or leaves the steps, or a step names none of the unitigs");
			if (pass == 0) {
				uint64_t at = 0;
				for (uint64_t t = 0; t < n_step; ++t) { const uint64_t v = cnt[(size_t)t]; cnt[(size_t)t] = at; at += v; }
				obs.assign((size_t)n_obs, al_obs_t{ ~0u, ~0u, ~0u, ~0u });
			}
		}
		for (const al_obs_t &o : obs) if (o.seq == ~0u && o.bubble == ~0u && o.flags == ~0u) return fail("a record was not written");
		tot.obs += n_obs; tot.full += n_full;
		if (records) {
			for (const al_obs_t &o : obs) rtext.append(line, (size_t)snprintf(line, sizeof line, "O %u %u %u %u\n", o.seq, o.bubble, o.flags, o.path));
			rtext.append(line, (size_t)snprintf(line, sizeof line, "N %llu %llu\n", (unsigned long long)n_obs, (unsigned long long)n_full));
		}
		if (fragments && !alt_fragments(text, c.name, obs.data(), n_obs, n_b, min_frag, !stats_only, &tot)) return fail("an observation record does not fit its chunk");
	}
	if (strncmp(mode, "damage-", 7) == 0) return fail("the damage went unseen");
	uint64_t n_call[4] = { 0, 0, 0, 0 };
	alt_alleles(text, rec.data(), sup.data(), n_b, (uint64_t)min_sup, !stats_only, n_call);
	alt_tail(text, tot, n_b, n_call);
	if (records) {
		for (const al_sup_t &s : sup)
			rtext.append(line, (size_t)snprintf(line, sizeof line, "S %llu %llu %llu %llu\n", (unsigned long long)s.full[0], (unsigned long long)s.full[1],
			                                    (unsigned long long)s.part[0], (unsigned long long)s.part[1]));
		text = rtext;
	}
	fwrite(text.data(), 1, text.size(), stdout);
	return 0;
}
