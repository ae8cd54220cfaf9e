/* phase_model_check.cpp -- `yak-amd bubbles -r -p` above the observation records (yak_amd/phase/phase_step.h, phase_text.h) as a sequential program
 * of its own, for the host compiler and its sanitizers: phase_model_check <model file> text|table|damage-bubble|damage-order|damage-sup
 * [grow|tight] [fwd|rev] reads the file tests/phase_util.py model_file() writes -- 64-bit words: k, min_cnt, min_sup, min_link, edges, stats_only, the numbers of
 * bubbles, of support entries and of chunks; the bubble records (ten words each); the support (four words each); then per chunk the numbers of its
 * sequences, their bases, its paths, its steps and its observation records, and the records (16 bytes each) -- and does what the kernels of
 * yak_amd/phase/phase.hip do, launch by launch and thread by thread, with the very functions they call: the full records counted, ranked and
 * written as entries; the votes into the pair table, which grows from 16 slots as the library's does (`grow`) or stands from the start at the
 * capacity of all its keys (`tight`); the edges out of the slots; the rounds of Boruvka's as the kernels stage them -- the best w, the best key,
 * the hook, the doubling, the rewrite --; the names, the nodes, the classification, the blocks; and the text (`table`: `G n_grow capacity n_pair n_round` instead).  `rev` runs the threads of every
 * launch last to first: nothing may depend on their order.  The damage modes spoil the input first: a record's bubble out of range, records out of
 * seq order, a support list one entry short.  Exit 1 after a message when the file cannot be read or does not fit: never a read outside. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../yak_amd/phase/phase_text.h"

static int fail(const char *what) { fprintf(stderr, "phase: %s\n", what); return 1; }
static bool words(FILE *fp, uint64_t *w, size_t n) { return fread(w, 8, n, fp) == n; }

struct Chunk { uint64_t head[4]; std::vector<al_obs_t> obs; };

struct Cas { uint64_t operator()(uint64_t *p, uint64_t expected, uint64_t desired) const { const uint64_t old = *p; if (old == expected) *p = desired; return old; } };
struct Add { void operator()(uint64_t *p, uint64_t v) const { *p += v; } };
struct Max { void operator()(uint32_t *p, uint32_t v) const { if (v > *p) *p = v; } };
struct Min { void operator()(uint64_t *p, uint64_t v) const { if (v < *p) *p = v; } };

int main(int argc, char **argv)
{
	if (argc < 3 || argc > 5) { fprintf(stderr, "usage: phase_model_check <model file> text|table|damage-bubble|damage-order|damage-sup [grow|tight] [fwd|rev]\n"); return 2; }
	const char *mode = argv[2];
	const bool tight = argc >= 4 && strcmp(argv[3], "tight") == 0, rev = argc == 5 && strcmp(argv[4], "rev") == 0;
	if ((argc >= 4 && !tight && strcmp(argv[3], "grow") != 0) || (argc == 5 && !rev && strcmp(argv[4], "fwd") != 0)) return fail("the table is grow or tight, the order fwd or rev");
	FILE *fp = fopen(argv[1], "rb");
	uint64_t head[9];
	if (!fp || !words(fp, head, 9)) return fail("cannot read the file");
	const int k = (int)head[0], min_cnt = (int)head[1], min_sup = (int)head[2], min_link = (int)head[3];
	const bool edges = head[4] != 0, stats_only = head[5] != 0;
	const uint64_t n_b = head[6], n_chunk = head[8];
	uint64_t n_sup = head[7];
	if (n_b >= (uint64_t)1 << 31 || n_sup >= (uint64_t)1 << 31 || n_chunk > 1 << 20) return fail("the numbers of the file do not fit");
	std::vector<bb_rec_t> rec((size_t)n_b);
	std::vector<al_sup_t> sup((size_t)n_sup);
	if (n_b && fread(rec.data(), sizeof(bb_rec_t), (size_t)n_b, fp) != n_b) return fail("the file is short");
	if (n_sup && fread(sup.data(), sizeof(al_sup_t), (size_t)n_sup, fp) != n_sup) return fail("the file is short");
	std::vector<Chunk> chunks((size_t)n_chunk);
	for (Chunk &c : chunks) {
		uint64_t h[5];
		if (!words(fp, h, 5) || h[4] > 1 << 24) return fail("the file is short");
		memcpy(c.head, h, sizeof c.head);
		c.obs.resize((size_t)h[4]);
		if (h[4] && fread(c.obs.data(), sizeof(al_obs_t), (size_t)h[4], fp) != h[4]) return fail("the file is short");
	}
	fclose(fp);

	/* the damage */
	Chunk *two = 0;
	for (Chunk &c : chunks) if (!two && c.obs.size() >= 2) two = &c;
	const bool damage = strncmp(mode, "damage-", 7) == 0;
	if (damage) {
		if (!two) return fail("nothing to damage");
		if (strcmp(mode, "damage-bubble") == 0) two->obs[two->obs.size() / 2].bubble = (uint32_t)n_b;
		else if (strcmp(mode, "damage-order") == 0) { two->obs[0].seq = two->obs.back().seq + 1; }
		else if (strcmp(mode, "damage-sup") == 0) { if (!n_sup) return fail("nothing to damage"); sup.pop_back(); --n_sup; }
		else return fail("the mode is none of text, table, damage-bubble, damage-order, damage-sup");
	} else if (strcmp(mode, "text") != 0 && strcmp(mode, "table") != 0) return fail("the mode is none of text, table, damage-bubble, damage-order, damage-sup");
	if (min_sup < 1 || min_link < 1) return fail("a minimum below 1");
	const auto at_of = [rev](uint64_t t, uint64_t n) { return rev ? n - 1 - t : t; };

	/* the feeds: k_ph_full<COUNT>, the exclusive sum, k_ph_full<EMIT>, k_ph_rehash, k_ph_vote */
	uint64_t cap = PH_CAP0, n_pair = 0, n_grow = 0;
	if (tight) {                                                   /* the capacity of all the keys: they are counted by a table that may grow */
		std::vector<uint64_t> keys;
		for (const Chunk &c : chunks) {
			uint64_t prev = 0, key, inc;
			bool have = false;
			for (const al_obs_t &o : c.obs) {
				if (!(o.flags & AL_FULL)) continue;
				const uint64_t e = ph_entry(&o);
				if (have && ph_vote(prev, e, &key, &inc)) { bool seen = false; for (uint64_t x : keys) seen |= x == key; if (!seen) keys.push_back(key); }
				prev = e; have = true;
			}
		}
		cap = ph_capacity(PH_CAP0, keys.size());
	}
	std::vector<ph_slot_t> slots((size_t)cap, ph_slot_t{ PH_EMPTY, 0 });
	pht_total_t tot = { 0, 0, 0, 0, 0, 0, 0 };
	for (const Chunk &c : chunks) {
		tot.n_seq += c.head[0]; tot.len += c.head[1]; tot.path += c.head[2]; tot.step += c.head[3]; tot.obs += c.obs.size();
		const uint64_t n = c.obs.size();
		if (n == 0) continue;
		std::vector<uint64_t> cnt((size_t)n);
		uint64_t bad = 0, n_full = 0;
		for (uint64_t t = 0; t < n; ++t) cnt[(size_t)at_of(t, n)] = (uint64_t)ph_full(c.obs.data(), at_of(t, n), n_b, &bad);
		if (bad) return fail("records do not fit: a bubble is none of the bubbles, or a sequence comes behind a later one");
		for (uint64_t t = 0; t < n; ++t) { const uint64_t v = cnt[(size_t)t]; cnt[(size_t)t] = n_full; n_full += v; }
		tot.full += n_full;
		if (n_full < 2) continue;
		std::vector<uint64_t> ent((size_t)n_full, PH_EMPTY);
		for (uint64_t t = 0; t < n; ++t) {
			const uint64_t x = at_of(t, n);
			if (!ph_full(c.obs.data(), x, n_b, &bad)) continue;
			if (cnt[(size_t)x] >= n_full) return fail("a rank outside the list");
			ent[(size_t)cnt[(size_t)x]] = ph_entry(&c.obs[(size_t)x]);
		}
		for (uint64_t e : ent) if (e == PH_EMPTY) return fail("an entry was not written");
		if (!tight && 2 * (n_pair + n_full) > cap) {
			const uint64_t next_cap = ph_capacity(cap, n_pair + n_full);
			std::vector<ph_slot_t> next((size_t)next_cap, ph_slot_t{ PH_EMPTY, 0 });
			for (uint64_t s = 0; s < cap; ++s) if (ph_move(slots.data(), at_of(s, cap), next.data(), next_cap, Cas()) != 0) return fail("a pair found no slot in the larger table");
			slots.swap(next); cap = next_cap; ++n_grow;
		}
		for (uint64_t t = 1; t < n_full; ++t) {
			const uint64_t x = rev ? n_full - t : t;
			uint64_t key, inc;
			if (!ph_vote(ent[(size_t)x - 1], ent[(size_t)x], &key, &inc)) continue;
			const int r = ph_add(slots.data(), cap, key, inc, Cas(), Add());
			if (r < 0) return fail("a vote found no slot");
			++tot.vote; n_pair += (uint64_t)r;
		}
	}
	if (n_sup != n_b) return fail("the support is not that of the bubbles");
	if (tight && cap != ph_capacity(PH_CAP0, n_pair)) return fail("the table does not stand at the capacity of its keys");

	/* the solve: k_ph_edges<COUNT>, the exclusive sum, k_ph_edges<EMIT>, k_ph_init */
	std::vector<uint64_t> cnt((size_t)cap);
	std::vector<ph_edge_t> edge;
	std::vector<ph_pair_t> pair;
	uint64_t n_edge = 0;
	for (uint64_t s = 0; s < cap; ++s) { ph_edge_t e; cnt[(size_t)s] = (uint64_t)ph_edge(slots.data(), s, sup.data(), (uint64_t)min_sup, (uint64_t)min_link, &e); }
	for (uint64_t s = 0; s < cap; ++s) { const uint64_t v = cnt[(size_t)s]; cnt[(size_t)s] = n_edge; n_edge += v; }
	edge.resize((size_t)n_edge);
	for (uint64_t s = 0; s < cap; ++s) { ph_edge_t e; ph_pair_t p; if (ph_edge(slots.data(), s, sup.data(), (uint64_t)min_sup, (uint64_t)min_link, &e)) edge[(size_t)cnt[(size_t)s]] = e; if (ph_pair(slots.data(), s, &p)) pair.push_back(p); }
	if (pair.size() != n_pair) return fail("the table does not hold the pairs that were counted");
	std::vector<uint32_t> comp((size_t)n_b), best_w((size_t)n_b, 0), name((size_t)n_b, PH_NONE);
	std::vector<uint8_t> par((size_t)n_b, 0);
	std::vector<uint64_t> up((size_t)n_b), best_k((size_t)n_b, PH_EMPTY);
	std::vector<ph_block_t> tal((size_t)n_b, ph_block_t{ 0, 0, 0, 0, 0, 0 });
	for (uint64_t b = 0; b < n_b; ++b) { comp[(size_t)b] = (uint32_t)b; up[(size_t)b] = b << 1; }
	uint64_t n_round = 0, n_forest = 0;
	/* the rounds: k_ph_best_w, k_ph_best_key, k_ph_hook, k_ph_flatten, k_ph_rewrite */
	for (; n_edge;) {
		uint64_t cross = 0;
		for (uint64_t t = 0; t < n_edge; ++t) cross += (uint64_t)ph_best_w(&edge[(size_t)at_of(t, n_edge)], comp.data(), best_w.data(), Max());
		++n_round;
		if (!cross) break;
		if (n_round > 40) return fail("edges still cross after 40 rounds");
		for (uint64_t t = 0; t < n_edge; ++t) ph_best_key(&edge[(size_t)at_of(t, n_edge)], comp.data(), best_w.data(), best_k.data(), Min());
		for (uint64_t t = 0; t < n_edge; ++t) n_forest += (uint64_t)ph_hook(&edge[(size_t)at_of(t, n_edge)], comp.data(), par.data(), best_w.data(), best_k.data(), up.data());
		for (uint64_t b = 0; b < n_b; ++b) { const uint64_t r = at_of(b, n_b); if (comp[(size_t)r] == (uint32_t)r) ph_flatten(up.data(), (uint32_t)r); }
		for (uint64_t b = 0; b < n_b; ++b) { ph_rewrite((uint32_t)b, comp.data(), par.data(), up.data()); best_w[(size_t)b] = 0; best_k[(size_t)b] = PH_EMPTY; }
	}
	/* k_ph_name, k_ph_nodes, k_ph_classify, k_ph_blocks */
	std::vector<ph_node_t> node((size_t)n_b);
	uint64_t n_het = 0, n_single = 0;
	for (uint64_t b = 0; b < n_b; ++b) { const uint64_t x = at_of(b, n_b); if (al_call(&sup[(size_t)x], (uint64_t)min_sup) == 0 && (uint32_t)x < name[comp[(size_t)x]]) name[comp[(size_t)x]] = (uint32_t)x; }
	for (uint64_t b = 0; b < n_b; ++b) {
		const int het = al_call(&sup[(size_t)b], (uint64_t)min_sup) == 0;
		const uint32_t nm = het ? name[comp[(size_t)b]] : 0;
		node[(size_t)b] = ph_node((uint32_t)b, het, nm, par.data());
		if (het) { ++tal[nm].n_bubble; ++n_het; }
	}
	for (ph_edge_t &e : edge) {
		const int disc = ph_discordant(&e, node.data());
		ph_block_t &b = tal[node[e.i].block];
		if (disc) { e.flags |= PH_DISC; ++b.n_disc; b.w_disc += e.w; }
		++b.n_edge; b.w_sum += e.w;
	}
	std::vector<ph_block_t> blk;
	for (uint64_t b = 0; b < n_b; ++b) {
		if (tal[(size_t)b].n_bubble == 1) ++n_single;
		if (tal[(size_t)b].n_bubble >= 2) { blk.push_back(tal[(size_t)b]); blk.back().block = (uint32_t)b; }
	}
	if (n_forest + blk.size() + n_single != n_het) return fail("the forest, the blocks and the bubbles alone do not add up to the het bubbles");
	if (damage) return fail("the damage went unseen");

	std::string text;
	uint64_t n_call[4] = { 0, 0, 0, 0 }, n_disc = 0, max_block = 0;
	const pht_solve_t sv = { n_pair, n_het, n_edge, n_forest, blk.size(), n_single };
	pht_head(text, k, min_cnt, min_sup, min_link);
	alt_alleles(text, rec.data(), sup.data(), n_b, (uint64_t)min_sup, !stats_only, n_call);
	if (!stats_only) pht_nodes(text, node.data(), n_b);
	pht_blocks(text, blk.data(), blk.size(), !stats_only, &n_disc, &max_block);
	if (!stats_only && edges && !pht_edges(text, edge, pair)) return fail("an edge without its pair");
	pht_tail(text, tot, n_b, sv, n_disc, max_block);
	if (strcmp(mode, "table") == 0) { printf("G %llu %llu %llu %llu\n", (unsigned long long)n_grow, (unsigned long long)cap, (unsigned long long)n_pair, (unsigned long long)n_round); return 0; }
	fwrite(text.data(), 1, text.size(), stdout);
	return 0;
}
