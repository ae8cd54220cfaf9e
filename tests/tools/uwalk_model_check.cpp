/* uwalk_model_check.cpp -- the device walk of `yak-amd unitigs -g` (yak_amd/walk/uwalk_step.h, uwalk_host.h) as a sequential program of its own, for
 * the host compiler and its sanitizers: uwalk_model_check <records> fasta|stats|map reads the file tests/graph_util.py record_file() writes (k,
 * min_cnt, the number of records, the 32-byte records) and does what the kernels of yak_amd/walk/walk.hip do, state by state, with the very
 * functions they call: the pairs from the records, doubling rounds between two buffers until a round finishes no state, the decision per node, the
 * two scans, the map entries, descriptors and bases of the open unitigs, and the cycles from their compacted records alone.  It prints the command's
 * FASTA, the U line of its -s form, or the map as `unitig at` per stored key with the descriptors as `D off n_node kc first` behind it.  Exit 1
 * after a message when the file cannot be read or the links are broken. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <utility>
#include "../../yak_amd/walk/uwalk_host.h"

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: uwalk_model_check <records> fasta|stats|map\n"); return 2; }
	FILE *fp = fopen(argv[1], "rb");
	uint32_t head[2];
	uint64_t n = 0;
	if (!fp || fread(head, 4, 2, fp) != 2 || fread(&n, 8, 1, fp) != 1) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
	std::vector<uw_node_t> rec((size_t)n);
	if (n && fread(rec.data(), sizeof(uw_node_t), (size_t)n, fp) != n) { fprintf(stderr, "%s is short\n", argv[1]); return 1; }
	fclose(fp);
	const int k = (int)head[0];
	const uint32_t min_cnt = head[1];

	/* the ranking: never in place */
	std::vector<uw_pair_t> a((size_t)(2 * n)), b((size_t)(2 * n));
	for (uint64_t v = 0; v < n; ++v) for (int d = 0; d < 2; ++d) a[uw_state(v, d)] = uw_init(&rec[v], v, d, min_cnt);
	uint64_t rounds = 0;
	for (;;) {
		uint64_t finished = 0;
		for (uint64_t s = 0; s < 2 * n; ++s) {
			uw_pair_t p = a[s];
			const uint64_t t = uw_target(p, 2 * n);
			if (t != UW_NONE) { int f; p = uw_jump(p, a[t], &f); finished += (uint64_t)f; }
			b[s] = p;
		}
		++rounds;
		std::swap(a, b);
		if (finished == 0) break;
		if (rounds > 64) { fprintf(stderr, "walk: the ranking did not end\n"); return 1; }
	}

	/* the decision, the scans, the open unitigs */
	std::vector<uw_place_t> dec((size_t)n);
	std::vector<int> kind((size_t)n, -2);                             /* 1 open, 0 cycle, -2 no node */
	std::vector<uint64_t> jr((size_t)n + 1, 0), off((size_t)n + 1, 0), idx;
	for (uint64_t v = 0; v < n; ++v) {
		if (uw_dead(a[2 * v])) continue;
		kind[v] = uw_decide(v, a[2 * v], a[2 * v + 1], &dec[v]);
		if (kind[v] < 0) { fprintf(stderr, "walk: the links from key %llu do not lead to an end node each way\n", (unsigned long long)v); return 1; }
		if (kind[v] == 0) idx.push_back(v);
	}
	for (uint64_t v = 0; v < n; ++v) {
		const bool start = kind[v] == 1 && dec[v].start == v;
		jr[v + 1] = jr[v] + (start ? 1 : 0);
		off[v + 1] = off[v] + (start ? dec[v].n_node + (uint64_t)k - 1 : 0);
	}
	const uint64_t n_open = jr[n], open_len = off[n];
	std::vector<uw_map_t> map((size_t)n, uw_map_t{ UW_NONE, 0 });
	std::vector<uw_desc_t> desc((size_t)n_open, uw_desc_t{ 0, 0, 0, 0 });
	std::string bases((size_t)open_len, '?');
	for (uint64_t v = 0; v < n; ++v) {
		if (kind[v] != 1) continue;
		const uint64_t e = dec[v].start, j = jr[e], o = off[e], p = dec[v].at >> 1;
		const int d = (int)(dec[v].at & 1);
		if (e >= n || j >= n_open || o + (uint64_t)k - 1 + p >= open_len) { fprintf(stderr, "walk: key %llu has no place in its unitig\n", (unsigned long long)v); return 1; }
		map[v] = uw_map_t{ j, dec[v].at };
		desc[j].kc += rec[v].count;
		if (p == 0) {
			desc[j].off = o; desc[j].n_node = a[2 * v].dist + a[2 * v + 1].dist + 1; desc[j].first = v << 1;
			for (int i = 0; i < k; ++i) bases[o + i] = uw_base_at(rec[v].x, d, k, i);
		} else bases[o + (uint64_t)k - 1 + p] = uw_last_base(rec[v].x, d, k);
	}

	/* the cycles: their records alone, compacted in listing order */
	std::vector<uw_node_t> crec;
	for (uint64_t v : idx) crec.push_back(rec[v]);
	uwh_cycles_t cy;
	std::string err;
	if (uwh_cycles(crec.data(), idx.data(), idx.size(), k, n_open, open_len, &cy, &err) != 0) { fprintf(stderr, "walk: %s\n", err.c_str()); return 1; }
	for (size_t i = 0; i < idx.size(); ++i) map[idx[i]] = cy.map[i];
	desc.insert(desc.end(), cy.desc.begin(), cy.desc.end());
	bases += cy.bases;

	uint64_t sum_len, max_len, n50;
	uwh_lengths(desc.data(), desc.size(), k, &sum_len, &max_len, &n50);
	if (sum_len != bases.size()) { fprintf(stderr, "walk: the descriptors hold %llu bases, the array %llu\n", (unsigned long long)sum_len, (unsigned long long)bases.size()); return 1; }
	if (strcmp(argv[2], "stats") == 0) fputs(uwh_u_line(n_open, cy.desc.size(), sum_len, max_len, n50).c_str(), stdout);
	else if (strcmp(argv[2], "map") == 0) {
		for (const uw_map_t &m : map) printf("%llu %llu\n", (unsigned long long)m.unitig, (unsigned long long)m.at);
		for (const uw_desc_t &u : desc) printf("D %llu %llu %llu %llu\n", (unsigned long long)u.off, (unsigned long long)u.n_node, (unsigned long long)u.kc, (unsigned long long)u.first);
		printf("R %llu %llu\n", (unsigned long long)rounds, (unsigned long long)idx.size());
	} else if (!uwh_fasta(desc.data(), desc.size(), bases.data(), k, [](const std::string &t) { return fwrite(t.data(), 1, t.size(), stdout) == t.size(); })) return 1;
	return fflush(stdout) == 0 ? 0 : 1;
}
