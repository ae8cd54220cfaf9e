/* gfa_model_check.cpp -- the links between unitigs of `yak-amd unitigs -G` (yak_amd/gfa/gfa_step.h, gfa_text.h) as a sequential program of its own,
 * for the host compiler and its sanitizers: gfa_model_check <file> gfa|stats|links reads the file tests/gfa_util.py model_file() writes (64-bit
 * words: k, min_cnt, the capacity of the end table or 0, the numbers of unitigs and bases, the graph's tallies, the U line's numbers, the
 * descriptors; then the bases) and does what the kernels of yak_amd/gfa/gfa.hip do, end by end, with the very functions they call: the claims of
 * the end nodes in the end table, the count of every oriented end, the exclusive scan, the emit at the offsets.  It prints the GFA, the -s text, or
 * the links as `from to` with a last line `T table_slots keys max_probe`.  Exit 1 after a message when the file cannot be read, the capacity is
 * below the number of keys, a claim meets no free slot or the descriptors do not fit the bases. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../yak_amd/gfa/gfa_text.h"

static int fail(const char *what) { fprintf(stderr, "gfa: %s\n", what); return 1; }

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: gfa_model_check <file> gfa|stats|links\n"); return 2; }
	FILE *fp = fopen(argv[1], "rb");
	uint64_t head[39];
	if (!fp || fread(head, 8, 39, fp) != 39) return fail("cannot read the file");
	const int k = (int)head[0];
	const uint64_t n_u = head[3], n_bases = head[4];
	gft_tallies_t t;
	t.k = k; t.min_cnt = (int)head[1];
	t.n_key = head[5]; t.n_node = head[6]; t.n_arc = head[7]; t.n_linked_side = head[8];
	for (int i = 0; i < 25; ++i) t.deg[i / 5][i % 5] = head[9 + i];
	t.n_open = head[34]; t.n_cycle = head[35]; t.sum_len = head[36]; t.max_len = head[37]; t.n50 = head[38];
	if (k < 3 || k > 31 || !(k & 1)) return fail("k must be odd and in [3, 31]");
	std::vector<gf_desc_t> desc((size_t)n_u);
	std::vector<char> bases((size_t)n_bases);                          /* exactly n_bases: a read past them is the sanitizer's */
	if (n_u && fread(desc.data(), sizeof(gf_desc_t), (size_t)n_u, fp) != n_u) return fail("the file is short");
	if (n_bases && fread(bases.data(), 1, (size_t)n_bases, fp) != n_bases) return fail("the file is short");
	fclose(fp);

	/* the end table */
	uint64_t n_key = 0;
	for (const gf_desc_t &u : desc) if (!(u.first & 1)) n_key += u.n_node > 1 ? 2 : 1;
	uint64_t cap = gf_capacity(n_key);
	if (head[2]) {
		if (head[2] < n_key) return fail("the capacity is below the number of keys");
		for (cap = 1; cap < head[2]; cap <<= 1) {}
	}
	std::vector<gf_slot_t> slots((size_t)cap, gf_slot_t{ GF_EMPTY, GF_EMPTY });
	std::vector<uint64_t> endw((size_t)(2 * n_u));
	uint64_t max_probe = 0, bad = 0;
	const auto cas = [](uint64_t *p, uint64_t expected, uint64_t desired) { const uint64_t old = *p; if (old == expected) *p = desired; return old; };
	for (uint64_t j = 0; j < n_u; ++j) {
		gf_ends_t e;
		if (gf_ends(&desc[j], j, bases.data(), n_bases, k, &e) < 0) return fail("a descriptor does not fit the bases");
		for (int i = 0; i < e.n_key; ++i) {
			uint64_t pr = 0;
			const int r = gf_claim(slots.data(), cap, e.key[i], e.val[i], cas, &pr);
			if (r == -1) return fail("an end node met no free slot");
			if (r == -2) return fail("an end node stands in two unitigs");
			if (pr > max_probe) max_probe = pr;
		}
		endw[2 * j] = e.w[0]; endw[2 * j + 1] = e.w[1];
	}

	/* count, scan, emit */
	const uint64_t n_end = 2 * n_u;
	std::vector<uint64_t> cnt((size_t)n_end + 1, 0);
	uint64_t end_deg[5] = { 0, 0, 0, 0, 0 }, to[4];
	for (uint64_t e = 0; e < n_end; ++e) {
		int open;
		const unsigned n = (unsigned)__builtin_popcount(gf_links(slots.data(), cap, endw[e], e, k, n_u, to, &open, &max_probe, &bad));
		cnt[e] = n;
		if (open) ++end_deg[n];
	}
	uint64_t n_link = 0;
	for (uint64_t e = 0; e <= n_end; ++e) { const uint64_t v = cnt[e]; cnt[e] = n_link; n_link += v; }
	std::vector<gf_link_t> links((size_t)n_link, gf_link_t{ ~(uint64_t)0, ~(uint64_t)0 });
	for (uint64_t e = 0; e < n_end; ++e) {
		int open;
		const unsigned mask = gf_links(slots.data(), cap, endw[e], e, k, n_u, to, &open, &max_probe, &bad);
		uint64_t at = cnt[e];
		if (at + (unsigned)__builtin_popcount(mask) != cnt[e + 1]) return fail("the emit does not repeat the count");
		for (int b = 0; b < 4; ++b) if (mask >> b & 1u) links[at++] = gf_link_t{ e, to[b] };
	}
	if (bad) return fail("a value of the end table fits no unitig");

	if (strcmp(argv[2], "stats") == 0) fputs(gft_stats(t, n_link, end_deg).c_str(), stdout);
	else if (strcmp(argv[2], "links") == 0) {
		for (const gf_link_t &l : links) printf("%llu %llu\n", (unsigned long long)l.from, (unsigned long long)l.to);
		printf("T %llu %llu %llu\n", (unsigned long long)cap, (unsigned long long)n_key, (unsigned long long)max_probe);
	} else if (!gft_gfa(desc.data(), n_u, bases.data(), n_bases, links.data(), n_link, k, [](const std::string &s) { return fwrite(s.data(), 1, s.size(), stdout) == s.size(); }))
		return fail("the text cannot be written");
	return fflush(stdout) == 0 ? 0 : 1;
}
