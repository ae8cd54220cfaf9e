/* clean_model_check.cpp -- one round of `yak-amd clean` (yak_amd/clean/clean_step.h, clean_text.h) as a sequential program of its own, for the host
 * compiler and its sanitizers: clean_model_check <file> report|records|image reads the file tests/clean_util.py model_file() writes (64-bit words:
 * k, min_cnt, tip_nodes, pop_pct, n_key, the numbers of unitigs, bases, links and bubbles; the descriptors, the links, the bubble records; then the
 * bases) and does what the kernels of yak_amd/clean/clean.hip do, link by link, unitig by unitig and record by record, with the very functions they
 * call: the first link of every end, the clip rule, the pop rule, the count, the exclusive scan, the emit at the ranks, the image byte by byte.  It
 * prints the report of a first round (the first line, the R line, the T and P lines), the records as their six words with a last line `S n_tip
 * tip_nodes n_tip_kept n_pop pop_nodes n_pop_kept n_rec img_bytes`, or the image.  Exit 1 after a message when the file cannot be read, the list
 * of links or a bubble record does not fit, or a removed unitig does not lie inside the bases. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../yak_amd/clean/clean_text.h"

static int fail(const char *what) { fprintf(stderr, "clean: %s\n", what); return 1; }

int main(int argc, char **argv)
{
	if (argc != 3) { fprintf(stderr, "usage: clean_model_check <file> report|records|image\n"); return 2; }
	FILE *fp = fopen(argv[1], "rb");
	uint64_t head[9];
	if (!fp || fread(head, 8, 9, fp) != 9) return fail("cannot read the file");
	const int k = (int)head[0], min_cnt = (int)head[1];
	const uint64_t tip_nodes = head[2], pop_pct = head[3], n_key = head[4], n_u = head[5], n_bases = head[6], n_link = head[7], n_bubble = head[8], n_end = 2 * n_u;
	if (k < 3 || k > 31 || !(k & 1)) return fail("k must be odd and in [3, 31]");
	if (tip_nodes > (1u << 20) || pop_pct > 100) return fail("an option is out of range");
	std::vector<bb_desc_t> desc((size_t)n_u);
	std::vector<bb_link_t> links((size_t)n_link);                       /* exactly n_link, n_bubble and n_bases: a read past them is the sanitizer's */
	std::vector<bb_rec_t> bub((size_t)n_bubble);
	std::vector<char> bases((size_t)n_bases);
	if (n_u && fread(desc.data(), sizeof(bb_desc_t), (size_t)n_u, fp) != n_u) return fail("the file is short");
	if (n_link && fread(links.data(), sizeof(bb_link_t), (size_t)n_link, fp) != n_link) return fail("the file is short");
	if (n_bubble && fread(bub.data(), sizeof(bb_rec_t), (size_t)n_bubble, fp) != n_bubble) return fail("the file is short");
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

	/* the tips, then the pops */
	uint64_t st[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, bad = 0;
	std::vector<uint64_t> why((size_t)n_u, 0), other((size_t)n_u, BB_NONE);
	for (uint64_t j = 0; j < n_u; ++j) {
		int cand;
		bb_desc_t u;
		why[(size_t)j] = (uint64_t)cl_tip(desc.data(), n_u, runs.data(), links.data(), n_link, j, tip_nodes, &other[(size_t)j], &cand, &u, &bad);
		if (why[(size_t)j] == CL_TIP) { ++st[0]; st[1] += u.n_node; }
		else if (cand) ++st[2];
	}
	if (bad) return fail("the links do not fit the unitigs");
	for (uint64_t i = 0; i < n_bubble; ++i) {
		uint64_t lo, hi, n_lo, kc_lo;
		const int p = cl_pop(&bub[(size_t)i], desc.data(), n_u, pop_pct, &lo, &hi, &n_lo, &kc_lo);
		if (p < 0) return fail("a bubble record does not fit: an arm outside the unitigs, or one with other nodes or counts");
		if (!p) { ++st[5]; continue; }
		if (why[(size_t)(lo >> 1)] != CL_KEEP) return fail("an arm that is a tip, or an arm of two bubbles");
		why[(size_t)(lo >> 1)] = CL_POP; other[(size_t)(lo >> 1)] = hi;
		++st[3]; st[4] += n_lo;
	}

	/* count, scan, emit */
	std::vector<uint64_t> rank((size_t)n_u + 1, 0), off((size_t)n_u + 1, 0);
	uint64_t n_rec = 0, img_bytes = 0;
	for (uint64_t j = 0; j < n_u; ++j) {
		rank[(size_t)j] = n_rec; off[(size_t)j] = img_bytes;
		if (why[(size_t)j] != CL_KEEP) { ++n_rec; img_bytes += desc[(size_t)j].n_node + (uint64_t)k; }
	}
	cl_rec_t none;
	memset(&none, 0xff, sizeof none);
	std::vector<cl_rec_t> rec((size_t)n_rec, none);
	for (uint64_t j = 0; j < n_u; ++j) {
		if (why[(size_t)j] == CL_KEEP) continue;
		if (rank[(size_t)j] >= n_rec) return fail("the emit does not repeat the count");
		const bb_desc_t u = desc[(size_t)j];
		rec[(size_t)rank[(size_t)j]] = cl_rec_t{ j, why[(size_t)j], u.n_node, u.kc, other[(size_t)j], off[(size_t)j] };
	}
	st[6] = n_rec; st[7] = img_bytes;
	if (n_rec != st[0] + st[3] || img_bytes != st[1] + st[4] + n_rec * (uint64_t)k) return fail("the records do not add up to the tallies");

	/* the image: exactly img_bytes, byte by byte as the lanes of a wave copy it */
	std::vector<char> img((size_t)img_bytes, '?');
	for (const cl_rec_t &r : rec) {
		uint64_t src = 0, len = 0;
		if (cl_span(&r, desc.data(), n_u, n_bases, img_bytes, k, &src, &len) != 0) return fail("a removed unitig does not lie inside the bases, or its place not inside the image");
		for (uint64_t p = 0; p < len; ++p) img[(size_t)(r.off + p)] = bases[(size_t)(src + p)];
		img[(size_t)(r.off + len)] = '\n';
	}

	typedef unsigned long long ull;
	const auto put = [](const std::string &s) { return fwrite(s.data(), 1, s.size(), stdout) == s.size(); };
	if (strcmp(argv[2], "records") == 0) {
		for (const cl_rec_t &r : rec) printf("%llu %llu %llu %llu %llu %llu\n", (ull)r.unitig, (ull)r.why, (ull)r.n_node, (ull)r.kc, (ull)r.other, (ull)r.off);
		printf("S %llu %llu %llu %llu %llu %llu %llu %llu\n", (ull)st[0], (ull)st[1], (ull)st[2], (ull)st[3], (ull)st[4], (ull)st[5], (ull)st[6], (ull)st[7]);
	} else if (strcmp(argv[2], "image") == 0) {
		if (img_bytes && fwrite(img.data(), 1, (size_t)img_bytes, stdout) != img_bytes) return fail("the image cannot be written");
	} else {
		const clt_round_t rnd = { n_key, n_u, n_link, n_bubble, st[0], st[1], st[3], st[4], st[1] + st[4] };
		if (!put(clt_head(k, min_cnt, (int)tip_nodes, (int)pop_pct) + clt_round(1, rnd)) || !clt_records(1, rec.data(), n_rec, put)) return fail("the text cannot be written");
	}
	return fflush(stdout) == 0 ? 0 : 1;
}
