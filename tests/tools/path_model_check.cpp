/* path_model_check.cpp -- `yak-amd paths` (yak_amd/path/path_step.h, path_text.h, yak_amd/layer/seq_reader.h) as a sequential program of its own,
 * for the host compiler and its sanitizers: path_model_check <model file> <sequences> hits|records|gaf|stats|reader|records-kept reads the file
 * tests/path_util.py model_file() writes (64-bit words: k, min_cnt, the capacity of the index or 0, min_len, the numbers of unitigs and of bases, the descriptors; then the bases)
 * and the sequences through SeqReader, and does what the kernels of yak_amd/path/path.hip do, tile by tile and thread by thread, with the very
 * functions they call: the staging, the claims of every node, the hits, the count per tile, the scan of the tile array in slices, the emit on top of
 * it, the tallies lane by lane.  Built with -DPX_THREADS_N=2 its tiles have 8 positions.  It prints the hits one a line, or the records (`P seq qs
 * qe ps step_off n_step`, `S step`, `Y n_kmer n_hit n_path n_step`, a last line `T table_slots keys max_probe`), or one of the two texts, or what
 * the reader gives (`name<tab>sequence` with the quality counted; with it kept, for records-kept, name, comment, sequence and quality, each as
 * its length, a colon and its bytes, and a newline behind the four).  Exit 1 after a message when a file cannot be read, the capacity is below
 * the number of keys, a claim meets no free slot or a key a second time, or the descriptors do not fit the bases. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../yak_amd/path/path_text.h"
#include "../../yak_amd/layer/seq_reader.h"

static int fail(const char *what) { fprintf(stderr, "path: %s\n", what); return 1; }

struct HostLoad16 {
	const unsigned char *g;
	void operator()(int64_t off, unsigned char *dst) const { memcpy(dst, g + off, 16); }
};
/* the window of a tile: from `from` rounded down to 16 up to `to`, 16 bytes at a time; returns the position of win[0] */
static int64_t stage(const std::vector<unsigned char> &img, int64_t n, int64_t from, int64_t to, std::vector<unsigned char> &win)
{
	const int64_t wbase = from >= 0 ? from / 16 * 16 : -((-from + 15) / 16 * 16);
	win.assign((size_t)((to - wbase + 15) / 16 * 16), 0);
	for (int64_t c = wbase; c < to; c += 16) px_stage_chunk(c, n, win.data() + (c - wbase), HostLoad16{ img.data() });
	return wbase;
}
static void load_hits(const std::vector<uint64_t> &hit, int64_t n, int64_t i0, uint64_t h[PX_ITEMS + 2])
{
	for (int q = 0; q < PX_ITEMS + 2; ++q) { const int64_t i = i0 - 1 + q; h[q] = i >= 0 && i < n ? hit[(size_t)i] : PX_NONE; }
}

int main(int argc, char **argv)
{
	if (argc != 4) { fprintf(stderr, "usage: path_model_check <model file> <sequences> hits|records|gaf|stats|reader|records-kept\n"); return 2; }
	const char *mode = argv[3];
	if (strcmp(mode, "reader") == 0 || strcmp(mode, "records-kept") == 0) {
		const bool kept = strcmp(mode, "records-kept") == 0;
		SeqReader rd(kept);
		seq_record_t r;
		if (!rd.open(argv[2])) return fail("cannot read the sequences");
		while (rd.next(r)) {
			if (!kept) { printf("%s\t%s\n", r.name.c_str(), r.seq.c_str()); continue; }
			for (const std::string *s : { &r.name, &r.comment, &r.seq, &r.qual }) { printf("%zu:", s->size()); fwrite(s->data(), 1, s->size(), stdout); }
			putchar('\n');
		}
		return rd.failed() ? fail("the sequences are damaged") : 0;
	}
	FILE *fp = fopen(argv[1], "rb");
	uint64_t head[6];
	if (!fp || fread(head, 8, 6, fp) != 6) return fail("cannot read the file");
	const int k = (int)head[0], min_cnt = (int)head[1], min_len = (int)head[3];
	const uint64_t n_u = head[4], n_bases = head[5];
	if (k < 3 || k > 31 || !(k & 1)) return fail("k must be odd and in [3, 31]");
	std::vector<gf_desc_t> desc((size_t)n_u);
	std::vector<unsigned char> bases((size_t)((n_bases + 15) / 16 * 16), '\n');      /* as the library allocates them: a read past that is the sanitizer's */
	if (n_u && fread(desc.data(), sizeof(gf_desc_t), (size_t)n_u, fp) != n_u) return fail("the file is short");
	if (n_bases && fread(bases.data(), 1, (size_t)n_bases, fp) != n_bases) return fail("the file is short");
	fclose(fp);

	/* what the open checks on the host: the descriptors tile the bases */
	uint64_t at = 0, n_node = 0;
	std::vector<uint32_t> nodes_of((size_t)n_u);
	for (uint64_t j = 0; j < n_u; ++j) {
		if (desc[j].off != at || !px_desc_fits(&desc[j], n_bases, k)) return fail("a descriptor does not fit the bases");
		at += desc[j].n_node + (uint64_t)(k - 1); n_node += desc[j].n_node;
		nodes_of[j] = (uint32_t)desc[j].n_node;
	}
	if (at != n_bases) return fail("the descriptors do not fit the bases");
	uint64_t cap = n_u ? gf_capacity(n_node) : 0;
	if (n_u && head[2]) {
		if (head[2] < n_node) return fail("the capacity is below the number of keys");
		for (cap = 1; cap < head[2]; cap <<= 1) {}
	}

	/* the index */
	std::vector<gf_slot_t> slots((size_t)cap, gf_slot_t{ GF_EMPTY, GF_EMPTY });
	const auto cas = [](uint64_t *p, uint64_t expected, uint64_t desired) { const uint64_t old = *p; if (old == expected) *p = desired; return old; };
	px_err_t e = { 0, 0, 0, 0, 0 };
	std::vector<unsigned char> win;
	for (uint64_t tile0 = 0; tile0 < n_bases; tile0 += PX_TILE) {
		const int64_t wbase = stage(bases, (int64_t)n_bases, (int64_t)tile0, (int64_t)tile0 + PX_TILE + PX_HALO, win);
		for (int t = 0; t < PX_THREADS; ++t)
			px_index_thread(desc.data(), n_u, n_bases, win.data(), wbase, tile0 + (uint64_t)t * PX_ITEMS, k, slots.data(), cap, cas, &e);
	}
	if (e.full) return fail("a node met no free slot");
	if (e.bad) return fail("a descriptor does not fit the bases");
	if (e.nonbase) return fail("a node does not fit: it holds a byte that is none of ACGT");
	if (e.dup) return fail("a node stands in two places");
	uint64_t n_key = 0;
	for (const gf_slot_t &s : slots) n_key += s.key != GF_EMPTY;
	if (n_key != n_node) return fail("the index does not hold every node");

	/* the sequences: one chunk */
	std::vector<std::string> seqs;
	std::vector<unsigned char> img;
	std::vector<uint64_t> off;
	std::vector<uint32_t> len;
	{
		SeqReader rd(false);
		seq_record_t r;
		if (!rd.open(argv[2])) return fail("cannot read the sequences");
		while (rd.next(r)) {
			const std::string &seq = r.seq;
			off.push_back(img.size()); len.push_back((uint32_t)seq.size());
			seqs.push_back(r.name);
			img.insert(img.end(), seq.begin(), seq.end());
			img.push_back('\n');
		}
		if (rd.failed()) return fail("the sequences are damaged");
	}
	const int64_t n = (int64_t)img.size(), n16 = (n + 15) / 16 * 16;
	img.resize((size_t)n16, 'A');                                  /* whatever lies behind the image is not looked at */
	unsigned char nt4[256];
	for (int c = 0; c < 256; ++c) nt4[c] = 4;
	for (int c = 0; c < 4; ++c) nt4[c] = nt4[(int)"ACGT"[c]] = nt4[(int)"acgt"[c]] = (unsigned char)c;
	nt4[(int)'U'] = nt4[(int)'u'] = 3;

	/* hits */
	std::vector<uint64_t> hit((size_t)n16, 0x5555555555555555ull);
	for (int64_t tile0 = 0; tile0 < n16; tile0 += PX_TILE) {                  /* (tiles of 8 end in front of n16, those of 1024 never do) */
		const int64_t wbase = stage(img, n, tile0 - PX_HALO, tile0 + PX_TILE, win);
		for (int t = 0; t < PX_THREADS; ++t) {
			const int64_t i0 = tile0 + (int64_t)t * PX_ITEMS;
			if (i0 >= n16) continue;
			uint64_t out[PX_ITEMS];
			px_hits_thread(slots.data(), cap, nt4, win.data(), wbase, i0, k, n_u, out, &e);
			for (int q = 0; q < PX_ITEMS; ++q) hit[(size_t)(i0 + q)] = out[q];
		}
	}
	if (e.bad) return fail("a value of the index names no unitig");
	for (int64_t i = n; i < n16; ++i) if (hit[(size_t)i] != PX_NONE) return fail("a hit behind the image");
	if (strcmp(mode, "hits") == 0) {
		for (int64_t i = 0; i < n; ++i) printf("%llu\n", (unsigned long long)hit[(size_t)i]);
		return 0;
	}

	/* count */
	const uint64_t m = ((uint64_t)n + PX_TILE - 1) / PX_TILE;
	std::vector<uint64_t> tile((size_t)(m + 1) * PXT_WORDS, 0);
	uint64_t h[PX_ITEMS + 2];
	unsigned fl[PX_ITEMS];
	for (uint64_t b = 0; b < m; ++b) {
		px_cnt_t all;
		px_cnt_zero(&all);
		for (int t = 0; t < PX_THREADS; ++t) {
			load_hits(hit, n, (int64_t)(b * PX_TILE) + (int64_t)t * PX_ITEMS, h);
			all = px_cnt_join(all, px_count_thread(h, fl));
		}
		px_tile_put(tile.data() + b * PXT_WORDS, &all);
	}
	/* scan: the slices of k_path_tile_scan */
	{
		const uint64_t per = (m + PX_THREADS - 1) / PX_THREADS;
		px_cnt_t own[PX_THREADS], before;
		px_cnt_zero(&before);
		for (uint64_t t = 0; t < PX_THREADS; ++t) { const uint64_t lo = t * per < m ? t * per : m, hi = lo + per < m ? lo + per : m; own[t] = px_tile_join(tile.data(), lo, hi); }
		for (uint64_t t = 0; t < PX_THREADS; ++t) {
			const uint64_t lo = t * per < m ? t * per : m, hi = lo + per < m ? lo + per : m;
			px_tile_apply(tile.data(), lo, hi, before);
			before = px_cnt_join(before, own[t]);
		}
		px_tile_put(tile.data() + m * PXT_WORDS, &before);
	}
	const uint64_t n_path = tile[m * PXT_WORDS + PXT_PATH], n_step = tile[m * PXT_WORDS + PXT_STEP];

	/* emit */
	const px_path_t poison = { ~(uint64_t)0, ~(uint64_t)0, ~0u, ~0u, ~0u, ~0u };
	std::vector<px_path_t> paths((size_t)n_path, poison);
	std::vector<uint64_t> steps((size_t)n_step, ~(uint64_t)0);
	px_emit_t a;
	a.seq_off = off.data(); a.n_seq = off.size(); a.desc = desc.data(); a.n_unitig = n_u;
	a.paths = paths.data(); a.cap_paths = n_path; a.steps = steps.data(); a.cap_steps = n_step; a.k = k;
	for (uint64_t b = 0; b < m; ++b) {
		px_cnt_t in_tile;
		px_cnt_zero(&in_tile);
		for (int t = 0; t < PX_THREADS; ++t) {
			const int64_t i0 = (int64_t)(b * PX_TILE) + (int64_t)t * PX_ITEMS;
			load_hits(hit, n, i0, h);
			const px_cnt_t own = px_count_thread(h, fl);
			px_cnt_t before = px_cnt_join(px_tile_get(tile.data() + b * PXT_WORDS), in_tile);
			for (int q = 0; q < PX_ITEMS; ++q) {
				px_emit_pos(&a, (uint64_t)i0 + (uint64_t)q, h[q + 1], fl[q], &before, &e);
				px_cnt_add(&before, fl[q]);
			}
			in_tile = px_cnt_join(in_tile, own);
		}
	}
	if (e.bad) return fail("a record does not fit the lists");
	for (const px_path_t &p : paths) if (p.step_off == poison.step_off || p.ps == poison.ps || p.seq == ~0u || p.n_step == ~0u || p.qs == ~0u || p.qe == ~0u) return fail("a field of a record was not written");
	for (uint64_t s : steps) if (s == ~(uint64_t)0) return fail("a step was not written");

	/* tallies */
	std::vector<px_tally_t> tally(off.size());
	for (size_t s = 0; s < off.size(); ++s) {
		uint64_t lo = off[s], hi = lo + len[s];
		hi = hi < (uint64_t)n ? hi : (uint64_t)n; lo = lo < hi ? lo : hi;
		uint32_t acc[4] = { 0, 0, 0, 0 };
		for (unsigned lane = 0; lane < PX_WAVE; ++lane) px_tally_seq(hit.data(), tile.data(), lo, hi, lane, PX_WAVE, acc);
		tally[s] = px_tally_t{ acc[0], acc[1], acc[2], acc[3] };
	}

	std::string text;
	if (strcmp(mode, "records") == 0) {
		for (const px_path_t &p : paths) printf("P %u %u %u %llu %llu %u\n", p.seq, p.qs, p.qe, (unsigned long long)p.ps, (unsigned long long)p.step_off, p.n_step);
		for (uint64_t s : steps) printf("S %llu\n", (unsigned long long)s);
		for (const px_tally_t &t : tally) printf("Y %u %u %u %u\n", t.n_kmer, t.n_hit, t.n_path, t.n_step);
		printf("T %llu %llu %llu\n", (unsigned long long)cap, (unsigned long long)n_key, (unsigned long long)e.probe);
		return 0;
	}
	if (strcmp(mode, "gaf") == 0) {
		if (!pxt_gaf(text, seqs, len.data(), paths.data(), n_path, steps.data(), n_step, nodes_of.data(), n_u, k, min_len)) return fail("a record does not fit its chunk");
	} else if (strcmp(mode, "stats") == 0) {
		pxt_total_t tot = { 0, 0, 0, 0, 0, 0 };
		pxt_stats_head(text, k, min_cnt);
		pxt_stats(text, seqs, len.data(), tally.data(), &tot);
		pxt_stats_tail(text, tot);
	} else return fail("the mode is none of hits, records, gaf, stats, reader");
	fwrite(text.data(), 1, text.size(), stdout);
	return 0;
}
