/* seg_sort_check.cpp -- whole multi-pass sorts through the tile arithmetic of k_seg_sort_pass (yak_amd/csrc/seg_sort_tile.h), on the CPU, against
 * std::stable_sort.  The model follows the kernel step by step: the first pass counts every digit's histogram, each pass scans its own, then per
 * tile: wave-major split, rank among the wave's equal digits round by round, per-wave counts -> prefix over the waves -> the digits' starts in the
 * tile -> the tile laid out by digit in a copy -> the copy stored in index order.  Every index is checked against the array it goes into (and the
 * program is built with the address sanitizer), every destination is written exactly once, and each pass must be the stable sort by its digit.
 * Prints "ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "../../yak_amd/csrc/seg_sort_tile.h"

typedef uint64_t u64;
typedef uint32_t u32;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "seg_sort_check: %s failed at line %d (nt %d, len %llu, dist %d, shift %d)\n", #c, __LINE__, g_nt, (unsigned long long)g_len, g_dist, g_shift); exit(1); } } while (0)
static int g_nt, g_dist, g_shift;
static u64 g_len;

static u64 rng_state = 88172645463325252ull;
static u64 rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

/* one pass over the segment [a, a + len) of src into dst; hist = the sort's sst_n_digits rows of this segment (filled by the pass with shift 0) */
static void pass(int nt, u64 a, u64 len, const std::vector<u64> &src_kc, const std::vector<u64> &src_t, std::vector<u64> &dst_kc, std::vector<u64> &dst_t,
                 int shift, std::vector<u32> &dig_hist, u64 seg_no, int n_dig)
{
	const int nwv = nt / 64, E = sst_per_thread(nt), TILE = sst_tile(nt);
	if (len == 0) return;
	if (len == 1) { dst_kc[a] = src_kc[a]; dst_t[a] = src_t[a]; return; }
	std::vector<u32> run(SST_NBIN, 0), start(SST_NBIN), base(SST_NBIN), wc((size_t)nwv * SST_NBIN);
	if (shift > 0 && n_dig > 1) {
		for (int q = 0; q < SST_NBIN; ++q) run[q] = dig_hist.at(sst_hist_row(seg_no, n_dig, shift / 8) + q);
	} else {
		for (u64 i = 0; i < len; ++i) {
			const u64 t = src_t[a + i];
			run[sst_digit(t, shift)]++;
			if (n_dig > 1) for (int j = 1; j < n_dig; ++j) dig_hist.at(sst_hist_row(seg_no, n_dig, j) + sst_digit(t, 8 * j))++;
		}
	}
	{ u32 e = 0; for (int q = 0; q < SST_NBIN; ++q) { const u32 v = run[q]; run[q] = e; e += v; } CHECK(e == len); }
	std::vector<u64> stage_t(TILE), stage_k(TILE);
	std::vector<char> written(len, 0);
	for (u64 tile = 0; tile < len; tile += TILE) {
		const u32 n_tile = (u32)std::min<u64>(TILE, len - tile);
		std::fill(wc.begin(), wc.end(), 0u);
		std::vector<u32> erk((size_t)nt * E, 0xffffffffu);
		std::vector<u64> et((size_t)nt * E), ek((size_t)nt * E);
		for (int wave = 0; wave < nwv; ++wave)
			for (int r = 0; r < E; ++r) {
				u32 seen[SST_NBIN] = {0};                        /* the ballots: lanes before this one with the same digit, in this round */
				for (int lane = 0; lane < 64; ++lane) {
					const u64 idx = sst_src_index(tile, wave, r, lane, E);
					if (idx >= len) continue;
					CHECK(idx < tile + n_tile);
					const u32 d = sst_digit(src_t[a + idx], shift);
					const size_t reg = ((size_t)wave * 64 + lane) * E + r;
					et[reg] = src_t[a + idx]; ek[reg] = src_kc[a + idx];
					erk[reg] = d << 24 | (wc[(size_t)wave * SST_NBIN + d] + seen[d]);
					seen[d]++;
				}
				for (int d = 0; d < SST_NBIN; ++d) wc[(size_t)wave * SST_NBIN + d] += seen[d];
			}
		for (int d = 0; d < SST_NBIN; ++d) start[d] = sst_wave_prefix(wc.data(), nwv, d);
		{
			u32 e = 0;
			for (int d = 0; d < SST_NBIN; ++d) { const u32 v = start[d]; start[d] = e; base[d] = sst_base(run[d], e); run[d] += v; e += v; }
			CHECK(e == n_tile);
		}
		std::vector<char> staged(TILE, 0);
		for (int tid = 0; tid < nt; ++tid)
			for (int r = 0; r < E; ++r) {
				const size_t reg = (size_t)tid * E + r;
				if (erk[reg] == 0xffffffffu) continue;
				const u32 d = erk[reg] >> 24, pos = sst_lds_pos(start[d], wc[(size_t)(tid >> 6) * SST_NBIN + d], erk[reg] & 0xffffff);
				CHECK(pos < n_tile && !staged[pos]);
				staged[pos] = 1; stage_t[pos] = et[reg]; stage_k[pos] = ek[reg];
			}
		for (int r = 0; r < E; ++r)
			for (int tid = 0; tid < nt; ++tid) {
				const u32 i = (u32)r * nt + tid;
				if (i >= n_tile) continue;
				CHECK(staged[i]);
				const u64 g = sst_global(a, base[sst_digit(stage_t[i], shift)], i);
				CHECK(g >= a && g < a + len && !written[g - a]);
				written[g - a] = 1; dst_t.at(g) = stage_t[i]; dst_kc.at(g) = stage_k[i];
			}
	}
	for (u64 i = 0; i < len; ++i) CHECK(written[i]);
}

/* a shard of segments of these lengths, sorted by all the digits of tbits-bit times */
static void sort_case(int nt, const std::vector<u64> &lens, int dist, int tbits)
{
	const size_t P = lens.size();
	std::vector<u64> off(P + 1, 0);
	for (size_t p = 0; p < P; ++p) off[p + 1] = off[p] + lens[p];
	const u64 n = off[P];
	std::vector<u64> kc[2], tt[2];
	for (int b = 0; b < 2; ++b) { kc[b].assign(n + 1, ~0ull); tt[b].assign(n + 1, ~0ull); }
	const u64 tmask = tbits >= 64 ? ~0ull : ((u64)1 << tbits) - 1;
	for (u64 i = 0; i < n; ++i) {
		u64 t = rng() & tmask;
		if (dist == 1) t = (t & ~(u64)0xff) | 0x5a;               /* the first digit is one value (the later ones stay uniform) */
		if (dist == 2) t = (t & ~(u64)0xff) | (32 * (t >> 8 & 7) + 30);   /* eight distinct first digits */
		if (dist == 3) t = 0x5a5a5a5a5a5a5a5aull & tmask;      /* every digit is one value */
		kc[0][i] = i; tt[0][i] = t;
	}
	const int n_dig = sst_n_digits(tbits);
	std::vector<u32> dig_hist(P * n_dig * SST_NBIN, 0);
	int cur = 0;
	g_nt = nt; g_dist = dist;
	for (int shift = 0; shift < tbits; shift += 8) {
		g_shift = shift;
		for (size_t p = 0; p < P; ++p) {
			g_len = lens[p];
			pass(nt, off[p], lens[p], kc[cur], tt[cur], kc[cur ^ 1], tt[cur ^ 1], shift, dig_hist, p, n_dig);
			/* the pass is the stable sort by its digit */
			std::vector<u64> ord(lens[p]);
			for (u64 i = 0; i < lens[p]; ++i) ord[i] = off[p] + i;
			const std::vector<u64> &st = tt[cur];
			std::stable_sort(ord.begin(), ord.end(), [&](u64 x, u64 y) { return sst_digit(st[x], shift) < sst_digit(st[y], shift); });
			for (u64 i = 0; i < lens[p]; ++i) CHECK(kc[cur ^ 1][off[p] + i] == kc[cur][ord[i]] && tt[cur ^ 1][off[p] + i] == tt[cur][ord[i]]);
		}
		CHECK(kc[cur ^ 1][n] == ~0ull && tt[cur ^ 1][n] == ~0ull);
		cur ^= 1;
	}
	/* the whole sort: by time, equal times in the order of the input */
	for (size_t p = 0; p < P; ++p) {
		g_len = lens[p];
		std::vector<u64> ord(lens[p]);
		for (u64 i = 0; i < lens[p]; ++i) ord[i] = off[p] + i;
		std::vector<u64> t0(n);
		for (u64 i = 0; i < n; ++i) t0[kc[cur][i]] = tt[cur][i];          /* time of input element kc */
		std::stable_sort(ord.begin(), ord.end(), [&](u64 x, u64 y) { return t0[x] < t0[y]; });
		for (u64 i = 0; i < lens[p]; ++i) CHECK(kc[cur][off[p] + i] == ord[i]);
	}
}

int main()
{
	const int nts[2] = {256, 1024};
	for (int v = 0; v < 2; ++v) {
		const int nt = nts[v];
		const u64 T = (u64)sst_tile(nt);
		if (!(sst_per_thread(nt) * 64 * (nt / 64) == sst_tile(nt) && nt >= SST_NBIN)) { fprintf(stderr, "tile shape\n"); return 1; }
		const std::vector<u64> lens = {0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 0, 3, 1};
		for (int dist = 0; dist < 4; ++dist) {
			sort_case(nt, lens, dist, 21);                        /* three digits, the third one thin */
			sort_case(nt, lens, dist, 8);                         /* one pass: no shared histograms */
			sort_case(nt, lens, dist, 17);
		}
		sort_case(nt, lens, 0, 40);                               /* times beyond 32 bits (the accumulator path) */
		sort_case(nt, {2 * T + 1, T + 1}, 2, 64);                  /* SST_MAX_DIGITS rows */
	}
	if (sst_n_digits(64) > SST_MAX_DIGITS) { fprintf(stderr, "digit rows\n"); return 1; }
	printf("ok\n");
	return 0;
}
