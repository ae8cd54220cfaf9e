/* path_step.h -- the per-thread steps of `yak-amd paths` (include/yak_amd_path.h).  No HIP in here, as in ../gfa/gfa_step.h,
 * whose k-mer arithmetic and open-addressing table this layer uses unchanged: GF_FN is `__host__ __device__` under hipcc and empty otherwise, so that
 * the kernels of path.hip and the sequential model of tests/tools/path_model_check.cpp (host compiler, sanitizers) call the very same functions.
 *
 * A workgroup of PX_THREADS threads serves a tile of PX_TILE consecutive positions, a thread PX_ITEMS consecutive ones.  The bytes a tile needs are
 * staged first (px_stage_chunk: 16 bytes at a time, the bytes outside [0, n) as '\n'), so a step never asks where the image ends: `win` is the
 * staged window, win[x] the byte at position wbase + x.
 *   index  the window is the tile and PX_HALO bytes behind it: position g of bases[] is node p = g - off_j of unitig j where p < n_node_j, its k-mer
 *          the bytes g .. g + k - 1
 *   hits   the window is PX_HALO bytes in front of the tile and the tile: Q_i ends at byte i
 * The flags of a position are a function of hit[i - 1], hit[i] and hit[i + 1] alone (px_flags); the count, the emit and the tallies derive them
 * again instead of keeping them.  What a thread, a workgroup and a tile hand on is a px_cnt_t under px_cnt_join(): four sums and the steps of the
 * path that is open at its end (a segmented sum: a path start sets it back). */
#ifndef YK_PATH_STEP_H
#define YK_PATH_STEP_H
#include "../gfa/gfa_step.h"

#define PX_NONE   (~(uint64_t)0)             /* YAKAMD_PATH_NONE */
#define PX_ABSENT (~(uint64_t)0 - 1)         /* YAKAMD_PATH_ABSENT */
#ifndef PX_THREADS_N                         /* the model of the kernels is also built with fewer threads: tiles of 8 positions */
#define PX_THREADS_N 256
#endif
enum { PX_THREADS = PX_THREADS_N, PX_ITEMS = 4, PX_TILE = PX_THREADS * PX_ITEMS, PX_HALO = 32, PX_WIN = PX_TILE + PX_HALO, PX_WAVE = 64 };
enum { PXF_KMER = 1, PXF_HIT = 2, PXF_PSTART = 4, PXF_SSTART = 8, PXF_PEND = 16 };
/* the words of a tile's entry in the tile array: as counted, and after the scan (the exclusive prefixes; PXT_SEGV the steps of the path that is
 * open where the tile begins) */
enum { PXT_PATH = 0, PXT_STEP = 1, PXT_HIT = 2, PXT_KMER = 3, PXT_SEGF = 4, PXT_SEGV = 5, PXT_WORDS = 8 };

typedef struct { uint64_t step_off, ps; uint32_t seq, n_step, qs, qe; } px_path_t;      /* yakamd_upath_t, include/yak_amd_path.h */
typedef struct { uint32_t n_kmer, n_hit, n_path, n_step; } px_tally_t;                  /* yakamd_ptally_t */
typedef struct { uint64_t probe, bad, full, dup, nonbase; } px_err_t;                   /* what a thread gathers beside its results */
typedef struct { uint64_t path, step, hit, kmer, seg_flag, seg_val; } px_cnt_t;

/* ---- staging: the 16 bytes of the window that hold positions c .. c + 15 (c a multiple of 16, possibly negative) of an image of n bytes whose
 * allocation reaches to n rounded up to 16: bytes outside [0, n) read '\n'.  load16(c, dst) fetches 16 bytes at offset c ---- */
template <class Load16> GF_FN void px_stage_chunk(int64_t c, int64_t n, unsigned char *dst, Load16 load16)
{
	if (c < 0 || c >= n) { for (int x = 0; x < 16; ++x) dst[x] = '\n'; return; }
	load16(c, dst);
	if (c + 16 > n) for (int x = (int)(n - c); x < 16; ++x) dst[x] = '\n';
}

/* ---- the index ---- */
/* A C G T -> 0 1 2 3, anything else 4: the bases of a walk are these four letters */
GF_FN unsigned px_acgt(unsigned c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' ? ((c >> 1 ^ c >> 2) & 3u) : 4u; }
/* 1 iff the n_node + k - 1 bases of d lie inside bases[0 .. n_bases) and its numbers fit a value of the index */
GF_FN int px_desc_fits(const gf_desc_t *d, uint64_t n_bases, int k)
{
	return d->n_node >= 1 && d->n_node < ((uint64_t)1 << 31) && d->off <= n_bases && d->n_node <= n_bases - d->off && (uint64_t)(k - 1) <= n_bases - d->off - d->n_node;
}
/* the last unitig with off <= g; n_unitig >= 1.  -1 when there is none */
GF_FN int64_t px_unitig_of(const gf_desc_t *desc, uint64_t n_unitig, uint64_t g)
{
	uint64_t lo = 0, hi = n_unitig;                                 /* off[lo - 1] <= g < off[hi] */
	while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (desc[mid].off <= g) lo = mid + 1; else hi = mid; }
	return (int64_t)lo - 1;
}
/* the nodes among positions g0 .. g0 + PX_ITEMS - 1 of bases[] are claimed: the unitig by one binary search, then forward; the k-mer packed once
 * from the window, then rolled */
template <class Cas> GF_FN void px_index_thread(const gf_desc_t *desc, uint64_t n_unitig, uint64_t n_bases, const unsigned char *win, int64_t wbase, uint64_t g0,
                                                int k, gf_slot_t *slots, uint64_t cap, Cas cas, px_err_t *e)
{
	if (g0 >= n_bases) return;
	int64_t j = px_unitig_of(desc, n_unitig, g0);
	if (j < 0) { ++e->bad; return; }
	gf_desc_t d = desc[j];
	if (!px_desc_fits(&d, n_bases, k)) { ++e->bad; return; }
	const uint64_t mask = ~(uint64_t)0 >> (64 - 2 * k);
	uint64_t w = 0;
	int len = 0;
	for (int x = 0; x < k - 1; ++x) {
		const unsigned c = px_acgt(win[(int64_t)g0 - wbase + x]);
		w = (w << 2 | (c & 3u)) & mask;
		len = c < 4u ? len + 1 : 0;
	}
	for (int q = 0; q < PX_ITEMS; ++q) {
		const uint64_t g = g0 + (uint64_t)q;
		if (g >= n_bases) return;
		const unsigned c = px_acgt(win[(int64_t)g - wbase + (k - 1)]);
		w = (w << 2 | (c & 3u)) & mask;
		len = c < 4u ? len + 1 : 0;
		uint64_t end = d.off + d.n_node + (uint64_t)(k - 1);
		while (g >= end) {                                          /* the next unitig begins where this one ends */
			if ((uint64_t)++j >= n_unitig) { ++e->bad; return; }
			d = desc[j];
			if (!px_desc_fits(&d, n_bases, k) || d.off != end) { ++e->bad; return; }
			end = d.off + d.n_node + (uint64_t)(k - 1);
		}
		const uint64_t p = g - d.off;
		if (p >= d.n_node) continue;                                /* the k - 1 positions behind the last node */
		if (len < k) { ++e->nonbase; continue; }
		if ((uint64_t)j >= ((uint64_t)1 << 31)) { ++e->bad; return; }
		const uint64_t key = gf_canon(w, k);
		uint64_t pr = 0;
		const int r = gf_claim(slots, cap, key, (uint64_t)j << 32 | p << 1 | (uint64_t)(w != key), cas, &pr);
		if (pr > e->probe) e->probe = pr;
		if (r == -1) ++e->full;
		if (r == -2) ++e->dup;
	}
}

/* ---- the hits of positions i0 .. i0 + PX_ITEMS - 1: the forward and the reverse word rolled together, one probe walk per k-mer.  The first slot of
 * every walk is fetched before any is looked at, so that a thread has its PX_ITEMS loads in flight together; a walk that does not end in its first
 * slot goes on through gf_find ---- */
#if defined(__HIPCC__)
#define PX_UNROLL _Pragma("unroll")
#else
#define PX_UNROLL
#endif
GF_FN void px_hits_thread(const gf_slot_t *slots, uint64_t cap, const unsigned char *nt4, const unsigned char *win, int64_t wbase, int64_t i0, int k,
                          uint64_t n_unitig, uint64_t out[PX_ITEMS], px_err_t *e)
{
	const uint64_t mask = ~(uint64_t)0 >> (64 - 2 * k);
	const int up = 2 * (k - 1);
	uint64_t f = 0, r = 0, key[PX_ITEMS];
	unsigned state[PX_ITEMS];                                       /* 0: no k-mer; 1: Q is canonical; 2: it is not */
	gf_slot_t first[PX_ITEMS];
	int len = 0;
	for (int x = k - 1; x >= 1; --x) {
		const unsigned c = nt4[win[i0 - x - wbase]];
		f = (f << 2 | (c & 3u)) & mask;
		r = r >> 2 | (uint64_t)(3u - (c & 3u)) << up;
		len = c < 4u ? len + 1 : 0;
	}
	PX_UNROLL
	for (int q = 0; q < PX_ITEMS; ++q) {
		const unsigned c = nt4[win[i0 + q - wbase]];
		f = (f << 2 | (c & 3u)) & mask;
		r = r >> 2 | (uint64_t)(3u - (c & 3u)) << up;
		len = c < 4u ? len + 1 : 0;
		key[q] = f < r ? f : r;
		state[q] = len < k ? 0u : f == key[q] ? 1u : 2u;
	}
	PX_UNROLL
	for (int q = 0; q < PX_ITEMS; ++q) {
		first[q].key = GF_EMPTY; first[q].val = 0;
		if (state[q] && cap) first[q] = slots[gf_hash(key[q]) & (cap - 1)];
	}
	PX_UNROLL
	for (int q = 0; q < PX_ITEMS; ++q) {
		if (!state[q]) { out[q] = PX_NONE; continue; }
		uint64_t val = first[q].val, pr = cap ? 1 : 0;
		int hit = first[q].key == key[q];
		if (!hit && first[q].key != GF_EMPTY) hit = gf_find(slots, cap, key[q], &val, &pr);
		if (pr > e->probe) e->probe = pr;
		if (!hit) { out[q] = PX_ABSENT; continue; }
		if (val >> 32 >= n_unitig) { ++e->bad; out[q] = PX_ABSENT; continue; }
		out[q] = val ^ (uint64_t)(state[q] == 2u);
	}
}

/* ---- flags ---- */
GF_FN int px_is_hit(uint64_t h) { return h < PX_ABSENT; }
/* 1 iff position i with hit b continues position i - 1 with hit a */
GF_FN int px_continues(uint64_t a, uint64_t b)
{
	if (!px_is_hit(a) || !px_is_hit(b) || a >> 32 != b >> 32 || ((a ^ b) & 1)) return 0;
	const uint32_t pa = (uint32_t)a >> 1, pb = (uint32_t)b >> 1;   /* below 2^31 */
	return (b & 1) ? pa == pb + 1u : pb == pa + 1u;
}
/* prev = PX_NONE at position 0, next = PX_NONE at the last position */
GF_FN unsigned px_flags(uint64_t prev, uint64_t cur, uint64_t next)
{
	if (cur == PX_NONE) return 0u;
	if (!px_is_hit(cur)) return PXF_KMER;
	unsigned fl = PXF_KMER | PXF_HIT;
	if (!px_is_hit(prev)) fl |= PXF_PSTART;
	if (!px_continues(prev, cur)) fl |= PXF_SSTART;
	if (!px_is_hit(next)) fl |= PXF_PEND;
	return fl;
}
GF_FN void px_cnt_zero(px_cnt_t *a) { a->path = a->step = a->hit = a->kmer = a->seg_flag = a->seg_val = 0; }
/* a position behind what a holds */
GF_FN void px_cnt_add(px_cnt_t *a, unsigned fl)
{
	a->kmer += fl & PXF_KMER ? 1u : 0u;
	a->hit += fl & PXF_HIT ? 1u : 0u;
	if (fl & PXF_PSTART) { ++a->path; a->seg_flag = 1; a->seg_val = 0; }
	if (fl & PXF_SSTART) { ++a->step; ++a->seg_val; }
}
/* what x holds and, behind it, what y holds; associative */
GF_FN px_cnt_t px_cnt_join(px_cnt_t x, px_cnt_t y)
{
	px_cnt_t z;
	z.path = x.path + y.path; z.step = x.step + y.step; z.hit = x.hit + y.hit; z.kmer = x.kmer + y.kmer;
	z.seg_flag = x.seg_flag | y.seg_flag;
	z.seg_val = y.seg_flag ? y.seg_val : x.seg_val + y.seg_val;
	return z;
}
/* the flags of positions i0 .. i0 + PX_ITEMS - 1 from h[0 .. PX_ITEMS + 1] = hit[i0 - 1 .. i0 + PX_ITEMS], and their px_cnt_t */
GF_FN px_cnt_t px_count_thread(const uint64_t h[PX_ITEMS + 2], unsigned fl[PX_ITEMS])
{
	px_cnt_t a;
	px_cnt_zero(&a);
	for (int q = 0; q < PX_ITEMS; ++q) { fl[q] = px_flags(h[q], h[q + 1], h[q + 2]); px_cnt_add(&a, fl[q]); }
	return a;
}

/* ---- emit ---- */
typedef struct {
	const uint64_t *seq_off; uint64_t n_seq;
	const gf_desc_t *desc; uint64_t n_unitig;
	px_path_t *paths; uint64_t cap_paths;
	uint64_t *steps; uint64_t cap_steps;
	int k;
} px_emit_t;
/* the last sequence with off <= i; -1 when there is none */
GF_FN int64_t px_seq_of(const uint64_t *seq_off, uint64_t n_seq, uint64_t i)
{
	uint64_t lo = 0, hi = n_seq;
	while (lo < hi) { const uint64_t mid = lo + ((hi - lo) >> 1); if (seq_off[mid] <= i) lo = mid + 1; else hi = mid; }
	return (int64_t)lo - 1;
}
/* position i with hit h and flags fl; before holds everything in front of i (absolute: the tile's prefix joined in).  A step start writes its step; a
 * path start step_off, ps, seq and qs of its record; a path end n_step and qe of the record of the same rank -- disjoint fields */
GF_FN void px_emit_pos(const px_emit_t *a, uint64_t i, uint64_t h, unsigned fl, const px_cnt_t *before, px_err_t *e)
{
	if (!(fl & (PXF_SSTART | PXF_PSTART | PXF_PEND))) return;
	px_cnt_t at = *before;
	px_cnt_add(&at, fl);                                            /* inclusive of i */
	if (fl & PXF_SSTART) {
		if (before->step >= a->cap_steps) { ++e->bad; return; }
		a->steps[before->step] = h >> 32 << 1 | (h & 1);
	}
	if (!(fl & (PXF_PSTART | PXF_PEND))) return;
	const uint64_t rank = at.path - 1;
	if (at.path < 1 || rank >= a->cap_paths) { ++e->bad; return; }
	const int64_t s = px_seq_of(a->seq_off, a->n_seq, i);
	if (s < 0) { ++e->bad; return; }
	const uint64_t off = a->seq_off[s];
	px_path_t *r = a->paths + rank;
	if (fl & PXF_PSTART) {
		const uint64_t j = h >> 32, p = (uint32_t)h >> 1;
		if (j >= a->n_unitig) { ++e->bad; return; }
		const uint64_t n = a->desc[j].n_node;
		if (p >= n) { ++e->bad; return; }
		r->step_off = before->step;
		r->ps = (h & 1) ? n - 1 - p : p;
		r->seq = (uint32_t)s;
		r->qs = (uint32_t)(i + 1 - (uint64_t)a->k - off);
	}
	if (fl & PXF_PEND) {
		if (at.seg_val > 0xffffffffull) { ++e->bad; return; }
		r->n_step = (uint32_t)at.seg_val;
		r->qe = (uint32_t)(i + 1 - off);
	}
}

/* ---- the tally of a sequence: lane `lane` of n_lane adds its share of positions [lo, hi) of hit[0 .. n) to acc[4] (k-mers, hits, paths, steps) ---- */
GF_FN void px_tally_range(const uint64_t *hit, uint64_t lo, uint64_t hi, unsigned lane, unsigned n_lane, uint32_t acc[4])
{
	for (uint64_t i = lo + lane; i < hi; i += n_lane) {
		const unsigned fl = px_flags(i ? hit[i - 1] : PX_NONE, hit[i], PX_NONE);
		acc[0] += fl & PXF_KMER ? 1u : 0u; acc[1] += fl & PXF_HIT ? 1u : 0u; acc[2] += fl & PXF_PSTART ? 1u : 0u; acc[3] += fl & PXF_SSTART ? 1u : 0u;
	}
}
/* the same for sequence [lo, hi) (hi <= n) with the scanned tile array: the whole tiles inside it come from two of its entries, by lane 0 */
GF_FN void px_tally_seq(const uint64_t *hit, const uint64_t *tile, uint64_t lo, uint64_t hi, unsigned lane, unsigned n_lane, uint32_t acc[4])
{
	const uint64_t t_lo = (lo + PX_TILE - 1) / PX_TILE, t_hi = hi / PX_TILE;
	if (t_lo >= t_hi) { px_tally_range(hit, lo, hi, lane, n_lane, acc); return; }
	px_tally_range(hit, lo, t_lo * PX_TILE, lane, n_lane, acc);
	px_tally_range(hit, t_hi * PX_TILE, hi, lane, n_lane, acc);
	if (lane == 0) {
		const uint64_t *a = tile + t_lo * PXT_WORDS, *b = tile + t_hi * PXT_WORDS;
		acc[0] += (uint32_t)(b[PXT_KMER] - a[PXT_KMER]); acc[1] += (uint32_t)(b[PXT_HIT] - a[PXT_HIT]);
		acc[2] += (uint32_t)(b[PXT_PATH] - a[PXT_PATH]); acc[3] += (uint32_t)(b[PXT_STEP] - a[PXT_STEP]);
	}
}

/* ---- the scan of the tile array, a slice [lo, hi) of it by one thread: its join first (px_tile_join), then, on top of what lies in front of the
 * slice, every entry replaced by what lies in front of it (px_tile_apply) ---- */
GF_FN px_cnt_t px_tile_get(const uint64_t *t)
{
	px_cnt_t c;
	c.path = t[PXT_PATH]; c.step = t[PXT_STEP]; c.hit = t[PXT_HIT]; c.kmer = t[PXT_KMER]; c.seg_flag = t[PXT_SEGF]; c.seg_val = t[PXT_SEGV];
	return c;
}
GF_FN void px_tile_put(uint64_t *t, const px_cnt_t *c)
{
	t[PXT_PATH] = c->path; t[PXT_STEP] = c->step; t[PXT_HIT] = c->hit; t[PXT_KMER] = c->kmer; t[PXT_SEGF] = c->seg_flag; t[PXT_SEGV] = c->seg_val;
}
GF_FN px_cnt_t px_tile_join(const uint64_t *tile, uint64_t lo, uint64_t hi)
{
	px_cnt_t a;
	px_cnt_zero(&a);
	for (uint64_t t = lo; t < hi; ++t) a = px_cnt_join(a, px_tile_get(tile + t * PXT_WORDS));
	return a;
}
GF_FN px_cnt_t px_tile_apply(uint64_t *tile, uint64_t lo, uint64_t hi, px_cnt_t before)
{
	for (uint64_t t = lo; t < hi; ++t) {
		const px_cnt_t own = px_tile_get(tile + t * PXT_WORDS);
		px_tile_put(tile + t * PXT_WORDS, &before);
		before = px_cnt_join(before, own);
	}
	return before;
}
#endif
