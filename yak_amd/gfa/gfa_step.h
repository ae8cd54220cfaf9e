/* gfa_step.h -- the per-thread steps of the links between unitigs (`yak-amd unitigs -G`; include/yak_amd_gfa.h).  No HIP in
 * here, as in ../walk/uwalk_step.h: GF_FN is `__host__ __device__` under hipcc and empty otherwise, so that the kernels of gfa.hip and the
 * sequential model of tests/tools/gfa_model_check.cpp (host compiler, sanitizers) call the very same functions.
 *
 * A k-mer is packed two bits a base, A C G T = 0 1 2 3, the first base highest (the keys of the table: yak_amd.h); its canonical form is the
 * smaller of it and its reverse complement.  The end table is open addressing with linear probing over gf_slot_t, capacity a power of two, a free
 * slot's key all ones (no k-mer of k < 32 bases is); a key is claimed by a 64-bit compare-and-swap that the caller passes in -- atomicCAS on the
 * device, a plain compare in the model -- and its value is stored beside it, to be read by later launches only.
 * A value is j << GF_VAL_SHIFT | flags: the key is the first and / or the last node of open unitig j, and GF_*_REV says that S_j reads that node
 * reverse-complemented.  endw[2j + o] is W of oriented end (j, o), the last k bases of (j, o) packed; GF_CYCLE for both ends of a cycle. */
#ifndef YK_GFA_STEP_H
#define YK_GFA_STEP_H
#include <stdint.h>

#if defined(__HIPCC__)
#define GF_FN __host__ __device__ static inline
#else
#define GF_FN static inline
#endif

#define GF_EMPTY (~(uint64_t)0)              /* the key of a free slot */
#define GF_CYCLE (~(uint64_t)0)              /* endw[] of a cycle's two ends */
#define GF_BAD   (~(uint64_t)1)              /* endw[] of a unitig whose descriptor does not fit the bases */
enum { GF_FIRST = 1, GF_FIRST_REV = 2, GF_LAST = 4, GF_LAST_REV = 8, GF_VAL_SHIFT = 4 };

typedef struct { uint64_t off, n_node, kc, first; } gf_desc_t;                 /* yakamd_udesc_t, include/yak_amd_walk.h */
typedef struct { uint64_t from, to; } gf_link_t;                               /* yakamd_ulink_t, include/yak_amd_gfa.h */
typedef struct alignas(16) { uint64_t key, val; } gf_slot_t;                   /* one 16-byte load */

/* ---- k-mers ---- */
/* the arithmetic of hm_revcomp (libyak_amd.so's kernels) restated: the pairs of bits reversed, complemented, moved down to 2k bits */
GF_FN uint64_t gf_revcomp(uint64_t x, int k)
{
	x = (x >> 2 & 0x3333333333333333ull) | (x & 0x3333333333333333ull) << 2;
	x = (x >> 4 & 0x0f0f0f0f0f0f0f0full) | (x & 0x0f0f0f0f0f0f0f0full) << 4;
	return ~__builtin_bswap64(x) >> (64 - 2 * k);
}
GF_FN uint64_t gf_canon(uint64_t z, int k) { const uint64_t rc = gf_revcomp(z, k); return z < rc ? z : rc; }
/* k bases of ASCII ACGT packed; -1 when a byte is none of the four */
GF_FN int gf_pack(const char *s, int k, uint64_t *out)
{
	uint64_t x = 0;
	for (int i = 0; i < k; ++i) {
		const unsigned c = (unsigned char)s[i];
		if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return -1;
		x = x << 2 | ((c >> 1 ^ c >> 2) & 3u);                  /* A 0, C 1, G 2, T 3 */
	}
	*out = x;
	return 0;
}
/* Z = W[1:] + b */
GF_FN uint64_t gf_extend(uint64_t w, int b, int k) { return (w << 2 | (uint64_t)b) & (~(uint64_t)0 >> (64 - 2 * k)); }

/* ---- the ends of unitig j: its two W and its keys.  1: open, e filled; 0: a cycle (no key, both W GF_CYCLE); -1: the descriptor does not fit
 * the n_bases bases or they are not ACGT (both W GF_BAD) ---- */
typedef struct { uint64_t w[2], key[2], val[2]; int n_key; } gf_ends_t;
GF_FN int gf_ends(const gf_desc_t *u, uint64_t j, const char *bases, uint64_t n_bases, int k, gf_ends_t *e)
{
	e->n_key = 0;
	e->w[0] = e->w[1] = GF_BAD;
	if (u->n_node < 1 || u->off > n_bases || u->n_node > n_bases - u->off || (uint64_t)(k - 1) > n_bases - u->off - u->n_node) return -1;
	if (u->first & 1) { e->w[0] = e->w[1] = GF_CYCLE; return 0; }
	uint64_t f, l;
	if (gf_pack(bases + u->off, k, &f) != 0) return -1;
	l = f;
	if (u->n_node > 1 && gf_pack(bases + u->off + u->n_node - 1, k, &l) != 0) return -1;
	const uint64_t cf = gf_canon(f, k), cl = gf_canon(l, k);
	e->w[0] = l;                                                  /* (j, +) ends in the last node as S_j reads it */
	e->w[1] = gf_revcomp(f, k);                                   /* (j, -) in the first node, reverse-complemented */
	if (u->n_node == 1) {
		e->key[0] = cf;
		e->val[0] = j << GF_VAL_SHIFT | GF_FIRST | GF_LAST | (f != cf ? GF_FIRST_REV | GF_LAST_REV : 0);
		e->n_key = 1;
	} else {
		e->key[0] = cf; e->val[0] = j << GF_VAL_SHIFT | GF_FIRST | (f != cf ? GF_FIRST_REV : 0);
		e->key[1] = cl; e->val[1] = j << GF_VAL_SHIFT | GF_LAST | (l != cl ? GF_LAST_REV : 0);
		e->n_key = 2;
	}
	return 1;
}

/* ---- the end table ---- */
GF_FN uint64_t gf_hash(uint64_t x)
{
	x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
	x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
	return x ^ x >> 33;
}
/* the capacity for n_key keys: a power of two at least twice as many */
GF_FN uint64_t gf_capacity(uint64_t n_key)
{
	uint64_t cap = 16;
	while (cap < 2 * n_key) cap <<= 1;
	return cap;
}
/* claim a slot for key and store val beside it: at most cap slots are tried.  0; -1: no free slot; -2: the key is there already.  *probes = the
 * slots inspected.  cas(&word, expected, desired) returns what the word held */
template <class Cas> GF_FN int gf_claim(gf_slot_t *slots, uint64_t cap, uint64_t key, uint64_t val, Cas cas, uint64_t *probes)
{
	uint64_t i = gf_hash(key) & (cap - 1);
	for (uint64_t n = 1; n <= cap; ++n, i = (i + 1) & (cap - 1)) {
		const uint64_t old = cas(&slots[i].key, GF_EMPTY, key);
		*probes = n;
		if (old == GF_EMPTY) { slots[i].val = val; return 0; }
		if (old == key) return -2;
	}
	return -1;
}
/* 1 and *val when key is in the table, else 0: the walk ends at the key, at a free slot, or after cap slots */
GF_FN int gf_find(const gf_slot_t *slots, uint64_t cap, uint64_t key, uint64_t *val, uint64_t *probes)
{
	uint64_t i = gf_hash(key) & (cap - 1);
	for (uint64_t n = 1; n <= cap; ++n, i = (i + 1) & (cap - 1)) {
		const gf_slot_t s = slots[i];
		*probes = n;
		if (s.key == key) { *val = s.val; return 1; }
		if (s.key == GF_EMPTY) return 0;
	}
	return 0;
}

/* ---- the link of an end whose W is w through base b: 1 and *to = j' << 1 | (1 for '-'), or 0.  *probes is raised to the slots inspected; *bad
 * is raised for a value that names no unitig or that fits not exactly one orientation ---- */
GF_FN int gf_link(const gf_slot_t *slots, uint64_t cap, uint64_t w, int b, int k, uint64_t n_unitig, uint64_t *to, uint64_t *probes, uint64_t *bad)
{
	const uint64_t z = gf_extend(w, b, k), c = gf_canon(z, k);
	uint64_t val = 0, pr = 0;
	const int hit = gf_find(slots, cap, c, &val, &pr);
	if (pr > *probes) *probes = pr;
	if (!hit) return 0;
	const uint64_t jj = val >> GF_VAL_SHIFT;
	const int fwd = z == c;                                        /* Z is the node as stored */
	const int plus = (val & GF_FIRST) && fwd == !(val & GF_FIRST_REV);           /* the first k bases of S_j' are Z */
	const int minus = (val & GF_LAST) && fwd == !!(val & GF_LAST_REV);           /* ... of revcomp(S_j') */
	if (jj >= n_unitig || plus == minus) { ++*bad; return 0; }
	*to = jj << 1 | (uint64_t)(plus ? 0 : 1);
	return 1;
}
/* ---- the links of oriented end e = 2j + o whose W is w: bit b of the result is set iff base b gives a link, to to[b] (a cycle's end: bit 0, to
 * itself); their order in the list is that of b.  *open is set iff the end belongs to an open unitig and is tallied in end_deg ---- */
GF_FN unsigned gf_links(const gf_slot_t *slots, uint64_t cap, uint64_t w, uint64_t e, int k, uint64_t n_unitig, uint64_t to[4], int *open, uint64_t *probes,
                        uint64_t *bad)
{
	*open = 0;
	to[0] = to[1] = to[2] = to[3] = 0;
	if (w == GF_CYCLE) { to[0] = e; return 1u; }
	if (w == GF_BAD) return 0u;
	*open = 1;
	unsigned mask = 0;
	if (gf_link(slots, cap, w, 0, k, n_unitig, &to[0], probes, bad)) mask |= 1u;
	if (gf_link(slots, cap, w, 1, k, n_unitig, &to[1], probes, bad)) mask |= 2u;
	if (gf_link(slots, cap, w, 2, k, n_unitig, &to[2], probes, bad)) mask |= 4u;
	if (gf_link(slots, cap, w, 3, k, n_unitig, &to[3], probes, bad)) mask |= 8u;
	return mask;
}
#endif
