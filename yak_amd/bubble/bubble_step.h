/* bubble_step.h -- the per-thread steps of the simple bubbles of the unitig graph (`yak-amd bubbles`; include/yak_amd_bubble.h; DESIGN.md section
 * 26).  No HIP in here, as in ../gfa/gfa_step.h: BB_FN is `__host__ __device__` under hipcc and empty otherwise, so that the kernels of bubble.hip
 * and the sequential model of tests/tools/bubble_model_check.cpp (host compiler, sanitizers) call the very same functions.
 *
 * An oriented end is e = j << 1 | o.  The links of the list are sorted by `from`, so those of an end are one run: runs[e] = (the index of its first
 * link, their number), first == BB_NONE for an end without a link.  Every index that comes from device data -- an end named by a link, a run, a
 * rank, an offset into the bases -- is checked against its bound before it is used; what does not fit is counted in *bad and decides nothing. */
#ifndef YK_BUBBLE_STEP_H
#define YK_BUBBLE_STEP_H
#include <stdint.h>

#if defined(__HIPCC__)
#define BB_FN __host__ __device__ static inline
#else
#define BB_FN static inline
#endif

#define BB_NONE (~(uint64_t)0)               /* runs[e].first of an end without a link; hd of arms of two lengths */
enum { BB_S = 0, BB_E = 1, BB_I = 2 };       /* YAKAMD_BUBBLE_*, include/yak_amd_bubble.h */
enum { BB_FORK = 1, BB_TIP = 2 };            /* what bb_find() says of an end beside the bubble */

typedef struct alignas(16) { uint64_t off, n_node, kc, first; } bb_desc_t;     /* yakamd_udesc_t, include/yak_amd_walk.h: two 16-byte loads */
typedef struct alignas(16) { uint64_t from, to; } bb_link_t;                   /* yakamd_ulink_t, include/yak_amd_gfa.h: one */
typedef struct alignas(16) { uint64_t first, n; } bb_run_t;                    /* links[first .. first + n) are those of an end */
typedef struct alignas(16) { uint64_t src, sink, arm[2], n_node[2], kc[2], hd, type; } bb_rec_t;   /* yakamd_bubble_t, include/yak_amd_bubble.h */

/* ---- step 1, link i of the n_link of the list: 0: it stands inside a run; 1: it opens the run of end *e, *run is what runs[*e] becomes; -1: the
 * list does not fit -- `from` falls below the link before, `from` or `to` names no end of the n_end, or the run has more than 4 links ---- */
BB_FN int bb_first(const bb_link_t *links, uint64_t n_link, uint64_t i, uint64_t n_end, uint64_t *e, bb_run_t *run)
{
	const bb_link_t l = links[i];
	if (l.from >= n_end || l.to >= n_end) return -1;
	if (i > 0) {
		const uint64_t before = links[i - 1].from;
		if (before > l.from) return -1;
		if (before == l.from) return 0;
	}
	uint64_t n = 1;
	while (n < 5 && n < n_link - i && links[i + n].from == l.from) ++n;
	if (n > 4) return -1;
	*e = l.from;
	run->first = i; run->n = n;
	return 1;
}

/* the run of end e, checked: 0 and *out (n == 0 for an end without a link), or -1 */
BB_FN int bb_run_of(const bb_run_t *runs, uint64_t n_end, uint64_t n_link, uint64_t e, bb_run_t *out)
{
	out->first = 0; out->n = 0;
	if (e >= n_end) return -1;
	const bb_run_t r = runs[e];
	if (r.first == BB_NONE) return 0;
	if (r.n < 1 || r.n > 4 || r.first >= n_link || r.n > n_link - r.first) return -1;
	*out = r;
	return 0;
}
/* link i of the run of end e: 0 and *to, or -1 when it is not a link of e or leads to no end */
BB_FN int bb_to(const bb_link_t *links, uint64_t n_end, uint64_t i, uint64_t e, uint64_t *to)
{
	const bb_link_t l = links[i];
	if (l.from != e || l.to >= n_end) return -1;
	*to = l.to;
	return 0;
}

/* ---- step 2, oriented end s < 2 n_unitig: 1 iff s is the source of a simple bubble and the side that reports it; then src, sink, arm, n_node and
 * kc of *r are filled.  *flags: BB_FORK for an end of an open unitig with two links or more, BB_TIP (and *tip_nodes) at the '+' end of a tip.
 * The definition costs two loads of a descriptor, seven of a run and four of a link, the record two descriptors more ---- */
BB_FN int bb_find(const bb_desc_t *desc, uint64_t n_unitig, const bb_run_t *runs, const bb_link_t *links, uint64_t n_link, uint64_t s, int k, bb_rec_t *r,
                  unsigned *flags, uint64_t *tip_nodes, uint64_t *bad)
{
	const uint64_t n_end = 2 * n_unitig;
	*flags = 0; *tip_nodes = 0;
	const bb_desc_t u = desc[s >> 1];
	if (u.first & 1) return 0;                                     /* a cycle: its ends are no source, no fork and no tip */
	bb_run_t rs, rx;
	if (bb_run_of(runs, n_end, n_link, s, &rs) != 0) { ++*bad; return 0; }
	if (rs.n >= 2) *flags |= BB_FORK;
	if (!(s & 1) && u.n_node < (uint64_t)k) {                      /* the '+' end speaks for the unitig */
		if (bb_run_of(runs, n_end, n_link, s ^ 1, &rx) != 0) { ++*bad; return 0; }
		if ((rs.n == 0) != (rx.n == 0)) { *flags |= BB_TIP; *tip_nodes = u.n_node; }
	}
	if (rs.n != 2) return 0;
	uint64_t a[2], t[2];
	if (bb_to(links, n_end, rs.first, s, &a[0]) != 0 || bb_to(links, n_end, rs.first + 1, s, &a[1]) != 0) { ++*bad; return 0; }
	if (a[0] >> 1 == a[1] >> 1 || a[0] >> 1 == s >> 1 || a[1] >> 1 == s >> 1) return 0;
	for (int i = 0; i < 2; ++i) {
		bb_run_t in, out;
		if (bb_run_of(runs, n_end, n_link, a[i] ^ 1, &in) != 0 || bb_run_of(runs, n_end, n_link, a[i], &out) != 0) { ++*bad; return 0; }
		if (in.n != 1 || out.n != 1) return 0;
		if (bb_to(links, n_end, out.first, a[i], &t[i]) != 0) { ++*bad; return 0; }
	}
	if (t[0] != t[1] || t[0] >> 1 == a[0] >> 1 || t[0] >> 1 == a[1] >> 1) return 0;
	if (bb_run_of(runs, n_end, n_link, t[0] ^ 1, &rx) != 0) { ++*bad; return 0; }
	if (rx.n != 2 || !(s < (t[0] ^ 1))) return 0;                  /* the other side reports it */
	const bb_desc_t d0 = desc[a[0] >> 1], d1 = desc[a[1] >> 1];
	r->src = s; r->sink = t[0];
	r->arm[0] = a[0]; r->arm[1] = a[1];
	r->n_node[0] = d0.n_node; r->n_node[1] = d1.n_node;
	r->kc[0] = d0.kc; r->kc[1] = d1.kc;
	return 1;
}

/* ---- step 3 ---- */
BB_FN uint64_t bb_type(uint64_t n1, uint64_t n2, int k) { return n1 != n2 ? BB_I : n1 == (uint64_t)k ? BB_S : BB_E; }
/* where the n_node + k - 1 bases of oriented arm a stand: 0 and *off, *len, or -1 when a names no unitig, its descriptor has another n_node than
 * the record or does not lie inside the n_bases bases */
BB_FN int bb_arm(const bb_desc_t *desc, uint64_t n_unitig, uint64_t n_bases, uint64_t a, uint64_t n_node, int k, uint64_t *off, uint64_t *len)
{
	if (a >> 1 >= n_unitig) return -1;
	const bb_desc_t u = desc[a >> 1];
	if (u.n_node != n_node || u.n_node < 1 || u.off > n_bases || u.n_node > n_bases - u.off || (uint64_t)(k - 1) > n_bases - u.off - u.n_node) return -1;
	*off = u.off; *len = u.n_node + (uint64_t)(k - 1);
	return 0;
}
/* base p of the oriented string of an arm, A C G T = 0 1 2 3: a '-' arm is read backwards and complemented.  -1 for a byte that is none of ACGT */
BB_FN int bb_base(const char *bases, uint64_t off, uint64_t len, int minus, uint64_t p)
{
	const unsigned c = (unsigned char)bases[minus ? off + len - 1 - p : off + p];
	if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return -1;
	const int b = (int)((c >> 1 ^ c >> 2) & 3u);
	return minus ? 3 - b : b;
}
/* position p of two arms of one length: 1 for a mismatch, 0 for a match, -1 for a byte that is no base */
BB_FN int bb_mismatch(const char *bases, const uint64_t off[2], uint64_t len, const uint64_t arm[2], uint64_t p)
{
	const int x = bb_base(bases, off[0], len, (int)(arm[0] & 1), p), y = bb_base(bases, off[1], len, (int)(arm[1] & 1), p);
	return x < 0 || y < 0 ? -1 : x != y;
}
#endif
