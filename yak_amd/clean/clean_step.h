/* clean_step.h -- the per-thread steps of the cleaning of the unitig graph (`yak-amd clean`; include/yak_amd_clean.h).  No HIP
 * in here, as in ../bubble/bubble_step.h, whose records, runs and checked reads it uses: CL_FN is `__host__ __device__` under hipcc and empty
 * otherwise, so that the kernels of clean.hip and the sequential model of tests/tools/clean_model_check.cpp (host compiler, sanitizers) call the
 * very same functions.
 *
 * Every index that comes from device data -- an end named by a link, a run, an arm of a bubble record, a rank, an offset into the bases or the
 * image -- is checked against its bound before it is used; what does not fit is counted in *bad and decides nothing. */
#ifndef YK_CLEAN_STEP_H
#define YK_CLEAN_STEP_H
#include <stdint.h>
#include "../bubble/bubble_step.h"

#define CL_FN BB_FN

enum { CL_KEEP = 0, CL_TIP = 1, CL_POP = 2 };                                  /* YAKAMD_CLEAN_*, include/yak_amd_clean.h */
typedef struct alignas(16) { uint64_t unitig, why, n_node, kc, other, off; } cl_rec_t;   /* yakamd_clean_rec_t: three 16-byte stores */

/* ---- the coverage order: exact, in 128 bits and, behind the factor of pop_pct, in 192 ---- */
CL_FN void cl_mul(uint64_t a, uint64_t b, uint64_t *hi, uint64_t *lo)
{
#if defined(__HIP_DEVICE_COMPILE__)
	*hi = __umul64hi(a, b); *lo = a * b;
#else
	const unsigned __int128 p = (unsigned __int128)a * b;
	*hi = (uint64_t)(p >> 64); *lo = (uint64_t)p;
#endif
}
/* the sign of kc_a n_b - kc_b n_a: above 0 iff a has the higher coverage */
CL_FN int cl_cov_cmp(uint64_t kc_a, uint64_t n_a, uint64_t kc_b, uint64_t n_b)
{
	uint64_t ah, al, bh, bl;
	cl_mul(kc_a, n_b, &ah, &al);
	cl_mul(kc_b, n_a, &bh, &bl);
	return ah != bh ? (ah > bh ? 1 : -1) : al != bl ? (al > bl ? 1 : -1) : 0;
}
CL_FN int cl_stronger(uint64_t ja, uint64_t kc_a, uint64_t n_a, uint64_t jb, uint64_t kc_b, uint64_t n_b)
{
	const int c = cl_cov_cmp(kc_a, n_a, kc_b, n_b);
	return c > 0 || (c == 0 && ja < jb);
}
/* (hi, lo) m as three words, *w0 the highest */
CL_FN void cl_mul3(uint64_t hi, uint64_t lo, uint64_t m, uint64_t *w0, uint64_t *w1, uint64_t *w2)
{
	uint64_t lh, ll, hh, hl;
	cl_mul(lo, m, &lh, &ll);
	cl_mul(hi, m, &hh, &hl);
	*w2 = ll;
	*w1 = hl + lh;
	*w0 = hh + (*w1 < hl ? 1 : 0);
}
/* 100 kc_lo n_hi <= pct kc_hi n_lo */
CL_FN int cl_pop_rule(uint64_t kc_lo, uint64_t n_lo, uint64_t kc_hi, uint64_t n_hi, uint64_t pct)
{
	uint64_t ah, al, bh, bl, a0, a1, a2, b0, b1, b2;
	cl_mul(kc_lo, n_hi, &ah, &al);
	cl_mul(kc_hi, n_lo, &bh, &bl);
	cl_mul3(ah, al, 100, &a0, &a1, &a2);
	cl_mul3(bh, bl, pct, &b0, &b1, &b2);
	return a0 != b0 ? a0 < b0 : a1 != b1 ? a1 < b1 : a2 <= b2;
}

/* ---- step 2, the tips ---- */
/* tipcand(e) of oriented end e < n_end: 1, 0, or -1 for a run that does not fit.  *u is the descriptor of e >> 1 */
CL_FN int cl_tipcand(const bb_desc_t *desc, const bb_run_t *runs, uint64_t n_end, uint64_t n_link, uint64_t e, uint64_t tip_nodes, bb_desc_t *u)
{
	bb_run_t re, rx;
	*u = desc[e >> 1];
	if (bb_run_of(runs, n_end, n_link, e, &re) != 0 || bb_run_of(runs, n_end, n_link, e ^ 1, &rx) != 0) return -1;
	return !(u->first & 1) && u->n_node < tip_nodes && re.n == 1 && rx.n == 0;
}
/* unitig j < n_unitig: CL_TIP iff it is clipped, else CL_KEEP; *cand = 1 iff one of its ends is a tip candidate, *other = the anchor end a then */
CL_FN int cl_tip(const bb_desc_t *desc, uint64_t n_unitig, const bb_run_t *runs, const bb_link_t *links, uint64_t n_link, uint64_t j, uint64_t tip_nodes,
                 uint64_t *other, int *cand, bb_desc_t *u, uint64_t *bad)
{
	const uint64_t n_end = 2 * n_unitig;
	*cand = 0; *other = BB_NONE;
	int c0 = cl_tipcand(desc, runs, n_end, n_link, j << 1, tip_nodes, u);
	if (c0 < 0) { ++*bad; return CL_KEEP; }
	if ((u->first & 1) || u->n_node >= tip_nodes) return CL_KEEP;
	uint64_t e = j << 1;
	if (!c0) {
		bb_desc_t again;
		e |= 1;
		c0 = cl_tipcand(desc, runs, n_end, n_link, e, tip_nodes, &again);
		if (c0 < 0) { ++*bad; return CL_KEEP; }
		if (!c0) return CL_KEEP;
	}
	*cand = 1;
	bb_run_t re, ra;
	uint64_t a;
	if (bb_run_of(runs, n_end, n_link, e, &re) != 0 || re.n != 1 || bb_to(links, n_end, re.first, e, &a) != 0) { ++*bad; return CL_KEEP; }
	*other = a;
	if (a >> 1 == j) return CL_KEEP;
	if (bb_run_of(runs, n_end, n_link, a ^ 1, &ra) != 0) { ++*bad; return CL_KEEP; }
	int clip = 0, mirror = 0;
	for (uint64_t i = 0; i < ra.n; ++i) {                              /* at most four: the run was checked */
		uint64_t x;
		if (bb_to(links, n_end, ra.first + i, a ^ 1, &x) != 0) { ++*bad; return CL_KEEP; }
		if (x == (e ^ 1)) { mirror = 1; continue; }
		bb_desc_t ux;
		const int cx = cl_tipcand(desc, runs, n_end, n_link, x ^ 1, tip_nodes, &ux);
		if (cx < 0) { ++*bad; return CL_KEEP; }
		if (!cx || cl_stronger(x >> 1, ux.kc, ux.n_node, j, u->kc, u->n_node)) clip = 1;
	}
	if (!mirror) { ++*bad; return CL_KEEP; }                           /* a link without its mirror: the list is not one of this graph */
	return clip ? CL_TIP : CL_KEEP;
}

/* ---- step 3, a bubble record: 1 iff its loser is popped; *lo, *hi the losing and the winning arm's end, *n_lo, *kc_lo the loser's.  -1 for an
 * arm outside the unitigs, a cycle, or one whose descriptor says another n_node or kc than the record ---- */
CL_FN int cl_pop(const bb_rec_t *r, const bb_desc_t *desc, uint64_t n_unitig, uint64_t pop_pct, uint64_t *lo, uint64_t *hi, uint64_t *n_lo, uint64_t *kc_lo)
{
	const uint64_t a0 = r->arm[0], a1 = r->arm[1], n0 = r->n_node[0], n1 = r->n_node[1], c0 = r->kc[0], c1 = r->kc[1];
	if (a0 >> 1 >= n_unitig || a1 >> 1 >= n_unitig || a0 >> 1 == a1 >> 1) return -1;
	const bb_desc_t u0 = desc[a0 >> 1], u1 = desc[a1 >> 1];
	if ((u0.first & 1) || u0.n_node != n0 || u0.kc != c0 || n0 < 1 || c0 < 1) return -1;
	if ((u1.first & 1) || u1.n_node != n1 || u1.kc != c1 || n1 < 1 || c1 < 1) return -1;
	const int first_wins = cl_cov_cmp(c0, n0, c1, n1) >= 0;
	*lo = first_wins ? a1 : a0; *hi = first_wins ? a0 : a1;
	*n_lo = first_wins ? n1 : n0; *kc_lo = first_wins ? c1 : c0;
	return pop_pct > 0 && cl_pop_rule(*kc_lo, *n_lo, first_wins ? c0 : c1, first_wins ? n0 : n1, pop_pct);
}

/* ---- step 5, where the n_node + k - 1 bases of record r stand and where they go: 0 and *src, *len, or -1 when the record names no unitig, has
 * another n_node than the descriptor, or either span leaves its array (the image takes len + 1 bytes at r->off) ---- */
CL_FN int cl_span(const cl_rec_t *r, const bb_desc_t *desc, uint64_t n_unitig, uint64_t n_bases, uint64_t img_bytes, int k, uint64_t *src, uint64_t *len)
{
	if (r->unitig >= n_unitig) return -1;
	if (bb_arm(desc, n_unitig, n_bases, r->unitig << 1, r->n_node, k, src, len) != 0) return -1;
	if (r->off > img_bytes || *len + 1 > img_bytes - r->off) return -1;
	return 0;
}
#endif
