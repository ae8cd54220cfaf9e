/* uwalk_step.h -- the per-state steps of the device walk of `yak-amd unitigs -g`: list ranking by pointer doubling over the
 * links of the records yakamd_graph_nodes_dev() writes.  No HIP in here, as in replay_plan.h: UW_FN is `__host__ __device__` under hipcc and empty
 * otherwise, so that the kernels of walk.hip and the sequential model of tests/tools/uwalk_model_check.cpp (host compiler, sanitizers) call the very
 * same functions.
 *
 * A traversal state (v, d) of DESIGN.md section 20 is the number s = 2v + d.  succ(s) follows link[d] of v to (u, t) and is the state (u, t ^ 1);
 * a state whose side has no link is terminal.  Links are symmetric, so the states form disjoint paths and cycles, every unitig once in each
 * direction.  A state's pair is (ptr, dist): the state `dist` steps ahead; UW_DONE in ptr says that this state is the terminal of the chain, which
 * then absorbs.  A key that is no node has UW_DEAD in both of its pairs. */
#ifndef YK_UWALK_STEP_H
#define YK_UWALK_STEP_H
#include <stdint.h>

#if defined(__HIPCC__)
#define UW_FN __host__ __device__ static inline
#else
#define UW_FN static inline
#endif

#define UW_NONE (~(uint64_t)0)
#define UW_DONE ((uint64_t)1 << 63)          /* in ptr: the state named is the terminal of the chain */
#define UW_DEAD (~(uint64_t)0)               /* ptr of a key that is no node */

typedef struct { uint64_t x, link[2]; uint32_t count, edges; } uw_node_t;     /* yakamd_gnode_t, include/yak_amd.h */
typedef struct { uint64_t ptr, dist; } uw_pair_t;
/* what a node knows after the ranking: the start node of its unitig (UW_NONE on a cycle), p << 1 | d of its place in it, the unitig's nodes */
typedef struct { uint64_t start, at, n_node; } uw_place_t;

/* the results (yakamd_umap_t and yakamd_udesc_t, include/yak_amd_walk.h) */
typedef struct { uint64_t unitig, at; } uw_map_t;
typedef struct { uint64_t off, n_node, kc, first; } uw_desc_t;

/* ---- state coding ---- */
UW_FN uint64_t uw_state(uint64_t v, int d) { return v << 1 | (uint64_t)d; }
UW_FN uint64_t uw_state_node(uint64_t s) { return s >> 1; }
UW_FN int uw_is_node(const uw_node_t *r, uint32_t min_cnt) { return r->count >= min_cnt; }
UW_FN int uw_done(uw_pair_t p) { return p.ptr != UW_DEAD && (p.ptr & UW_DONE) != 0; }
UW_FN int uw_dead(uw_pair_t p) { return p.ptr == UW_DEAD; }

/* ---- init from a record: the pair of state (v, d) before the first round ---- */
UW_FN uw_pair_t uw_init(const uw_node_t *r, uint64_t v, int d, uint32_t min_cnt)
{
	uw_pair_t p;
	if (!uw_is_node(r, min_cnt)) { p.ptr = UW_DEAD; p.dist = 0; return p; }
	const uint64_t lk = r->link[d];
	if (lk == UW_NONE) { p.ptr = uw_state(v, d) | UW_DONE; p.dist = 0; return p; }
	p.ptr = lk ^ 1;                            /* (u, t) -> the state (u, t ^ 1) */
	p.dist = 1;
	return p;
}

/* ---- one jump ---- */
/* the state whose pair this one reads in a round, or UW_NONE: a key that is no node, a finished state, a link that leads out of the n_state states */
UW_FN uint64_t uw_target(uw_pair_t p, uint64_t n_state) { return uw_dead(p) || (p.ptr & UW_DONE) || p.ptr >= n_state ? UW_NONE : p.ptr; }
/* the pair of a state after a round, from its own pair p and the pair q of its target (both of the round before); *finished is set iff the state
 * reached its terminal in this round */
UW_FN uw_pair_t uw_jump(uw_pair_t p, uw_pair_t q, int *finished)
{
	uw_pair_t o;
	*finished = 0;
	if (uw_dead(q)) return p;                  /* a link into a key that is no node: the state stays where it is and is reported as a cycle */
	o.ptr = q.ptr;
	o.dist = p.dist + q.dist;
	*finished = (q.ptr & UW_DONE) != 0;
	return o;
}

/* ---- the orientation / position decision of node v from the final pairs a = (v, 0) and b = (v, 1).  1: on an open unitig, *w filled; 0: on a
 * cycle (neither state reached a terminal); -1: the links are broken (one state ended and the other did not, or both ends are the same other
 * node) ---- */
UW_FN int uw_decide(uint64_t v, uw_pair_t a, uw_pair_t b, uw_place_t *w)
{
	const int da = uw_done(a), db = uw_done(b);
	if (!da && !db) { w->start = UW_NONE; w->at = 0; w->n_node = 0; return 0; }
	if (da != db) return -1;
	const uint64_t e0 = uw_state_node(a.ptr & ~UW_DONE), r0 = a.dist, e1 = uw_state_node(b.ptr & ~UW_DONE), r1 = b.dist;
	w->n_node = r0 + r1 + 1;
	if (e1 < e0) { w->start = e1; w->at = r1 << 1 | 0; return 1; }          /* the unitig comes from e1 and passes v as stored */
	if (e0 < e1) { w->start = e0; w->at = r0 << 1 | 1; return 1; }          /* it comes from e0 and passes v reverse-complemented */
	if (e0 != v || r0 != 0 || r1 != 0) return -1;
	w->start = v; w->at = 0;                                                  /* a node without a link: as stored */
	return 1;
}

/* ---- the bases of a node as read ---- */
/* the last base of x read in direction d */
UW_FN char uw_last_base(uint64_t x, int d, int k) { return "ACGT"[d == 0 ? x & 3 : 3 - (x >> 2 * (k - 1) & 3)]; }
/* base i (0 = first) of the k bases of x read in direction d */
UW_FN char uw_base_at(uint64_t x, int d, int k, int i)
{
	return "ACGT"[d == 0 ? x >> 2 * (k - 1 - i) & 3 : 3 - (x >> 2 * i & 3)];
}
#endif
