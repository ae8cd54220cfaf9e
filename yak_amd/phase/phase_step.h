/* phase_step.h -- the per-thread steps of the phasing of the bubbles' alleles from read support (`yak-amd bubbles -r -p`; include/yak_amd_phase.h;
 * DESIGN.md section 32).  No HIP in here, as in ../allele/allele_step.h: PH_FN is `__host__ __device__` under hipcc and empty otherwise, so that the
 * kernels of phase.hip and the sequential model of tools/phase_model_check.cpp (host compiler, sanitizers) call the very same functions.  The
 * atomics come in as functors: cas(p, expected, desired) returns what *p held, add(p, v), umax(p, v) and umin(p, v) change *p.
 *
 * An entry is seq << 32 | bubble << 1 | a, a pair's key i << 32 | j with i < j, its value cis << 32 | trans, the order's key of an edge
 * (w, i << 32 | j): the larger w first, then the smaller key.  comp[b] is the root of b's component and par[b] the parity of b against that root;
 * up[r] = parent << 1 | parity of a root against its parent, r << 1 for a root that stands.  Every index that comes from the caller's device data --
 * the bubble of a record -- is checked against its bound before it is used; what does not fit is counted in *bad and decides nothing. */
#ifndef YK_PHASE_STEP_H
#define YK_PHASE_STEP_H
#include <stdint.h>
#include "../allele/allele_step.h"

#define PH_FN AL_FN
#define PH_EMPTY (~(uint64_t)0)              /* the key of a free slot, the best key of a root without an edge */
#define PH_NONE (~(uint32_t)0)               /* the block of a bubble that is not het */
enum { PH_X = 1, PH_FOREST = 2, PH_DISC = 4 };       /* the bits of yakamd_pedge_t.flags */
enum { PH_CAP0 = 16 };                       /* the first capacity of the pair table */

typedef struct alignas(16) { uint64_t key, val; } ph_slot_t;
typedef struct alignas(16) { uint32_t i, j, cis, trans; } ph_pair_t;                               /* yakamd_ppair_t, include/yak_amd_phase.h */
typedef struct alignas(8)  { uint32_t block, flags; } ph_node_t;                                   /* yakamd_pnode_t */
typedef struct alignas(16) { uint32_t i, j, w, flags; } ph_edge_t;                                 /* yakamd_pedge_t */
typedef struct alignas(16) { uint32_t block, n_bubble, n_edge, n_disc; uint64_t w_sum, w_disc; } ph_block_t;      /* yakamd_pblock_t */

/* ---- step 1, record t of a feed: 1 iff it is a full observation.  A bubble outside the n_bubble, or a seq below that of the record before it,
 * is counted in *bad and is none ---- */
PH_FN int ph_full(const al_obs_t *obs, uint64_t t, uint64_t n_bubble, uint64_t *bad)
{
	const al_obs_t o = obs[t];
	if ((uint64_t)o.bubble >= n_bubble || (t && obs[t - 1].seq > o.seq)) { ++*bad; return 0; }
	return (o.flags & AL_FULL) != 0;
}
PH_FN uint64_t ph_entry(const al_obs_t *o) { return (uint64_t)o->seq << 32 | (uint64_t)o->bubble << 1 | (uint64_t)(o->flags & AL_A); }

/* ---- step 2, entry `cur` behind entry `prev`: 1 iff the two vote (one seq, two bubbles), then *key is the pair's and *inc what its value
 * grows by: cis in the upper word, trans in the lower ---- */
PH_FN int ph_vote(uint64_t prev, uint64_t cur, uint64_t *key, uint64_t *inc)
{
	const uint32_t b1 = (uint32_t)prev >> 1, b2 = (uint32_t)cur >> 1;
	if (prev >> 32 != cur >> 32 || b1 == b2) return 0;
	*key = b1 < b2 ? (uint64_t)b1 << 32 | b2 : (uint64_t)b2 << 32 | b1;
	*inc = ((prev ^ cur) & 1) ? 1 : (uint64_t)1 << 32;
	return 1;
}

/* ---- the pair table: open addressing, linear probing, a power of two of slots, at least twice the keys ---- */
PH_FN uint64_t ph_hash(uint64_t x)
{
	x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
	x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
	return x ^ x >> 33;
}
/* the capacity that holds n_key keys at half full or less, from `cap` upwards */
PH_FN uint64_t ph_capacity(uint64_t cap, uint64_t n_key)
{
	while (cap < 2 * n_key) cap <<= 1;
	return cap;
}
/* the slot of key, claimed if it has none yet: at most cap slots are tried.  The slot's index, *fresh = 1 iff this call claimed it; cap: no
 * free slot, which a table at half full or less never has */
template <class Cas> PH_FN uint64_t ph_claim(ph_slot_t *slots, uint64_t cap, uint64_t key, Cas cas, int *fresh)
{
	uint64_t s = ph_hash(key) & (cap - 1);
	*fresh = 0;
	for (uint64_t n = 0; n < cap; ++n, s = (s + 1) & (cap - 1)) {
		const uint64_t old = cas(&slots[s].key, PH_EMPTY, key);
		if (old == PH_EMPTY) { *fresh = 1; return s; }
		if (old == key) return s;
	}
	return cap;
}
/* a vote into the table: 0, 1 for the first vote of its pair; -1: no free slot, nothing is added */
template <class Cas, class Add> PH_FN int ph_add(ph_slot_t *slots, uint64_t cap, uint64_t key, uint64_t inc, Cas cas, Add add)
{
	int fresh;
	const uint64_t s = ph_claim(slots, cap, key, cas, &fresh);
	if (s >= cap) return -1;
	add(&slots[s].val, inc);
	return fresh;
}
/* a slot of the old table into the new, larger one: the keys are unique, so one claim and one plain store.  0; -1: no free slot or the key twice */
template <class Cas> PH_FN int ph_move(const ph_slot_t *old, uint64_t s, ph_slot_t *slots, uint64_t cap, Cas cas)
{
	const ph_slot_t v = old[s];
	int fresh;
	if (v.key == PH_EMPTY) return 0;
	const uint64_t at = ph_claim(slots, cap, v.key, cas, &fresh);
	if (at >= cap || !fresh) return -1;
	slots[at].val = v.val;
	return 0;
}
PH_FN int ph_pair(const ph_slot_t *slots, uint64_t s, ph_pair_t *p)
{
	const ph_slot_t v = slots[s];
	if (v.key == PH_EMPTY) return 0;
	p->i = (uint32_t)(v.key >> 32); p->j = (uint32_t)v.key; p->cis = (uint32_t)(v.val >> 32); p->trans = (uint32_t)v.val;
	return 1;
}

/* ---- step 3, the edge of slot s: both bubbles het at min_sup and |cis - trans| >= min_link.  The bubbles of a key are below n_bubble: ph_full()
 * has seen to it ---- */
PH_FN int ph_edge(const ph_slot_t *slots, uint64_t s, const al_sup_t *sup, uint64_t min_sup, uint64_t min_link, ph_edge_t *e)
{
	ph_pair_t p;
	if (!ph_pair(slots, s, &p)) return 0;
	if (al_call(&sup[p.i], min_sup) != 0 || al_call(&sup[p.j], min_sup) != 0) return 0;
	const uint32_t w = p.cis > p.trans ? p.cis - p.trans : p.trans - p.cis;
	if ((uint64_t)w < min_link) return 0;
	e->i = p.i; e->j = p.j; e->w = w; e->flags = p.trans > p.cis ? PH_X : 0;
	return 1;
}
PH_FN uint64_t ph_key(const ph_edge_t *e) { return (uint64_t)e->i << 32 | e->j; }

/* ---- a round of Boruvka's over the edges.  (a) an edge between two components offers its w to both roots: 1 iff it crosses ---- */
template <class Max> PH_FN int ph_best_w(const ph_edge_t *e, const uint32_t *comp, uint32_t *best_w, Max umax)
{
	const uint32_t ci = comp[e->i], cj = comp[e->j];
	if (ci == cj) return 0;
	umax(best_w + ci, e->w); umax(best_w + cj, e->w);
	return 1;
}
/* (b) among the edges that reach a root's best w, the smallest key */
template <class Min> PH_FN void ph_best_key(const ph_edge_t *e, const uint32_t *comp, const uint32_t *best_w, uint64_t *best_k, Min umin)
{
	const uint32_t ci = comp[e->i], cj = comp[e->j];
	if (ci == cj) return;
	if (best_w[ci] == e->w) umin(best_k + ci, ph_key(e));
	if (best_w[cj] == e->w) umin(best_k + cj, ph_key(e));
}
/* (c) the edge a root chose is a forest edge, and the choosing root hooks under the other with the parity of the two roots against each other;
 * where both chose it, the larger root alone.  A root chooses one edge, so up[] of a root has one writer.  1 iff the edge joins the forest */
PH_FN int ph_hook(ph_edge_t *e, const uint32_t *comp, const uint8_t *par, const uint32_t *best_w, const uint64_t *best_k, uint64_t *up)
{
	const uint32_t ci = comp[e->i], cj = comp[e->j];
	if (ci == cj) return 0;
	const uint64_t key = ph_key(e);
	const int by_i = best_w[ci] == e->w && best_k[ci] == key, by_j = best_w[cj] == e->w && best_k[cj] == key;
	if (!by_i && !by_j) return 0;
	const uint64_t x = (uint64_t)((par[e->i] ^ par[e->j] ^ (e->flags & PH_X)) & 1);
	if (by_i && (!by_j || ci > cj)) up[ci] = (uint64_t)cj << 1 | x;
	if (by_j && (!by_i || cj > ci)) up[cj] = (uint64_t)ci << 1 | x;
	e->flags |= PH_FOREST;
	return 1;
}
/* (d) pointer doubling with parity for root r: (parent, parity) becomes (what the parent points to, the two parities joined) until the parent
 * stands, and up[r] is stored once.  A word of up[] is read and written whole, and every value it ever holds names an ancestor with the parity
 * against it, so the doubling of other roots may fall between, and an older value read for a newer only costs steps: the result is the root that
 * stands and the parity against it, whatever the timing.  The thread's own word stays in a register: nothing waits for a store to be seen */
PH_FN void ph_flatten(volatile uint64_t *up, uint32_t r)
{
	uint64_t u = up[r];
	for (;;) {
		const uint64_t g = up[u >> 1];
		if (g >> 1 == u >> 1) break;
		u = (g & ~(uint64_t)1) | ((u ^ g) & 1);
	}
	up[r] = u;
}
/* (e) bubble b under the root its root hangs under now */
PH_FN void ph_rewrite(uint32_t b, uint32_t *comp, uint8_t *par, const uint64_t *up)
{
	const uint64_t u = up[comp[b]];
	comp[b] = (uint32_t)(u >> 1); par[b] ^= (uint8_t)(u & 1);
}

/* ---- step 4: the node of bubble b whose block is named `name` (the smallest bubble of its component), and a non-forest edge's concordance ---- */
PH_FN ph_node_t ph_node(uint32_t b, int het, uint32_t name, const uint8_t *par)
{
	ph_node_t n;
	n.block = het ? name : PH_NONE; n.flags = het ? (uint32_t)((par[b] ^ par[name]) & 1) : 0;
	return n;
}
PH_FN int ph_discordant(const ph_edge_t *e, const ph_node_t *node)
{
	return !(e->flags & PH_FOREST) && (e->flags & PH_X) != ((node[e->i].flags ^ node[e->j].flags) & 1);
}
#endif
