/*
 * phase.hip -- libyak_amd_phase.so: the alleles of the simple bubbles phased from read support on the GPU (include/yak_amd_phase.h; DESIGN.md
 * section 32).  A layer above libyak_amd_allele.so and the libraries below that: it calls their public functions only (what yakamd_alleles() calls,
 * and yakamd_allele_open / _obs_dev / _support_dev / _close) and owns its device memory (hipMalloc / hipFree).  The per-thread steps are those of
 * phase_step.h, the texts those of phase_text.h, the reader and the chunk loop those of ../layer/layer_seqs.h; every launch goes through YK_LAUNCH
 * of ../csrc/tally.h into this library's own tally (yakamd_phase_tally_*).  The host scaffolding and the scan are those of ../layer/layer_host.h and
 * ../layer/layer_dev.h, which the layers share.
 *
 *   k_ph_full<COUNT>   a thread per record: the bubble against n_bubble, the seq against the record before; cnt[t] = (is a full one)
 *   k_ph_tile_sum, k_ph_tile_scan, k_ph_scan_apply
 *                      the exclusive scan of cnt[] in place: tiles of 1024, their sums scanned by one workgroup; every compaction here uses it
 *   k_ph_full<EMIT>    a full record writes its entry seq << 32 | bubble << 1 | a at its rank
 *   k_ph_clear         a new table: every key all ones, every value 0, one 16-byte store per slot
 *   k_ph_rehash        a thread per slot of the old table: one claim and one plain store in the new one
 *   k_ph_vote          a thread per entry, against the entry before it: the pair's key claimed by a 64-bit compare-and-swap from all ones, its
 *                      value cis << 32 | trans raised by one 64-bit atomic add; the votes and the new keys summed per wave, then per
 *                      workgroup in LDS: one global atomic per workgroup of a grid of 2048 at the most
 *   k_ph_pairs<MODE>   the voted pairs compacted out of the slots, for yakamd_phase_pairs_dev()
 *   k_ph_edges<MODE>   the edges compacted out of the slots and the support
 *   k_ph_init          comp[b] = b, par[b] = 0, up[b] = b << 1, best[] and name[] empty, the block tallies 0
 *   k_ph_best_w, k_ph_best_key, k_ph_hook, k_ph_flatten, k_ph_rewrite
 *                      a round of Boruvka's: atomicMax of w per root and a flag set if an edge crosses, atomicMin of i << 32 | j among the edges
 *                      that reach it, the chosen edges marked and their roots hooked, the hooks doubled with parity, comp[] and par[] rewritten
 *   k_ph_name, k_ph_nodes, k_ph_classify, k_ph_blocks<MODE>
 *                      atomicMin of b per root; the node records and n_bubble per block; bit 2 of the non-forest edges and the block tallies by
 *                      64-bit atomics; the blocks of two or more compacted
 * All sums are integer sums and all minima and maxima are of a strict order, so nothing depends on the order of the threads; all stores are
 * vector stores.
 */
#include "yak.h"
#include "yak_amd_phase.h"
#define LAYER_NAME "phase"
#include "../layer/layer_host.h"
#include "../layer/layer_seqs.h"
#include "../layer/layer_dev.h"
#include "phase_step.h"
#include "phase_text.h"

static_assert(sizeof(yakamd_ppair_t) == 16 && sizeof(ph_pair_t) == 16 && sizeof(yakamd_pnode_t) == 8 && sizeof(ph_node_t) == 8, "the records as declared");
static_assert(sizeof(yakamd_pedge_t) == 16 && sizeof(ph_edge_t) == 16 && sizeof(yakamd_pblock_t) == 32 && sizeof(ph_block_t) == 32 && sizeof(yakamd_phopt_t) == 32, "the records as declared");
static_assert(sizeof(yakamd_aobs_t) == sizeof(al_obs_t) && sizeof(yakamd_asup_t) == sizeof(al_sup_t) && sizeof(yakamd_bubble_t) == sizeof(bb_rec_t), "the records of the layers below");
static_assert(YAKAMD_PEDGE_X == PH_X && YAKAMD_PEDGE_FOREST == PH_FOREST && YAKAMD_PEDGE_DISC == PH_DISC, "the flags as declared");

namespace {

enum { PH_THREADS = 256, PH_ITEMS = 4, PH_TILE = PH_THREADS * PH_ITEMS, PH_WAVE = 64, PH_MAX_ROUND = 40 };
/* the words of stat[]: what does not fit (a record of k_ph_full, a vote or a slot without a free slot), the votes of k_ph_vote with its new keys
 * from bit 32, the forest edges, the het bubbles, the blocks of one; then per round 1 iff an edge crossed */
enum { PHS_BAD = 0, PHS_NOSLOT = 1, PHS_VOTE = 2, PHS_FOREST = 3, PHS_HET = 4, PHS_SINGLE = 5, PHS_CROSS = 8, PHS_N = PHS_CROSS + PH_MAX_ROUND };
enum PhMode { COUNT = 0, EMIT = 1 };

struct DevAdd64 { __device__ void operator()(uint64_t *p, uint64_t v) const { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); } };
struct DevMax32 { __device__ void operator()(uint32_t *p, uint32_t v) const { atomicMax(reinterpret_cast<unsigned*>(p), (unsigned)v); } };
struct DevMin64 { __device__ void operator()(uint64_t *p, uint64_t v) const { atomicMin(reinterpret_cast<u64*>(p), (u64)v); } };

/* a wave's sum into a word of stat[]: one atomic per wave that has something.  For what is nearly always 0 -- the misfits -- and for short grids */
__device__ inline void tally(u64 v, u64 *stat, int at)
{
	v = wave_sum(v);
	if ((threadIdx.x & (PH_WAVE - 1)) == 0 && v) atomicAdd(stat + at, v);
}
/* the same for a sum that every wave has: the waves' sums meet in a word of LDS, which the workgroup has set to 0 and synchronised on, and one
 * global atomic per workgroup carries it on.  Every wave of a launch adding to one word of stat[] by itself was most of the run time of
 * k_ph_full<COUNT> and k_ph_vote when they were first measured (profiles/phase_pmc_atomics.txt): atomics on one address go through the L2 one by one */
__device__ inline void tally_wg(u64 v, u64 *s_sum, u64 *stat, int at)
{
	v = wave_sum(v);
	if ((threadIdx.x & (PH_WAVE - 1)) == 0 && v) atomicAdd(s_sum, v);
	__syncthreads();
	if (threadIdx.x == 0 && *s_sum) atomicAdd(stat + at, *s_sum);
}

template<int MODE> __global__ __launch_bounds__(PH_THREADS)
void k_ph_full(const al_obs_t *__restrict__ obs, u64 n_obs, u64 n_bubble, u64 *__restrict__ cnt, uint64_t *__restrict__ ent, u64 n_full, u64 *stat)
{
	const u64 t = (u64)blockIdx.x * PH_THREADS + threadIdx.x;
	u64 bad = 0;
	if (t < n_obs) {
		uint64_t bd = 0;
		const u64 full = (u64)ph_full(obs, t, n_bubble, &bd);
		bad = bd;
		if (MODE == COUNT) cnt[t] = full;
		else if (full) {
			const u64 at = cnt[t];
			if (at >= n_full) ++bad;                                       /* a rank outside the list: tallied, not written */
			else { const al_obs_t o = obs[t]; ent[at] = ph_entry(&o); }
		}
	}
	tally(bad, stat, PHS_BAD);
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_tile_sum(const u64 *__restrict__ cnt, u64 n, u64 *__restrict__ tsum) { tile_sum<PH_THREADS, PH_ITEMS, u64, AddU64>(cnt, n, tsum); }
__global__ __launch_bounds__(PH_THREADS)
void k_ph_tile_scan(u64 *__restrict__ tsum, u64 m) { tile_scan<PH_THREADS, u64, AddU64>(tsum, m); }
__global__ __launch_bounds__(PH_THREADS)
void k_ph_scan_apply(u64 *__restrict__ cnt, u64 n, const u64 *__restrict__ tsum) { scan_apply<PH_THREADS, PH_ITEMS, u64, AddU64>(cnt, n, tsum); }

__global__ __launch_bounds__(PH_THREADS)
void k_ph_clear(ph_slot_t *__restrict__ slots, u64 cap)
{
	for (u64 s = (u64)blockIdx.x * PH_THREADS + threadIdx.x; s < cap; s += (u64)gridDim.x * PH_THREADS)
		*reinterpret_cast<v2*>(slots + s) = make_ulonglong2(PH_EMPTY, 0);
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_rehash(const ph_slot_t *__restrict__ old, u64 old_cap, ph_slot_t *slots, u64 cap, u64 *stat)
{
	u64 bad = 0;
	for (u64 s = (u64)blockIdx.x * PH_THREADS + threadIdx.x; s < old_cap; s += (u64)gridDim.x * PH_THREADS)
		bad += ph_move(old, s, slots, cap, DevCas()) != 0;
	tally(bad, stat, PHS_NOSLOT);
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_vote(const uint64_t *__restrict__ ent, u64 n_full, ph_slot_t *slots, u64 cap, u64 *stat)
{
	__shared__ u64 s_sum;
	if (threadIdx.x == 0) s_sum = 0;
	__syncthreads();
	u64 both = 0, bad = 0;                                         /* the votes, and from bit 32 the new keys: a feed has less than 2^32 of either */
	for (u64 t = (u64)blockIdx.x * PH_THREADS + threadIdx.x + 1; t < n_full; t += (u64)gridDim.x * PH_THREADS) {
		uint64_t key, inc;
		if (!ph_vote(ent[t - 1], ent[t], &key, &inc)) continue;
		const int r = ph_add(slots, cap, key, inc, DevCas(), DevAdd64());
		if (r < 0) ++bad; else both += 1 + ((u64)r << 32);
	}
	tally_wg(both, &s_sum, stat, PHS_VOTE);
	tally(bad, stat, PHS_NOSLOT);
}

/* COUNT: cnt[s] = 1 iff slot s holds a pair.  EMIT: cnt[s] is its rank in pair[0 .. n) */
template<int MODE> __global__ __launch_bounds__(PH_THREADS)
void k_ph_pairs(const ph_slot_t *__restrict__ slots, u64 cap, u64 *__restrict__ cnt, ph_pair_t *__restrict__ pair, u64 n, u64 *stat)
{
	const u64 s = (u64)blockIdx.x * PH_THREADS + threadIdx.x;
	u64 bad = 0;
	if (s < cap) {
		ph_pair_t p;
		const int is = ph_pair(slots, s, &p);
		if (MODE == COUNT) cnt[s] = (u64)is;
		else if (is) {
			if (cnt[s] >= n) ++bad;
			else *reinterpret_cast<uint4*>(pair + cnt[s]) = make_uint4(p.i, p.j, p.cis, p.trans);
		}
	}
	tally(bad, stat, PHS_BAD);
}

template<int MODE> __global__ __launch_bounds__(PH_THREADS)
void k_ph_edges(const ph_slot_t *__restrict__ slots, u64 cap, const al_sup_t *__restrict__ sup, u64 min_sup, u64 min_link, u64 *__restrict__ cnt,
                ph_edge_t *__restrict__ edge, u64 n, u64 *stat)
{
	const u64 s = (u64)blockIdx.x * PH_THREADS + threadIdx.x;
	u64 bad = 0;
	if (s < cap) {
		ph_edge_t e;
		const int is = ph_edge(slots, s, sup, min_sup, min_link, &e);
		if (MODE == COUNT) cnt[s] = (u64)is;
		else if (is) {
			if (cnt[s] >= n) ++bad;
			else *reinterpret_cast<uint4*>(edge + cnt[s]) = make_uint4(e.i, e.j, e.w, e.flags);
		}
	}
	tally(bad, stat, PHS_BAD);
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_init(u64 n_bubble, uint32_t *__restrict__ comp, uint8_t *__restrict__ par, uint64_t *__restrict__ up, uint32_t *__restrict__ best_w,
               uint64_t *__restrict__ best_k, uint32_t *__restrict__ name, ph_block_t *__restrict__ tal)
{
	for (u64 b = (u64)blockIdx.x * PH_THREADS + threadIdx.x; b < n_bubble; b += (u64)gridDim.x * PH_THREADS) {
		comp[b] = (uint32_t)b; par[b] = 0; up[b] = b << 1; best_w[b] = 0; best_k[b] = PH_EMPTY; name[b] = PH_NONE;
		reinterpret_cast<v2*>(tal + b)[0] = make_ulonglong2(0, 0);
		reinterpret_cast<v2*>(tal + b)[1] = make_ulonglong2(0, 0);
	}
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_best_w(const ph_edge_t *__restrict__ edge, u64 n_edge, const uint32_t *__restrict__ comp, uint32_t *best_w, u64 *stat, int round)
{
	const u64 t = (u64)blockIdx.x * PH_THREADS + threadIdx.x;
	u64 cross = 0;
	if (t < n_edge) { const ph_edge_t e = edge[t]; cross = (u64)ph_best_w(&e, comp, best_w, DevMax32()); }
	cross = wave_sum(cross);                                       /* the host asks whether any edge crosses, not how many: a plain store of 1 */
	if ((threadIdx.x & (PH_WAVE - 1)) == 0 && cross) stat[PHS_CROSS + round] = 1;
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_best_key(const ph_edge_t *__restrict__ edge, u64 n_edge, const uint32_t *__restrict__ comp, const uint32_t *__restrict__ best_w, uint64_t *best_k)
{
	const u64 t = (u64)blockIdx.x * PH_THREADS + threadIdx.x;
	if (t < n_edge) { const ph_edge_t e = edge[t]; ph_best_key(&e, comp, best_w, best_k, DevMin64()); }
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_hook(ph_edge_t *edge, u64 n_edge, const uint32_t *__restrict__ comp, const uint8_t *__restrict__ par, const uint32_t *__restrict__ best_w,
               const uint64_t *__restrict__ best_k, uint64_t *up, u64 *stat)
{
	__shared__ u64 s_sum;
	if (threadIdx.x == 0) s_sum = 0;
	__syncthreads();
	const u64 t = (u64)blockIdx.x * PH_THREADS + threadIdx.x;
	u64 forest = 0;
	if (t < n_edge) {
		ph_edge_t e = edge[t];
		forest = (u64)ph_hook(&e, comp, par, best_w, best_k, up);
		if (forest) edge[t].flags = e.flags;
	}
	tally_wg(forest, &s_sum, stat, PHS_FOREST);
}

/* the roots of this round -- comp[r] == r -- double their hooks until each points at a root that stands */
__global__ __launch_bounds__(PH_THREADS)
void k_ph_flatten(u64 n_bubble, const uint32_t *__restrict__ comp, uint64_t *up)
{
	for (u64 r = (u64)blockIdx.x * PH_THREADS + threadIdx.x; r < n_bubble; r += (u64)gridDim.x * PH_THREADS)
		if (comp[r] == (uint32_t)r) ph_flatten(up, (uint32_t)r);
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_rewrite(u64 n_bubble, uint32_t *comp, uint8_t *par, const uint64_t *__restrict__ up, uint32_t *__restrict__ best_w, uint64_t *__restrict__ best_k)
{
	for (u64 b = (u64)blockIdx.x * PH_THREADS + threadIdx.x; b < n_bubble; b += (u64)gridDim.x * PH_THREADS) {
		ph_rewrite((uint32_t)b, comp, par, up);
		best_w[b] = 0; best_k[b] = PH_EMPTY;
	}
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_name(u64 n_bubble, const al_sup_t *__restrict__ sup, u64 min_sup, const uint32_t *__restrict__ comp, uint32_t *name)
{
	for (u64 b = (u64)blockIdx.x * PH_THREADS + threadIdx.x; b < n_bubble; b += (u64)gridDim.x * PH_THREADS)
		if (al_call(sup + b, min_sup) == 0) atomicMin(reinterpret_cast<unsigned*>(name + comp[b]), (unsigned)b);
}

__global__ __launch_bounds__(PH_THREADS)
void k_ph_nodes(u64 n_bubble, const al_sup_t *__restrict__ sup, u64 min_sup, const uint32_t *__restrict__ comp, const uint8_t *__restrict__ par,
                const uint32_t *__restrict__ name, ph_node_t *__restrict__ node, ph_block_t *tal, u64 *stat)
{
	__shared__ u64 s_sum;
	if (threadIdx.x == 0) s_sum = 0;
	__syncthreads();
	u64 n_het = 0;
	for (u64 b = (u64)blockIdx.x * PH_THREADS + threadIdx.x; b < n_bubble; b += (u64)gridDim.x * PH_THREADS) {
		const int het = al_call(sup + b, min_sup) == 0;
		const uint32_t nm = het ? name[comp[b]] : 0;
		const ph_node_t n = ph_node((uint32_t)b, het, nm, par);
		*reinterpret_cast<uint2*>(node + b) = make_uint2(n.block, n.flags);
		if (het) { atomicAdd(&tal[nm].n_bubble, 1u); ++n_het; }
	}
	tally_wg(n_het, &s_sum, stat, PHS_HET);
}

/* every edge into its block's tallies -- n_edge and n_disc by one 64-bit atomic, w_sum, w_disc --, bit 2 of the non-forest edges */
__global__ __launch_bounds__(PH_THREADS)
void k_ph_classify(ph_edge_t *edge, u64 n_edge, const ph_node_t *__restrict__ node, ph_block_t *tal)
{
	const u64 t = (u64)blockIdx.x * PH_THREADS + threadIdx.x;
	if (t >= n_edge) return;
	const ph_edge_t e = edge[t];
	const u64 disc = (u64)ph_discordant(&e, node);
	ph_block_t *b = tal + node[e.i].block;
	if (disc) edge[t].flags = e.flags | PH_DISC;
	atomicAdd(reinterpret_cast<u64*>(&b->n_edge), 1 | disc << 32);
	atomicAdd(reinterpret_cast<u64*>(&b->w_sum), (u64)e.w);
	if (disc) atomicAdd(reinterpret_cast<u64*>(&b->w_disc), (u64)e.w);
}

/* COUNT: cnt[b] = 1 iff b names a block of two or more; the blocks of one counted.  EMIT: the record at its rank */
template<int MODE> __global__ __launch_bounds__(PH_THREADS)
void k_ph_blocks(const ph_block_t *__restrict__ tal, u64 n_bubble, u64 *__restrict__ cnt, ph_block_t *__restrict__ blk, u64 n, u64 *stat)
{
	__shared__ u64 s_sum;
	if (threadIdx.x == 0) s_sum = 0;
	__syncthreads();
	const u64 b = (u64)blockIdx.x * PH_THREADS + threadIdx.x;
	u64 single = 0, bad = 0;
	if (b < n_bubble) {
		const v2 lo = reinterpret_cast<const v2*>(tal + b)[0];
		const u64 nb = lo.x >> 32;
		if (MODE == COUNT) { cnt[b] = nb >= 2; single = nb == 1; }
		else if (nb >= 2) {
			if (cnt[b] >= n) ++bad;
			else {
				reinterpret_cast<v2*>(blk + cnt[b])[0] = make_ulonglong2(nb << 32 | b, lo.y);
				reinterpret_cast<v2*>(blk + cnt[b])[1] = reinterpret_cast<const v2*>(tal + b)[1];
			}
		}
	}
	if (MODE == COUNT) tally_wg(single, &s_sum, stat, PHS_SINGLE);
	tally(bad, stat, PHS_BAD);
}

/* ---------------- host ---------------- */

thread_local double g_ms[5];                                       /* the compaction; the votes with the growth; the solve; copies; text */

const u64 MAX_GRID = 0x7fffffffull;                                /* a grid's first dimension */

}   // namespace

struct yakamd_phase_tab {
	int dev;
	bool solved;
	yakamd_phstat_t st;
	u64 n_vote, vote_limit;                                            /* the votes since the open or the last reset, and what they must stay below */
	DevBuf slots, stat, cnt, tsum, ent, pair, edge, node, tal, blk, comp, par, up, best_w, best_k, name;
};

namespace {

inline unsigned blocks_of(u64 n) { return (unsigned)((n + PH_THREADS - 1) / PH_THREADS); }

int read_stat(yakamd_phase_t *ph, u64 h_stat[PHS_N])
{
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, ph->stat.p, PHS_N * 8, hipMemcpyDeviceToHost));
	return 0;
}

/* cnt[0 .. n) becomes its exclusive scan, *total its sum */
int scan(yakamd_phase_t *ph, u64 n, u64 *total)
{
	const u64 m = (n + PH_TILE - 1) / PH_TILE;
	u64 *d_cnt = (u64*)ph->cnt.p, *d_tsum = (u64*)ph->tsum.p;
	YK_LAUNCH(k_ph_tile_sum, dim3((unsigned)m), dim3(PH_THREADS), 0, 0, (const u64*)d_cnt, n, d_tsum);
	YK_LAUNCH(k_ph_tile_scan, dim3(1), dim3(PH_THREADS), 0, 0, d_tsum, m);
	YK_LAUNCH(k_ph_scan_apply, dim3((unsigned)m), dim3(PH_THREADS), 0, 0, d_cnt, n, (const u64*)d_tsum);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(total, d_tsum + m, 8, hipMemcpyDeviceToHost));
	return 0;
}

/* room in cnt[] and tsum[] for a scan over n entries */
bool scan_room(yakamd_phase_t *ph, u64 n) { return ph->cnt.need((size_t)n * 8) && ph->tsum.need((size_t)((n + PH_TILE - 1) / PH_TILE + 1) * 8); }

int new_table(DevBuf &slots, u64 cap)
{
	if (!slots.get((size_t)cap * sizeof(ph_slot_t))) return fail("phase: no device memory for a table of %llu slots", cap);
	YK_LAUNCH(k_ph_clear, dim3(grid_for(cap, PH_THREADS)), dim3(PH_THREADS), 0, 0, (ph_slot_t*)slots.p, cap);
	HIPCK(hipGetLastError());
	return 0;
}

/* the table at `cap` slots: its slots moved into a new one */
int grow(yakamd_phase_t *ph, u64 cap)
{
	DevBuf next;
	u64 h_stat[PHS_N];
	if (new_table(next, cap) != 0) return -1;
	YK_LAUNCH(k_ph_rehash, dim3(grid_for(ph->st.capacity, PH_THREADS)), dim3(PH_THREADS), 0, 0, (const ph_slot_t*)ph->slots.p, (u64)ph->st.capacity, (ph_slot_t*)next.p, cap,
	          (u64*)ph->stat.p);
	if (read_stat(ph, h_stat) != 0) return -1;
	if (h_stat[PHS_NOSLOT]) return fail("phase votes: %llu of the %llu pairs found no slot among the %llu of the larger table", h_stat[PHS_NOSLOT], (u64)ph->st.n_pair, cap);
	std::swap(ph->slots.p, next.p); std::swap(ph->slots.have, next.have);
	ph->st.capacity = cap; ++ph->st.n_grow;
	return 0;
}

}   // namespace

extern "C" const char *yakamd_phase_last_error(void) { return g_err; }
extern "C" void yakamd_phase_ms(double ms[5]) { for (int i = 0; i < 5; ++i) ms[i] = g_ms[i]; }
extern "C" void yakamd_phopt_init(yakamd_phopt_t *o)
{
	if (!o) return;
	o->min_cnt = 1; o->min_sup = 2; o->min_link = 2; o->edges = 0; o->stats_only = 0; o->reserved = 0; o->chunk_size = (int64_t)1 << 28;
}

extern "C" yakamd_phase_t *yakamd_phase_open(int64_t n_bubble)
{
	for (int i = 0; i < 5; ++i) g_ms[i] = 0;
	if (n_bubble < 0 || n_bubble >= (int64_t)1 << 31) { fail("phase: %lld bubbles: an entry holds a bubble below 2^31", (long long)n_bubble); return 0; }
	yakamd_phase_t *ph = new (std::nothrow) yakamd_phase_t();
	if (!ph) { fail("phase: no memory"); return 0; }
	memset(&ph->st, 0, sizeof ph->st);
	ph->dev = 0; ph->solved = false; ph->n_vote = 0; ph->vote_limit = (u64)1 << 32;
	ph->st.n_bubble = (u64)n_bubble; ph->st.capacity = PH_CAP0;
	const char *lim = getenv("YAKAMD_PHASE_VOTE_LIMIT");             /* a test switch: 2^32 votes are more than a test feeds */
	if (lim && *lim) { const u64 v = strtoull(lim, 0, 10); if (v >= 1 && v < ph->vote_limit) ph->vote_limit = v; }
	const u64 n = (u64)n_bubble;
	const bool ok = hipGetDevice(&ph->dev) == hipSuccess && ph->stat.get(PHS_N * 8) && ph->node.get(n * 8) && ph->tal.get(n * 32) && ph->comp.get(n * 4) && ph->par.get(n) &&
	                ph->up.get(n * 8) && ph->best_w.get(n * 4) && ph->best_k.get(n * 8) && ph->name.get(n * 4) && hipMemset(ph->stat.p, 0, PHS_N * 8) == hipSuccess;
	if (!ok) { fail("phase: no device, or no device memory for %llu bubbles", n); delete ph; return 0; }
	if (new_table(ph->slots, PH_CAP0) != 0) { delete ph; return 0; }
	return ph;
}

extern "C" void yakamd_phase_close(yakamd_phase_t *ph)
{
	if (!ph) return;
	OnDevice dev(ph->dev);
	delete ph;
}

extern "C" int yakamd_phase_stats(yakamd_phase_t *ph, yakamd_phstat_t *st)
{
	if (!ph || !st) return fail("phase stats: no table, or no place for the numbers");
	*st = ph->st;
	return 0;
}

extern "C" int yakamd_phase_reset(yakamd_phase_t *ph)
{
	if (!ph) return fail("phase reset: no table");
	OnDevice dev(ph->dev);
	YK_LAUNCH(k_ph_clear, dim3(grid_for(ph->st.capacity, PH_THREADS)), dim3(PH_THREADS), 0, 0, (ph_slot_t*)ph->slots.p, (u64)ph->st.capacity);
	HIPCK(hipGetLastError());
	ph->st.n_pair = 0; ph->n_vote = 0; ph->solved = false;
	return 0;
}

extern "C" int yakamd_phase_votes_dev(yakamd_phase_t *ph, const yakamd_aobs_t *d_obs, int64_t n_obs, int64_t n_out[2])
{
	if (!ph) return fail("phase votes: no table");
	if (!n_out) return fail("phase votes: no place for the two numbers");
	n_out[0] = n_out[1] = 0;
	if (n_obs < 0) return fail("phase votes: %lld records", (long long)n_obs);
	if (((uintptr_t)d_obs & 15) != 0) return fail("phase votes: the records must be 16-byte aligned");
	if (n_obs > 0 && !d_obs) return fail("phase votes: %lld records without their list", (long long)n_obs);
	if (n_obs == 0) return 0;                                      /* no record: no launch */
	const u64 n = (u64)n_obs, g = (n + PH_THREADS - 1) / PH_THREADS;
	if (g > MAX_GRID) return fail("phase votes: %lld records are more than one launch serves", (long long)n_obs);
	if (ph->n_vote + (n - 1) >= ph->vote_limit)
		return fail("phase votes: %llu votes so far and up to %llu more: the two counters of a pair are 32 bits, so the votes stay below %llu", ph->n_vote, n - 1, ph->vote_limit);
	OnDevice dev(ph->dev);
	if (!scan_room(ph, n)) return fail("phase votes: no device memory for %lld records", (long long)n_obs);
	u64 *d_stat = (u64*)ph->stat.p, h_stat[PHS_N], n_full = 0;
	double t0 = now_ms();
	HIPCK(hipMemset(d_stat, 0, PHS_N * 8));
	YK_LAUNCH(k_ph_full<COUNT>, dim3((unsigned)g), dim3(PH_THREADS), 0, 0, (const al_obs_t*)d_obs, n, (u64)ph->st.n_bubble, (u64*)ph->cnt.p, (uint64_t*)0, (u64)0, d_stat);
	if (scan(ph, n, &n_full) != 0 || read_stat(ph, h_stat) != 0) return -1;
	if (h_stat[PHS_BAD])
		return fail("phase votes: %llu of the %lld records do not fit: a bubble is none of the %llu, or a sequence comes behind a later one", h_stat[PHS_BAD], (long long)n_obs,
		            (u64)ph->st.n_bubble);
	if (n_full > n) return fail("phase votes: the scan holds %llu full records of %llu", n_full, n);
	n_out[0] = (int64_t)n_full;
	ph->solved = false;                                            /* a feed that was taken: the results of a solve before it no longer stand */
	if (n_full < 2) { g_ms[0] += now_ms() - t0; return 0; }        /* one entry has no neighbour */
	if (!ph->ent.need((size_t)n_full * 8)) return fail("phase votes: no device memory for %llu entries", n_full);
	YK_LAUNCH(k_ph_full<EMIT>, dim3((unsigned)g), dim3(PH_THREADS), 0, 0, (const al_obs_t*)d_obs, n, (u64)ph->st.n_bubble, (u64*)ph->cnt.p, (uint64_t*)ph->ent.p, n_full, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipDeviceSynchronize());
	g_ms[0] += now_ms() - t0; t0 = now_ms();
	if (2 * (ph->st.n_pair + n_full) > ph->st.capacity && grow(ph, ph_capacity(ph->st.capacity, ph->st.n_pair + n_full)) != 0) return -1;
	YK_LAUNCH(k_ph_vote, dim3(grid_for(n_full, PH_THREADS)), dim3(PH_THREADS), 0, 0, (const uint64_t*)ph->ent.p, n_full, (ph_slot_t*)ph->slots.p, (u64)ph->st.capacity, d_stat);
	if (read_stat(ph, h_stat) != 0) return -1;
	g_ms[1] += now_ms() - t0;
	const u64 n_vote = h_stat[PHS_VOTE] & 0xffffffffull, n_fresh = h_stat[PHS_VOTE] >> 32;
	ph->st.n_pair += n_fresh; ph->n_vote += n_vote;
	if (h_stat[PHS_BAD] || h_stat[PHS_NOSLOT])
		return fail("phase votes: %llu entries had a rank outside the list and %llu votes found no slot among the %llu of the table", h_stat[PHS_BAD], h_stat[PHS_NOSLOT],
		            (u64)ph->st.capacity);
	n_out[1] = (int64_t)n_vote;
	return 0;
}

extern "C" int64_t yakamd_phase_pairs_dev(yakamd_phase_t *ph, void *d, int64_t cap)
{
	if (!ph) return copy_out(false, 0, 0, 0, sizeof(ph_pair_t), d, cap, "phase pairs", "table", "the entries");
	const u64 n = ph->st.n_pair, n_slot = ph->st.capacity;
	if (!d || cap < (int64_t)n || n == 0) return (int64_t)n;
	if (((uintptr_t)d & 15) != 0) return fail("phase pairs: the entries must be 16-byte aligned");      /* before the launches, not behind them in copy_out() */
	OnDevice dev(ph->dev);
	const double t0 = now_ms();
	u64 total = 0, h_stat[PHS_N];
	if (!scan_room(ph, n_slot) || !ph->pair.need((size_t)n * sizeof(ph_pair_t))) return fail("phase pairs: no device memory for %llu pairs", n);
	HIPCK(hipMemset(ph->stat.p, 0, PHS_N * 8));
	YK_LAUNCH(k_ph_pairs<COUNT>, dim3(blocks_of(n_slot)), dim3(PH_THREADS), 0, 0, (const ph_slot_t*)ph->slots.p, n_slot, (u64*)ph->cnt.p, (ph_pair_t*)0, (u64)0, (u64*)ph->stat.p);
	if (scan(ph, n_slot, &total) != 0) return -1;
	if (total != n) return fail("phase pairs: the table holds %llu pairs, its counter %llu", total, n);
	YK_LAUNCH(k_ph_pairs<EMIT>, dim3(blocks_of(n_slot)), dim3(PH_THREADS), 0, 0, (const ph_slot_t*)ph->slots.p, n_slot, (u64*)ph->cnt.p, (ph_pair_t*)ph->pair.p, n, (u64*)ph->stat.p);
	if (read_stat(ph, h_stat) != 0) return -1;
	if (h_stat[PHS_BAD]) return fail("phase pairs: %llu pairs had a rank outside the list", h_stat[PHS_BAD]);
	g_ms[3] += now_ms() - t0;
	return copy_out(true, ph->dev, ph->pair.p, n, sizeof(ph_pair_t), d, cap, "phase pairs", "table", "the entries");
}

extern "C" int yakamd_phase_solve_dev(yakamd_phase_t *ph, const yakamd_asup_t *d_sup, int64_t n_sup, int32_t min_sup, int32_t min_link)
{
	if (!ph) return fail("phase solve: no table");
	if (n_sup != (int64_t)ph->st.n_bubble) return fail("phase solve: the support of %lld bubbles for %llu", (long long)n_sup, (u64)ph->st.n_bubble);
	if (min_sup < 1 || min_link < 1) return fail("phase solve: min_sup %d, min_link %d: both are at least 1", min_sup, min_link);
	if (((uintptr_t)d_sup & 15) != 0) return fail("phase solve: the support must be 16-byte aligned");
	if (n_sup > 0 && !d_sup) return fail("phase solve: %lld bubbles without their support", (long long)n_sup);
	yakamd_phstat_t &st = ph->st;
	ph->solved = false;
	st.n_het = st.n_edge = st.n_forest = st.n_block = st.n_single = st.n_round = 0;
	if (st.n_bubble == 0) { ph->solved = true; return 0; }         /* no bubble: no launch */
	OnDevice dev(ph->dev);
	const double t0 = now_ms();
	const u64 n_b = st.n_bubble, n_slot = st.capacity, ms = (u64)min_sup;
	const al_sup_t *sup = (const al_sup_t*)d_sup;
	u64 *d_stat = (u64*)ph->stat.p, h_stat[PHS_N], n_edge = 0, n_block = 0;
	uint32_t *comp = (uint32_t*)ph->comp.p, *best_w = (uint32_t*)ph->best_w.p, *name = (uint32_t*)ph->name.p;
	uint8_t *par = (uint8_t*)ph->par.p;
	uint64_t *up = (uint64_t*)ph->up.p, *best_k = (uint64_t*)ph->best_k.p;
	ph_block_t *tal = (ph_block_t*)ph->tal.p;
	if (!scan_room(ph, n_slot > n_b ? n_slot : n_b)) return fail("phase solve: no device memory for %llu slots and %llu bubbles", n_slot, n_b);
	HIPCK(hipMemset(d_stat, 0, PHS_N * 8));
	const unsigned gb = grid_for(n_b, PH_THREADS);
	YK_LAUNCH(k_ph_init, dim3(gb), dim3(PH_THREADS), 0, 0, n_b, comp, par, up, best_w, best_k, name, tal);
	if (st.n_pair) {
		YK_LAUNCH(k_ph_edges<COUNT>, dim3(blocks_of(n_slot)), dim3(PH_THREADS), 0, 0, (const ph_slot_t*)ph->slots.p, n_slot, sup, ms, (u64)min_link, (u64*)ph->cnt.p, (ph_edge_t*)0, (u64)0, d_stat);
		if (scan(ph, n_slot, &n_edge) != 0) return -1;
	}
	if (n_edge > st.n_pair) return fail("phase solve: %llu edges of %llu pairs", n_edge, (u64)st.n_pair);
	ph_edge_t *edge = 0;
	const unsigned ge = blocks_of(n_edge);
	if (n_edge) {
		if (!ph->edge.need((size_t)n_edge * sizeof(ph_edge_t))) return fail("phase solve: no device memory for %llu edges", n_edge);
		edge = (ph_edge_t*)ph->edge.p;
		YK_LAUNCH(k_ph_edges<EMIT>, dim3(blocks_of(n_slot)), dim3(PH_THREADS), 0, 0, (const ph_slot_t*)ph->slots.p, n_slot, sup, ms, (u64)min_link, (u64*)ph->cnt.p, edge, n_edge, d_stat);
		for (int round = 0;; ++round) {
			if (round == PH_MAX_ROUND) return fail("phase solve: edges still cross after %d rounds", round);
			YK_LAUNCH(k_ph_best_w, dim3(ge), dim3(PH_THREADS), 0, 0, (const ph_edge_t*)edge, n_edge, (const uint32_t*)comp, best_w, d_stat, round);
			if (read_stat(ph, h_stat) != 0) return -1;
			++st.n_round;
			if (h_stat[PHS_BAD]) return fail("phase solve: %llu edges had a rank outside the list", h_stat[PHS_BAD]);
			if (h_stat[PHS_CROSS + round] == 0) break;
			YK_LAUNCH(k_ph_best_key, dim3(ge), dim3(PH_THREADS), 0, 0, (const ph_edge_t*)edge, n_edge, (const uint32_t*)comp, (const uint32_t*)best_w, best_k);
			YK_LAUNCH(k_ph_hook, dim3(ge), dim3(PH_THREADS), 0, 0, edge, n_edge, (const uint32_t*)comp, (const uint8_t*)par, (const uint32_t*)best_w, (const uint64_t*)best_k, up, d_stat);
			YK_LAUNCH(k_ph_flatten, dim3(gb), dim3(PH_THREADS), 0, 0, n_b, (const uint32_t*)comp, up);
			YK_LAUNCH(k_ph_rewrite, dim3(gb), dim3(PH_THREADS), 0, 0, n_b, comp, par, (const uint64_t*)up, best_w, best_k);
		}
	}
	YK_LAUNCH(k_ph_name, dim3(gb), dim3(PH_THREADS), 0, 0, n_b, sup, ms, (const uint32_t*)comp, name);
	YK_LAUNCH(k_ph_nodes, dim3(gb), dim3(PH_THREADS), 0, 0, n_b, sup, ms, (const uint32_t*)comp, (const uint8_t*)par, (const uint32_t*)name, (ph_node_t*)ph->node.p, tal, d_stat);
	if (n_edge) YK_LAUNCH(k_ph_classify, dim3(ge), dim3(PH_THREADS), 0, 0, edge, n_edge, (const ph_node_t*)ph->node.p, tal);
	YK_LAUNCH(k_ph_blocks<COUNT>, dim3(blocks_of(n_b)), dim3(PH_THREADS), 0, 0, (const ph_block_t*)tal, n_b, (u64*)ph->cnt.p, (ph_block_t*)0, (u64)0, d_stat);
	if (scan(ph, n_b, &n_block) != 0) return -1;
	if (n_block > n_b / 2) return fail("phase solve: %llu blocks of two or more among %llu bubbles", n_block, n_b);
	if (n_block) {
		if (!ph->blk.need((size_t)n_block * sizeof(ph_block_t))) return fail("phase solve: no device memory for %llu blocks", n_block);
		YK_LAUNCH(k_ph_blocks<EMIT>, dim3(blocks_of(n_b)), dim3(PH_THREADS), 0, 0, (const ph_block_t*)tal, n_b, (u64*)ph->cnt.p, (ph_block_t*)ph->blk.p, n_block, d_stat);
	}
	if (read_stat(ph, h_stat) != 0) return -1;
	if (h_stat[PHS_BAD]) return fail("phase solve: %llu records had a rank outside their list", h_stat[PHS_BAD]);
	st.n_het = h_stat[PHS_HET]; st.n_edge = n_edge; st.n_forest = h_stat[PHS_FOREST]; st.n_block = n_block; st.n_single = h_stat[PHS_SINGLE];
	if (st.n_forest + st.n_block + st.n_single != st.n_het)
		return fail("phase solve: %llu forest edges, %llu blocks and %llu bubbles alone do not add up to %llu het bubbles", (u64)st.n_forest, n_block, (u64)st.n_single, (u64)st.n_het);
	ph->solved = true;
	g_ms[2] += now_ms() - t0;
	return 0;
}

namespace {
int64_t result_out(yakamd_phase_t *ph, DevBuf yakamd_phase_tab::*buf, uint64_t yakamd_phstat_t::*n, u64 each, void *d, int64_t cap, const char *what)
{
	if (ph && !ph->solved) return fail("%s: no solve since the open, the last votes or the last reset", what);
	return copy_out(ph != 0, ph ? ph->dev : 0, ph ? (ph->*buf).p : 0, ph ? ph->st.*n : 0, each, d, cap, what, "table", "the entries");
}
}   // namespace

extern "C" int64_t yakamd_phase_nodes_dev(yakamd_phase_t *ph, void *d, int64_t cap) { return result_out(ph, &yakamd_phase_tab::node, &yakamd_phstat_t::n_bubble, sizeof(ph_node_t), d, cap, "phase nodes"); }
extern "C" int64_t yakamd_phase_edges_dev(yakamd_phase_t *ph, void *d, int64_t cap) { return result_out(ph, &yakamd_phase_tab::edge, &yakamd_phstat_t::n_edge, sizeof(ph_edge_t), d, cap, "phase edges"); }
extern "C" int64_t yakamd_phase_blocks_dev(yakamd_phase_t *ph, void *d, int64_t cap) { return result_out(ph, &yakamd_phase_tab::blk, &yakamd_phstat_t::n_block, sizeof(ph_block_t), d, cap, "phase blocks"); }

/* ---- the command ---- */
namespace {

struct ChunkDev { SeqChunkDev seqs; DevBuf hit, paths, steps, obs; };

/* one chunk through the device: its paths, its observations into the support, their votes into the table */
int run_chunk(yakamd_allele_t *al, yakamd_phase_t *ph, yakamd_path_t *px, SeqChunk &c, ChunkDev &d, pht_total_t *tot)
{
	const size_t n_seq = c.name.size();
	size_t n = 0;
	if (n_seq == 0) return 0;
	tot->n_seq += n_seq; tot->len += c.bases;
	if (!d.hit.need((size_t)up16(c.img.size()) * 8)) return fail("yakamd_phase: no device memory for a chunk of %zu bytes", c.img.size());
	if (d.seqs.upload("yakamd_phase", c, &n, &g_ms[3]) != 0) return -1;
	const uint64_t *d_off = (const uint64_t*)d.seqs.off.p;
	const uint32_t *d_len = (const uint32_t*)d.seqs.len.p;
	if (yakamd_path_hits_dev(px, d.seqs.img.p, (int64_t)n, (uint64_t*)d.hit.p) != 0) return fail_below(yakamd_path_last_error());
	int64_t np[2], again[2], no[2], nv[2];
	int rc = yakamd_path_chain_dev(px, (const uint64_t*)d.hit.p, (int64_t)n, d_off, d_len, (int64_t)n_seq, 0, 0, 0, 0, 0, np);
	if (rc < 0) return fail_below(yakamd_path_last_error());
	tot->path += (uint64_t)np[0]; tot->step += (uint64_t)np[1];
	if (np[0] == 0) return 0;
	if (!d.paths.need((size_t)np[0] * 32) || !d.steps.need((size_t)np[1] * 8)) return fail("yakamd_phase: no device memory for %lld paths of %lld steps", (long long)np[0], (long long)np[1]);
	rc = yakamd_path_chain_dev(px, (const uint64_t*)d.hit.p, (int64_t)n, d_off, d_len, (int64_t)n_seq, (yakamd_upath_t*)d.paths.p, np[0], (uint64_t*)d.steps.p, np[1], 0, again);
	if (rc < 0) return fail_below(yakamd_path_last_error());
	if (rc != 0) return fail("yakamd_phase: the writing call counted %lld paths of %lld steps, the counting call %lld of %lld", (long long)again[0], (long long)again[1], (long long)np[0], (long long)np[1]);
	rc = yakamd_allele_obs_dev(al, (const yakamd_upath_t*)d.paths.p, np[0], (const uint64_t*)d.steps.p, np[1], 0, 0, no);
	if (rc < 0) return fail_below(yakamd_allele_last_error());
	tot->obs += (uint64_t)no[0]; tot->full += (uint64_t)no[1];
	if (no[0] == 0) return 0;
	if (!d.obs.need((size_t)no[0] * 16)) return fail("yakamd_phase: no device memory for %lld observations", (long long)no[0]);
	rc = yakamd_allele_obs_dev(al, (const yakamd_upath_t*)d.paths.p, np[0], (const uint64_t*)d.steps.p, np[1], (yakamd_aobs_t*)d.obs.p, no[0], again);
	if (rc < 0) return fail_below(yakamd_allele_last_error());
	if (rc != 0 || again[0] != no[0] || again[1] != no[1])
		return fail("yakamd_phase: the writing call counted %lld observations, the counting call %lld", (long long)again[0], (long long)no[0]);
	if (yakamd_phase_votes_dev(ph, (const yakamd_aobs_t*)d.obs.p, no[0], nv) != 0) return -1;
	if (nv[0] != no[1]) return fail("yakamd_phase: %lld full records among the observations, %lld counted with them", (long long)nv[0], (long long)no[1]);
	tot->vote += (uint64_t)nv[1];
	return 0;
}

/* n entries of a result through device memory of ours to the host */
template<class T> int fetch(yakamd_phase_t *ph, int64_t (*get)(yakamd_phase_t*, void*, int64_t), DevBuf &d, std::vector<T> &out)
{
	const int64_t n = get(ph, 0, 0);
	if (n < 0) return -1;
	out.resize((size_t)n);
	if (n == 0) return 0;
	if (!d.need((size_t)n * sizeof(T))) return fail("yakamd_phase: no device memory for %lld entries of a result", (long long)n);
	if (get(ph, d.p, n) != n) return -1;
	HIPCK(hipMemcpy(out.data(), d.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
	return 0;
}

}   // namespace

extern "C" int yakamd_phase(const yakamd_phopt_t *opt, yak_ch_t *ch, const char *reads_fn, const char *out_fn)
{
	if (!opt) return fail("yakamd_phase: no options");
	if (opt->min_sup < 1) return fail("yakamd_phase: min_sup %d", opt->min_sup);
	if (opt->min_link < 1) return fail("yakamd_phase: min_link %d", opt->min_link);
	if (opt->chunk_size < 1) return fail("yakamd_phase: chunk_size %lld", (long long)opt->chunk_size);
	if (!reads_fn) return fail("yakamd_phase: no reads");
	if (ch && yakamd_ch_hpc(ch)) return fail("yakamd_phase: the table is marked homopolymer-compressed: its unitigs are no sequences to lay reads onto");
	SeqReader rd(false);                                           /* of a quality its length alone */
	if (ch && !rd.open(reads_fn)) return fail("yakamd_phase: cannot read '%s'", reads_fn);
	WalkGuard W{ yakamd_uwalk_open(ch, opt->min_cnt) };
	if (!W.p) return fail_below(yakamd_walk_last_error());
	const int k = ch->k;
	Guard<yakamd_gfa_t, yakamd_gfa_close> G{ yakamd_gfa_open(W.p, k) };
	if (!G.p) return fail_below(yakamd_gfa_last_error());
	Guard<yakamd_bubble_set_t, yakamd_bubble_close> B{ yakamd_bubble_open(W.p, G.p, k) };
	if (!B.p) return fail_below(yakamd_bubble_last_error());
	Guard<yakamd_allele_t, yakamd_allele_close> A{ yakamd_allele_open(W.p, B.p) };
	if (!A.p) return fail_below(yakamd_allele_last_error());
	Guard<yakamd_path_t, yakamd_path_close> P{ yakamd_path_open(W.p, k) };
	if (!P.p) return fail_below(yakamd_path_last_error());
	yakamd_alstat_t as;
	if (yakamd_allele_stats(A.p, &as) != 0) return fail_below(yakamd_allele_last_error());
	const u64 n_b = as.n_bubble;
	std::vector<bb_rec_t> rec;
	std::vector<al_sup_t> sup;
	try { rec.resize((size_t)n_b); sup.resize((size_t)n_b); } catch (const std::bad_alloc&) { return fail("yakamd_phase: %llu bubbles do not fit the host's memory", n_b); }
	DevBuf d_rec, d_sup, d_res;
	double t0 = now_ms();
	if (n_b) {                                                     /* the bubble records, for the A lines, while the bubbles are open */
		if (!d_rec.get((size_t)n_b * sizeof(bb_rec_t)) || !d_sup.get((size_t)n_b * sizeof(al_sup_t))) return fail("yakamd_phase: no device memory for %llu bubbles", n_b);
		if (yakamd_bubble_records_dev(B.p, d_rec.p, (int64_t)n_b) != (int64_t)n_b) return fail_below(yakamd_bubble_last_error());
		HIPCK(hipMemcpy(rec.data(), d_rec.p, (size_t)n_b * sizeof(bb_rec_t), hipMemcpyDeviceToHost));
		d_rec.drop();
	}
	B.close(); G.close(); W.close();
	Guard<yakamd_phase_t, yakamd_phase_close> H{ yakamd_phase_open((int64_t)n_b) };
	yakamd_phase_t *ph = H.p;
	if (!ph) return -1;
	g_ms[3] += now_ms() - t0;
	OutFile out(out_fn);
	if (!out.f) return fail("yakamd_phase: cannot write '%s'", out.name);
	bool ok = true;
	ChunkDev d;
	std::string text;
	pht_total_t tot = { 0, 0, 0, 0, 0, 0, 0 };
	if (seq_chunks("yakamd_phase", rd, reads_fn, opt->chunk_size, 0, [&](SeqChunk &c, bool last) { return run_chunk(A.p, ph, P.p, c, d, &tot); }) != 0) return -1;
	if (n_b && yakamd_allele_support_dev(A.p, d_sup.p, (int64_t)n_b) != (int64_t)n_b) return fail_below(yakamd_allele_last_error());
	if (yakamd_phase_solve_dev(ph, (const yakamd_asup_t*)d_sup.p, (int64_t)n_b, opt->min_sup, opt->min_link) != 0) return -1;
	t0 = now_ms();
	std::vector<ph_node_t> node;
	std::vector<ph_block_t> blk;
	std::vector<ph_edge_t> edge;
	std::vector<ph_pair_t> pair;
	try {
		if (n_b) HIPCK(hipMemcpy(sup.data(), d_sup.p, (size_t)n_b * sizeof(al_sup_t), hipMemcpyDeviceToHost));
		if (fetch(ph, yakamd_phase_blocks_dev, d_res, blk) != 0) return -1;
		if (!opt->stats_only && fetch(ph, yakamd_phase_nodes_dev, d_res, node) != 0) return -1;
		if (!opt->stats_only && opt->edges && (fetch(ph, yakamd_phase_edges_dev, d_res, edge) != 0 || fetch(ph, yakamd_phase_pairs_dev, d_res, pair) != 0)) return -1;
		g_ms[3] += now_ms() - t0; t0 = now_ms();
		const yakamd_phstat_t &st = ph->st;
		const pht_solve_t sv = { st.n_pair, st.n_het, st.n_edge, st.n_forest, st.n_block, st.n_single };
		uint64_t n_call[4] = { 0, 0, 0, 0 }, n_disc = 0, max_block = 0;
		pht_head(text, k, opt->min_cnt, opt->min_sup, opt->min_link);
		alt_alleles(text, rec.data(), sup.data(), n_b, (uint64_t)opt->min_sup, !opt->stats_only, n_call);
		if (n_call[0] != st.n_het) return fail("yakamd_phase: %llu het bubbles by the support, %llu by the solve", (u64)n_call[0], (u64)st.n_het);
		if (!opt->stats_only) pht_nodes(text, node.data(), n_b);
		pht_blocks(text, blk.data(), blk.size(), !opt->stats_only, &n_disc, &max_block);
		if (!opt->stats_only && opt->edges && !pht_edges(text, edge, pair)) return fail("yakamd_phase: an edge without its pair");
		pht_tail(text, tot, n_b, sv, n_disc, max_block);
	} catch (const std::bad_alloc&) { return fail("yakamd_phase: no host memory for the results and the text"); }
	flush(text, &out, true, &ok);
	if (!(out.finish() && ok)) return fail("yakamd_phase: cannot write '%s'", out.name);
	g_ms[4] += now_ms() - t0;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] phase: %llu votes on %llu pairs of %llu bubbles, %llu rounds, the table grew %llu times to %llu slots: compaction %.1f ms, votes %.1f ms, solve %.1f ms, copies %.1f ms, text %.1f ms\n",
		        (u64)tot.vote, (u64)ph->st.n_pair, n_b, (u64)ph->st.n_round, (u64)ph->st.n_grow, (u64)ph->st.capacity, g_ms[0], g_ms[1], g_ms[2], g_ms[3], g_ms[4]);
	return 0;
}

LAYER_TALLY_EXPORTS(phase)
