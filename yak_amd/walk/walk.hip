/*
 * walk.hip -- libyak_amd_walk.so: the unitigs of a count table's de Bruijn graph walked on the GPU (include/yak_amd_walk.h).
 * A layer above libyak_amd.so: it calls its public functions only (yakamd_graph_open / _stats / _nodes_dev / _close, yakamd_last_error) and owns its
 * device memory (hipMalloc / hipFree).  The per-state steps are those of uwalk_step.h, the host's share (cycles, tallies, text) that of uwalk_host.h;
 * every launch goes through YK_LAUNCH of ../csrc/tally.h into this library's own tally (yakamd_walk_tally_*).  The host scaffolding and the scans are
 * those of ../layer/layer_host.h and ../layer/layer_dev.h, which the three layers share.
 *
 *   k_uw_init          the pair (ptr, dist) of both states of every stored key from its record
 *   k_uw_jump          one doubling round from one pair buffer into the other (never in place: a 16-byte pair is not read atomically), and the
 *                      number of states that reached their terminal in it.  A round in which none does ends the ranking: the finished states of a
 *                      chain are contiguous from its end, so every state still unfinished lies on a cycle
 *   k_uw_decide        per node the start node of its unitig and its place p << 1 | d in it (uw_decide); the start nodes flagged with their
 *                      unitig's bases for the two scans
 *   k_uw_tile_sum, k_uw_tile_scan, k_uw_scan_apply
 *                      the exclusive scan of a (u64, u64) array in place: tiles of 1024, their sums scanned by one workgroup
 *   k_uw_emit          map entries, descriptors (kc by integer atomics) and bases of the open unitigs: one store per node, k for v_0
 *   k_uw_cyc_flag, k_uw_cyc_gather, k_uw_cyc_scatter
 *                      the records of the nodes on cycles compacted in listing order for the host, and the host's map entries put in place
 * All results are addressed by listing index or by j; all stores are vector stores, all tallies integer atomics whose order changes no result.
 */
#include "yak.h"
#define LAYER_NAME "walk"
#include "../layer/layer_host.h"
#include "../layer/layer_dev.h"
#include "uwalk_step.h"
#include "uwalk_host.h"

static_assert(sizeof(yakamd_gnode_t) == 32 && sizeof(uw_node_t) == 32, "a graph record is 32 bytes");
static_assert(sizeof(yakamd_umap_t) == sizeof(uw_map_t) && sizeof(yakamd_udesc_t) == sizeof(uw_desc_t) && sizeof(uw_pair_t) == 16, "the results as declared");

namespace {

enum { UW_THREADS = 256, UW_ITEMS = 4, UW_TILE = UW_THREADS * UW_ITEMS, UW_WAVE = 64, UW_SCAN_THREADS = 1024, UW_MAX_ROUNDS = 66 };
enum { UWT_CYCLE = 0, UWT_BAD = 1, UWT_N = 4 };                   /* tally words: nodes on cycles, nodes whose links or places are not consistent */
#define UW_DEC_CYCLE 0                                            /* dec[v] = (UW_NONE, this): a node on a cycle */
#define UW_DEC_ABSENT 1                                           /* ... a key that is no node */

__device__ inline uw_pair_t ld_pair(const uw_pair_t *p) { const v2 v = *reinterpret_cast<const v2*>(p); uw_pair_t o; o.ptr = v.x; o.dist = v.y; return o; }
__device__ inline void st_pair(uw_pair_t *p, uw_pair_t o) { *reinterpret_cast<v2*>(p) = make_ulonglong2(o.ptr, o.dist); }
__device__ inline uw_node_t ld_node(const uw_node_t *p)
{
	const v2 a = reinterpret_cast<const v2*>(p)[0], b = reinterpret_cast<const v2*>(p)[1];
	uw_node_t r;
	r.x = a.x; r.link[0] = a.y; r.link[1] = b.x; r.count = (uint32_t)b.y; r.edges = (uint32_t)(b.y >> 32);
	return r;
}

__global__ __launch_bounds__(UW_THREADS)
void k_uw_init(const uw_node_t *__restrict__ rec, u64 n, uint32_t min_cnt, uw_pair_t *__restrict__ out)
{
	for (u64 v = (u64)blockIdx.x * UW_THREADS + threadIdx.x; v < n; v += (u64)gridDim.x * UW_THREADS) {
		const uw_node_t r = ld_node(rec + v);
		st_pair(out + 2 * v, uw_init(&r, v, 0, min_cnt));
		st_pair(out + 2 * v + 1, uw_init(&r, v, 1, min_cnt));
	}
}

__global__ __launch_bounds__(UW_THREADS)
void k_uw_jump(const uw_pair_t *__restrict__ src, uw_pair_t *__restrict__ dst, u64 n_state, u64 *__restrict__ n_finished)
{
	u64 fin = 0;
	for (u64 s = (u64)blockIdx.x * UW_THREADS + threadIdx.x; s < n_state; s += (u64)gridDim.x * UW_THREADS) {
		uw_pair_t p = ld_pair(src + s);
		const u64 t = uw_target(p, n_state);
		if (t != UW_NONE) {
			int f;
			p = uw_jump(p, ld_pair(src + t), &f);
			fin += (u64)f;
		}
		st_pair(dst + s, p);
	}
	fin = wave_sum(fin);
	if ((threadIdx.x & (UW_WAVE - 1)) == 0 && fin) atomicAdd(n_finished, fin);
}

/* dec[v] = (start node, p << 1 | d), or (UW_NONE, UW_DEC_CYCLE / UW_DEC_ABSENT); sc[v] = (1, n_node + k - 1) for a start node, else (0, 0) */
__global__ __launch_bounds__(UW_THREADS)
void k_uw_decide(const uw_pair_t *__restrict__ fin, u64 n, int k, v2 *__restrict__ dec, v2 *__restrict__ sc, u64 *__restrict__ tally)
{
	u64 cyc = 0, bad = 0;
	for (u64 v = (u64)blockIdx.x * UW_THREADS + threadIdx.x; v < n; v += (u64)gridDim.x * UW_THREADS) {
		const uw_pair_t a = ld_pair(fin + 2 * v), b = ld_pair(fin + 2 * v + 1);
		v2 d = make_ulonglong2(UW_NONE, UW_DEC_ABSENT), s = make_ulonglong2(0, 0);
		if (!uw_dead(a)) {
			uw_place_t w;
			const int r = uw_decide(v, a, b, &w);
			if (r > 0) {
				d = make_ulonglong2(w.start, w.at);
				if (w.start == v) s = make_ulonglong2(1, w.n_node + (u64)k - 1);
			} else if (r == 0) { d.y = UW_DEC_CYCLE; ++cyc; }
			else ++bad;
		}
		dec[v] = d;
		sc[v] = s;
	}
	cyc = wave_sum(cyc); bad = wave_sum(bad);
	if ((threadIdx.x & (UW_WAVE - 1)) == 0) {
		if (cyc) atomicAdd(tally + UWT_CYCLE, cyc);
		if (bad) atomicAdd(tally + UWT_BAD, bad);
	}
}

/* the exclusive scan of a (u64, u64) array in place (../layer/layer_dev.h): tiles of UW_TILE, their sums scanned by one workgroup of UW_SCAN_THREADS */
__global__ __launch_bounds__(UW_THREADS)
void k_uw_tile_sum(const v2 *__restrict__ sc, u64 n, v2 *__restrict__ tsum) { tile_sum<UW_THREADS, UW_ITEMS, v2, AddV2>(sc, n, tsum); }
__global__ __launch_bounds__(UW_SCAN_THREADS)
void k_uw_tile_scan(v2 *__restrict__ tsum, u64 m) { tile_scan<UW_SCAN_THREADS, v2, AddV2>(tsum, m); }
__global__ __launch_bounds__(UW_THREADS)
void k_uw_scan_apply(v2 *__restrict__ sc, u64 n, const v2 *__restrict__ tsum) { scan_apply<UW_THREADS, UW_ITEMS, v2, AddV2>(sc, n, tsum); }

/* the open unitigs: sc[e] = (j, off) of start node e.  A place outside the arrays (inconsistent links) is tallied, not written */
__global__ __launch_bounds__(UW_THREADS)
void k_uw_emit(const uw_node_t *__restrict__ rec, const uw_pair_t *__restrict__ fin, const v2 *__restrict__ dec, const v2 *__restrict__ sc, u64 n, int k,
               v2 *__restrict__ map, uw_desc_t *__restrict__ desc, u64 n_desc, char *__restrict__ bases, u64 n_bases, u64 *__restrict__ tally)
{
	u64 bad = 0;
	for (u64 v = (u64)blockIdx.x * UW_THREADS + threadIdx.x; v < n; v += (u64)gridDim.x * UW_THREADS) {
		const v2 d = dec[v];
		if (d.x == UW_NONE) {
			if (d.y != UW_DEC_CYCLE) map[v] = make_ulonglong2(UW_NONE, 0);
			continue;
		}
		if (d.x >= n) { ++bad; continue; }
		const v2 se = sc[d.x];
		const u64 j = se.x, off = se.y, p = d.y >> 1;
		const int dir = (int)(d.y & 1);
		if (j >= n_desc || off + (u64)k - 1 + p >= n_bases) { ++bad; continue; }
		const uw_node_t r = ld_node(rec + v);
		map[v] = make_ulonglong2(j, d.y);
		atomicAdd(reinterpret_cast<u64*>(&desc[j].kc), (u64)r.count);
		if (p == 0) {
			const uw_pair_t a = ld_pair(fin + 2 * v), b = ld_pair(fin + 2 * v + 1);
			*reinterpret_cast<v2*>(&desc[j].off) = make_ulonglong2(off, a.dist + b.dist + 1);
			desc[j].first = v << 1;
			for (int i = 0; i < k; ++i) bases[off + i] = uw_base_at(r.x, dir, k, i);
		} else bases[off + (u64)k - 1 + p] = uw_last_base(r.x, dir, k);
	}
	bad = wave_sum(bad);
	if ((threadIdx.x & (UW_WAVE - 1)) == 0 && bad) atomicAdd(tally + UWT_BAD, bad);
}

__global__ __launch_bounds__(UW_THREADS)
void k_uw_cyc_flag(const v2 *__restrict__ dec, u64 n, v2 *__restrict__ sc)
{
	for (u64 v = (u64)blockIdx.x * UW_THREADS + threadIdx.x; v < n; v += (u64)gridDim.x * UW_THREADS) {
		const v2 d = dec[v];
		sc[v] = make_ulonglong2(d.x == UW_NONE && d.y == UW_DEC_CYCLE ? 1 : 0, 0);
	}
}

/* sc[v].x = the number of cycle nodes in front of v: idx[] and out[] in listing order */
__global__ __launch_bounds__(UW_THREADS)
void k_uw_cyc_gather(const uw_node_t *__restrict__ rec, const v2 *__restrict__ dec, const v2 *__restrict__ sc, u64 n, u64 *__restrict__ idx, uw_node_t *__restrict__ out, u64 cap)
{
	for (u64 v = (u64)blockIdx.x * UW_THREADS + threadIdx.x; v < n; v += (u64)gridDim.x * UW_THREADS) {
		const v2 d = dec[v];
		if (d.x != UW_NONE || d.y != UW_DEC_CYCLE) continue;
		const u64 at = sc[v].x;
		if (at >= cap) continue;
		idx[at] = v;
		reinterpret_cast<v2*>(out + at)[0] = reinterpret_cast<const v2*>(rec + v)[0];
		reinterpret_cast<v2*>(out + at)[1] = reinterpret_cast<const v2*>(rec + v)[1];
	}
}

__global__ __launch_bounds__(UW_THREADS)
void k_uw_cyc_scatter(const u64 *__restrict__ idx, const v2 *__restrict__ ent, u64 nc, u64 n, v2 *__restrict__ map)
{
	for (u64 i = (u64)blockIdx.x * UW_THREADS + threadIdx.x; i < nc; i += (u64)gridDim.x * UW_THREADS) {
		const u64 v = idx[i];
		if (v < n) map[v] = ent[i];
	}
}

/* ---------------- host ---------------- */

thread_local double g_ms[6];                                       /* of this thread's last call */

/* the exclusive scan of sc[0 .. n) in place; tot = the sums */
int scan_pairs(v2 *sc, u64 n, v2 *tsum, u64 tot[2])
{
	const u64 m = (n + UW_TILE - 1) / UW_TILE;
	YK_LAUNCH(k_uw_tile_sum, dim3((unsigned)m), dim3(UW_THREADS), 0, 0, sc, n, tsum);
	YK_LAUNCH(k_uw_tile_scan, dim3(1), dim3(UW_SCAN_THREADS), 0, 0, tsum, m);
	YK_LAUNCH(k_uw_scan_apply, dim3((unsigned)m), dim3(UW_THREADS), 0, 0, sc, n, tsum);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(tot, tsum + m, 16, hipMemcpyDeviceToHost));
	return 0;
}

}   // namespace

struct yakamd_uwalk {
	int k, dev;
	yakamd_gstat_t gst;
	yakamd_uwstat_t st;
	DevBuf map, desc, bases;
	std::vector<uw_desc_t> h_desc;
};

namespace {

/* the upper bounds known before the walk, from the graph's tallies: open unitigs = n_node - n_linked_side / 2; a cycle has at least two nodes, all
 * four sides of them linked */
struct Need { u64 n, n_desc, n_bases, n_tile, work, kept; };
Need need_of(const yakamd_gstat_t &g, int k)
{
	Need q;
	q.n = g.n_key;
	q.n_desc = g.n_node - g.n_linked_side / 2 + g.n_linked_side / 4;
	q.n_bases = g.n_node + q.n_desc * (u64)(k - 1);
	q.n_tile = (q.n + UW_TILE - 1) / UW_TILE;
	/* records, two pair buffers (the spare one holds dec[] and sc[] after the rounds), the cycle nodes' indices, the tile sums, the counters */
	q.work = q.n * (32 + 32 + 32 + 8) + (q.n_tile + 1) * 16 + (UW_MAX_ROUNDS + UWT_N) * 8 + 5 * 256;
	q.kept = q.n * 16 + q.n_desc * 32 + q.n_bases + 3 * 256;
	return q;
}

int walk_run(yakamd_uwalk *w, yakamd_graph_t **gp, yak_ch_t *h, int min_cnt)
{
	yakamd_graph_t *g = *gp;
	const int k = h->k;
	const Need q = need_of(w->gst, k);
	const u64 n = q.n;
	yakamd_uwstat_t &st = w->st;
	st.n_key = n; st.n_node = w->gst.n_node;
	HIPCK(hipGetDevice(&w->dev));                                  /* the table's: yakamd_graph_open made it current */
	size_t free_b = 0, total_b = 0;
	HIPCK(hipMemGetInfo(&free_b, &total_b));
	const char *lim = getenv("YAKAMD_WALK_MAX_BYTES");
	const u64 limit = lim && *lim ? strtoull(lim, 0, 10) : (u64)free_b;
	if (q.work + q.kept > limit)
		return fail("walk: %llu bytes of device memory are needed for %llu stored keys (%llu while it runs, %llu kept), %llu are free", q.work + q.kept, n, q.work, q.kept, limit);
	double t0 = now_ms();
	if (n == 0) return 0;
	DevBuf rec, pa, pb, idx, tsum, cnt;
	if (!rec.get(n * 32) || !pa.get(n * 32) || !pb.get(n * 32) || !idx.get(n * 8) || !tsum.get((q.n_tile + 1) * 16) || !cnt.get((UW_MAX_ROUNDS + UWT_N) * 8)
	    || !w->map.get(n * 16) || !w->desc.get(q.n_desc * 32) || !w->bases.get(q.n_bases))
		return fail("walk: no device memory for %llu bytes", q.work + q.kept);
	const double t_alloc = now_ms();
	if (yakamd_graph_nodes_dev(g, 0, 1 << h->pre, rec.p, (int64_t)n) != (int64_t)n) return fail_below(yakamd_last_error());
	const double t_rec = now_ms();
	yakamd_graph_close(g); *gp = 0;                                /* its scratch is not needed any more */
	g_ms[1] = now_ms() - t0;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] walk: allocation %.1f ms, records %.1f ms, graph close %.1f ms\n", t_alloc - t0, t_rec - t_alloc, now_ms() - t_rec);
	t0 = now_ms();

	/* ranking */
	u64 *d_cnt = (u64*)cnt.p, *d_tally = d_cnt + UW_MAX_ROUNDS;
	HIPCK(hipMemset(d_cnt, 0, (UW_MAX_ROUNDS + UWT_N) * 8));
	uw_pair_t *src = (uw_pair_t*)pa.p, *dst = (uw_pair_t*)pb.p;
	const uw_node_t *d_rec = (const uw_node_t*)rec.p;
	YK_LAUNCH(k_uw_init, dim3(grid_for(n, UW_THREADS)), dim3(UW_THREADS), 0, 0, d_rec, n, (uint32_t)min_cnt, src);
	for (;;) {
		if (st.rounds >= UW_MAX_ROUNDS) return fail("walk: the ranking did not end in %d rounds", (int)UW_MAX_ROUNDS);
		YK_LAUNCH(k_uw_jump, dim3(grid_for(2 * n, UW_THREADS)), dim3(UW_THREADS), 0, 0, (const uw_pair_t*)src, dst, 2 * n, d_cnt + st.rounds);
		HIPCK(hipGetLastError());
		u64 finished = 0;
		HIPCK(hipMemcpy(&finished, d_cnt + st.rounds, 8, hipMemcpyDeviceToHost));
		++st.rounds;
		std::swap(src, dst);
		if (finished == 0) break;
	}
	g_ms[2] = now_ms() - t0; t0 = now_ms();

	/* numbering and bases of the open unitigs; the spare pair buffer holds dec[] and sc[] */
	const uw_pair_t *fin = src;
	v2 *dec = (v2*)dst, *sc = dec + n, *d_map = (v2*)w->map.p;
	uw_desc_t *d_desc = (uw_desc_t*)w->desc.p;
	YK_LAUNCH(k_uw_decide, dim3(grid_for(n, UW_THREADS)), dim3(UW_THREADS), 0, 0, fin, n, k, dec, sc, d_tally);
	u64 tot[2], tally[UWT_N];
	if (scan_pairs(sc, n, (v2*)tsum.p, tot)) return -1;
	HIPCK(hipMemcpy(tally, d_tally, sizeof tally, hipMemcpyDeviceToHost));
	st.n_open = tot[0];
	const u64 open_len = tot[1], nc = tally[UWT_CYCLE];
	if (tally[UWT_BAD] || st.n_open > q.n_desc || open_len > q.n_bases || nc > n)
		return fail("walk: the links of %llu nodes do not lead to an end node each way", tally[UWT_BAD]);
	HIPCK(hipMemset(d_desc, 0, q.n_desc * 32 < 256 ? 256 : q.n_desc * 32));
	YK_LAUNCH(k_uw_emit, dim3(grid_for(n, UW_THREADS)), dim3(UW_THREADS), 0, 0, d_rec, fin, (const v2*)dec, (const v2*)sc, n, k, d_map, d_desc, st.n_open, (char*)w->bases.p, open_len, d_tally);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(tally, d_tally, sizeof tally, hipMemcpyDeviceToHost));
	if (tally[UWT_BAD]) return fail("walk: %llu nodes have no place in their unitig", tally[UWT_BAD]);

	/* the cycles: their records alone go to the host, compacted in listing order; the pair buffer that held the final pairs is free now */
	u64 cyc_len = 0;
	if (nc) {
		uw_node_t *d_out = (uw_node_t*)src;
		YK_LAUNCH(k_uw_cyc_flag, dim3(grid_for(n, UW_THREADS)), dim3(UW_THREADS), 0, 0, (const v2*)dec, n, sc);
		if (scan_pairs(sc, n, (v2*)tsum.p, tot)) return -1;
		if (tot[0] != nc) return fail("walk: %llu nodes on cycles were tallied and %llu found", nc, tot[0]);
		YK_LAUNCH(k_uw_cyc_gather, dim3(grid_for(n, UW_THREADS)), dim3(UW_THREADS), 0, 0, d_rec, (const v2*)dec, (const v2*)sc, n, (u64*)idx.p, d_out, nc);
		HIPCK(hipGetLastError());
		std::vector<uw_node_t> h_rec;
		std::vector<uint64_t> h_idx;
		uwh_cycles_t cy;
		std::string err;
		try {
			h_rec.resize((size_t)nc); h_idx.resize((size_t)nc);
			HIPCK(hipMemcpy(h_rec.data(), d_out, nc * 32, hipMemcpyDeviceToHost));
			HIPCK(hipMemcpy(h_idx.data(), idx.p, nc * 8, hipMemcpyDeviceToHost));
			st.host_nodes = nc;
			if (uwh_cycles(h_rec.data(), h_idx.data(), nc, k, st.n_open, open_len, &cy, &err) != 0) return fail("walk: %s", err.c_str());
		} catch (const std::bad_alloc&) { return fail("walk: the %llu nodes on cycles do not fit the host's memory", nc); }
		st.n_cycle = cy.desc.size();
		cyc_len = cy.bases.size();
		if (st.n_open + st.n_cycle > q.n_desc || open_len + cyc_len > q.n_bases) return fail("walk: more cycles than the graph's tallies allow");
		HIPCK(hipMemcpy(d_desc + st.n_open, cy.desc.data(), st.n_cycle * 32, hipMemcpyHostToDevice));
		HIPCK(hipMemcpy((char*)w->bases.p + open_len, cy.bases.data(), cyc_len, hipMemcpyHostToDevice));
		HIPCK(hipMemcpy(d_out, cy.map.data(), nc * 16, hipMemcpyHostToDevice));
		YK_LAUNCH(k_uw_cyc_scatter, dim3(grid_for(nc, UW_THREADS)), dim3(UW_THREADS), 0, 0, (const u64*)idx.p, (const v2*)d_out, nc, n, d_map);
		HIPCK(hipGetLastError());
	}
	HIPCK(hipDeviceSynchronize());
	g_ms[3] = now_ms() - t0; t0 = now_ms();

	/* the descriptors come out for the tallies and the text */
	const u64 n_u = st.n_open + st.n_cycle;
	try { w->h_desc.resize((size_t)n_u); } catch (const std::bad_alloc&) { return fail("walk: the descriptors of %llu unitigs do not fit the host's memory", n_u); }
	if (n_u) HIPCK(hipMemcpy(w->h_desc.data(), d_desc, n_u * 32, hipMemcpyDeviceToHost));
	try { uwh_lengths(w->h_desc.data(), n_u, k, &st.sum_len, &st.max_len, &st.n50); } catch (const std::bad_alloc&) { return fail("walk: no host memory for the lengths"); }
	if (st.sum_len != open_len + cyc_len) return fail("walk: the descriptors hold %llu bases, the scan %llu", (u64)st.sum_len, open_len + cyc_len);
	g_ms[4] = now_ms() - t0;
	return 0;
}

}   // namespace

extern "C" const char *yakamd_walk_last_error(void) { return g_err; }
extern "C" void yakamd_uwalk_ms(double ms[6]) { for (int i = 0; i < 6; ++i) ms[i] = g_ms[i]; }

extern "C" yakamd_uwalk_t *yakamd_uwalk_open(yak_ch_t *h, int min_cnt)
{
	for (int i = 0; i < 6; ++i) g_ms[i] = 0;
	const double t0 = now_ms();
	yakamd_graph_t *g = yakamd_graph_open(h, min_cnt);
	if (!g) { fail_below(yakamd_last_error()); return 0; }
	struct Graph { yakamd_graph_t *g; ~Graph() { yakamd_graph_close(g); } } G{ g };
	yakamd_uwalk_t *w = new (std::nothrow) yakamd_uwalk_t();
	if (!w) { fail("walk: no memory"); return 0; }
	w->k = h->k; w->dev = 0;
	memset(&w->st, 0, sizeof w->st);
	if (yakamd_graph_stats(g, &w->gst) != 0) { fail_below(yakamd_last_error()); delete w; return 0; }
	g_ms[0] = now_ms() - t0;
	if (walk_run(w, &G.g, h, min_cnt) != 0) { delete w; return 0; }
	return w;
}

extern "C" void yakamd_uwalk_close(yakamd_uwalk_t *w)
{
	if (!w) return;
	OnDevice dev(w->dev);
	delete w;
}

extern "C" int yakamd_uwalk_stats(yakamd_uwalk_t *w, yakamd_uwstat_t *st)
{
	if (!w || !st) return fail("walk stats: no walk, or no place for them");
	*st = w->st;
	return 0;
}

extern "C" int yakamd_uwalk_gstat(yakamd_uwalk_t *w, yakamd_gstat_t *st)
{
	if (!w || !st) return fail("walk gstat: no walk, or no place for them");
	*st = w->gst;
	return 0;
}

/* entries of 16 and 32 bytes must be aligned, single bases need not be */
static int64_t w_out(yakamd_uwalk_t *w, const void *src, u64 n, u64 each, void *d, int64_t cap, const char *what)
{
	return copy_out(w != 0, w ? w->dev : 0, src, n, each, d, cap, what, "walk", each > 1 ? "the entries" : 0);
}
extern "C" int64_t yakamd_uwalk_map_dev(yakamd_uwalk_t *w, void *d, int64_t cap) { return w_out(w, w ? w->map.p : 0, w ? w->st.n_key : 0, 16, d, cap, "walk map"); }
extern "C" int64_t yakamd_uwalk_desc_dev(yakamd_uwalk_t *w, void *d, int64_t cap) { return w_out(w, w ? w->desc.p : 0, w ? w->st.n_open + w->st.n_cycle : 0, 32, d, cap, "walk desc"); }
extern "C" int64_t yakamd_uwalk_bases_dev(yakamd_uwalk_t *w, void *d, int64_t cap) { return w_out(w, w ? w->bases.p : 0, w ? w->st.sum_len : 0, 1, d, cap, "walk bases"); }

/* the command: the walk, then the text from the descriptors and, for the FASTA, the bases */
extern "C" int yakamd_unitigs_dev(const yakamd_ugopt_t *opt, yak_ch_t *ch, const char *out_fn)
{
	if (!opt) return fail("yakamd_unitigs_dev: no options");
	WalkGuard W{ yakamd_uwalk_open(ch, opt->min_cnt) };
	yakamd_uwalk_t *w = W.p;
	if (!w) return -1;
	const yakamd_uwstat_t &u = w->st;
	double t0 = now_ms();
	std::string bases;
	if (!opt->stats_only && u.sum_len) {
		try { bases.resize((size_t)u.sum_len); } catch (const std::bad_alloc&) { return fail("yakamd_unitigs_dev: %llu bases do not fit the host's memory", (u64)u.sum_len); }
		OnDevice dev(w->dev);
		HIPCK(hipMemcpy(&bases[0], w->bases.p, (size_t)u.sum_len, hipMemcpyDeviceToHost));
	}
	g_ms[4] += now_ms() - t0; t0 = now_ms();
	OutFile of(out_fn);
	FILE *out = of.f;
	if (!out) return fail("yakamd_unitigs_dev: cannot write '%s'", of.name);
	bool ok = true;
	if (opt->stats_only) {
		const yakamd_gstat_t &s = w->gst;
		fprintf(out, "#unitigs\tk=%d\tmin_cnt=%d\n", w->k, opt->min_cnt);
		fprintf(out, "N\t%llu\t%llu\t%llu\t%llu\n", (u64)s.n_key, (u64)s.n_node, (u64)s.n_arc, (u64)s.n_linked_side);
		for (int l = 0; l < 5; ++l)
			for (int r = 0; r < 5; ++r)
				if (s.deg[l][r]) fprintf(out, "D\t%d\t%d\t%llu\n", l, r, (u64)s.deg[l][r]);
		fputs(uwh_u_line(u.n_open, u.n_cycle, u.sum_len, u.max_len, u.n50).c_str(), out);
	} else {
		try { ok = uwh_fasta(w->h_desc.data(), w->h_desc.size(), bases.data(), w->k, [&of](const std::string &t) { return of.write(t); }); }
		catch (const std::bad_alloc&) { return fail("yakamd_unitigs_dev: no host memory for the text"); }
	}
	if (!(of.finish() && ok)) return fail("yakamd_unitigs_dev: cannot write '%s'", of.name);
	g_ms[5] = now_ms() - t0;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] unitigs -g: graph %.1f ms, records %.1f ms, %llu rounds %.1f ms, numbering and bases %.1f ms, copies out %.1f ms, text %.1f ms\n",
		        g_ms[0], g_ms[1], (u64)u.rounds, g_ms[2], g_ms[3], g_ms[4], g_ms[5]);
	return 0;
}

LAYER_TALLY_EXPORTS(walk)
