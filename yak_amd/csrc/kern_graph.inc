/* kern_graph.inc -- part of kernels.hip (one translation unit, included in this order): the de Bruijn graph of a count table, `yak-amd unitigs` (not
 * in the reference; DESIGN.md section 20).  A node is a stored canonical k-mer x (k odd, below 32) with a count of at least min_cnt.  Side 0 (R)
 * appends a base b, z = (x << 2 | b) & (4^k - 1); side 1 (L) prepends it, z = x >> 2 | b << 2 (k - 1); the neighbour is y = min(z, revcomp_k(z)),
 * and bit 4 s + b of a node's edge mask is set iff y is a node.  y faces x with side t: from R, t = L if y == z, else R; from L, t = R if y == z,
 * else L.  Side (x, s) is linked to (y, t) iff it has one edge, y != x and (y, t) has one edge.
 * The kernels run over the arena's slots themselves, so a key's slot is known.  A tile is GR_THREADS consecutive slots of one sub-table; sub-table p
 * has ceil(capacity / GR_THREADS) of them, tile0[p] = the tiles of the sub-tables before p.  A persistent grid: a workgroup owns a run of tiles, a
 * step takes one tile, lane t its slot t, so the sub-table is the same for the whole workgroup and only advances.
 *   k_graph_edges<F>  edges[slot] = the edge mask of the key in `slot` (0 where the slot is free or its key is no node): eight probes of the whole
 *                     image per node, k_hetmer's probe, F of them requested before the first is waited for (F = 4, two rounds, is the default; F = 8: all at once);
 *                     deg[l * 5 + r] += 1 per node of l left and r right edges
 *   k_graph_rank      wrank[w] = used slots of w's sub-table in the 32-slot words before word w: with key0[p] = the stored keys of the sub-tables
 *                     before p, a slot's listing index -- its place in yakamd_kmers_dev()'s order -- is key0[p] + wrank[slot / 32] + popcount(used
 *                     bits of the word below the slot).  off[p] is a multiple of 32: a word belongs to one sub-table
 *   k_graph_link<M>   per side of one edge a probe for the neighbour's slot and a look at its edge byte.  GR_COUNT: tally[GR_LINKED] += linked
 *                     sides.  GR_EMIT: the 32-byte record {x, link[0], link[1], count | edges << 32} of every stored key of the tiles at its listing
 *                     index less out_key0; link[s] = listing index of y << 1 | t, or ~0
 * All stores are vector stores, all tallies integer atomics: no result depends on the grid or on the order of the atomics. */
#define GR_THREADS 512
#define GR_LINKED 25
#define GR_NONE (~0ull)
enum { GR_COUNT = 0, GR_EMIT = 1 };

struct GrArgs {
	const u64 *tile0;          /* [P + 1] */
	const u64 *key0;           /* [P + 1] */
	uint8_t *edges;            /* [n_slots] */
	u32 *wrank;                /* [n_slots / 32] */
	u64 *tally;                /* [32]: deg[l * 5 + r], then GR_LINKED */
	u64 *out;                  /* EMIT: four words per record */
	u64 out_key0, out_n;       /* EMIT: the listing index of the first record, and their number */
	u64 t_lo, t_hi;            /* the tiles of this launch */
	u64 n_slots;
	int P, k, min_cnt;
	int tab;                   /* the table's sub-table directory in LDS (pre <= 12) */
};

/* the sub-table directory of the probes: from LDS (off | bits << 58, 63 = no capacity) or from the image */
struct GrDir {
	const u64 *s_dir;
	const u64 YK_GLOBAL *karena;
	ImgView img;
	u64 mask;
	u32 pmask;
	int tab;
};

__device__ __forceinline__ void gr_dir_fill(const GrArgs &a, const ImgView &img, u64 *s_dir)
{
	if (a.tab) for (u32 p = threadIdx.x; p < (u32)a.P; p += GR_THREADS) { const u32 b = img.bits[p]; s_dir[p] = img.off[p] | (u64)(b == YK_NOCAP ? 63u : b) << 58; }
	__syncthreads();
}

__device__ __forceinline__ GrDir gr_dir(const GrArgs &a, const ImgView &img, const u64 *s_dir)
{
	GrDir d;
	d.s_dir = s_dir; d.karena = yk_global(u64, img.keys); d.img = img; d.mask = (1ull << 2 * a.k) - 1; d.pmask = (1u << img.pre) - 1; d.tab = a.tab;
	return d;
}

/* one probe in three parts, so that several can be in flight: where y's chain starts; the first load; the walk along the chain */
struct GrProbe { u64 kid, aoff, kc; u32 idx, nmask, sub; bool live; };

__device__ __forceinline__ void gr_probe_begin(GrProbe &q, u64 y, bool want, const GrDir &d)
{
	q.kid = 0; q.aoff = 0; q.idx = 0; q.nmask = 0; q.sub = 0; q.kc = YK_EMPTY; q.live = false;
	if (!want) return;
	const u64 h = yk_hash64(y, d.mask);
	const u32 p = (u32)h & d.pmask;
	u64 off; u32 bits;
	if (d.tab) { const u64 e = d.s_dir[p]; off = e & ((1ull << 58) - 1); bits = (u32)(e >> 58); bits = bits == 63u ? YK_NOCAP : bits; }
	else { bits = d.img.bits[p]; off = d.img.off[p]; }
	if (bits == YK_NOCAP) return;
	q.live = true; q.sub = p; q.kid = h >> d.img.pre; q.aoff = off; q.nmask = (1u << bits) - 1; q.idx = yk_h2b((u32)q.kid, bits);
}

__device__ __forceinline__ void gr_probe_load(GrProbe &q, const GrDir &d) { if (q.live) q.kc = d.karena[q.aoff + q.idx]; }

/* the count of the probed key, 0 where it is not stored; q.aoff + q.idx = its slot */
__device__ __forceinline__ u32 gr_probe_end(GrProbe &q, const GrDir &d)
{
	if (!q.live) return 0;
	const u32 first = q.idx;
	while (q.kc != YK_EMPTY) {
		if (q.kc >> 10 == q.kid) return (u32)(q.kc & 1023u);
		q.idx = (q.idx + 1) & q.nmask;
		if (q.idx == first) break;
		q.kc = d.karena[q.aoff + q.idx];
	}
	q.live = false;
	return 0;
}

__device__ __forceinline__ u64 gr_ext(u64 x, int s, u32 b, int k, u64 mask) { return s == 0 ? ((x << 2 | b) & mask) : (x >> 2 | (u64)b << 2 * (k - 1)); }

/* the tile a workgroup works on: its sub-table, and the slot and state of this lane's key */
struct GrTile {
	int p;
	u64 slot;
	u32 usedw;                 /* the `used` word of the slot */
	bool valid, used;
};

__device__ __forceinline__ int gr_first_sub(const u64 YK_GLOBAL *tile0, int P, u64 t)   /* the last p <= P - 1 with tile0[p] <= t */
{
	int l = 0;
	for (int r = P; r - l > 1; ) { const int m = (l + r) >> 1; if (tile0[m] <= t) l = m; else r = m; }
	return l;
}

__device__ __forceinline__ GrTile gr_tile(const GrArgs &a, const ImgView &img, const u64 YK_GLOBAL *tile0, int &p, u64 t)
{
	while (p + 1 < a.P && tile0[p + 1] <= t) ++p;
	GrTile T;
	T.p = p; T.slot = 0; T.usedw = 0; T.valid = false; T.used = false;
	const u32 bits = yk_global(u32, img.bits)[p];
	if (bits == YK_NOCAP) return T;
	const u64 local = (t - tile0[p]) * GR_THREADS + threadIdx.x;
	T.slot = yk_global(u64, img.off)[p] + local;
	T.valid = local < (1ull << bits) && T.slot < a.n_slots;
	if (T.valid) { T.usedw = yk_global(u32, img.used)[T.slot >> 5]; T.used = (T.usedw >> (T.slot & 31) & 1u) != 0; }
	return T;
}

template <int F>
__global__ __launch_bounds__(GR_THREADS)
void k_graph_edges(GrArgs a, ImgView img)
{
	extern __shared__ __attribute__((aligned(16))) u64 s_gr[];
	__shared__ u32 s_deg[25];
	if (threadIdx.x < 25) s_deg[threadIdx.x] = 0;
	gr_dir_fill(a, img, s_gr);
	const GrDir dir = gr_dir(a, img, s_gr);
	const u64 YK_GLOBAL *tile0 = yk_global(u64, a.tile0);
	uint8_t YK_GLOBAL *edges = yk_global_rw(uint8_t, a.edges);
	const u64 n_t = a.t_hi - a.t_lo, per = (n_t + gridDim.x - 1) / gridDim.x;
	const u64 lo = a.t_lo + per * blockIdx.x, hi = lo + per < a.t_hi ? lo + per : a.t_hi;
	u32 n11 = 0;                                                   /* deg[1][1], the common case: counted per lane */
	int p = lo < hi ? gr_first_sub(tile0, a.P, lo) : 0;
	for (u64 t = lo; t < hi; ++t) {
		const GrTile T = gr_tile(a, img, tile0, p, t);
		u64 x = 0;
		bool node = false;
		if (T.used) {
			const u64 w = dir.karena[T.slot];
			node = (u32)(w & 1023u) >= (u32)a.min_cnt;
			x = yk_hash64_inv((w >> 10) << img.pre | (u64)T.p, dir.mask);
		}
		u32 e = 0;
#pragma unroll
		for (int g = 0; g < 8; g += F) {
			GrProbe q[F];
#pragma unroll
			for (int j = 0; j < F; ++j) {
				const u64 z = gr_ext(x, (g + j) >> 2, (u32)(g + j) & 3u, a.k, dir.mask), rc = hm_revcomp(z, a.k);
				gr_probe_begin(q[j], z < rc ? z : rc, node, dir);
			}
#pragma unroll
			for (int j = 0; j < F; ++j) gr_probe_load(q[j], dir);
#pragma unroll
			for (int j = 0; j < F; ++j) if (gr_probe_end(q[j], dir) >= (u32)a.min_cnt) e |= 1u << (g + j);
		}
		if (T.valid) edges[T.slot] = (uint8_t)e;
		if (node) {
			const u32 l = (u32)__popc(e >> 4), r = (u32)__popc(e & 15u);
			if (l == 1 && r == 1) ++n11;
			else atomicAdd(&s_deg[l * 5 + r], 1u);
		}
	}
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) n11 += __shfl_xor(n11, o);
	if ((threadIdx.x & (WAVE - 1)) == 0 && n11) atomicAdd(&s_deg[6], n11);
	__syncthreads();
	if (threadIdx.x < 25 && s_deg[threadIdx.x]) atomicAdd((unsigned long long*)a.tally + threadIdx.x, (unsigned long long)s_deg[threadIdx.x]);
}

/* one workgroup per sub-table: the exclusive scan of popcount(used word) over its words */
__global__ __launch_bounds__(256)
void k_graph_rank(GrArgs a, ImgView img)
{
	__shared__ u32 s_w[256 / WAVE];
	const int p = blockIdx.x;
	const u32 bits = img.bits[p];
	if (bits == YK_NOCAP) return;
	const u64 cap = 1ull << bits, w0 = img.off[p] >> 5, n_w = (cap + 31) >> 5;
	const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
	const u32 YK_GLOBAL *used = yk_global(u32, img.used);
	u32 YK_GLOBAL *wrank = yk_global_rw(u32, a.wrank);
	u32 run = 0;
	for (u64 base = 0; base < n_w; base += 256) {
		const u64 i = base + threadIdx.x;
		const bool in = i < n_w && ((w0 + i) << 5) < a.n_slots;
		u32 v = in ? used[w0 + i] : 0;
		if (cap < 32) v &= (1u << cap) - 1;
		const u32 c = (u32)__popc(v);
		u32 inc = c;
#pragma unroll
		for (int o = 1; o < WAVE; o <<= 1) { const u32 y = __shfl_up(inc, o); if (lane >= (u32)o) inc += y; }
		if (lane == WAVE - 1) s_w[wave] = inc;
		__syncthreads();
		u32 before = run, all = 0;
		for (u32 v2 = 0; v2 < 256 / WAVE; ++v2) { if (v2 < wave) before += s_w[v2]; all += s_w[v2]; }
		if (in) wrank[w0 + i] = before + inc - c;
		run += all;
		__syncthreads();                                          /* s_w is written again in the next round */
	}
}

template <int MODE>
__global__ __launch_bounds__(GR_THREADS)
void k_graph_link(GrArgs a, ImgView img)
{
	extern __shared__ __attribute__((aligned(16))) u64 s_gr[];
	gr_dir_fill(a, img, s_gr);
	const GrDir dir = gr_dir(a, img, s_gr);
	const u64 YK_GLOBAL *tile0 = yk_global(u64, a.tile0);
	const u64 YK_GLOBAL *key0 = yk_global(u64, a.key0);
	const uint8_t YK_GLOBAL *edges = yk_global(uint8_t, a.edges);
	const u32 YK_GLOBAL *wrank = yk_global(u32, a.wrank);
	const u32 YK_GLOBAL *usedv = yk_global(u32, img.used);
	const u64 n_t = a.t_hi - a.t_lo, per = (n_t + gridDim.x - 1) / gridDim.x;
	const u64 lo = a.t_lo + per * blockIdx.x, hi = lo + per < a.t_hi ? lo + per : a.t_hi;
	u32 n_linked = 0;
	int p = lo < hi ? gr_first_sub(tile0, a.P, lo) : 0;
	for (u64 t = lo; t < hi; ++t) {
		const GrTile T = gr_tile(a, img, tile0, p, t);
		u64 x = 0, link[2] = { GR_NONE, GR_NONE };
		u32 e = 0, cx = 0;
		if (T.used) {
			const u64 w = dir.karena[T.slot];
			cx = (u32)(w & 1023u);
			e = edges[T.slot];
			if (MODE == GR_EMIT || e) x = yk_hash64_inv((w >> 10) << img.pre | (u64)T.p, dir.mask);
		}
		GrProbe q[2];
		u32 face[2];
#pragma unroll
		for (int s = 0; s < 2; ++s) {
			const u32 nib = e >> 4 * s & 15u;
			const bool one = __popc(nib) == 1;
			const u64 z = gr_ext(x, s, one ? (u32)__ffs(nib) - 1 : 0u, a.k, dir.mask), rc = hm_revcomp(z, a.k);
			const u64 y = z < rc ? z : rc;
			face[s] = s == 0 ? (y == z ? 1u : 0u) : (y == z ? 0u : 1u);
			gr_probe_begin(q[s], y, one && y != x, dir);
		}
#pragma unroll
		for (int s = 0; s < 2; ++s) gr_probe_load(q[s], dir);
#pragma unroll
		for (int s = 0; s < 2; ++s) {
			if (gr_probe_end(q[s], dir) < (u32)a.min_cnt || !q[s].live) continue;
			const u64 ys = q[s].aoff + q[s].idx;
			if (__popc((u32)edges[ys] >> 4 * face[s] & 15u) != 1) continue;
			++n_linked;
			if (MODE == GR_EMIT)
				link[s] = (key0[q[s].sub] + wrank[ys >> 5] + (u64)__popc(usedv[ys >> 5] & ((1u << (ys & 31)) - 1))) << 1 | face[s];
		}
		if (MODE == GR_EMIT && T.used) {
			const u64 at = key0[T.p] - a.out_key0 + wrank[T.slot >> 5] + (u64)__popc(T.usedw & ((1u << (T.slot & 31)) - 1));
			if (at < a.out_n) {
				yk_u64x2 YK_GLOBAL *rec = (yk_u64x2 YK_GLOBAL*)a.out + at * 2;
				yk_u64x2 v0, v1;
				v0.x = x; v0.y = link[0]; v1.x = link[1]; v1.y = (u64)cx | (u64)e << 32;
				rec[0] = v0; rec[1] = v1;
			}
		}
	}
	if (MODE == GR_COUNT) {
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) n_linked += __shfl_xor(n_linked, o);
		if ((threadIdx.x & (WAVE - 1)) == 0 && n_linked) atomicAdd((unsigned long long*)a.tally + GR_LINKED, (unsigned long long)n_linked);
	}
}
