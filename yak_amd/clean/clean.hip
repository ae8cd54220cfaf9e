/*
 * clean.hip -- libyak_amd_clean.so: the compacted de Bruijn graph of a count table cleaned on the GPU, its tips clipped and its simple bubbles
 * popped round by round (include/yak_amd_clean.h).  A layer above libyak_amd_bubble.so, libyak_amd_gfa.so, libyak_amd_walk.so
 * and libyak_amd.so: it calls their public functions only -- the getters of the walk, the links and the bubbles for the graph, and yak_ch_init,
 * yakamd_pass_begin, yakamd_feed_bases_dev, yakamd_pass_end, yak_ch_subtract, yak_ch_shrink and yak_ch_dump for the table -- and owns its device
 * memory (hipMalloc / hipFree).  The per-thread steps are those of clean_step.h, the texts those of clean_text.h; every launch goes through
 * YK_LAUNCH of ../csrc/tally.h into this library's own tally (yakamd_clean_tally_*).  The host scaffolding and the scan are those of
 * ../layer/layer_host.h and ../layer/layer_dev.h, which the layers share.
 *
 *   k_cln_first        a thread per link: the list is checked as it is read, the first link of a run writes runs[from] = (its index, their
 *                      number), as k_bub_first does
 *   k_cln_tips         a thread per unitig: the clip rule (cl_tip); wo[j] = (why, the anchor end), one 16-byte store; tips clipped, their nodes and
 *                      the candidates kept are summed per wave, one LDS atomic per wave, one 64-bit global atomic per workgroup and counter
 *   k_cln_pops         a thread per bubble record: the pop rule (cl_pop); wo[loser] = (2, the winning arm's end) -- an arm belongs to one bubble,
 *                      so the stores do not collide; arms popped, their nodes and the bubbles kept tallied the same way
 *   k_cln_find<COUNT>  a thread per unitig: cnt[j] = (1, n_node + k) for a removed unitig, (0, 0) otherwise
 *   k_cln_tile_sum, k_cln_tile_scan, k_cln_scan_apply
 *                      the exclusive scan of cnt[] in place, both words at once: tiles of 1024, their sums scanned by one workgroup
 *   k_cln_find<EMIT>   a removed unitig writes its record at its rank, three 16-byte stores
 *   k_cln_image        a wave per record: the lanes stride over the n_node + k - 1 bases of the unitig and copy them to img[off ..], one lane
 *                      writes '\n' behind them
 * All results are addressed by unitig and rank; the tallies are integer sums; all stores are vector stores.
 */
#include "yak.h"
#include "yak_amd_clean.h"
#define LAYER_NAME "clean"
#include "../layer/layer_host.h"
#include "../layer/layer_dev.h"
#include "clean_step.h"
#include "clean_text.h"

static_assert(sizeof(yakamd_udesc_t) == sizeof(bb_desc_t) && sizeof(yakamd_ulink_t) == sizeof(bb_link_t) && sizeof(yakamd_bubble_t) == sizeof(bb_rec_t), "the records as declared");
static_assert(sizeof(yakamd_clean_rec_t) == 48 && sizeof(cl_rec_t) == 48 && sizeof(yakamd_cleanstat_t) == 64 && sizeof(yakamd_cleanround_t) == 72 &&
              sizeof(clt_round_t) == 72 && sizeof(yakamd_cleanopt_t) == 20, "the records as declared");

namespace {

enum { CL_THREADS = 256, CL_ITEMS = 4, CL_TILE = CL_THREADS * CL_ITEMS, CL_WAVE = 64, CL_WAVES = CL_THREADS / CL_WAVE };
/* the words of stat[]: tips clipped, their nodes, candidates kept; arms popped, their nodes, bubbles kept; then what does not fit: links of
 * k_cln_first, unitigs of k_cln_tips, records of k_cln_pops, unitigs of k_cln_find (a mark that is none, a rank outside the list), records of
 * k_cln_image */
enum { CLS_TIP = 0, CLS_TIP_NODES = 1, CLS_TIP_KEPT = 2, CLS_POP = 3, CLS_POP_NODES = 4, CLS_POP_KEPT = 5, CLS_BAD_LINK = 8, CLS_BAD_TIP = 9, CLS_BAD_POP = 10,
       CLS_BAD_FIND = 11, CLS_BAD_IMG = 12, CLS_N = 16 };
enum ClMode { COUNT = 0, EMIT = 1 };

/* three sums of a workgroup into stat[at .. at + 3): per wave, one LDS atomic per wave, one global atomic per workgroup and counter; s_t[] is zero
 * and the workgroup in step */
__device__ inline void tally3(u64 *s_t, u64 a, u64 b, u64 c, u64 *stat, int at)
{
	a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
	if ((threadIdx.x & (CL_WAVE - 1)) == 0) {
		if (a) atomicAdd(&s_t[0], a);
		if (b) atomicAdd(&s_t[1], b);
		if (c) atomicAdd(&s_t[2], c);
	}
	__syncthreads();
	if (threadIdx.x < 3 && s_t[threadIdx.x]) atomicAdd(stat + at + threadIdx.x, s_t[threadIdx.x]);
}
__device__ inline void tally_bad(u64 bad, u64 *stat, int at)
{
	bad = wave_sum(bad);
	if ((threadIdx.x & (CL_WAVE - 1)) == 0 && bad) atomicAdd(stat + at, bad);
}

__global__ __launch_bounds__(CL_THREADS)
void k_cln_first(const bb_link_t *__restrict__ links, u64 n_link, u64 n_end, bb_run_t *__restrict__ runs, u64 *stat)
{
	u64 bad = 0;
	for (u64 i = (u64)blockIdx.x * CL_THREADS + threadIdx.x; i < n_link; i += (u64)gridDim.x * CL_THREADS) {
		uint64_t e = 0;
		bb_run_t run;
		const int r = bb_first(links, n_link, i, n_end, &e, &run);
		if (r < 0) ++bad;
		if (r == 1) *reinterpret_cast<v2*>(runs + e) = make_ulonglong2(run.first, run.n);      /* e < n_end: bb_first has checked it */
	}
	tally_bad(bad, stat, CLS_BAD_LINK);
}

__global__ __launch_bounds__(CL_THREADS)
void k_cln_tips(const bb_desc_t *__restrict__ desc, u64 n_unitig, const bb_run_t *__restrict__ runs, const bb_link_t *__restrict__ links, u64 n_link, u64 tip_nodes,
                v2 *__restrict__ wo, u64 *stat)
{
	__shared__ u64 s_t[3];
	if (threadIdx.x < 3) s_t[threadIdx.x] = 0;
	__syncthreads();
	u64 tip = 0, nodes = 0, kept = 0, bad = 0;
	for (u64 j = (u64)blockIdx.x * CL_THREADS + threadIdx.x; j < n_unitig; j += (u64)gridDim.x * CL_THREADS) {
		uint64_t other, bd = 0;
		int cand;
		bb_desc_t u;
		const int why = cl_tip(desc, n_unitig, runs, links, n_link, j, tip_nodes, &other, &cand, &u, &bd);
		bad += bd;
		wo[j] = make_ulonglong2((u64)why, other);
		if (why == CL_TIP) { ++tip; nodes += u.n_node; }
		else if (cand) ++kept;
	}
	tally3(s_t, tip, nodes, kept, stat, CLS_TIP);
	tally_bad(bad, stat, CLS_BAD_TIP);
}

__global__ __launch_bounds__(CL_THREADS)
void k_cln_pops(const bb_rec_t *__restrict__ bub, u64 n_bubble, const bb_desc_t *__restrict__ desc, u64 n_unitig, u64 pop_pct, v2 *__restrict__ wo, u64 *stat)
{
	__shared__ u64 s_t[3];
	if (threadIdx.x < 3) s_t[threadIdx.x] = 0;
	__syncthreads();
	u64 pop = 0, nodes = 0, kept = 0, bad = 0;
	for (u64 i = (u64)blockIdx.x * CL_THREADS + threadIdx.x; i < n_bubble; i += (u64)gridDim.x * CL_THREADS) {
		bb_rec_t r;
		const v2 *in = reinterpret_cast<const v2*>(bub + i);
		const v2 a = in[1], n = in[2], c = in[3];                      /* the arms, their nodes and counts: three 16-byte loads */
		r.arm[0] = a.x; r.arm[1] = a.y; r.n_node[0] = n.x; r.n_node[1] = n.y; r.kc[0] = c.x; r.kc[1] = c.y;
		uint64_t lo, hi, n_lo, kc_lo;
		const int p = cl_pop(&r, desc, n_unitig, pop_pct, &lo, &hi, &n_lo, &kc_lo);
		if (p < 0) { ++bad; continue; }
		if (p) { wo[lo >> 1] = make_ulonglong2((u64)CL_POP, hi); ++pop; nodes += n_lo; }     /* lo >> 1 < n_unitig: cl_pop has checked it */
		else ++kept;
	}
	tally3(s_t, pop, nodes, kept, stat, CLS_POP);
	tally_bad(bad, stat, CLS_BAD_POP);
}

/* COUNT: cnt[j] = (1, n_node + k) iff unitig j goes.  EMIT: cnt[j] is (its rank in rec[0 .. n_rec), where its bases start in the image) */
template<int MODE> __global__ __launch_bounds__(CL_THREADS)
void k_cln_find(const v2 *__restrict__ wo, const bb_desc_t *__restrict__ desc, u64 n_unitig, int k, v2 *__restrict__ cnt, cl_rec_t *__restrict__ rec, u64 n_rec, u64 *stat)
{
	u64 bad = 0;
	for (u64 j = (u64)blockIdx.x * CL_THREADS + threadIdx.x; j < n_unitig; j += (u64)gridDim.x * CL_THREADS) {
		const v2 w = wo[j];
		if (w.x > CL_POP) { ++bad; if (MODE == COUNT) cnt[j] = make_ulonglong2(0, 0); continue; }
		if (MODE == COUNT) {
			cnt[j] = w.x != CL_KEEP ? make_ulonglong2(1, desc[j].n_node + (u64)k) : make_ulonglong2(0, 0);
		} else if (w.x != CL_KEEP) {
			const v2 at = cnt[j];
			if (at.x >= n_rec) { ++bad; continue; }                        /* a rank outside the list: tallied, not written */
			const bb_desc_t u = desc[j];
			v2 *out = reinterpret_cast<v2*>(rec + at.x);
			out[0] = make_ulonglong2(j, w.x);
			out[1] = make_ulonglong2(u.n_node, u.kc);
			out[2] = make_ulonglong2(w.y, at.y);
		}
	}
	tally_bad(bad, stat, CLS_BAD_FIND);
}

/* the exclusive scan of cnt[] in place (../layer/layer_dev.h): tiles of CL_TILE, their sums scanned by one workgroup */
__global__ __launch_bounds__(CL_THREADS)
void k_cln_tile_sum(const v2 *__restrict__ cnt, u64 n, v2 *__restrict__ tsum) { tile_sum<CL_THREADS, CL_ITEMS, v2, AddV2>(cnt, n, tsum); }
__global__ __launch_bounds__(CL_THREADS)
void k_cln_tile_scan(v2 *__restrict__ tsum, u64 m) { tile_scan<CL_THREADS, v2, AddV2>(tsum, m); }
__global__ __launch_bounds__(CL_THREADS)
void k_cln_scan_apply(v2 *__restrict__ cnt, u64 n, const v2 *__restrict__ tsum) { scan_apply<CL_THREADS, CL_ITEMS, v2, AddV2>(cnt, n, tsum); }

/* a wave per record: the unitig's bases and a newline into the image */
__global__ __launch_bounds__(CL_THREADS)
void k_cln_image(const cl_rec_t *__restrict__ rec, u64 n_rec, const bb_desc_t *__restrict__ desc, u64 n_unitig, const char *__restrict__ bases, u64 n_bases, int k,
                 char *__restrict__ img, u64 img_bytes, u64 *stat)
{
	const unsigned lane = threadIdx.x & (CL_WAVE - 1);
	u64 bad = 0;
	for (u64 i = (u64)blockIdx.x * CL_WAVES + threadIdx.x / CL_WAVE; i < n_rec; i += (u64)gridDim.x * CL_WAVES) {      /* uniform in the wave */
		cl_rec_t r;
		const v2 *in = reinterpret_cast<const v2*>(rec + i);
		const v2 a = in[0], b = in[1], c = in[2];
		r.unitig = a.x; r.why = a.y; r.n_node = b.x; r.kc = b.y; r.other = c.x; r.off = c.y;
		uint64_t src = 0, len = 0;
		if (cl_span(&r, desc, n_unitig, n_bases, img_bytes, k, &src, &len) != 0) { bad += lane == 0; continue; }
		for (u64 p = lane; p < len; p += CL_WAVE) img[r.off + p] = bases[src + p];     /* src + len <= n_bases, r.off + len < img_bytes: cl_span */
		if (lane == 0) img[r.off + len] = '\n';
	}
	tally_bad(bad, stat, CLS_BAD_IMG);
}

/* ---------------- host ---------------- */

thread_local double g_ms[8];                                       /* of this thread's last call, summed over its rounds */
enum { MS_WALK = 0, MS_LINKS = 1, MS_BUBBLES = 2, MS_DECIDE = 3, MS_IMAGE = 4, MS_DROP = 5, MS_SUBTRACT = 6, MS_TEXT = 7 };

}   // namespace

struct yakamd_clean_set {
	int k, dev;
	yakamd_cleanstat_t st;
	DevBuf rec, img;
};

namespace {

/* the options as a call may give them */
int opt_check(int tip_nodes, int pop_pct)
{
	if (tip_nodes < 0 || tip_nodes > YAKAMD_CLEAN_MAX_TIP_NODES) return fail("clean: tip_nodes = %d: it must be in [0, %d]", tip_nodes, YAKAMD_CLEAN_MAX_TIP_NODES);
	if (pop_pct < 0 || pop_pct > 100) return fail("clean: pop_pct = %d: it must be in [0, 100]", pop_pct);
	return 0;
}

/* what yakamd_clean_open refuses, before any device work */
int clean_check(yakamd_uwalk_t *w, yakamd_gfa_t *g, yakamd_bubble_set_t *b, int k, int tip_nodes, int pop_pct, yakamd_uwstat_t *us, yakamd_gfastat_t *gs, yakamd_bubstat_t *bs)
{
	if (!w) return fail("clean: no walk");
	if (!g) return fail("clean: no links");
	if (!b) return fail("clean: no bubbles");
	if (k < 3 || k > 31 || !(k & 1)) return fail("clean: k = %d: the graph is defined for an odd k in [3, 31]", k);
	if (opt_check(tip_nodes, pop_pct) != 0) return -1;
	if (yakamd_uwalk_stats(w, us) != 0) return fail_below(yakamd_walk_last_error());
	if (yakamd_gfa_stats(g, gs) != 0) return fail_below(yakamd_gfa_last_error());
	if (yakamd_bubble_stats(b, bs) != 0) return fail_below(yakamd_bubble_last_error());
	if (us->sum_len != us->n_node + (us->n_open + us->n_cycle) * (u64)(k - 1))
		return fail("clean: k = %d does not fit the walk: %llu bases in %llu unitigs of %llu nodes", k, (u64)us->sum_len, (u64)(us->n_open + us->n_cycle), (u64)us->n_node);
	if (gs->n_unitig != us->n_open + us->n_cycle || gs->n_open != us->n_open)
		return fail("clean: the links are those of %llu unitigs (%llu open), the walk has %llu (%llu open)", (u64)gs->n_unitig, (u64)gs->n_open,
		            (u64)(us->n_open + us->n_cycle), (u64)us->n_open);
	const int64_t n_bubble = yakamd_bubble_records_dev(b, 0, 0);
	if (n_bubble < 0) return fail_below(yakamd_bubble_last_error());
	if ((u64)n_bubble != bs->n_bubble || bs->n_bubble > 2 * gs->n_unitig || bs->n_fork > gs->n_open * 2 || 2 * bs->n_bubble > bs->n_fork)
		return fail("clean: the bubbles (%llu of %llu forks) are not those of these %llu unitigs", (u64)bs->n_bubble, (u64)bs->n_fork, (u64)gs->n_unitig);
	u64 forks = 0;
	for (int d = 2; d < 5; ++d) forks += gs->end_deg[d];
	if (forks != bs->n_fork) return fail("clean: the bubbles were called on a graph of %llu forks, the links have %llu", (u64)bs->n_fork, forks);
	return 0;
}

int clean_run(yakamd_clean_set *c, yakamd_uwalk_t *w, yakamd_gfa_t *g, yakamd_bubble_set_t *b, const yakamd_uwstat_t &us, const yakamd_gfastat_t &gs,
              const yakamd_bubstat_t &bs, int tip_nodes, int pop_pct)
{
	const int k = c->k;
	const u64 n_u = us.n_open + us.n_cycle, n_end = 2 * n_u, n_link = gs.n_link, n_bases = us.sum_len, n_bubble = bs.n_bubble;
	HIPCK(hipGetDevice(&c->dev));
	if (n_u == 0) return 0;
	double t0 = now_ms();

	/* copies of the walk's results, of the links and of the bubbles, through the getters */
	DevBuf desc, bases, links, bub;
	if (!desc.get(n_u * 32) || !bases.get(n_bases) || !links.get(n_link * 16) || !bub.get(n_bubble * sizeof(bb_rec_t)))
		return fail("clean: no device memory for %llu bytes", n_u * 32 + n_bases + n_link * 16 + n_bubble * 80);
	if (yakamd_uwalk_desc_dev(w, desc.p, (int64_t)n_u) != (int64_t)n_u || yakamd_uwalk_bases_dev(w, bases.p, (int64_t)n_bases) != (int64_t)n_bases)
		return fail_below(yakamd_walk_last_error());
	if (yakamd_gfa_links_dev(g, links.p, (int64_t)n_link) != (int64_t)n_link) return fail_below(yakamd_gfa_last_error());
	if (yakamd_bubble_records_dev(b, bub.p, (int64_t)n_bubble) != (int64_t)n_bubble) return fail_below(yakamd_bubble_last_error());
	const u64 m = (n_u + CL_TILE - 1) / CL_TILE;
	DevBuf runs, wo, cnt, tsum, stat;
	if (!runs.get(n_end * 16) || !wo.get(n_u * 16) || !cnt.get(n_u * 16) || !tsum.get((m + 1) * 16) || !stat.get(CLS_N * 8))
		return fail("clean: no device memory for %llu bytes", n_end * 16 + n_u * 32 + (m + 1) * 16);
	u64 *d_stat = (u64*)stat.p, h_stat[CLS_N];
	v2 *d_wo = (v2*)wo.p, *d_cnt = (v2*)cnt.p, *d_tsum = (v2*)tsum.p;
	const bb_desc_t *d_desc = (const bb_desc_t*)desc.p;
	const bb_link_t *d_links = (const bb_link_t*)links.p;
	HIPCK(hipMemset(runs.p, 0xff, n_end * 16));                    /* every end without a link */
	HIPCK(hipMemset(d_stat, 0, CLS_N * 8));

	YK_LAUNCH(k_cln_first, dim3(grid_for(n_link, CL_THREADS)), dim3(CL_THREADS), 0, 0, d_links, n_link, n_end, (bb_run_t*)runs.p, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[CLS_BAD_LINK])
		return fail("clean: %llu of the %llu links do not fit: the list is not sorted, names an end outside the %llu unitigs or gives an end more than 4 links",
		            h_stat[CLS_BAD_LINK], n_link, n_u);

	YK_LAUNCH(k_cln_tips, dim3(grid_for(n_u, CL_THREADS)), dim3(CL_THREADS), 0, 0, d_desc, n_u, (const bb_run_t*)runs.p, d_links, n_link, (u64)tip_nodes, d_wo, d_stat);
	YK_LAUNCH(k_cln_pops, dim3(grid_for(n_bubble, CL_THREADS)), dim3(CL_THREADS), 0, 0, (const bb_rec_t*)bub.p, n_bubble, d_desc, n_u, (u64)pop_pct, d_wo, d_stat);
	YK_LAUNCH(k_cln_find<COUNT>, dim3(grid_for(n_u, CL_THREADS)), dim3(CL_THREADS), 0, 0, (const v2*)d_wo, d_desc, n_u, k, d_cnt, (cl_rec_t*)0, (u64)0, d_stat);
	YK_LAUNCH(k_cln_tile_sum, dim3((unsigned)m), dim3(CL_THREADS), 0, 0, (const v2*)d_cnt, n_u, d_tsum);
	YK_LAUNCH(k_cln_tile_scan, dim3(1), dim3(CL_THREADS), 0, 0, d_tsum, m);
	YK_LAUNCH(k_cln_scan_apply, dim3((unsigned)m), dim3(CL_THREADS), 0, 0, d_cnt, n_u, (const v2*)d_tsum);
	HIPCK(hipGetLastError());
	u64 total[2] = { 0, 0 };
	HIPCK(hipMemcpy(total, d_tsum + m, 16, hipMemcpyDeviceToHost));
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[CLS_BAD_TIP]) return fail("clean: the links do not fit the unitigs (%llu unitigs)", h_stat[CLS_BAD_TIP]);
	if (h_stat[CLS_BAD_POP]) return fail("clean: %llu of the %llu bubble records name an arm outside the %llu unitigs, or one with other nodes or counts", h_stat[CLS_BAD_POP], n_bubble, n_u);
	const u64 n_rec = total[0], img_bytes = total[1];
	if (h_stat[CLS_BAD_FIND] || n_rec != h_stat[CLS_TIP] + h_stat[CLS_POP] || img_bytes != h_stat[CLS_TIP_NODES] + h_stat[CLS_POP_NODES] + n_rec * (u64)k)
		return fail("clean: %llu unitigs are marked for %llu tips and %llu arms (%llu bytes for %llu nodes)", n_rec, h_stat[CLS_TIP], h_stat[CLS_POP], img_bytes,
		            h_stat[CLS_TIP_NODES] + h_stat[CLS_POP_NODES]);
	if (h_stat[CLS_POP] + h_stat[CLS_POP_KEPT] != n_bubble) return fail("clean: %llu bubbles were decided, %llu were given", h_stat[CLS_POP] + h_stat[CLS_POP_KEPT], n_bubble);
	if (!c->rec.get(n_rec * sizeof(cl_rec_t))) return fail("clean: no device memory for %llu records", n_rec);
	YK_LAUNCH(k_cln_find<EMIT>, dim3(grid_for(n_u, CL_THREADS)), dim3(CL_THREADS), 0, 0, (const v2*)d_wo, d_desc, n_u, k, d_cnt, (cl_rec_t*)c->rec.p, n_rec, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[CLS_BAD_FIND]) return fail("clean: %llu unitigs have no place in the list of %llu records", h_stat[CLS_BAD_FIND], n_rec);
	g_ms[MS_DECIDE] += now_ms() - t0; t0 = now_ms();

	/* the image: a multiple of 4096 bytes, newlines behind the last record, for a feed that reads whole words */
	const u64 img_cap = (img_bytes + 4095) / 4096 * 4096 + 4096;
	if (!c->img.get(img_cap)) return fail("clean: no device memory for an image of %llu bytes", img_bytes);
	HIPCK(hipMemset(c->img.p, '\n', img_cap));
	YK_LAUNCH(k_cln_image, dim3(grid_for(n_rec * CL_WAVE, CL_THREADS)), dim3(CL_THREADS), 0, 0, (const cl_rec_t*)c->rec.p, n_rec, d_desc, n_u, (const char*)bases.p, n_bases, k,
	          (char*)c->img.p, img_bytes, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[CLS_BAD_IMG]) return fail("clean: %llu of the %llu removed unitigs do not lie inside the %llu bases, or their place not inside the image", h_stat[CLS_BAD_IMG], n_rec, n_bases);
	yakamd_cleanstat_t &st = c->st;
	st.n_tip = h_stat[CLS_TIP]; st.tip_nodes = h_stat[CLS_TIP_NODES]; st.n_tip_kept = h_stat[CLS_TIP_KEPT];
	st.n_pop = h_stat[CLS_POP]; st.pop_nodes = h_stat[CLS_POP_NODES]; st.n_pop_kept = h_stat[CLS_POP_KEPT];
	st.n_rec = n_rec; st.img_bytes = img_bytes;
	g_ms[MS_IMAGE] += now_ms() - t0;
	return 0;
}

yakamd_clean_set_t *clean_open(yakamd_uwalk_t *w, yakamd_gfa_t *g, yakamd_bubble_set_t *b, int k, int tip_nodes, int pop_pct, yakamd_uwstat_t *us, yakamd_gfastat_t *gs,
                               yakamd_bubstat_t *bs)
{
	if (clean_check(w, g, b, k, tip_nodes, pop_pct, us, gs, bs) != 0) return 0;
	yakamd_clean_set_t *c = new (std::nothrow) yakamd_clean_set_t();
	if (!c) { fail("clean: no memory"); return 0; }
	c->k = k; c->dev = 0;
	memset(&c->st, 0, sizeof c->st);
	if (clean_run(c, w, g, b, *us, *gs, *bs, tip_nodes, pop_pct) != 0) { delete c; return 0; }
	return c;
}

struct TableGuard { yak_ch_t *h; ~TableGuard() { if (h) yak_ch_destroy(h); } };

/* the options of a round or a command, tip_nodes resolved against the table's k */
int round_opt(const yakamd_cleanopt_t *o, yak_ch_t *h, const char *who, int *tip_nodes)
{
	if (!o) return fail("%s: no options", who);
	if (!h) return fail("%s: not an engine table", who);
	*tip_nodes = o->tip_nodes == -1 ? h->k : o->tip_nodes;
	if (o->min_cnt < 1 || o->min_cnt > YAK_MAX_COUNT) return fail("%s: min_cnt %d: it must be in [1, %d]", who, o->min_cnt, YAK_MAX_COUNT);
	if (o->max_rounds < 1 || o->max_rounds > 64) return fail("%s: max_rounds = %d: it must be in [1, 64]", who, o->max_rounds);
	return opt_check(*tip_nodes, o->pop_pct);
}

/* one round; list: the records of the removed unitigs, for the T and P lines */
int64_t round_run(yak_ch_t *h, int min_cnt, int tip_nodes, int pop_pct, yakamd_cleanround_t *st, std::vector<cl_rec_t> *list)
{
	yakamd_cleanround_t none;
	if (!st) st = &none;
	memset(st, 0, sizeof *st);
	double t0 = now_ms();
	WalkGuard W{ yakamd_uwalk_open(h, min_cnt) };
	if (!W.p) return fail_below(yakamd_walk_last_error());
	g_ms[MS_WALK] += now_ms() - t0; t0 = now_ms();
	Guard<yakamd_gfa_t, yakamd_gfa_close> G{ yakamd_gfa_open(W.p, h->k) };
	if (!G.p) return fail_below(yakamd_gfa_last_error());
	g_ms[MS_LINKS] += now_ms() - t0; t0 = now_ms();
	Guard<yakamd_bubble_set_t, yakamd_bubble_close> B{ yakamd_bubble_open(W.p, G.p, h->k) };
	if (!B.p) return fail_below(yakamd_bubble_last_error());
	g_ms[MS_BUBBLES] += now_ms() - t0;
	yakamd_uwstat_t us;
	yakamd_gfastat_t gs;
	yakamd_bubstat_t bs;
	Guard<yakamd_clean_set_t, yakamd_clean_close> C{ clean_open(W.p, G.p, B.p, h->k, tip_nodes, pop_pct, &us, &gs, &bs) };
	if (!C.p) return -1;
	B.close(); G.close(); W.close();                               /* their device memory is free for D */
	const yakamd_cleanstat_t &cs = C.p->st;
	st->n_key = us.n_key; st->n_unitig = gs.n_unitig; st->n_link = gs.n_link; st->n_bubble = bs.n_bubble;
	st->n_tip = cs.n_tip; st->tip_nodes = cs.tip_nodes; st->n_pop = cs.n_pop; st->pop_nodes = cs.pop_nodes;
	if (cs.n_rec == 0) return 0;                                   /* nothing goes: the table stays as it is, no D */
	t0 = now_ms();
	const u64 nodes = cs.tip_nodes + cs.pop_nodes;
	OnDevice dev(C.p->dev);
	if (list) {
		try { list->resize((size_t)cs.n_rec); } catch (const std::bad_alloc&) { return fail("clean: %llu records do not fit the host's memory", (u64)cs.n_rec); }
		HIPCK(hipMemcpy(list->data(), C.p->rec.p, (size_t)cs.n_rec * sizeof(cl_rec_t), hipMemcpyDeviceToHost));
	}
	TableGuard D{ yak_ch_init(h->k, h->pre, 0, 0) };
	if (!D.h) return fail_below(yakamd_last_error());
	int d_dev = -1;
	HIPCK(hipGetDevice(&d_dev));
	if (d_dev != C.p->dev) return fail("clean: the table lives on device %d and a new table opens on device %d: set YAKAMD_DEVICE to %d", C.p->dev, d_dev, C.p->dev);
	if (yakamd_pass_begin(D.h, 1) != 0) return fail_below(yakamd_last_error());
	const int fed = yakamd_feed_bases_dev(D.h, C.p->img.p, (int64_t)cs.img_bytes, 0);
	const int64_t n_new = yakamd_pass_end(D.h);                    /* closes the pass whatever the feed did */
	if (fed != 0 || n_new < 0) return fail_below(yakamd_last_error());
	D.h->tot += (uint64_t)n_new;
	if ((u64)n_new != nodes) return fail("clean: the drop image of %llu nodes gave %lld k-mers", nodes, (long long)n_new);
	g_ms[MS_DROP] += now_ms() - t0; t0 = now_ms();
	yak_ch_subtract(h, D.h, 0);
	if (h->tot > us.n_key || us.n_key - h->tot != nodes)
		return fail("clean: the table of %llu k-mers has %llu after %llu were to go", (u64)us.n_key, (u64)h->tot, nodes);
	st->removed = nodes;
	g_ms[MS_SUBTRACT] += now_ms() - t0;
	return (int64_t)nodes;
}

}   // namespace

extern "C" const char *yakamd_clean_last_error(void) { return g_err; }
extern "C" void yakamd_clean_ms(double ms[8]) { for (int i = 0; i < 8; ++i) ms[i] = g_ms[i]; }
extern "C" void yakamd_cleanopt_init(yakamd_cleanopt_t *o) { o->min_cnt = 1; o->tip_nodes = -1; o->pop_pct = 100; o->max_rounds = 8; o->list = 0; }

extern "C" yakamd_clean_set_t *yakamd_clean_open(yakamd_uwalk_t *w, yakamd_gfa_t *g, yakamd_bubble_set_t *b, int k, int tip_nodes, int pop_pct)
{
	for (int i = 0; i < 8; ++i) g_ms[i] = 0;
	yakamd_uwstat_t us;
	yakamd_gfastat_t gs;
	yakamd_bubstat_t bs;
	return clean_open(w, g, b, k, tip_nodes, pop_pct, &us, &gs, &bs);
}

extern "C" void yakamd_clean_close(yakamd_clean_set_t *c)
{
	if (!c) return;
	OnDevice dev(c->dev);
	delete c;
}

extern "C" int yakamd_clean_stats(yakamd_clean_set_t *c, yakamd_cleanstat_t *st)
{
	if (!c || !st) return fail("clean stats: no decisions, or no place for them");
	*st = c->st;
	return 0;
}

extern "C" int64_t yakamd_clean_records_dev(yakamd_clean_set_t *c, void *d, int64_t cap)
{
	return copy_out(c != 0, c ? c->dev : 0, c ? c->rec.p : 0, c ? c->st.n_rec : 0, sizeof(cl_rec_t), d, cap, "clean records", "decisions", "the entries");
}

extern "C" int64_t yakamd_clean_image_dev(yakamd_clean_set_t *c, void *d, int64_t cap)
{
	return copy_out(c != 0, c ? c->dev : 0, c ? c->img.p : 0, c ? c->st.img_bytes : 0, 1, d, cap, "clean image", "decisions", "the image");
}

extern "C" int64_t yakamd_clean_round(yak_ch_t *h, const yakamd_cleanopt_t *o, yakamd_cleanround_t *st)
{
	for (int i = 0; i < 8; ++i) g_ms[i] = 0;
	int tip_nodes = 0;
	if (round_opt(o, h, "yakamd_clean_round", &tip_nodes) != 0) return -1;
	return round_run(h, o->min_cnt, tip_nodes, o->pop_pct, st, 0);
}

/* the command: the shrink, the rounds, the dump and the report.  The first walk comes before either output: what it refuses leaves no file */
extern "C" int yakamd_clean(const yakamd_cleanopt_t *o, yak_ch_t *ch, const char *out_yak, const char *report_fn)
{
	for (int i = 0; i < 8; ++i) g_ms[i] = 0;
	int tip_nodes = 0;
	if (round_opt(o, ch, "yakamd_clean", &tip_nodes) != 0) return -1;
	if (!out_yak || !*out_yak) return fail("yakamd_clean: no name for the cleaned table");
	u64 n_in = 0;
	{
		WalkGuard probe{ yakamd_uwalk_open(ch, o->min_cnt) };          /* everything the walk refuses, before the table is touched */
		yakamd_uwstat_t us;
		if (!probe.p || yakamd_uwalk_stats(probe.p, &us) != 0) return fail_below(yakamd_walk_last_error());
		n_in = us.n_key;                                               /* a restored table does not say in `tot` how many keys it holds */
	}
	std::string text = clt_head(ch->k, o->min_cnt, tip_nodes, o->pop_pct);
	u64 n_shrunk = n_in, n_out = n_in;
	if (o->min_cnt > 1) { yak_ch_shrink(ch, o->min_cnt, YAK_MAX_COUNT, 0); n_shrunk = n_out = ch->tot; }
	u64 rounds = 0;
	try {
		for (int r = 1; r <= o->max_rounds; ++r) {
			yakamd_cleanround_t st;
			std::vector<cl_rec_t> list;
			const int64_t removed = round_run(ch, o->min_cnt, tip_nodes, o->pop_pct, &st, o->list ? &list : 0);
			if (removed < 0) return -1;
			const double t0 = now_ms();
			clt_round_t s;
			memcpy(&s, &st, sizeof s);
			text += clt_round((u64)r, s);
			if (!clt_records((u64)r, list.data(), list.size(), [&text](const std::string &t) { text += t; return true; })) return fail("yakamd_clean: a record of round %d is neither a tip nor an arm", r);
			rounds = (u64)r;
			n_out = st.n_key - st.removed;
			g_ms[MS_TEXT] += now_ms() - t0;
			if (removed == 0) break;
		}
		text += clt_last(rounds, n_in, n_shrunk, n_out);
	} catch (const std::bad_alloc&) { return fail("yakamd_clean: no host memory for the report"); }
	const double t0 = now_ms();
	if (yak_ch_dump(ch, out_yak) != 0) return fail("yakamd_clean: cannot write '%s'", out_yak);
	if (report_fn) {
		OutFile out(report_fn);
		if (!out.f) return fail("yakamd_clean: cannot write '%s'", out.name);
		const bool ok = out.write(text);
		if (!(out.finish() && ok)) return fail("yakamd_clean: cannot write '%s'", out.name);
	}
	g_ms[MS_TEXT] += now_ms() - t0;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] clean: %llu rounds, %llu -> %llu -> %llu k-mers: walk %.1f ms, links %.1f ms, bubbles %.1f ms, decisions %.1f ms, image %.1f ms, drop table %.1f ms, subtract %.1f ms, text %.1f ms\n",
		        rounds, n_in, n_shrunk, n_out, g_ms[0], g_ms[1], g_ms[2], g_ms[3], g_ms[4], g_ms[5], g_ms[6], g_ms[7]);
	return 0;
}

LAYER_TALLY_EXPORTS(clean)
