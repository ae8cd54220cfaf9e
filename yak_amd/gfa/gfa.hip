/*
 * gfa.hip -- libyak_amd_gfa.so: the links between the unitigs of a count table's de Bruijn graph made on the GPU, and the graph as GFA 1
 * (include/yak_amd_gfa.h).  A layer above libyak_amd_walk.so and libyak_amd.so: it calls their public functions only
 * (yakamd_uwalk_open / _stats / _gstat / _desc_dev / _bases_dev / _close, yakamd_walk_last_error) and owns its device memory
 * (hipMalloc / hipFree).  The per-thread steps are those of gfa_step.h, the texts those of gfa_text.h; every launch goes through YK_LAUNCH of
 * ../csrc/tally.h into this library's own tally (yakamd_gfa_tally_*).  The host scaffolding and the scan are those of ../layer/layer_host.h and
 * ../layer/layer_dev.h, which the three layers share.
 *
 *   k_gfa_ends         a thread per unitig: W of its two oriented ends into endw[], and for an open unitig the canonical k-mers of its first and
 *                      last node claimed in the end table (64-bit atomicCAS on the key word, the value stored beside it and read by later
 *                      launches only); a cycle's ends are marked.  A probe walk is bounded by the capacity: no free slot is tallied, never spun on
 *   k_gfa_links<COUNT> a thread per oriented end: the four Z, their canonical forms, four look-ups; the number of links into cnt[2j + o], the
 *                      tally end_deg[] through LDS with one 64-bit atomic per workgroup and bin.  A cycle's end counts 1
 *   k_gfa_tile_sum, k_gfa_tile_scan, k_gfa_scan_apply
 *                      the exclusive scan of cnt[] in place: tiles of 1024, their sums scanned by one workgroup
 *   k_gfa_links<EMIT>  the same decision again; an end writes its links at its offset, a 16-byte store each
 * All results are addressed by j, o and b; the tallies are integer sums (max_probe, a measurement, a maximum); all stores are vector stores.
 */
#include "yak.h"
#include "yak_amd_gfa.h"
#define LAYER_NAME "gfa"
#include "../layer/layer_host.h"
#include "../layer/layer_dev.h"
#include "gfa_step.h"
#include "gfa_text.h"

static_assert(sizeof(yakamd_udesc_t) == sizeof(gf_desc_t) && sizeof(yakamd_ulink_t) == sizeof(gf_link_t) && sizeof(gf_slot_t) == 16, "the records as declared");

namespace {

enum { GF_THREADS = 256, GF_ITEMS = 4, GF_TILE = GF_THREADS * GF_ITEMS, GF_WAVE = 64 };
/* the words of stat[]: end_deg[0 .. 4], the longest probe walk, unitigs whose descriptor or values do not fit, claims that met no free slot, claims
 * of a key that was there already */
enum { GFS_DEG = 0, GFS_PROBE = 5, GFS_BAD = 6, GFS_FULL = 7, GFS_DUP = 8, GFS_N = 16 };
enum GfMode { COUNT = 0, EMIT = 1 };

/* what a thread gathered, into stat[]: a wave's sums and its maximum by one atomic each */
__device__ inline void tally_out(u64 *stat, u64 probe, u64 bad, u64 full, u64 dup)
{
	probe = wave_max(probe); bad = wave_sum(bad); full = wave_sum(full); dup = wave_sum(dup);
	if ((threadIdx.x & (GF_WAVE - 1)) == 0) {
		if (probe) atomicMax(stat + GFS_PROBE, probe);
		if (bad) atomicAdd(stat + GFS_BAD, bad);
		if (full) atomicAdd(stat + GFS_FULL, full);
		if (dup) atomicAdd(stat + GFS_DUP, dup);
	}
}

__global__ __launch_bounds__(GF_THREADS)
void k_gfa_ends(const gf_desc_t *__restrict__ desc, u64 n_unitig, const char *__restrict__ bases, u64 n_bases, int k, gf_slot_t *slots, u64 cap,
                u64 *__restrict__ endw, u64 *stat)
{
	u64 probe = 0, bad = 0, full = 0, dup = 0;
	for (u64 j = (u64)blockIdx.x * GF_THREADS + threadIdx.x; j < n_unitig; j += (u64)gridDim.x * GF_THREADS) {
		const v2 a = reinterpret_cast<const v2*>(desc + j)[0], b = reinterpret_cast<const v2*>(desc + j)[1];
		gf_desc_t u;
		u.off = a.x; u.n_node = a.y; u.kc = b.x; u.first = b.y;
		gf_ends_t e;
		if (gf_ends(&u, j, bases, n_bases, k, &e) < 0) ++bad;          /* every offset is checked against n_bases in there */
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			if (i >= e.n_key) continue;
			uint64_t pr = 0;
			const int r = gf_claim(slots, cap, e.key[i], e.val[i], DevCas(), &pr);
			probe = pr > probe ? pr : probe;
			if (r == -1) ++full;
			if (r == -2) ++dup;
		}
		*reinterpret_cast<v2*>(endw + 2 * j) = make_ulonglong2(e.w[0], e.w[1]);
	}
	tally_out(stat, probe, bad, full, dup);
}

/* COUNT: cnt[e] = the links of oriented end e, end_deg[] tallied.  EMIT: cnt[e] is the offset of its links in links[0 .. n_link) */
template<int MODE> __global__ __launch_bounds__(GF_THREADS)
void k_gfa_links(const gf_slot_t *__restrict__ slots, u64 cap, const u64 *__restrict__ endw, u64 n_end, int k, u64 n_unitig, u64 *__restrict__ cnt,
                 gf_link_t *__restrict__ links, u64 n_link, u64 *stat)
{
	__shared__ unsigned s_deg[5];
	if (MODE == COUNT) {
		if (threadIdx.x < 5) s_deg[threadIdx.x] = 0;
		__syncthreads();
	}
	u64 probe = 0, bad = 0;
	for (u64 e = (u64)blockIdx.x * GF_THREADS + threadIdx.x; e < n_end; e += (u64)gridDim.x * GF_THREADS) {
		uint64_t to[4], pr = 0, bd = 0;
		int open;
		const unsigned mask = gf_links(slots, cap, endw[e], e, k, n_unitig, to, &open, &pr, &bd);
		const unsigned n = (unsigned)__popc(mask);
		probe = pr > probe ? pr : probe;
		bad += bd;
		if (MODE == COUNT) {
			cnt[e] = n;
			if (open) atomicAdd(&s_deg[n], 1u);
		} else {
			u64 at = cnt[e];
			if (at > n_link || n > n_link - at) { ++bad; continue; }   /* an offset outside the list: tallied, not written */
#pragma unroll
			for (int b = 0; b < 4; ++b)
				if (mask >> b & 1u) *reinterpret_cast<v2*>(links + at++) = make_ulonglong2(e, to[b]);
		}
	}
	if (MODE == COUNT) {
		__syncthreads();
		if (threadIdx.x < 5 && s_deg[threadIdx.x]) atomicAdd(stat + GFS_DEG + threadIdx.x, (u64)s_deg[threadIdx.x]);
	}
	tally_out(stat, probe, bad, 0, 0);
}

/* the exclusive scan of cnt[] in place (../layer/layer_dev.h): tiles of GF_TILE, their sums scanned by one workgroup */
__global__ __launch_bounds__(GF_THREADS)
void k_gfa_tile_sum(const u64 *__restrict__ cnt, u64 n, u64 *__restrict__ tsum) { tile_sum<GF_THREADS, GF_ITEMS, u64, AddU64>(cnt, n, tsum); }
__global__ __launch_bounds__(GF_THREADS)
void k_gfa_tile_scan(u64 *__restrict__ tsum, u64 m) { tile_scan<GF_THREADS, u64, AddU64>(tsum, m); }
__global__ __launch_bounds__(GF_THREADS)
void k_gfa_scan_apply(u64 *__restrict__ cnt, u64 n, const u64 *__restrict__ tsum) { scan_apply<GF_THREADS, GF_ITEMS, u64, AddU64>(cnt, n, tsum); }

/* ---------------- host ---------------- */

thread_local double g_ms[4];                                       /* of this thread's last call */

}   // namespace

struct yakamd_gfa {
	int k, dev;
	yakamd_gfastat_t st;
	u64 n_bases;
	DevBuf links, desc, bases;                                   /* desc and bases are kept for the text of yakamd_unitigs_gfa only */
	std::vector<gf_desc_t> h_desc;
};

namespace {

/* what yakamd_gfa_open refuses, before any device work */
int gfa_check(yakamd_uwalk_t *w, int k, yakamd_uwstat_t *us)
{
	if (!w) return fail("gfa: no walk");
	if (k < 3 || k > 31 || !(k & 1)) return fail("gfa: k = %d: the links are defined for an odd k in [3, 31]", k);
	if (yakamd_uwalk_stats(w, us) != 0) return fail_below(yakamd_walk_last_error());
	if (us->sum_len != us->n_node + (us->n_open + us->n_cycle) * (u64)(k - 1))
		return fail("gfa: k = %d does not fit the walk: %llu bases in %llu unitigs of %llu nodes", k, (u64)us->sum_len, (u64)(us->n_open + us->n_cycle), (u64)us->n_node);
	return 0;
}

int gfa_run(yakamd_gfa *g, yakamd_uwalk_t *w, const yakamd_uwstat_t &us, bool keep)
{
	const int k = g->k;
	yakamd_gfastat_t &st = g->st;
	const u64 n_u = us.n_open + us.n_cycle, n_end = 2 * n_u;
	st.n_unitig = n_u; st.n_open = us.n_open; st.n_cycle = us.n_cycle;
	g->n_bases = us.sum_len;
	HIPCK(hipGetDevice(&g->dev));
	if (n_u == 0) return 0;
	double t0 = now_ms();

	/* copies of the walk's results, the descriptors on the host as well: the number of keys comes from them */
	const int rc = copy_walk(w, n_u, us.sum_len, 1, g->desc, g->bases, g->h_desc);
	if (rc) return rc < 0 ? -1 : fail("gfa: no device memory for %llu bytes", n_u * 32 + (u64)us.sum_len);
	u64 n_key = 0, n_open = 0;
	for (const gf_desc_t &u : g->h_desc) if (!(u.first & 1)) { ++n_open; n_key += u.n_node > 1 ? 2 : 1; }
	if (n_open != us.n_open) return fail("gfa: %llu descriptors of open unitigs, the walk states %llu", n_open, (u64)us.n_open);
	u64 cap = gf_capacity(n_key), want = 0;
	if (!slots_from_env("YAKAMD_GFA_SLOTS", n_key, &cap, &want)) return fail("gfa: YAKAMD_GFA_SLOTS = %llu: the end table has %llu keys", want, n_key);
	st.table_slots = cap;
	const double t_copy = now_ms();

	const u64 m = (n_end + GF_TILE - 1) / GF_TILE;
	DevBuf slots, endw, cnt, tsum, stat;
	if (!slots.get(cap * 16) || !endw.get(n_end * 8) || !cnt.get(n_end * 8) || !tsum.get((m + 1) * 8) || !stat.get(GFS_N * 8))
		return fail("gfa: no device memory for %llu bytes", cap * 16 + n_end * 16 + (m + 1) * 8);
	u64 *d_stat = (u64*)stat.p, *d_cnt = (u64*)cnt.p, *d_tsum = (u64*)tsum.p, h_stat[GFS_N];
	HIPCK(hipMemset(slots.p, 0xff, cap * 16));                     /* every key GF_EMPTY */
	HIPCK(hipMemset(d_stat, 0, GFS_N * 8));
	HIPCK(hipDeviceSynchronize());
	const double t_table = now_ms();
	YK_LAUNCH(k_gfa_ends, dim3(grid_for(n_u, GF_THREADS)), dim3(GF_THREADS), 0, 0, (const gf_desc_t*)g->desc.p, n_u, (const char*)g->bases.p, (u64)us.sum_len, k, (gf_slot_t*)slots.p, cap,
	          (u64*)endw.p, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[GFS_FULL]) return fail("gfa: %llu end nodes met no free slot among the %llu of the end table", h_stat[GFS_FULL], cap);
	if (h_stat[GFS_BAD]) return fail("gfa: the descriptors of %llu unitigs do not fit the %llu bases", h_stat[GFS_BAD], (u64)us.sum_len);
	if (h_stat[GFS_DUP]) return fail("gfa: %llu end nodes stand in two unitigs", h_stat[GFS_DUP]);
	const double t_ends = now_ms();
	if (!keep) { g->desc.drop(); g->bases.drop(); std::vector<gf_desc_t>().swap(g->h_desc); }     /* endw[] and the table hold all that the links need */
	g_ms[0] = now_ms() - t0;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] gfa: copies of the walk's results %.1f ms, allocation and clearing of %llu slots %.1f ms, k_gfa_ends %.1f ms, release %.1f ms\n",
		        t_copy - t0, cap, t_table - t_copy, t_ends - t_table, now_ms() - t_ends);
	t0 = now_ms();

	YK_LAUNCH(k_gfa_links<COUNT>, dim3(grid_for(n_end, GF_THREADS)), dim3(GF_THREADS), 0, 0, (const gf_slot_t*)slots.p, cap, (const u64*)endw.p, n_end, k, n_u, d_cnt, (gf_link_t*)0, (u64)0, d_stat);
	YK_LAUNCH(k_gfa_tile_sum, dim3((unsigned)m), dim3(GF_THREADS), 0, 0, (const u64*)d_cnt, n_end, d_tsum);
	YK_LAUNCH(k_gfa_tile_scan, dim3(1), dim3(GF_THREADS), 0, 0, d_tsum, m);
	YK_LAUNCH(k_gfa_scan_apply, dim3((unsigned)m), dim3(GF_THREADS), 0, 0, d_cnt, n_end, (const u64*)d_tsum);
	HIPCK(hipGetLastError());
	u64 n_link = 0;
	HIPCK(hipMemcpy(&n_link, d_tsum + m, 8, hipMemcpyDeviceToHost));
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	u64 ends = 0;
	for (int d = 0; d < 5; ++d) { st.end_deg[d] = h_stat[GFS_DEG + d]; ends += h_stat[GFS_DEG + d]; }
	if (h_stat[GFS_BAD] || ends != 2 * us.n_open || n_link > 4 * n_end)
		return fail("gfa: the end table does not fit the unitigs (%llu values, %llu of %llu ends of open unitigs)", h_stat[GFS_BAD], ends, 2 * (u64)us.n_open);
	st.n_link = n_link;
	g_ms[1] = now_ms() - t0; t0 = now_ms();

	if (!g->links.get(n_link * 16)) return fail("gfa: no device memory for %llu links", n_link);
	YK_LAUNCH(k_gfa_links<EMIT>, dim3(grid_for(n_end, GF_THREADS)), dim3(GF_THREADS), 0, 0, (const gf_slot_t*)slots.p, cap, (const u64*)endw.p, n_end, k, n_u, d_cnt, (gf_link_t*)g->links.p, n_link, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[GFS_BAD]) return fail("gfa: %llu ends have no place in the list of %llu links", h_stat[GFS_BAD], n_link);
	st.max_probe = h_stat[GFS_PROBE];
	g_ms[2] = now_ms() - t0;
	return 0;
}

yakamd_gfa_t *gfa_open(yakamd_uwalk_t *w, int k, bool keep)
{
	for (int i = 0; i < 4; ++i) g_ms[i] = 0;
	yakamd_uwstat_t us;
	if (gfa_check(w, k, &us) != 0) return 0;
	yakamd_gfa_t *g = new (std::nothrow) yakamd_gfa_t();
	if (!g) { fail("gfa: no memory"); return 0; }
	g->k = k; g->dev = 0; g->n_bases = 0;
	memset(&g->st, 0, sizeof g->st);
	if (gfa_run(g, w, us, keep) != 0) { delete g; return 0; }
	return g;
}

}   // namespace

extern "C" const char *yakamd_gfa_last_error(void) { return g_err; }
extern "C" void yakamd_gfa_ms(double ms[4]) { for (int i = 0; i < 4; ++i) ms[i] = g_ms[i]; }

extern "C" yakamd_gfa_t *yakamd_gfa_open(yakamd_uwalk_t *w, int k) { return gfa_open(w, k, false); }

extern "C" void yakamd_gfa_close(yakamd_gfa_t *g)
{
	if (!g) return;
	OnDevice dev(g->dev);
	delete g;
}

extern "C" int yakamd_gfa_stats(yakamd_gfa_t *g, yakamd_gfastat_t *st)
{
	if (!g || !st) return fail("gfa stats: no links, or no place for them");
	*st = g->st;
	return 0;
}

extern "C" int64_t yakamd_gfa_links_dev(yakamd_gfa_t *g, void *d, int64_t cap)
{
	return copy_out(g != 0, g ? g->dev : 0, g ? g->links.p : 0, g ? g->st.n_link : 0, 16, d, cap, "gfa links", "links", "the entries");
}

/* the command: the walk, the links, then the text from the tallies or from the descriptors, the bases and the links */
extern "C" int yakamd_unitigs_gfa(const yakamd_ugopt_t *opt, yak_ch_t *ch, const char *out_fn)
{
	if (!opt) return fail("yakamd_unitigs_gfa: no options");
	WalkGuard W{ yakamd_uwalk_open(ch, opt->min_cnt) };
	if (!W.p) return fail_below(yakamd_walk_last_error());
	Guard<yakamd_gfa_t, yakamd_gfa_close> G{ gfa_open(W.p, ch->k, !opt->stats_only) };
	yakamd_gfa_t *g = G.p;
	if (!g) return -1;
	const double t0 = now_ms();
	yakamd_gstat_t gs;
	yakamd_uwstat_t us;
	if (yakamd_uwalk_gstat(W.p, &gs) != 0 || yakamd_uwalk_stats(W.p, &us) != 0) return fail_below(yakamd_walk_last_error());
	std::string bases;
	std::vector<gf_link_t> links;
	if (!opt->stats_only) {
		try { bases.resize((size_t)g->n_bases); links.resize((size_t)g->st.n_link); }
		catch (const std::bad_alloc&) { return fail("yakamd_unitigs_gfa: %llu bases and %llu links do not fit the host's memory", g->n_bases, (u64)g->st.n_link); }
		OnDevice dev(g->dev);
		if (g->n_bases) HIPCK(hipMemcpy(&bases[0], g->bases.p, (size_t)g->n_bases, hipMemcpyDeviceToHost));
		if (g->st.n_link) HIPCK(hipMemcpy(links.data(), g->links.p, (size_t)g->st.n_link * 16, hipMemcpyDeviceToHost));
	}
	OutFile out(out_fn);
	if (!out.f) return fail("yakamd_unitigs_gfa: cannot write '%s'", out.name);
	bool ok = true;
	try {
		if (opt->stats_only)
			ok = out.write(gft_stats(gft_tallies(g->k, opt->min_cnt, gs, us), g->st.n_link, g->st.end_deg));
		else
			ok = gft_gfa(g->h_desc.data(), g->h_desc.size(), bases.data(), g->n_bases, links.data(), links.size(), g->k,
			             [&out](const std::string &t) { return out.write(t); });
	} catch (const std::bad_alloc&) { return fail("yakamd_unitigs_gfa: no host memory for the text"); }
	if (!(out.finish() && ok)) return fail("yakamd_unitigs_gfa: cannot write '%s'", out.name);
	g_ms[3] = now_ms() - t0;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] unitigs -G: %llu links of %llu unitigs: end table (%llu slots, longest probe %llu) %.1f ms, count and scan %.1f ms, emit %.1f ms, text %.1f ms\n",
		        (u64)g->st.n_link, (u64)g->st.n_unitig, (u64)g->st.table_slots, (u64)g->st.max_probe, g_ms[0], g_ms[1], g_ms[2], g_ms[3]);
	return 0;
}

LAYER_TALLY_EXPORTS(gfa)
