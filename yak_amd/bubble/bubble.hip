/*
 * bubble.hip -- libyak_amd_bubble.so: the simple bubbles of the compacted de Bruijn graph of a count table called on the GPU, its tips and forks
 * tallied (include/yak_amd_bubble.h).  A layer above libyak_amd_gfa.so, libyak_amd_walk.so and libyak_amd.so: it calls their
 * public functions only (yakamd_uwalk_open / _stats / _gstat / _desc_dev / _bases_dev / _close, yakamd_gfa_open / _stats / _links_dev / _close and
 * their last errors) and owns its device memory (hipMalloc / hipFree).  The per-thread steps are those of bubble_step.h, the texts those of
 * bubble_text.h; every launch goes through YK_LAUNCH of ../csrc/tally.h into this library's own tally (yakamd_bubble_tally_*).  The host
 * scaffolding and the scan are those of ../layer/layer_host.h and ../layer/layer_dev.h, which the layers share.
 *
 *   k_bub_first        a thread per link: the list is checked as it is read (sorted by `from`, every end below 2 n_unitig, at most 4 links an
 *                      end); the first link of a run counts the run and writes runs[from] = (its index, their number), one 16-byte store.  runs[]
 *                      is pre-set to none
 *   k_bub_find<COUNT>  a thread per oriented end: the definition applied (bb_find), cnt[e] = 1 for the reporting source of a bubble; forks, tips,
 *                      their nodes and the longest arm tallied through LDS with one 64-bit atomic per workgroup and counter
 *   k_bub_tile_sum, k_bub_tile_scan, k_bub_scan_apply
 *                      the exclusive scan of cnt[] in place: tiles of 1024, their sums scanned by one workgroup
 *   k_bub_find<EMIT>   the same decision again; a source writes src, sink, arm, n_node and kc at its rank, four 16-byte stores
 *   k_bub_classify     a wave per bubble: the type from n_node; for arms of one length the lanes stride over the positions of the two oriented
 *                      strings and sum the mismatches; one 16-byte store of hd and type, n_type through LDS
 * All results are addressed by end and rank; the tallies are integer sums and one maximum; all stores are vector stores.
 */
#include "yak.h"
#include "yak_amd_bubble.h"
#define LAYER_NAME "bubble"
#include "../layer/layer_host.h"
#include "../layer/layer_dev.h"
#include "bubble_step.h"
#include "bubble_text.h"

static_assert(sizeof(yakamd_udesc_t) == sizeof(bb_desc_t) && sizeof(yakamd_ulink_t) == sizeof(bb_link_t) && sizeof(bb_run_t) == 16, "the records as declared");
static_assert(sizeof(yakamd_bubble_t) == 80 && sizeof(bb_rec_t) == 80 && sizeof(yakamd_bubstat_t) == 64 && sizeof(bbt_stats_t) == 64, "the records as declared");

namespace {

enum { BB_THREADS = 256, BB_ITEMS = 4, BB_TILE = BB_THREADS * BB_ITEMS, BB_WAVE = 64, BB_WAVES = BB_THREADS / BB_WAVE };
/* the words of stat[]: the forks, the tips, their nodes, the longest arm, n_type[3]; then what does not fit: links of k_bub_first, ends of
 * k_bub_find (a run, a link or a rank outside its list), bubbles of k_bub_classify (an arm outside the bases, a byte that is no base) */
enum { BBS_FORK = 0, BBS_TIP = 1, BBS_TIP_NODES = 2, BBS_MAX_ARM = 3, BBS_TYPE = 4, BBS_BAD_LINK = 7, BBS_BAD_END = 8, BBS_BAD_ARM = 9, BBS_N = 16 };
enum BbMode { COUNT = 0, EMIT = 1 };

__global__ __launch_bounds__(BB_THREADS)
void k_bub_first(const bb_link_t *__restrict__ links, u64 n_link, u64 n_end, bb_run_t *__restrict__ runs, u64 *stat)
{
	u64 bad = 0;
	for (u64 i = (u64)blockIdx.x * BB_THREADS + threadIdx.x; i < n_link; i += (u64)gridDim.x * BB_THREADS) {
		uint64_t e = 0;
		bb_run_t run;
		const int r = bb_first(links, n_link, i, n_end, &e, &run);
		if (r < 0) ++bad;
		if (r == 1) *reinterpret_cast<v2*>(runs + e) = make_ulonglong2(run.first, run.n);      /* e < n_end: bb_first has checked it */
	}
	bad = wave_sum(bad);
	if ((threadIdx.x & (BB_WAVE - 1)) == 0 && bad) atomicAdd(stat + BBS_BAD_LINK, bad);
}

/* COUNT: cnt[e] = 1 iff end e reports a bubble, the tallies.  EMIT: cnt[e] is the rank of its bubble in rec[0 .. n_bubble) */
template<int MODE> __global__ __launch_bounds__(BB_THREADS)
void k_bub_find(const bb_desc_t *__restrict__ desc, u64 n_unitig, const bb_run_t *__restrict__ runs, const bb_link_t *__restrict__ links, u64 n_link, int k,
                u64 *__restrict__ cnt, bb_rec_t *__restrict__ rec, u64 n_bubble, u64 *stat)
{
	__shared__ u64 s_t[4];                                         /* forks, tips, their nodes, the longest arm */
	if (MODE == COUNT) {
		if (threadIdx.x < 4) s_t[threadIdx.x] = 0;
		__syncthreads();
	}
	const u64 n_end = 2 * n_unitig;
	u64 fork = 0, tip = 0, nodes = 0, arm = 0, bad = 0;
	for (u64 e = (u64)blockIdx.x * BB_THREADS + threadIdx.x; e < n_end; e += (u64)gridDim.x * BB_THREADS) {
		bb_rec_t r;
		unsigned flags;
		uint64_t tn, bd = 0;
		const int is = bb_find(desc, n_unitig, runs, links, n_link, e, k, &r, &flags, &tn, &bd);
		bad += bd;
		if (MODE == COUNT) {
			cnt[e] = (u64)is;
			fork += flags & BB_FORK ? 1 : 0;
			tip += flags & BB_TIP ? 1 : 0;
			nodes += tn;
			if (is) { const u64 m = r.n_node[0] > r.n_node[1] ? r.n_node[0] : r.n_node[1]; arm = m > arm ? m : arm; }
		} else if (is) {
			const u64 at = cnt[e];
			if (at >= n_bubble) { ++bad; continue; }                   /* a rank outside the list: tallied, not written */
			v2 *out = reinterpret_cast<v2*>(rec + at);
			out[0] = make_ulonglong2(r.src, r.sink);
			out[1] = make_ulonglong2(r.arm[0], r.arm[1]);
			out[2] = make_ulonglong2(r.n_node[0], r.n_node[1]);
			out[3] = make_ulonglong2(r.kc[0], r.kc[1]);
		}
	}
	if (MODE == COUNT) {
		fork = wave_sum(fork); tip = wave_sum(tip); nodes = wave_sum(nodes); arm = wave_max(arm);
		if ((threadIdx.x & (BB_WAVE - 1)) == 0) {
			if (fork) atomicAdd(&s_t[0], fork);
			if (tip) atomicAdd(&s_t[1], tip);
			if (nodes) atomicAdd(&s_t[2], nodes);
			if (arm) atomicMax(&s_t[3], arm);
		}
		__syncthreads();
		if (threadIdx.x < 3 && s_t[threadIdx.x]) atomicAdd(stat + BBS_FORK + threadIdx.x, s_t[threadIdx.x]);
		if (threadIdx.x == 3 && s_t[3]) atomicMax(stat + BBS_MAX_ARM, s_t[3]);
	}
	bad = wave_sum(bad);
	if ((threadIdx.x & (BB_WAVE - 1)) == 0 && bad) atomicAdd(stat + BBS_BAD_END, bad);
}

/* the exclusive scan of cnt[] in place (../layer/layer_dev.h): tiles of BB_TILE, their sums scanned by one workgroup */
__global__ __launch_bounds__(BB_THREADS)
void k_bub_tile_sum(const u64 *__restrict__ cnt, u64 n, u64 *__restrict__ tsum) { tile_sum<BB_THREADS, BB_ITEMS, u64, AddU64>(cnt, n, tsum); }
__global__ __launch_bounds__(BB_THREADS)
void k_bub_tile_scan(u64 *__restrict__ tsum, u64 m) { tile_scan<BB_THREADS, u64, AddU64>(tsum, m); }
__global__ __launch_bounds__(BB_THREADS)
void k_bub_scan_apply(u64 *__restrict__ cnt, u64 n, const u64 *__restrict__ tsum) { scan_apply<BB_THREADS, BB_ITEMS, u64, AddU64>(cnt, n, tsum); }

/* a wave per bubble: hd and type behind the eight words k_bub_find<EMIT> wrote */
__global__ __launch_bounds__(BB_THREADS)
void k_bub_classify(bb_rec_t *__restrict__ rec, u64 n_bubble, const bb_desc_t *__restrict__ desc, u64 n_unitig, const char *__restrict__ bases, u64 n_bases, int k,
                    u64 *stat)
{
	__shared__ unsigned s_t[4];                                    /* n_type[3], the bubbles that do not fit */
	if (threadIdx.x < 4) s_t[threadIdx.x] = 0;
	__syncthreads();
	const unsigned lane = threadIdx.x & (BB_WAVE - 1);
	for (u64 b = (u64)blockIdx.x * BB_WAVES + threadIdx.x / BB_WAVE; b < n_bubble; b += (u64)gridDim.x * BB_WAVES) {      /* uniform in the wave */
		const v2 a = reinterpret_cast<const v2*>(rec + b)[1], n = reinterpret_cast<const v2*>(rec + b)[2];
		const uint64_t arm[2] = { a.x, a.y };
		const u64 type = bb_type(n.x, n.y, k);
		u64 hd = BB_NONE, bad = 0;
		if (type != BB_I) {
			uint64_t off[2] = { 0, 0 }, len = 0, len2 = 0;
			if (bb_arm(desc, n_unitig, n_bases, arm[0], n.x, k, &off[0], &len) != 0 || bb_arm(desc, n_unitig, n_bases, arm[1], n.y, k, &off[1], &len2) != 0) {
				bad = lane == 0;
				len = 0;
			}
			u64 mis = 0;
			for (u64 p = lane; p < len; p += BB_WAVE) {
				const int m = bb_mismatch(bases, off, len, arm, p);
				if (m < 0) ++bad; else mis += (u64)m;
			}
			hd = wave_sum(mis);
			bad = wave_sum(bad);
		}
		if (lane == 0) {
			reinterpret_cast<v2*>(rec + b)[4] = make_ulonglong2(hd, type);
			atomicAdd(&s_t[type], 1u);
			if (bad) atomicAdd(&s_t[3], 1u);
		}
	}
	__syncthreads();
	if (threadIdx.x < 3 && s_t[threadIdx.x]) atomicAdd(stat + BBS_TYPE + threadIdx.x, (u64)s_t[threadIdx.x]);
	if (threadIdx.x == 3 && s_t[3]) atomicAdd(stat + BBS_BAD_ARM, (u64)s_t[3]);
}

/* ---------------- host ---------------- */

thread_local double g_ms[5];                                       /* of this thread's last call */

}   // namespace

struct yakamd_bubble_set {
	int k, dev;
	yakamd_bubstat_t st;
	u64 n_unitig, n_bases;
	DevBuf rec, desc, bases;                                     /* desc and bases are kept for the text of yakamd_bubbles only */
};

namespace {

/* what yakamd_bubble_open refuses, before any device work */
int bubble_check(yakamd_uwalk_t *w, yakamd_gfa_t *g, int k, yakamd_uwstat_t *us, yakamd_gfastat_t *gs)
{
	if (!w) return fail("bubble: no walk");
	if (!g) return fail("bubble: no links");
	if (k < 3 || k > 31 || !(k & 1)) return fail("bubble: k = %d: the bubbles are defined for an odd k in [3, 31]", k);
	if (yakamd_uwalk_stats(w, us) != 0) return fail_below(yakamd_walk_last_error());
	if (yakamd_gfa_stats(g, gs) != 0) return fail_below(yakamd_gfa_last_error());
	if (us->sum_len != us->n_node + (us->n_open + us->n_cycle) * (u64)(k - 1))
		return fail("bubble: k = %d does not fit the walk: %llu bases in %llu unitigs of %llu nodes", k, (u64)us->sum_len, (u64)(us->n_open + us->n_cycle), (u64)us->n_node);
	if (gs->n_unitig != us->n_open + us->n_cycle || gs->n_open != us->n_open)
		return fail("bubble: the links are those of %llu unitigs (%llu open), the walk has %llu (%llu open)", (u64)gs->n_unitig, (u64)gs->n_open,
		            (u64)(us->n_open + us->n_cycle), (u64)us->n_open);
	return 0;
}

int bubble_run(yakamd_bubble_set *b, yakamd_uwalk_t *w, yakamd_gfa_t *g, const yakamd_uwstat_t &us, const yakamd_gfastat_t &gs, bool keep)
{
	const int k = b->k;
	yakamd_bubstat_t &st = b->st;
	const u64 n_u = us.n_open + us.n_cycle, n_end = 2 * n_u, n_link = gs.n_link, n_bases = us.sum_len;
	b->n_unitig = n_u; b->n_bases = n_bases;
	HIPCK(hipGetDevice(&b->dev));
	if (n_u == 0) return 0;
	double t0 = now_ms();

	/* copies of the walk's results and of the links, through the getters */
	DevBuf links;
	if (!b->desc.get(n_u * 32) || !b->bases.get(n_bases) || !links.get(n_link * 16))
		return fail("bubble: no device memory for %llu bytes", n_u * 32 + n_bases + n_link * 16);
	if (yakamd_uwalk_desc_dev(w, b->desc.p, (int64_t)n_u) != (int64_t)n_u || yakamd_uwalk_bases_dev(w, b->bases.p, (int64_t)n_bases) != (int64_t)n_bases)
		return fail_below(yakamd_walk_last_error());
	if (yakamd_gfa_links_dev(g, links.p, (int64_t)n_link) != (int64_t)n_link) return fail_below(yakamd_gfa_last_error());
	const u64 m = (n_end + BB_TILE - 1) / BB_TILE;
	DevBuf runs, cnt, tsum, stat;
	if (!runs.get(n_end * 16) || !cnt.get(n_end * 8) || !tsum.get((m + 1) * 8) || !stat.get(BBS_N * 8))
		return fail("bubble: no device memory for %llu bytes", n_end * 24 + (m + 1) * 8);
	u64 *d_stat = (u64*)stat.p, *d_cnt = (u64*)cnt.p, *d_tsum = (u64*)tsum.p, h_stat[BBS_N];
	const bb_desc_t *d_desc = (const bb_desc_t*)b->desc.p;
	const bb_link_t *d_links = (const bb_link_t*)links.p;
	HIPCK(hipMemset(runs.p, 0xff, n_end * 16));                    /* every end without a link */
	HIPCK(hipMemset(d_stat, 0, BBS_N * 8));
	HIPCK(hipDeviceSynchronize());
	g_ms[0] = now_ms() - t0; t0 = now_ms();

	YK_LAUNCH(k_bub_first, dim3(grid_for(n_link, BB_THREADS)), dim3(BB_THREADS), 0, 0, d_links, n_link, n_end, (bb_run_t*)runs.p, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[BBS_BAD_LINK])
		return fail("bubble: %llu of the %llu links do not fit: the list is not sorted, names an end outside the %llu unitigs or gives an end more than 4 links",
		            h_stat[BBS_BAD_LINK], n_link, n_u);
	g_ms[1] = now_ms() - t0; t0 = now_ms();

	YK_LAUNCH(k_bub_find<COUNT>, dim3(grid_for(n_end, BB_THREADS)), dim3(BB_THREADS), 0, 0, d_desc, n_u, (const bb_run_t*)runs.p, d_links, n_link, k, d_cnt, (bb_rec_t*)0, (u64)0, d_stat);
	YK_LAUNCH(k_bub_tile_sum, dim3((unsigned)m), dim3(BB_THREADS), 0, 0, (const u64*)d_cnt, n_end, d_tsum);
	YK_LAUNCH(k_bub_tile_scan, dim3(1), dim3(BB_THREADS), 0, 0, d_tsum, m);
	YK_LAUNCH(k_bub_scan_apply, dim3((unsigned)m), dim3(BB_THREADS), 0, 0, d_cnt, n_end, (const u64*)d_tsum);
	HIPCK(hipGetLastError());
	u64 n_bubble = 0;
	HIPCK(hipMemcpy(&n_bubble, d_tsum + m, 8, hipMemcpyDeviceToHost));
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[BBS_BAD_END] || n_bubble > n_end)
		return fail("bubble: the links do not fit the unitigs (%llu ends, %llu bubbles of %llu ends)", h_stat[BBS_BAD_END], n_bubble, n_end);
	if (!b->rec.get(n_bubble * sizeof(bb_rec_t))) return fail("bubble: no device memory for %llu bubbles", n_bubble);
	YK_LAUNCH(k_bub_find<EMIT>, dim3(grid_for(n_end, BB_THREADS)), dim3(BB_THREADS), 0, 0, d_desc, n_u, (const bb_run_t*)runs.p, d_links, n_link, k, d_cnt, (bb_rec_t*)b->rec.p, n_bubble, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[BBS_BAD_END]) return fail("bubble: %llu ends have no place in the list of %llu bubbles", h_stat[BBS_BAD_END], n_bubble);
	g_ms[2] = now_ms() - t0; t0 = now_ms();

	YK_LAUNCH(k_bub_classify, dim3(grid_for(n_bubble * BB_WAVE, BB_THREADS)), dim3(BB_THREADS), 0, 0, (bb_rec_t*)b->rec.p, n_bubble, d_desc, n_u, (const char*)b->bases.p, n_bases, k, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[BBS_BAD_ARM]) return fail("bubble: the arms of %llu bubbles do not fit the %llu bases, or hold a byte that is none of ACGT", h_stat[BBS_BAD_ARM], n_bases);
	if (h_stat[BBS_TYPE] + h_stat[BBS_TYPE + 1] + h_stat[BBS_TYPE + 2] != n_bubble)
		return fail("bubble: %llu bubbles were classified, %llu were found", h_stat[BBS_TYPE] + h_stat[BBS_TYPE + 1] + h_stat[BBS_TYPE + 2], n_bubble);
	st.n_bubble = n_bubble;
	for (int i = 0; i < 3; ++i) st.n_type[i] = h_stat[BBS_TYPE + i];
	st.n_tip = h_stat[BBS_TIP]; st.tip_nodes = h_stat[BBS_TIP_NODES]; st.max_arm_nodes = h_stat[BBS_MAX_ARM]; st.n_fork = h_stat[BBS_FORK];
	g_ms[3] = now_ms() - t0;
	if (!keep) { b->desc.drop(); b->bases.drop(); }                /* the records are all that a caller without the text needs */
	return 0;
}

yakamd_bubble_set_t *bubble_open(yakamd_uwalk_t *w, yakamd_gfa_t *g, int k, bool keep)
{
	for (int i = 0; i < 5; ++i) g_ms[i] = 0;
	yakamd_uwstat_t us;
	yakamd_gfastat_t gs;
	if (bubble_check(w, g, k, &us, &gs) != 0) return 0;
	yakamd_bubble_set_t *b = new (std::nothrow) yakamd_bubble_set_t();
	if (!b) { fail("bubble: no memory"); return 0; }
	b->k = k; b->dev = 0; b->n_unitig = b->n_bases = 0;
	memset(&b->st, 0, sizeof b->st);
	if (bubble_run(b, w, g, us, gs, keep) != 0) { delete b; return 0; }
	return b;
}

}   // namespace

extern "C" const char *yakamd_bubble_last_error(void) { return g_err; }
extern "C" void yakamd_bubble_ms(double ms[5]) { for (int i = 0; i < 5; ++i) ms[i] = g_ms[i]; }

extern "C" yakamd_bubble_set_t *yakamd_bubble_open(yakamd_uwalk_t *w, yakamd_gfa_t *g, int k) { return bubble_open(w, g, k, false); }

extern "C" void yakamd_bubble_close(yakamd_bubble_set_t *b)
{
	if (!b) return;
	OnDevice dev(b->dev);
	delete b;
}

extern "C" int yakamd_bubble_stats(yakamd_bubble_set_t *b, yakamd_bubstat_t *st)
{
	if (!b || !st) return fail("bubble stats: no bubbles, or no place for them");
	*st = b->st;
	return 0;
}

extern "C" int64_t yakamd_bubble_records_dev(yakamd_bubble_set_t *b, void *d, int64_t cap)
{
	return copy_out(b != 0, b ? b->dev : 0, b ? b->rec.p : 0, b ? b->st.n_bubble : 0, sizeof(bb_rec_t), d, cap, "bubble records", "bubbles", "the entries");
}

/* the command: the walk, the links, the bubbles, then the text from the tallies or from the records, the descriptors and the bases */
extern "C" int yakamd_bubbles(const yakamd_ugopt_t *opt, yak_ch_t *ch, const char *out_fn)
{
	if (!opt) return fail("yakamd_bubbles: no options");
	WalkGuard W{ yakamd_uwalk_open(ch, opt->min_cnt) };
	if (!W.p) return fail_below(yakamd_walk_last_error());
	Guard<yakamd_gfa_t, yakamd_gfa_close> G{ yakamd_gfa_open(W.p, ch->k) };
	if (!G.p) return fail_below(yakamd_gfa_last_error());
	Guard<yakamd_bubble_set_t, yakamd_bubble_close> B{ bubble_open(W.p, G.p, ch->k, !opt->stats_only) };
	yakamd_bubble_set_t *b = B.p;
	if (!b) return -1;
	const double t0 = now_ms();
	yakamd_gstat_t gs;
	yakamd_uwstat_t us;
	yakamd_gfastat_t fs;
	if (yakamd_uwalk_gstat(W.p, &gs) != 0 || yakamd_uwalk_stats(W.p, &us) != 0) return fail_below(yakamd_walk_last_error());
	if (yakamd_gfa_stats(G.p, &fs) != 0) return fail_below(yakamd_gfa_last_error());
	std::string bases;
	std::vector<bb_desc_t> desc;
	std::vector<bb_rec_t> rec;
	if (!opt->stats_only && b->st.n_bubble) {
		try { bases.resize((size_t)b->n_bases); desc.resize((size_t)b->n_unitig); rec.resize((size_t)b->st.n_bubble); }
		catch (const std::bad_alloc&) { return fail("yakamd_bubbles: %llu bases and %llu bubbles do not fit the host's memory", b->n_bases, (u64)b->st.n_bubble); }
		OnDevice dev(b->dev);
		HIPCK(hipMemcpy(&bases[0], b->bases.p, (size_t)b->n_bases, hipMemcpyDeviceToHost));
		HIPCK(hipMemcpy(desc.data(), b->desc.p, (size_t)b->n_unitig * 32, hipMemcpyDeviceToHost));
		HIPCK(hipMemcpy(rec.data(), b->rec.p, rec.size() * sizeof(bb_rec_t), hipMemcpyDeviceToHost));
	}
	OutFile out(out_fn);
	if (!out.f) return fail("yakamd_bubbles: cannot write '%s'", out.name);
	bool ok = true;
	try {
		if (opt->stats_only) {
			bbt_stats_t s;
			memcpy(&s, &b->st, sizeof s);
			ok = out.write(gft_stats(gft_tallies(b->k, opt->min_cnt, gs, us), fs.n_link, fs.end_deg) + bbt_stats_line(s));
		} else
			ok = bbt_bubbles(rec.data(), rec.size(), desc.data(), b->n_unitig, bases.data(), b->n_bases, b->k, opt->min_cnt,
			                 [&out](const std::string &t) { return out.write(t); });
	} catch (const std::bad_alloc&) { return fail("yakamd_bubbles: no host memory for the text"); }
	if (!(out.finish() && ok)) return fail("yakamd_bubbles: cannot write '%s'", out.name);
	g_ms[4] = now_ms() - t0;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] bubbles: %llu bubbles (S %llu, E %llu, I %llu) of %llu forks, %llu tips: copies %.1f ms, first links %.1f ms, find %.1f ms, classify %.1f ms, text %.1f ms\n",
		        (u64)b->st.n_bubble, (u64)b->st.n_type[0], (u64)b->st.n_type[1], (u64)b->st.n_type[2], (u64)b->st.n_fork, (u64)b->st.n_tip, g_ms[0], g_ms[1], g_ms[2], g_ms[3], g_ms[4]);
	return 0;
}

LAYER_TALLY_EXPORTS(bubble)
