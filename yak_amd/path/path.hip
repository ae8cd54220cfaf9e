/*
 * path.hip -- libyak_amd_path.so: sequences laid onto the unitig graph of a count table as paths, on the GPU (include/yak_amd_path.h; DESIGN.md
 * section 23).  A layer above libyak_amd_walk.so and libyak_amd.so: it calls their public functions only (yakamd_uwalk_open / _stats / _desc_dev /
 * _bases_dev / _close, yakamd_walk_last_error, yakamd_ch_hpc, seq_nt4_table) and owns its device memory (hipMalloc / hipFree).  The per-thread steps
 * are those of path_step.h (with ../gfa/gfa_step.h's k-mers and table), the texts those of path_text.h, the reader and the chunk loop those of ../layer/layer_seqs.h; every
 * launch goes through YK_LAUNCH of ../csrc/tally.h into this library's own tally (yakamd_path_tally_*).  The host scaffolding and the workgroup scan
 * are those of ../layer/layer_host.h and ../layer/layer_dev.h, which the layers share.
 *
 * A workgroup of 256 threads serves a tile of 1024 positions, a thread 4 consecutive ones.
 *   k_path_index      over the positions of the walk's bases: the tile and k - 1 bytes behind it staged in LDS by 16-byte loads; a thread finds its
 *                     unitig by one binary search of desc.off and moves forward from there, packs its first k-mer from LDS and rolls, skips the
 *                     k - 1 positions behind a unitig's last node and claims canon(N) by a 64-bit atomicCAS, the value stored beside the key
 *   k_path_hits       over the image: k - 1 bytes in front of the tile and the tile staged the same way, seq_nt4_table in LDS too; the forward and the
 *                     reverse word rolled together, one probe walk per k-mer (a slot is one 16-byte load), two 16-byte stores per thread
 *   k_path_count      per tile the path starts, step starts, hits and k-mers, and the steps of the path open at its end, from hit[] alone
 *   k_path_tile_scan  one workgroup, any number of tiles: every entry becomes what lies in front of its tile, the totals behind the last
 *   k_path_emit       the flags again, ranked inside the tile through LDS on top of the tile's entry: a step start writes its step, a path start
 *                     step_off, ps, seq and qs of its record, the path end of the same rank n_step and qe
 *   k_path_tally      a wave per sequence: the whole tiles inside it from two entries of the tile array, the rest counted from hit[]
 * Nothing but hit[] (8 bytes a position) and the tile array (64 bytes a tile) is kept between the kernels.  All results are addressed by position
 * and rank; the tallies are integer sums (max_probe, a measurement, a maximum); all stores are vector stores.
 */
#include "yak.h"
#include "yak_amd_path.h"
#define LAYER_NAME "path"
#include "../layer/layer_host.h"
#include "../layer/layer_seqs.h"
#include "../layer/layer_dev.h"
#include "path_step.h"
#include "path_text.h"

static_assert(sizeof(yakamd_udesc_t) == sizeof(gf_desc_t) && sizeof(yakamd_upath_t) == sizeof(px_path_t) && sizeof(px_path_t) == 32 &&
              sizeof(yakamd_ptally_t) == sizeof(px_tally_t) && sizeof(gf_slot_t) == 16, "the records as declared");
static_assert(YAKAMD_PATH_NONE == PX_NONE && YAKAMD_PATH_ABSENT == PX_ABSENT && PX_WIN % 16 == 0 && PX_HALO >= 30, "the constants as declared");

static_assert(PX_WAVE == LY_WAVE, "one wave size");

/* px_cnt_t for the workgroup scan of ../layer/layer_dev.h: its shuffle, found beside the type, and its join */
__device__ inline px_cnt_t scan_shfl_up(const px_cnt_t &a, int o)
{
	px_cnt_t y;
	y.path = __shfl_up((u64)a.path, o); y.step = __shfl_up((u64)a.step, o); y.hit = __shfl_up((u64)a.hit, o); y.kmer = __shfl_up((u64)a.kmer, o);
	y.seg_flag = __shfl_up((u64)a.seg_flag, o); y.seg_val = __shfl_up((u64)a.seg_val, o);
	return y;
}
struct CntJoin {
	__device__ static px_cnt_t zero() { px_cnt_t z; px_cnt_zero(&z); return z; }
	__device__ px_cnt_t operator()(const px_cnt_t &front, const px_cnt_t &own) const { return px_cnt_join(front, own); }
};

namespace {

/* the words of stat[]: the longest probe walk; descriptors, values or ranks that do not fit; claims that met no free slot; claims of a key that was
 * there already; nodes with a byte that is none of ACGT */
enum { PXS_PROBE = 0, PXS_BAD = 1, PXS_FULL = 2, PXS_DUP = 3, PXS_NONBASE = 4, PXS_N = 8 };

struct DevLoad16 {
	const unsigned char *g;
	__device__ void operator()(int64_t off, unsigned char *dst) const { *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(g + off); }
};

/* what a thread gathered, into stat[]: a wave's sums and its maximum by one atomic each */
__device__ inline void err_out(u64 *stat, const px_err_t &e)
{
	const u64 probe = wave_max(e.probe), bad = wave_sum(e.bad), full = wave_sum(e.full), dup = wave_sum(e.dup), nonbase = wave_sum(e.nonbase);
	if ((threadIdx.x & (PX_WAVE - 1)) == 0) {
		if (probe) atomicMax(stat + PXS_PROBE, probe);
		if (bad) atomicAdd(stat + PXS_BAD, bad);
		if (full) atomicAdd(stat + PXS_FULL, full);
		if (dup) atomicAdd(stat + PXS_DUP, dup);
		if (nonbase) atomicAdd(stat + PXS_NONBASE, nonbase);
	}
}

/* the window [wbase, wbase + PX_WIN) of an image of n bytes into LDS, 16 bytes a load; wbase is a multiple of 16 */
__device__ inline void stage(const unsigned char *g, int64_t n, int64_t wbase, unsigned char *s_win)
{
	for (int c = threadIdx.x; c < PX_WIN / 16; c += PX_THREADS) px_stage_chunk(wbase + 16 * c, n, s_win + 16 * c, DevLoad16{ g });
}

__global__ __launch_bounds__(PX_THREADS)
void k_path_index(const gf_desc_t *__restrict__ desc, u64 n_unitig, const unsigned char *__restrict__ bases, u64 n_bases, int k, gf_slot_t *slots, u64 cap, u64 *stat)
{
	__shared__ alignas(16) unsigned char s_win[PX_WIN];
	const int64_t tile0 = (int64_t)blockIdx.x * PX_TILE;
	stage(bases, (int64_t)n_bases, tile0, s_win);
	__syncthreads();
	px_err_t e = { 0, 0, 0, 0, 0 };
	px_index_thread(desc, n_unitig, n_bases, s_win, tile0, (u64)tile0 + (u64)threadIdx.x * PX_ITEMS, k, slots, cap, DevCas(), &e);
	err_out(stat, e);
}

__global__ __launch_bounds__(PX_THREADS)
void k_path_hits(const gf_slot_t *__restrict__ slots, u64 cap, const unsigned char *__restrict__ nt4, const unsigned char *__restrict__ bases, int64_t n_bytes, int k,
                 u64 n_unitig, u64 *__restrict__ hit, u64 *stat)
{
	__shared__ alignas(16) unsigned char s_win[PX_WIN];
	__shared__ unsigned char s_nt4[256];
	const int64_t tile0 = (int64_t)blockIdx.x * PX_TILE, wbase = tile0 - PX_HALO, i0 = tile0 + (int64_t)threadIdx.x * PX_ITEMS;
	stage(bases, n_bytes, wbase, s_win);
	s_nt4[threadIdx.x] = nt4[threadIdx.x];
	__syncthreads();
	px_err_t e = { 0, 0, 0, 0, 0 };
	if (i0 < ((n_bytes + 15) & ~(int64_t)15)) {                    /* i0 is a multiple of 4: its four positions lie in front of that bound with it */
		uint64_t out[PX_ITEMS];
		px_hits_thread(slots, cap, s_nt4, s_win, wbase, i0, k, n_unitig, out, &e);
		*reinterpret_cast<v2*>(hit + i0) = make_ulonglong2(out[0], out[1]);
		*reinterpret_cast<v2*>(hit + i0 + 2) = make_ulonglong2(out[2], out[3]);
	}
	err_out(stat, e);
}

/* h[0 .. 5] = hit[i0 - 1 .. i0 + 4], PX_NONE outside [0, n); hit[] reaches to n rounded up to 16 */
__device__ inline void load_hits(const u64 *__restrict__ hit, int64_t n, int64_t i0, uint64_t h[PX_ITEMS + 2])
{
#pragma unroll
	for (int q = 0; q < PX_ITEMS + 2; ++q) h[q] = PX_NONE;
	if (i0 >= n) return;
	const v2 a = *reinterpret_cast<const v2*>(hit + i0), b = *reinterpret_cast<const v2*>(hit + i0 + 2);
	h[1] = a.x;
	if (i0 + 1 < n) h[2] = a.y;
	if (i0 + 2 < n) h[3] = b.x;
	if (i0 + 3 < n) h[4] = b.y;
	if (i0 > 0) h[0] = hit[i0 - 1];
	if (i0 + 4 < n) h[5] = hit[i0 + 4];
}

__global__ __launch_bounds__(PX_THREADS)
void k_path_count(const u64 *__restrict__ hit, int64_t n, uint64_t *__restrict__ tile)
{
	uint64_t h[PX_ITEMS + 2];
	unsigned fl[PX_ITEMS];
	load_hits(hit, n, (int64_t)blockIdx.x * PX_TILE + (int64_t)threadIdx.x * PX_ITEMS, h);
	const px_cnt_t own = px_count_thread(h, fl);
	px_cnt_t before, total;
	block_scan<PX_THREADS, px_cnt_t, CntJoin>(own, &before, &total);
	if (threadIdx.x == 0) px_tile_put(tile + (u64)blockIdx.x * PXT_WORDS, &total);
}

/* the entries of tiles 0 .. m - 1 become what lies in front of each, entry m the totals: each thread a contiguous slice */
__global__ __launch_bounds__(PX_THREADS)
void k_path_tile_scan(uint64_t *__restrict__ tile, u64 m)
{
	const u64 per = (m + PX_THREADS - 1) / PX_THREADS, lo = (u64)threadIdx.x * per < m ? (u64)threadIdx.x * per : m, hi = lo + per < m ? lo + per : m;
	const px_cnt_t own = px_tile_join(tile, lo, hi);
	px_cnt_t before, total;
	block_scan<PX_THREADS, px_cnt_t, CntJoin>(own, &before, &total);
	px_tile_apply(tile, lo, hi, before);
	if (threadIdx.x == 0) px_tile_put(tile + m * PXT_WORDS, &total);
}

__global__ __launch_bounds__(PX_THREADS)
void k_path_emit(const u64 *__restrict__ hit, int64_t n, const uint64_t *__restrict__ tile, px_emit_t a, u64 *stat)
{
	uint64_t h[PX_ITEMS + 2];
	unsigned fl[PX_ITEMS];
	const int64_t i0 = (int64_t)blockIdx.x * PX_TILE + (int64_t)threadIdx.x * PX_ITEMS;
	load_hits(hit, n, i0, h);
	const px_cnt_t own = px_count_thread(h, fl);
	px_cnt_t before, total;
	block_scan<PX_THREADS, px_cnt_t, CntJoin>(own, &before, &total);
	before = px_cnt_join(px_tile_get(tile + (u64)blockIdx.x * PXT_WORDS), before);
	px_err_t e = { 0, 0, 0, 0, 0 };
#pragma unroll
	for (int q = 0; q < PX_ITEMS; ++q) {
		px_emit_pos(&a, (u64)i0 + (u64)q, h[q + 1], fl[q], &before, &e);
		px_cnt_add(&before, fl[q]);
	}
	err_out(stat, e);
}

__global__ __launch_bounds__(PX_THREADS)
void k_path_tally(const uint64_t *__restrict__ hit, u64 n, const uint64_t *__restrict__ tile, const uint64_t *__restrict__ seq_off, const uint32_t *__restrict__ seq_len, u64 n_seq,
                  px_tally_t *__restrict__ tally)
{
	const unsigned lane = threadIdx.x & (PX_WAVE - 1);
	const u64 per = PX_THREADS / PX_WAVE;
	for (u64 s = (u64)blockIdx.x * per + threadIdx.x / PX_WAVE; s < n_seq; s += (u64)gridDim.x * per) {
		u64 lo = seq_off[s], hi = lo + seq_len[s];
		hi = hi < n ? hi : n; lo = lo < hi ? lo : hi;
		uint32_t acc[4] = { 0, 0, 0, 0 };
		px_tally_seq(hit, tile, lo, hi, lane, PX_WAVE, acc);
#pragma unroll
		for (int x = 0; x < 4; ++x)
#pragma unroll
			for (int o = PX_WAVE / 2; o > 0; o >>= 1) acc[x] += __shfl_down(acc[x], o);
		if (lane == 0) *reinterpret_cast<uint4*>(tally + s) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
	}
}

/* ---------------- host ---------------- */

thread_local double g_ms[6];

const u64 MAX_TILES = 0x7fffffffull;                              /* a grid's first dimension */
u64 tiles_of(u64 n) { return (n + PX_TILE - 1) / PX_TILE; }

}   // namespace

struct yakamd_path {
	int k, dev;
	yakamd_pxstat_t st;
	DevBuf slots, desc, nt4, stat, tile;
	std::vector<uint32_t> n_node;                                  /* per unitig, for the text */
};

namespace {

/* what yakamd_path_open refuses before any device work; *cap = the slots of the index, *need = its bytes with the copies */
int path_check(yakamd_uwalk_t *w, int k, yakamd_uwstat_t *us, u64 *cap, u64 *need)
{
	if (!w) return fail("path: no walk");
	if (k < 3 || k > 31 || !(k & 1)) return fail("path: k = %d: the paths are defined for an odd k in [3, 31]", k);
	if (yakamd_uwalk_stats(w, us) != 0) return fail_below(yakamd_walk_last_error());
	const u64 n_u = us->n_open + us->n_cycle;
	if (us->sum_len != us->n_node + n_u * (u64)(k - 1))
		return fail("path: k = %d does not fit the walk: %llu bases in %llu unitigs of %llu nodes", k, (u64)us->sum_len, n_u, (u64)us->n_node);
	if (n_u >= (u64)1 << 31 || (n_u && us->max_len - (u64)(k - 1) >= (u64)1 << 31))
		return fail("path: %llu unitigs, the longest of %llu nodes: a value of the index holds less than 2^31 of either", n_u, n_u ? (u64)us->max_len - (u64)(k - 1) : 0);
	*cap = n_u ? gf_capacity(us->n_node) : 0;
	u64 want = 0;
	if (n_u && !slots_from_env("YAKAMD_PATH_SLOTS", us->n_node, cap, &want)) return fail("path: YAKAMD_PATH_SLOTS = %llu: the index has %llu keys", want, (u64)us->n_node);
	*need = *cap * 16 + n_u * 32 + up16(us->sum_len);
	return 0;
}

int path_build(yakamd_path *px, yakamd_uwalk_t *w, const yakamd_uwstat_t &us, u64 cap, u64 need)
{
	const int k = px->k;
	const u64 n_u = us.n_open + us.n_cycle, n_bases = us.sum_len;
	px->st.n_unitig = n_u; px->st.n_node = us.n_node; px->st.table_slots = cap; px->st.max_probe = 0;
	HIPCK(hipGetDevice(&px->dev));
	size_t free_b = 0, total_b = 0;
	HIPCK(hipMemGetInfo(&free_b, &total_b));
	const char *lim = getenv("YAKAMD_PATH_MAX_BYTES");
	const u64 limit = lim && *lim ? strtoull(lim, 0, 10) : (u64)free_b;
	if (need > limit)
		return fail("path: %llu bytes of device memory are needed for the index of %llu nodes (%llu slots of 16 bytes, %llu descriptors, %llu bases), %llu are free",
		             need, (u64)us.n_node, cap, n_u, n_bases, limit);
	const double t0 = now_ms();
	if (!px->nt4.get(256) || !px->stat.get(PXS_N * 8)) return fail("path: no device memory");
	HIPCK(hipMemcpy(px->nt4.p, seq_nt4_table, 256, hipMemcpyHostToDevice));
	HIPCK(hipMemset(px->stat.p, 0, PXS_N * 8));
	if (n_u == 0) { g_ms[0] = now_ms() - t0; return 0; }
	if (tiles_of(n_bases) > MAX_TILES) return fail("path: %llu bases are more than one launch serves", n_bases);

	DevBuf bases;
	/* the descriptors on the host: their nodes for the text, and one look at whether they tile the bases */
	std::vector<gf_desc_t> h_desc;
	const int rc = px->slots.get(cap * 16) ? copy_walk(w, n_u, n_bases, 16, px->desc, bases, h_desc) : 1;
	if (rc) return rc < 0 ? -1 : fail("path: no device memory for %llu bytes", need);
	try { px->n_node.resize((size_t)n_u); } catch (const std::bad_alloc&) { return fail("path: the descriptors of %llu unitigs do not fit the host's memory", n_u); }
	u64 at = 0, nodes = 0;
	for (u64 j = 0; j < n_u; ++j) {
		const gf_desc_t &u = h_desc[(size_t)j];
		if (u.off != at || !px_desc_fits(&u, n_bases, k)) return fail("path: the descriptor of unitig %llu does not fit the %llu bases", j, n_bases);
		at += u.n_node + (u64)(k - 1); nodes += u.n_node;
		px->n_node[(size_t)j] = (uint32_t)u.n_node;
	}
	if (at != n_bases || nodes != us.n_node) return fail("path: the descriptors hold %llu nodes in %llu bases, the walk states %llu in %llu", nodes, at, (u64)us.n_node, n_bases);

	u64 *d_stat = (u64*)px->stat.p, h_stat[PXS_N];
	HIPCK(hipMemset(px->slots.p, 0xff, cap * 16));                 /* every key GF_EMPTY */
	YK_LAUNCH(k_path_index, dim3((unsigned)tiles_of(n_bases)), dim3(PX_THREADS), 0, 0, (const gf_desc_t*)px->desc.p, n_u, (const unsigned char*)bases.p, n_bases, k,
	          (gf_slot_t*)px->slots.p, cap, d_stat);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[PXS_FULL]) return fail("path: %llu nodes met no free slot among the %llu of the index", h_stat[PXS_FULL], cap);
	if (h_stat[PXS_BAD]) return fail("path: the descriptors do not fit the %llu bases at %llu places", n_bases, h_stat[PXS_BAD]);
	if (h_stat[PXS_NONBASE]) return fail("path: %llu nodes hold a byte that is none of ACGT", h_stat[PXS_NONBASE]);
	if (h_stat[PXS_DUP]) return fail("path: %llu nodes stand in two places of the unitigs", h_stat[PXS_DUP]);
	px->st.max_probe = h_stat[PXS_PROBE];
	g_ms[0] = now_ms() - t0;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] path: the index of %llu nodes in %llu slots (longest probe %llu) %.1f ms\n", (u64)us.n_node, cap, (u64)px->st.max_probe, g_ms[0]);
	return 0;
}

/* stat[] after a launch: its longest probe into the stats, its misfits as a failure */
int path_after(yakamd_path *px, const char *what)
{
	u64 h_stat[PXS_N];
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, px->stat.p, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[PXS_PROBE] > px->st.max_probe) px->st.max_probe = h_stat[PXS_PROBE];
	if (h_stat[PXS_BAD]) {
		(void)hipMemset(px->stat.p, 0, PXS_N * 8);
		return fail("path %s: %llu values do not fit the unitigs, the sequences or the lists", what, h_stat[PXS_BAD]);
	}
	return 0;
}

}   // namespace

extern "C" const char *yakamd_path_last_error(void) { return g_err; }
extern "C" void yakamd_path_ms(double ms[6]) { for (int i = 0; i < 6; ++i) ms[i] = g_ms[i]; }
extern "C" void yakamd_ppopt_init(yakamd_ppopt_t *o)
{
	if (!o) return;
	o->min_cnt = 1; o->min_len = 0; o->stats_only = 0; o->reserved = 0; o->chunk_size = (int64_t)1 << 28;
}

extern "C" yakamd_path_t *yakamd_path_open(yakamd_uwalk_t *w, int k)
{
	for (int i = 0; i < 6; ++i) g_ms[i] = 0;
	yakamd_uwstat_t us;
	u64 cap = 0, need = 0;
	if (path_check(w, k, &us, &cap, &need) != 0) return 0;
	yakamd_path_t *px = new (std::nothrow) yakamd_path_t();
	if (!px) { fail("path: no memory"); return 0; }
	px->k = k; px->dev = 0;
	memset(&px->st, 0, sizeof px->st);
	if (path_build(px, w, us, cap, need) != 0) { delete px; return 0; }
	return px;
}

extern "C" void yakamd_path_close(yakamd_path_t *px)
{
	if (!px) return;
	OnDevice dev(px->dev);
	delete px;
}

extern "C" int yakamd_path_stats(yakamd_path_t *px, yakamd_pxstat_t *st)
{
	if (!px || !st) return fail("path stats: no index, or no place for the numbers");
	*st = px->st;
	return 0;
}

extern "C" int yakamd_path_hits_dev(yakamd_path_t *px, const void *d_bases, int64_t n_bytes, uint64_t *d_hit)
{
	if (!px) return fail("path hits: no index");
	if (n_bytes < 0) return fail("path hits: %lld bytes", (long long)n_bytes);
	if (n_bytes == 0) return 0;
	if (!d_bases || !d_hit || (((uintptr_t)d_bases | (uintptr_t)d_hit) & 15) != 0) return fail("path hits: the image and the hits must be given and 16-byte aligned");
	if (tiles_of((u64)n_bytes) > MAX_TILES) return fail("path hits: %lld bytes are more than one launch serves", (long long)n_bytes);
	const double t0 = now_ms();
	YK_LAUNCH(k_path_hits, dim3((unsigned)tiles_of((u64)n_bytes)), dim3(PX_THREADS), 0, 0, (const gf_slot_t*)px->slots.p, (u64)px->st.table_slots, (const unsigned char*)px->nt4.p,
	          (const unsigned char*)d_bases, n_bytes, px->k, (u64)px->st.n_unitig, (u64*)d_hit, (u64*)px->stat.p);
	const int rc = path_after(px, "hits");
	g_ms[1] += now_ms() - t0;
	return rc;
}

extern "C" int yakamd_path_chain_dev(yakamd_path_t *px, const uint64_t *d_hit, int64_t n_bytes, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                                     yakamd_upath_t *d_paths, int64_t cap_paths, uint64_t *d_steps, int64_t cap_steps, yakamd_ptally_t *d_tally, int64_t n_out[2])
{
	if (!px) return fail("path chain: no index");
	if (!n_out) return fail("path chain: no place for the two numbers");
	n_out[0] = n_out[1] = 0;
	if (n_bytes < 0 || n_seq < 0) return fail("path chain: %lld bytes, %lld sequences", (long long)n_bytes, (long long)n_seq);
	if (n_seq > 0 && (!d_seq_off || !d_seq_len)) return fail("path chain: %lld sequences without their offsets and lengths", (long long)n_seq);
	if ((((uintptr_t)d_hit | (uintptr_t)d_paths | (uintptr_t)d_tally) & 15) != 0 || (((uintptr_t)d_steps | (uintptr_t)d_seq_off) & 7) != 0 || ((uintptr_t)d_seq_len & 3) != 0)
		return fail("path chain: the hits, the records and the tallies must be 16-byte aligned, the steps and the offsets 8-byte, the lengths 4-byte");
	if (n_bytes == 0) {                                            /* no position: no launch */
		if (d_tally && n_seq > 0) HIPCK(hipMemset(d_tally, 0, (size_t)n_seq * sizeof(yakamd_ptally_t)));
		return 0;
	}
	if (!d_hit) return fail("path chain: no hits");
	if (n_seq < 1) return fail("path chain: %lld bytes in no sequence", (long long)n_bytes);
	const u64 m = tiles_of((u64)n_bytes);
	if (m > MAX_TILES) return fail("path chain: %lld bytes are more than one launch serves", (long long)n_bytes);
	if (!px->tile.need((size_t)(m + 1) * PXT_WORDS * 8)) return fail("path chain: no device memory for %llu tiles", m);
	uint64_t *d_tile = (uint64_t*)px->tile.p, tot[PXT_WORDS];
	double t0 = now_ms();
	YK_LAUNCH(k_path_count, dim3((unsigned)m), dim3(PX_THREADS), 0, 0, (const u64*)d_hit, n_bytes, d_tile);
	YK_LAUNCH(k_path_tile_scan, dim3(1), dim3(PX_THREADS), 0, 0, d_tile, m);
	if (d_tally) {
		const u64 g = ((u64)n_seq + PX_THREADS / PX_WAVE - 1) / (PX_THREADS / PX_WAVE);
		YK_LAUNCH(k_path_tally, dim3((unsigned)(g < (1u << 20) ? g : (1u << 20))), dim3(PX_THREADS), 0, 0, d_hit, (u64)n_bytes, (const uint64_t*)d_tile, d_seq_off,
		          d_seq_len, (u64)n_seq, (px_tally_t*)d_tally);
	}
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(tot, d_tile + m * PXT_WORDS, sizeof tot, hipMemcpyDeviceToHost));
	n_out[0] = (int64_t)tot[PXT_PATH]; n_out[1] = (int64_t)tot[PXT_STEP];
	g_ms[2] += now_ms() - t0; t0 = now_ms();
	if (!d_paths || !d_steps || cap_paths < n_out[0] || cap_steps < n_out[1]) return 1;
	if (n_out[0] == 0) return 0;
	px_emit_t a;
	a.seq_off = d_seq_off; a.n_seq = (u64)n_seq;
	a.desc = (const gf_desc_t*)px->desc.p; a.n_unitig = px->st.n_unitig;
	a.paths = (px_path_t*)d_paths; a.cap_paths = (u64)n_out[0];
	a.steps = d_steps; a.cap_steps = (u64)n_out[1];
	a.k = px->k;
	YK_LAUNCH(k_path_emit, dim3((unsigned)m), dim3(PX_THREADS), 0, 0, (const u64*)d_hit, n_bytes, (const uint64_t*)d_tile, a, (u64*)px->stat.p);
	const int rc = path_after(px, "chain");
	g_ms[3] += now_ms() - t0;
	return rc;
}

/* ---- the command ---- */
namespace {

struct ChunkDev { SeqChunkDev seqs; DevBuf hit, tally, paths, steps; };

/* one chunk through the device; its text behind `text` */
int run_chunk(yakamd_path *px, const yakamd_ppopt_t &o, SeqChunk &c, ChunkDev &d, std::string &text, pxt_total_t *tot)
{
	const size_t n_seq = c.name.size();
	size_t n = 0;
	if (n_seq == 0) return 0;
	if (!d.hit.need((size_t)up16(c.img.size()) * 8) || !d.tally.need(n_seq * 16)) return fail("yakamd_paths: no device memory for a chunk of %zu bytes", c.img.size());
	if (d.seqs.upload("yakamd_paths", c, &n, &g_ms[4]) != 0) return -1;
	const uint64_t *d_off = (const uint64_t*)d.seqs.off.p;
	const uint32_t *d_len = (const uint32_t*)d.seqs.len.p;
	if (yakamd_path_hits_dev(px, d.seqs.img.p, (int64_t)n, (uint64_t*)d.hit.p) != 0) return -1;
	int64_t n_out[2];
	int rc = yakamd_path_chain_dev(px, (const uint64_t*)d.hit.p, (int64_t)n, d_off, d_len, (int64_t)n_seq, 0, 0, 0, 0, (yakamd_ptally_t*)d.tally.p, n_out);
	if (rc < 0) return -1;
	std::vector<px_path_t> paths;
	std::vector<uint64_t> steps;
	std::vector<px_tally_t> tally;
	double t0;
	if (o.stats_only) {
		tally.resize(n_seq);
		t0 = now_ms();
		HIPCK(hipMemcpy(tally.data(), d.tally.p, n_seq * 16, hipMemcpyDeviceToHost));
		g_ms[4] += now_ms() - t0; t0 = now_ms();
		pxt_stats(text, c.name, c.len.data(), tally.data(), tot);
		g_ms[5] += now_ms() - t0;
		return 0;
	}
	if (n_out[0] == 0) return 0;
	if (!d.paths.need((size_t)n_out[0] * 32) || !d.steps.need((size_t)n_out[1] * 8)) return fail("yakamd_paths: no device memory for %lld paths of %lld steps", (long long)n_out[0], (long long)n_out[1]);
	int64_t again[2];
	rc = yakamd_path_chain_dev(px, (const uint64_t*)d.hit.p, (int64_t)n, d_off, d_len, (int64_t)n_seq, (yakamd_upath_t*)d.paths.p, n_out[0], (uint64_t*)d.steps.p, n_out[1], 0, again);
	if (rc != 0) return rc < 0 ? -1 : fail("yakamd_paths: the writing call counted %lld paths of %lld steps, the counting call %lld of %lld", (long long)again[0], (long long)again[1],
	                                        (long long)n_out[0], (long long)n_out[1]);
	paths.resize((size_t)n_out[0]); steps.resize((size_t)n_out[1]);
	t0 = now_ms();
	HIPCK(hipMemcpy(paths.data(), d.paths.p, paths.size() * 32, hipMemcpyDeviceToHost));
	HIPCK(hipMemcpy(steps.data(), d.steps.p, steps.size() * 8, hipMemcpyDeviceToHost));
	g_ms[4] += now_ms() - t0; t0 = now_ms();
	if (!pxt_gaf(text, c.name, c.len.data(), paths.data(), paths.size(), steps.data(), steps.size(), px->n_node.data(), px->n_node.size(), px->k, o.min_len))
		return fail("yakamd_paths: a path record does not fit its chunk");
	g_ms[5] += now_ms() - t0;
	return 0;
}

}   // namespace

extern "C" int yakamd_paths(const yakamd_ppopt_t *opt, yak_ch_t *ch, const char *fn, const char *out_fn)
{
	if (!opt) return fail("yakamd_paths: no options");
	if (opt->min_len < 0) return fail("yakamd_paths: min_len %d", opt->min_len);
	if (opt->chunk_size < 1) return fail("yakamd_paths: chunk_size %lld", (long long)opt->chunk_size);
	if (!fn) return fail("yakamd_paths: no sequences");
	if (ch && yakamd_ch_hpc(ch)) return fail("yakamd_paths: the table is marked homopolymer-compressed: its unitigs are no sequences to lay others onto");
	SeqReader rd(false);                                           /* of a quality its length alone */
	if (ch && !rd.open(fn)) return fail("yakamd_paths: cannot read '%s'", fn);
	WalkGuard W{ yakamd_uwalk_open(ch, opt->min_cnt) };
	if (!W.p) return fail_below(yakamd_walk_last_error());
	Guard<yakamd_path_t, yakamd_path_close> P{ yakamd_path_open(W.p, ch->k) };
	yakamd_path_t *px = P.p;
	if (!px) return -1;
	W.close();
	OutFile out(out_fn);
	if (!out.f) return fail("yakamd_paths: cannot write '%s'", out.name);
	bool ok = true;
	ChunkDev d;
	std::string text;
	pxt_total_t tot = { 0, 0, 0, 0, 0, 0 };
	if (opt->stats_only) pxt_stats_head(text, px->k, opt->min_cnt);
	if (seq_chunks("yakamd_paths", rd, fn, opt->chunk_size, 0, [&](SeqChunk &c, bool last) {
		if (run_chunk(px, *opt, c, d, text, &tot) != 0) return -1;
		if (last && opt->stats_only) pxt_stats_tail(text, tot);
		flush(text, &out, last, &ok);
		return 0;
	}) != 0) return -1;
	if (!(out.finish() && ok)) return fail("yakamd_paths: cannot write '%s'", out.name);
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] paths: index %.1f ms, hits %.1f ms, count and scan %.1f ms, emit %.1f ms, copies %.1f ms, text %.1f ms (longest probe %llu)\n", g_ms[0], g_ms[1],
		        g_ms[2], g_ms[3], g_ms[4], g_ms[5], (u64)px->st.max_probe);
	return 0;
}

LAYER_TALLY_EXPORTS(path)
