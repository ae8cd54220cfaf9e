/*
 * allele.hip -- libyak_amd_allele.so: the alleles of the simple bubbles of the unitig graph supported with reads on the GPU (include/yak_amd_allele.h;
 * DESIGN.md section 31).  A layer above libyak_amd_path.so, libyak_amd_bubble.so, libyak_amd_gfa.so, libyak_amd_walk.so and libyak_amd.so: it
 * calls their public functions only (yakamd_uwalk_open / _stats / _close, yakamd_gfa_open / _close, yakamd_bubble_open / _stats / _records_dev /
 * _close, yakamd_path_open / _hits_dev / _chain_dev / _close, their last errors and yakamd_ch_hpc) and owns its device memory (hipMalloc /
 * hipFree).  The per-thread steps are those of allele_step.h, the texts those of allele_text.h, the reader and the chunk loop those of
 * ../layer/layer_seqs.h; every launch goes through YK_LAUNCH of ../csrc/tally.h into this library's own tally (yakamd_allele_tally_*).  The host
 * scaffolding and the scan are those of ../layer/layer_host.h and ../layer/layer_dev.h, which the layers share.
 *
 *   k_al_index         a thread per bubble record, its arms by one 16-byte load: each of the two claims arm_of[j] by a 32-bit compare-and-swap from ~0, so a second claim
 *                      of one unitig is seen; an arm outside the unitigs is counted and claims nothing
 *   k_al_find<COUNT>   a thread per step, a workgroup 256 consecutive steps: two lanes of two waves find the paths of the workgroup's first and
 *                      last step by a search over step_off and leave them in LDS, every thread then searches between the two only -- 256 steps
 *                      inside one long read's path need no search at all; the decision (al_find), cnt[t] = (is an observation, is a full one), one
 *                      16-byte store; n_obs and n_full summed per wave, one LDS atomic per wave, one 64-bit global atomic per workgroup and counter
 *   k_al_tile_sum, k_al_tile_scan, k_al_scan_apply
 *                      the exclusive scan of cnt[] in place, both words at once: tiles of 1024, their sums scanned by one workgroup
 *   k_al_find<EMIT>    the same decision again; an observation writes its record at its rank, one 16-byte store, and adds 1 to its word of the
 *                      support, one 64-bit global atomic: observations are sparse (a step on an arm) and integer sums do not depend on the order
 * All records are addressed by step and rank; the tallies and the support are integer sums; all stores are vector stores.
 */
#include "yak.h"
#include "yak_amd_allele.h"
#define LAYER_NAME "allele"
#include "../layer/layer_host.h"
#include "../layer/layer_seqs.h"
#include "../layer/layer_dev.h"
#include "allele_step.h"
#include "allele_text.h"

static_assert(sizeof(yakamd_bubble_t) == sizeof(bb_rec_t) && sizeof(yakamd_upath_t) == sizeof(al_path_t) && sizeof(al_path_t) == 32, "the records as declared");
static_assert(sizeof(yakamd_aobs_t) == 16 && sizeof(al_obs_t) == 16 && sizeof(yakamd_asup_t) == 32 && sizeof(al_sup_t) == 32 && sizeof(yakamd_alopt_t) == 32, "the records as declared");
static_assert(YAKAMD_AOBS_A == AL_A && YAKAMD_AOBS_FULL == AL_FULL && YAKAMD_AOBS_REV == AL_REV, "the flags as declared");

namespace {

enum { AL_THREADS = 256, AL_ITEMS = 4, AL_TILE = AL_THREADS * AL_ITEMS, AL_WAVE = 64 };
/* the words of stat[]: the observations and the full ones of k_al_find<COUNT>; then what does not fit: arms of k_al_index outside the unitigs,
 * arms whose unitig another arm holds, steps of k_al_find (a path's range, a step's unitig, a rank outside the list) */
enum { ALS_OBS = 0, ALS_FULL = 1, ALS_BAD_ARM = 4, ALS_DUP_ARM = 5, ALS_BAD_STEP = 6, ALS_N = 8 };
enum AlMode { COUNT = 0, EMIT = 1 };

struct DevCas32 {
	__device__ uint32_t operator()(uint32_t *p, uint32_t expected, uint32_t desired) const { return (uint32_t)atomicCAS(reinterpret_cast<unsigned*>(p), (unsigned)expected, (unsigned)desired); }
};

__device__ inline void tally_bad(u64 bad, u64 *stat, int at)
{
	bad = wave_sum(bad);
	if ((threadIdx.x & (AL_WAVE - 1)) == 0 && bad) atomicAdd(stat + at, bad);
}

__global__ __launch_bounds__(AL_THREADS)
void k_al_index(const bb_rec_t *__restrict__ rec, u64 n_bubble, u64 n_unitig, uint32_t *arm_of, u64 *stat)
{
	u64 bad = 0, dup = 0;
	for (u64 i = (u64)blockIdx.x * AL_THREADS + threadIdx.x; i < n_bubble; i += (u64)gridDim.x * AL_THREADS) {
		const v2 arm = reinterpret_cast<const v2*>(rec + i)[1];        /* both arms: one 16-byte load */
		const int r0 = al_claim(arm.x, i, 0, n_unitig, arm_of, DevCas32()), r1 = al_claim(arm.y, i, 1, n_unitig, arm_of, DevCas32());
		bad += (r0 == AL_BAD_ARM) + (r1 == AL_BAD_ARM); dup += (r0 == AL_DUP_ARM) + (r1 == AL_DUP_ARM);
	}
	tally_bad(bad, stat, ALS_BAD_ARM);
	tally_bad(dup, stat, ALS_DUP_ARM);
}

/* COUNT: cnt[t] = (1 iff step t is an observation, 1 iff a full one), the two totals.  EMIT: cnt[t].x is the rank of its record in obs[0 .. n_obs).
 * One workgroup per AL_THREADS steps: the grid is as large as the steps need */
template<int MODE> __global__ __launch_bounds__(AL_THREADS)
void k_al_find(const al_path_t *__restrict__ paths, u64 n_path, const uint64_t *__restrict__ steps, u64 n_step, u64 n_unitig, const uint32_t *__restrict__ arm_of,
               const bb_rec_t *__restrict__ rec, v2 *__restrict__ cnt, al_obs_t *__restrict__ obs, u64 n_obs, al_sup_t *sup, u64 *stat)
{
	__shared__ u64 s_p[2];                                         /* the paths of the workgroup's first and last step */
	__shared__ u64 s_t[2];                                         /* observations, full ones */
	const u64 t0 = (u64)blockIdx.x * AL_THREADS, t = t0 + threadIdx.x;
	if (threadIdx.x < 2) s_t[threadIdx.x] = 0;
	if (t0 < n_step && (threadIdx.x == 0 || threadIdx.x == AL_WAVE)) {      /* one lane each of two waves: the two searches run side by side */
		const u64 last = t0 + AL_THREADS - 1 < n_step ? t0 + AL_THREADS - 1 : n_step - 1;
		s_p[threadIdx.x / AL_WAVE] = al_path_of(paths, 0, n_path - 1, threadIdx.x ? last : t0);
	}
	__syncthreads();
	u64 is = 0, full = 0, bad = 0;
	if (t < n_step) {
		al_obs_t o;
		uint64_t bd = 0;
		is = (u64)al_find(paths, s_p[0], s_p[1], steps, n_step, t, n_unitig, arm_of, rec, &o, &bd);
		bad = bd;
		full = is && (o.flags & AL_FULL) ? 1 : 0;
		if (MODE == COUNT) {
			cnt[t] = make_ulonglong2(is, full);
		} else if (is) {
			const u64 at = cnt[t].x;
			if (at >= n_obs) ++bad;                                        /* a rank outside the list: tallied, not written */
			else {
				*reinterpret_cast<uint4*>(obs + at) = make_uint4(o.seq, o.bubble, o.flags, o.path);
				atomicAdd(reinterpret_cast<u64*>(full ? sup[o.bubble].full : sup[o.bubble].part) + (o.flags & AL_A), (u64)1);
			}
		}
	}
	if (MODE == COUNT) {
		is = wave_sum(is); full = wave_sum(full);
		if ((threadIdx.x & (AL_WAVE - 1)) == 0) {
			if (is) atomicAdd(&s_t[0], is);
			if (full) atomicAdd(&s_t[1], full);
		}
		__syncthreads();
		if (threadIdx.x < 2 && s_t[threadIdx.x]) atomicAdd(stat + ALS_OBS + threadIdx.x, s_t[threadIdx.x]);
	}
	tally_bad(bad, stat, ALS_BAD_STEP);
}

/* the exclusive scan of cnt[] in place (../layer/layer_dev.h), both words at once: tiles of AL_TILE, their sums scanned by one workgroup */
__global__ __launch_bounds__(AL_THREADS)
void k_al_tile_sum(const v2 *__restrict__ cnt, u64 n, v2 *__restrict__ tsum) { tile_sum<AL_THREADS, AL_ITEMS, v2, AddV2>(cnt, n, tsum); }
__global__ __launch_bounds__(AL_THREADS)
void k_al_tile_scan(v2 *__restrict__ tsum, u64 m) { tile_scan<AL_THREADS, v2, AddV2>(tsum, m); }
__global__ __launch_bounds__(AL_THREADS)
void k_al_scan_apply(v2 *__restrict__ cnt, u64 n, const v2 *__restrict__ tsum) { scan_apply<AL_THREADS, AL_ITEMS, v2, AddV2>(cnt, n, tsum); }

/* ---------------- host ---------------- */

thread_local double g_ms[5];                                       /* the arm map; count and scan, emit, copies, text */

const u64 MAX_GRID = 0x7fffffffull;                                /* a grid's first dimension */

}   // namespace

struct yakamd_allele {
	int dev;
	yakamd_alstat_t st;
	DevBuf arm_of, rec, sup, stat, cnt, tsum;
};

namespace {

int allele_build(yakamd_allele *al, yakamd_bubble_set_t *b)
{
	const u64 n_u = al->st.n_unitig, n_b = al->st.n_bubble;
	HIPCK(hipGetDevice(&al->dev));
	const double t0 = now_ms();
	if (!al->arm_of.get(n_u * 4) || !al->rec.get(n_b * sizeof(bb_rec_t)) || !al->sup.get(n_b * sizeof(al_sup_t)) || !al->stat.get(ALS_N * 8))
		return fail("allele: no device memory for %llu bytes", n_u * 4 + n_b * (sizeof(bb_rec_t) + sizeof(al_sup_t)));
	HIPCK(hipMemset(al->arm_of.p, 0xff, al->arm_of.have));         /* every unitig AL_NONE */
	HIPCK(hipMemset(al->sup.p, 0, al->sup.have));
	HIPCK(hipMemset(al->stat.p, 0, ALS_N * 8));
	if (n_b == 0) { g_ms[0] = now_ms() - t0; return 0; }
	if (yakamd_bubble_records_dev(b, al->rec.p, (int64_t)n_b) != (int64_t)n_b) return fail_below(yakamd_bubble_last_error());
	const char *damage = getenv("YAKAMD_ALLELE_DAMAGE");           /* a test switch: a genuine set of bubbles never claims a unitig twice */
	if (damage && strcmp(damage, "dup") == 0)                      /* the last record's second arm becomes the first record's first */
		HIPCK(hipMemcpy((char*)al->rec.p + (n_b - 1) * sizeof(bb_rec_t) + offsetof(bb_rec_t, arm) + 8, (char*)al->rec.p + offsetof(bb_rec_t, arm), 8, hipMemcpyDeviceToDevice));
	u64 h_stat[ALS_N];
	YK_LAUNCH(k_al_index, dim3(grid_for(n_b, AL_THREADS)), dim3(AL_THREADS), 0, 0, (const bb_rec_t*)al->rec.p, n_b, n_u, (uint32_t*)al->arm_of.p, (u64*)al->stat.p);
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, al->stat.p, sizeof h_stat, hipMemcpyDeviceToHost));
	if (h_stat[ALS_BAD_ARM]) return fail("allele: %llu arms of the %llu bubbles name none of the %llu unitigs of the walk", h_stat[ALS_BAD_ARM], n_b, n_u);
	if (h_stat[ALS_DUP_ARM]) return fail("allele: %llu arms of the %llu bubbles name a unitig that another arm holds: an arm belongs to one bubble", h_stat[ALS_DUP_ARM], n_b);
	al->st.n_arm = 2 * n_b;
	g_ms[0] = now_ms() - t0;
	return 0;
}

/* stat[] after a launch of k_al_find: its misfits as a failure, its two totals in tot[] */
int allele_after(yakamd_allele *al, const char *what, u64 n_path, u64 n_step, u64 tot[2])
{
	u64 h_stat[ALS_N];
	HIPCK(hipGetLastError());
	HIPCK(hipMemcpy(h_stat, al->stat.p, sizeof h_stat, hipMemcpyDeviceToHost));
	tot[0] = h_stat[ALS_OBS]; tot[1] = h_stat[ALS_FULL];
	if (h_stat[ALS_BAD_STEP])
		return fail("allele obs: %s: %llu of the %llu steps do not fit: the range of a path among the %llu does not follow the path before it or leaves the steps, a step names none of the %llu unitigs, or a rank lies outside the list",
		            what, h_stat[ALS_BAD_STEP], n_step, n_path, (u64)al->st.n_unitig);
	return 0;
}

}   // namespace

extern "C" const char *yakamd_allele_last_error(void) { return g_err; }
extern "C" void yakamd_allele_ms(double ms[5]) { for (int i = 0; i < 5; ++i) ms[i] = g_ms[i]; }
extern "C" void yakamd_alopt_init(yakamd_alopt_t *o)
{
	if (!o) return;
	o->min_cnt = 1; o->min_sup = 2; o->min_frag = 1; o->fragments = 0; o->stats_only = 0; o->reserved = 0; o->chunk_size = (int64_t)1 << 28;
}

extern "C" yakamd_allele_t *yakamd_allele_open(yakamd_uwalk_t *w, yakamd_bubble_set_t *b)
{
	for (int i = 0; i < 5; ++i) g_ms[i] = 0;
	if (!w) { fail("allele: no walk"); return 0; }
	if (!b) { fail("allele: no bubbles"); return 0; }
	yakamd_uwstat_t us;
	yakamd_bubstat_t bs;
	if (yakamd_uwalk_stats(w, &us) != 0) { fail_below(yakamd_walk_last_error()); return 0; }
	if (yakamd_bubble_stats(b, &bs) != 0) { fail_below(yakamd_bubble_last_error()); return 0; }
	const u64 n_u = us.n_open + us.n_cycle;
	if (n_u >= (u64)1 << 31 || bs.n_bubble >= (u64)1 << 31) {
		fail("allele: %llu unitigs and %llu bubbles: an entry of the arm map holds less than 2^31 of either", n_u, (u64)bs.n_bubble);
		return 0;
	}
	yakamd_allele_t *al = new (std::nothrow) yakamd_allele_t();
	if (!al) { fail("allele: no memory"); return 0; }
	al->dev = 0;
	al->st.n_unitig = n_u; al->st.n_bubble = bs.n_bubble; al->st.n_arm = 0;
	if (allele_build(al, b) != 0) { delete al; return 0; }
	return al;
}

extern "C" void yakamd_allele_close(yakamd_allele_t *al)
{
	if (!al) return;
	OnDevice dev(al->dev);
	delete al;
}

extern "C" int yakamd_allele_stats(yakamd_allele_t *al, yakamd_alstat_t *st)
{
	if (!al || !st) return fail("allele stats: no arm map, or no place for the numbers");
	*st = al->st;
	return 0;
}

extern "C" int yakamd_allele_reset(yakamd_allele_t *al)
{
	if (!al) return fail("allele reset: no arm map");
	OnDevice dev(al->dev);
	HIPCK(hipMemset(al->sup.p, 0, al->sup.have));
	return 0;
}

extern "C" int64_t yakamd_allele_support_dev(yakamd_allele_t *al, void *d, int64_t cap)
{
	return copy_out(al != 0, al ? al->dev : 0, al ? al->sup.p : 0, al ? al->st.n_bubble : 0, sizeof(al_sup_t), d, cap, "allele support", "arm map", "the entries");
}

extern "C" int yakamd_allele_obs_dev(yakamd_allele_t *al, const yakamd_upath_t *d_paths, int64_t n_path, const uint64_t *d_steps, int64_t n_step, yakamd_aobs_t *d_obs,
                                     int64_t cap, int64_t n_out[2])
{
	if (!al) return fail("allele obs: no arm map");
	if (!n_out) return fail("allele obs: no place for the two numbers");
	n_out[0] = n_out[1] = 0;
	if (n_path < 0 || n_step < 0 || cap < 0) return fail("allele obs: %lld paths, %lld steps, room for %lld records", (long long)n_path, (long long)n_step, (long long)cap);
	if ((((uintptr_t)d_paths | (uintptr_t)d_obs) & 15) != 0 || ((uintptr_t)d_steps & 7) != 0) return fail("allele obs: the paths and the records must be 16-byte aligned, the steps 8-byte");
	if (n_step > 0 && (!d_paths || !d_steps)) return fail("allele obs: %lld steps without their list or without their paths", (long long)n_step);
	if (n_step > 0 && (n_path < 1 || n_path > n_step || n_path >= (int64_t)1 << 32))
		return fail("allele obs: %lld steps in %lld paths: a path has a step or more, and a record holds a path below 2^32", (long long)n_step, (long long)n_path);
	const u64 g = ((u64)n_step + AL_THREADS - 1) / AL_THREADS, m = ((u64)n_step + AL_TILE - 1) / AL_TILE;
	if (g > MAX_GRID) return fail("allele obs: %lld steps are more than one launch serves", (long long)n_step);
	if (n_step == 0 || al->st.n_bubble == 0) return d_obs ? 0 : 1;      /* no step, or no arm: no launch */
	OnDevice dev(al->dev);
	if (!al->cnt.need((size_t)n_step * 16) || !al->tsum.need((size_t)(m + 1) * 16)) return fail("allele obs: no device memory for %lld steps", (long long)n_step);
	u64 *d_stat = (u64*)al->stat.p, tot[2], again[2];
	v2 *d_cnt = (v2*)al->cnt.p, *d_tsum = (v2*)al->tsum.p, h_sum;
	const al_path_t *paths = (const al_path_t*)d_paths;
	double t0 = now_ms();
	HIPCK(hipMemset(d_stat, 0, ALS_N * 8));
	YK_LAUNCH(k_al_find<COUNT>, dim3((unsigned)g), dim3(AL_THREADS), 0, 0, paths, (u64)n_path, d_steps, (u64)n_step, (u64)al->st.n_unitig, (const uint32_t*)al->arm_of.p,
	          (const bb_rec_t*)al->rec.p, d_cnt, (al_obs_t*)0, (u64)0, (al_sup_t*)0, d_stat);
	YK_LAUNCH(k_al_tile_sum, dim3((unsigned)m), dim3(AL_THREADS), 0, 0, (const v2*)d_cnt, (u64)n_step, d_tsum);
	YK_LAUNCH(k_al_tile_scan, dim3(1), dim3(AL_THREADS), 0, 0, d_tsum, m);
	YK_LAUNCH(k_al_scan_apply, dim3((unsigned)m), dim3(AL_THREADS), 0, 0, d_cnt, (u64)n_step, (const v2*)d_tsum);
	const int rc = allele_after(al, "the count", (u64)n_path, (u64)n_step, tot);
	if (rc == 0) HIPCK(hipMemcpy(&h_sum, d_tsum + m, 16, hipMemcpyDeviceToHost));
	g_ms[1] += now_ms() - t0; t0 = now_ms();
	if (rc != 0) return -1;
	if (h_sum.x != tot[0] || h_sum.y != tot[1] || tot[1] > tot[0] || tot[0] > (u64)n_step)
		return fail("allele obs: the scan holds %llu observations, %llu of them full, the tally %llu and %llu", (u64)h_sum.x, (u64)h_sum.y, tot[0], tot[1]);
	n_out[0] = (int64_t)tot[0]; n_out[1] = (int64_t)tot[1];
	if (!d_obs || cap < n_out[0]) return 1;
	if (n_out[0] == 0) return 0;
	YK_LAUNCH(k_al_find<EMIT>, dim3((unsigned)g), dim3(AL_THREADS), 0, 0, paths, (u64)n_path, d_steps, (u64)n_step, (u64)al->st.n_unitig, (const uint32_t*)al->arm_of.p,
	          (const bb_rec_t*)al->rec.p, d_cnt, (al_obs_t*)d_obs, tot[0], (al_sup_t*)al->sup.p, d_stat);
	const int rc2 = allele_after(al, "the emit", (u64)n_path, (u64)n_step, again);
	g_ms[2] += now_ms() - t0;
	return rc2;
}

/* ---- the command ---- */
namespace {

struct ChunkDev { SeqChunkDev seqs; DevBuf hit, paths, steps, obs; };

/* one chunk through the device: its paths, its observations into the support, its F lines behind `text` */
int run_chunk(yakamd_allele *al, yakamd_path_t *px, const yakamd_alopt_t &o, SeqChunk &c, ChunkDev &d, std::string &text, alt_total_t *tot)
{
	const size_t n_seq = c.name.size();
	size_t n = 0;
	if (n_seq == 0) return 0;
	tot->n_seq += n_seq; tot->len += c.bases;
	if (!d.hit.need((size_t)up16(c.img.size()) * 8)) return fail("yakamd_alleles: no device memory for a chunk of %zu bytes", c.img.size());
	if (d.seqs.upload("yakamd_alleles", c, &n, &g_ms[3]) != 0) return -1;
	const uint64_t *d_off = (const uint64_t*)d.seqs.off.p;
	const uint32_t *d_len = (const uint32_t*)d.seqs.len.p;
	if (yakamd_path_hits_dev(px, d.seqs.img.p, (int64_t)n, (uint64_t*)d.hit.p) != 0) return fail_below(yakamd_path_last_error());
	int64_t np[2], again[2], no[2];
	int rc = yakamd_path_chain_dev(px, (const uint64_t*)d.hit.p, (int64_t)n, d_off, d_len, (int64_t)n_seq, 0, 0, 0, 0, 0, np);
	if (rc < 0) return fail_below(yakamd_path_last_error());
	tot->path += (uint64_t)np[0]; tot->step += (uint64_t)np[1];
	if (np[0] == 0) return 0;
	if (!d.paths.need((size_t)np[0] * 32) || !d.steps.need((size_t)np[1] * 8)) return fail("yakamd_alleles: no device memory for %lld paths of %lld steps", (long long)np[0], (long long)np[1]);
	rc = yakamd_path_chain_dev(px, (const uint64_t*)d.hit.p, (int64_t)n, d_off, d_len, (int64_t)n_seq, (yakamd_upath_t*)d.paths.p, np[0], (uint64_t*)d.steps.p, np[1], 0, again);
	if (rc < 0) return fail_below(yakamd_path_last_error());
	if (rc != 0) return fail("yakamd_alleles: the writing call counted %lld paths of %lld steps, the counting call %lld of %lld", (long long)again[0], (long long)again[1], (long long)np[0], (long long)np[1]);
	rc = yakamd_allele_obs_dev(al, (const yakamd_upath_t*)d.paths.p, np[0], (const uint64_t*)d.steps.p, np[1], 0, 0, no);
	if (rc < 0) return -1;
	tot->obs += (uint64_t)no[0]; tot->full += (uint64_t)no[1];
	if (no[0] == 0) return 0;
	if (!d.obs.need((size_t)no[0] * 16)) return fail("yakamd_alleles: no device memory for %lld observations", (long long)no[0]);
	rc = yakamd_allele_obs_dev(al, (const yakamd_upath_t*)d.paths.p, np[0], (const uint64_t*)d.steps.p, np[1], (yakamd_aobs_t*)d.obs.p, no[0], again);
	if (rc < 0) return -1;
	if (rc != 0 || again[0] != no[0] || again[1] != no[1])
		return fail("yakamd_alleles: the writing call counted %lld observations, the counting call %lld", (long long)again[0], (long long)no[0]);
	if (!o.fragments) return 0;
	std::vector<al_obs_t> obs((size_t)no[0]);
	double t0 = now_ms();
	HIPCK(hipMemcpy(obs.data(), d.obs.p, obs.size() * 16, hipMemcpyDeviceToHost));
	g_ms[3] += now_ms() - t0; t0 = now_ms();
	if (!alt_fragments(text, c.name, obs.data(), obs.size(), al->st.n_bubble, (uint64_t)o.min_frag, !o.stats_only, tot))
		return fail("yakamd_alleles: an observation record does not fit its chunk");
	g_ms[4] += now_ms() - t0;
	return 0;
}

}   // namespace

extern "C" int yakamd_alleles(const yakamd_alopt_t *opt, yak_ch_t *ch, const char *reads_fn, const char *out_fn)
{
	if (!opt) return fail("yakamd_alleles: no options");
	if (opt->min_sup < 1) return fail("yakamd_alleles: min_sup %d", opt->min_sup);
	if (opt->min_frag < 1) return fail("yakamd_alleles: min_frag %d", opt->min_frag);
	if (opt->chunk_size < 1) return fail("yakamd_alleles: chunk_size %lld", (long long)opt->chunk_size);
	if (!reads_fn) return fail("yakamd_alleles: no reads");
	if (ch && yakamd_ch_hpc(ch)) return fail("yakamd_alleles: the table is marked homopolymer-compressed: its unitigs are no sequences to lay reads onto");
	SeqReader rd(false);                                           /* of a quality its length alone */
	if (ch && !rd.open(reads_fn)) return fail("yakamd_alleles: cannot read '%s'", reads_fn);
	WalkGuard W{ yakamd_uwalk_open(ch, opt->min_cnt) };
	if (!W.p) return fail_below(yakamd_walk_last_error());
	const int k = ch->k;
	Guard<yakamd_gfa_t, yakamd_gfa_close> G{ yakamd_gfa_open(W.p, k) };
	if (!G.p) return fail_below(yakamd_gfa_last_error());
	Guard<yakamd_bubble_set_t, yakamd_bubble_close> B{ yakamd_bubble_open(W.p, G.p, k) };
	if (!B.p) return fail_below(yakamd_bubble_last_error());
	Guard<yakamd_allele_t, yakamd_allele_close> A{ yakamd_allele_open(W.p, B.p) };
	yakamd_allele_t *al = A.p;
	if (!al) return -1;
	Guard<yakamd_path_t, yakamd_path_close> P{ yakamd_path_open(W.p, k) };
	if (!P.p) return fail_below(yakamd_path_last_error());
	B.close(); G.close(); W.close();
	const u64 n_b = al->st.n_bubble;
	std::vector<bb_rec_t> rec;
	std::vector<al_sup_t> sup;
	try { rec.resize((size_t)n_b); sup.resize((size_t)n_b); } catch (const std::bad_alloc&) { return fail("yakamd_alleles: %llu bubbles do not fit the host's memory", n_b); }
	OutFile out(out_fn);
	if (!out.f) return fail("yakamd_alleles: cannot write '%s'", out.name);
	bool ok = true;
	ChunkDev d;
	std::string text;
	alt_total_t tot = { 0, 0, 0, 0, 0, 0, 0 };
	alt_head(text, k, opt->min_cnt, opt->min_sup);
	if (seq_chunks("yakamd_alleles", rd, reads_fn, opt->chunk_size, 0, [&](SeqChunk &c, bool last) {
		if (run_chunk(al, P.p, *opt, c, d, text, &tot) != 0) return -1;
		flush(text, &out, false, &ok);
		return 0;
	}) != 0) return -1;
	double t0 = now_ms();
	if (n_b) {
		OnDevice dev(al->dev);
		HIPCK(hipMemcpy(rec.data(), al->rec.p, (size_t)n_b * sizeof(bb_rec_t), hipMemcpyDeviceToHost));
		HIPCK(hipMemcpy(sup.data(), al->sup.p, (size_t)n_b * sizeof(al_sup_t), hipMemcpyDeviceToHost));
	}
	g_ms[3] += now_ms() - t0; t0 = now_ms();
	uint64_t n_call[4] = { 0, 0, 0, 0 };
	try {
		alt_alleles(text, rec.data(), sup.data(), n_b, (uint64_t)opt->min_sup, !opt->stats_only, n_call);
		alt_tail(text, tot, n_b, n_call);
	} catch (const std::bad_alloc&) { return fail("yakamd_alleles: no host memory for the text"); }
	flush(text, &out, true, &ok);
	if (!(out.finish() && ok)) return fail("yakamd_alleles: cannot write '%s'", out.name);
	g_ms[4] += now_ms() - t0;
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] alleles: %llu observations (%llu full) of %llu bubbles in %llu steps: arm map %.1f ms, count and scan %.1f ms, emit %.1f ms, copies %.1f ms, text %.1f ms\n",
		        (u64)tot.obs, (u64)tot.full, n_b, (u64)tot.step, g_ms[0], g_ms[1], g_ms[2], g_ms[3], g_ms[4]);
	return 0;
}

LAYER_TALLY_EXPORTS(allele)
