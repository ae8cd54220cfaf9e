/*
 * correct.hip -- libyak_amd_correct.so: single substitution errors of reads repaired on the GPU against a count table (include/yak_amd_correct.h;
 * DESIGN.md section 30).  A layer above libyak_amd.so alone: it calls yakamd_lookup_dev for every probe of the table, yakamd_ch_hpc and
 * seq_nt4_table, nothing else, and owns its device memory (hipMalloc / hipFree).  The per-thread steps are those of correct_step.h, the texts those
 * of correct_text.h, the reader and the chunk loop those of ../layer/layer_seqs.h; every launch goes through the launch macro of ../csrc/tally.h into this library's own
 * tally (yakamd_correct_tally_*).  The host scaffolding and the scan are those of ../layer/layer_host.h and ../layer/layer_dev.h.
 *
 *   k_cor_find<COUNT>  a workgroup per group of eight tiles of 1024 positions of the count array, a tile at a time staged in LDS with one entry in front and k + 1 behind (16-byte
 *                      loads where the array allows them); a thread per position, four rounds of 256.  A position that starts a run looks at most
 *                      k entries ahead and classifies it (cr_run); the candidates of the group are counted into tsum[group].  The same pass adds
 *                      n_kmer, n_weak and n_cand to the tally of each position's sequence -- found among the offsets and lengths of the tile's
 *                      sequences, staged in LDS while they are 96 at the most --: the lanes of a wave that share a sequence are summed first, one
 *                      lane adds for them -- reads of 150 bases put two sequences into most waves -- into counters of the tile in LDS, which go
 *                      to memory once per tile and sequence
 *   k_cor_tile_scan    the exclusive scan of tsum[] by one workgroup (../layer/layer_dev.h), the total behind it
 *   k_cor_find<EMIT>   the same classification; a candidate writes its record at tsum[group] + the candidates of the group's tiles in front + its rank
 *                      in the tile, two 16-byte stores
 *   k_cor_trials       a wave per candidate: the 6k bytes of its three trial windows, the lanes striding over them, so that a wave writes whole lines
 *   k_cor_decide       a wave per candidate: a lane per entry of a trial's counts, a ballot per trial; lane 0 fills from, to, fit and why with one
 *                      8-byte store, writes the corrected byte and adds to the sequence's tally
 * All results are addressed by position and rank; the tallies are integer sums; all stores are vector stores.
 */
#include "yak.h"
#include "yak_amd_correct.h"
#define LAYER_NAME "correct"
#include "../layer/layer_host.h"
#include "../layer/layer_seqs.h"
#include "../layer/layer_dev.h"
#include "correct_step.h"
#include "correct_text.h"

static_assert(sizeof(yakamd_fix_t) == 32 && sizeof(cr_fix_t) == 32 && sizeof(yakamd_ctally_t) == 32 && sizeof(cr_tally_t) == 32 && sizeof(yakamd_cropt_t) == 24,
              "the records as declared");

namespace {

enum { CR_THREADS = 256, CR_ITEMS = 4, CR_TILE = CR_THREADS * CR_ITEMS, CR_WAVE = 64, CR_WAVES = CR_THREADS / CR_WAVE,
       CR_FRONT = 8,                /* entries in front of the tile in LDS: the last of them is position base - 1, the tile itself is 16-byte aligned */
       CR_BACK = 40,                /* entries behind it: k + 1 <= 32, in whole 16-byte words */
       CR_GROUP = 8,                /* consecutive tiles a workgroup takes: one sum of candidates per group keeps the scan over them short */
       CR_SEQS = 96 };              /* sequences of a tile whose offsets and lengths are staged in LDS; a tile that holds more reads them from memory */
/* the words of stat[]: what does not fit -- a rank outside the list in k_cor_find<EMIT>, a record outside the image or on a byte that is no base in
 * k_cor_trials and k_cor_decide */
enum { CRS_BAD_FIND = 0, CRS_BAD_TRIAL = 1, CRS_BAD_DECIDE = 2, CRS_N = 4 };
enum CrMode { COUNT = 0, EMIT = 1 };

struct TileAt {                                                    /* the count array through the tile in LDS: positions base - 1 .. base + CR_TILE + CR_BACK - 1 */
	const uint16_t *s;
	int64_t base;
	__device__ uint32_t operator()(int64_t i) const { return s[i - base + CR_FRONT]; }
};
struct DevBase {
	const uint8_t *b;
	__device__ uint8_t operator()(uint64_t g) const { return b[g]; }
};

__device__ inline void tally_bad(u64 bad, u64 *stat, int at)
{
	bad = wave_sum(bad);
	if ((threadIdx.x & (CR_WAVE - 1)) == 0 && bad) atomicAdd(stat + at, bad);
}

__device__ inline void load_fix(const cr_fix_t *rec, cr_fix_t *r)
{
	const v2 *in = reinterpret_cast<const v2*>(rec);
	const v2 a = in[0], b = in[1];
	r->at = a.x; r->seq = (uint32_t)a.y; r->p = (uint32_t)(a.y >> 32); r->st = (uint32_t)b.x; r->en = (uint32_t)(b.x >> 32);
	r->from = (uint8_t)b.y; r->to = (uint8_t)(b.y >> 8); r->fit = (uint8_t)(b.y >> 16); r->why = (uint8_t)(b.y >> 24); r->reserved = (uint32_t)(b.y >> 32);
}

/* COUNT: tsum[group] = the candidates that start in the group's tiles, and the tallies.  EMIT: tsum[] is scanned, the records are written */
template<int MODE> __global__ __launch_bounds__(CR_THREADS)
void k_cor_find(const uint16_t *__restrict__ cnt, int64_t n, int k, uint32_t c, int min_run, const uint64_t *__restrict__ off, const uint32_t *__restrict__ len, int64_t n_seq,
                u64 *__restrict__ tsum, u64 m, cr_fix_t *__restrict__ rec, u64 n_rec, cr_tally_t *__restrict__ tally, u64 *stat)
{
	__shared__ __attribute__((aligned(16))) uint16_t s_cnt[CR_FRONT + CR_TILE + CR_BACK];
	__shared__ uint32_t s_wc[CR_ITEMS * CR_WAVES];
	__shared__ int64_t s_seq[2];
	__shared__ uint64_t s_off[CR_SEQS];
	__shared__ uint32_t s_len[CR_SEQS];
	__shared__ uint32_t s_tal[CR_SEQS * 3];                            /* COUNT: n_kmer, n_weak and n_cand of the tile's staged sequences */
	const unsigned lane = threadIdx.x & (CR_WAVE - 1), wave = threadIdx.x / CR_WAVE;
	u64 bad = 0;
	const u64 mg = (m + CR_GROUP - 1) / CR_GROUP;
	for (u64 grp = blockIdx.x; grp < mg; grp += gridDim.x) {
	u64 run = MODE == EMIT ? tsum[grp] : 0;                            /* the candidates in front of the tile: of the group (COUNT), of the image (EMIT) */
	int64_t known = -1;                                                /* sequences known to start at or in front of the tile: those of the tile before */
	for (u64 tile = grp * CR_GROUP; tile < m && tile < (grp + 1) * CR_GROUP; ++tile) {
		const int64_t base = (int64_t)tile * CR_TILE;
		for (int v = threadIdx.x; v < (CR_TILE + CR_BACK) / 8; v += CR_THREADS) {
			const int64_t g = base + 8 * v;
			uint16_t *to = s_cnt + CR_FRONT + 8 * v;
			if (g + 8 <= n) *reinterpret_cast<uint4*>(to) = *reinterpret_cast<const uint4*>(cnt + g);      /* cnt is 16-byte aligned, g a multiple of 8 */
			else for (int e = 0; e < 8; ++e) to[e] = g + e < n ? cnt[g + e] : (uint16_t)CR_NONE;
		}
		if (threadIdx.x == CR_THREADS - 1) s_cnt[CR_FRONT - 1] = base > 0 ? cnt[base - 1] : (uint16_t)CR_NONE;
		/* the sequences that can hold a position of the tile: from the last one that starts at or in front of its first position.  A binary search
		 * over all sequences is some twenty dependent reads by one thread while the workgroup waits: only the group's first tile pays it */
		if (threadIdx.x == 0) {
			const int64_t u = known < 0 ? cr_seq_upto(off, n_seq, (uint64_t)base) : cr_seq_upto_from(off, n_seq, known, (uint64_t)base);
			s_seq[0] = u > 0 ? u - 1 : 0;
		}
		if (threadIdx.x == CR_WAVE) {
			const uint64_t last = (uint64_t)(base + CR_TILE < n ? base + CR_TILE : n) - 1;
			s_seq[1] = known < 0 ? cr_seq_upto(off, n_seq, last) : cr_seq_upto_from(off, n_seq, known, last);
		}
		__syncthreads();
		known = s_seq[1];
		const TileAt at{ s_cnt, base };
		const int64_t s_lo = s_seq[0], n_s = s_seq[1] - s_seq[0];
		const bool staged = n_s <= CR_SEQS;                            /* uniform in the workgroup */
		if (staged) {
			for (int j = threadIdx.x; j < n_s; j += CR_THREADS) { s_off[j] = off[s_lo + j]; s_len[j] = len[s_lo + j]; s_tal[3 * j] = s_tal[3 * j + 1] = s_tal[3 * j + 2] = 0; }
			__syncthreads();
		}
		const uint64_t *t_off = staged ? s_off : off + s_lo;           /* the tile's sequences, numbered from s_lo */
		const uint32_t *t_len = staged ? s_len : len + s_lo;
		bool cand[CR_ITEMS];
		uint32_t seq[CR_ITEMS], st[CR_ITEMS], en[CR_ITEMS], p[CR_ITEMS], rank[CR_ITEMS];
#pragma unroll
		for (int it = 0; it < CR_ITEMS; ++it) {
			const int64_t i = base + it * CR_THREADS + (int64_t)threadIdx.x;
			const uint32_t v = at(i);                                   /* CR_NONE from n on */
			const bool starts = cr_weak(v, c) && !cr_weak(at(i - 1), c);
			/* the tallies want the sequence of every position that exists, the records that of a run's first position alone */
			const int64_t s = (MODE == COUNT ? cr_exists(v) != 0 : starts) ? cr_seq_of(t_off, t_len, 0, n_s, (uint64_t)i) : -1;
			const bool in = s >= 0, wk = in && cr_weak(v, c);
			cand[it] = false; seq[it] = (uint32_t)(s_lo + s); st[it] = en[it] = p[it] = 0;
			if (in && starts) {
				int run_len;
				st[it] = (uint32_t)((uint64_t)i - t_off[s]);
				cand[it] = cr_run(at, i, st[it], k, c, min_run, &en[it], &p[it], &run_len) != 0;
			}
			const u64 cmask = __ballot(cand[it]);
			rank[it] = (uint32_t)__popcll(cmask & (((u64)1 << lane) - 1));
			if (lane == 0) s_wc[it * CR_WAVES + wave] = (uint32_t)__popcll(cmask);
			if (MODE == COUNT && tally) {
				/* per sequence of the wave: its lanes summed, one lane adds -- into the tile's counters in LDS while the sequences are staged,
				 * which go to memory once per tile and sequence below.  21 bits a counter: a wave adds 64 at the most */
				const u64 own = (u64)in | (u64)wk << 21 | (u64)cand[it] << 42;
				u64 todo = __ballot(in);
				while (todo) {
					const int lead = __ffsll((long long)todo) - 1;
					const uint32_t sj = (uint32_t)__shfl((int)seq[it], lead);
					const bool mine = in && seq[it] == sj;
					const u64 sum = wave_sum(mine ? own : 0);
					if (lane == 0) {
						const uint32_t nk = (uint32_t)(sum & 0x1fffff), nw = (uint32_t)(sum >> 21 & 0x1fffff), nc = (uint32_t)(sum >> 42);
						if (staged) {
							uint32_t *t3 = s_tal + 3 * (sj - (uint32_t)s_lo);      /* sj - s_lo < n_s <= CR_SEQS: cr_seq_of */
							atomicAdd(t3, nk);
							if (nw) atomicAdd(t3 + 1, nw);
							if (nc) atomicAdd(t3 + 2, nc);
						} else {
							atomicAdd(&tally[sj].n_kmer, nk);
							if (nw) { atomicAdd(&tally[sj].n_weak, nw); atomicAdd(&tally[sj].n_weak_after, nw); }
							if (nc) atomicAdd(&tally[sj].n_cand, nc);
						}
					}
					todo &= ~__ballot(mine);
				}
			}
		}
		__syncthreads();
		u64 in_tile = 0;
		for (int j = 0; j < CR_ITEMS * CR_WAVES; ++j) in_tile += s_wc[j];
		if (MODE == COUNT) {
			if (tally && staged) {
				for (int j = threadIdx.x; j < n_s; j += CR_THREADS) {
					const uint32_t nk = s_tal[3 * j], nw = s_tal[3 * j + 1], nc = s_tal[3 * j + 2];
					cr_tally_t *t = tally + s_lo + j;
					/* n_kmer and n_weak are the two halves of the record's first 8 bytes: one atomic; n_kmer stays below 2^32 and carries nothing over */
					if (nk) atomicAdd(reinterpret_cast<u64*>(t), (u64)nk | (u64)nw << 32);
					if (nw) atomicAdd(&t->n_weak_after, nw);
					if (nc) atomicAdd(&t->n_cand, nc);
				}
			}
		} else {
			const u64 first = run;
#pragma unroll
			for (int it = 0; it < CR_ITEMS; ++it) {
				if (!cand[it]) continue;
				u64 r = first + rank[it];
				for (int j = 0; j < it * CR_WAVES + (int)wave; ++j) r += s_wc[j];
				if (r >= n_rec) { ++bad; continue; }                       /* a rank outside the list: tallied, not written */
				v2 *out = reinterpret_cast<v2*>(rec + r);
				out[0] = make_ulonglong2(base + it * CR_THREADS + (u64)threadIdx.x - st[it] + p[it], (u64)seq[it] | (u64)p[it] << 32);
				out[1] = make_ulonglong2((u64)st[it] | (u64)en[it] << 32, 0);
			}
		}
		run += in_tile;
		__syncthreads();                                               /* the next tile writes s_cnt, s_wc and s_seq again */
	}
	if (MODE == COUNT && threadIdx.x == 0) tsum[grp] = run;
	}
	if (MODE == EMIT) tally_bad(bad, stat, CRS_BAD_FIND);
}

__global__ __launch_bounds__(CR_THREADS)
void k_cor_tile_scan(u64 *__restrict__ tsum, u64 m) { tile_scan<CR_THREADS, u64, AddU64>(tsum, m); }

/* a wave per record: the three trial windows, 6k bytes, and behind the last record the newlines up to a multiple of 16 */
__global__ __launch_bounds__(CR_THREADS)
void k_cor_trials(const uint8_t *__restrict__ bases, u64 n_bytes, const cr_fix_t *__restrict__ rec, u64 n_rec, int k, uint8_t *__restrict__ trials, u64 *stat)
{
	const unsigned lane = threadIdx.x & (CR_WAVE - 1);
	const u64 stride = 6 * (u64)k;
	u64 bad = 0;
	for (u64 i = (u64)blockIdx.x * CR_WAVES + threadIdx.x / CR_WAVE; i < n_rec; i += (u64)gridDim.x * CR_WAVES) {      /* uniform in the wave */
		cr_fix_t r;
		load_fix(rec + i, &r);
		const int o = cr_rec_ok(&r, k, n_bytes, -1) ? cr_nt4(bases[r.at]) : 4;
		if (o > 3) {                                                   /* tallied; its windows are newlines */
			bad += lane == 0;
			for (u64 j = lane; j < stride; j += CR_WAVE) trials[stride * i + j] = (uint8_t)'\n';
			continue;
		}
		for (u64 j = lane; j < stride; j += CR_WAVE) trials[stride * i + j] = cr_trial_byte(DevBase{ bases }, &r, k, o, (int)j);
	}
	const u64 end = stride * n_rec, pad = (end + 15) / 16 * 16 - end;
	if (blockIdx.x == 0 && threadIdx.x < pad) trials[end + threadIdx.x] = (uint8_t)'\n';
	tally_bad(bad, stat, CRS_BAD_TRIAL);
}

/* a wave per record: the three trials reduced, the decision, the corrected byte, the sequence's tally */
__global__ __launch_bounds__(CR_THREADS)
void k_cor_decide(const uint16_t *__restrict__ tc, cr_fix_t *__restrict__ rec, u64 n_rec, int k, uint32_t c, uint8_t *__restrict__ bases, u64 n_bytes,
                  cr_tally_t *__restrict__ tally, int64_t n_seq, u64 *stat)
{
	const unsigned lane = threadIdx.x & (CR_WAVE - 1);
	u64 bad = 0;
	for (u64 i = (u64)blockIdx.x * CR_WAVES + threadIdx.x / CR_WAVE; i < n_rec; i += (u64)gridDim.x * CR_WAVES) {      /* uniform in the wave */
		cr_fix_t r;
		load_fix(rec + i, &r);
		const bool ok = cr_rec_ok(&r, k, n_bytes, n_seq) != 0;
		const uint8_t from = ok ? bases[r.at] : 0;
		const int o = ok ? cr_nt4(from) : 4;
		if (o > 3) { bad += lane == 0; continue; }
		const unsigned run = r.en - r.st;                              /* 1 .. k: a lane per entry */
		int fit = 0;
		for (int a = 0; a < 3; ++a) {
			const uint32_t v = lane < run ? tc[cr_trial_entry(i, a, k, (int)lane)] : c;
			if (__ballot(lane < run && !(cr_exists(v) && !cr_weak(v, c))) == 0) fit |= 1 << cr_trial_code(o, a);
		}
		if (lane == 0) {
			uint8_t to;
			const int why = cr_decide(fit, from, &to);
			reinterpret_cast<u64*>(rec + i)[3] = (u64)from | (u64)to << 8 | (u64)fit << 16 | (u64)why << 24;
			if (why == CR_DONE) bases[r.at] = to;
			if (tally) {
				atomicAdd(why == CR_DONE ? &tally[r.seq].n_fixed : why == CR_AMBIG ? &tally[r.seq].n_ambig : &tally[r.seq].n_nofit, 1u);
				if (why == CR_DONE) atomicSub(&tally[r.seq].n_weak_after, run);
			}
		}
	}
	tally_bad(bad, stat, CRS_BAD_DECIDE);
}

/* ---------------- host ---------------- */

thread_local double g_ms[6];                                       /* of this thread's last call */
enum { MS_LOOKUP1 = 0, MS_FIND = 1, MS_TRIALS = 2, MS_LOOKUP2 = 3, MS_DECIDE = 4, MS_TEXT = 5 };


/* device memory kept from one image to the next */
struct Work {
	DevBuf tsum, stat, cnt, fix, trials, tcnt;
};

/* the step's own base table is the library's */
int nt4_check()
{
	for (int b = 0; b < 256; ++b) if (cr_nt4((uint8_t)b) != seq_nt4_table[b]) return fail("correct: byte %d has code %d in seq_nt4_table", b, seq_nt4_table[b]);
	return 0;
}

int check_opts(const char *who, int k, int min_cnt, int min_run)
{
	if (k < 1 || k >= 32) return fail("%s: k = %d: k must be below 32 (reference qv.c:44)", who, k);
	if (min_cnt < 1 || min_cnt > YAK_MAX_COUNT) return fail("%s: min_cnt %d: it must be in [1, %d]", who, min_cnt, YAK_MAX_COUNT);
	if (min_run < 1 || min_run > k) return fail("%s: min_run %d: it must be in [1, k = %d]", who, min_run, k);
	return 0;
}
int check_sizes(const char *who, int64_t n_bytes, int64_t n_seq)
{
	if (n_bytes < 0 || n_bytes > (int64_t)1 << 40 || n_seq < 0 || n_seq > (int64_t)0xfffffffe) return fail("%s: bad n_bytes or n_seq", who);
	return 0;
}
int check_seqs(const char *who, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq, const yakamd_ctally_t *d_tally)
{
	if (n_seq > 0 && (!d_seq_off || !d_seq_len)) return fail("%s: %lld sequences without their offsets or lengths", who, (long long)n_seq);
	if (((uintptr_t)d_seq_off & 7) != 0 || ((uintptr_t)d_seq_len & 3) != 0 || ((uintptr_t)d_tally & 15) != 0)
		return fail("%s: the offsets must be 8-byte, the lengths 4-byte and the tallies 16-byte aligned", who);
	return 0;
}

int read_stat(Work &w, u64 *h_stat) { HIPCK(hipMemcpy(h_stat, w.stat.p, CRS_N * 8, hipMemcpyDeviceToHost)); return 0; }

/* the candidates counted, with the tallies; the scanned tile sums stay in w.tsum for find_emit */
int64_t find_count(Work &w, int k, int min_cnt, int min_run, const void *d_cnt, int64_t n_bytes, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                   yakamd_ctally_t *d_tally)
{
	if (d_tally && n_seq > 0) HIPCK(hipMemset(d_tally, 0, (size_t)n_seq * sizeof(yakamd_ctally_t)));
	if (n_bytes == 0) return 0;
	const u64 m = ((u64)n_bytes + CR_TILE - 1) / CR_TILE, mg = (m + CR_GROUP - 1) / CR_GROUP;
	if (!w.tsum.need((mg + 1) * 8) || !w.stat.need(CRS_N * 8)) return fail("correct: no device memory for %llu bytes", (mg + 1) * 8);
	HIPCK(hipMemset(w.stat.p, 0, CRS_N * 8));
	YK_LAUNCH(k_cor_find<COUNT>, dim3((unsigned)(mg < (1u << 20) ? mg : (1u << 20))), dim3(CR_THREADS), 0, 0, (const uint16_t*)d_cnt, n_bytes, k, (uint32_t)min_cnt, min_run, d_seq_off,
	          d_seq_len, n_seq, (u64*)w.tsum.p, m, (cr_fix_t*)0, (u64)0, (cr_tally_t*)d_tally, (u64*)w.stat.p);
	YK_LAUNCH(k_cor_tile_scan, dim3(1), dim3(CR_THREADS), 0, 0, (u64*)w.tsum.p, mg);
	HIPCK(hipGetLastError());
	u64 total = 0;
	HIPCK(hipMemcpy(&total, (u64*)w.tsum.p + mg, 8, hipMemcpyDeviceToHost));
	return (int64_t)total;
}

/* their records, after find_count on the same arguments */
int find_emit(Work &w, int k, int min_cnt, int min_run, const void *d_cnt, int64_t n_bytes, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
              yakamd_fix_t *d_fix, int64_t n_fix)
{
	const u64 m = ((u64)n_bytes + CR_TILE - 1) / CR_TILE, mg = (m + CR_GROUP - 1) / CR_GROUP;
	YK_LAUNCH(k_cor_find<EMIT>, dim3((unsigned)(mg < (1u << 20) ? mg : (1u << 20))), dim3(CR_THREADS), 0, 0, (const uint16_t*)d_cnt, n_bytes, k, (uint32_t)min_cnt, min_run, d_seq_off,
	          d_seq_len, n_seq, (u64*)w.tsum.p, m, (cr_fix_t*)d_fix, (u64)n_fix, (cr_tally_t*)0, (u64*)w.stat.p);
	HIPCK(hipGetLastError());
	u64 h_stat[CRS_N];
	if (read_stat(w, h_stat) != 0) return -1;
	if (h_stat[CRS_BAD_FIND]) return fail("correct: %llu candidates have no place in the list of %lld records", h_stat[CRS_BAD_FIND], (long long)n_fix);
	return 0;
}

int trials_run(Work &w, int k, const void *d_bases, int64_t n_bytes, const yakamd_fix_t *d_fix, int64_t n_fix, void *d_trials)
{
	if (!w.stat.need(CRS_N * 8)) return fail("correct: no device memory");
	HIPCK(hipMemset(w.stat.p, 0, CRS_N * 8));
	YK_LAUNCH(k_cor_trials, dim3(grid_for((u64)n_fix * CR_WAVE, CR_THREADS)), dim3(CR_THREADS), 0, 0, (const uint8_t*)d_bases, (u64)n_bytes, (const cr_fix_t*)d_fix, (u64)n_fix, k,
	          (uint8_t*)d_trials, (u64*)w.stat.p);
	HIPCK(hipGetLastError());
	u64 h_stat[CRS_N];
	if (read_stat(w, h_stat) != 0) return -1;
	if (h_stat[CRS_BAD_TRIAL]) return fail("correct: %llu of the %lld records do not lie inside the image of %lld bytes, or on a byte that is no base", h_stat[CRS_BAD_TRIAL],
	                                       (long long)n_fix, (long long)n_bytes);
	return 0;
}

int decide_run(Work &w, int k, int min_cnt, const void *d_tcnt, yakamd_fix_t *d_fix, int64_t n_fix, void *d_bases, int64_t n_bytes, yakamd_ctally_t *d_tally, int64_t n_seq)
{
	if (!w.stat.need(CRS_N * 8)) return fail("correct: no device memory");
	HIPCK(hipMemset(w.stat.p, 0, CRS_N * 8));
	YK_LAUNCH(k_cor_decide, dim3(grid_for((u64)n_fix * CR_WAVE, CR_THREADS)), dim3(CR_THREADS), 0, 0, (const uint16_t*)d_tcnt, (cr_fix_t*)d_fix, (u64)n_fix, k, (uint32_t)min_cnt,
	          (uint8_t*)d_bases, (u64)n_bytes, (cr_tally_t*)d_tally, d_tally ? n_seq : (int64_t)-1, (u64*)w.stat.p);
	HIPCK(hipGetLastError());
	u64 h_stat[CRS_N];
	if (read_stat(w, h_stat) != 0) return -1;
	if (h_stat[CRS_BAD_DECIDE]) return fail("correct: %llu of the %lld records do not lie inside the image of %lld bytes and the %lld sequences, or on a byte that is no base",
	                                        h_stat[CRS_BAD_DECIDE], (long long)n_fix, (long long)n_bytes, (long long)n_seq);
	return 0;
}

/* what a correction refuses of a table and its options, before any device work; the empty lookup is the library below saying what it refuses */
int table_check(const char *who, yak_ch_t *h, int min_cnt, int min_run)
{
	if (!h) return fail("%s: not an engine table", who);
	if (yakamd_ch_hpc(h)) return fail("%s: the table is marked homopolymer-compressed: its k-mers are not those of the reads as they are written", who);
	if (min_cnt < 1 || min_cnt > YAK_MAX_COUNT) return fail("%s: min_cnt %d: it must be in [1, %d]", who, min_cnt, YAK_MAX_COUNT);
	if (yakamd_lookup_dev(h, 0, 0, 0) != 0) return fail_below(yakamd_last_error());
	if (check_opts(who, h->k, min_cnt, min_run) != 0 || nt4_check() != 0) return -1;
	return 0;
}

/* lookup, find, trials, lookup and decide on one image in place; *fix: where the records are, the caller's list or w.fix */
int64_t image_run(Work &w, yak_ch_t *h, int min_cnt, int min_run, void *d_bases, int64_t n_bytes, const uint64_t *d_seq_off, const uint32_t *d_seq_len, int64_t n_seq,
                  yakamd_fix_t *d_fix, int64_t cap, yakamd_ctally_t *d_tally, yakamd_fix_t **fix)
{
	const int k = h->k;
	if (fix) *fix = 0;
	if (n_bytes == 0) return find_count(w, k, min_cnt, min_run, 0, 0, d_seq_off, d_seq_len, n_seq, d_tally);
	if (!w.cnt.need(up16((u64)n_bytes) * 2)) return fail("correct: no device memory for the counts of %lld bytes", (long long)n_bytes);
	double t0 = now_ms();
	if (yakamd_lookup_dev(h, d_bases, n_bytes, w.cnt.p) != 0) return fail_below(yakamd_last_error());
	g_ms[MS_LOOKUP1] += now_ms() - t0; t0 = now_ms();
	const int64_t n_fix = find_count(w, k, min_cnt, min_run, w.cnt.p, n_bytes, d_seq_off, d_seq_len, n_seq, d_tally);
	if (n_fix <= 0) { g_ms[MS_FIND] += now_ms() - t0; return n_fix; }
	yakamd_fix_t *list = d_fix && cap >= n_fix ? d_fix : 0;
	if (!list) {
		if (!w.fix.need((size_t)n_fix * sizeof(cr_fix_t))) return fail("correct: no device memory for %lld records", (long long)n_fix);
		list = (yakamd_fix_t*)w.fix.p;
	}
	if (find_emit(w, k, min_cnt, min_run, w.cnt.p, n_bytes, d_seq_off, d_seq_len, n_seq, list, n_fix) != 0) return -1;
	g_ms[MS_FIND] += now_ms() - t0; t0 = now_ms();
	const u64 t_bytes = up16(6 * (u64)k * (u64)n_fix);
	if (!w.trials.need(t_bytes) || !w.tcnt.need(t_bytes * 2)) return fail("correct: no device memory for the trials of %lld candidates", (long long)n_fix);
	if (trials_run(w, k, d_bases, n_bytes, list, n_fix, w.trials.p) != 0) return -1;
	g_ms[MS_TRIALS] += now_ms() - t0; t0 = now_ms();
	if (yakamd_lookup_dev(h, w.trials.p, (int64_t)t_bytes, w.tcnt.p) != 0) return fail_below(yakamd_last_error());
	g_ms[MS_LOOKUP2] += now_ms() - t0; t0 = now_ms();
	if (decide_run(w, k, min_cnt, w.tcnt.p, list, n_fix, d_bases, n_bytes, d_tally, n_seq) != 0) return -1;
	g_ms[MS_DECIDE] += now_ms() - t0;
	if (fix) *fix = list;
	return n_fix;
}

}   // namespace

extern "C" const char *yakamd_correct_last_error(void) { return g_err; }
extern "C" void yakamd_correct_ms(double ms[6]) { for (int i = 0; i < 6; ++i) ms[i] = g_ms[i]; }
extern "C" void yakamd_cropt_init(yakamd_cropt_t *o) { o->min_cnt = 3; o->min_run = 1; o->list = 0; o->stats_only = 0; o->chunk_size = (int64_t)1 << 28; }

extern "C" int64_t yakamd_correct_find_dev(int k, int min_cnt, int min_run, const void *d_cnt_u16, int64_t n_bytes, const uint64_t *d_seq_off, const uint32_t *d_seq_len,
                                           int64_t n_seq, yakamd_fix_t *d_fix, int64_t cap, yakamd_ctally_t *d_tally)
{
	const char *who = "correct find";
	if (check_opts(who, k, min_cnt, min_run) != 0 || check_sizes(who, n_bytes, n_seq) != 0 || check_seqs(who, d_seq_off, d_seq_len, n_seq, d_tally) != 0) return -1;
	if (n_bytes > 0 && !d_cnt_u16) return fail("%s: no count array", who);
	if ((((uintptr_t)d_cnt_u16 | (uintptr_t)d_fix) & 15) != 0) return fail("%s: the counts and the records must be 16-byte aligned", who);
	Work w;
	const int64_t n_fix = find_count(w, k, min_cnt, min_run, d_cnt_u16, n_bytes, d_seq_off, d_seq_len, n_seq, d_tally);
	if (n_fix <= 0 || !d_fix || cap < n_fix) { if (n_fix >= 0) HIPCK(hipDeviceSynchronize()); return n_fix; }
	return find_emit(w, k, min_cnt, min_run, d_cnt_u16, n_bytes, d_seq_off, d_seq_len, n_seq, d_fix, n_fix) != 0 ? -1 : n_fix;
}

extern "C" int64_t yakamd_correct_trials_dev(int k, const void *d_bases, int64_t n_bytes, const yakamd_fix_t *d_fix, int64_t n_fix, void *d_trials, int64_t cap_bytes)
{
	const char *who = "correct trials";
	if (k < 1 || k >= 32) return fail("%s: k = %d: k must be below 32 (reference qv.c:44)", who, k);
	if (check_sizes(who, n_bytes, 0) != 0 || n_fix < 0 || n_fix > n_bytes) return fail("%s: bad n_bytes or n_fix", who);
	if ((((uintptr_t)d_bases | (uintptr_t)d_fix | (uintptr_t)d_trials) & 15) != 0) return fail("%s: the image, the records and the trials must be 16-byte aligned", who);
	const int64_t need = (int64_t)up16(6 * (u64)k * (u64)n_fix);
	if (!d_trials || cap_bytes < need) return need;
	if (n_fix == 0) return 0;
	if (!d_bases || !d_fix) return fail("%s: no image or no records", who);
	if (nt4_check() != 0) return -1;
	Work w;
	return trials_run(w, k, d_bases, n_bytes, d_fix, n_fix, d_trials) != 0 ? -1 : need;
}

extern "C" int yakamd_correct_decide_dev(int k, int min_cnt, const void *d_trial_cnt_u16, yakamd_fix_t *d_fix, int64_t n_fix, void *d_bases, int64_t n_bytes,
                                         yakamd_ctally_t *d_tally, int64_t n_seq)
{
	const char *who = "correct decide";
	if (check_opts(who, k, min_cnt, 1) != 0 || check_sizes(who, n_bytes, n_seq) != 0 || n_fix < 0 || n_fix > n_bytes) return fail("%s: bad k, min_cnt, n_bytes, n_seq or n_fix", who);
	if ((((uintptr_t)d_trial_cnt_u16 | (uintptr_t)d_fix | (uintptr_t)d_bases | (uintptr_t)d_tally) & 15) != 0)
		return fail("%s: the counts, the records, the image and the tallies must be 16-byte aligned", who);
	if (n_fix == 0) return 0;
	if (!d_trial_cnt_u16 || !d_fix || !d_bases) return fail("%s: no counts, no records or no image", who);
	if (nt4_check() != 0) return -1;
	Work w;
	return decide_run(w, k, min_cnt, d_trial_cnt_u16, d_fix, n_fix, d_bases, n_bytes, d_tally, n_seq);
}

extern "C" int64_t yakamd_correct_image_dev(yak_ch_t *h, int min_cnt, int min_run, void *d_bases, int64_t n_bytes, const uint64_t *d_seq_off, const uint32_t *d_seq_len,
                                            int64_t n_seq, yakamd_fix_t *d_fix, int64_t cap, yakamd_ctally_t *d_tally)
{
	const char *who = "correct image";
	for (int i = 0; i < 6; ++i) g_ms[i] = 0;
	if (!h) return fail("%s: not an engine table", who);
	if (check_sizes(who, n_bytes, n_seq) != 0 || check_seqs(who, d_seq_off, d_seq_len, n_seq, d_tally) != 0) return -1;
	if (n_bytes > 0 && !d_bases) return fail("%s: no image", who);
	if ((((uintptr_t)d_bases | (uintptr_t)d_fix) & 15) != 0) return fail("%s: the image and the records must be 16-byte aligned", who);
	if (table_check(who, h, min_cnt, min_run) != 0) return -1;
	Work w;
	return image_run(w, h, min_cnt, min_run, d_bases, n_bytes, d_seq_off, d_seq_len, n_seq, d_fix, cap, d_tally, 0);
}

/* ---- the command ---- */
namespace {

struct ChunkDev { SeqChunkDev seqs; DevBuf tally; };

/* one chunk through the device; its lines behind `report`, its reads behind `reads` */
int run_chunk(Work &w, yak_ch_t *h, const yakamd_cropt_t &o, SeqChunk &c, ChunkDev &d, std::string &report, std::string &reads, crt_total_t *tot, OutFile *report_out,
              OutFile *reads_out, bool *ok)
{
	const size_t n_seq = c.name.size();
	size_t n = 0;
	if (n_seq == 0) return 0;
	double t0 = now_ms();
	if (!d.tally.need(n_seq * sizeof(cr_tally_t))) return fail("yakamd_correct: no device memory for a chunk of %zu bytes", c.img.size());
	if (d.seqs.upload("yakamd_correct", c, &n, 0) != 0) return -1;
	g_ms[MS_TEXT] += now_ms() - t0;
	yakamd_fix_t *d_fix = 0;
	const int64_t n_fix = image_run(w, h, o.min_cnt, o.min_run, d.seqs.img.p, (int64_t)n, (const uint64_t*)d.seqs.off.p, (const uint32_t*)d.seqs.len.p, (int64_t)n_seq, 0, 0,
	                                (yakamd_ctally_t*)d.tally.p, &d_fix);
	if (n_fix < 0) return -1;
	t0 = now_ms();
	std::vector<cr_tally_t> tally(n_seq);
	std::vector<cr_fix_t> fix;
	HIPCK(hipMemcpy(tally.data(), d.tally.p, n_seq * sizeof(cr_tally_t), hipMemcpyDeviceToHost));
	if (n_fix > 0 && !o.stats_only) HIPCK(hipMemcpy(c.img.data(), d.seqs.img.p, n, hipMemcpyDeviceToHost));
	if (n_fix > 0 && o.list) {
		fix.resize((size_t)n_fix);
		HIPCK(hipMemcpy(fix.data(), d_fix, (size_t)n_fix * sizeof(cr_fix_t), hipMemcpyDeviceToHost));
	}
	size_t f = 0;
	for (size_t j = 0; j < n_seq; ++j) {
		crt_seq(report, c.name[j], c.len[j], tally[j], tot);
		for (; f < fix.size() && fix[f].seq <= j; ++f) if (fix[f].seq == j && fix[f].why == CR_DONE) crt_fix(report, c.name[j], fix[f]);
		if (!o.stats_only) crt_read(reads, c.name[j], c.comment[j], c.qual[j], c.img.data() + c.off[j], c.len[j]);
		flush(reads, reads_out, false, ok);
		flush(report, report_out, false, ok);
	}
	g_ms[MS_TEXT] += now_ms() - t0;
	return 0;
}

}   // namespace

extern "C" int yakamd_correct(const yakamd_cropt_t *o, yak_ch_t *ch, const char *fn, const char *out_fn, const char *report_fn)
{
	for (int i = 0; i < 6; ++i) g_ms[i] = 0;
	if (!o) return fail("yakamd_correct: no options");
	if (o->chunk_size < 1) return fail("yakamd_correct: chunk_size %lld", (long long)o->chunk_size);
	if (table_check("yakamd_correct", ch, o->min_cnt, o->min_run) != 0) return -1;
	if (!fn) return fail("yakamd_correct: no reads");
	SeqReader rd(true);                                            /* the qualities are written out again */
	if (!rd.open(fn)) return fail("yakamd_correct: cannot read '%s'", fn);
	struct Out {                                                   /* an output that may be absent */
		OutFile *f;
		explicit Out(bool on, const char *name) : f(on ? new (std::nothrow) OutFile(name) : 0) {}
		~Out() { delete f; }
	} reads_out(!o->stats_only, out_fn), report_out(report_fn != 0, report_fn);
	if (!o->stats_only && (!reads_out.f || !reads_out.f->f)) return fail("yakamd_correct: cannot write '%s'", out_fn ? out_fn : "-");
	if (report_fn && (!report_out.f || !report_out.f->f)) return fail("yakamd_correct: cannot write '%s'", report_fn);
	bool ok = true;
	Work w;
	ChunkDev d;
	std::string report, reads;
	crt_total_t tot;
	memset(&tot, 0, sizeof tot);
	crt_head(report, ch->k, o->min_cnt, o->min_run);
	if (seq_chunks("yakamd_correct", rd, fn, o->chunk_size, &g_ms[MS_TEXT], [&](SeqChunk &c, bool last) {
		if (run_chunk(w, ch, *o, c, d, report, reads, &tot, report_out.f, reads_out.f, &ok) != 0) return -1;
		const double t0 = now_ms();
		if (last) crt_last(report, tot);
		flush(reads, reads_out.f, last, &ok);
		flush(report, report_out.f, last, &ok);
		g_ms[MS_TEXT] += now_ms() - t0;
		return 0;
	}) != 0) return -1;
	if (reads_out.f && !(reads_out.f->finish() && ok)) return fail("yakamd_correct: cannot write '%s'", reads_out.f->name);
	if (report_out.f && !(report_out.f->finish() && ok)) return fail("yakamd_correct: cannot write '%s'", report_out.f->name);
	if (getenv("YAKAMD_VERBOSE"))
		fprintf(stderr, "[yak_amd] correct: lookup %.1f ms, find %.1f ms, trials %.1f ms, second lookup %.1f ms, decisions %.1f ms, text %.1f ms\n", g_ms[0], g_ms[1], g_ms[2],
		        g_ms[3], g_ms[4], g_ms[5]);
	return 0;
}

LAYER_TALLY_EXPORTS(correct)
