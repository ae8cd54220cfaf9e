/* kern_trioeval.inc -- part of kernels.hip (one translation unit): the streak reduction of `yak trioeval` (reference trioeval.c:89-116)
 * over the flags k_lookup<uint8_t> writes (yakamd_triobin_lookup_dev).
 *
 * A position's type is 1 where its flag is 2 (pat solid, mat absent), 2 where it is 8, 0 elsewhere (also where no k-mer ends, TB_NOKMER).
 * A streak is a maximal run [s, e) of one type t > 0 with e - s >= min_n.  The '\n' after every record of an image has no k-mer, so a typed
 * run never crosses a record: the runs are found over the whole flag array as one flat array of positions, with no notion of records, and
 * their cost does not depend on how long a record is (k_tb_reduce walks one read with one wave; a 100 Mb contig would be a million steps).
 *   k_te_runs<0>   per tile of TE_TILE positions: the number of run starts (t > 0, t != type before) and run ends (t > 0, t != type after)
 *   k_te_scan      exclusive scans of those tile counts (one block per array)
 *   k_te_runs<1>   the starts and the (exclusive) ends scattered in position order: start j pairs with end j, however many tiles the run spans
 *   k_te_keep<0>   per block of runs: the number with e - s >= min_n
 *   k_te_keep<1>   the kept runs compacted in order as {record, s, e, t} (record-relative s and e; the record by binary search over off[])
 *   k_te_seq       per record d[2] and c[4] (trioeval.c:92-99): each thread folds TE_ITEMS consecutive streaks, closing a record with
 *                  atomics when the record changes; what is open at the end is combined across the wave by a segmented scan (the list is
 *                  ordered by record), so a record with millions of streaks costs one atomic per counter and wave
 * Buffers are sized from the counts, never from one run per position: the host reads the number of runs back once, and sizes the
 * streak list by it (k_te_seq reads the number kept on the device).
 *
 * The run finder's map from a byte to a type is its template parameter M: TeMapTrio above, or TeMapLow for `yak chkerr` (reference
 * chkerr.c:60-67), whose bytes k_lookup<uint8_t, ., true> writes: 1 where the k-mer is low, so a run of type 1 is a streak of low k-mers at
 * consecutive end positions, broken by a k-mer that is not low and by a position where none ends.  chkerr keeps a run when e - s > min_streak
 * (min_n = min_streak + 1) and needs no per-record counters: k_te_seq is trioeval's alone.
 *
 * k_sc_reduce is `yak sexchr`'s tally (reference sexchr.c:57-65) over the flags of the three SEXCHR loads, also flat over the array: each thread
 * folds TE_PER positions (one 16-byte load) of each of SC_ITERS tiles, their record found by a binary search over off[] and searched again when
 * a later record starts; a record closed inside a thread is added with atomics, the one open at its end by a segmented scan over the wave
 * (records ascend with the lanes), so a chromosome-length record costs one atomic per counter and wave.
 */
#define TE_THREADS 256
#define TE_PER 16                              /* positions per thread: one 16-byte load */
#define TE_TILE (TE_THREADS * TE_PER)
#define TE_ITEMS 16                            /* runs or streaks per thread in k_te_keep / k_te_seq */
#define TE_NONE 0xffffffffu

/* the position-to-type maps of the run finder: trioeval's flags (2 -> 1, 8 -> 2) and chkerr's low bytes (1 -> 1; 0 and CE_NOKMER -> 0) */
struct TeMapTrio { static __device__ __forceinline__ u32 type(u32 v) { return v == 2u ? 1u : v == 8u ? 2u : 0u; } };
struct TeMapLow { static __device__ __forceinline__ u32 type(u32 v) { return v == 1u ? 1u : 0u; } };

/* exclusive prefix of x over the block's TE_THREADS threads; *total = the block's sum */
__device__ __forceinline__ u32 te_block_scan(u32 x, u32 *total)
{
	__shared__ u32 s_w[TE_THREADS / WAVE];
	const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
	u32 inc = x;
#pragma unroll
	for (int o = 1; o < WAVE; o <<= 1) { const u32 y = __shfl_up(inc, o); if (lane >= (u32)o) inc += y; }
	if (lane == WAVE - 1) s_w[wave] = inc;
	__syncthreads();
	u32 before = 0, tot = 0;
#pragma unroll
	for (u32 w = 0; w < TE_THREADS / WAVE; ++w) { const u32 v = s_w[w]; before += w < wave ? v : 0u; tot += v; }
	__syncthreads();
	*total = tot;
	return before + inc - x;
}

/* SCATTER = 0: tcnt[tile] = run starts, tcnt[n_tiles + tile] = run ends of the tile.  SCATTER = 1: starts at st[toff[tile] ..], exclusive
 * ends at en[toff[n_tiles + 1 + tile] ..] (toff = the two scans, n_tiles + 1 entries each) */
template <bool SCATTER, typename M>
__global__ __launch_bounds__(TE_THREADS)
void k_te_runs(const uint8_t *__restrict__ flag, int64_t n, int64_t n_tiles, u32 *__restrict__ tcnt, const u64 *__restrict__ toff,
               u64 *__restrict__ st, u64 *__restrict__ en)
{
	const int64_t tile = blockIdx.x;
	const int64_t p0 = tile * TE_TILE + (int64_t)threadIdx.x * TE_PER;
	u32 t[TE_PER];
	if (p0 + TE_PER <= n && ((uintptr_t)(flag + p0) & 15) == 0) {
		const uint4 w = *(const uint4*)(flag + p0);
		const u32 ws[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
		for (int j = 0; j < TE_PER; ++j) t[j] = M::type(ws[j >> 2] >> (8 * (j & 3)) & 0xffu);
	} else {
#pragma unroll
		for (int j = 0; j < TE_PER; ++j) t[j] = p0 + j < n ? M::type(flag[p0 + j]) : 0u;
	}
	u32 prev = p0 > 0 && p0 - 1 < n ? M::type(flag[p0 - 1]) : 0u;
	const u32 after = p0 + TE_PER < n ? M::type(flag[p0 + TE_PER]) : 0u;
	u32 smask = 0, emask = 0;
#pragma unroll
	for (int j = 0; j < TE_PER; ++j) {
		const u32 cur = t[j], nxt = j + 1 < TE_PER ? t[j + 1] : after;
		if (cur && cur != prev) smask |= 1u << j;
		if (cur && cur != nxt) emask |= 1u << j;
		prev = cur;
	}
	u32 s_tot, e_tot;
	const u32 s_before = te_block_scan((u32)__popc(smask), &s_tot);
	const u32 e_before = te_block_scan((u32)__popc(emask), &e_tot);
	if (!SCATTER) {
		if (threadIdx.x == 0) { tcnt[tile] = s_tot; tcnt[n_tiles + tile] = e_tot; }
		return;
	}
	u64 *ps = st + toff[tile] + s_before, *pe = en + toff[n_tiles + 1 + tile] + e_before;
	for (u32 m = smask; m; m &= m - 1) *ps++ = (u64)(p0 + __ffs(m) - 1);
	for (u32 m = emask; m; m &= m - 1) *pe++ = (u64)(p0 + __ffs(m));
}

/* exclusive scan of blockIdx.x's array cnt[blockIdx.x * m ..] into off[blockIdx.x * (m + 1) ..], its sum in the last entry: one block of
 * 1024 threads per array, each thread a contiguous slice (m is a tile or block count, ~2.5e5 for 1 G positions) */
__global__ __launch_bounds__(1024)
void k_te_scan(const u32 *__restrict__ cnt, int64_t m, u64 *__restrict__ off)
{
	__shared__ u64 s_w[1024 / WAVE];
	cnt += blockIdx.x * m;
	off += blockIdx.x * (m + 1);
	const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
	const int64_t per = (m + 1023) / 1024, b = (int64_t)threadIdx.x * per, e = b + per < m ? b + per : m;
	u64 s = 0;
	for (int64_t i = b; i < e; ++i) s += cnt[i];
	u64 inc = s;
#pragma unroll
	for (int o = 1; o < WAVE; o <<= 1) { const u64 y = __shfl_up(inc, o); if (lane >= (u32)o) inc += y; }
	if (lane == WAVE - 1) s_w[wave] = inc;
	__syncthreads();
	u64 run = inc - s, tot = 0;
	for (u32 w = 0; w < 1024 / WAVE; ++w) { const u64 v = s_w[w]; run += w < wave ? v : 0u; tot += v; }
	for (int64_t i = b; i < e; ++i) { off[i] = run; run += cnt[i]; }
	if (threadIdx.x == 0) off[m] = tot;
}

/* TE_ITEMS consecutive runs per thread.  SCATTER = 0: kcnt[block] = runs of the block with e - s >= min_n.  SCATTER = 1: those runs to
 * list[koff[block] ..] in order as {record, s - off[record], e - off[record], type} */
template <bool SCATTER, typename M>
__global__ __launch_bounds__(TE_THREADS)
void k_te_keep(const u64 *__restrict__ st, const u64 *__restrict__ en, const uint8_t *__restrict__ flag, int64_t n_runs, int min_n,
               u32 *__restrict__ kcnt, const u64 *__restrict__ koff, const u64 *__restrict__ seq_off, int64_t n_seq, uint4 *__restrict__ list)
{
	const int64_t r0 = ((int64_t)blockIdx.x * TE_THREADS + threadIdx.x) * TE_ITEMS;
	u32 keep = 0, nk = 0;
#pragma unroll
	for (int j = 0; j < TE_ITEMS; ++j) {
		const int64_t r = r0 + j;
		if (r < n_runs && (int64_t)(en[r] - st[r]) >= (int64_t)min_n) { keep |= 1u << j; ++nk; }
	}
	u32 tot;
	const u32 before = te_block_scan(nk, &tot);
	if (!SCATTER) {
		if (threadIdx.x == 0) kcnt[blockIdx.x] = tot;
		return;
	}
	uint4 *o = list + koff[blockIdx.x] + before;
	for (u32 m = keep; m; m &= m - 1) {
		const int64_t r = r0 + __ffs(m) - 1;
		const u64 s = st[r], e = en[r];
		int64_t lo = 0, hi = n_seq;                   /* the last record with off <= s */
		while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (seq_off[mid] <= s) lo = mid + 1; else hi = mid; }
		const int64_t j = lo > 0 ? lo - 1 : 0;
		const u64 base = seq_off[j];
		*o++ = make_uint4((u32)j, (u32)(s - base), (u32)(e - base), M::type(flag[s]));
	}
}

/* cnt6[6 j ..] += d[0], d[1], c[0..3] of record j (trioeval.c:92-99; zeroed by the caller), from the ordered streak list of *n_list entries */
__global__ __launch_bounds__(TE_THREADS)
void k_te_seq(const uint4 *__restrict__ list, const u64 *__restrict__ n_list, int k, int *__restrict__ cnt6)
{
	const u32 lane = threadIdx.x & (WAVE - 1);
	const int64_t n = (int64_t)*n_list;           /* k_te_scan's total: the grid was sized by the runs, before the kept ones were counted */
	const int64_t i0 = ((int64_t)blockIdx.x * TE_THREADS + threadIdx.x) * TE_ITEMS;
	u32 cur = TE_NONE, pseq = TE_NONE, ptype = 0;
	int a[6] = { 0, 0, 0, 0, 0, 0 };
	if (i0 > 0 && i0 < n) { const uint4 p = list[i0 - 1]; pseq = p.x; ptype = p.w; }
	for (int j = 0; j < TE_ITEMS; ++j) {
		const int64_t i = i0 + j;
		if (i >= n) break;
		const uint4 s = list[i];
		if (s.x != cur) {
			if (cur != TE_NONE)
				for (int q = 0; q < 6; ++q) if (a[q]) atomicAdd(&cnt6[(int64_t)cur * 6 + q], a[q]);
			cur = s.x;
			for (int q = 0; q < 6; ++q) a[q] = 0;
		}
		const int c = (int)s.w - 1, nn = ((int)(s.z - s.y) + k - 1) / k;
		a[c] += nn;                                   /* d[c] */
		a[2 + (c << 1 | c)] += nn - 1;
		if (pseq == s.x) a[2 + (((int)ptype - 1) << 1 | c)] += 1;
		pseq = s.x; ptype = s.w;
	}
	/* the segment open at the end: an inclusive segmented scan over the wave (equal records are adjacent lanes), added by its last lane */
#pragma unroll
	for (int o = 1; o < WAVE; o <<= 1) {
		const u32 os = __shfl_up(cur, o);
		const bool take = lane >= (u32)o && os == cur;
#pragma unroll
		for (int q = 0; q < 6; ++q) { const int y = __shfl_up(a[q], o); a[q] += take ? y : 0; }
	}
	const u32 ns = __shfl_down(cur, 1);
	if (cur != TE_NONE && (lane == WAVE - 1 || ns != cur))
		for (int q = 0; q < 6; ++q) if (a[q]) atomicAdd(&cnt6[(int64_t)cur * 6 + q], a[q]);
}

int64_t yk_te_tiles(int64_t n) { return (n + TE_TILE - 1) / TE_TILE; }
int64_t yk_te_keep_blocks(int64_t n_runs) { return (n_runs + TE_THREADS * TE_ITEMS - 1) / (TE_THREADS * TE_ITEMS); }

/* (macros, not templates: the launch tally names an instantiation as its launch site writes it) */
#define YK_TE_RUNS(M) do { \
		if (scatter) YK_LAUNCH((k_te_runs<true, M>), dim3((unsigned)nt), dim3(TE_THREADS), 0, s, flag, n, nt, tcnt, toff, st, en); \
		else YK_LAUNCH((k_te_runs<false, M>), dim3((unsigned)nt), dim3(TE_THREADS), 0, s, flag, n, nt, tcnt, toff, st, en); \
	} while (0)
void yk_launch_te_runs(const uint8_t *flag, int64_t n, u32 *tcnt, const u64 *toff, u64 *st, u64 *en, int scatter, hipStream_t s, int low)
{
	const int64_t nt = yk_te_tiles(n);
	if (nt <= 0) return;
	if (low) YK_TE_RUNS(TeMapLow);
	else YK_TE_RUNS(TeMapTrio);
}
#undef YK_TE_RUNS

void yk_launch_te_scan(const u32 *cnt, int64_t m, int n_arrays, u64 *off, hipStream_t s)
{
	YK_LAUNCH(k_te_scan, dim3((unsigned)n_arrays), dim3(1024), 0, s, cnt, m, off);
}

#define YK_TE_KEEP(M) do { \
		if (scatter) YK_LAUNCH((k_te_keep<true, M>), dim3((unsigned)nb), dim3(TE_THREADS), 0, s, st, en, flag, n_runs, min_n, kcnt, koff, seq_off, n_seq, (uint4*)list); \
		else YK_LAUNCH((k_te_keep<false, M>), dim3((unsigned)nb), dim3(TE_THREADS), 0, s, st, en, flag, n_runs, min_n, kcnt, koff, seq_off, n_seq, (uint4*)list); \
	} while (0)
void yk_launch_te_keep(const u64 *st, const u64 *en, const uint8_t *flag, int64_t n_runs, int min_n, u32 *kcnt, const u64 *koff,
                       const u64 *seq_off, int64_t n_seq, void *list, int scatter, hipStream_t s, int low)
{
	const int64_t nb = yk_te_keep_blocks(n_runs);
	if (nb <= 0) return;
	if (low) YK_TE_KEEP(TeMapLow);
	else YK_TE_KEEP(TeMapTrio);
}
#undef YK_TE_KEEP

void yk_launch_te_seq(const void *list, const u64 *n_list, int64_t n_max, int k, int *cnt6, hipStream_t s)
{
	const int64_t nb = yk_te_keep_blocks(n_max);
	if (nb <= 0) return;
	YK_LAUNCH(k_te_seq, dim3((unsigned)nb), dim3(TE_THREADS), 0, s, (const uint4*)list, n_list, k, cnt6);
}

/* cnt[4 j ..] += n_k, n_sexchr, n_sex1, n_sex2 of record j (sexchr.c:57-65: flag > 0, == 1, == 2 over the positions where a k-mer ends); a position
 * counts for record j when it lies in [off[j], off[j] + len[j]).  A workgroup folds SC_ITERS consecutive tiles, thread t the TE_PER positions at
 * t * TE_PER of each (a wave reads 1 KiB per step); a thread's record only moves forward.  It ends on the record of its last position plast, which
 * grows with the lane, so equal records are adjacent lanes for the segmented scan.  Same-address atomics were the cost on long contigs (four
 * records: every wave adds to the same four words): folding 16 tiles per workgroup takes them from 47 % of the lookup's time to a few. */
#define SC_ITERS 16
__device__ __forceinline__ int64_t sc_record(const u64 *__restrict__ seq_off, int64_t n_seq, u64 p)
{
	int64_t lo = 0, hi = n_seq;                       /* the last record with off <= p */
	while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (seq_off[mid] <= p) lo = mid + 1; else hi = mid; }
	return lo > 0 ? lo - 1 : 0;
}

__global__ __launch_bounds__(TE_THREADS)
void k_sc_reduce(const uint8_t *__restrict__ flag, int64_t n, const u64 *__restrict__ seq_off, const u32 *__restrict__ seq_len, int64_t n_seq,
                 unsigned long long *__restrict__ cnt)
{
	const u32 lane = threadIdx.x & (WAVE - 1);
	const int64_t b0 = (int64_t)blockIdx.x * SC_ITERS * TE_TILE + (int64_t)threadIdx.x * TE_PER;
	const int64_t last = b0 + (int64_t)(SC_ITERS - 1) * TE_TILE + TE_PER - 1;
	const u64 plast = (u64)(last < n ? last : n - 1);
	u32 a[4] = { 0, 0, 0, 0 };
	int64_t j = sc_record(seq_off, n_seq, (u64)(b0 < n ? b0 : n - 1));
	u64 nxt = j + 1 < n_seq ? seq_off[j + 1] : ~0ull, end = seq_off[j] + seq_len[j];
	for (int it = 0; it < SC_ITERS; ++it) {
		const int64_t p0 = b0 + (int64_t)it * TE_TILE;
		if (p0 >= n) break;
		u32 f[TE_PER];
		if (p0 + TE_PER <= n && ((uintptr_t)(flag + p0) & 15) == 0) {
			const uint4 w = *(const uint4*)(flag + p0);
			const u32 ws[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
			for (int q = 0; q < TE_PER; ++q) f[q] = ws[q >> 2] >> (8 * (q & 3)) & 0xffu;
		} else {
#pragma unroll
			for (int q = 0; q < TE_PER; ++q) f[q] = p0 + q < n ? flag[p0 + q] : TB_NOKMER;
		}
#pragma unroll
		for (int q = 0; q < TE_PER; ++q) {
			const u32 v = f[q];
			if (v == TB_NOKMER) continue;
			const u64 p = (u64)(p0 + q);
			if (p >= nxt) {                           /* a later record: close this one */
#pragma unroll
				for (int c = 0; c < 4; ++c) { if (a[c]) atomicAdd(&cnt[j * 4 + c], (unsigned long long)a[c]); a[c] = 0; }
				j = sc_record(seq_off, n_seq, p);
				nxt = j + 1 < n_seq ? seq_off[j + 1] : ~0ull;
				end = seq_off[j] + seq_len[j];
			}
			if (p >= end) continue;
			a[0] += 1u; a[1] += v > 0u; a[2] += v == 1u; a[3] += v == 2u;
		}
	}
	if (plast >= nxt) {                               /* end on plast's record */
#pragma unroll
		for (int c = 0; c < 4; ++c) { if (a[c]) atomicAdd(&cnt[j * 4 + c], (unsigned long long)a[c]); a[c] = 0; }
		j = sc_record(seq_off, n_seq, plast);
	}
	const u32 cur = (u32)j;
	/* the record open at the end: an inclusive segmented scan over the wave (equal records are adjacent lanes), added by its last lane */
#pragma unroll
	for (int o = 1; o < WAVE; o <<= 1) {
		const u32 os = __shfl_up(cur, o);
		const bool take = lane >= (u32)o && os == cur;
#pragma unroll
		for (int c = 0; c < 4; ++c) { const u32 y = __shfl_up(a[c], o); a[c] += take ? y : 0u; }
	}
	const u32 ns = __shfl_down(cur, 1);
	if (lane == WAVE - 1 || ns != cur)
#pragma unroll
		for (int c = 0; c < 4; ++c) if (a[c]) atomicAdd(&cnt[(u64)cur * 4 + c], (unsigned long long)a[c]);
}

void yk_launch_sc_reduce(const uint8_t *flag, int64_t n, const u64 *seq_off, const u32 *seq_len, int64_t n_seq, u64 *cnt, hipStream_t s)
{
	const int64_t nt = yk_te_tiles(n), nb = (nt + SC_ITERS - 1) / SC_ITERS;
	if (nt <= 0 || n_seq <= 0) return;
	YK_LAUNCH(k_sc_reduce, dim3((unsigned)nb), dim3(TE_THREADS), 0, s, flag, n, seq_off, seq_len, n_seq, (unsigned long long*)cnt);
}
