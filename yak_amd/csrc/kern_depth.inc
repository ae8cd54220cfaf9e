/* kern_depth.inc -- part of kernels.hip (one translation unit, included in this order): the segmented reduction of `yak-amd depth` (DESIGN section 16)
 * over the per-position counts k_lookup<unsigned short> writes.  A window is a slice of that array (dp_slice); its k-mers are the elements that are
 * not DP_NOKMER, a count above 1023 -- the lookup writes none -- is read as 1023.  Per window: n_kmer, n_present (count > 0), sum, the lower median
 * (index (n_kmer - 1) / 2 of the sorted counts) and max, all 0 without a k-mer.
 *   k_dp_short   one wave per window of a batch.  A window of at most T positions is reduced here: its values sit in the lanes' registers (up to
 *                DP_REG per lane) or are read again from L2 per step; counts and the 10 steps of the bitwise radix select of the median are ballots
 *                (registers) or per-lane counts and a wave reduction (re-read) -- no LDS, nothing to clear.  A longer window takes a slot of the
 *                batch's list of long windows and a range of tiles (one 64-bit atomic hands out both, so the tile ranges ascend with the slots).
 *   k_dp_long    one workgroup per tile (DP_RUN positions) of a long window: a 1024-bin histogram in LDS, its non-zero bins added to the window's
 *                global histogram with integer atomics -- the sums do not depend on the order.
 *   k_dp_finish  one wave per long window walks the 1024 bins: 16 per lane, a wave scan of the lanes' totals finds the median's lane.
 * Nothing of the result depends on which slot a window got or on the order of the atomics. */
#define DP_THREADS 256
#define DP_REG 8                           /* values a lane keeps in registers: windows of up to 64 * DP_REG positions */
#define DP_RUN 16384                       /* positions of a long window per workgroup of k_dp_long */
#define DP_NOKMER 0xffffu
#define DP_TILE_BITS 40                    /* the batch counter: long windows << 40 | their tiles */
typedef u32 dp_u32x4 __attribute__((ext_vector_type(4)));

struct DpOut { u32 n_kmer, n_present, median, max; u64 sum; };     /* yakamd_win_t */

/* window g: `first` = index of its first element in cnt, *n = its number of positions.  Sequence j = the last one with win_off[j] <= g (every
 * sequence has at least one window; w = 0: window g is sequence g); window jw = g - win_off[j] covers the k-mer starts [jw w, min(L, (jw + 1) w)),
 * a start s is element s + k - 1, and starts >= L - k + 1 have none.  Clipped to [0, n_bytes): offsets the caller got wrong read nothing outside */
__device__ __forceinline__ u64 dp_slice(const DpArgs &a, u64 g, u32 *n)
{
	const u64 YK_GLOBAL *woff = yk_global(u64, a.win_off);
	u64 j = g, jw = 0;
	if (a.w) {
		u64 l = 0;
		for (u64 r = (u64)a.n_seq; r - l > 1; ) { const u64 m = (l + r) >> 1; if (woff[m] <= g) l = m; else r = m; }
		j = l; jw = g - woff[j];
	}
	*n = 0;
	if (j >= (u64)a.n_seq) return 0;
	const u64 L = yk_global(u32, a.seq_len)[j], off = yk_global(u64, a.seq_off)[j];
	const u64 s0 = a.w ? (jw <= L / a.w ? jw * a.w : L) : 0;
	const u64 s1 = a.w && a.w < L - s0 ? s0 + a.w : L;
	const u64 lo = s0 + (u64)a.k - 1, hi = s1 + (u64)a.k - 1 < L ? s1 + (u64)a.k - 1 : L;
	const u64 first = off + lo;
	if (hi <= lo || first >= (u64)a.n_bytes) return 0;
	const u64 room = (u64)a.n_bytes - first;
	*n = (u32)(hi - lo < room ? hi - lo : room);
	return first;
}

__device__ __forceinline__ u32 dp_wave_sum(u32 v) { for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ u32 dp_wave_max(u32 v) { for (int o = WAVE / 2; o > 0; o >>= 1) { const u32 t = __shfl_xor(v, o); v = t > v ? t : v; } return v; }

__global__ __launch_bounds__(DP_THREADS)
void k_dp_short(DpArgs a, u64 g0, u32 n_win, u32 T, DpOut *__restrict__ out, u32 *__restrict__ long_list, u64 *__restrict__ tile_base, u32 long_cap,
                unsigned long long *counter)
{
	const u32 lane = threadIdx.x & (WAVE - 1);
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
	const unsigned short YK_GLOBAL *cnt = yk_global(unsigned short, a.cnt);
	for (u64 i = (u64)blockIdx.x * (DP_THREADS / WAVE) + wave; i < n_win; i += (u64)gridDim.x * (DP_THREADS / WAVE)) {
		u32 n;
		const u64 first = dp_slice(a, g0 + i, &n);
		if (n > T) {                                              /* a long window: a slot and its tiles */
			if (lane == 0) {
				const u64 tiles = ((u64)n + DP_RUN - 1) / DP_RUN;
				const u64 old = atomicAdd(counter, (unsigned long long)(1ull << DP_TILE_BITS | tiles));
				const u64 slot = old >> DP_TILE_BITS;
				if (slot < long_cap) { long_list[slot] = (u32)i; tile_base[slot] = old & ((1ull << DP_TILE_BITS) - 1); }
			}
			continue;
		}
		u32 nk = 0, np = 0, sum = 0, mx = 0, med = 0;
		if (n <= WAVE * DP_REG) {                                 /* the values in registers, the counts as ballots */
			u32 v[DP_REG];
#pragma unroll
			for (int r = 0; r < DP_REG; ++r) {
				const u32 p = (u32)r * WAVE + lane;
				const u32 x = p < n ? cnt[first + p] : DP_NOKMER;
				v[r] = x == DP_NOKMER || x < 1024u ? x : 1023u;
			}
			u32 alive = 0;                                         /* bit r: v[r] is a k-mer that still matches the median's upper bits */
#pragma unroll
			for (int r = 0; r < DP_REG; ++r) {
				if ((u32)r * WAVE >= n) break;
				const bool ok = v[r] != DP_NOKMER;
				nk += (u32)__popcll(__ballot(ok));
				np += (u32)__popcll(__ballot(ok && v[r] > 0));
				if (ok) { alive |= 1u << r; sum += v[r]; mx = v[r] > mx ? v[r] : mx; }
			}
			sum = dp_wave_sum(sum); mx = dp_wave_max(mx);
			u32 rank = nk ? (nk - 1) / 2 : 0;
			for (int bit = 9; nk && bit >= 0; --bit) {
				u32 c0 = 0;
#pragma unroll
				for (int r = 0; r < DP_REG; ++r) {
					if ((u32)r * WAVE >= n) break;
					c0 += (u32)__popcll(__ballot((alive >> r & 1) && !(v[r] >> bit & 1)));
				}
				const u32 one = rank >= c0;
				if (one) { rank -= c0; med |= 1u << bit; }
#pragma unroll
				for (int r = 0; r < DP_REG; ++r) if ((v[r] >> bit & 1) != one) alive &= ~(1u << r);
			}
		} else {                                                  /* read again per step: T positions are a few KB, in L2 after the first pass */
			for (u32 p = lane; p < n; p += WAVE) {
				u32 x = cnt[first + p];
				if (x == DP_NOKMER) continue;
				x = x < 1024u ? x : 1023u;
				++nk; np += x > 0; sum += x; mx = x > mx ? x : mx;
			}
			nk = dp_wave_sum(nk); np = dp_wave_sum(np); sum = dp_wave_sum(sum); mx = dp_wave_max(mx);
			u32 rank = nk ? (nk - 1) / 2 : 0;
			for (int bit = 9; nk && bit >= 0; --bit) {
				u32 c0 = 0;
				for (u32 p = lane; p < n; p += WAVE) {
					u32 x = cnt[first + p];
					if (x == DP_NOKMER) continue;
					x = x < 1024u ? x : 1023u;
					c0 += (x >> (bit + 1)) == (med >> (bit + 1)) && !(x >> bit & 1);
				}
				c0 = dp_wave_sum(c0);
				if (rank >= c0) { rank -= c0; med |= 1u << bit; }
			}
		}
		if (lane == 0) { DpOut o; o.n_kmer = nk; o.n_present = np; o.median = med; o.max = mx; o.sum = sum; out[i] = o; }
	}
}

/* tile blockIdx.x + tile0 of the batch belongs to the last slot of [slot0, slot0 + n_slots) whose tile_base is not above it (a window without a
 * position has no tile and shares its base with the slot behind it); the window's histogram is hist + 1024 (slot - slot0).  cnt is 16-byte aligned:
 * a lane reads eight elements at once from the aligned 16 bytes around them and drops those outside its tile */
__global__ __launch_bounds__(DP_THREADS)
void k_dp_long(DpArgs a, u64 g0, const u32 *__restrict__ long_list, const u64 *__restrict__ tile_base, u32 slot0, u32 n_slots, u64 tile0,
               unsigned long long *__restrict__ hist)
{
	__shared__ u32 s_hist[1024];
	for (u32 i = threadIdx.x; i < 1024; i += DP_THREADS) s_hist[i] = 0;
	__syncthreads();
	const u64 YK_GLOBAL *tb = yk_global(u64, tile_base);
	const u64 tile = tile0 + blockIdx.x;
	u32 l = slot0;
	for (u32 r = slot0 + n_slots; r - l > 1; ) { const u32 m = l + (r - l) / 2; if (tb[m] <= tile) l = m; else r = m; }
	u32 n;
	const u64 first = dp_slice(a, g0 + yk_global(u32, long_list)[l], &n);
	const u64 p0 = (tile - tb[l]) * DP_RUN;
	if (p0 < n) {
		const u64 lo = first + p0, hi = first + (p0 + DP_RUN < n ? p0 + DP_RUN : n);
		const dp_u32x4 YK_GLOBAL *v4 = (const dp_u32x4 YK_GLOBAL*)a.cnt;
		for (u64 e = (lo & ~7ull) + 8ull * threadIdx.x; e < hi; e += 8ull * DP_THREADS) {
			const dp_u32x4 q = v4[e >> 3];
#pragma unroll
			for (int u = 0; u < 8; ++u) {
				const u32 x = (u & 1 ? q[u >> 1] >> 16 : q[u >> 1]) & 0xffffu;
				if (e + u >= lo && e + u < hi && x != DP_NOKMER) atomicAdd(&s_hist[x < 1024u ? x : 1023u], 1u);
			}
		}
	}
	__syncthreads();
	unsigned long long *h = hist + (u64)(l - slot0) * 1024;
	for (u32 i = threadIdx.x; i < 1024; i += DP_THREADS) if (s_hist[i]) atomicAdd(&h[i], (unsigned long long)s_hist[i]);
}

__global__ __launch_bounds__(DP_THREADS)
void k_dp_finish(const unsigned long long *__restrict__ hist, const u32 *__restrict__ long_list, u32 slot0, u32 n_slots, DpOut *__restrict__ out)
{
	const u32 lane = threadIdx.x & (WAVE - 1);
	const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
	for (u32 s = blockIdx.x * (DP_THREADS / WAVE) + wave; s < n_slots; s += gridDim.x * (DP_THREADS / WAVE)) {
		const u64 YK_GLOBAL *h = yk_global(u64, hist) + (u64)s * 1024 + lane * 16;
		u64 c[16], tot = 0, sum = 0;
		u32 mx = 0;
#pragma unroll
		for (int b = 0; b < 16; ++b) { c[b] = h[b]; tot += c[b]; sum += c[b] * (u64)(lane * 16 + b); if (c[b]) mx = lane * 16 + b; }
		u64 incl = tot;                                            /* bins up to this lane's last */
		for (int o = 1; o < WAVE; o <<= 1) { const u64 t = __shfl_up(incl, o); if ((int)lane >= o) incl += t; }
		const u64 nk = __shfl(incl, WAVE - 1), zero = __shfl(c[0], 0);
		for (int o = WAVE / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
		mx = dp_wave_max(mx);
		const u64 rank = nk ? (nk - 1) / 2 : 0;
		u32 med = 0;
		if (nk && incl - tot <= rank && rank < incl) {             /* one lane */
			u64 at = incl - tot;
#pragma unroll
			for (int b = 0; b < 16; ++b) { if (at <= rank && rank < at + c[b]) med = lane * 16 + b; at += c[b]; }
		}
		med = dp_wave_max(med);
		if (lane == 0) { DpOut o; o.n_kmer = (u32)nk; o.n_present = (u32)(nk - zero); o.median = med; o.max = mx; o.sum = sum; out[long_list[slot0 + s]] = o; }
	}
}
