/* kern_pass2.inc -- part of kernels.hip (one translation unit, included in this order): count-existing passes on records grouped by sub-table (k_img_count_own / _rng), khashl resize to any capacity */
/* ------------------------------------------------------------------------------------------
 * launch wrappers
 * ------------------------------------------------------------------------------------------ */
static inline int grid_for(u64 n, int per_block = 256, int cap = 256 * 8)
{
	u64 g = (n + per_block - 1) / per_block;
	if (g < 1) g = 1;
	if (g > (u64)cap) g = cap;            /* 256 CUs x 8 workgroups, grid-stride beyond that */
	return (int)g;
}

/* ------------------------------------------------------------------------------------------
 * khashl resize to ANY capacity (khashl.h:152-195; yak_ch_tighten htab.c:102-110 shrinks, the
 * pre-resize of yak_ch_merge htab.c:262-266 grows by more than one doubling).  These are one-off
 * maintenance calls, so each sub-table is simply walked by one lane with the literal rule
 * (replay_double is that rule for any old / new size); the workgroup copies and normalises around it.
 * ------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(256)
void k_resize(const ResizeTask *tasks, const u64 *__restrict__ old_keys, const u32 *__restrict__ old_used,
              u64 *new_keys, u32 *new_used, u32 *scr_used)
{
	__shared__ u32 s_progress;
	const ResizeTask T = tasks[blockIdx.x];
	if (T.old_bits == YK_NOCAP) return;
	const u32 n = 1u << T.old_bits, tid = threadIdx.x;
	u64 *keys = new_keys + T.new_off;
	u32 *nu = new_used + (T.new_off >> 5), *cur = scr_used + (T.new_off >> 5);
	for (u32 i = tid; i < n; i += 256) keys[i] = old_keys[T.old_off + i];
	if (T.new_bits == T.old_bits && !T.rehash) {             /* untouched: plain copy */
		for (u32 w = tid; w < (n + 31) / 32; w += 256) nu[w] = old_used[(T.old_off >> 5) + w];
		return;
	}
	const u32 N = 1u << T.new_bits;
	for (u32 w = tid; w < (n + 31) / 32; w += 256) cur[w] = old_used[(T.old_off >> 5) + w];
	for (u32 w = tid; w < (N + 31) / 32; w += 256) nu[w] = 0;
	__syncthreads();
	if (tid == 0) replay_double(keys, cur, nu, n, N, T.new_bits, &s_progress);
	__syncthreads();
	const u32 span = n > N ? n : N;
	for (u32 i = tid; i < span; i += 256) if (i >= N || !bm_get(nu, i)) keys[i] = YK_EMPTY;
}

/* table keys of one sub-table (slot order) -> full hashes + list positions, for a merge pass; cnt != 0: and their 10-bit counts (yakamd_ch_sum) */
__global__ __launch_bounds__(256)
void k_keys_to_hashes(const u64 *__restrict__ kc, const u64 *__restrict__ seg_off, int pre, u64 *__restrict__ hash, u32 *__restrict__ t,
                      unsigned short *__restrict__ cnt)
{
	const u64 a = seg_off[blockIdx.x], b = seg_off[blockIdx.x + 1];
	for (u64 i = a + threadIdx.x; i < b; i += 256) {
		hash[i] = (kc[i] >> 10) << pre | blockIdx.x; t[i] = (u32)i;
		if (cnt) cnt[i] = (unsigned short)(kc[i] & 1023u);
	}
}

/* ==========================================================================================
 * Count-existing passes on sub-tables too large for k_img_count_lds (its bitmap + rank table + one
 * counter per key must fit one workgroup's LDS: ~70 K keys).  The hashes of a sub-table are split
 * once more by the HOME-SLOT RANGE of their key -- khashl.h:98 takes the home slot from the top bits
 * of one 32-bit product, so the top bits of that product name a contiguous range of 2^RNG_LOG slots --
 * and ONE workgroup then owns a range: `used` bits and one 16-bit counter per slot in LDS, the key
 * compare against HBM/L2, plain read-modify-writes at the end.  A probe that runs past the end of
 * the range (linear probing across the boundary) is handed over: appended to `list` and counted by
 * k_img_count_h afterwards; if the list overflows, a second sweep (CROSS = 1) redoes exactly those
 * instances with global reads and atomics.
 * ========================================================================================== */
#define RNG_LOG 16
/* range id, out of 2^rb per sub-table; a sub-table with fewer ranges uses every 2^(rb - rbp)-th id */
__device__ __forceinline__ u32 rng_of(u64 h, const ImgView &img, int rb, int rng_log)
{
	const u32 p = (u32)h & ((1u << img.pre) - 1), bits = img.bits[p];
	if (bits == YK_NOCAP || (int)bits <= rng_log || rb == 0) return 0;
	const int rbp = (int)bits - rng_log;
	return ((u32)(h >> img.pre) * 2654435769u) >> (32 - rbp) << (rb - rbp);
}

template <int MODE>   /* 0 = histogram, 1 = write-combining scatter (groups of 8 hashes) */
__global__ __launch_bounds__(WC_NT)
void k_hpart2(const Chunk2 *chunks, ImgView img, int rb, int rng_log, u32 *rows2, const u64 *__restrict__ sbstart, u64 *__restrict__ out)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	const Chunk2 c = chunks[blockIdx.x];
	const u64 *src = (const u64*)c.rec;
	const int S2 = 1 << rb;
	const u32 tid = threadIdx.x;
	if (MODE == 0) {
		for (int j = tid; j < S2; j += WC_NT) s_dyn[j] = 0;
		__syncthreads();
		for (u32 i = tid; i < c.n; i += WC_NT) atomicAdd(&s_dyn[rng_of(src[i], img, rb, rng_log)], 1u);
		__syncthreads();
		for (int j = tid; j < S2; j += WC_NT) rows2[(size_t)blockIdx.x * S2 + j] = s_dyn[j];
		return;
	}
	WcView w;
	wc_carve<8, XW_CAP_H, false>(w, s_dyn, S2, WC_NT);
	const u32 *row = rows2 + (size_t)blockIdx.x * S2;
	for (int b = tid; b < S2; b += WC_NT) {
		w.cnt[b] = 0; w.head[b] = row[b];
		w.tail[b] = (c.spare & 1) ? (u32)sbstart[(size_t)c.bucket * S2 + b + 1] : row[S2 + b];
	}
	if (tid < 2) w.ntask[tid] = 0;
	__syncthreads();
	const u32 n_round = (c.n + WC_NT - 1) / WC_NT;
	for (u32 rd = 0; rd < n_round; ++rd) {
		const u32 i = rd * WC_NT + tid, par = rd & 1;
		if (i < c.n) { const u64 h = src[i]; wc_place<8, XW_CAP_H, false>(w, rng_of(h, img, rb, rng_log), h, 0, par, out); }
		__syncthreads();
		wc_flush<8, XW_CAP_H, false>(w, par, out);
		__syncthreads();
	}
	wc_drain<8, XW_CAP_H, false>(w, S2, out);
}

template <int CROSS>
__global__ __launch_bounds__(1024)
void k_img_count_rng(const u64 *__restrict__ rec, const u64 *__restrict__ sbstart, ImgView img, int plo, int rb, int rng_log,
                     u64 *__restrict__ list, u32 *list_n, u32 list_cap)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	const u32 bkt = ((u32)plo << rb) + blockIdx.x, p = bkt >> rb, r = bkt & ((1u << rb) - 1), tid = threadIdx.x;
	const u32 bits = img.bits[p];
	const u64 lo = sbstart[bkt], hi = sbstart[bkt + 1];
	if (bits == YK_NOCAP || lo == hi) return;
	const int rbp = (int)bits > rng_log ? (int)bits - rng_log : 0;
	const u32 cap = 1u << bits, nmask = cap - 1, len = cap >> rbp, start = (r >> (rb - rbp)) * len, nw = (len + 31) / 32;
	const u64 off = img.off[p];
	u32 *s_bm = s_dyn, *s_ct = s_dyn + nw;                             /* used bits | one 16-bit counter per slot of the range */
	for (u32 w = tid; w < nw; w += 1024) s_bm[w] = img.used[((off + start) >> 5) + w];
	for (u32 i = tid; i < (len + 1) / 2; i += 1024) s_ct[i] = 0;
	__syncthreads();
	for (u64 i = lo + tid; i < hi; i += 1024) {
		const u64 h = rec[i], kid = h >> img.pre;
		const u32 first = yk_h2b((u32)kid, bits) - start;              /* the partition put the home slot in this range */
		u32 li = first;
		for (;;) {
			if (!(s_bm[li >> 5] >> (li & 31) & 1)) break;                 /* khashl get: stop at the first unused slot */
			if (img.keys[off + start + li] >> 10 == kid) {
				if (!CROSS) {
					const u32 sh = 16 * (li & 1);
					if ((s_ct[li >> 1] >> sh & 0xffffu) < 4096u) atomicAdd(&s_ct[li >> 1], 1u << sh);   /* only min(count, 1023) matters */
				}
				break;
			}
			++li;
			if (rbp == 0) { li &= nmask; if (li == first) break; continue; }   /* the range is the whole table: plain wrap-around */
			if (li < len) continue;
			if (!CROSS) {                                                 /* the probe leaves the range */
				const u32 at = atomicAdd(&list_n[0], 1u);
				if (at < list_cap) list[at] = h; else atomicAdd(&list_n[1], 1u);
			} else {
				const u32 home = (start + first) & nmask;
				for (u32 s2 = (start + len) & nmask; s2 != home; s2 = (s2 + 1) & nmask) {
					const u64 g = off + s2;
					if (!(img.used[g >> 5] >> (g & 31) & 1)) break;
					if (img.keys[g] >> 10 == kid) { atomicAdd(&img.delta[g], 1u); break; }
				}
			}
			break;
		}
	}
	if (CROSS) return;
	__syncthreads();
	for (u32 li = tid; li < len; li += 1024) {
		const u32 c = s_ct[li >> 1] >> (16 * (li & 1)) & 0xffffu;
		if (c) img.delta[off + start + li] += c;                          /* exclusive owner: plain read-modify-write */
	}
}

/* ==========================================================================================
 * Count-existing passes with the KEYS in LDS (the default for records grouped by sub-table).
 * k_img_count_lds keeps bitmap + counters of a whole sub-table in one workgroup's LDS but compares
 * every probe against a key in HBM/L2: 64 bytes fetched per 8-byte compare, the measured traffic was
 * 4x the algorithmic bytes.  Here a sub-table is cut into 2^rbp slot ranges and ONE workgroup owns a
 * range outright: its `used` bits, a per-word rank table, the keys of its used slots packed in rank
 * order and a 16-bit counter per key all sit in LDS, so a probe is LDS work only.  The records are
 * not partitioned again: the 2^rbp workgroups of a sub-table all stream the sub-table's records and
 * keep those whose home slot (top bits of khashl's 32-bit product, khashl.h:98) falls in their range.
 * blockIdx is mapped so that these workgroups run on ONE XCD next to each other in time: the stream
 * comes from HBM once and from that XCD's L2 for the others.  A probe that runs past the end of its
 * range goes to `list` (counted by k_img_count_h afterwards; CROSS = 1 is the second sweep if the list
 * overflowed).  A range with more keys than the LDS budget counts its records with device atomics.
 * ========================================================================================== */
#define OWN_U 8
template <int W, int CROSS>
__global__ __launch_bounds__(1024)
void k_img_count_own(const u64 *__restrict__ rec, const u64 *__restrict__ bstart, ImgView img, int plo, int n_p, int rb, int rng_log, u32 kmax,
                     u64 *__restrict__ list, u32 *list_n, u32 list_cap, int ytag)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	__shared__ u32 s_wsum[16];
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const u32 xcd = blockIdx.x & 7, y = blockIdx.x >> 3, pi = ((y >> rb) << 3) + xcd, r = y & ((1u << rb) - 1);
	if (pi >= (u32)n_p) return;
	const u32 p = (u32)plo + pi, bits = img.bits[p];
	const u64 lo = bstart[p], hi = bstart[p + 1];
	if (bits == YK_NOCAP || lo == hi) return;
	const int rbp = (int)bits > rng_log ? (int)bits - rng_log : 0;     /* log2 ranges of this sub-table */
	if (r >> rbp) return;
	const u32 cap = 1u << bits, nmask = cap - 1, L = cap >> rbp, start = r * L, nw = (L + 31) / 32;
	const u64 off = img.off[p];
	u32 *s_br = s_dyn;                                            /* word w of the bitmap at [2w], the rank of its first slot at [2w + 1]: one 8-byte read per probe */
	u64 *s_k = (u64*)(s_dyn + 2 * ((nw + 1) & ~1u));
	u32 *s_ct = (u32*)(s_k + kmax);
	/* bitmap + exclusive popcount scan (every thread owns a contiguous run of words) */
	const u32 per = (nw + 1023) / 1024;
	u32 mine = 0;
	for (u32 j = 0; j < per; ++j) {
		const u32 w = tid * per + j;
		if (w < nw) { const u32 x = img.used[((off + start) >> 5) + w]; s_br[2 * w] = x; mine += __popc(x); }
	}
	u32 incl = mine;
	for (int o = 1; o < 64; o <<= 1) { const u32 t = __shfl_up(incl, o); if (lane >= (u32)o) incl += t; }
	if (lane == 63) s_wsum[wave] = incl;
	__syncthreads();
	u32 base = incl - mine, total = 0;
	for (u32 w2 = 0; w2 < 16; ++w2) { if (w2 < wave) base += s_wsum[w2]; total += s_wsum[w2]; }
	const bool fits = total <= kmax;
	const u32 rsel = rbp ? 32 - rbp : 0;
	if (!fits) {                                                   /* cannot happen with the host's sizing rule short of a pathological table */
		if (CROSS) return;
		for (u64 i = lo + tid; i < hi; i += 1024) {
			const u64 h = ytag == 2 ? (rec[W * i] >> YK_R8_TAG_BITS) << img.pre | p : ytag ? (rec[W * i] >> img.pre) << img.pre | p : rec[W * i];
			if (rbp && ((u32)(h >> img.pre) * 2654435769u) >> rsel != r) continue;
			const int64_t hit = img_find(img, h);
			if (hit >= 0) atomicAdd(&img.delta[hit], 1u);
		}
		return;
	}
	{
		u32 rr = base;
		for (u32 j = 0; j < per; ++j) {
			const u32 w = tid * per + j;
			if (w >= nw) break;
			s_br[2 * w + 1] = rr;
			u32 x = s_br[2 * w];
			while (x) { const u32 b = __ffs((int)x) - 1; x &= x - 1; s_k[rr++] = img.keys[off + start + w * 32 + b]; }
		}
	}
	for (u32 i = tid; i < (total + 1) / 2; i += 1024) s_ct[i] = 0;
	__syncthreads();
	auto probe = [&](const u64 h) {
		const u64 kid = h >> img.pre;
		const u32 first = (((u32)kid * 2654435769u) >> (32 - bits)) - start;
		u32 s = first;
		u64 wr = *(const u64*)&s_br[2 * (s >> 5)];                   /* a cluster walk stays inside one bitmap word most of the time: one read, then keys only */
		for (;;) {
			const u32 word = (u32)wr;
			if (!(word >> (s & 31) & 1)) break;                          /* khashl get: stop at the first unused slot */
			const u32 rr = (u32)(wr >> 32) + __popc(word & ((1u << (s & 31)) - 1));
			if (s_k[rr] >> 10 == kid) {
				if (!CROSS) {
					const u32 sh = 16 * (rr & 1);
					if ((s_ct[rr >> 1] >> sh & 0xffffu) < 4096u) atomicAdd(&s_ct[rr >> 1], 1u << sh);   /* only min(count, 1023) matters */
				}
				break;
			}
			++s;
			if (rbp == 0) { s &= nmask; if (s == first) break; if ((s & 31) == 0) wr = *(const u64*)&s_br[2 * (s >> 5)]; continue; }   /* the range is the whole table: plain wrap-around */
			if (s < L) { if ((s & 31) == 0) wr = *(const u64*)&s_br[2 * (s >> 5)]; continue; }
			if (!CROSS) {                                                /* the probe leaves the range */
				const u32 at = atomicAdd(&list_n[0], 1u);
				if (at < list_cap) list[at] = ytag ? (h >> img.pre) << img.pre | p : h; else atomicAdd(&list_n[1], 1u);
			} else {
				const u32 home = (start + first) & nmask;
				for (u32 s2 = (start + L) & nmask; s2 != home; s2 = (s2 + 1) & nmask) {
					const u64 g = off + s2;
					if (!(img.used[g >> 5] >> (g & 31) & 1)) break;
					if (img.keys[g] >> 10 == kid) { atomicAdd(&img.delta[g], 1u); break; }
				}
			}
			break;
		}
	};
	/* OWN_U records per lane are requested together (the stream comes from L2 / HBM: one exposed latency per
	 * OWN_U records instead of one per record); the records of this range -- one in 2^rbp -- are packed into
	 * a per-wave LDS queue and probed 64 at a time, so the probe code runs with full waves */
	u64 *s_q = (u64*)(s_ct + ((kmax + 1) / 2 + 1 & ~1u)) + wave * 128;
	u32 qn = 0;
	const u64 STEP = (u64)1024 * OWN_U;
	const u32 ypm = (1u << img.pre) - 1, ysh = (u32)img.pre - (u32)rbp;          /* ytag records: the product's top `pre` bits sit in the low bits */
	auto fetch = [&](u64 (&hv)[OWN_U], const u64 i0) {
#pragma unroll
		for (int u = 0; u < OWN_U; ++u) { const u64 i = i0 + (u64)u * 1024 + tid; hv[u] = rec[W * (i < hi ? i : hi - 1)]; }   /* always a load: the wait counts stay static (consume checks the index) */
	};
	auto consume = [&](const u64 (&hv)[OWN_U], const u64 i0) {
#pragma unroll
		for (int u = 0; u < OWN_U; ++u) {
			const bool valid = i0 + (u64)u * 1024 + tid < hi;
			/* ytag == 2: tagged level-1 records of the pass before (yakamd_count_retained): hash >> pre above the 12 tag bits */
			const u64 hq = ytag == 2 ? (hv[u] >> YK_R8_TAG_BITS) << img.pre : hv[u];
			if (rbp == 0) { if (valid) probe(hq); continue; }
			const bool match = valid && (ytag == 1 ? ((u32)hv[u] & ypm) >> ysh == r : ((u32)(hq >> img.pre) * 2654435769u) >> rsel == r);
			const u64 mk = __ballot(match);
			if (match) s_q[qn + __popcll(mk & lanemask_lt())] = hq;
			qn += (u32)__popcll(mk);
			if (qn >= 64) { qn -= 64; probe(s_q[qn + lane]); }
		}
	};
	/* (a second register set with the next OWN_U records in flight while these are probed was measured: same time, and the eight
	 * range workgroups of a sub-table drift apart in the stream, so HBM fetches rise from 1.2x to 2.2x of the records) */
	u64 ha[OWN_U];
	for (u64 i0 = lo; i0 < hi; i0 += STEP) { fetch(ha, i0); consume(ha, i0); }
	if (lane < qn) probe(s_q[lane]);
	if (CROSS) return;
	__syncthreads();
	for (u32 j = 0; j < per; ++j) {
		const u32 w = tid * per + j;
		if (w >= nw) break;
		u32 x = s_br[2 * w], rr = s_br[2 * w + 1];
		while (x) {
			const u32 b = __ffs((int)x) - 1;
			x &= x - 1;
			const u32 c = s_ct[rr >> 1] >> (16 * (rr & 1)) & 0xffffu;
			if (c) img.delta[off + start + w * 32 + b] += c;             /* exclusive owner: plain read-modify-write */
			++rr;
		}
	}
}

