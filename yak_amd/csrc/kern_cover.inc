/* kern_cover.inc -- part of kernels.hip (one translation unit): `yak-amd cover` (not in the reference; DESIGN.md section 19), one fused streaming
 * pass over the array t that k_lookup<unsigned short> writes for a base image of n positions (yakamd_lookup_dev).
 *
 * hit(j) = t[j] != 0xffff and lo <= min(t[j], 1023) <= hi: the k-mer ENDING at j fulfils the predicate.  cov(i) = 1 where some j in
 * [i, min(i + k - 1, n - 1)] has hit(j): base i lies inside a hitting k-mer.  The definition is over the flat array and knows nothing of records,
 * and on a real image that is correct: a k-mer that ends at j and reaches back to i contains every byte between them, so a separator, an N or any
 * other invalid byte in between makes t[j] = 0xffff.  Hence no cover crosses a record and an invalid byte is never covered -- the same argument that
 * lets kern_trioeval.inc find its runs without a notion of records -- and the pass costs the same per position for one 100 Mb contig and for a
 * million reads.
 *
 * A workgroup folds CV_ITERS consecutive tiles of TE_TILE positions, thread x the TE_PER positions at x * TE_PER of each, as k_sc_reduce does.  Per
 * tile:
 *   bits     every thread turns its 16 elements (two 16-byte loads) into 16 hit bits and stores them as one u16 of a bit string in LDS; four
 *            lanes add the 64 positions behind the tile (the halo: k - 1 <= 30 of them are looked at) and one the position in front of it
 *   cover    after one barrier a thread takes the 64 bits from the position in front of its own on (two LDS words, funnel-shifted) and ORs the
 *            string with itself shifted by 1 .. k - 1 in at most 5 doubling steps: bit b = cov(p0 - 1 + b).  The k positions around a tile
 *            edge are computed by both neighbours; there is no second pass and no atomic on LDS
 *   outputs  cov as one 16-byte store of 0 / 1 bytes, and with MASK the 16 bytes of the image with the covered letters in lower case (1) or the
 *            covered bytes as 'N' (2).  Positions from n up to the next multiple of 16 get 0 and '\n'; nothing behind that is written
 *   tally    n_kmer, n_hit, n_cov and n_run (cov(i) and, i == off[s] or not cov(i - 1)) of the positions inside [off[s], off[s] + len[s]); the
 *            record is found by a binary search over off[] and then only moves forward (cv_forward, cv_step); a record closed inside a thread
 *            is added with atomics; what a lane holds for a record that its next tile lies behind, and what is open at the thread's end, goes
 *            through a segmented scan over the wave (records ascend with the lanes), at the end also over the workgroup's four waves, so
 *            that lanes which hold the same record send one atomic per counter between them
 * The LDS words are double-buffered, so a tile costs one barrier.  Per position 2 bytes are read (3 with MASK) and 1 written (2 with MASK).
 */
#define CV_ITERS 16
#define CV_WORDS (TE_TILE / 64 + 2)            /* [0] bit 63 = hit(tile - 1); [1 .. 64] the tile; [65] the halo */

/* the hit bits of the 16 elements at p (a multiple of 16, below n): two 16-byte loads, inside the allocation's multiple of 16 elements */
__device__ __forceinline__ u32 cv_hits16(const CvArgs &a, int64_t p, u32 *kmer)
{
	const uint4 w0 = *(const uint4*)(a.t + p), w1 = *(const uint4*)(a.t + p + 8);
	const u32 ws[8] = { w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w };
	const int64_t left = a.n - p;
	u32 h = 0, km = 0;
#pragma unroll
	for (int q = 0; q < 16; ++q) {
		const u32 v = ws[q >> 1] >> (16 * (q & 1)) & 0xffffu, c = v < 1023u ? v : 1023u;
		const bool in = q < left && v != 0xffffu;
		km |= (u32)in << q;
		h |= (u32)(in && c >= a.lo && c <= a.hi) << q;
	}
	*kmer = km;
	return h;
}

/* the last record with off <= p, known to lie behind record j (off[j + 1] <= p): a record only moves forward, and mostly not far -- doubling
 * steps from j, then the binary search between the last two */
__device__ __forceinline__ int64_t cv_forward(const u64 *__restrict__ seq_off, int64_t n_seq, int64_t j, u64 p)
{
	int64_t lo = j + 1, step = 1;                     /* off[lo] <= p */
	while (lo + step < n_seq && seq_off[lo + step] <= p) { lo += step; step <<= 1; }
	int64_t hi = lo + step < n_seq ? lo + step : n_seq;   /* off[hi] > p, or hi = n_seq */
	++lo;
	while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (seq_off[mid] <= p) lo = mid + 1; else hi = mid; }
	return lo - 1;
}

/* the same at a tile step, which takes a thread TE_TILE positions on: records of about one length are passed at a steady rate, so the records
 * around `guess` (the step before, repeated) are looked at first -- four loads that do not wait for each other instead of a chain of a dozen.  A
 * record c is the answer iff off[c] <= p < off[c + 1], whatever led to c */
__device__ __forceinline__ int64_t cv_step(const u64 *__restrict__ seq_off, int64_t n_seq, int64_t j, int64_t guess, u64 p)
{
	if (guess > j) {
		u64 o[4];
#pragma unroll
		for (int q = 0; q < 4; ++q) { const int64_t i = guess - 1 + q; o[q] = i < n_seq ? seq_off[i] : ~0ull; }
#pragma unroll
		for (int q = 0; q < 3; ++q) if (o[q] <= p && p < o[q + 1]) return guess - 1 + q;
	}
	return cv_forward(seq_off, n_seq, j, p);
}

/* the lanes with `on` give up what they hold for their record `cur` (records ascend with the lanes, equal ones are adjacent, and within one record
 * the lanes with `on` are its upper ones): an inclusive segmented scan over the wave, one atomic per counter by the last lane of each segment */
__device__ __forceinline__ void cv_flush(u32 *__restrict__ tally, u32 cur, bool on, u32 *acc, u32 lane)
{
	const u32 key = on ? cur : TE_NONE;                   /* no record has this number (check_counts) */
#pragma unroll
	for (int o = 1; o < WAVE; o <<= 1) {
		const u32 os = __shfl_up(key, o);
		const bool take = on && lane >= (u32)o && os == key;
#pragma unroll
		for (int x = 0; x < 4; ++x) { const u32 y = __shfl_up(acc[x], o); acc[x] += take ? y : 0u; }
	}
	const u32 ns = __shfl_down(key, 1);
	if (!on) return;
	if (lane == WAVE - 1 || ns != key)
#pragma unroll
		for (int x = 0; x < 4; ++x) if (acc[x]) atomicAdd(&tally[(u64)cur * 4 + x], acc[x]);
#pragma unroll
	for (int x = 0; x < 4; ++x) acc[x] = 0;
}

template <int MASK>
__global__ __launch_bounds__(TE_THREADS)
void k_cover(CvArgs a)
{
	__shared__ u64 s_w[2][CV_WORDS];
	const u32 lane = threadIdx.x & (WAVE - 1);
	const int64_t n = a.n, n_seq = a.n_seq;
	const int64_t t0 = (int64_t)blockIdx.x * CV_ITERS * TE_TILE, b0 = t0 + (int64_t)threadIdx.x * TE_PER;
	const int64_t last = b0 + (int64_t)(CV_ITERS - 1) * TE_TILE + TE_PER - 1;
	const u64 plast = (u64)(last < n ? last : n - 1);
	u32 acc[4] = { 0, 0, 0, 0 };
	int64_t j = 0;
	u64 beg = 0, end = 0, nxt = ~0ull;
	if (n_seq > 0) {
		j = sc_record(a.seq_off, n_seq, (u64)(b0 < n ? b0 : n - 1));
		beg = a.seq_off[j]; end = beg + a.seq_len[j];
		nxt = j + 1 < n_seq ? a.seq_off[j + 1] : ~0ull;
	}
	int64_t j_it = j, dj = 0;                             /* the record at the last tile step, and how many records that step passed */
	for (int it = 0; it < CV_ITERS; ++it) {
		const int64_t tile = t0 + (int64_t)it * TE_TILE, p0 = tile + (int64_t)threadIdx.x * TE_PER;
		if (tile >= n) break;                             /* the same for the whole workgroup */
		u64 *w = s_w[it & 1];
		u32 kmer = 0;
		const u32 hit = p0 < n ? cv_hits16(a, p0, &kmer) : 0u;
		((unsigned short*)(w + 1))[threadIdx.x] = (unsigned short)hit;
		if (threadIdx.x >= TE_THREADS - 4) {              /* the halo, by four lanes of the last wave */
			const u32 x = threadIdx.x - (TE_THREADS - 4);
			const int64_t p = tile + TE_TILE + (int64_t)x * TE_PER;
			u32 unused;
			((unsigned short*)(w + 1 + TE_TILE / 64))[x] = (unsigned short)(p < n ? cv_hits16(a, p, &unused) : 0u);
		} else if (threadIdx.x == TE_THREADS - 5) {       /* the position in front of the tile */
			u32 v = 0xffffu;
			if (tile > 0) v = a.t[tile - 1];
			const u32 c = v < 1023u ? v : 1023u;
			w[0] = (u64)(v != 0xffffu && c >= a.lo && c <= a.hi) << 63;
		}
		__syncthreads();
		if (p0 < n) {
		/* bit b of c = cov(p0 - 1 + b): the string from absolute bit 64 + 16 x - 1 on; its shift within a word is 63, 15, 31 or 47, never 0 */
		const u32 at = 63u + (u32)threadIdx.x * TE_PER, sh = at & 63u;
		u64 c = w[at >> 6] >> sh | w[(at >> 6) + 1] << (64u - sh);
		for (int span = 1; span < a.k; ) {                /* c = OR of the string shifted by 0 .. span - 1 */
			const int s = span < a.k - span ? span : a.k - span;
			c |= c >> s;
			span += s;
		}
		const u32 c17 = (u32)c & 0x1ffffu, cov = c17 >> 1;
		const int64_t left = n - p0;
		const u32 live = left >= 16 ? 0xffffu : (1u << left) - 1u, cv = cov & live;
		uint4 o;
		u32 ob[4];
#pragma unroll
		for (int q = 0; q < 4; ++q) { const u32 m = cv >> (4 * q); ob[q] = (m & 1u) | (m & 2u) << 7 | (m & 4u) << 14 | (m & 8u) << 21; }
		o.x = ob[0]; o.y = ob[1]; o.z = ob[2]; o.w = ob[3];
		*(uint4*)(a.cov + p0) = o;
		if (MASK) {
			const uint4 bw = *(const uint4*)(a.bases + p0);
			u32 bs[4] = { bw.x, bw.y, bw.z, bw.w };
#pragma unroll
			for (int q = 0; q < 16; ++q) {
				const u32 b = bs[q >> 2] >> (8 * (q & 3)) & 0xffu;
				u32 m = b;
				if (q >= left) m = '\n';
				else if (cv >> q & 1u) m = MASK == 2 ? (u32)'N' : ((b | 0x20u) - 'a' < 26u ? b | 0x20u : b);
				bs[q >> 2] ^= (b ^ m) << (8 * (q & 3));
			}
			*(uint4*)(a.masked + p0) = make_uint4(bs[0], bs[1], bs[2], bs[3]);
		}
		if (n_seq > 0) {
		if ((u64)p0 >= nxt) {                             /* the step from the last tile led to a later record; cv_flush() has emptied acc[] */
			j = cv_step(a.seq_off, n_seq, j, j_it + dj, (u64)p0);
			beg = a.seq_off[j]; end = beg + a.seq_len[j];
			nxt = j + 1 < n_seq ? a.seq_off[j + 1] : ~0ull;
		}
		dj = j - j_it; j_it = j;
		const u32 prev = c17 & 0xffffu;                   /* bit q = cov(p0 + q - 1) */
		if ((u64)p0 > beg && (u64)p0 + TE_PER <= end && (u64)p0 + TE_PER <= nxt) {      /* inside the open record */
			acc[0] += __popc(kmer); acc[1] += __popc(hit); acc[2] += __popc(cv); acc[3] += __popc(cv & ~prev);
		} else {
		const u32 any = (kmer | cv) & live;
#pragma unroll
		for (int q = 0; q < TE_PER; ++q) {
			if (!(any >> q & 1u)) continue;
			const u64 p = (u64)(p0 + q);
			if (p >= nxt) {                               /* a later record: close this one */
#pragma unroll
				for (int x = 0; x < 4; ++x) { if (acc[x]) atomicAdd(&a.tally[j * 4 + x], acc[x]); acc[x] = 0; }
				j = cv_forward(a.seq_off, n_seq, j, p);
				beg = a.seq_off[j]; end = beg + a.seq_len[j];
				nxt = j + 1 < n_seq ? a.seq_off[j + 1] : ~0ull;
			}
			if (p < beg || p >= end) continue;
			acc[0] += kmer >> q & 1u; acc[1] += hit >> q & 1u;
			if (cv >> q & 1u) { acc[2] += 1u; acc[3] += p == beg || !(prev >> q & 1u); }
		}
		}
		}
		}
		/* a lane whose next tile lies behind its open record gives that record up now, together with the lanes beside it that hold the same one */
		if (n_seq > 0 && it + 1 < CV_ITERS) {
			const bool give = p0 + TE_TILE < n && (u64)(p0 + TE_TILE) >= nxt;
			if (__any(give)) cv_flush(a.tally, (u32)j, give, acc, lane);
		}
	}
	if (n_seq <= 0) return;
	if (plast >= nxt) {                                   /* end on plast's record */
#pragma unroll
		for (int x = 0; x < 4; ++x) { if (acc[x]) atomicAdd(&a.tally[j * 4 + x], acc[x]); acc[x] = 0; }
		j = cv_forward(a.seq_off, n_seq, j, plast);
	}
	const u32 cur = (u32)j;
	/* the record open at the end: an inclusive segmented scan over the wave (equal records are adjacent lanes), added by its last lane */
#pragma unroll
	for (int o = 1; o < WAVE; o <<= 1) {
		const u32 os = __shfl_up(cur, o);
		const bool take = lane >= (u32)o && os == cur;
#pragma unroll
		for (int x = 0; x < 4; ++x) { const u32 y = __shfl_up(acc[x], o); acc[x] += take ? y : 0u; }
	}
	const u32 ns = __shfl_down(cur, 1);
	/* a wave's last segment may go on in the next wave: the four of them meet in LDS, so that a record longer than the workgroup's 64 Ki positions
	 * costs one atomic per counter and workgroup -- atomics on one address take about 10 ns each, whoever sends them */
	__shared__ u32 s_end[TE_THREADS / WAVE][5];
	if (lane == WAVE - 1) {
		s_end[threadIdx.x / WAVE][0] = cur;
#pragma unroll
		for (int x = 0; x < 4; ++x) s_end[threadIdx.x / WAVE][1 + x] = acc[x];
	} else if (ns != cur) {
#pragma unroll
		for (int x = 0; x < 4; ++x) if (acc[x]) atomicAdd(&a.tally[(u64)cur * 4 + x], acc[x]);
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		u32 rec = s_end[0][0], sum[4] = { s_end[0][1], s_end[0][2], s_end[0][3], s_end[0][4] };
		for (int w = 1; w < TE_THREADS / WAVE; ++w) {
			if (s_end[w][0] != rec) {
				for (int x = 0; x < 4; ++x) { if (sum[x]) atomicAdd(&a.tally[(u64)rec * 4 + x], sum[x]); sum[x] = 0; }
				rec = s_end[w][0];
			}
			for (int x = 0; x < 4; ++x) sum[x] += s_end[w][1 + x];
		}
		for (int x = 0; x < 4; ++x) if (sum[x]) atomicAdd(&a.tally[(u64)rec * 4 + x], sum[x]);
	}
}

int64_t yk_cover_tile(void) { return TE_TILE; }
int64_t yk_cover_group(void) { return (int64_t)CV_ITERS * TE_TILE; }

void yk_launch_cover(CvArgs a, int mask, hipStream_t st)
{
	const int64_t nt = yk_te_tiles(a.n), nb = (nt + CV_ITERS - 1) / CV_ITERS;
	if (nt <= 0) return;
	if (mask == 0) YK_LAUNCH((k_cover<0>), dim3((unsigned)nb), dim3(TE_THREADS), 0, st, a);
	else if (mask == 1) YK_LAUNCH((k_cover<1>), dim3((unsigned)nb), dim3(TE_THREADS), 0, st, a);
	else YK_LAUNCH((k_cover<2>), dim3((unsigned)nb), dim3(TE_THREADS), 0, st, a);
}
