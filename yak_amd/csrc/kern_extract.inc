/* kern_extract.inc -- part of kernels.hip (one translation unit, included in this order): extraction (K1), level-1 radix partition with software write combining, table image probing, the lookup-only path of yak qv */
/* ------------------------------------------------------------------------------------------
 * K1: extraction.  One workgroup = one tile of XT_TILE stream positions.
 *   phase 1: 16 B/lane coalesced loads, nt4 translation, 2-bit packing into LDS (+32-base halo)
 *   phase 2: lane <-> position; the k-mer ending at the position is a 2k-bit window of the packed
 *            stream; reverse strand = complement of the window, forward = 2-bit-group reversal;
 *            canonical = min; yak_hash64.  A window is emitted iff its k validity bits are all set,
 *            which is exactly the `l` run counter of count.c:33-42.
 *   phase 3: wave ballot + prefix compaction, one global cursor bump per workgroup, coalesced
 *            stores of (hash, position).
 * ------------------------------------------------------------------------------------------ */
#define XT_TILE    4096
#define XT_THREADS 256
#define XT_ROUNDS  (XT_TILE / XT_THREADS)
#define XT_HALO    64          /* left context: k - 1 <= 62 bases */

struct XtTile {
	u32 code[(XT_TILE + XT_HALO) / 16 + 4];      /* 2 bits per base, 16 bases per word, base j of the stream at bits 2(j%16) */
	u32 valid[(XT_TILE + XT_HALO) / 32 + 4];     /* 1 bit per base: ACGT or not */
	unsigned char lut[256];
};

__device__ __forceinline__ void xt_init(XtTile &S)
{
	const int tid = threadIdx.x;
	if (tid < 64) ((u32*)S.lut)[tid] = ((const u32*)d_nt4)[tid];
	if (tid < 4) { S.code[(XT_TILE + XT_HALO) / 16 + tid] = 0; S.valid[(XT_TILE + XT_HALO) / 32 + tid] = 0; }
	__syncthreads();
}

/* phase 1: translate + pack the tile [tile0 - HALO, tile0 + XT_TILE) into LDS; ends with a barrier */
/* `valid` != 0: the stream comes packed (yakamd_feed_packed_dev) -- `bases` is then the array of 2-bit codes, 16 bases per 32-bit
 * word in the tile's own layout, `valid` one bit per base; tiles start at multiples of 16 positions, so a word is a word */
__device__ __forceinline__ void xt_load(XtTile &S, const uint8_t *__restrict__ bases, int64_t tile0, int64_t n, const u32 *__restrict__ valid = 0)
{
	const int64_t origin = tile0 - XT_HALO;
	for (int w = threadIdx.x; w < (XT_TILE + XT_HALO) / 16; w += blockDim.x) {
		const int64_t pos = origin + 16 * (int64_t)w;
		u32 code = 0, val = 0;
		if (valid) {
			if (pos >= 0 && pos < n) {
				code = ((const u32*)bases)[pos >> 4];
				val = (valid[pos >> 5] >> (pos & 16)) & 0xffffu;
				if (pos + 16 > n) val &= (1u << (n - pos)) - 1;
				u32 m = 0;                                                    /* invalid positions carry code 0, as the ASCII path leaves them */
				for (int j = 0; j < 16; ++j) m |= (val >> j & 1u) * (3u << (2 * j));
				code &= m;
			}
		} else if (pos >= 0 && pos + 16 <= n) {
			const uint4 v = *(const uint4*)(bases + pos);
			const u32 q[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
			for (int j = 0; j < 16; ++j) {
				const u32 c = S.lut[(q[j >> 2] >> (8 * (j & 3))) & 0xff];
				if (c < 4) { code |= c << (2 * j); val |= 1u << j; }
			}
		} else {
			for (int j = 0; j < 16; ++j) {
				const int64_t x = pos + j;
				if (x >= 0 && x < n) {
					const u32 c = S.lut[bases[x]];
					if (c < 4) { code |= c << (2 * j); val |= 1u << j; }
				}
			}
		}
		S.code[w] = code;
		((unsigned short*)S.valid)[w] = (unsigned short)val;
	}
	__syncthreads();
}

/* xt_load in two halves for the ASCII stream, so that a workgroup that walks several tiles has the next tile's 16 bytes per lane in flight while it
 * works on the current one (the tile in LDS is single: the load is the only part that can overlap).  xt_fetch issues the loads of the lanes whose
 * 16 bases lie wholly inside the stream; xt_put translates what arrived (or, at the stream's ends, reads byte by byte) and ends with a barrier */
template <int NT> struct XtRaw { uint4 v[((XT_TILE + XT_HALO) / 16 + NT - 1) / NT]; };

template <int NT>
__device__ __forceinline__ void xt_fetch(XtRaw<NT> &R, const uint8_t *__restrict__ bases, int64_t tile0, int64_t n)   /* n >= 16 */
{
	const int64_t origin = tile0 - XT_HALO, top = (n - 16) & ~(int64_t)15;
#pragma unroll
	for (int i = 0; i < (int)(sizeof(R.v) / sizeof(R.v[0])); ++i) {
		/* no branch around the load (a value merged from two paths is copied, and the copy waits for the load): every lane loads, from a clamped
		 * address; what a lane outside the stream or the tile gets is never looked at */
		int64_t pos = origin + 16 * (int64_t)((int)threadIdx.x + i * NT);
		pos = pos < 0 ? 0 : pos > top ? top : pos;
		R.v[i] = *(const uint4*)(bases + pos);
	}
}

template <int NT>
__device__ __forceinline__ void xt_put(XtTile &S, const XtRaw<NT> &R, const uint8_t *__restrict__ bases, int64_t tile0, int64_t n)
{
	const int64_t origin = tile0 - XT_HALO;
#pragma unroll
	for (int i = 0; i < (int)(sizeof(R.v) / sizeof(R.v[0])); ++i) {
		const int w = (int)threadIdx.x + i * NT;
		if (w >= (XT_TILE + XT_HALO) / 16) break;
		const int64_t pos = origin + 16 * (int64_t)w;
		u32 code = 0, val = 0;
		if (pos >= 0 && pos + 16 <= n) {
			const u32 q[4] = { R.v[i].x, R.v[i].y, R.v[i].z, R.v[i].w };
#pragma unroll
			for (int j = 0; j < 16; ++j) {
				const u32 c = S.lut[(q[j >> 2] >> (8 * (j & 3))) & 0xff];
				if (c < 4) { code |= c << (2 * j); val |= 1u << j; }
			}
		} else {
#pragma unroll 1                                                      /* the stream's two ends only: kept rolled, or its sixteen addresses are hoisted out of the tile loop into registers */
			for (int j = 0; j < 16; ++j) {
				const int64_t x = pos + j;
				if (x >= 0 && x < n) {
					const u32 c = S.lut[bases[x]];
					if (c < 4) { code |= c << (2 * j); val |= 1u << j; }
				}
			}
		}
		S.code[w] = code;
		((unsigned short*)S.valid)[w] = (unsigned short)val;
	}
	__syncthreads();
}

__device__ __forceinline__ u64 yk_hash64_64(u64 x)                   /* reference yak-priv.h:23-33 */
{
	x = ~x + (x << 21);
	x ^= x >> 24;
	x = x + (x << 3) + (x << 8);
	x ^= x >> 14;
	x = x + (x << 2) + (x << 4);
	x ^= x >> 28;
	x = x + (x << 31);
	return x;
}

/* even bits of a 64-bit word packed into the low 32 bits */
__device__ __forceinline__ u64 yk_even_bits(u64 x)
{
	x &= 0x5555555555555555ull;
	x = (x | x >> 1) & 0x3333333333333333ull;
	x = (x | x >> 2) & 0x0f0f0f0f0f0f0f0full;
	x = (x | x >> 4) & 0x00ff00ff00ff00ffull;
	x = (x | x >> 8) & 0x0000ffff0000ffffull;
	return (x | x >> 16) & 0xffffffffull;
}

__device__ u32 d_bad_hash;       /* k >= 32 only: a 64-bit hash equal to a table sentinel was met */

/* k in [32, 63] (reference count.c:45-60 + yak-priv.h:35-39): the four k-bit planes are the low / high
 * bits of the forward strand (first base most significant) and the complemented low / high bits of
 * the reverse strand; the strand is chosen on the high planes, the hash is the sum of two 64-bit mixes */
__device__ __forceinline__ bool xt_kmer_long(const XtTile &S, int q, int k, int pre, int64_t tile0, int64_t n, u64 *h)
{
	const int e = XT_HALO + q;                 /* q = position inside the tile of the k-mer's last base */
	const int s = e - k + 1;
	const int v0 = s >> 5, vo = s & 31;
	const u64 va = (u64)S.valid[v0] | (u64)S.valid[v0 + 1] << 32, vb = S.valid[v0 + 2];
	u64 V = va >> vo;
	if (vo) V |= vb << (64 - vo);
	const u64 kones = (1ull << k) - 1;
	const int w0 = s >> 4, o = 2 * (s & 15);
	const u64 a = (u64)S.code[w0] | (u64)S.code[w0 + 1] << 32, b = (u64)S.code[w0 + 2] | (u64)S.code[w0 + 3] << 32;
	u64 lo = a >> o, hi = b >> o;
	if (o) { lo |= b << (64 - o); hi |= (u64)S.code[w0 + 4] << (64 - o); }
	const u64 L = (yk_even_bits(lo) | yk_even_bits(hi) << 32) & kones;
	const u64 H = (yk_even_bits(lo >> 1) | yk_even_bits(hi >> 1) << 32) & kones;
	const u64 x0 = __brevll(L) >> (64 - k), x1 = __brevll(H) >> (64 - k), x2 = ~L & kones, x3 = ~H & kones;
	const u64 hv = x1 < x3 ? yk_hash64_64(x0) + yk_hash64_64(x1) : yk_hash64_64(x2) + yk_hash64_64(x3);
	*h = hv;
	const bool ok = (V & kones) == kones && tile0 + q < n;
	if (ok && (hv >> pre) == (~0ull >> pre)) d_bad_hash = 1;       /* would collide with the EMPTY slot pattern */
	return ok;
}

/* phase 2: hashed canonical k-mer ending at tile position q; false if the window holds a non-ACGT
 * byte or lies beyond n */
/* KC != 0: k is that constant (31, yak's default: the masks and the last shift fold into the instructions); the windows are 96-bit funnel shifts
 * of three code words (v_alignbit_b32), the 2-bit-group reversal works on the two halves */
template <int KC = 0>
__device__ __forceinline__ bool xt_kmer(const XtTile &S, int q, int k_, u64 mask_, u64 kones_, int64_t tile0, int64_t n, u64 *h)
{
	const int k = KC ? KC : k_;
	const u64 mask = KC ? (1ull << (2 * (KC & 31))) - 1 : mask_;
	const u32 kones = KC ? (u32)((1ull << (KC & 31)) - 1) : (u32)kones_;
	const int e = XT_HALO + q;                                      /* LDS base index of the k-mer's last base */
	const int s = e - k + 1;
	const u32 V = __builtin_amdgcn_alignbit(S.valid[(s >> 5) + 1], S.valid[s >> 5], (u32)s & 31);   /* k <= 31 validity bits */
	const int w0 = s >> 4;
	const u32 o = 2 * ((u32)s & 15);
	const u32 c0 = S.code[w0], c1 = S.code[w0 + 1], c2 = S.code[w0 + 2];
	const u64 W = ((u64)__builtin_amdgcn_alignbit(c2, c1, o) << 32 | __builtin_amdgcn_alignbit(c1, c0, o)) & mask;
	const u64 rv = ~W & mask;                          /* count.c:37: base j of the window at bits 2j, complemented */
	u32 rl = __brev((u32)(W >> 32)), rh = __brev((u32)W);             /* count.c:36: first base most significant */
	rl = ((rl >> 1) & 0x55555555u) | ((rl & 0x55555555u) << 1);
	rh = ((rh >> 1) & 0x55555555u) | ((rh & 0x55555555u) << 1);
	const u64 fw = ((u64)rh << 32 | rl) >> (64 - 2 * k);
	*h = yk_hash64(fw < rv ? fw : rv, mask);
	return (V & kones) == kones && tile0 + q < n;
}

/* compacting extraction (no partition): used for the explicit extract entry point */
__global__ __launch_bounds__(XT_THREADS)
void k_extract(const uint8_t *__restrict__ bases, int64_t pos0, int64_t n, int64_t t_sub, int k, int pre, int plo, int phi,
               u64 *__restrict__ out_hash, u32 *__restrict__ out_t, u64 *cursor)
{
	__shared__ XtTile S;
	__shared__ u32 s_cnt[XT_ROUNDS * 4];
	__shared__ u64 s_base;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int64_t tile0 = pos0 + (int64_t)blockIdx.x * XT_TILE;   /* pos0 is a multiple of 16 */
	xt_init(S);
	xt_load(S, bases, tile0, n);
	const u64 mask = k < 32 ? (1ull << (2 * k)) - 1 : ~0ull, kones = (1ull << k) - 1;
	const u32 pmask = (1u << pre) - 1;
	u64 hv[XT_ROUNDS];
	u32 okm = 0;
#pragma unroll
	for (int r = 0; r < XT_ROUNDS; ++r) {
		u64 h;
		const int q = r * XT_THREADS + (int)threadIdx.x;
			bool ok = k < 32 ? xt_kmer(S, q, k, mask, kones, tile0, n, &h) : xt_kmer_long(S, q, k, pre, tile0, n, &h);
		const u32 p = (u32)h & pmask;
		ok = ok && (int)p >= plo && (int)p < phi;
		hv[r] = h;
		okm |= (u32)ok << r;
		const u64 b = __ballot(ok);
		if (lane == 0) s_cnt[r * 4 + wave] = __popcll(b);
	}
	__syncthreads();
	if (tid == 0) {
		u32 acc = 0;
		for (int i = 0; i < XT_ROUNDS * 4; ++i) { const u32 c = s_cnt[i]; s_cnt[i] = acc; acc += c; }
		s_base = acc ? atomicAdd(cursor, (u64)acc) : 0;
	}
	__syncthreads();
	const u64 base = s_base;
#pragma unroll
	for (int r = 0; r < XT_ROUNDS; ++r) {
		const bool ok = okm >> r & 1;
		const u64 b = __ballot(ok);
		if (ok) {
			const u64 d = base + s_cnt[r * 4 + wave] + __popcll(b & lanemask_lt());
			out_hash[d] = hv[r];
			out_t[d] = (u32)(tile0 + r * XT_THREADS + tid - t_sub);
		}
	}
}

/* ------------------------------------------------------------------------------------------
 * K1 with radix partition: the hashed k-mers of a batch are grouped by the top `nb_bits` of their
 * sub-table prefix, so that every later pass walks the accumulator / bloom / table image one
 * contiguous region at a time (the regions being worked on at any moment stay cache resident).
 * Two sweeps over the bases, no global atomics:
 *   hist   : one workgroup = XP_T tiles; bucket counts in an LDS histogram -> one row of `rows`
 *   scan   : rows -> exclusive offsets (per bucket across workgroups) + bucket starts
 *   scatter: same workgroups recompute their k-mers and place them with LDS cursors
 * The same two kernels partition already-hashed records (SRC = 1: exchanged k-mers of the
 * multi-GPU path, yak_ch_insert_list).
 * ------------------------------------------------------------------------------------------ */
#define XP_T 16                                   /* tiles per workgroup: 65536 stream positions */

__device__ __forceinline__ u32 bucket_of(u64 h, int pre, int nb_bits)
{
	const u32 p = (u32)h & ((1u << pre) - 1);
	return nb_bits <= pre ? p >> (pre - nb_bits) : p;   /* nb_bits is clamped to pre by the host */
}

template <int MODE, int KC = 0>   /* KC: xt_kmer's constant k.  MODE 0 = histogram, 1 = scatter {hash, position}, 2 = scatter hash only (count-existing passes), 3 = histogram that also counts, per bucket, the 1024-position rounds that contribute to it (count | rounds << 24) */
__global__ __launch_bounds__(XT_THREADS)
void k_xpart(const uint8_t *__restrict__ bases, int64_t pos0, int64_t n, int64_t t_sub, int k, int pre, int plo, int phi,
             int nb_bits, u32 *rows, Rec *__restrict__ out, const u32 *__restrict__ valid)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_bkt[];
	__shared__ XtTile S;
	const int NB = 1 << nb_bits;
	u32 *row = rows + (size_t)blockIdx.x * NB;
	u32 *s_lastr = s_bkt + NB, *s_nr = s_bkt + 2 * NB;                /* MODE 3 only */
	if (MODE == 3) for (int j = threadIdx.x; j < NB; j += XT_THREADS) { s_lastr[j] = 0; s_nr[j] = 0; }
	for (int j = threadIdx.x; j < NB; j += XT_THREADS) s_bkt[j] = (MODE == 1 || MODE == 2) ? row[j] : 0;
	xt_init(S);
	const u64 mask = k < 32 ? (1ull << (2 * k)) - 1 : ~0ull, kones = (1ull << k) - 1;
	const u32 pmask = (1u << pre) - 1;
	auto rounds = [&](const int64_t tile0, const int t) {
#pragma unroll 4
		for (int r = 0; r < XT_ROUNDS; ++r) {
			u64 h;
			const int q = r * XT_THREADS + (int)threadIdx.x;
			bool ok = KC ? xt_kmer<KC>(S, q, k, mask, kones, tile0, n, &h) : k < 32 ? xt_kmer(S, q, k, mask, kones, tile0, n, &h) : xt_kmer_long(S, q, k, pre, tile0, n, &h);
			const u32 p = (u32)h & pmask;
			ok = ok && (int)p >= plo && (int)p < phi;
			if (ok) {
				const u32 bk = bucket_of(h, pre, nb_bits);
				const u32 d = atomicAdd(&s_bkt[bk], 1u);
				if (MODE == 1) out[d] = make_ulonglong2(h, (u64)(u32)(tile0 + r * XT_THREADS + threadIdx.x - t_sub));
				if (MODE == 2) ((u64*)out)[d] = h;
				if (MODE == 3) {                                        /* waves drift apart inside a tile: a bit per round, counted at the end */
					const u32 R = (u32)t * (XT_TILE / 1024) + (u32)r * XT_THREADS / 1024;
					static_assert(XP_T * (XT_TILE / 1024) <= 64, "one bit per round in two words");
					atomicOr(R < 32 ? &s_lastr[bk] : &s_nr[bk], 1u << (R & 31));
				}
			}
		}
		__syncthreads();
	};
	const int64_t first = pos0 + (int64_t)blockIdx.x * XP_T * XT_TILE;
	if (valid || n < 16) {
		for (int t = 0; t < XP_T && first + (int64_t)t * XT_TILE < n; ++t) {
			xt_load(S, bases, first + (int64_t)t * XT_TILE, n, valid);
			rounds(first + (int64_t)t * XT_TILE, t);
		}
	} else {
		XtRaw<XT_THREADS> raw;
		xt_fetch<XT_THREADS>(raw, bases, first, n);
		for (int t = 0; t < XP_T && first + (int64_t)t * XT_TILE < n; ++t) {
			const int64_t tile0 = first + (int64_t)t * XT_TILE;
			xt_put<XT_THREADS>(S, raw, bases, tile0, n);
			xt_fetch<XT_THREADS>(raw, bases, tile0 + XT_TILE, n);         /* the next tile, in flight during this one's rounds */
			rounds(tile0, t);
		}
	}
	if (MODE == 0) { __syncthreads(); for (int j = threadIdx.x; j < NB; j += XT_THREADS) row[j] = s_bkt[j]; }
	if (MODE == 3) { __syncthreads(); for (int j = threadIdx.x; j < NB; j += XT_THREADS) row[j] = s_bkt[j] | (u32)(__popc(s_lastr[j]) + __popc(s_nr[j])) << 24; }
}

/* ------------------------------------------------------------------------------------------
 * Software write combining for the partition scatters.  A lone 8- or 16-byte store to a random
 * address costs a whole memory transaction (stores are not merged behind the CU: ~21 G records/s
 * measured on gfx950, whatever the record size), while GS neighbouring lanes storing one aligned
 * 64-byte group run at 110-220 G records/s.  So each bucket gets a CAP-record stack in LDS; a round
 * places one record per thread, and every stack that then holds enough to reach the next 64-byte
 * boundary of its output run is flushed as one aligned group by GS lanes.  The order of records
 * inside a bucket is free (later stages order by stream position themselves), so a stack is all
 * the bookkeeping needed.  A record that finds its stack full (a burst of one bucket inside a
 * round) is stored alone, taken from the END of the workgroup's run of that bucket, so the groups
 * stay aligned.  HAS_T: {hash, position} records of 16 bytes (GS = 4), else bare hashes (GS = 8).
 * ------------------------------------------------------------------------------------------ */
struct WcView { u64 *h; u32 *t, *cnt, *head, *tail, *task, *ntask; };

template <int GS, int CAP, bool HAS_T>
__device__ __forceinline__ size_t wc_carve(WcView &w, u32 *lds, int NB, int NT)
{
	w.h = (u64*)lds;
	u32 *p = lds + 2 * (size_t)NB * CAP;
	w.t = p; if (HAS_T) p += (size_t)NB * CAP;
	w.cnt = p; w.head = p + NB; w.tail = p + 2 * NB; w.task = p + 3 * NB; w.ntask = w.task + NT;
	return 0;
}
template <int GS, int CAP, bool HAS_T> __host__ __device__ constexpr size_t wc_lds_bytes(int NB, int NT)
{
	return (size_t)NB * CAP * (HAS_T ? 12 : 8) + (size_t)NB * 12 + (size_t)NT * 4 + 16;
}

template <bool HAS_T> __device__ __forceinline__ void wc_store(void *out, u32 d, u64 h, u32 t)
{
	if (HAS_T) ((Rec*)out)[d] = make_ulonglong2(h, (u64)t); else ((u64*)out)[d] = h;
}

template <int GS, int CAP, bool HAS_T>
__device__ __forceinline__ void wc_place(const WcView &w, u32 b, u64 h, u32 t, u32 par, void *out)
{
	const u32 pos = atomicAdd(&w.cnt[b], 1u);
	if (pos < (u32)CAP) { yk_lds_rw(u64, w.h)[b * CAP + pos] = h; if (HAS_T) yk_lds_rw(u32, w.t)[b * CAP + pos] = t; }
	else wc_store<HAS_T>(out, atomicSub(&w.tail[b], 1u) - 1, h, t);
	if (pos == (u32)(GS - 1) - (w.head[b] & (GS - 1))) w.task[atomicAdd(&w.ntask[par], 1u)] = b;   /* this record completes a group */
}

/* between two barriers: flush every stack listed this round; GS lanes of one wave per stack */
template <int GS, int CAP, bool HAS_T>
__device__ __forceinline__ void wc_flush(const WcView &w, u32 par, void *out)
{
	const u32 nt = w.ntask[par], q = threadIdx.x & (GS - 1);
	for (u32 ti = threadIdx.x / GS; ti < nt; ti += blockDim.x / GS) {
		const u32 b = w.task[ti];
		const u32 cn = w.cnt[b], stored = cn < (u32)CAP ? cn : (u32)CAP, h0 = w.head[b], need = GS - (h0 & (GS - 1));
		const u32 two = stored - need >= (u32)GS;                 /* a second whole group behind the first */
		const u32 flushed = need + GS * two, rem = stored - flushed;
		if (q < need) wc_store<HAS_T>(out, h0 + q, w.h[b * CAP + q], HAS_T ? w.t[b * CAP + q] : 0);
		if (two) wc_store<HAS_T>(out, h0 + need + q, w.h[b * CAP + need + q], HAS_T ? w.t[b * CAP + need + q] : 0);
		u64 mh = 0; u32 mt = 0;
		if (q < rem) { mh = w.h[b * CAP + flushed + q]; if (HAS_T) mt = w.t[b * CAP + flushed + q]; }
		__builtin_amdgcn_wave_barrier();
		if (q < rem) { w.h[b * CAP + q] = mh; if (HAS_T) w.t[b * CAP + q] = mt; }
		if (q == 0) { w.head[b] = h0 + flushed; w.cnt[b] = rem; }
	}
	if (threadIdx.x == 0) w.ntask[par ^ 1] = 0;
}

/* after the last round: what is left in the stacks (fewer records than reach the next boundary) */
template <int GS, int CAP, bool HAS_T>
__device__ __forceinline__ void wc_drain(const WcView &w, int NB, void *out)
{
	const u32 q = threadIdx.x & (GS - 1);
	for (u32 b = threadIdx.x / GS; b < (u32)NB; b += blockDim.x / GS) {
		const u32 cn = w.cnt[b], stored = cn < (u32)CAP ? cn : (u32)CAP;
		if (q < stored) wc_store<HAS_T>(out, w.head[b] + q, w.h[b * CAP + q], HAS_T ? w.t[b * CAP + q] : 0);
	}
}

/* The same write combining, STABLE at round granularity (tagged 8-byte records, groups of 8): a record that finds its stack
 * full is stored at once at its final place, head + position in the stack's count, and the flush of that round then empties the
 * whole stack in front of it -- so inside a bucket the records of a round stay together and the rounds stay in order.  Uses
 * w.tail as the per-bucket toggle. */
template <int CAP>
__device__ __forceinline__ void wcs_place(const WcView &w, u32 b, u64 v, u32 par, u64 *out)
{
	const u32 pos = atomicAdd(&w.cnt[b], 1u), h0 = w.head[b];
	if (pos < (u32)CAP) yk_lds_rw(u64, w.h)[b * CAP + pos] = v; else yk_global_rw(u64, out)[h0 + pos] = v;
	if (pos == 7u - (h0 & 7u)) w.task[atomicAdd(&w.ntask[par], 1u)] = b;
}
template <int CAP>
__device__ __forceinline__ void wcs_flush(const WcView &w, u32 par, u64 *out)
{
	const u32 nt = w.ntask[par], q = threadIdx.x & 7;
	for (u32 ti = threadIdx.x / 8; ti < nt; ti += blockDim.x / 8) {
		const u32 b = w.task[ti];
		const u32 cn = w.cnt[b], h0 = w.head[b];
		if (cn > (u32)CAP) {                                            /* the round overflowed the stack: everything goes, the direct stores sit behind it */
			for (u32 i = q; i < (u32)CAP; i += 8) out[h0 + i] = w.h[b * CAP + i];
			__builtin_amdgcn_wave_barrier();
			if (q == 0) { w.head[b] = h0 + cn; w.cnt[b] = 0; }
			continue;
		}
		const u32 need = 8 - (h0 & 7);
		const u32 two = cn - need >= 8u;
		const u32 flushed = need + 8 * two, rem = cn - flushed;
		if (q < need) out[h0 + q] = w.h[b * CAP + q];
		if (two) out[h0 + need + q] = w.h[b * CAP + need + q];
		u64 mh = 0;
		if (q < rem) mh = w.h[b * CAP + flushed + q];
		__builtin_amdgcn_wave_barrier();
		if (q < rem) w.h[b * CAP + q] = mh;
		if (q == 0) { w.head[b] = h0 + flushed; w.cnt[b] = rem; }
	}
	if (threadIdx.x == 0) w.ntask[par ^ 1] = 0;
}

#define XW_CAP_S 7                                     /* 2 workgroups per CU; the 8th record of a group is stored directly and takes the stack with it */
template <bool TAG, int KC = 0>   /* KC: xt_kmer's constant k.  TAG: tagged records (rows carry the toggle); else bare hashes for the count-existing passes (plain rows) */
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))    /* two workgroups per CU: <= 64 VGPRs and <= 80 SGPRs */
void k_xpart_wcs(const uint8_t *__restrict__ bases, int64_t pos0, int64_t n, int k, int pre, int plo, int phi,
                 int nb_bits, const u32 *__restrict__ rows, u64 *__restrict__ out, int ytag, const u32 *__restrict__ valid)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	__shared__ XtTile S;
	const int NB = 1 << nb_bits, tid = threadIdx.x;
	WcView w;
	wc_carve<8, XW_CAP_S, false>(w, s_dyn, NB, 1024);
	const u32 *row = rows + (size_t)blockIdx.x * NB;
	for (int b = tid; b < NB; b += 1024) { const u32 v = row[b]; w.cnt[b] = 0; w.head[b] = TAG ? v & 0x7fffffffu : v; w.tail[b] = v >> 31; }
	if (tid < 2) w.ntask[tid] = 0;
	xt_init(S);
	const u64 mask = (1ull << (2 * k)) - 1, kones = (1ull << k) - 1;
	const u32 pmask = (1u << pre) - 1;
	u32 par = 0;
	auto rounds = [&](const int64_t tile0) {
#pragma unroll 1                                                      /* unrolled, the four rounds keep their addresses in registers and spill: a reload after a barrier waits for every store in flight */
		for (int r = 0; r < XT_TILE / 1024; ++r, par ^= 1) {
			u64 h;
			bool ok = xt_kmer<KC>(S, r * 1024 + tid, k, mask, kones, tile0, n, &h);
			const u32 p = (u32)h & pmask;
			ok = ok && (int)p >= plo && (int)p < phi;
			u32 bk = 0, tg = 0;
			if (ok) {
				bk = bucket_of(h, pre, nb_bits);
				if (TAG) tg = w.tail[bk];
				/* bare hashes, ytag: the sub-table's own bits (the bucket says them) make room for the top bits of the home-slot product
				 * (khashl.h __kh_h2b), so that k_img_count_own's range test is a shift and a compare */
				const u64 hv = ytag ? (h & ~(u64)pmask) | (((u32)(h >> pre) * 2654435769u) >> (32 - pre)) : h;
				wcs_place<XW_CAP_S>(w, bk, TAG ? (h >> pre) << YK_R8_TAG_BITS | (u64)(tg << 10) | (u32)tid : hv, par, out);
			}
			__syncthreads();
			if (TAG && ok) w.tail[bk] = tg ^ 1;                           /* every lane of the bucket writes the same value: the next contributing round gets the other toggle */
			wcs_flush<XW_CAP_S>(w, par, out);
			__syncthreads();
		}
	};
	const int64_t first = pos0 + (int64_t)blockIdx.x * XP_T * XT_TILE;
	if (valid || n < 16) {
		for (int t = 0; t < XP_T && first + (int64_t)t * XT_TILE < n; ++t) {
			xt_load(S, bases, first + (int64_t)t * XT_TILE, n, valid);
			rounds(first + (int64_t)t * XT_TILE);
		}
	} else {
		XtRaw<1024> raw;
		xt_fetch<1024>(raw, bases, first, n);
		for (int t = 0; t < XP_T && first + (int64_t)t * XT_TILE < n; ++t) {
			const int64_t tile0 = first + (int64_t)t * XT_TILE;
			xt_put<1024>(S, raw, bases, tile0, n);
			xt_fetch<1024>(raw, bases, tile0 + XT_TILE, n);               /* the next tile, in flight during this one's rounds */
			rounds(tile0);
		}
	}
	wc_drain<8, XW_CAP_S, false>(w, NB, out);
}

/* k_xpart's scatter with write combining: 1024 threads, one round = one quarter tile */
#define XW_NT 1024
#define XW_CAP_T 6          /* {hash, position}: groups of 4 */
#define XW_CAP_H 11         /* hash only: groups of 8 */
template <int MODE>   /* 1 = {hash, position}, 2 = hash only */
__global__ __launch_bounds__(XW_NT)
void k_xpart_wc(const uint8_t *__restrict__ bases, int64_t pos0, int64_t n, int64_t t_sub, int k, int pre, int plo, int phi,
                int nb_bits, const u32 *__restrict__ rows, const u64 *__restrict__ bstart, void *__restrict__ out, const u32 *__restrict__ valid)
{
	constexpr bool HAS_T = MODE == 1;
	constexpr int GS = HAS_T ? 4 : 8, CAP = HAS_T ? XW_CAP_T : XW_CAP_H;
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	__shared__ XtTile S;
	const int NB = 1 << nb_bits, tid = threadIdx.x;
	WcView w;
	wc_carve<GS, CAP, HAS_T>(w, s_dyn, NB, XW_NT);
	const u32 *row = rows + (size_t)blockIdx.x * NB;
	const bool last = blockIdx.x + 1 == gridDim.x;
	for (int b = tid; b < NB; b += XW_NT) {
		w.cnt[b] = 0; w.head[b] = row[b];
		w.tail[b] = last ? (u32)bstart[b + 1] : row[NB + b];      /* the next workgroup's run starts where mine ends */
	}
	if (tid < 2) w.ntask[tid] = 0;
	xt_init(S);
	const u64 mask = k < 32 ? (1ull << (2 * k)) - 1 : ~0ull, kones = (1ull << k) - 1;
	const u32 pmask = (1u << pre) - 1;
	u32 par = 0;
	auto rounds = [&](const int64_t tile0) {
#pragma unroll 1
		for (int r = 0; r < XT_TILE / XW_NT; ++r, par ^= 1) {
			const int q = r * XW_NT + tid;
			u64 h;
			bool ok = k < 32 ? xt_kmer(S, q, k, mask, kones, tile0, n, &h) : xt_kmer_long(S, q, k, pre, tile0, n, &h);
			const u32 p = (u32)h & pmask;
			ok = ok && (int)p >= plo && (int)p < phi;
			if (ok) wc_place<GS, CAP, HAS_T>(w, bucket_of(h, pre, nb_bits), h, (u32)(tile0 + q - t_sub), par, out);
			__syncthreads();
			wc_flush<GS, CAP, HAS_T>(w, par, out);
			__syncthreads();
		}
	};
	const int64_t first = pos0 + (int64_t)blockIdx.x * XP_T * XT_TILE;
	if (valid || n < 16) {
		for (int t = 0; t < XP_T && first + (int64_t)t * XT_TILE < n; ++t) {
			xt_load(S, bases, first + (int64_t)t * XT_TILE, n, valid);
			rounds(first + (int64_t)t * XT_TILE);
		}
	} else {
		XtRaw<XW_NT> raw;
		xt_fetch<XW_NT>(raw, bases, first, n);
		for (int t = 0; t < XP_T && first + (int64_t)t * XT_TILE < n; ++t) {
			const int64_t tile0 = first + (int64_t)t * XT_TILE;
			xt_put<XW_NT>(S, raw, bases, tile0, n);
			xt_fetch<XW_NT>(raw, bases, tile0 + XT_TILE, n);
			rounds(tile0);
		}
	}
	wc_drain<GS, CAP, HAS_T>(w, NB, out);
}

#define RP_CHUNK 65536
template <int MODE>
__global__ __launch_bounds__(256)
void k_rpart(const u64 *__restrict__ in_hash, const u32 *__restrict__ in_t, int64_t n, int pre, int plo, int phi,
             int nb_bits, u32 *rows, Rec *__restrict__ out)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_bkt[];
	const int NB = 1 << nb_bits;
	u32 *row = rows + (size_t)blockIdx.x * NB;
	for (int j = threadIdx.x; j < NB; j += 256) s_bkt[j] = MODE ? row[j] : 0;
	__syncthreads();
	const int64_t lo = (int64_t)blockIdx.x * RP_CHUNK, hi = lo + RP_CHUNK < n ? lo + RP_CHUNK : n;
	const u32 pmask = (1u << pre) - 1;
	for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
		const u64 h = in_hash[i];
		const u32 p = (u32)h & pmask;
		if ((int)p >= plo && (int)p < phi) {
			const u32 d = atomicAdd(&s_bkt[bucket_of(h, pre, nb_bits)], 1u);
			if (MODE) out[d] = make_ulonglong2(h, (u64)in_t[i]);
		}
	}
	if (!MODE) { __syncthreads(); for (int j = threadIdx.x; j < NB; j += 256) row[j] = s_bkt[j]; }
}

/* rows[blk][b] (counts) -> rows[blk][b] (absolute start of that workgroup's run in bucket b);
 * bstart[b] = first record of bucket b, bstart[NB] = total.  Rows are summed in PS_G groups so the
 * scan is three short, wide kernels instead of one long serial one. */
#define PS_G 64
#define PS_PAR (1ull << 63)
template <bool PAR>   /* PAR: rows hold count | contributing rounds << 24; bit 63 of the sums carries the parity of the rounds */
__global__ __launch_bounds__(256)
void k_part_sum(const u32 *rows, int n_blk, int NB, u64 *partial)
{
	const int b = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
	if (b >= NB) return;
	const int per = (n_blk + PS_G - 1) / PS_G, lo = g * per, hi = lo + per < n_blk ? lo + per : n_blk;
	u64 acc = 0;
	for (int i = lo; i < hi; ++i) { const u32 v = rows[(size_t)i * NB + b]; if (PAR) acc = (acc + (v & 0xffffffu)) ^ ((u64)(v >> 24 & 1) << 63); else acc += v; }
	partial[(size_t)g * NB + b] = acc;
}

__global__ __launch_bounds__(256)
void k_part_mid(u64 *partial, int NB, u64 *bstart)
{
	__shared__ u64 s_tot[256];
	__shared__ u64 s_carry;
	if (threadIdx.x == 0) s_carry = 0;
	__syncthreads();
	for (int b0 = 0; b0 < NB; b0 += 256) {
		const int b = b0 + threadIdx.x;
		u64 run = 0;
		if (b < NB) for (int g = 0; g < PS_G; ++g) { const u64 c = partial[(size_t)g * NB + b]; partial[(size_t)g * NB + b] = run; run = (run + (c & ~PS_PAR)) ^ (c & PS_PAR); }   /* bit 63: parity of the rounds so far (always 0 without PAR) */
		run &= ~PS_PAR;
		s_tot[threadIdx.x] = run;
		__syncthreads();
		if (threadIdx.x == 0) {
			u64 acc = s_carry;
			for (int j = 0; j < 256; ++j) { const u64 c = s_tot[j]; s_tot[j] = acc; acc += c; }
			s_carry = acc;
		}
		__syncthreads();
		if (b < NB) bstart[b] = s_tot[threadIdx.x];
		__syncthreads();
	}
	if (threadIdx.x == 0) bstart[NB] = s_carry;
}

template <bool PAR>
__global__ __launch_bounds__(256)
void k_part_fin(u32 *rows, int n_blk, int NB, const u64 *partial, const u64 *bstart)
{
	const int b = blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
	if (b >= NB) return;
	const int per = (n_blk + PS_G - 1) / PS_G, lo = g * per, hi = lo + per < n_blk ? lo + per : n_blk;
	const u64 pg = partial[(size_t)g * NB + b];
	u64 run = bstart[b] + (pg & ~PS_PAR);
	u32 par = (u32)(pg >> 63);
	for (int i = lo; i < hi; ++i) {
		const u32 c = rows[(size_t)i * NB + b];
		if (PAR) { rows[(size_t)i * NB + b] = (u32)run | par << 31; run += c & 0xffffffu; par ^= c >> 24 & 1; }   /* start (< 2^31) | toggle of the workgroup's first contributing round */
		else { rows[(size_t)i * NB + b] = (u32)run; run += c; }
	}
}

static void launch_part_scan(u32 *rows, int n_blk, int nb_bits, u64 *partial, u64 *bstart, hipStream_t st, bool par = false)
{
	const int NB = 1 << nb_bits;
	if (par) YK_LAUNCH(k_part_sum<true>, dim3((NB + 255) / 256, PS_G), dim3(256), 0, st, rows, n_blk, NB, partial);
	else YK_LAUNCH(k_part_sum<false>, dim3((NB + 255) / 256, PS_G), dim3(256), 0, st, rows, n_blk, NB, partial);
	YK_LAUNCH(k_part_mid, dim3(1), dim3(256), 0, st, partial, NB, bstart);
	if (par) YK_LAUNCH(k_part_fin<true>, dim3((NB + 255) / 256, PS_G), dim3(256), 0, st, rows, n_blk, NB, partial, bstart);
	else YK_LAUNCH(k_part_fin<false>, dim3((NB + 255) / 256, PS_G), dim3(256), 0, st, rows, n_blk, NB, partial, bstart);
}

/* ------------------------------------------------------------------------------------------
 * table image probing (khashl get, reference khashl.h:137-150 / htab.c:93-100)
 * ------------------------------------------------------------------------------------------ */
__device__ __forceinline__ int64_t img_find(const ImgView &img, u64 key)
{
	const u32 p = (u32)key & ((1u << img.pre) - 1);
	const u32 bits = img.bits[p];
	if (bits == YK_NOCAP) return -1;
	const u64 kid = key >> img.pre;
	const u64 off = img.off[p];
	const u32 nmask = (1u << bits) - 1;
	u32 i = yk_h2b((u32)kid, bits);
	const u32 first = i;
	for (;;) {
		const u64 a = off + i;
		if (!(img.used[a >> 5] >> (a & 31) & 1)) return -1;
		if (img.keys[a] >> 10 == kid) return (int64_t)a;
		i = (i + 1) & nmask;
		if (i == first) return -1;
	}
}

/* ------------------------------------------------------------------------------------------
 * lookup-only paths: t = max(0, yak_ch_get()) of the k-mer ENDING at every position of a base image, all ones of the output element where
 * none ends (window shorter than k or holding a non-ACGT byte); then a reduction per sequence.
 *   `yak qv` (reference qv.c:34-86): u16 t (QV_NOKMER); per sequence tot = k-mers, non0 = present ones, and the sequences with
 *   non0 >= tot * min_frac add all their t values to the 1024-bin histogram.
 *   `yak triobin` (reference triobin.c:41-101): u8 t (TB_NOKMER), a flag.  The table comes from the two YAK_LOAD_TRIOBIN loads, which OR a
 *   2-bit class per parent into the count field, so a flag is 4 bits.
 * ------------------------------------------------------------------------------------------ */
#define QV_NOKMER 0xffffu
__device__ __forceinline__ bool lk_used(const ImgView &img, u64 slot) { return img.used[slot >> 5] >> (slot & 31) & 1; }
#define TB_NOKMER 0xffu
__device__ u32 d_tb_over;          /* triobin: a probed count field above 15 was met */
/* yak_ch_get() clamped at 0 (qv.c:59-60, triobin.c:62-84), read-only and on the key array alone: the image keeps every unused slot at YK_EMPTY
 * (k_replay publishes it so), and no stored key equals it, so the `used` bitmap -- a second random 64-byte read per probe -- is not needed.  At
 * k < 32 no 2k < 64-bit key can equal it.  At k >= 32 a 64-bit hash can make (hash >> pre) << 10 all ones, but a TRIOBIN load stores a count
 * field of at most 15, never 1023.  A count field above 15 means the table did not come from those loads (the reference would index past its
 * c[16]): the one-byte lookup raises d_tb_over and its caller fails.
 * The sub-tables' {offset, log2 capacity} sit in LDS (dynamic: 8 bytes per sub-table while pre <= 12): a probe is then one dependent global read,
 * not three; LK_U positions of a lane are hashed first and their home slots requested together (the probe of one position used to wait for the
 * one before it) */
/* CE (`yak chkerr`, reference chkerr.c:60-61): the byte is 1 where the signed yak_ch_get() < min_cnt (-1 for an absent k-mer, so min_cnt 0 marks the
 * absent ones alone), 0 where it is not, CE_NOKMER where no k-mer ends.  The table is a YAK_LOAD_ALL one: at k >= 32 a stored key at count 1023 can
 * equal YK_EMPTY, so there a YK_EMPTY slot asks the `used` bitmap before the probe stops (as img_find and k_inspect<., true> do).  CE = false
 * compiles to the code it did before the mode existed (min_cnt unused). */
#define LK_U 2                             /* probes a lane keeps in flight */
#define CE_NOKMER 0xffu
template <typename T, bool LONG, bool CE = false>   /* T: unsigned short (qv) or uint8_t (triobin's flag, chkerr's low byte); LONG: k in [32, 63],
                                                     * yak_hash_long (triobin.c:78-81) */
__global__ __launch_bounds__(XT_THREADS)
void k_lookup(const uint8_t *__restrict__ bases, int64_t n, int k, ImgView img, T *__restrict__ out, int tab, int min_cnt)
{
	static_assert(!CE || sizeof(T) == 1, "chkerr writes one byte per position");
	constexpr u32 NOKMER = CE ? 0xffffffffu : (u32)(T)~0u;   /* CE: a count of 255 is not "no k-mer" */
	constexpr u32 ABSENT = 1024u;          /* CE: above every count field */
	constexpr bool FLAG = sizeof(T) == 1 && !CE;   /* a flag holds 4 bits */
	__shared__ XtTile S;
	extern __shared__ __attribute__((aligned(16))) u64 s_tab[];
	const u32 pmask = (1u << img.pre) - 1;
	if (tab) for (u32 p = threadIdx.x; p <= pmask; p += XT_THREADS) { const u32 b = img.bits[p]; s_tab[p] = img.off[p] | (u64)(b == YK_NOCAP ? 63u : b) << 58; }
	xt_init(S);
	const u64 mask = LONG ? 0 : (1ull << (2 * k)) - 1, kones = LONG ? 0 : (1ull << k) - 1;
	const u64 YK_GLOBAL *karena = yk_global(u64, img.keys);
	u32 over = 0;
	for (int t = 0; t < XP_T; ++t) {
		const int64_t tile0 = ((int64_t)blockIdx.x * XP_T + t) * XT_TILE;
		if (tile0 >= n) break;
		xt_load(S, bases, tile0, n);
		for (int r0 = 0; r0 < XT_ROUNDS; r0 += LK_U) {
			u64 kid[LK_U], kc[LK_U];
			const u64 YK_GLOBAL *keys[LK_U];
			u32 idx[LK_U], nmask[LK_U], v[LK_U];
			bool live[LK_U];
#pragma unroll
			for (int u = 0; u < LK_U; ++u) {
				const int q = (r0 + u) * XT_THREADS + (int)threadIdx.x;
				u64 h;
				const bool ok = LONG ? xt_kmer_long(S, q, k, img.pre, tile0, n, &h) : xt_kmer(S, q, k, mask, kones, tile0, n, &h);
				const u32 p = (u32)h & pmask;
				v[u] = ok ? (CE ? ABSENT : 0u) : NOKMER;
				/* htab.c:93-100 compares (hash >> pre) << 10 >> 10: the stored key keeps 54 bits of it, all of them at k < 32 (pre >= 10) */
				live[u] = false; kid[u] = LONG ? (h >> img.pre) & (~0ull >> 10) : h >> img.pre; keys[u] = karena; idx[u] = 0; nmask[u] = 0;
				if (ok) {
					u64 off; u32 bits;
					if (tab) { const u64 e = s_tab[p]; off = e & ((1ull << 58) - 1); bits = (u32)(e >> 58); bits = bits == 63u ? YK_NOCAP : bits; }
					else { bits = img.bits[p]; off = img.off[p]; }
					if (bits != YK_NOCAP) { live[u] = true; keys[u] = karena + off; nmask[u] = (1u << bits) - 1; idx[u] = yk_h2b((u32)kid[u], bits); }
				}
			}
#pragma unroll
			for (int u = 0; u < LK_U; ++u) kc[u] = live[u] ? keys[u][idx[u]] : YK_EMPTY;
#pragma unroll
			for (int u = 0; u < LK_U; ++u) {
				const u32 first = idx[u];
				while (kc[u] != YK_EMPTY || (CE && LONG && live[u] && lk_used(img, (u64)(keys[u] - karena) + idx[u]))) {
					if (kc[u] >> 10 == kid[u]) { v[u] = (u32)(kc[u] & 1023u); break; }
					idx[u] = (idx[u] + 1) & nmask[u];
					if (idx[u] == first) break;
					kc[u] = keys[u][idx[u]];
				}
				if (FLAG && v[u] != NOKMER && v[u] > 15u) { over = 1; v[u] &= 15u; }
				if (CE) v[u] = v[u] == NOKMER ? CE_NOKMER : (v[u] == ABSENT ? -1 : (int)v[u]) < min_cnt ? 1u : 0u;
				const int64_t pos = tile0 + (r0 + u) * XT_THREADS + (int)threadIdx.x;
				if (pos < n) out[pos] = (T)v[u];
			}
		}
		__syncthreads();
	}
	if (FLAG && over) d_tb_over = 1;
}

/* one wave per sequence; tot = 0xffffffff marks a sequence below min_len (qv.c:45) */
__global__ __launch_bounds__(256)
void k_qv_reduce(const unsigned short *__restrict__ t, const u64 *__restrict__ roff, const u32 *__restrict__ rlen, int64_t n_reads,
                 int min_len, double min_frac, u32 *tot_out, u32 *non0_out, unsigned long long *hist)
{
	__shared__ u32 s_hist[1024];
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (u32 i = threadIdx.x; i < 1024; i += 256) s_hist[i] = 0;
	__syncthreads();
	for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n_reads; r += (int64_t)gridDim.x * 4) {
		const u64 off = roff[r];
		const u32 len = rlen[r];
		if ((int64_t)len < (int64_t)min_len) { if (lane == 0) { tot_out[r] = 0xffffffffu; non0_out[r] = 0; } continue; }
		u32 tot = 0, non0 = 0;
		for (u32 i = lane; i < len; i += 64) { const u32 v = t[off + i]; if (v != QV_NOKMER) { ++tot; non0 += v > 0; } }
		for (int o = 32; o > 0; o >>= 1) { tot += __shfl_xor(tot, o); non0 += __shfl_xor(non0, o); }
		if (lane == 0) { tot_out[r] = tot; non0_out[r] = non0; }
		if ((double)non0 < (double)tot * min_frac) continue;                /* qv.c:83 */
		for (u32 i = lane; i < len; i += 64) { const u32 v = t[off + i]; if (v != QV_NOKMER) atomicAdd(&s_hist[v], 1u); }
	}
	__syncthreads();
	for (u32 i = threadIdx.x; i < 1024; i += 256) if (s_hist[i]) atomicAdd(&hist[i], (unsigned long long)s_hist[i]);
}

/* triobin's per-read reduction (triobin.c:74-100): one wave per read, 64 positions per step.
 *   c[16]  histogram of the flags over the positions that have a k-mer; nk = their number
 *   sc[2]  a position's type is 1 where flag == 2 (pat solid, mat absent), 2 where flag == 8, 0
 *          elsewhere (also where no k-mer ends); every maximal run of one type t > 0 and length
 *          >= k - 4 adds its length to sc[t - 1]
 * The run open at a step's start is carried as (start, type); the step's run starts are a ballot,
 * walked bit by bit with scalar ops.  A run of type 0 "opens" at position 0: it adds nothing, and a
 * read that starts with a typed position closes it at once.
 * Output per read: 19 int32 = c[0..15], sc[0], sc[1], nk. */
__global__ __launch_bounds__(256)
void k_tb_reduce(const uint8_t *__restrict__ flag, const u64 *__restrict__ roff, const u32 *__restrict__ rlen, int64_t n_reads, int k,
                 int *__restrict__ cnt)
{
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t min_run = (int64_t)k - 4;
	for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n_reads; r += (int64_t)gridDim.x * 4) {
		const uint8_t *f = flag + roff[r];
		const u32 len = rlen[r];
		u32 mine = 0;                                 /* lane j < 16: c[j] */
		int64_t run0 = 0, sc0 = 0, sc1 = 0;
		u32 rtype = 0;
		u32 nxt = lane < len ? f[lane] : TB_NOKMER;
		for (u32 base = 0; base < len; base += 64) {
			const u32 i = base + lane;
			const u32 v = nxt;
			nxt = i + 64 < len ? f[i + 64] : TB_NOKMER;              /* the next step's load in flight during this one */
			const u32 ty = v == 2u ? 1u : v == 8u ? 2u : 0u;
			const u64 in = __ballot(i < len);
			const u64 t1 = __ballot(ty == 1u), t2 = __ballot(ty == 2u);
#pragma unroll
			for (u32 j = 0; j < 16; ++j) { const u32 c = (u32)__popcll(__ballot(v == j)); mine += lane == j ? c : 0u; }
			/* run starts: positions whose type differs from the one before (lane 0: from the run carried in) */
			const u32 prev = __shfl_up(ty, 1);
			const u64 starts = __ballot(lane == 0 ? ty != rtype : ty != prev) & in;
			for (u64 m = starts; m; m &= m - 1) {
				const u32 j = (u32)__ffsll((unsigned long long)m) - 1;
				const int64_t p = (int64_t)base + j, l = p - run0;
				if (rtype && l >= min_run) { if (rtype == 1) sc0 += l; else sc1 += l; }
				run0 = p;
				rtype = (t1 >> j & 1) ? 1u : (t2 >> j & 1) ? 2u : 0u;
			}
		}
		{
			const int64_t l = (int64_t)len - run0;
			if (rtype && l >= min_run) { if (rtype == 1) sc0 += l; else sc1 += l; }
		}
		int *o = cnt + r * 19;
		if (lane < 16) o[lane] = (int)mine;
		u32 nk = 0;
		for (int j = 0; j < 16; ++j) nk += __shfl(mine, j);
		if (lane == 16) o[16] = (int)sc0;
		if (lane == 17) o[17] = (int)sc1;
		if (lane == 18) o[18] = (int)nk;
	}
}

/* width 2: qv's counts (k < 32); width 1: triobin's flags, after clearing the flag yk_tb_over_seen() reads */
void yk_launch_lookup(const uint8_t *bases, int64_t n, int k, ImgView img, void *out, int width, hipStream_t st)
{
	if (n <= 0) return;
	/* one sweep over the whole image.  (Probing one prefix range of the image at a time -- each small enough for the 256 MB Infinity Cache, the queries
	 * extracted once per sweep -- was measured on the benchmark's 512 MB image: 2 sweeps 38 ms against 36, 4 sweeps 52; more probes of a lane in flight,
	 * 2 / 4 / 8: 34.3 / 35.2 / 40.8 ms against 34.7.  ~48 G probes/s is the rate at which DRAM rows can be opened) */
	const int tab = img.pre <= 12;
	const size_t lds = tab ? (size_t)8 << img.pre : 0;
	const dim3 grid(yk_xpart_blocks(n)), block(XT_THREADS);
	if (width == 2) { YK_LAUNCH((k_lookup<unsigned short, false>), grid, block, lds, st, bases, n, k, img, (unsigned short*)out, tab, 0); return; }
	void *over = 0;
	if (hipGetSymbolAddress(&over, HIP_SYMBOL(d_tb_over)) == hipSuccess) (void)hipMemsetAsync(over, 0, 4, st);
	if (k < 32) YK_LAUNCH((k_lookup<uint8_t, false>), grid, block, lds, st, bases, n, k, img, (uint8_t*)out, tab, 0);
	else YK_LAUNCH((k_lookup<uint8_t, true>), grid, block, lds, st, bases, n, k, img, (uint8_t*)out, tab, 0);
}

/* chkerr's low byte per position (1 / 0 / CE_NOKMER), k in [1, 63] */
void yk_launch_ce_lookup(const uint8_t *bases, int64_t n, int k, ImgView img, uint8_t *out, int min_cnt, hipStream_t st)
{
	if (n <= 0) return;
	const int tab = img.pre <= 12;
	const size_t lds = tab ? (size_t)8 << img.pre : 0;
	const dim3 grid(yk_xpart_blocks(n)), block(XT_THREADS);
	if (k < 32) YK_LAUNCH((k_lookup<uint8_t, false, true>), grid, block, lds, st, bases, n, k, img, out, tab, min_cnt);
	else YK_LAUNCH((k_lookup<uint8_t, true, true>), grid, block, lds, st, bases, n, k, img, out, tab, min_cnt);
}

int yk_tb_over_seen(hipStream_t st)
{
	u32 v = 0;
	(void)hipStreamSynchronize(st);
	(void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(d_tb_over), 4);
	return (int)v;
}

void yk_launch_qv_reduce(const unsigned short *t, const u64 *roff, const u32 *rlen, int64_t n_reads, int min_len, double min_frac,
                         u32 *tot_out, u32 *non0_out, u64 *hist, hipStream_t st)
{
	if (n_reads <= 0) return;
	const int64_t want = (n_reads + 3) / 4;
	YK_LAUNCH(k_qv_reduce, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, st, t, roff, rlen, n_reads, min_len, min_frac,
	                   tot_out, non0_out, (unsigned long long*)hist);
}

void yk_launch_tb_reduce(const uint8_t *flag, const u64 *roff, const u32 *rlen, int64_t n_reads, int k, int *cnt, hipStream_t st)
{
	if (n_reads <= 0) return;
	const int64_t want = (n_reads + 3) / 4;
	YK_LAUNCH(k_tb_reduce, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, st, flag, roff, rlen, n_reads, k, cnt);
}
