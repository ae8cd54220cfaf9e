/* kern_hpc.inc -- part of kernels.hip: homopolymer compression of a base image (not in the reference; DESIGN.md section 18).
 *
 * Position i of an image is DROPPED iff i > 0, positions i and i - 1 are both valid (code 0..3 under d_nt4) and hold the same code; every other
 * position is kept, an invalid one too (it ends the run before it and is written as '\n').  The output is the kept positions in order as an ASCII
 * image: 'A' 'C' 'G' 'T' or '\n', then '\n' up to the next multiple of 16 bytes.  A stream compaction in three launches, none of which waits for
 * another workgroup:
 *   k_hpc_count     tcnt[tile] = kept positions of the tile
 *   k_te_scan       their exclusive scan (kern_trioeval.inc: one block; the tiles are 4 Ki or 16 Ki positions)
 *   k_hpc_scatter   the flags again, the tile's kept bytes put together in LDS, written out in whole 16-byte words
 * and a fourth for the callers that address sequences inside the image:
 *   k_hpc_remap     off_out[j] / len_out[j] = kept positions before / inside sequence j: the scan's entry of its tile plus a recount inside that tile
 *
 * The input is a template parameter.  HpAscii: the ASCII image, 16 positions (one 16-byte load) per lane, coded through the table in LDS.  HpPacked:
 * the packed image of yakamd_feed_packed_dev, 64 positions per lane (one 16-byte load of code words, two validity words).  Both hand a lane its
 * positions as 2-bit code words plus a validity mask, and the flags are computed on whole words: position j differs from j - 1 where the code word
 * XOR itself shifted by one code is non-zero in code j.  The shift pulls in the code of the position before the lane's first one -- the halo: the
 * last code of the word before (and its validity bit), read from memory by the lane itself, so the first lane of a tile needs nothing from the tile
 * before it and position 0 of the image has no predecessor.
 */
#define HP_THREADS TE_THREADS                  /* te_block_scan's block */

struct HpAscii {
	enum { PER = 16, CW = 1 };
	const uint8_t *a;
	/* positions [p0, p0 + 16) below n (p0 < n): their codes, 2 bits each (0 where invalid), and validity bits */
	__device__ __forceinline__ void load(int64_t p0, int64_t n, const unsigned char *lut, u32 *cw, u64 *vm) const
	{
		u32 c = 0, v = 0;
		if (p0 + PER <= n) {
			const uint4 w = *(const uint4*)(a + p0);
			const u32 ws[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
			for (int j = 0; j < PER; ++j) { const u32 x = lut[ws[j >> 2] >> (8 * (j & 3)) & 0xffu]; c |= (x & 3u) << (2 * j); v |= (u32)(x < 4u) << j; }
		} else {
			for (int j = 0; j < PER && p0 + j < n; ++j) { const u32 x = lut[a[p0 + j]]; c |= (x & 3u) << (2 * j); v |= (u32)(x < 4u) << j; }
		}
		cw[0] = c; *vm = v;
	}
	/* code | validity << 2 of position p (0 <= p < n) */
	__device__ __forceinline__ u32 halo(int64_t p, const unsigned char *lut) const { const u32 x = lut[a[p]]; return x < 4u ? x | 4u : 0u; }
};

struct HpPacked {
	enum { PER = 64, CW = 4 };
	const u32 *codes, *valid;
	/* words that begin at or behind position n are not read (yak_amd.h: nothing beyond the last partial word) */
	__device__ __forceinline__ void load(int64_t p0, int64_t n, const unsigned char *, u32 *cw, u64 *vm) const
	{
		const int64_t w = p0 >> 4, vw = p0 >> 5;
		if (p0 + PER <= n) {
			const uint4 q = *(const uint4*)(codes + w);
			cw[0] = q.x; cw[1] = q.y; cw[2] = q.z; cw[3] = q.w;
			*vm = (u64)valid[vw] | (u64)valid[vw + 1] << 32;
		} else {
#pragma unroll
			for (int i = 0; i < CW; ++i) cw[i] = p0 + 16 * i < n ? codes[w + i] : 0u;
			*vm = (u64)valid[vw] | (p0 + 32 < n ? (u64)valid[vw + 1] << 32 : 0ull);
		}
	}
	__device__ __forceinline__ u32 halo(int64_t p, const unsigned char *) const
	{
		const u32 v = valid[p >> 5] >> (p & 31) & 1u;
		return v ? (codes[p >> 4] >> (2 * (p & 15)) & 3u) | 4u : 0u;
	}
};

/* the 16 even bits of x, packed */
__device__ __forceinline__ u32 hp_even_bits(u32 x)
{
	x &= 0x55555555u;
	x = (x | x >> 1) & 0x33333333u;
	x = (x | x >> 2) & 0x0f0f0f0fu;
	x = (x | x >> 4) & 0x00ff00ffu;
	return (x | x >> 8) & 0xffffu;
}

/* the kept positions of a lane: L::PER positions from p0 (< n) on; the lane's code words and validity mask come back for the scatter */
template <class L>
__device__ __forceinline__ u64 hp_keep(const L &in, int64_t p0, int64_t n, const unsigned char *lut, u32 *cw, u64 *vm)
{
	in.load(p0, n, lut, cw, vm);
	const u32 h = p0 > 0 ? in.halo(p0 - 1, lut) : 0u;
	const u64 inb = n - p0 >= (int64_t)L::PER ? (L::PER == 64 ? ~0ull : (1ull << (L::PER & 63)) - 1) : (1ull << (n - p0)) - 1;
	*vm &= inb;
	u64 ne = 0;
	u32 pc = h & 3u;
#pragma unroll
	for (int i = 0; i < L::CW; ++i) {
		const u32 x = cw[i] ^ (cw[i] << 2 | pc);
		pc = cw[i] >> 30;
		ne |= (u64)hp_even_bits(x | x >> 1) << (16 * i);
	}
	const u64 drop = *vm & (*vm << 1 | (u64)(h >> 2)) & ~ne;
	return ~drop & inb;
}

template <class L>
__global__ __launch_bounds__(HP_THREADS)
void k_hpc_count(L in, int64_t n, u32 *__restrict__ tcnt)
{
	__shared__ u32 s_lut[64];
	if (L::CW == 1) { if (threadIdx.x < 64) s_lut[threadIdx.x] = ((const u32*)d_nt4)[threadIdx.x]; __syncthreads(); }
	const int64_t p0 = ((int64_t)blockIdx.x * HP_THREADS + threadIdx.x) * L::PER;
	u32 cw[L::CW] = {}; u64 vm = 0;
	const u64 keep = p0 < n ? hp_keep(in, p0, n, (const unsigned char*)s_lut, cw, &vm) : 0ull;
	u32 tot;
	te_block_scan((u32)__popcll(keep), &tot);
	if (threadIdx.x == 0) tcnt[blockIdx.x] = tot;
}

/* toff = the exclusive scan of tcnt, n_tiles + 1 words.  The tile's bytes are laid out in LDS at the misalignment of their destination, so that
 * the 16-byte words of LDS are the 16-byte words of `out`: whole words in between, single bytes in front of the first and behind the last whole
 * word (the neighbouring tiles write the other bytes of those two words).  The last tile adds the '\n' up to the next multiple of 16 */
template <class L>
__global__ __launch_bounds__(HP_THREADS)
void k_hpc_scatter(L in, int64_t n, const u64 *__restrict__ toff, int64_t n_tiles, uint8_t *__restrict__ out)
{
	__shared__ u32 s_lut[64];
	__shared__ __attribute__((aligned(16))) unsigned char s_out[HP_THREADS * L::PER + 16];
	if (L::CW == 1) { if (threadIdx.x < 64) s_lut[threadIdx.x] = ((const u32*)d_nt4)[threadIdx.x]; __syncthreads(); }
	const int64_t p0 = ((int64_t)blockIdx.x * HP_THREADS + threadIdx.x) * L::PER;
	u32 cw[L::CW] = {}; u64 vm = 0;
	const u64 keep = p0 < n ? hp_keep(in, p0, n, (const unsigned char*)s_lut, cw, &vm) : 0ull;
	u32 tot;
	const u32 before = te_block_scan((u32)__popcll(keep), &tot);
	const u64 dst0 = toff[blockIdx.x];
	const u32 a = (u32)(dst0 & 15);
	u32 o = a + before;
#pragma unroll
	for (int i = 0; i < L::CW; ++i)
		for (u32 m = (u32)(keep >> (16 * i)) & 0xffffu; m; m &= m - 1) {
			const int j = __ffs(m) - 1;
			s_out[o++] = (vm >> (16 * i + j) & 1) ? (unsigned char)(0x54474341u >> (8 * (cw[i] >> (2 * j) & 3u))) : (unsigned char)'\n';
		}
	__syncthreads();
	uint8_t *base = out + (dst0 - a);                          /* 16-byte aligned; LDS byte i is base[i] */
	const u32 e = a + tot, hb = min(e, (a + 15u) & ~15u), be = max(hb, e & ~15u);
	if (threadIdx.x < 16) { const u32 i = a + threadIdx.x; if (i < hb) base[i] = s_out[i]; }
	else if (threadIdx.x < 32) { const u32 i = be + threadIdx.x - 16; if (i < e) base[i] = s_out[i]; }
	for (u32 c = hb / 16 + threadIdx.x; c < be / 16; c += HP_THREADS) ((uint4*)base)[c] = ((const uint4*)s_out)[c];
	if (blockIdx.x == n_tiles - 1 && threadIdx.x >= 32 && threadIdx.x < 48) {
		const u64 n_out = dst0 + tot, i = n_out + threadIdx.x - 32;
		if (i < ((n_out + 15) & ~15ull)) out[i] = '\n';
	}
}

/* kept positions in [lo, hi) of the ASCII image, counted by one wave (16 positions per lane and step); every lane returns the sum */
__device__ __forceinline__ u32 hp_wave_count(const HpAscii &in, int64_t n, int64_t lo, int64_t hi)
{
	u32 c = 0;
	for (int64_t q = (lo & ~(int64_t)15) + 16 * (int64_t)(threadIdx.x & (WAVE - 1)); q < hi; q += 16 * WAVE) {
		u32 cw[1]; u64 vm;
		const u64 keep = hp_keep(in, q, n, d_nt4, cw, &vm);
		const u32 lb = q < lo ? (u32)(lo - q) : 0u, hb = hi - q < 16 ? (u32)(hi - q) : 16u;
		c += (u32)__popcll(keep & ((1ull << hb) - 1) & ~((1ull << lb) - 1));
	}
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o);
	return c;
}

/* one wave per sequence: off_out[j] = kept positions before off[j], len_out[j] = kept positions in [off[j], off[j] + len[j]) (both ends clamped
 * to n).  toff = the tile scan of the ASCII form (tiles of HP_THREADS * 16 positions); no per-position index exists anywhere */
__global__ __launch_bounds__(HP_THREADS)
void k_hpc_remap(HpAscii in, int64_t n, const u64 *__restrict__ toff, const u64 *__restrict__ off, const u32 *__restrict__ len, int64_t n_seq,
                 u64 *__restrict__ off_out, u32 *__restrict__ len_out)
{
	const int64_t TILE = HP_THREADS * HpAscii::PER;
	const int64_t j = ((int64_t)blockIdx.x * HP_THREADS + threadIdx.x) / WAVE;
	if (j >= n_seq) return;
	const int64_t o = (int64_t)off[j] < n ? (int64_t)off[j] : n, e = o + (int64_t)len[j] < n ? o + (int64_t)len[j] : n;
	const u64 kb = toff[o / TILE] + hp_wave_count(in, n, o / TILE * TILE, o);
	const u64 ln = e / TILE == o / TILE ? hp_wave_count(in, n, o, e) : toff[e / TILE] + hp_wave_count(in, n, e / TILE * TILE, e) - kb;
	if ((threadIdx.x & (WAVE - 1)) == 0) { off_out[j] = kb; len_out[j] = (u32)ln; }
}
