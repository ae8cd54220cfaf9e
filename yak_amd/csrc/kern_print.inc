/* kern_print.inc -- part of kernels.hip (one translation unit, included in this order): the listing of `yak print` (reference main.c:302-320 on
 * yak_ch_getseq, htab.c:353-367).  The input is the .yak body of sub-tables [sub_lo, sub_lo + n_sub) as yk_ctx_dump_image_dev() lays it out: per
 * sub-table one {capacity, size} word, then its stored words (hash >> pre) << 10 | count in ascending slot order -- the order getseq walks.  Key i
 * of the range (0 <= i < n) belongs to sub-table j = the last one with off[j] <= i and lies at img[i + j + 1]; its k-mer is
 *     x = yk_hash64_inv((word >> 10) << pre | (sub_lo + j), 4^k - 1)                          (htab.c:365), its count c = word & 1023.
 *   k_kmers        x[i] and c[i], flat
 *   k_print_sizes  with counts: the bytes of each tile's lines (a line is k + 2 + digits(c) bytes), scanned by k_te_scan
 *   k_print        the text.  A tile is PR_TILE consecutive keys; without counts line i starts at i * (k + 1), with counts at the tile's scanned
 *                  offset plus the scan of the line lengths inside the tile.  A line is 16-37 bytes at an offset that is no multiple of 4, so the
 *                  lanes do not store their lines: the workgroup builds the tile's bytes in LDS, shifted by (address of the tile's first byte)
 *                  mod 16, and stores the span with 16-byte vector stores from aligned LDS reads; only the bytes in front of the first and behind
 *                  the last aligned 16 of the span are stored one by one.  Lane t builds lines t, t + 256, ...: neighbouring lanes write
 *                  neighbouring lines (a stride of one line, not of four) */
#define PR_THREADS 256
#define PR_PER 4
#define PR_TILE (PR_THREADS * PR_PER)
typedef u32 pr_u32x4 __attribute__((ext_vector_type(4)));         /* one 16-byte LDS read and global store */

struct PrArgs {
	const u64 *img;
	const u64 *off;            /* [n_sub + 1], off[0] = 0, off[n_sub] = n */
	u64 n;
	int n_sub, sub_lo, k, pre;
};

__device__ __forceinline__ int pr_sub(const u64 YK_GLOBAL *off, int n_sub, u64 i)   /* the last j < n_sub with off[j] <= i */
{
	int l = 0;
	for (int r = n_sub; r - l > 1; ) { const int m = (l + r) >> 1; if (off[m] <= i) l = m; else r = m; }
	return l;
}

__device__ __forceinline__ u32 pr_digits(u32 c) { return c < 10 ? 1u : c < 100 ? 2u : c < 1000 ? 3u : 4u; }

__global__ __launch_bounds__(PR_THREADS)
void k_kmers(PrArgs a, u64 *__restrict__ out_x, unsigned short *__restrict__ out_c)
{
	const u64 YK_GLOBAL *off = yk_global(u64, a.off);
	const u64 YK_GLOBAL *img = yk_global(u64, a.img);
	const u64 mask = (1ull << 2 * a.k) - 1;
	for (u64 i = (u64)blockIdx.x * PR_THREADS + threadIdx.x; i < a.n; i += (u64)gridDim.x * PR_THREADS) {
		const int j = pr_sub(off, a.n_sub, i);
		const u64 w = img[i + (u64)j + 1];
		out_x[i] = yk_hash64_inv((w >> 10) << a.pre | (u64)(a.sub_lo + j), mask);
		out_c[i] = (unsigned short)(w & 1023u);
	}
}

__global__ __launch_bounds__(PR_THREADS)
void k_print_sizes(PrArgs a, u32 *__restrict__ tile_bytes)
{
	__shared__ u32 s_w[PR_THREADS / WAVE];
	const u64 YK_GLOBAL *off = yk_global(u64, a.off);
	const u64 YK_GLOBAL *img = yk_global(u64, a.img);
	const u64 base = (u64)blockIdx.x * PR_TILE;
	u32 s = 0;
#pragma unroll
	for (int u = 0; u < PR_PER; ++u) {
		const u64 i = base + u * PR_THREADS + threadIdx.x;
		if (i >= a.n) continue;
		const int j = pr_sub(off, a.n_sub, i);
		s += (u32)a.k + 2 + pr_digits((u32)(img[i + (u64)j + 1] & 1023u));
	}
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
	if ((threadIdx.x & (WAVE - 1)) == 0) s_w[threadIdx.x / WAVE] = s;
	__syncthreads();
	if (threadIdx.x == 0) { u32 t = 0; for (int w = 0; w < PR_THREADS / WAVE; ++w) t += s_w[w]; tile_bytes[blockIdx.x] = t; }
}

template <bool CNT>
__global__ __launch_bounds__(PR_THREADS)
void k_print(PrArgs a, const u64 *__restrict__ tile_off, uint8_t *text)
{
	extern __shared__ pr_u32x4 s_pr[];                                /* the tile's bytes from byte `pad` on: 16 + PR_TILE * (longest line) */
	__shared__ u32 s_at[CNT ? PR_TILE : 1];                        /* with counts: a line's length, then its offset inside the tile */
	__shared__ u32 s_w[PR_THREADS / WAVE];
	uint8_t *s_txt = (uint8_t*)s_pr;
	const u64 YK_GLOBAL *off = yk_global(u64, a.off);
	const u64 YK_GLOBAL *img = yk_global(u64, a.img);
	const u64 base = (u64)blockIdx.x * PR_TILE;
	const u32 n_here = (u32)(a.n - base < PR_TILE ? a.n - base : PR_TILE), L = (u32)a.k + 1;
	const u64 mask = (1ull << 2 * a.k) - 1;
	const u64 byte0 = CNT ? tile_off[blockIdx.x] : base * L;
	const u32 n_bytes = CNT ? (u32)(tile_off[blockIdx.x + 1] - byte0) : n_here * L;
	uint8_t *dst = text + byte0;
	const u32 pad = (u32)((uintptr_t)dst & 15);
	u64 x[PR_PER];
	u32 c[PR_PER];
#pragma unroll
	for (int u = 0; u < PR_PER; ++u) {
		const u32 q = u * PR_THREADS + threadIdx.x;
		x[u] = 0; c[u] = 0;
		if (q < n_here) {
			const u64 i = base + q;
			const int j = pr_sub(off, a.n_sub, i);
			const u64 w = img[i + (u64)j + 1];
			x[u] = yk_hash64_inv((w >> 10) << a.pre | (u64)(a.sub_lo + j), mask);
			c[u] = (u32)(w & 1023u);
		}
		if (CNT) s_at[q] = q < n_here ? L + 1 + pr_digits(c[u]) : 0;
	}
	if (CNT) {                                                     /* exclusive scan of the line lengths in line order: four consecutive lines per lane */
		__syncthreads();
		const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
		u32 l4[PR_PER], s = 0;
#pragma unroll
		for (int u = 0; u < PR_PER; ++u) { l4[u] = s_at[threadIdx.x * PR_PER + u]; s += l4[u]; }
		u32 inc = s;
#pragma unroll
		for (int o = 1; o < WAVE; o <<= 1) { const u32 y = __shfl_up(inc, o); if (lane >= (u32)o) inc += y; }
		if (lane == WAVE - 1) s_w[wave] = inc;
		__syncthreads();
		u32 run = inc - s;
		for (u32 w = 0; w < wave; ++w) run += s_w[w];
#pragma unroll
		for (int u = 0; u < PR_PER; ++u) { s_at[threadIdx.x * PR_PER + u] = run; run += l4[u]; }
		__syncthreads();
	}
#pragma unroll
	for (int u = 0; u < PR_PER; ++u) {
		const u32 q = u * PR_THREADS + threadIdx.x;
		if (q >= n_here) continue;
		uint8_t *p = s_txt + pad + (CNT ? s_at[q] : q * L);
		for (int b = 0; b < a.k; ++b) p[b] = (uint8_t)(0x54474341u >> (((u32)(x[u] >> 2 * (a.k - 1 - b)) & 3u) << 3));   /* "ACGT"[x >> 2j & 3], main.c:309 */
		p += a.k;
		if (CNT) {
			*p++ = '\t';
			const u32 v = c[u], d = pr_digits(v);
			if (d > 3) *p++ = (uint8_t)('0' + v / 1000);
			if (d > 2) *p++ = (uint8_t)('0' + v / 100 % 10);
			if (d > 1) *p++ = (uint8_t)('0' + v / 10 % 10);
			*p++ = (uint8_t)('0' + v % 10);
		}
		*p = '\n';
	}
	__syncthreads();
	/* the span [dst, dst + n_bytes): `head` bytes up to the first address that is a multiple of 16, whole 16s, the rest */
	const u32 to_al = (16 - pad) & 15, head = to_al < n_bytes ? to_al : n_bytes, n16 = (n_bytes - head) >> 4, tail = n_bytes - head - (n16 << 4);
	uint8_t YK_GLOBAL *g = yk_global_rw(uint8_t, dst);
	if (threadIdx.x < head) g[threadIdx.x] = s_txt[pad + threadIdx.x];
	pr_u32x4 YK_GLOBAL *g16 = yk_global_rw(pr_u32x4, dst + head);
	const pr_u32x4 *s16 = s_pr + ((pad + head) >> 4);
	for (u32 v = threadIdx.x; v < n16; v += PR_THREADS) g16[v] = s16[v];
	if (threadIdx.x < tail) { const u32 at = head + (n16 << 4) + threadIdx.x; g[at] = s_txt[pad + at]; }
}

extern "C" {

u64 yk_print_tiles(u64 n) { return (n + PR_TILE - 1) / PR_TILE; }

static PrArgs pr_args(const u64 *img, const u64 *off, u64 n, int n_sub, int sub_lo, int k, int pre)
{
	PrArgs a;
	a.img = img; a.off = off; a.n = n; a.n_sub = n_sub; a.sub_lo = sub_lo; a.k = k; a.pre = pre;
	return a;
}

int yk_launch_kmers(const u64 *img, const u64 *off, u64 n, int n_sub, int sub_lo, int k, int pre, u64 *x, unsigned short *c, hipStream_t st)
{
	if (n == 0) return 0;
	const u64 grid = std::min<u64>((n + PR_THREADS - 1) / PR_THREADS, 1u << 20);
	YK_LAUNCH(k_kmers, dim3((unsigned)grid), dim3(PR_THREADS), 0, st, pr_args(img, off, n, n_sub, sub_lo, k, pre), x, c);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

int yk_launch_print_sizes(const u64 *img, const u64 *off, u64 n, int n_sub, int k, u32 *tile_bytes, hipStream_t st)
{
	if (n == 0) return 0;
	if (yk_print_tiles(n) >> 31) return -1;
	YK_LAUNCH(k_print_sizes, dim3((unsigned)yk_print_tiles(n)), dim3(PR_THREADS), 0, st, pr_args(img, off, n, n_sub, 0, k, 0), tile_bytes);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

int yk_launch_print(const u64 *img, const u64 *off, u64 n, int n_sub, int sub_lo, int k, int pre, int with_counts, const u64 *tile_off,
                    uint8_t *text, hipStream_t st)
{
	if (n == 0) return 0;
	if (k < 1 || k > 31 || (yk_print_tiles(n) >> 31)) return -1;
	const PrArgs a = pr_args(img, off, n, n_sub, sub_lo, k, pre);
	const size_t lds = (16 + (size_t)PR_TILE * (k + (with_counts ? 6 : 1)) + 15) & ~(size_t)15;   /* at most 37.9 KB (+ 4 KB of offsets with counts) */
	if (with_counts) YK_LAUNCH((k_print<true>), dim3((unsigned)yk_print_tiles(n)), dim3(PR_THREADS), lds, st, a, tile_off, text);
	else YK_LAUNCH((k_print<false>), dim3((unsigned)yk_print_tiles(n)), dim3(PR_THREADS), lds, st, a, tile_off, text);
	return hipGetLastError() == hipSuccess ? 0 : -1;
}

} /* extern "C" */
