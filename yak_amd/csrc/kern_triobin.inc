/* kern_triobin.inc -- part of kernels.hip (one translation unit, after kern_extract.inc): the device half of `yak triobin` (reference triobin.c:41-101) */
/* ------------------------------------------------------------------------------------------
 * flag lookup: out[i] = max(0, yak_ch_get()) of the k-mer ENDING at byte i of a base image, TB_NOKMER
 * where none ends (window shorter than k or holding a non-ACGT byte); triobin.c:62-84.  The table comes
 * from the two YAK_LOAD_TRIOBIN loads, which OR a 2-bit class per parent into the count field, so a flag
 * is 4 bits and the output one byte per position.
 *
 * The probe is k_lookup's (kern_extract.inc): sub-table table in LDS, TB_U home slots requested
 * together, the key array alone.  That the key array alone suffices holds for k >= 32 too, for a
 * different reason than in qv: a 64-bit hash can make (hash >> pre) << 10 all ones, but a TRIOBIN load
 * stores a count field of at most 15, never 1023, so no stored key equals YK_EMPTY.  A count field
 * above 15 means the table did not come from those loads (the reference would index past its c[16]):
 * the lookup raises d_tb_over and its caller fails.
 * ------------------------------------------------------------------------------------------ */
#define TB_NOKMER 0xffu
#define TB_U 2                     /* probes a lane keeps in flight (k_lookup's measured best) */
__device__ u32 d_tb_over;          /* a probed count field above 15 was met */

template <bool LONG>               /* LONG: k in [32, 63], yak_hash_long (triobin.c:78-81) */
__global__ __launch_bounds__(XT_THREADS)
void k_tb_lookup(const uint8_t *__restrict__ bases, int64_t n, int k, ImgView img, uint8_t *__restrict__ out, int tab)
{
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
		for (int r0 = 0; r0 < XT_ROUNDS; r0 += TB_U) {
			u64 kid[TB_U], kc[TB_U];
			const u64 YK_GLOBAL *keys[TB_U];
			u32 idx[TB_U], nmask[TB_U], v[TB_U];
			bool live[TB_U];
#pragma unroll
			for (int u = 0; u < TB_U; ++u) {
				const int q = (r0 + u) * XT_THREADS + (int)threadIdx.x;
				u64 h;
				const bool ok = LONG ? xt_kmer_long(S, q, k, img.pre, tile0, n, &h) : xt_kmer(S, q, k, mask, kones, tile0, n, &h);
				const u32 p = (u32)h & pmask;
				v[u] = ok ? 0u : TB_NOKMER;
				/* htab.c:93-100 compares (hash >> pre) << 10 >> 10: the stored key keeps 54 bits of it */
				live[u] = false; kid[u] = (h >> img.pre) & (~0ull >> 10); keys[u] = karena; idx[u] = 0; nmask[u] = 0;
				if (ok) {
					u64 off; u32 bits;
					if (tab) { const u64 e = s_tab[p]; off = e & ((1ull << 58) - 1); bits = (u32)(e >> 58); bits = bits == 63u ? YK_NOCAP : bits; }
					else { bits = img.bits[p]; off = img.off[p]; }
					if (bits != YK_NOCAP) { live[u] = true; keys[u] = karena + off; nmask[u] = (1u << bits) - 1; idx[u] = yk_h2b((u32)kid[u], bits); }
				}
			}
#pragma unroll
			for (int u = 0; u < TB_U; ++u) kc[u] = live[u] ? keys[u][idx[u]] : YK_EMPTY;
#pragma unroll
			for (int u = 0; u < TB_U; ++u) {
				const u32 first = idx[u];
				while (kc[u] != YK_EMPTY) {
					if (kc[u] >> 10 == kid[u]) { v[u] = (u32)(kc[u] & 1023u); break; }
					idx[u] = (idx[u] + 1) & nmask[u];
					if (idx[u] == first) break;
					kc[u] = keys[u][idx[u]];
				}
				if (v[u] != TB_NOKMER && v[u] > 15u) { over = 1; v[u] &= 15u; }
				const int64_t pos = tile0 + (r0 + u) * XT_THREADS + (int)threadIdx.x;
				if (pos < n) out[pos] = (uint8_t)v[u];
			}
		}
		__syncthreads();
	}
	if (over) d_tb_over = 1;
}

/* ------------------------------------------------------------------------------------------
 * per-read reduction (triobin.c:74-100): one wave per read, 64 positions per step.
 *   c[16]  histogram of the flags over the positions that have a k-mer; nk = their number
 *   sc[2]  a position's type is 1 where flag == 2 (pat solid, mat absent), 2 where flag == 8, 0
 *          elsewhere (also where no k-mer ends); every maximal run of one type t > 0 and length
 *          >= k - 4 adds its length to sc[t - 1]
 * The run open at a step's start is carried as (start, type); the step's run starts are a ballot,
 * walked bit by bit with scalar ops.  A run of type 0 "opens" at position 0: it adds nothing, and a
 * read that starts with a typed position closes it at once.
 * Output per read: 19 int32 = c[0..15], sc[0], sc[1], nk.
 * ------------------------------------------------------------------------------------------ */
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

void yk_launch_tb_lookup(const uint8_t *bases, int64_t n, int k, ImgView img, uint8_t *out, hipStream_t st)
{
	if (n <= 0) return;
	void *over = 0;
	if (hipGetSymbolAddress(&over, HIP_SYMBOL(d_tb_over)) == hipSuccess) (void)hipMemsetAsync(over, 0, 4, st);
	const int tab = img.pre <= 12;
	const size_t lds = tab ? (size_t)8 << img.pre : 0;
	if (k < 32) hipLaunchKernelGGL((k_tb_lookup<false>), dim3(yk_xpart_blocks(n)), dim3(XT_THREADS), lds, st, bases, n, k, img, out, tab);
	else hipLaunchKernelGGL((k_tb_lookup<true>), dim3(yk_xpart_blocks(n)), dim3(XT_THREADS), lds, st, bases, n, k, img, out, tab);
}

int yk_tb_over_seen(hipStream_t st)
{
	u32 v = 0;
	(void)hipStreamSynchronize(st);
	(void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(d_tb_over), 4);
	return (int)v;
}

void yk_launch_tb_reduce(const uint8_t *flag, const u64 *roff, const u32 *rlen, int64_t n_reads, int k, int *cnt, hipStream_t st)
{
	if (n_reads <= 0) return;
	const int64_t want = (n_reads + 3) / 4;
	hipLaunchKernelGGL(k_tb_reduce, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, st, flag, roff, rlen, n_reads, k, cnt);
}
