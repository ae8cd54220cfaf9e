/* kern_inspect.inc -- part of kernels.hip (one translation unit, included in this order): the table join of `yak inspect`
 * (reference inspect.c:47-62).  Every stored key of table A, in dump order, adds one to J[c0][c1]: c0 = its count in A, c1 = max(0,
 * yak_ch_get()) of table B (0 without B).  The probe hash is rebuilt from the key and its sub-table i, (key >> 10) << pre_A | i, or --
 * InArgs.ref -- is the stored key itself, as inspect.c:58 calls yak_ch_get() with it. */

/* one launch: the keys of A's sub-tables [sub_lo, sub_lo + n_sub); those of sub-table sub_lo + j are keys[off[j] .. off[j + 1]), or with hdr
 * the .yak body (yk_ctx_dump_image_dev): each sub-table's {capacity, size} word in front of its keys, key i of it at keys[off[j] + j + 1 + i] */
struct InArgs {
	const u64 *keys;
	const u64 *off;            /* [n_sub + 1], off[0] = 0, off[n_sub] = n */
	u64 n;
	u64 *J;                    /* [1024 * 1024], row c0 */
	int n_sub, sub_lo, hdr, pre_a;
	int blo, bhi;              /* B's sub-tables this launch probes: a key whose probe lands elsewhere belongs to another shard of B */
	int ref;
	int tab_a, tab_b;          /* A's offsets / B's sub-table directory in LDS */
};

#define IN_THREADS 512
#define IN_U 4                     /* probes a lane keeps in flight */
#define IN_C 128                   /* the LDS corner: c0, c1 < IN_C */
#define IN_CORNER_BYTES (IN_C * IN_C * 4)

/* A persistent grid: workgroup b owns a contiguous run of keys, a step takes IN_THREADS * IN_U consecutive ones (lane t: t, t + IN_THREADS, ...),
 * so a lane's keys only move forward and its sub-table index only advances.  The probe is k_lookup's: the home slot from the LDS directory, then
 * the key array alone (the image keeps unused slots at YK_EMPTY).  LONG (k >= 32): a YAK_LOAD_ALL table can store a key equal to YK_EMPTY (a
 * 64-bit hash with (hash >> pre) << 10 all ones at count 1023), so there a YK_EMPTY slot asks the `used` bitmap, as img_find does.
 * The counts of the low corner go to the workgroup's LDS histogram (u32: a workgroup sees fewer than 2^32 keys), the rest to J by u64 atomics;
 * each workgroup adds its non-zero corner bins to J once at the end.  Integer sums: the result does not depend on the order of the atomics. */
template <bool HASB, bool LONG>
__global__ __launch_bounds__(IN_THREADS)
void k_inspect(InArgs a, ImgView img)
{
	extern __shared__ __attribute__((aligned(16))) u64 s_in[];
	u32 *s_hist = (u32*)s_in;
	u64 *s_dir = s_in + IN_CORNER_BYTES / 8;
	const u32 pmask = HASB ? (1u << img.pre) - 1 : 0;
	u64 *s_off = s_dir + (HASB && a.tab_b ? pmask + 1 : 0);
	for (u32 i = threadIdx.x; i < IN_C * IN_C; i += IN_THREADS) s_hist[i] = 0;
	if (HASB && a.tab_b)
		for (u32 p = threadIdx.x; p <= pmask; p += IN_THREADS) { const u32 b = img.bits[p]; s_dir[p] = img.off[p] | (u64)(b == YK_NOCAP ? 63u : b) << 58; }
	if (a.tab_a) for (int j = threadIdx.x; j < a.n_sub; j += IN_THREADS) s_off[j] = a.off[j];   /* off[n_sub] = n: 80 KiB at pre 10, two workgroups per CU */
	__syncthreads();
	const u64 YK_GLOBAL *goff = yk_global(u64, a.off);
	const u64 YK_GLOBAL *gkeys = yk_global(u64, a.keys);
	const u64 YK_GLOBAL *karena = yk_global(u64, img.keys);
	const u32 YK_GLOBAL *used = yk_global(u32, img.used);
	unsigned long long *J = (unsigned long long*)a.J;
#define IN_OFF(j) (a.tab_a ? ((j) < a.n_sub ? s_off[j] : a.n) : goff[j])
	const u64 per = (a.n + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < a.n ? lo + per : a.n;
	int si = 0;                                               /* the sub-table of key `lo`: the last j with off[j] <= lo */
	for (int l = 0, r = a.n_sub; r - l > 1; ) { const int m = (l + r) >> 1; if (IN_OFF(m) <= lo) { l = m; si = m; } else r = m; }
	for (u64 base = lo; base < hi; base += IN_THREADS * IN_U) {
		u64 kid[IN_U], kc[IN_U], aoff[IN_U];
		u32 idx[IN_U], nmask[IN_U], c0[IN_U], c1[IN_U];
		bool in[IN_U], live[IN_U];
#pragma unroll
		for (int u = 0; u < IN_U; ++u) {
			const u64 i = base + u * IN_THREADS + threadIdx.x;
			in[u] = i < hi; live[u] = false; c0[u] = 0; c1[u] = 0; kid[u] = 0; aoff[u] = 0; idx[u] = 0; nmask[u] = 0;
			if (!in[u]) continue;
			while (IN_OFF(si + 1) <= i) ++si;
			const u64 key = gkeys[i + (a.hdr ? (u64)si + 1 : 0)];
			c0[u] = (u32)(key & 1023u);
			if (!HASB) continue;
			const u64 h = a.ref ? key : (key >> 10) << a.pre_a | (u64)(a.sub_lo + si);
			const u32 p = (u32)h & pmask;
			if ((int)p < a.blo || (int)p >= a.bhi) { in[u] = false; continue; }
			kid[u] = (h >> img.pre) & (~0ull >> 10);           /* htab.c:97 keeps 54 bits of hash >> pre */
			u64 off; u32 bits;
			if (a.tab_b) { const u64 e = s_dir[p]; off = e & ((1ull << 58) - 1); bits = (u32)(e >> 58); bits = bits == 63u ? YK_NOCAP : bits; }
			else { bits = img.bits[p]; off = img.off[p]; }
			if (bits != YK_NOCAP) { live[u] = true; aoff[u] = off; nmask[u] = (1u << bits) - 1; idx[u] = yk_h2b((u32)kid[u], bits); }
		}
		if (HASB) {
#pragma unroll
			for (int u = 0; u < IN_U; ++u) kc[u] = live[u] ? karena[aoff[u] + idx[u]] : YK_EMPTY;
#pragma unroll
			for (int u = 0; u < IN_U; ++u) {
				if (!live[u]) continue;
				const u32 first = idx[u];
				for (;;) {
					if (kc[u] == YK_EMPTY) {
						if (!LONG) break;
						const u64 s = aoff[u] + idx[u];
						if (!(used[s >> 5] >> (s & 31) & 1)) break;
					}
					if (kc[u] >> 10 == kid[u]) { c1[u] = (u32)(kc[u] & 1023u); break; }
					idx[u] = (idx[u] + 1) & nmask[u];
					if (idx[u] == first) break;
					kc[u] = karena[aoff[u] + idx[u]];
				}
			}
		}
#pragma unroll
		for (int u = 0; u < IN_U; ++u) {
			if (!in[u]) continue;
			if (c0[u] < IN_C && c1[u] < IN_C) atomicAdd(&s_hist[c0[u] * IN_C + c1[u]], 1u);
			else atomicAdd(&J[(u64)c0[u] * 1024 + c1[u]], 1ull);
		}
	}
#undef IN_OFF
	__syncthreads();
	for (u32 i = threadIdx.x; i < IN_C * IN_C; i += IN_THREADS) {
		const u32 v = s_hist[i];
		if (v) atomicAdd(&J[(u64)(i / IN_C) * 1024 + i % IN_C], (unsigned long long)v);
	}
}
