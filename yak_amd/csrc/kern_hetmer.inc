/* kern_hetmer.inc -- part of kernels.hip (one translation unit, included in this order): the het-mer pairs of `yak-amd hetmers` (not in the
 * reference; DESIGN.md section 17), a self-join of a count table with its own middle-base neighbours.  The input is the .yak body of sub-tables
 * [sub_lo, sub_lo + n_sub) as yk_ctx_dump_image_dev() lays it out, with the key offsets of kern_print.inc: key i of the range belongs to sub-table
 * j = the last one with off[j] <= i and lies at img[i + j + 1].  Its k-mer is x = yk_hash64_inv((word >> 10) << pre | (sub_lo + j), 4^k - 1), the
 * canonical one (k odd, below 32), its count c = word & 1023; a key with c < min_cnt is absent, as a member and as a partner.  For d = 1, 2, 3 the
 * variant y' = x ^ d << (k - 1) differs from x in the middle base alone, y = min(y', revcomp_k(y')) is its canonical form, and the partners of x
 * are the distinct y != x stored with a count of at least min_cnt: three probes of the whole resident image, k_lookup's probe.  x and its partners
 * are a group of 1 to 4 members; the member smaller than all its partners reports it, and a group of two is a pair {x < y}.
 *   k_hetmer<HM_TALLY>   n_group[size] += 1 per group, J[min(cx, cy)][max(cx, cy)] += 1 per pair
 *   k_hetmer<HM_COUNT>   tile_cnt[t] = pairs reported in tile t (HM_THREADS consecutive keys); scanned by k_te_scan
 *   k_hetmer<HM_WRITE>   the records {x, y, cx, cy} of tile t from list[tile_off[t]] on, in key order: the listing order of x */
#define HM_THREADS 512
#define HM_C 128                   /* the LDS corner of J: lo, hi < HM_C */
#define HM_CORNER_BYTES (HM_C * HM_C * 4)
enum { HM_TALLY = 0, HM_COUNT = 1, HM_WRITE = 2 };

struct HmArgs {
	const u64 *img;
	const u64 *off;            /* [n_sub + 1], off[0] = 0, off[n_sub] = n */
	u64 n;
	u64 *J;                    /* TALLY: [1024 * 1024], row lo */
	u64 *group;                /* TALLY: [5], [s] = groups of s members */
	u32 *tile_cnt;             /* COUNT: [tiles] */
	const u64 *tile_off;       /* WRITE: [tiles + 1] */
	u64 *list;                 /* WRITE: three words per record: x, y, cx | cy << 32 */
	int n_sub, sub_lo, k, min_cnt;
	int tab;                   /* the table's sub-table directory in LDS (pre <= 12) */
	int tab_off;               /* the range's key offsets in LDS (n_sub <= 4096) */
};

/* the reverse complement of a k-mer in 2 bits per base, first base highest: the 32 2-bit fields of the word reversed (swaps of 2, 4 and 8 bits, then
 * of the bytes), complemented (3 - c == c ^ 3) and moved down to the low 2k bits; the zero fields above the k-mer become the ones that are shifted out */
__device__ __forceinline__ u64 hm_revcomp(u64 x, int k)
{
	x = (x >> 2 & 0x3333333333333333ull) | (x & 0x3333333333333333ull) << 2;
	x = (x >> 4 & 0x0f0f0f0f0f0f0f0full) | (x & 0x0f0f0f0f0f0f0f0full) << 4;
	return ~__builtin_bswap64(x) >> (64 - 2 * k);
}

/* A persistent grid, as k_inspect: workgroup b owns a contiguous run of whole tiles, a step takes one tile, lane t its key t, so a lane's keys
 * only move forward and its sub-table index only advances.  One key per lane and step: its three probes are requested together and only then
 * waited for -- three in flight per lane, between k_lookup's two and k_inspect's four.  The probe reads the key array alone: the image keeps
 * unused slots at YK_EMPTY, which no 2k < 64-bit key equals, so the `used` bitmap is not read.
 * TALLY: the pairs of the low corner go to the workgroup's LDS histogram (u32: a workgroup sees fewer than 2^32 keys), the rest to J by u64
 * atomics; the group sizes are counted per lane and added once per wave at the end.  Integer sums: no result depends on the order of the atomics.
 * COUNT / WRITE: a reporting key's rank in its tile is the number of reporting keys before it -- a ballot per wave and the waves' sums in LDS. */
template <int MODE>
__global__ __launch_bounds__(HM_THREADS)
void k_hetmer(HmArgs a, ImgView img)
{
	extern __shared__ __attribute__((aligned(16))) u64 s_hm[];
	__shared__ u32 s_w[HM_THREADS / WAVE];
	u32 *s_hist = (u32*)s_hm;
	u64 *s_dir = s_hm + (MODE == HM_TALLY ? HM_CORNER_BYTES / 8 : 0);
	const u32 pmask = (1u << img.pre) - 1;
	u64 *s_off = s_dir + (a.tab ? pmask + 1 : 0);
	if (MODE == HM_TALLY) for (u32 i = threadIdx.x; i < HM_C * HM_C; i += HM_THREADS) s_hist[i] = 0;
	if (a.tab) for (u32 p = threadIdx.x; p <= pmask; p += HM_THREADS) { const u32 b = img.bits[p]; s_dir[p] = img.off[p] | (u64)(b == YK_NOCAP ? 63u : b) << 58; }
	if (a.tab_off) for (int j = threadIdx.x; j < a.n_sub; j += HM_THREADS) s_off[j] = a.off[j];   /* off[n_sub] = n */
	__syncthreads();
	const u64 YK_GLOBAL *goff = yk_global(u64, a.off);
	const u64 YK_GLOBAL *gimg = yk_global(u64, a.img);
	const u64 YK_GLOBAL *karena = yk_global(u64, img.keys);
	unsigned long long *J = (unsigned long long*)a.J;
#define HM_OFF(j) (a.tab_off ? ((j) < a.n_sub ? s_off[j] : a.n) : goff[j])
	const u64 tiles = (a.n + HM_THREADS - 1) / HM_THREADS, per = (tiles + gridDim.x - 1) / gridDim.x * HM_THREADS;
	const u64 lo = per * blockIdx.x, hi = lo + per < a.n ? lo + per : a.n;
	const u64 mask = (1ull << 2 * a.k) - 1;
	const int mid = a.k - 1;                                      /* the middle base sits at bits [k - 1, k + 1) */
	const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
	u32 g1 = 0, g2 = 0, g3 = 0, g4 = 0;
	int si = 0;                                                   /* the sub-table of key `lo`: the last j with off[j] <= lo */
	for (int l = 0, r = a.n_sub; r - l > 1; ) { const int m = (l + r) >> 1; if (HM_OFF(m) <= lo) { l = m; si = m; } else r = m; }
	for (u64 base = lo; base < hi; base += HM_THREADS) {
		const u64 i = base + threadIdx.x;
		u64 x = 0, y[3], kid[3], kc[3], aoff[3];
		u32 idx[3], nmask[3], cy[3], cx = 0;
		bool live[3], member = false;
#pragma unroll
		for (int d = 0; d < 3; ++d) { live[d] = false; y[d] = 0; kid[d] = 0; aoff[d] = 0; idx[d] = 0; nmask[d] = 0; cy[d] = 0; }
		if (i < hi) {
			while (HM_OFF(si + 1) <= i) ++si;
			const u64 w = gimg[i + (u64)si + 1];
			cx = (u32)(w & 1023u);
			member = cx >= (u32)a.min_cnt;
			if (member) {
				x = yk_hash64_inv((w >> 10) << img.pre | (u64)(a.sub_lo + si), mask);
#pragma unroll
				for (int d = 0; d < 3; ++d) {
					const u64 v = x ^ (u64)(d + 1) << mid, rc = hm_revcomp(v, a.k);
					y[d] = v < rc ? v : rc;
				}
				/* palindromic flanks: one variant is x itself in the other orientation, the other two are one k-mer */
				live[0] = y[0] != x;
				live[1] = y[1] != x && y[1] != y[0];
				live[2] = y[2] != x && y[2] != y[0] && y[2] != y[1];
#pragma unroll
				for (int d = 0; d < 3; ++d) {
					if (!live[d]) continue;
					const u64 h = yk_hash64(y[d], mask);
					const u32 p = (u32)h & pmask;
					kid[d] = h >> img.pre;
					u64 off; u32 bits;
					if (a.tab) { const u64 e = s_dir[p]; off = e & ((1ull << 58) - 1); bits = (u32)(e >> 58); bits = bits == 63u ? YK_NOCAP : bits; }
					else { bits = img.bits[p]; off = img.off[p]; }
					live[d] = bits != YK_NOCAP;
					if (live[d]) { aoff[d] = off; nmask[d] = (1u << bits) - 1; idx[d] = yk_h2b((u32)kid[d], bits); }
				}
			}
		}
#pragma unroll
		for (int d = 0; d < 3; ++d) kc[d] = live[d] ? karena[aoff[d] + idx[d]] : YK_EMPTY;
		u32 n_part = 0, c_part = 0;
		u64 y_min = ~0ull;
#pragma unroll
		for (int d = 0; d < 3; ++d) {
			if (!live[d]) continue;
			const u32 first = idx[d];
			while (kc[d] != YK_EMPTY) {
				if (kc[d] >> 10 == kid[d]) { cy[d] = (u32)(kc[d] & 1023u); break; }
				idx[d] = (idx[d] + 1) & nmask[d];
				if (idx[d] == first) break;
				kc[d] = karena[aoff[d] + idx[d]];
			}
			if (cy[d] >= (u32)a.min_cnt) { ++n_part; c_part = cy[d]; y_min = y[d] < y_min ? y[d] : y_min; }
		}
		const bool reports = member && x < y_min;                 /* the group's smallest member (y_min = ~0 without a partner) */
		const bool pair = reports && n_part == 1;
		if (MODE == HM_TALLY) {
			if (reports) { g1 += n_part == 0; g2 += n_part == 1; g3 += n_part == 2; g4 += n_part == 3; }
			if (pair) {
				const u32 c_lo = cx < c_part ? cx : c_part, c_hi = cx < c_part ? c_part : cx;
				if (c_hi < HM_C) atomicAdd(&s_hist[c_lo * HM_C + c_hi], 1u);
				else atomicAdd(&J[(u64)c_lo * 1024 + c_hi], 1ull);
			}
		} else {
			const u64 b = __ballot(pair);
			if (lane == 0) s_w[wave] = (u32)__popcll(b);
			__syncthreads();
			const u64 tile = base / HM_THREADS;
			if (MODE == HM_COUNT) {
				if (threadIdx.x == 0) { u32 t = 0; for (u32 v = 0; v < HM_THREADS / WAVE; ++v) t += s_w[v]; a.tile_cnt[tile] = t; }
			} else if (pair) {
				u64 at = a.tile_off[tile] + (u64)__popcll(b & ((1ull << lane) - 1));
				for (u32 v = 0; v < wave; ++v) at += s_w[v];
				u64 YK_GLOBAL *rec = yk_global_rw(u64, a.list) + at * 3;
				rec[0] = x; rec[1] = y_min; rec[2] = (u64)cx | (u64)c_part << 32;
			}
			__syncthreads();                                          /* s_w is written again in the next step */
		}
	}
#undef HM_OFF
	if (MODE == HM_TALLY) {
		unsigned long long *G = (unsigned long long*)a.group;
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) { g1 += __shfl_xor(g1, o); g2 += __shfl_xor(g2, o); g3 += __shfl_xor(g3, o); g4 += __shfl_xor(g4, o); }
		if (lane == 0) {
			if (g1) atomicAdd(&G[1], (unsigned long long)g1);
			if (g2) atomicAdd(&G[2], (unsigned long long)g2);
			if (g3) atomicAdd(&G[3], (unsigned long long)g3);
			if (g4) atomicAdd(&G[4], (unsigned long long)g4);
		}
		__syncthreads();
		for (u32 i = threadIdx.x; i < HM_C * HM_C; i += HM_THREADS) {
			const u32 v = s_hist[i];
			if (v) atomicAdd(&J[(u64)(i / HM_C) * 1024 + i % HM_C], (unsigned long long)v);
		}
	}
}
