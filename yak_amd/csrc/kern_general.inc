/* kern_general.inc -- part of kernels.hip (one translation unit, included in this order): the general path (accumulator table + device atomics: pre > 13, out-of-order feeds), operations on the table image, the order-exact bloom gate K2, selection */
/* ------------------------------------------------------------------------------------------
 * accumulator table (our own layout: one 32-B slot per distinct k-mer, linear probing).
 * Slot index = prefix-major: the high bits select the sub-table region so that a later
 * prefix-partitioned pass touches one contiguous region per sub-table.
 * ------------------------------------------------------------------------------------------ */
__device__ __forceinline__ u64 acc_home(const AccTab &t, u64 key)
{
	const int rb = t.bits - t.pre;
	const u64 p = key & ((1ull << t.pre) - 1);
	const u64 r = ((key >> t.pre) * 0x9E3779B97F4A7C15ull) >> (64 - rb);
	return p << rb | r;
}

/* find-or-claim; returns the slot, *created = 1 if this call claimed it */
__device__ __forceinline__ AccSlot *acc_claim(const AccTab &t, u64 key, bool *created)
{
	u64 i = acc_home(t, key);
	*created = false;
	for (;;) {
		AccSlot *s = t.s + i;
		u64 cur = s->key;
		if (cur == key) return s;
		if (cur == YK_EMPTY) {
			cur = atomicCAS(&s->key, YK_EMPTY, key);
			if (cur == YK_EMPTY) { *created = true; return s; }
			if (cur == key) return s;
		}
		i = (i + 1) & t.mask;
	}
}

__device__ __forceinline__ AccSlot *acc_find(const AccTab &t, u64 key)
{
	u64 i = acc_home(t, key);
	for (;;) {
		AccSlot *s = t.s + i;
		const u64 cur = s->key;
		if (cur == key) return s;
		if (cur == YK_EMPTY) return 0;
		i = (i + 1) & t.mask;
	}
}

__global__ __launch_bounds__(256)
void k_acc_init(AccSlot *s, u64 n)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		ulonglong2 *q = (ulonglong2*)(s + i);
		q[0] = make_ulonglong2(YK_EMPTY, YK_TINF);
		q[1] = make_ulonglong2(YK_TINF, 0ull);
	}
}

/* K3: every k-mer instance -> accumulator.  Per instance: one 32-B slot read, a CAS only for a new
 * key, atomicMin on t1/t2 only when the instance can still lower them (both only ever decrease,
 * so a stale read errs on the safe side), one fire-and-forget count increment. */
__global__ __launch_bounds__(256)
void k_acc_insert(const Rec *__restrict__ rec, int64_t n, u64 t0,
                  AccTab tab, ImgView img, int img_nonempty, int bloom_mode, u64 *newlist, u64 *counters)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const int lane = threadIdx.x & 63;
	u32 n_exist = 0;
	for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
		const int64_t i = i0 + threadIdx.x;
		bool created = false;
		AccSlot *s = 0;
		if (i < n) {
			const Rec rc = rec[i];
			const u64 key = rc.x, t = t0 + (u32)rc.y;
			int64_t hit = -1;
			if (img_nonempty) hit = img_find(img, key);
			if (hit >= 0) {
				atomicAdd(&img.delta[hit], 1u);       /* a put-call on an existing key: count only */
				++n_exist;
			} else {
				s = acc_claim(tab, key, &created);
				const ulonglong2 tt = *(const ulonglong2*)&s->t1;      /* {t1, t2}, possibly stale-high */
				const u32 c = s->cnt;
				if (c < 4096u) atomicAdd(&s->cnt, 1u);        /* only min(cnt, 1023[+1]) is ever used */
				if (bloom_mode) {
					u64 loser = t;
					if (t < tt.x) {
						const u64 old = atomicMin(&s->t1, t);
						loser = old < t ? t : old;            /* the larger of the two leaves t1 */
					}
					if (loser != YK_TINF && loser < tt.y) atomicMin(&s->t2, loser);
				} else if (t < tt.x) atomicMin(&s->t1, t);
			}
		}
		const u64 b = __ballot(created);
		if (b) {
			u64 base = 0;
			const int leader = __ffsll((long long)b) - 1;
			if (lane == leader) base = atomicAdd(&counters[YKC_NEW], (u64)__popcll(b));
			base = __shfl(base, leader);
			if (created && newlist) newlist[base + __popcll(b & lanemask_lt())] = (u64)(s - tab.s);
		}
	}
	if (img_nonempty) {
		for (int o = 32; o; o >>= 1) n_exist += __shfl_down(n_exist, o);
		if (lane == 0 && n_exist) atomicAdd(&counters[YKC_EXIST], (u64)n_exist);
	}
}

__global__ __launch_bounds__(256)
void k_acc_rehash(AccTab oldt, AccTab newt)
{
	const u64 n = oldt.mask + 1, stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		const AccSlot o = oldt.s[i];
		if (o.key == YK_EMPTY) continue;
		bool created;
		AccSlot *s = acc_claim(newt, o.key, &created);
		s->t1 = o.t1; s->t2 = o.t2; s->cnt = o.cnt; s->flags = o.flags;
	}
}

/* K4: create_new == 0 (reference htab.c:71-75): look the key up in the existing table image and
 * count the hit; the saturating fold into the 10 count bits happens once at the end of the pass */
__global__ __launch_bounds__(256)
void k_img_count(const Rec *__restrict__ rec, int64_t n, ImgView img)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		const int64_t hit = img_find(img, rec[i].x);
		if (hit >= 0) atomicAdd(&img.delta[hit], 1u);
	}
}

/* K4 with exclusive ownership (records grouped by sub-table prefix): ONE workgroup counts all
 * instances of one sub-table.  The sub-table's `used` bitmap and a per-word rank table live in LDS,
 * so a hit is turned into the rank of its slot among the used slots and counted in a 16-bit LDS
 * counter -- no global atomics; only the key compare reads HBM/L2.  The counters are flushed into
 * the per-slot delta array with plain read-modify-writes (nobody else touches this sub-table). */
template <int W>   /* record width in u64 words: 2 = {hash, position}, 1 = hash only */
__global__ __launch_bounds__(1024)
void k_img_count_lds(const u64 *__restrict__ rec, const u64 *__restrict__ bstart, ImgView img, int plo, u64 *__restrict__ compact, u32 stride)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	__shared__ u32 s_wsum[16];
	const u32 p = (u32)plo + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const u32 bits = img.bits[p];
	const u64 lo = bstart[p], hi = bstart[p + 1];
	if (bits == YK_NOCAP || lo == hi) return;
	const u32 cap = 1u << bits, nw = (cap + 31) / 32;
	const u64 off = img.off[p];
	u32 *s_bm = s_dyn, *s_rk = s_dyn + nw, *s_ct = s_dyn + 2 * nw;      /* bitmap | rank of each word's first slot | 16-bit counters */
	/* bitmap + exclusive popcount scan (every thread owns a contiguous run of words) */
	const u32 per = (nw + 1023) / 1024;
	u32 mine = 0;
	for (u32 j = 0; j < per; ++j) {
		const u32 w = tid * per + j;
		if (w < nw) { const u32 x = img.used[(off >> 5) + w]; s_bm[w] = x; mine += __popc(x); }
	}
	u32 incl = mine;
	for (int o = 1; o < 64; o <<= 1) { const u32 t = __shfl_up(incl, o); if (lane >= (u32)o) incl += t; }
	if (lane == 63) s_wsum[wave] = incl;
	__syncthreads();
	u32 base = incl - mine;
	for (u32 w2 = 0; w2 < wave; ++w2) base += s_wsum[w2];
	u32 total = 0;
	for (u32 w2 = 0; w2 < 16; ++w2) total += s_wsum[w2];
	for (u32 j = 0; j < per; ++j) {
		const u32 w = tid * per + j;
		if (w < nw) { s_rk[w] = base; base += __popc(s_bm[w]); }
	}
	for (u32 i = tid; i < (total + 1) / 2; i += 1024) s_ct[i] = 0;
	/* the keys of the used slots, packed in rank order: the random key reads of the probe loop then
	 * fall into count x 8 bytes instead of capacity x 8 -- 2.5x denser, so far more of the 256
	 * sub-tables in flight stay in the 256 MB Infinity Cache */
	u64 *ck = compact + (size_t)blockIdx.x * stride;
	{
		u32 r = incl - mine;
		for (u32 w2 = 0; w2 < wave; ++w2) r += s_wsum[w2];
		for (u32 j = 0; j < per; ++j) {
			const u32 w = tid * per + j;
			if (w >= nw) break;
			u32 x = s_bm[w];
			while (x) { const u32 b = __ffs((int)x) - 1; x &= x - 1; ck[r++] = img.keys[off + w * 32 + b]; }
		}
	}
	__syncthreads();
	const u32 nmask = cap - 1;
	for (u64 i = lo + tid; i < hi; i += 1024) {
		const u64 kid = __builtin_nontemporal_load(&rec[W * i]) >> img.pre;   /* streamed once: keep it out of the caches the keys live in */
		u32 s = yk_h2b((u32)kid, bits);
		const u32 first = s;
		for (;;) {
			const u32 word = s_bm[s >> 5];
			if (!(word >> (s & 31) & 1)) break;                           /* khashl get: stop at the first unused slot */
			const u32 r = s_rk[s >> 5] + __popc(word & ((1u << (s & 31)) - 1));
			if (ck[r] >> 10 == kid) {
				const u32 sh = 16 * (r & 1);
				if ((s_ct[r >> 1] >> sh & 0xffffu) < 4096u) atomicAdd(&s_ct[r >> 1], 1u << sh);   /* only min(count, 1023) matters */
				break;
			}
			s = (s + 1) & nmask;
			if (s == first) break;
		}
	}
	__syncthreads();
	for (u32 j = 0; j < per; ++j) {
		const u32 w = tid * per + j;
		if (w >= nw) break;
		u32 x = s_bm[w], r = s_rk[w];
		while (x) {
			const u32 b = __ffs((int)x) - 1;
			x &= x - 1;
			const u32 c = s_ct[r >> 1] >> (16 * (r & 1)) & 0xffffu;
			if (c) img.delta[off + w * 32 + b] += c;
			++r;
		}
	}
}

/* same on bare hash values (pass 2 of the sharded path ships 8 bytes per instance) */
__global__ __launch_bounds__(256)
void k_img_count_h(const u64 *__restrict__ hash, int64_t n, ImgView img)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		const int64_t hit = img_find(img, hash[i]);
		if (hit >= 0) atomicAdd(&img.delta[hit], 1u);
	}
}

/* reference htab.c:80-91 (yak_ch_inc): one key, saturating ++; out[0] = arena slot or ~0, out[1] = new count */
__global__ void k_img_inc(ImgView img, u64 hash, u64 *out)
{
	const int64_t a = img_find(img, hash);
	if (a < 0) { out[0] = ~0ull; out[1] = 0; return; }
	u64 kc = img.keys[a];
	if ((kc & 1023) < 1023) img.keys[a] = ++kc;
	out[0] = (u64)a; out[1] = kc & 1023;
}

__global__ __launch_bounds__(256)
void k_img_fold(ImgView img, u64 n_slots)                    /* htab.c:68-69,73-74: saturate at 1023 */
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
		const u32 d = img.delta[i];
		if (d) {
			const u64 kc = img.keys[i];
			const u64 c = (kc & 1023) + d;
			img.keys[i] = (kc & ~1023ull) | (c > 1023 ? 1023 : c);
			img.delta[i] = 0;
		}
	}
}

/* reference htab.c:145-169 (histogram of counts over all stored k-mers) and htab.c:219-235 (setcnt) */
__global__ __launch_bounds__(256)
void k_img_hist(ImgView img, u64 n_slots, unsigned long long *hist)
{
	__shared__ u32 s_h[1024];
	for (u32 i = threadIdx.x; i < 1024; i += 256) s_h[i] = 0;
	__syncthreads();
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride)
		if (img.used[i >> 5] >> (i & 31) & 1) atomicAdd(&s_h[img.keys[i] & 1023u], 1u);
	__syncthreads();
	for (u32 i = threadIdx.x; i < 1024; i += 256) if (s_h[i]) atomicAdd(&hist[i], (unsigned long long)s_h[i]);
}

__global__ __launch_bounds__(256)
void k_img_setcnt(ImgView img, u64 n_slots, u32 cnt)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride)
		if (img.used[i >> 5] >> (i & 31) & 1) img.keys[i] = (img.keys[i] & ~1023ull) | cnt;
}

/* bump: instead of 0 the count of a stored key becomes min(count + 1, 1023) -- the clear and the count pass over the input of the pass before in
 * one sweep (engine_pass.cpp yakamd_count_retained: that pass counts every instance, the pass before counted all but the first) */
__global__ __launch_bounds__(256)
void k_img_clear(ImgView img, u64 n_slots, int bump)         /* reference htab.c:116-125 */
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride)
		if (img.used[i >> 5] >> (i & 31) & 1) {
			const u64 kc = img.keys[i];
			img.keys[i] = !bump ? kc & ~1023ull : (kc & 1023) < 1023 ? kc + 1 : kc;
		}
}

/* yakamd_ch_sum, second step: entry i of a listing of ANOTHER table's keys -- hash[i] the key's full hash, cnt[i] its count c1 >= 1 there -- is
 * looked up in the image, where the create pass before (the one yak_ch_merge runs) has put every listed key and added one to its count; the count
 * field becomes min(1023, cur + c1 - 1): c1 for a key that pass created, old + c1 for one it found, and 1023 stays 1023.
 * The keys of a table are distinct, so a slot has at most one writer: a plain 8-byte load and store, no atomics, no delta array, no fold.  A lane
 * that probes past a slot another lane is rewriting reads the old or the new word; the two differ in the count field alone, which no compare
 * looks at (LONG: a word that turns into YK_EMPTY asks the bitmap, which says used).
 * The probe is k_lookup's: the sub-tables' {offset, log2 capacity} in LDS while pre <= 12 (`tab`), AC_U entries of a lane hashed first and their
 * home slots requested together, then one dependent global read per step.  The listing is read coalesced (entry base + u * AC_THREADS + lane)
 * and is grouped by sub-table, so a wave's probes fall into one or two sub-tables.  LONG (k >= 32): a YAK_LOAD_ALL key at count 1023 can equal
 * YK_EMPTY, so there a YK_EMPTY slot asks the `used` bitmap before the probe stops, as img_find and k_lookup<., true, true> do.
 * Entries of sub-tables outside [plo, phi) belong to another shard of the image's table and are skipped, as the feed of the create pass skipped
 * them.  A listed key of the range that is NOT found -- there is none after that pass -- raises *missing: the caller fails, the sum is never
 * silently short. */
#define AC_THREADS 256
#define AC_U 2                             /* probes a lane keeps in flight */
template <bool LONG>
__global__ __launch_bounds__(AC_THREADS)
void k_img_add_counts(const u64 *__restrict__ hash, const unsigned short *__restrict__ cnt, u64 n, ImgView img, int plo, int phi, int tab, u32 *missing)
{
	extern __shared__ __attribute__((aligned(16))) u64 s_ac[];
	const u32 pmask = (1u << img.pre) - 1;
	if (tab) {
		for (u32 p = threadIdx.x; p <= pmask; p += AC_THREADS) { const u32 b = img.bits[p]; s_ac[p] = img.off[p] | (u64)(b == YK_NOCAP ? 63u : b) << 58; }
		__syncthreads();
	}
	const u64 YK_GLOBAL *ghash = yk_global(u64, hash);
	const unsigned short YK_GLOBAL *gcnt = yk_global(unsigned short, cnt);
	u64 YK_GLOBAL *karena = yk_global_rw(u64, img.keys);
	bool miss = false;
	const u64 step = (u64)gridDim.x * AC_THREADS * AC_U;
	for (u64 base = (u64)blockIdx.x * AC_THREADS * AC_U; base < n; base += step) {
		u64 kid[AC_U], kc[AC_U], slot[AC_U];
		u32 idx[AC_U], nmask[AC_U], c1[AC_U];
		bool live[AC_U];
#pragma unroll
		for (int u = 0; u < AC_U; ++u) {
			const u64 i = base + (u64)u * AC_THREADS + threadIdx.x;
			live[u] = false; kid[u] = 0; slot[u] = 0; idx[u] = 0; nmask[u] = 0; c1[u] = 0;
			if (i >= n) continue;
			const u64 h = ghash[i];
			c1[u] = gcnt[i];
			const u32 p = (u32)h & pmask;
			if ((int)p < plo || (int)p >= phi || c1[u] == 0) continue;
			kid[u] = (h >> img.pre) & (~0ull >> 10);               /* the stored key keeps 54 bits of hash >> pre (htab.c:97) */
			u64 off; u32 bits;
			if (tab) { const u64 e = s_ac[p]; off = e & ((1ull << 58) - 1); bits = (u32)(e >> 58); bits = bits == 63u ? YK_NOCAP : bits; }
			else { bits = img.bits[p]; off = img.off[p]; }
			if (bits == YK_NOCAP) { miss = true; continue; }
			live[u] = true; slot[u] = off; nmask[u] = (1u << bits) - 1; idx[u] = yk_h2b((u32)kid[u], bits);
		}
#pragma unroll
		for (int u = 0; u < AC_U; ++u) kc[u] = live[u] ? karena[slot[u] + idx[u]] : YK_EMPTY;
#pragma unroll
		for (int u = 0; u < AC_U; ++u) {
			if (!live[u]) continue;
			const u32 first = idx[u];
			bool found = false;
			for (;;) {
				if (kc[u] == YK_EMPTY && !(LONG && lk_used(img, slot[u] + idx[u]))) break;
				if (kc[u] >> 10 == kid[u]) {
					const u32 c = (u32)(kc[u] & 1023u) + c1[u] - 1u;       /* cur >= 1: the create pass counted this key once */
					karena[slot[u] + idx[u]] = (kc[u] & ~1023ull) | (c > 1023u ? 1023u : c);
					found = true;
					break;
				}
				idx[u] = (idx[u] + 1) & nmask[u];
				if (idx[u] == first) break;
				kc[u] = karena[slot[u] + idx[u]];
			}
			miss |= !found;
		}
	}
	if (miss) *missing = 1u;
}

/* ------------------------------------------------------------------------------------------
 * last put-call per sub-table.  khashl grows at the NEXT put-call after the load factor reaches
 * 0.75 (khashl.h:202), even when that call finds its key.  So the layout needs, per sub-table, the
 * stream time of the last put-call of the pass.  Only the tail of the stream can matter; the host
 * scans the tail first and the whole batch only for sub-tables the tail did not reach.
 * ------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(256)
void k_lastput(const Rec *__restrict__ rec, int64_t n, u64 t0, u64 t_from,
               AccTab tab, ImgView img, int img_nonempty, int bloom_mode, const u32 *only_missing, u64 *lp_batch)
{
	const int64_t stride = (int64_t)gridDim.x * blockDim.x;
	const u32 pmask = (1u << tab.pre) - 1;
	for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
		const Rec rc = rec[i];
		const u64 t = t0 + (u32)rc.y;
		if (t < t_from) continue;
		const u64 key = rc.x;
		const u32 p = (u32)key & pmask;
		if (only_missing && !(only_missing[p >> 5] >> (p & 31) & 1)) continue;
		bool put = true;
		if (bloom_mode && !(img_nonempty && img_find(img, key) >= 0)) {
			const AccSlot *s = acc_find(tab, key);
			/* the first occurrence is a put-call only if it passed the gate (htab.c:63-65) */
			if (s && s->t1 == t && !(s->flags & YK_FLAG_FP)) put = false;
		}
		if (put) atomicMax(&lp_batch[p], t + 1);
	}
}

__global__ void k_lastput_merge(u64 *lastput, const u64 *lp_batch, u32 *missing, u32 *n_missing, int P, int plo, int phi)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= P) return;
	const u64 v = lp_batch[p];
	if (v) { if (v > lastput[p]) lastput[p] = v; }
	else if (p >= plo && p < phi) { atomicOr(&missing[p >> 5], 1u << (p & 31)); atomicAdd(n_missing, 1u); }
}

/* ------------------------------------------------------------------------------------------
 * K2: order-exact blocked bloom gate (reference bbf.c:25-42 + htab.c:63-65).
 * Only the FIRST occurrence of a k-mer can be rejected by the gate, and it is accepted iff every
 * one of its probe bits was set by the first occurrence of some other k-mer earlier in the stream.
 * Per time-ordered batch, over the keys first seen in the batch:
 *   test   : probe bits against the pre-batch filter -> all set: accepted (FP); else missing mask
 *   set    : OR the missing bits in; a bit found already set here was set by another key of the
 *            same batch -> note it in the (hashed) `multi` filter
 *   check  : a key whose missing bits are ALL noted is a candidate (its fate depends on order)
 *   mapfill/resolve : exact order for candidates through a min-time map over the noted bits
 * ------------------------------------------------------------------------------------------ */
struct BfProbe { u64 bit_base; u32 h1, h2, nd; };

__device__ __forceinline__ BfProbe bf_probe(const BloomView &bf, u64 key, int pre)
{
	BfProbe q;
	const u64 p = key & ((1ull << pre) - 1), x = key >> pre;
	const int xb = bf.nb - 9;
	const u64 blk = x & ((1ull << xb) - 1);
	q.h1 = (u32)(x >> xb) & 511;
	q.h2 = bf.nb < 64 ? (u32)(x >> bf.nb) & 511 : 0;
	if ((q.h2 & 31) == 0) q.h2 = (q.h2 + 1) & 511;
	const u32 cyc = 512u / (q.h2 & (0u - q.h2));         /* probes repeat after 512/gcd(h2,512) steps */
	q.nd = (u32)bf.n_hash < cyc ? (u32)bf.n_hash : cyc;
	q.bit_base = p << bf.nb | blk << 9;
	return q;
}

__global__ __launch_bounds__(256)
void k_bf_test(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, u64 *miss)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_new; i += stride) {
		AccSlot *s = tab.s + newlist[i];
		const BfProbe q = bf_probe(bf, s->key, tab.pre);
		const u32 *blk = bf.bits32 + (q.bit_base >> 5);
		bool any = false;
		for (int w = 0; w < bf.mw; ++w) {
			u64 m = 0;
			for (u32 j = w * 64; j < q.nd && j < (u32)(w + 1) * 64; ++j) {
				const u32 z = (q.h1 + j * q.h2) & 511;
				if (!(blk[z >> 5] >> (z & 31) & 1)) m |= 1ull << (j & 63);
			}
			miss[i * bf.mw + w] = m;
			any |= m != 0;
		}
		if (!any) s->flags |= YK_FLAG_FP;
	}
}

__device__ __forceinline__ u32 multi_idx(u64 bitid, int multi_bits) { return (u32)(yk_mix64(bitid) >> (64 - multi_bits)); }

__global__ __launch_bounds__(256)
void k_bf_set(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, const u64 *miss,
              u32 *multi, int multi_bits, u64 *counters)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_new; i += stride) {
		const AccSlot *s = tab.s + newlist[i];
		if (s->flags & YK_FLAG_FP) continue;
		const BfProbe q = bf_probe(bf, s->key, tab.pre);
		u32 *blk = bf.bits32 + (q.bit_base >> 5);
		for (int w = 0; w < bf.mw; ++w) {
			u64 m = miss[i * bf.mw + w];
			while (m) {
				const u32 j = w * 64 + (__ffsll((long long)m) - 1);
				m &= m - 1;
				const u32 z = (q.h1 + j * q.h2) & 511, bit = 1u << (z & 31);
				const u32 old = atomicOr(&blk[z >> 5], bit);
				if (old & bit) {
					const u32 x = multi_idx(q.bit_base + z, multi_bits);
					atomicOr(&multi[x >> 5], 1u << (x & 31));
					counters[YKC_ANYMULTI] = 1;
				}
			}
		}
	}
}

__global__ __launch_bounds__(256)
void k_bf_check(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, const u64 *miss,
                const u32 *multi, int multi_bits, u64 *cand, u64 *counters)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_new; i += stride) {
		const AccSlot *s = tab.s + newlist[i];
		if (s->flags & YK_FLAG_FP) continue;
		const BfProbe q = bf_probe(bf, s->key, tab.pre);
		bool all = true;
		u32 n_noted = 0;
		for (int w = 0; w < bf.mw; ++w) {
			u64 m = miss[i * bf.mw + w];
			while (m) {
				const u32 j = w * 64 + (__ffsll((long long)m) - 1);
				m &= m - 1;
				const u32 z = (q.h1 + j * q.h2) & 511;
				const u32 x = multi_idx(q.bit_base + z, multi_bits);
				if (multi[x >> 5] >> (x & 31) & 1) ++n_noted; else all = false;
			}
		}
		if (n_noted) atomicAdd(&counters[YKC_NMARKED], (u64)n_noted);
		if (all) cand[atomicAdd(&counters[YKC_NCAND], 1ull)] = i;
	}
}

/* min-time map: open addressing, key = bit id + 1 (0 = free), value = ~(earliest first-occurrence
 * time) so that a zero-filled map means "never" and atomicMax implements the minimum */
__device__ __forceinline__ void map_min(u64 *map, int map_bits, u64 bitid, u64 t)
{
	const u64 mask = (1ull << map_bits) - 1, k1 = bitid + 1;
	u64 i = yk_mix64(bitid) >> (64 - map_bits);
	for (;;) {
		u64 cur = map[2 * i];
		if (cur == 0) cur = atomicCAS(&map[2 * i], 0ull, k1);
		if (cur == 0 || cur == k1) { atomicMax(&map[2 * i + 1], ~t); return; }
		i = (i + 1) & mask;
	}
}

__device__ __forceinline__ u64 map_get(const u64 *map, int map_bits, u64 bitid)
{
	const u64 mask = (1ull << map_bits) - 1, k1 = bitid + 1;
	u64 i = yk_mix64(bitid) >> (64 - map_bits);
	for (;;) {
		const u64 cur = map[2 * i];
		if (cur == k1) return ~map[2 * i + 1];
		if (cur == 0) return YK_TINF;
		i = (i + 1) & mask;
	}
}

__global__ __launch_bounds__(256)
void k_bf_mapfill(AccTab tab, const u64 *newlist, u64 n_new, BloomView bf, const u64 *miss,
                  const u32 *multi, int multi_bits, u64 *map, int map_bits)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_new; i += stride) {
		const AccSlot *s = tab.s + newlist[i];
		if (s->flags & YK_FLAG_FP) continue;
		const BfProbe q = bf_probe(bf, s->key, tab.pre);
		const u64 t1 = s->t1;
		for (int w = 0; w < bf.mw; ++w) {
			u64 m = miss[i * bf.mw + w];
			while (m) {
				const u32 j = w * 64 + (__ffsll((long long)m) - 1);
				m &= m - 1;
				const u32 z = (q.h1 + j * q.h2) & 511;
				const u32 x = multi_idx(q.bit_base + z, multi_bits);
				if (multi[x >> 5] >> (x & 31) & 1) map_min(map, map_bits, q.bit_base + z, t1);
			}
		}
	}
}

__global__ __launch_bounds__(256)
void k_bf_resolve(AccTab tab, const u64 *newlist, const u64 *cand, u64 n_cand, BloomView bf,
                  const u64 *miss, const u64 *map, int map_bits)
{
	const u64 stride = (u64)gridDim.x * blockDim.x;
	for (u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x; c < n_cand; c += stride) {
		const u64 i = cand[c];
		AccSlot *s = tab.s + newlist[i];
		const BfProbe q = bf_probe(bf, s->key, tab.pre);
		const u64 t1 = s->t1;
		bool all = true;
		for (int w = 0; w < bf.mw && all; ++w) {
			u64 m = miss[i * bf.mw + w];
			while (m) {
				const u32 j = w * 64 + (__ffsll((long long)m) - 1);
				m &= m - 1;
				const u32 z = (q.h1 + j * q.h2) & 511;
				if (!(map_get(map, map_bits, q.bit_base + z) < t1)) { all = false; break; }
			}
		}
		if (all) s->flags |= YK_FLAG_FP;
	}
}

/* ------------------------------------------------------------------------------------------
 * selection: accumulator slots that enter the table -> (insertion time T, key<<10|count) records
 * grouped by sub-table.  No bloom: T = t1, count = occurrences (htab.c:66-69).  Bloom: accepted at
 * the first occurrence (T = t1, every occurrence counted) or at the second (T = t2, one less).
 * ------------------------------------------------------------------------------------------ */
__device__ __forceinline__ bool acc_select(const AccSlot &s, int bloom_mode, int pre, u32 *p, u64 *T, u64 *kc)
{
	if (s.key == YK_EMPTY) return false;
	u64 c = s.cnt;
	if (!bloom_mode || (s.flags & YK_FLAG_FP)) *T = s.t1;
	else if (s.t2 != YK_TINF) { *T = s.t2; c -= 1; }
	else return false;
	if (c > 1023) c = 1023;
	*p = (u32)s.key & ((1u << pre) - 1);
	*kc = (s.key >> pre) << 10 | c;
	return true;
}

/* One workgroup owns SEL_CHUNK consecutive accumulator slots.  The accumulator is prefix-major,
 * so a chunk holds keys of one or two sub-tables only: counts are aggregated in an LDS histogram
 * and flushed with a handful of global atomics per workgroup instead of one per key. */
#define SEL_CHUNK 8192
#define SEL_MAXP  8192

__global__ __launch_bounds__(256)
void k_select_count(AccTab tab, int bloom_mode, u32 *seg_cnt)
{
	__shared__ u32 s_hist[SEL_MAXP];
	const u32 P = 1u << tab.pre;
	const bool lds = P <= SEL_MAXP;
	const u64 n = tab.mask + 1, lo = (u64)blockIdx.x * SEL_CHUNK, hi = lo + SEL_CHUNK < n ? lo + SEL_CHUNK : n;
	if (lds) { for (u32 p = threadIdx.x; p < P; p += 256) s_hist[p] = 0; __syncthreads(); }
	for (u64 i = lo + threadIdx.x; i < hi; i += 256) {
		const AccSlot s = tab.s[i];
		u32 p; u64 T, kc;
		if (acc_select(s, bloom_mode, tab.pre, &p, &T, &kc)) atomicAdd(lds ? &s_hist[p] : &seg_cnt[p], 1u);
	}
	if (lds) {
		__syncthreads();
		for (u32 p = threadIdx.x; p < P; p += 256) if (s_hist[p]) atomicAdd(&seg_cnt[p], s_hist[p]);
	}
}

__global__ __launch_bounds__(256)
void k_select_scatter(AccTab tab, int bloom_mode, const u64 *seg_off, u32 *seg_cur, u64 *rec_kc, u64 *rec_t)
{
	__shared__ u32 s_hist[SEL_MAXP];
	const u32 P = 1u << tab.pre;
	const bool lds = P <= SEL_MAXP;
	const u64 n = tab.mask + 1, lo = (u64)blockIdx.x * SEL_CHUNK, hi = lo + SEL_CHUNK < n ? lo + SEL_CHUNK : n;
	if (lds) {
		for (u32 p = threadIdx.x; p < P; p += 256) s_hist[p] = 0;
		__syncthreads();
		for (u64 i = lo + threadIdx.x; i < hi; i += 256) {
			const AccSlot s = tab.s[i];
			u32 p; u64 T, kc;
			if (acc_select(s, bloom_mode, tab.pre, &p, &T, &kc)) atomicAdd(&s_hist[p], 1u);
		}
		__syncthreads();
		/* reserve this workgroup's range of every sub-table it met; s_hist becomes the running cursor */
		for (u32 p = threadIdx.x; p < P; p += 256) { const u32 c = s_hist[p]; if (c) s_hist[p] = atomicAdd(&seg_cur[p], c); }
		__syncthreads();
	}
	for (u64 i = lo + threadIdx.x; i < hi; i += 256) {      /* second read of the chunk hits L2 */
		const AccSlot s = tab.s[i];
		u32 p; u64 T, kc;
		if (acc_select(s, bloom_mode, tab.pre, &p, &T, &kc)) {
			const u64 d = seg_off[p] + atomicAdd(lds ? &s_hist[p] : &seg_cur[p], 1u);
			rec_kc[d] = kc; rec_t[d] = T;
		}
	}
}

