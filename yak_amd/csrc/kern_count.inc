/* kern_count.inc -- part of kernels.hip (one translation unit, included in this order): exclusive-ownership counting: level-2 partition, k_lc2 and the tiers behind it, k_cnt2 (count pass on retained records), gather of the selected keys */
/* ==========================================================================================
 * FAST PATH: exclusive-ownership counting.
 * Device atomics on gfx950 execute at the memory side whatever their scope, ~10 G/s at best, and a
 * pass needs 1-3 of them per k-mer instance.  So the instances of a pass are radix-partitioned
 * twice -- by sub-table prefix (k_xpart / k_rpart), then into sub-buckets small enough for an
 * LDS hash table (k_part2) -- and ONE workgroup then owns a sub-bucket outright: it counts its
 * k-mers with LDS atomics only, owns the bloom blocks they map to (so the gate of bbf.c:25-42 /
 * htab.c:63-65 is evaluated per 512-bit block, sequentially in stream order, exactly as the
 * reference does), and emits just the keys that enter the table.  No global atomics per instance.
 * ========================================================================================== */
__device__ __forceinline__ u32 sub_of(u64 h, const FastParams &fp)
{
	/* the bits of x = hash >> pre that this sweep routes by (FastParams.sw / ssh): with a filter a sub-bucket is a contiguous range of bloom blocks,
	 * without one any bit slice is uniform (yak_hash64 mixes well) */
	const u64 x = h >> fp.pre;
	if (fp.s2_bits == 0) return 0;
	return (u32)((x & ((1ull << fp.sw) - 1)) >> fp.ssh) & ((1u << fp.s2_bits) - 1);
}

/* ---- the two 8-byte record formats of the fast path (yk_device.h YK_R8_*, FastParams.rec8_*) ---- */
/* rank of tagged record i in its bucket's stream: records of one round are contiguous and share the toggle bit; inside the round
 * the position field orders them.  `src` points at the chunk's first record; [-before, n + after) is the bucket */
__device__ __forceinline__ u32 r8_rank(const u64 *src_, int64_t i, u32 before, u32 n, u32 after)
{
	const u64 YK_GLOBAL *src = yk_global(u64, src_);
	const u64 me = src[i];
	const u32 tg = (u32)me & YK_R8_TOGGLE, pos = (u32)me & 1023u;
	int64_t a = i, e = i + 1;
	while (a > -(int64_t)before && ((u32)src[a - 1] & YK_R8_TOGGLE) == tg) --a;
	while (e < (int64_t)n + after && ((u32)src[e] & YK_R8_TOGGLE) == tg) ++e;
	u32 r = 0;
	for (int64_t j = a; j < e; ++j) r += ((u32)src[j] & 1023u) < pos;
	return (u32)((int64_t)before + a) + r;
}
/* one level-2 input record -> (hash, time): Rec {hash, position} + tbase, or a tagged record of sub-table c.bucket */
template <bool NEED_T>
__device__ __forceinline__ void p2_load(const Chunk2 &c, u32 i, const FastParams &fp, u64 *h, u32 *t)
{
	if (c.fmt == 1) {
		const u64 *src = (const u64*)c.rec;
		*h = (yk_global(u64, src)[i] >> YK_R8_TAG_BITS) << fp.pre | c.bucket;
		if (NEED_T) *t = c.tbase + r8_rank(src, (int64_t)i, c.before, c.n, c.after);
	} else {
		const Rec rc = yk_global_rec(c.rec, i);
		*h = rc.x;
		if (NEED_T) *t = (u32)rc.y + c.tbase;
	}
}
/* level-2 output / counting input: the sub-bucket's bits taken out of hash >> pre, the rank below it */
__device__ __forceinline__ u64 r8_pack(u64 h, u32 t, const FastParams &fp)
{
	const u64 x = h >> fp.pre;
	const int sh = fp.sw - fp.s2_tot;
	return (((x >> (sh + fp.s2_tot)) << sh) | (x & ((1ull << sh) - 1))) << fp.tb | t;
}
__device__ __forceinline__ Rec r8_unpack(u64 r, u32 sb, const FastParams &fp)
{
	const u64 xs = r >> fp.tb;
	const int sh = fp.sw - fp.s2_tot;
	const u64 x = ((xs >> sh) << (sh + fp.s2_tot)) | ((u64)(sb & ((1u << fp.s2_tot) - 1)) << sh) | (xs & ((1ull << sh) - 1));
	return make_ulonglong2(x << fp.pre | (sb >> fp.s2_tot), r & ((1ull << fp.tb) - 1));
}
/* the same without the prefix: {hash >> pre, rank} */
__device__ __forceinline__ Rec r8_unpack_x(u64 r, u32 sb, const FastParams &fp)
{
	const u64 xs = r >> fp.tb;
	const int sh = fp.sw - fp.s2_tot;
	const u64 x = ((xs >> sh) << (sh + fp.s2_tot)) | ((u64)(sb & ((1u << fp.s2_tot) - 1)) << sh) | (xs & ((1ull << sh) - 1));
	return make_ulonglong2(x, r & ((1ull << fp.tb) - 1));
}
__device__ __forceinline__ Rec lc_rec(const FastParams &fp, const Rec *rec, u64 i, u32 sb)
{
	return fp.rec8_out ? r8_unpack(((const u64*)rec)[i], sb, fp) : rec[i];
}
/* the same in two steps, for loads that are requested long before they are used (decoding at once would wait for the data) */
__device__ __forceinline__ Rec lc_raw(const FastParams &fp, const Rec *rec, u64 i)
{
	return fp.rec8_out ? make_ulonglong2(((const u64*)rec)[i], 0) : rec[i];
}
__device__ __forceinline__ Rec lc_dec(const FastParams &fp, const Rec raw, u32 sb)
{
	return fp.rec8_out ? r8_unpack(raw.x, sb, fp) : raw;
}

/* TS: the same sweeps as one pass of the sort by insertion time -- the records are {key, time} pairs and the "sub-bucket" is the time's bin */
template <bool TS> __device__ __forceinline__ u32 p2_sub(u64 h, u32 t, const FastParams &fp)
{
	if (TS) return (t >> fp.ssh) & ((1u << fp.s2_bits) - 1);
	return sub_of(h, fp);
}

template <int MODE, bool TS = false>   /* 0 = histogram, 1 = scatter */
__global__ __launch_bounds__(1024)
void k_part2(const Chunk2 *chunks, FastParams fp, u32 *rows2, const u64 *__restrict__ bbase, Rec *__restrict__ out)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_bkt[];
	const Chunk2 c = chunks[blockIdx.x];
	if (MODE) out = fp.rec8_out ? (Rec*)((u64*)out + bbase[c.bucket]) : out + bbase[c.bucket];   /* rows2 holds 32-bit offsets inside the bucket's output (a slice may hold more than 2^32 records, a bucket may not) */
	const int S2 = 1 << fp.s2_bits, NT = blockDim.x;
	u32 *row = rows2 + (size_t)blockIdx.x * S2;
	for (int j = threadIdx.x; j < S2; j += NT) s_bkt[j] = MODE ? row[j] : 0;
	__syncthreads();
	for (u32 i = threadIdx.x; i < c.n; i += NT) {
		u64 h; u32 t = 0;
		p2_load<MODE != 0 || TS>(c, i, fp, &h, &t);
		const u32 d = atomicAdd(&s_bkt[p2_sub<TS>(h, t, fp)], 1u);
		if (MODE) { if (fp.rec8_out) ((u64*)out)[d] = r8_pack(h, t, fp); else out[d] = make_ulonglong2(h, (u64)t); }
	}
	if (!MODE) { __syncthreads(); for (int j = threadIdx.x; j < S2; j += NT) row[j] = s_bkt[j]; }
}

/* the same scatter with write combining (see WcView above): 1024 records per round */
#define WC_CAP 5
#define WC_NT  1024
#define WC_SEG 2048          /* sub-buckets whose stacks fit in LDS at once */
template <bool TS = false>
__global__ __launch_bounds__(WC_NT)
void k_part2_wc(const Chunk2 *chunks, FastParams fp, const u32 *__restrict__ rows2, const u64 *__restrict__ sbstart, const u64 *__restrict__ bbase, Rec *__restrict__ out)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	const Chunk2 c = chunks[blockIdx.x];
	const u64 base = bbase[c.bucket];
	out += base;
	const int S2 = 1 << fp.s2_bits, SEG = S2 < WC_SEG ? S2 : WC_SEG;
	const u32 tid = threadIdx.x;
	WcView w;
	wc_carve<4, WC_CAP, true>(w, s_dyn, SEG, WC_NT);
	const u32 *row = rows2 + (size_t)blockIdx.x * S2;
	const u32 n_round = (c.n + WC_NT - 1) / WC_NT;
	/* more sub-buckets than stacks fit in LDS: one sweep over the chunk per segment of WC_SEG
	 * sub-buckets (the chunk is small enough to come back from L2) */
	for (int seg0 = 0; seg0 < S2; seg0 += SEG) {
		__syncthreads();
		for (int b = tid; b < SEG; b += WC_NT) {
			w.cnt[b] = 0; w.head[b] = row[seg0 + b];
			w.tail[b] = (c.spare & 1) ? (u32)(sbstart[(size_t)c.bucket * S2 + seg0 + b + 1] - base) : row[S2 + seg0 + b];   /* start of the next chunk's run = end of mine */
		}
		if (tid < 2) w.ntask[tid] = 0;
		__syncthreads();
		for (u32 rd = 0; rd < n_round; ++rd) {
			const u32 i = rd * WC_NT + tid, par = rd & 1;
			if (i < c.n) {
				u64 h; u32 t;
				p2_load<true>(c, i, fp, &h, &t);
				const u32 sub = p2_sub<TS>(h, t, fp) - (u32)seg0;
				if (sub < (u32)SEG) wc_place<4, WC_CAP, true>(w, sub, h, t, par, out);
			}
			__syncthreads();
			wc_flush<4, WC_CAP, true>(w, par, out);
			__syncthreads();
		}
		wc_drain<4, WC_CAP, true>(w, SEG, out);
	}
}

/* the level-2 scatter for 8-byte output records: groups of 8 (64 bytes), one stack of WC8_CAP entries per sub-bucket (no tail
 * array: a record that finds its stack full is stored at its final place, wcs_place / wcs_flush) */
#define WC8_CAP 8
/* Input: tagged records only (fp.rec8_in).  The rank of a record (r8_rank) needs its round's neighbours; chasing them through
 * global memory is a chain of dependent loads per round, so the tags of four consecutive rounds of the stream live in an LDS ring
 * (16-bit words: in-the-stream << 11 | toggle << 10 | position; round q in slot q & 3): while round rd is ranked the ring holds
 * rd - 1, rd and rd + 1 -- a run is at most 1024 records long, so that window always holds it whole -- and rd + 2 is being
 * requested.  A run is 1.5 records long on average (one sub-table's share of 1024 stream positions): the three neighbours on
 * either side are read and compared without a branch, and only a record whose run reaches beyond them walks on. */
/* OUT16: the first sweep of a two-sweep partition -- the same ranks from the same ring, {hash, rank} records out (groups of four, k_part2_wc's stacks) */
/* CAP8: entries per stack.  7 (the eighth record of a group is stored directly and takes the stack with it, as in k_xpart_wcs) brings 1024 sub-buckets'
 * stacks to 76 KB with the ring: two workgroups per CU */
template <bool OUT16, int CAP8 = WC8_CAP>
__global__ __launch_bounds__(WC_NT)
void k_part2_wc8(const Chunk2 *chunks, FastParams fp, const u32 *__restrict__ rows2, const u64 *__restrict__ sbstart, const u64 *__restrict__ bbase, u64 *__restrict__ out_)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	__shared__ unsigned short s_tag[4 * WC_NT + 8];                    /* ring entry y at [y + 3]; the first and last three mirrored beyond either end: a lane's window y - 3 .. y + 3 is seven consecutive words */
	const Chunk2 c = chunks[blockIdx.x];
	const u64 obase = bbase[c.bucket];
	u64 *out = out_ + (OUT16 ? 2 * obase : obase);
	const int S2 = 1 << fp.s2_bits, SEG = S2 < WC_SEG ? S2 : WC_SEG;
	const u32 tid = threadIdx.x;
	WcView w;
	if (OUT16) wc_carve<4, WC_CAP, true>(w, s_dyn, SEG, WC_NT);
	else {
		w.h = (u64*)s_dyn; w.t = 0;
		w.cnt = s_dyn + 2 * (size_t)SEG * CAP8; w.head = w.cnt + SEG; w.tail = 0; w.task = w.head + SEG; w.ntask = w.task + WC_NT;
	}
	const u32 *row = rows2 + (size_t)blockIdx.x * S2;
	const int n_round = (int)((c.n + WC_NT - 1) / WC_NT);
	const u64 YK_GLOBAL *src = yk_global(u64, c.rec);                              /* global, not FLAT: the loads two rounds ahead must not count on the LDS counter */
	const int64_t g_lo = -(int64_t)c.before, g_hi = (int64_t)c.n + c.after;      /* the sub-table's stream of this batch, relative to the chunk */
	auto fetch = [&](int q) -> u64 { const int64_t g = (int64_t)q * WC_NT + tid; return g >= g_lo && g < g_hi ? src[g] : 0; };
	auto post = [&](int q, u64 r) {                                                  /* round q's tags -> ring slot q & 3; a position outside the stream belongs to no run */
		const int64_t g = (int64_t)q * WC_NT + tid;
		const u32 y = ((u32)q & 3u) * WC_NT + tid;
		const unsigned short v = (unsigned short)(g >= g_lo && g < g_hi ? 0x800u | ((u32)r & 0x7ffu) : 0u);
		s_tag[y + 3] = v;
		if (y < 3) s_tag[y + 3 + 4 * WC_NT] = v;
		if (y >= 4 * WC_NT - 3) s_tag[y + 3 - 4 * WC_NT] = v;
	};
	for (int seg0 = 0; seg0 < S2; seg0 += SEG) {
		__syncthreads();
		for (int b = tid; b < SEG; b += WC_NT) {
			w.cnt[b] = 0; w.head[b] = row[seg0 + b];
			if (OUT16) w.tail[b] = (c.spare & 1) ? (u32)(sbstart[(size_t)c.bucket * S2 + seg0 + b + 1] - obase) : row[S2 + seg0 + b];   /* start of the next chunk's run = end of mine */
		}
		if (tid < 2) w.ntask[tid] = 0;
		u64 cur, nxt;
		{ const u64 r = fetch(-1); cur = fetch(0); nxt = fetch(1); post(-1, r); post(0, cur); post(1, nxt); }
		__syncthreads();
		for (int rd = 0; rd < n_round; ++rd) {
			const u32 i = (u32)rd * WC_NT + tid, par = (u32)rd & 1;
			const u64 nn = fetch(rd + 2);
			if (i < c.n) {
				/* rank = the record's place in the stream - the records of its run that lie before it + those of the run with a smaller position */
				const u32 me = 0x800u | ((u32)cur & 0x7ffu), pos = (u32)cur & 1023u, x = ((u32)rd & 3u) * WC_NT + tid;
				auto at = [&](int d) -> u32 { return s_tag[((x + (u32)d) & (4 * WC_NT - 1)) + 3]; };
				auto same = [&](u32 nb) -> bool { return ((nb ^ me) & 0xC00u) == 0; };   /* in the stream, and the same toggle */
				const unsigned short *win = s_tag + x;                              /* win[3] is the record's own word */
				const u32 n1 = win[4], n2 = win[5], n3 = win[6], p1 = win[2], p2 = win[1], p3 = win[0];
				const bool u1 = same(n1), u2 = u1 && same(n2), u3 = u2 && same(n3), d1 = same(p1), d2 = d1 && same(p2), d3 = d2 && same(p3);
				u32 below = (u32)d1 + (u32)d2 + (u32)d3;
				u32 r = (u32)(u1 && (n1 & 1023u) < pos) + (u32)(u2 && (n2 & 1023u) < pos) + (u32)(u3 && (n3 & 1023u) < pos)
				      + (u32)(d1 && (p1 & 1023u) < pos) + (u32)(d2 && (p2 & 1023u) < pos) + (u32)(d3 && (p3 & 1023u) < pos);
				if (u3) for (int d = 4; ; ++d) { const u32 nb = at(d); if (!same(nb)) break; r += (nb & 1023u) < pos; }        /* a long run (a repeat: many positions of one round in one sub-table) */
				if (d3) for (int d = -4; ; --d) { const u32 nb = at(d); if (!same(nb)) break; r += (nb & 1023u) < pos; ++below; }
				const u32 t = c.tbase + c.before + i - below + r;
				const u64 h = (cur >> YK_R8_TAG_BITS) << fp.pre | c.bucket;
				const u32 sub = sub_of(h, fp) - (u32)seg0;
				if (sub < (u32)SEG) { if (OUT16) wc_place<4, WC_CAP, true>(w, sub, h, t, par, out); else wcs_place<CAP8>(w, sub, r8_pack(h, t, fp), par, out); }
			}
			__syncthreads();
			/* over the slot of round rd - 1, which nobody reads any more.  Before the flush: waiting for the record means waiting for every store
			 * issued before it (one counter, in order), and behind the flush those would be this round's own stores */
			post(rd + 2, nn);
			if (OUT16) wc_flush<4, WC_CAP, true>(w, par, out); else wcs_flush<CAP8>(w, par, out);
			cur = nxt; nxt = nn;
			__syncthreads();
		}
		if (OUT16) wc_drain<4, WC_CAP, true>(w, SEG, out);
		else for (u32 b = tid / 8; b < (u32)SEG; b += WC_NT / 8) {        /* what is left in the stacks */
			const u32 q = tid & 7, cn = w.cnt[b];
			if (q < cn) out[w.head[b] + q] = w.h[b * CAP8 + q];
		}
	}
}

/* the second sweep of a two-sweep level-2 partition (more than 2^13 sub-buckets per sub-table): the first sweep left {hash, rank} records grouped by
 * the high sub-bucket bits; a chunk is a run of one such group (c.bucket = sub-table << high bits | group), the ranks are explicit, so there is no
 * ring -- the same stacks and groups of 8 as k_part2_wc8, the records requested two rounds ahead */
__global__ __launch_bounds__(WC_NT)
void k_part2_wc8r(const Chunk2 *chunks, FastParams fp, const u32 *__restrict__ rows2, const u64 *__restrict__ bbase, u64 *__restrict__ out)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	const Chunk2 c = chunks[blockIdx.x];
	out += bbase[c.bucket];
	const int S2 = 1 << fp.s2_bits, SEG = S2 < WC_SEG ? S2 : WC_SEG;
	const u32 tid = threadIdx.x;
	WcView w;
	w.h = (u64*)s_dyn; w.t = 0;
	w.cnt = s_dyn + 2 * (size_t)SEG * WC8_CAP; w.head = w.cnt + SEG; w.tail = 0; w.task = w.head + SEG; w.ntask = w.task + WC_NT;
	const u32 *row = rows2 + (size_t)blockIdx.x * S2;
	const int n_round = (int)((c.n + WC_NT - 1) / WC_NT);
	auto fetch = [&](int q) -> Rec { const u32 g = (u32)q * WC_NT + tid; return g < c.n ? yk_global_rec(c.rec, g) : make_ulonglong2(0, 0); };
	for (int seg0 = 0; seg0 < S2; seg0 += SEG) {
		__syncthreads();
		for (int b = tid; b < SEG; b += WC_NT) { w.cnt[b] = 0; w.head[b] = row[seg0 + b]; }
		if (tid < 2) w.ntask[tid] = 0;
		Rec cur = fetch(0), nxt = fetch(1);
		__syncthreads();
		for (int rd = 0; rd < n_round; ++rd) {
			const u32 i = (u32)rd * WC_NT + tid, par = (u32)rd & 1;
			const Rec nn = fetch(rd + 2);
			if (i < c.n) {
				const u32 sub = sub_of(cur.x, fp) - (u32)seg0;
				if (sub < (u32)SEG) wcs_place<WC8_CAP>(w, sub, r8_pack(cur.x, (u32)cur.y + c.tbase, fp), par, out);
			}
			__syncthreads();
			wcs_flush<WC8_CAP>(w, par, out);
			cur = nxt; nxt = nn;
			__syncthreads();
		}
		for (u32 b = tid / 8; b < (u32)SEG; b += WC_NT / 8) {             /* what is left in the stacks */
			const u32 q = tid & 7, cn = w.cnt[b];
			if (q < cn) out[w.head[b] + q] = w.h[b * WC8_CAP + q];
		}
	}
}

/* one workgroup per level-1 bucket: rows2 counts -> absolute offsets; sbstart[bucket * S2 + s] */
__global__ __launch_bounds__(256)
void k_part2_scan(const u32 *chunk_first, const u64 *bbase, int s2_bits, u32 *rows2, u64 *sbstart, int P, int rel)   /* rel: the chunks' offsets are relative to the bucket's base (32 bits hold them whatever the slice's size) */
{
	__shared__ u64 s_tot[256];
	__shared__ u64 s_carry;
	const int S2 = 1 << s2_bits, b = blockIdx.x;
	const u32 c0 = chunk_first[b], c1 = chunk_first[b + 1];
	if (threadIdx.x == 0) s_carry = bbase[b];
	__syncthreads();
	for (int s0 = 0; s0 < S2; s0 += 256) {
		const int s = s0 + threadIdx.x;
		u64 tot = 0;
		if (s < S2) for (u32 c = c0; c < c1; ++c) tot += rows2[(size_t)c * S2 + s];
		s_tot[threadIdx.x] = tot;
		__syncthreads();
		if (threadIdx.x == 0) {
			u64 acc = s_carry;
			for (int j = 0; j < 256; ++j) { const u64 t = s_tot[j]; s_tot[j] = acc; acc += t; }
			s_carry = acc;
		}
		__syncthreads();
		if (s < S2) {
			u64 run = s_tot[threadIdx.x];
			sbstart[(size_t)b * S2 + s] = run;
			const u64 sub = rel ? bbase[b] : 0;
			for (u32 c = c0; c < c1; ++c) { const u32 v = rows2[(size_t)c * S2 + s]; rows2[(size_t)c * S2 + s] = (u32)(run - sub); run += v; }
		}
		__syncthreads();
	}
	if (b == P - 1 && threadIdx.x == 0) sbstart[(size_t)P * S2] = s_carry;
}

#define LC_EXIST 0x40000000u
#define LC_FP    0x80000000u
#define LC_CMASK 0x000fffffu              /* occurrences, clamped; bits 29:20 = rank inside a bloom block */
#define T32_INF  0xffffffffu
#define LC_BLOOM_WORDS 2048               /* bloom range staged in LDS: up to 128 blocks of 512 bits */

/* The tier behind k_lc2, for the sub-buckets it passes on (more distinct k-mers than its LDS table takes) and for the passes it does not run at all
 * (n_hash > 32, a sub-bucket that owns more blocks of the filter than k_lc2 stages, the test switch YAKAMD_LC2=0): the same algorithm -- one
 * workgroup owns the sub-bucket, counts with atomics on tables of its own, evaluates the gate of bbf.c:25-42 / htab.c:63-65 per 512-bit block in
 * order of first occurrence -- with the tables in global scratch (any number of distinct k-mers) and the filter where it lies in memory.  Exact, and
 * slow: nothing of a benchmark workload comes here.  (Rounds 1-4 had two LDS tiers in between; k_lc2 took their work in round 2 and round 5 took
 * them out.) */
struct LcTab { u64 *K; u32 *T1, *T2, *CN, *TM; u64 *SO; u32 *SP; u32 cap; };

__device__ __forceinline__ void lc_sync() { block_sync_global(); }

__device__ __forceinline__ u32 lc_home(u64 key, int pre, u32 cap) { return (u32)(((key >> pre) * 0x9E3779B97F4A7C15ull) >> 24) & (cap - 1); }

struct BfSeq { u32 h1, h2, nd; };
__device__ __forceinline__ BfSeq lc_seq(u64 key, const FastParams &fp)       /* probe sequence inside the 512-bit block (bbf.c:28-33) */
{
	BfSeq q;
	const u64 x = key >> fp.pre;
	q.h1 = (u32)(x >> (fp.nb - 9)) & 511;
	q.h2 = fp.nb < 64 ? (u32)(x >> fp.nb) & 511 : 0;
	if ((q.h2 & 31) == 0) q.h2 = (q.h2 + 1) & 511;
	const u32 cyc = 512u >> (__ffs((int)q.h2) - 1);           /* the probes repeat after 512 / gcd(h2, 512) steps */
	q.nd = (u32)fp.n_hash < cyc ? (u32)fp.n_hash : cyc;
	return q;
}
__device__ __forceinline__ BfSeq lc_seq_x(u64 x, const FastParams &fp)     /* the same from x = hash >> pre */
{
	BfSeq q;
	q.h1 = (u32)(x >> (fp.nb - 9)) & 511;
	q.h2 = fp.nb < 64 ? (u32)(x >> fp.nb) & 511 : 0;
	if ((q.h2 & 31) == 0) q.h2 = (q.h2 + 1) & 511;
	const u32 cyc = 512u >> (__ffs((int)q.h2) - 1);
	q.nd = (u32)fp.n_hash < cyc ? (u32)fp.n_hash : cyc;
	return q;
}

__device__ void lc_body(const FastParams &fp, const LcTab &T, u32 sb, const u64 *__restrict__ sbstart,
                        const Rec *__restrict__ rec, u32 *bloom32, const ImgView &img, const LcOut &O,
                        u32 *s_misc /* [8] in LDS */)
{
	const int tid = threadIdx.x;
	const u32 p = sb >> fp.s2_bits;
	const u64 lo = sbstart[sb], hi = sbstart[sb + 1];
	const int bb = fp.nb - 9, lb = bb - fp.s2_bits;              /* log2 bloom blocks owned by this sub-bucket */
	u32 *gw = 0;                                                   /* first word of the owned bloom range */
	if (fp.bloom_mode) gw = bloom32 + ((((u64)p << fp.nb) | ((u64)(sb & ((1u << fp.s2_bits) - 1)) << (lb + 9))) >> 5);
	if (lo == hi) {
		if (tid == 0) { O.nsel[sb] = 0; O.lp[sb] = 0; O.nd[sb] = 0; }
		return;
	}
	u32 *s_ndist = s_misc, *s_lp = s_misc + 2, *s_ne = s_misc + 3, *s_run = s_misc + 7;
	const bool pre0 = lo + tid < hi, pre1 = lo + 256 + tid < hi, pre2 = lo + 512 + tid < hi;
	Rec r0 = make_ulonglong2(0, 0), r1 = r0, r2 = r0;
	if (pre0) r0 = lc_raw(fp, rec, lo + tid);
	if (pre1) r1 = lc_raw(fp, rec, lo + 256 + tid);
	if (pre2) r2 = lc_raw(fp, rec, lo + 512 + tid);
	for (u32 i = tid; i < T.cap; i += 256) { T.K[i] = YK_EMPTY; T.T1[i] = T32_INF; T.T2[i] = T32_INF; T.CN[i] = 0; T.TM[i] = 0; }
	if (tid < 8) s_misc[tid] = 0;
	lc_sync();

	/* A: count; first / second / last occurrence times (same loser rule as k_acc_insert).  The first
	 * three records of every lane were requested before the table was initialised.  The table has at least
	 * twice as many slots as the sub-bucket has records: it cannot fill */
	u32 tmax = 0;
	auto put = [&](const Rec rc) {
		const u64 key = rc.x;
		const u32 t = (u32)rc.y;
		u32 s = lc_home(key, fp.pre, T.cap);
		for (;; s = (s + 1) & (T.cap - 1)) {
			u64 cur = T.K[s];
			if (cur == key) break;
			if (cur == YK_EMPTY) {
				cur = atomicCAS(&T.K[s], YK_EMPTY, key);
				if (cur == YK_EMPTY) { atomicAdd(s_ndist, 1u); break; }
				if (cur == key) break;
			}
		}
		if ((T.CN[s] & LC_CMASK) < 0x80000u) atomicAdd(&T.CN[s], 1u);   /* only min(count, 1023) is ever used */
		const u32 old = atomicMin(&T.T1[s], t);
		if (fp.bloom_mode) {
			if (old != T32_INF) atomicMin(&T.T2[s], old > t ? old : t);
			atomicMax(&T.TM[s], t);
		}
		tmax = t + 1 > tmax ? t + 1 : tmax;
	};
	if (pre0) put(lc_dec(fp, r0, sb));
	if (pre1) put(lc_dec(fp, r1, sb));
	if (pre2) put(lc_dec(fp, r2, sb));
	for (u64 i = lo + 768 + tid; i < hi; i += 256) put(lc_rec(fp, rec, i, sb));
	if (!fp.bloom_mode && tmax) atomicMax(s_lp, tmax);      /* without a filter every instance is a put-call */
	lc_sync();
	if (fp.dbg & 16) return;

	/* B: keys already in the table image only gain counts (htab.c:66-69 on an existing key) */
	if (fp.img_nonempty) {
		for (u32 s = tid; s < T.cap; s += 256) {
			if (T.K[s] == YK_EMPTY) continue;
			const int64_t idx = img_find(img, T.K[s]);
			if (idx >= 0) {
				const u64 kc = img.keys[idx], c = (kc & 1023) + (T.CN[s] & LC_CMASK);
				img.keys[idx] = fp.or_mode == 1 ? kc | (T.T1[s] & 15u) : fp.or_mode == 2 ? kc : (kc & ~1023ull) | (c > 1023 ? 1023 : c);
				T.CN[s] |= LC_EXIST;
			}
		}
		lc_sync();
	}

	/* C: the bloom gate (bbf.c:25-42 + htab.c:63-65).  This workgroup is the only one whose k-mers map
	 * to these 512-bit blocks.  A key passes at its first occurrence iff each of its probe bits was
	 * set before -- by the pre-existing filter or by a key of the same block seen earlier: the new keys
	 * are sorted by (block, first occurrence) and one lane per block applies its keys in that order */
	if (fp.bloom_mode && !(fp.dbg & 32)) {
		const u64 lmask = (1ull << lb) - 1;
		if (tid == 0) *s_ne = 0;
		lc_sync();
		for (u32 s = tid; s < T.cap; s += 256) {
			if (T.K[s] == YK_EMPTY || (T.CN[s] & LC_EXIST)) continue;
			const u64 blk_local = (T.K[s] >> fp.pre) & lmask;
			const u32 j = atomicAdd(s_ne, 1u);
			T.SO[j] = blk_local << 32 | T.T1[s]; T.SP[j] = s;
		}
		lc_sync();
		const u32 ne = *s_ne;
		u32 m = 1; while (m < ne) m <<= 1;
		for (u32 i = ne + tid; i < m; i += 256) { T.SO[i] = ~0ull; T.SP[i] = 0; }
		lc_sync();
		for (u32 k2 = 2; k2 <= m; k2 <<= 1)
			for (u32 j = k2 >> 1; j > 0; j >>= 1) {
				for (u32 i = tid; i < m; i += 256) {
					const u32 l = i ^ j;
					if (l > i) {
						const u64 a0 = T.SO[i], b0 = T.SO[l];
						if ((a0 > b0) == ((i & k2) == 0)) {
							T.SO[i] = b0; T.SO[l] = a0;
							const u32 t = T.SP[i]; T.SP[i] = T.SP[l]; T.SP[l] = t;
						}
					}
				}
				lc_sync();
			}
		for (u32 j0 = tid; j0 < ne; j0 += 256) {
			const u64 blk_local = T.SO[j0] >> 32;
			if (j0 && (T.SO[j0 - 1] >> 32) == blk_local) continue;      /* not the first key of its block */
			u32 *w = gw + (blk_local << 4);
			for (u32 j = j0; j < ne && (T.SO[j] >> 32) == blk_local; ++j) {
				const u32 s = T.SP[j];
				const BfSeq q = lc_seq(T.K[s], fp);
				u32 hits = 0;
				for (u32 i = 0, z = q.h1; i < q.nd; ++i, z = (z + q.h2) & 511) {
					const u32 word = w[z >> 5], bit = 1u << (z & 31);
					if (word & bit) ++hits; else w[z >> 5] = word | bit;
				}
				if (hits == q.nd) T.CN[s] |= LC_FP;
			}
		}
		lc_sync();
		/* D: last put-call = last instance that is not a rejected first occurrence (htab.c:63-65) */
		u32 best = 0;
		for (u32 s = tid; s < T.cap; s += 256) {
			if (T.K[s] == YK_EMPTY) continue;
			const u32 cn = T.CN[s];
			if ((cn & (LC_EXIST | LC_FP)) || (cn & LC_CMASK) >= 2) best = T.TM[s] + 1 > best ? T.TM[s] + 1 : best;
		}
		if (best) atomicMax(s_lp, best);
		lc_sync();
	}

	/* E: keys entering the table -> (key<<10|count, insertion time): to the front of the sub-bucket's own record range in
	 * the output arrays (a sub-bucket never selects more keys than it has records); k_lc_compact gathers the fragments */
	for (u32 s = tid; s < T.cap; s += 256) {
		if (T.K[s] == YK_EMPTY || (T.CN[s] & LC_EXIST)) continue;
		u32 c = T.CN[s] & LC_CMASK, Tt;
		if (!fp.bloom_mode || (T.CN[s] & LC_FP)) Tt = T.T1[s];
		else if (T.T2[s] != T32_INF) { Tt = T.T2[s]; c -= 1; }
		else continue;
		if (c > 1023) c = 1023;
		if (fp.or_mode) c = T.T1[s] & (fp.or_mode == 1 ? 15u : 1023u);   /* a key seen once per load: its flag / saved count travels in the time's low bits */
		const u32 r = atomicAdd(s_run, 1u);
		O.kc[lo + r] = (T.K[s] >> fp.pre) << 10 | c; O.T[lo + r] = fp.t_pass0 + Tt;
		if (O.c2) { const u32 n = T.CN[s] & LC_CMASK; O.c2[lo + r] = (unsigned short)(n > 1023 ? 1023 : n); }   /* every instance: the count pass's share */
	}
	lc_sync();
	if (tid == 0) { O.nsel[sb] = *s_run; O.lp[sb] = *s_lp; O.nd[sb] = *s_ndist; }
}

__global__ __launch_bounds__(256)
void k_lds_count_ovf(FastParams fp, const u64 *sbstart, const Rec *rec, u32 *bloom32, ImgView img, LcOut O,
                     const u32 *ovf_list, const u64 *scr_off, u64 *scr)
{
	__shared__ u32 s_misc[8];
	const u32 sb = ovf_list[blockIdx.x];
	const u64 n = sbstart[sb + 1] - sbstart[sb];
	u32 cap = 4096; while (cap < 2 * n) cap <<= 1;
	u64 *base = scr + scr_off[blockIdx.x];                      /* 40 B per slot = 5 u64 */
	LcTab T; T.cap = cap;
	T.K = base; T.SO = base + cap;
	T.T1 = (u32*)(base + 2 * (u64)cap); T.T2 = T.T1 + cap; T.CN = T.T2 + cap; T.SP = T.CN + cap; T.TM = T.SP + cap;
	lc_body(fp, T, sb, sbstart, rec, bloom32, img, O, s_misc);
}

/* ------------------------------------------------------------------------------------------
 * k_lc2: the first tier of the exclusive-ownership counting, built for latency: a sub-bucket's ~560
 * records keep a workgroup busy for a few thousand cycles only, nearly all of them waiting (global
 * loads, dependent LDS atomics, barriers).  So
 *   * a workgroup walks every gridDim-th sub-bucket and requests the next one's records at the top of an
 *     iteration, to take them over at the top of the next (the global latency disappears behind a whole
 *     iteration of LDS work).  The grid is 64 times what is resident (yk_launch_lc2): ~25 sub-buckets per
 *     workgroup, handed out by the dispatcher as slots free up, measured 13 % faster than 1280 workgroups
 *     walking 1640 each;
 *   * the LDS table is organised by bloom block: the home slot of a key is (block inside the staged
 *     range) x (slots per block) + a few hash bits, so the keys of one 512-bit block sit in one probe
 *     cluster and "the other keys of my block" is a short scan from the block's first slot -- no
 *     grouping passes, no per-block lists, no limit on the keys per block;
 *   * the gate of bbf.c:25-42 / htab.c:63-65 is evaluated per key, all keys in parallel (fused with the
 *     bits and the selection while the filter is untouched, see below): a key passes at
 *     its first occurrence iff each of its probe bits is set in the filter as it was before this
 *     sub-bucket or belongs to a key of the same block whose first occurrence is earlier (every
 *     instance sets its bits whatever the gate says); then all bits are ORed in (order-free);
 *   * nothing is reserved with global atomics: the selected keys go to the front of the sub-bucket's
 *     own record range in the output arrays (LcOut), k_lc_compact gathers them per sub-table.
 * Three barriers per sub-bucket.  Sub-buckets this tier cannot take (too many distinct k-mers for the
 * LDS table) are listed for k_lds_count_ovf untouched.  Needs n_hash <= 32 and, with a filter, a
 * staged range (<= 128 blocks per sub-bucket); the host falls back to k_lds_count otherwise.
 * ------------------------------------------------------------------------------------------ */
#define LC2_FULL_BF 624                   /* distinct k-mers a sub-bucket may hold with a staged filter: 32000 B of LDS per workgroup = 25 allocation granules, 5 workgroups per CU */
#define LC2_FP    0x8000u                 /* 16-bit per-key word: occurrences (12 bits, clamped) | flags */
#define LC2_EXIST 0x4000u
#define LC2_CMASK 0x0fffu

__device__ u64 d_lc2_prof[8];      /* YAKAMD_DBG & 128: shader clocks per phase, summed over the workgroups (lane 0 of each) */
/* the filter, a non-empty table image and the clock instrumentation are compile-time variants: as run-time flags they (and the fourteen
 * accumulator registers of the instrumentation) cost enough registers to spill, and a spill reload waits for every load in flight -- the next
 * sub-bucket's records among them.
 * STAGE: the sub-bucket's range of the filter is staged in LDS (s_BL).  A filter nobody has written yet whose bits nobody will read either
 * (FastParams.bf_virgin && bf_nowb: the one-slice first pass of `yak count -b` that keeps its records, main.c:53-57) needs no stage at all -- the
 * gate looks at the earlier keys of the block only and the bits would be thrown away: BLOOM && !STAGE drops the 8 KB, the zeroing and the
 * atomicOr's, and with them the limit of 128 blocks per sub-bucket (sub-buckets of twice the size: half as many level-2 stacks).
 * CAPB: log2 slots of the LDS table.  Without a filter there are no second / last times to keep, and the same 31 KB hold 2048 slots: sub-buckets
 * of up to 1200 records (1536 distinct k-mers) instead of 600 */
template <bool BLOOM, bool STAGE, int CAPB> struct Lc2Cfg {
	static constexpr u32 CAP = 1u << CAPB;
	static constexpr u32 FULL = BLOOM && STAGE ? LC2_FULL_BF : CAP / 4 * 3;
};
/* WV: workgroups per CU = waves per SIMD (4 waves per workgroup); 6 fits the 24 KB of the variant without a stage if the registers stay within 80 */
template <bool BLOOM, bool IMG, bool PROF, bool REC8, bool STAGE = BLOOM, int CAPB = 10, int WV = 5>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WV, WV)))
void k_lc2(FastParams fp, const u64 *__restrict__ sbstart, const Rec *__restrict__ rec, u32 *bloom32, ImgView img, LcOut O,
           u64 *counters, u32 *ovf_list, u32 n_sb)
{
	static_assert(!STAGE || BLOOM, "a stage without a filter");
	static_assert(!BLOOM || CAPB == 10, "the gate packs slot numbers into 10 bits");
	constexpr u32 LC2_CAP = Lc2Cfg<BLOOM, STAGE, CAPB>::CAP;
	__shared__ __attribute__((aligned(16))) u64 s_K[LC2_CAP];                        /* a block's home slots are read 16 bytes at a time: keys, first times */
	__shared__ __attribute__((aligned(16))) u32 s_T1[LC2_CAP];
	__shared__ u32 s_T2[BLOOM ? LC2_CAP : 1], s_TM[BLOOM ? LC2_CAP : 1], s_CN[LC2_CAP / 2];
	__shared__ __attribute__((aligned(16))) u32 s_BL[STAGE ? LC_BLOOM_WORDS : 4];
	__shared__ unsigned short s_list[Lc2Cfg<BLOOM, STAGE, CAPB>::FULL];              /* slots of the distinct k-mers, in claim order */
	__shared__ u32 s_misc[8];
	const u32 tid = threadIdx.x;
	constexpr bool bloom = BLOOM;
	const bool virgin = BLOOM && (!STAGE || fp.bf_virgin != 0);
	const int lb = bloom ? fp.nb - 9 - fp.s2_bits : 0;             /* log2 bloom blocks owned by a sub-bucket */
	const int rsh = CAPB - lb;                                     /* log2 table slots per block */
	const u32 R = 1u << rsh, nbw = STAGE ? 16u << lb : 0;
	const u64 lmask = (1ull << lb) - 1;
	const u32 sb0 = (u32)fp.plo << fp.s2_bits;
	u32 *s_ndist = s_misc, *s_ovf = s_misc + 1, *s_lp = s_misc + 2, *s_run = s_misc + 3;
	constexpr u32 full = Lc2Cfg<BLOOM, STAGE, CAPB>::FULL;

	auto cn_get = [&](u32 s) -> u32 { return s_CN[s >> 1] >> (16 * (s & 1)) & 0xffffu; };
	for (u32 i = tid; i < LC2_CAP; i += 256) { s_K[i] = YK_EMPTY; s_T1[i] = T32_INF; if (BLOOM) { s_T2[i] = T32_INF; s_TM[i] = 0; } }
	for (u32 i = tid; i < LC2_CAP / 2; i += 256) s_CN[i] = 0;
	if (STAGE && virgin) for (u32 i = tid; i < nbw; i += 256) s_BL[i] = 0;
	if (tid < 8) s_misc[tid] = 0;
	/* the NEXT sub-bucket's first 768 records are requested at the top of an iteration and taken over at the top of the next one: a whole
	 * iteration to arrive.  REC8: 8-byte level-2 records (fp.rec8_out), half the registers in flight */
	struct Raw8 { u64 x; };
	typedef typename std::conditional<REC8, Raw8, Rec>::type RawT;
	auto raw_at = [&](u64 i) -> RawT { RawT v; if constexpr (REC8) v.x = ((const u64*)rec)[i]; else v = rec[i]; return v; };
	/* a record as {x = hash >> pre, time}: the LDS table, the gate and the output work on x -- the prefix is the sub-table's, the same for every key of a
	 * workgroup's sub-bucket (decoding to the full hash and shifting it back was two 64-bit shifts per record and one per use) */
	auto dec = [&](const RawT v, u32 sb_) -> Rec { if constexpr (REC8) return r8_unpack_x(v.x, sb_, fp); else return make_ulonglong2(v.x >> fp.pre, v.y); };
	u32 it = blockIdx.x;
	u64 lon = 0, hin = 0;
	constexpr bool PF2 = !STAGE && WV == 5;           /* sub-buckets of more than 768 records are the rule here: the second round's records are requested ahead as well */
	RawT n0, n1, n2, n3, n4, n5;
	n0.x = 0; n1.x = 0; n2.x = 0; n3.x = 0; n4.x = 0; n5.x = 0;
	auto request = [&](u32 j) {
		lon = 0; hin = 0;
		if (j < n_sb) { lon = sbstart[sb0 + j]; hin = sbstart[sb0 + j + 1]; }
		if (lon + tid < hin) n0 = raw_at(lon + tid);
		if (lon + 256 + tid < hin) n1 = raw_at(lon + 256 + tid);
		if (lon + 512 + tid < hin) n2 = raw_at(lon + 512 + tid);
		if (PF2) {
			if (lon + 768 + tid < hin) n3 = raw_at(lon + 768 + tid);
			if (lon + 1024 + tid < hin) n4 = raw_at(lon + 1024 + tid);
			if (lon + 1280 + tid < hin) n5 = raw_at(lon + 1280 + tid);
		}
	};
	request(it);
	__syncthreads();

	auto home = [&](u64 key) -> u32 {
		/* the block's slots, then a few mixed bits: the key folded to 32 bits times the golden ratio, top bits (one quarter-rate multiply; the bits the
		 * keys of a sub-bucket share -- block, sub-bucket -- are constants under the fold) */
		const u64 x = key;
		return ((u32)(x & lmask) << rsh) | ((((u32)x ^ (u32)(x >> 32)) * 0x9E3779B9u) >> (32 - CAPB) & (R - 1));
	};
	u32 tmax = 0;

	u64 pf[7] = { 0, 0, 0, 0, 0, 0, 0 };
	while (it < n_sb) {
		const u32 sb = sb0 + it, itn = it + gridDim.x;
		const u64 lo = lon, hi = hin;
		const RawT r0 = n0, r1 = n1, r2 = n2;                             /* the only loads in flight here are these: the copies wait for exactly them */
		RawT r3, r4, r5;
		r3.x = 0; r4.x = 0; r5.x = 0;
		if (PF2) { r3 = n3; r4 = n4; r5 = n5; }
		request(itn);
		u32 *gw = bloom ? bloom32 + ((((u64)(sb >> fp.s2_bits) << fp.nb) | ((u64)(sb & ((1u << fp.s2_bits) - 1)) << (lb + 9))) >> 5) : 0;
		if (STAGE && !virgin) for (u32 i = tid; i < nbw; i += 256) s_BL[i] = gw[i];
		const bool prof = PROF && tid == 0;
		u64 tp0 = 0, tp1 = 0, tp2 = 0, tp3 = 0;
		if (prof) tp0 = __builtin_readcyclecounter();
		/* A: count; first / second / last occurrence (same loser rule as k_acc_insert) */
		tmax = 0;
		u64 tpw = 0;
		if (PROF) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (prof) tpw = __builtin_readcyclecounter(); }
		RawT a0 = r0, a1 = r1, a2 = r2;
		for (u64 base = lo; base < hi; base += 768) {
			/* the lane's (up to) three records go through the table side by side: every step is three independent LDS
			 * operations and one wait, instead of three dependent chains one after the other.  A sub-bucket of more than 768
			 * records takes further rounds of the same, their records read here (the first round's came with the prefetch) */
			if (PF2 && base == lo + 768) { a0 = r3; a1 = r4; a2 = r5; }
			else if (base != lo) {
				if (base + tid < hi) a0 = raw_at(base + tid);
				if (base + 256 + tid < hi) a1 = raw_at(base + 256 + tid);
				if (base + 512 + tid < hi) a2 = raw_at(base + 512 + tid);
			}
			const Rec rc[3] = { dec(a0, sb), dec(a1, sb), dec(a2, sb) };
			bool v[3] = { base + tid < hi, base + 256 + tid < hi, base + 512 + tid < hi }, res[3], won[3], tried[3];
			u32 sl[3], at[3], cn[3], old[3];
			u64 cur[3];
#pragma unroll
			for (int i = 0; i < 3; ++i) { sl[i] = home(rc[i].x); cur[i] = v[i] ? s_K[sl[i]] : 0; }
#pragma unroll
			for (int i = 0; i < 3; ++i) {
				res[i] = v[i] && cur[i] == rc[i].x; won[i] = false; tried[i] = v[i] && cur[i] == YK_EMPTY;
				if (tried[i]) cur[i] = atomicCAS(&s_K[sl[i]], YK_EMPTY, rc[i].x);
			}
#pragma unroll
			for (int i = 0; i < 3; ++i) if (tried[i]) { won[i] = cur[i] == YK_EMPTY; res[i] = won[i] || cur[i] == rc[i].x; }
#pragma unroll
			for (int i = 0; i < 3; ++i) if (won[i]) at[i] = atomicAdd(s_ndist, 1u);
#pragma unroll
			for (int i = 0; i < 3; ++i) if (won[i] && at[i] < full) s_list[at[i]] = (unsigned short)sl[i];
#pragma unroll
			for (int i = 0; i < 3; ++i) if (v[i] && !res[i]) {                 /* the home slot belongs to another key: walk on */
				const u64 key = rc[i].x;
				u32 q = (sl[i] + 1) & (LC2_CAP - 1), n = 1;
				for (; n < LC2_CAP; ++n, q = (q + 1) & (LC2_CAP - 1)) {
					u64 c2 = s_K[q];
					if (c2 == key) break;
					if (c2 == YK_EMPTY) {
						c2 = atomicCAS(&s_K[q], YK_EMPTY, key);
						if (c2 == YK_EMPTY) { const u32 a2 = atomicAdd(s_ndist, 1u); if (a2 < full) s_list[a2] = (unsigned short)q; break; }
						if (c2 == key) break;
					}
				}
				if (n == LC2_CAP) { *s_ovf = 1; v[i] = false; }
				sl[i] = q;
			}
#pragma unroll
			for (int i = 0; i < 3; ++i) cn[i] = v[i] ? cn_get(sl[i]) : 0;
#pragma unroll
			for (int i = 0; i < 3; ++i) if (v[i]) {
				if ((cn[i] & LC2_CMASK) < 0x800u) atomicAdd(&s_CN[sl[i] >> 1], 1u << (16 * (sl[i] & 1)));   /* only min(count, 1024) is ever used; 256 racing lanes cannot carry out of the field */
				old[i] = atomicMin(&s_T1[sl[i]], (u32)rc[i].y);
			}
#pragma unroll
			for (int i = 0; i < 3; ++i) if (v[i]) {
				const u32 t = (u32)rc[i].y;
				if (bloom) {
					if (old[i] != T32_INF) atomicMin(&s_T2[sl[i]], old[i] > t ? old[i] : t);
					atomicMax(&s_TM[sl[i]], t);
				}
				tmax = t + 1 > tmax ? t + 1 : tmax;
			}
		}
		if (!bloom && tmax) atomicMax(s_lp, tmax);                /* without a filter every instance is a put-call */
		u64 tpp = 0;
		if (prof) tpp = __builtin_readcyclecounter();
		__syncthreads();
		if (prof) tp1 = __builtin_readcyclecounter();
		const u32 ndist = *s_ndist;
		const bool give_up = *s_ovf || ndist > full;
		if (!give_up && !(fp.dbg & 16)) {
			/* B: keys already in the table image only gain counts (htab.c:66-69 on an existing key) */
			if (IMG) {
				for (u32 li = tid; li < ndist; li += 256) {
					const u32 s = s_list[li];
					const int64_t idx = img_find(img, s_K[s] << fp.pre | (sb >> fp.s2_bits));
					if (idx >= 0) {
						const u64 kc = img.keys[idx], c = (kc & 1023) + (cn_get(s) & LC2_CMASK);
						img.keys[idx] = fp.or_mode == 1 ? kc | (s_T1[s] & 15u) : fp.or_mode == 2 ? kc : (kc & ~1023ull) | (c > 1023 ? 1023 : c);
						atomicOr(&s_CN[s >> 1], LC2_EXIST << (16 * (s & 1)));
					}
				}
				__syncthreads();
			}
			/* A filter nobody has written yet (fp.bf_virgin: the whole first slice of a pass): the gate never reads the staged range, so gate, bits and
			 * selection of a key are one step of one lane -- list -> {key, count, times} -> first times of the block's eight home slots -> the few
			 * earlier keys among them -> bits, output: four or five LDS round trips instead of the two dozen of the two loops below */
			if (bloom && virgin && !(fp.dbg & 32)) {
				u32 best = 0;
				for (u32 li = tid; li < ndist; li += 256) {
					const u32 s = s_list[li];
					const u64 kx = s_K[s];
					const u32 cn = cn_get(s), t1x = s_T1[s], t2x = s_T2[s], tmx = s_TM[s];
					const bool exist = IMG && (cn & LC2_EXIST);
					bool fpk = false;
					if (!exist) {
						const BfSeq q = lc_seq_x(kx, fp);
						const u32 blk = (u32)(kx & lmask), r0s = blk << rsh;
						u32 miss = q.nd >= 32 ? 0xffffffffu : (1u << q.nd) - 1;
						u64 zp = 0, nz = 0x8000800080008000ull;                    /* n_hash <= 4: the key's probes in four 16-bit fields; field i keeps its top bit while probe i is matched by nobody */
						if (q.nd <= 4) for (u32 i = 0, z = q.h1; i < 4; ++i, z = (z + q.h2) & 511) zp |= (u64)(i < q.nd ? z : 0x3ffu) << (16 * i);
						auto cover = [&](const u64 ky) {                            /* an earlier key of the same block: its probe bits count as set */
							const BfSeq y = lc_seq_x(ky, fp);
							if (q.nd <= 4) {
								for (u32 a2 = 0, w = y.h1; a2 < y.nd; ++a2, w = (w + y.h2) & 511)
									nz &= (zp ^ (w * 0x0001000100010001ull)) + 0x7fff7fff7fff7fffull;   /* fields are < 2^10: no carry between them */
							} else {
								for (u32 a2 = 0, w = y.h1; a2 < y.nd; ++a2, w = (w + y.h2) & 511)
									for (u32 i = 0, z = q.h1; i < q.nd; ++i, z = (z + q.h2) & 511) if (z == w) miss &= ~(1u << i);
							}
						};
						u32 d = 0;
						if (R == 8) {
							/* the first times of the block's eight home slots (two 16-byte reads) say which of them hold an earlier key (an empty slot's
							 * time is infinite); only those keys are read -- a block holds less than one key on average */
							const uint4 *tb = (const uint4*)(s_T1 + r0s);
							const uint4 ta = tb[0], tc = tb[1];
							const u32 tt[8] = { ta.x, ta.y, ta.z, ta.w, tc.x, tc.y, tc.z, tc.w };
							u32 cand = 0;
#pragma unroll
							for (u32 i = 0; i < 8; ++i) cand |= (u32)(tt[i] < t1x) << i;      /* the key's own slot holds t1x itself */
							while (cand) {
								const u32 i = (u32)__ffs((int)cand) - 1;
								cand &= cand - 1;
								const u64 ky = s_K[r0s + i];
								if ((u32)(ky & lmask) == blk && !(IMG && (cn_get(r0s + i) & LC2_EXIST))) cover(ky);
							}
							d = tt[7] == T32_INF ? LC2_CAP : 8;                       /* slot 7 unused: no key of this block can sit beyond */
						} else if (R == 4) {                                          /* 256 blocks per sub-bucket (no stage): four home slots, one 16-byte read */
							const uint4 ta = *(const uint4*)(s_T1 + r0s);
							const u32 tt[4] = { ta.x, ta.y, ta.z, ta.w };
							u32 cand = 0;
#pragma unroll
							for (u32 i = 0; i < 4; ++i) cand |= (u32)(tt[i] < t1x) << i;
							while (cand) {
								const u32 i = (u32)__ffs((int)cand) - 1;
								cand &= cand - 1;
								const u64 ky = s_K[r0s + i];
								if ((u32)(ky & lmask) == blk && !(IMG && (cn_get(r0s + i) & LC2_EXIST))) cover(ky);
							}
							d = tt[3] == T32_INF ? LC2_CAP : 4;
						}
						for (; d < LC2_CAP; ++d) {
							const u32 jx = (r0s + d) & (LC2_CAP - 1);
							const u64 ky = s_K[jx];
							if (ky == YK_EMPTY) { if (d + 1 >= R) break; continue; }   /* no key of this block can sit beyond */
							if (jx == s || (u32)(ky & lmask) != blk || s_T1[jx] >= t1x || (IMG && (cn_get(jx) & LC2_EXIST))) continue;
							cover(ky);
						}
						if (q.nd <= 4) miss &= ~((u32)(~nz >> 15 & 1) | (u32)(~nz >> 30 & 2) | (u32)(~nz >> 45 & 4) | (u32)(~nz >> 60 & 8));
						fpk = miss == 0;                                            /* yak_bf_insert() == n_hash */
						if (STAGE) {
							u32 *w = s_BL + (blk << 4);
							for (u32 i = 0, z = q.h1; i < q.nd; ++i, z = (z + q.h2) & 511) atomicOr(&w[z >> 5], 1u << (z & 31));
						}
					}
					/* last put-call = last instance that is not a rejected first occurrence (htab.c:63-65) */
					if (exist || fpk || (cn & LC2_CMASK) >= 2) best = tmx + 1 > best ? tmx + 1 : best;
					if (exist) continue;
					u32 c = cn & LC2_CMASK, Tt;
					if (fpk) Tt = t1x;
					else if (t2x != T32_INF) { Tt = t2x; c -= 1; }
					else continue;
					if (c > 1023) c = 1023;
					if (fp.or_mode) c = t1x & (fp.or_mode == 1 ? 15u : 1023u);      /* a key seen once per load: its flag / saved count travels in the time's low bits */
					const u32 r = atomicAdd(s_run, 1u);
					O.kc[lo + r] = kx << 10 | c; O.T[lo + r] = fp.t_pass0 + Tt;
					if (O.c2) { const u32 n = cn & LC2_CMASK; O.c2[lo + r] = (unsigned short)(n > 1023 ? 1023 : n); }   /* clamped at >= 0x800, exact below */
				}
				if (best) atomicMax(s_lp, best);
				if (prof) tp2 = __builtin_readcyclecounter();
			} else {
			/* C: the gate, one lane per key.  First the earlier keys of the same block are collected (a short
			 * scan of the block's probe cluster), then their probe bits are matched against the key's own:
			 * for n_hash <= 4 the key's probes are packed into four 16-bit fields and one peer probe is
			 * compared with all of them at once */
			if (bloom && !(fp.dbg & 32)) {
				for (u32 li = tid; li < ndist; li += 256) {
					const u32 s = s_list[li];
					const u64 kx = s_K[s];
					if (IMG && (cn_get(s) & LC2_EXIST)) continue;
					const BfSeq q = lc_seq_x(kx, fp);
					const u32 blk = (u32)(kx & lmask), t1x = s_T1[s];
					u32 miss = q.nd >= 32 ? 0xffffffffu : (1u << q.nd) - 1;
					if (!virgin) {
						const u32 *w = s_BL + (blk << 4);
						for (u32 i = 0, z = q.h1; i < q.nd; ++i, z = (z + q.h2) & 511) if (w[z >> 5] >> (z & 31) & 1) miss &= ~(1u << i);
					}
					u64 peers = 0; u32 np = 0;                                    /* up to 6 slot numbers of 10 bits */
					const u32 r0s = blk << rsh;
					auto consider = [&](const u32 j, const u64 ky) {
						if (j == s || (u32)(ky & lmask) != blk || s_T1[j] >= t1x || (IMG && (cn_get(j) & LC2_EXIST))) return;
						if (np < 6) peers |= (u64)j << (10 * np);
						else {                                                      /* a crowded block: the plain way */
							const BfSeq y = lc_seq_x(ky, fp);
							for (u32 a2 = 0, w = y.h1; a2 < y.nd; ++a2, w = (w + y.h2) & 511)
								for (u32 i = 0, z = q.h1; i < q.nd; ++i, z = (z + q.h2) & 511) if (z == w) miss &= ~(1u << i);
						}
						++np;
					};
					u32 d = 0;
					if (R == 8 && miss) {                                         /* the block's eight home slots with four 16-byte reads, no dependent chain */
						const ulonglong2 *kb = (const ulonglong2*)(s_K + r0s);
						const ulonglong2 q0 = kb[0], q1 = kb[1], q2 = kb[2], q3 = kb[3];
						const u64 kk[8] = { q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y };
#pragma unroll
						for (u32 i = 0; i < 8; ++i) if (kk[i] != YK_EMPTY) consider(r0s + i, kk[i]);
						d = kk[7] == YK_EMPTY ? LC2_CAP : 8;                        /* slot 7 unused: no key of this block can sit beyond */
					}
					for (; miss && d < LC2_CAP; ++d) {
						const u32 j = (r0s + d) & (LC2_CAP - 1);
						const u64 ky = s_K[j];
						if (ky == YK_EMPTY) { if (d + 1 >= R) break; continue; }     /* no key of this block can sit beyond */
						consider(j, ky);
					}
					if (np > 6) np = 6;
					if (miss && np) {
						if (q.nd <= 4) {
							u64 zp = 0;
							for (u32 i = 0, z = q.h1; i < 4; ++i, z = (z + q.h2) & 511) zp |= (u64)(i < q.nd ? z : 0x3ffu) << (16 * i);
							u64 nz = 0x8000800080008000ull;                        /* field i keeps its top bit while probe i is matched by nobody */
							for (u32 e = 0; e < np; ++e) {
								const BfSeq y = lc_seq_x(s_K[(u32)(peers >> (10 * e)) & 1023u], fp);
								for (u32 a2 = 0, w = y.h1; a2 < y.nd; ++a2, w = (w + y.h2) & 511)
									nz &= (zp ^ (w * 0x0001000100010001ull)) + 0x7fff7fff7fff7fffull;   /* fields are < 2^10: no carry between them */
							}
							const u32 cov = (u32)(~nz >> 15 & 1) | (u32)(~nz >> 30 & 2) | (u32)(~nz >> 45 & 4) | (u32)(~nz >> 60 & 8);
							miss &= ~cov;
						} else {
							for (u32 e = 0; e < np; ++e) {
								const BfSeq y = lc_seq_x(s_K[(u32)(peers >> (10 * e)) & 1023u], fp);
								for (u32 a2 = 0, w = y.h1; a2 < y.nd; ++a2, w = (w + y.h2) & 511)
									for (u32 i = 0, z = q.h1; i < q.nd; ++i, z = (z + q.h2) & 511) if (z == w) miss &= ~(1u << i);
							}
						}
					}
					if (miss == 0) atomicOr(&s_CN[s >> 1], LC2_FP << (16 * (s & 1)));   /* yak_bf_insert() == n_hash */
				}
				if (!virgin) __syncthreads();                                  /* every gate has read the filter as it was */
			}
			if (prof) tp2 = __builtin_readcyclecounter();
			/* C' + D + E: set the bits, last put-call, keys entering the table */
			u32 best = 0;
			for (u32 li = tid; li < ndist; li += 256) {
				const u32 s = s_list[li];
				const u64 kx = s_K[s];
				const u32 cn = cn_get(s);
				if (bloom && !(fp.dbg & 32)) {
					if (!IMG || !(cn & LC2_EXIST)) {
						const BfSeq q = lc_seq_x(kx, fp);
						u32 *w = s_BL + ((u32)(kx & lmask) << 4);
						for (u32 i = 0, z = q.h1; i < q.nd; ++i, z = (z + q.h2) & 511) atomicOr(&w[z >> 5], 1u << (z & 31));
					}
					/* last put-call = last instance that is not a rejected first occurrence (htab.c:63-65) */
					if ((cn & ((IMG ? LC2_EXIST : 0u) | LC2_FP)) || (cn & LC2_CMASK) >= 2) best = s_TM[s] + 1 > best ? s_TM[s] + 1 : best;
				}
				if (IMG && (cn & LC2_EXIST)) continue;
				u32 c = cn & LC2_CMASK, Tt;
				if (!bloom || (cn & LC2_FP)) Tt = s_T1[s];
				else if (s_T2[s] != T32_INF) { Tt = s_T2[s]; c -= 1; }
				else continue;
				if (c > 1023) c = 1023;
				if (fp.or_mode) c = s_T1[s] & (fp.or_mode == 1 ? 15u : 1023u);       /* a key seen once per load: its flag / saved count travels in the time's low bits */
				const u32 r = atomicAdd(s_run, 1u);
				O.kc[lo + r] = kx << 10 | c; O.T[lo + r] = fp.t_pass0 + Tt;
				if (O.c2) { const u32 n = cn & LC2_CMASK; O.c2[lo + r] = (unsigned short)(n > 1023 ? 1023 : n); }
			}
			if (best) atomicMax(s_lp, best);
			}
		}
		__syncthreads();
		if (prof) tp3 = __builtin_readcyclecounter();
		/* write-back, per-sub-bucket results, clean tables for the next sub-bucket */
		if (give_up) {
			if (virgin) for (u32 i = tid; i < (16u << lb); i += 256) gw[i] = 0;       /* the next tier expects real zeros (it works on the filter in memory) */
			if (tid == 0) { ovf_list[atomicAdd(&counters[YKC_NOVF2], 1ull)] = sb; O.nsel[sb] = 0; O.lp[sb] = 0; O.nd[sb] = 0; }
		} else {
			if (STAGE && !(fp.dbg & 64) && !fp.bf_nowb) {                    /* 16 bytes per lane and step; an untouched filter's stage is zeroed for the next sub-bucket on the way */
				uint4 *g4 = (uint4*)gw, *b4 = (uint4*)s_BL;
				for (u32 i = tid; i < nbw / 4; i += 256) { g4[i] = b4[i]; if (virgin) b4[i] = make_uint4(0, 0, 0, 0); }
			}
			if (tid == 0) { O.nsel[sb] = *s_run; O.lp[sb] = *s_lp; O.nd[sb] = ndist; }
		}
		if (tid == 0) { s_misc[0] = 0; s_misc[1] = 0; s_misc[2] = 0; s_misc[3] = 0; }
		if (give_up) {
			for (u32 i = tid; i < LC2_CAP; i += 256) { s_K[i] = YK_EMPTY; s_T1[i] = T32_INF; if (BLOOM) { s_T2[i] = T32_INF; s_TM[i] = 0; } }
			for (u32 i = tid; i < LC2_CAP / 2; i += 256) s_CN[i] = 0;
		} else for (u32 li = tid; li < ndist; li += 256) {
			const u32 s = s_list[li];
			s_K[s] = YK_EMPTY; s_T1[s] = T32_INF; s_CN[s >> 1] = 0;
			if (BLOOM) { s_T2[s] = T32_INF; s_TM[s] = 0; }
		}
		if (STAGE && virgin && (give_up || (fp.dbg & 64) || fp.bf_nowb)) for (u32 i = tid; i < nbw; i += 256) s_BL[i] = 0;
		it = itn;
		__syncthreads();
		if (prof) {
			const u64 tp4 = __builtin_readcyclecounter();
			pf[0] += tp1 - tp0; pf[1] += tp2 > tp1 ? tp2 - tp1 : 0; pf[2] += tp3 - (tp2 > tp1 ? tp2 : tp1);
			pf[3] += tp4 - tp3; pf[4] += 1; pf[5] += tpw - tp0; pf[6] += tpp - tpw;
		}
	}
	if (PROF && tid == 0) for (int i = 0; i < 7; ++i) atomicAdd(&d_lc2_prof[i], pf[i]);
}

/* The filter of a pass whose write-back k_lc2 skipped (FastParams.bf_nowb: a filtered count's first pass is followed by yak_ch_destroy_bf, main.c:55 --
 * 16 GiB written for nobody), rebuilt from the pass's retained sub-bucket records if something does read it after all: every instance sets its
 * probe bits whatever the gate said (bbf.c:34-40), so the filter is the OR of the bits of every record.  One workgroup per sub-bucket, its range of
 * blocks staged in LDS as in k_lc2 (<= 128 blocks); the caller has zeroed the filter */
__global__ __launch_bounds__(256)
void k_bf_rebuild(FastParams fp, const u64 *__restrict__ sbstart, const Rec *__restrict__ rec, u32 *bloom32, u32 n_sb)
{
	__shared__ __attribute__((aligned(16))) u32 s_BL[2 * LC_BLOOM_WORDS];             /* k_lc2 without a stage takes sub-buckets of up to 256 blocks */
	const u32 tid = threadIdx.x, sb0 = (u32)fp.plo << fp.s2_bits;
	const int lb = fp.nb - 9 - fp.s2_bits;
	const u32 nbw = 16u << lb;
	const u64 lmask = (1ull << lb) - 1;
	for (u32 it = blockIdx.x; it < n_sb; it += gridDim.x) {
		const u32 sb = sb0 + it;
		const u64 lo = sbstart[sb], hi = sbstart[sb + 1];
		if (lo == hi) continue;                                            /* (uniform) nothing maps here: the zeros stay */
		for (u32 i = tid; i < nbw; i += 256) s_BL[i] = 0;
		__syncthreads();
		for (u64 i = lo + tid; i < hi; i += 256) {
			const Rec rc = lc_rec(fp, rec, i, sb);
			const BfSeq q = lc_seq(rc.x, fp);
			u32 *w = s_BL + ((u32)((rc.x >> fp.pre) & lmask) << 4);
			for (u32 j = 0, z = q.h1; j < q.nd; ++j, z = (z + q.h2) & 511) atomicOr(&w[z >> 5], 1u << (z & 31));
		}
		__syncthreads();
		u32 *gw = bloom32 + ((((u64)(sb >> fp.s2_bits) << fp.nb) | ((u64)(sb & ((1u << fp.s2_bits) - 1)) << (lb + 9))) >> 5);
		uint4 *g4 = (uint4*)gw, *b4 = (uint4*)s_BL;
		for (u32 i = tid; i < nbw / 4; i += 256) g4[i] = b4[i];
		__syncthreads();
	}
}

/* ------------------------------------------------------------------------------------------
 * k_cnt2: the count pass (create_new = 0, reference htab.c:71-75) over the SAME input as the pass before, on the records that pass left
 * grouped by sub-bucket (the level-2 partition) and on the list of keys every sub-bucket put into the table.  All instances of a k-mer sit
 * in one sub-bucket, so a workgroup owns the counters of its sub-bucket's keys outright: the keys go into a small LDS set, the records are
 * streamed once (one LDS lookup, one LDS increment per hit), and every key then adds its count to its slot of the table image (one table
 * probe per KEY instead of one per instance; exclusive owner: a plain read-modify-write).  Persistent workgroups with the next sub-bucket's
 * first records in flight, as in k_lc2.  A sub-bucket with more keys than the LDS set takes (other tiers of the insert kernel) looks every
 * instance up in the image with device atomics.  k_img_fold saturates the counts afterwards.
 * k_lc2 owned the same sub-buckets of the same records and had these counts in LDS already: it hands them out (LcOut.c2), and the count pass
 * is then k_cnt2_apply alone.  k_cnt2 stays for a pass 1 that did not keep them (engine_slice.cpp: YAKAMD_CNT2_FUSED=0).
 * ------------------------------------------------------------------------------------------ */
/* C2_CAP slots for up to C2_FULL keys: 2048 / 1280 hold whatever k_lc2 lets through (28 KB of LDS, six workgroups per CU); reads with
 * coverage put a few dozen keys into a sub-bucket, and 512 / 320 (7 KB) lets the CU's wave slots, eight workgroups, be the limit */
template <int C2_CAP, int C2_FULL>
__global__ __launch_bounds__(256)
void k_cnt2(FastParams fp, const u64 *__restrict__ sbstart, const Rec *__restrict__ rec, const u64 *__restrict__ key_off, const u64 *__restrict__ key_kc,
            ImgView img, u32 n_sb, u32 *__restrict__ key_cnt, u32 *used_delta)
{
	__shared__ u64 s_K[C2_CAP];
	__shared__ u32 s_C[C2_CAP];
	__shared__ unsigned short s_slot[C2_FULL];
	const u32 tid = threadIdx.x;
	const u32 sb0 = (u32)fp.plo << fp.s2_bits;
	for (u32 i = tid; i < C2_CAP; i += 256) { s_K[i] = YK_EMPTY; s_C[i] = 0; }
	auto home = [&](u64 x) -> u32 { return (((u32)x ^ (u32)(x >> 32)) * 0x9E3779B9u) >> 20 & (C2_CAP - 1); };   /* one quarter-rate multiply instead of the three of a 64-bit product */
	/* 8-byte records only (the retained level-2 records always are: engine_slice.cpp keep2).  The NEXT sub-bucket's first 768 records and first 256 keys
	 * (a sub-bucket of reads holds a few dozen) are requested at the top of an iteration and taken over at its end: a whole iteration to arrive */
	const u64 *rec8 = (const u64*)rec;
	u32 it = blockIdx.x;
	u64 lon = 0, hin = 0, kon = 0;
	u32 nkn = 0;
	u64 n0 = 0, n1 = 0, n2 = 0, kn = 0;
	auto request = [&](u32 j) {                                        /* sub-bucket j of this workgroup's walk -> the n registers */
		lon = hin = kon = 0; nkn = 0;
		if (j < n_sb) { lon = sbstart[sb0 + j]; hin = sbstart[sb0 + j + 1]; kon = key_off[sb0 + j]; nkn = (u32)(key_off[sb0 + j + 1] - kon); }
		if (tid < nkn) kn = key_kc[kon + tid];
		if (lon + tid < hin) n0 = rec8[lon + tid];
		if (lon + 256 + tid < hin) n1 = rec8[lon + 256 + tid];
		if (lon + 512 + tid < hin) n2 = rec8[lon + 512 + tid];
	};
	request(it);
	__syncthreads();
	while (it < n_sb) {
		/* take over what was requested an iteration ago (the only loads in flight here: the copies wait for exactly those), then request the next */
		const u32 sb = sb0 + it, itn = it + gridDim.x, nk = nkn;
		const u64 lo = lon, hi = hin, ko = kon;
		const u64 r0 = n0, r1 = n1, r2 = n2, kpre = kn;
		request(itn);
		const bool in_lds = nk <= C2_FULL;
		if (in_lds) {
			for (u32 i = tid; i < nk; i += 256) {                            /* the keys this sub-bucket put into the table */
				const u64 x = (i < 256 ? kpre : key_kc[ko + i]) >> 10;
				u32 s = home(x);
				for (;;) {
					const u64 cur = atomicCAS(&s_K[s], YK_EMPTY, x);
					if (cur == YK_EMPTY || cur == x) break;
					s = (s + 1) & (C2_CAP - 1);
				}
				s_slot[i] = (unsigned short)s;
			}
			__syncthreads();
		}
		auto take = [&](const u64 raw) {
			const Rec rc = r8_unpack(raw, sb, fp);
			if (in_lds) {
				const u64 x = rc.x >> fp.pre;
				u32 s = home(x);
				for (;;) {
					const u64 cur = s_K[s];
					if (cur == x) { atomicAdd(&s_C[s], 1u); break; }
					if (cur == YK_EMPTY) break;
					s = (s + 1) & (C2_CAP - 1);
				}
			} else {
				const int64_t idx = img_find(img, rc.x);
				if (idx >= 0) { atomicAdd(&img.delta[idx], 1u); *used_delta = 1; }   /* (the host then folds the pending counts in: k_img_fold) */
			}
		};
		if (lo + tid < hi) take(r0);
		if (lo + 256 + tid < hi) take(r1);
		if (lo + 512 + tid < hi) take(r2);
		for (u64 i = lo + 768 + tid; i < hi; i += 256) take(rec8[i]);
		__syncthreads();
		if (in_lds) {
			/* the counts go out next to the keys (coalesced); k_cnt2_apply adds them to the table image, one lane per key: the table probe is a chain
			 * of dependent global reads that a couple of dozen lanes of this workgroup would wait for at every sub-bucket */
			for (u32 i = tid; i < nk; i += 256) { const u32 s = s_slot[i]; key_cnt[ko + i] = s_C[s]; s_K[s] = YK_EMPTY; s_C[s] = 0; }
		} else for (u32 i = tid; i < nk; i += 256) key_cnt[ko + i] = 0;    /* counted straight into the image */
		it = itn;
		__syncthreads();
	}
}

/* counts of k_cnt2 -> table image: key i of sub-table p (the list is grouped by sub-table: seg_base).
 * fix: the image's counts have been raised by one already (k_img_clear's bump) from the counts c1 the pass before left, which the list still holds
 * (key_kc[i] & 1023).  That is the key's count key_cnt[i] wherever the pass before counted every instance but the first -- every key but the few
 * whose first instance the filter let through (k_lc2: fpk) -- so a key is skipped when key_cnt[i] == min(c1 + 1, 1023), and only the others are
 * probed and get key_cnt[i] as their count */
__global__ __launch_bounds__(256)
void k_cnt2_apply(const u64 *__restrict__ key_kc, const u32 *__restrict__ key_cnt, const u64 *__restrict__ seg_base, int plo, int pre, ImgView img, int fix)
{
	const u32 p = (u32)plo + blockIdx.y;
	const u64 a = seg_base[p], b = seg_base[p + 1];
	for (u64 i = a + (u64)blockIdx.x * 256 + threadIdx.x; i < b; i += (u64)gridDim.x * 256) {
		const u32 c = key_cnt[i];
		if (fix) {
			const u32 c1 = (u32)key_kc[i] & 1023u;
			if (c == (c1 < 1023u ? c1 + 1 : 1023u)) continue;
		} else if (!c) continue;
		/* the probe reads the key array alone: the image keeps every unused slot at YK_EMPTY, which no 2k < 64-bit key equals (as k_lookup; this
		 * path only exists for k < 32) -- the `used` bitmap would be a second random read per step of the probe */
		const u64 kid = key_kc[i] >> 10;
		const u32 bits = img.bits[p];
		if (bits == YK_NOCAP) continue;
		const u64 *keys = img.keys + img.off[p];
		const u32 nmask = (1u << bits) - 1;
		u32 s = yk_h2b((u32)kid, bits);
		const u32 first = s;
		for (;;) {
			const u64 kc = keys[s];
			if (kc == YK_EMPTY) break;
			if (kc >> 10 == kid) {                                            /* a key occurs once in the list: nobody else touches its slot -- the count goes in at once, saturated (htab.c:73-74) */
				const u64 n = fix ? c : (kc & 1023) + c;
				yk_global_rw(u64, img.keys)[img.off[p] + s] = (kc & ~1023ull) | (n > 1023 ? 1023 : n);
				break;
			}
			s = (s + 1) & nmask;
			if (s == first) break;
		}
	}
}

/* first key of every sub-bucket in the gathered (unsorted) key list: seg_base[p] + exclusive scan of nsel inside sub-table p; key_off[n_sb] = all keys */
__global__ __launch_bounds__(256)
void k_nsel_scan(const u32 *__restrict__ nsel, int s2_bits, int plo, int phi, int P, const u64 *__restrict__ seg_base, u64 *__restrict__ key_off)
{
	__shared__ u32 s_w[5];
	const u32 p = blockIdx.x, S2 = 1u << s2_bits, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const size_t b0 = (size_t)p * S2;
	const bool mine = (int)p >= plo && (int)p < phi;
	u64 run = seg_base[p];
	for (u32 j0 = 0; j0 < S2; j0 += 256) {
		__syncthreads();
		const u32 j = j0 + tid, n = (mine && j < S2) ? nsel[b0 + j] : 0;
		u32 incl = n;
		for (int o = 1; o < 64; o <<= 1) { const u32 x = __shfl_up(incl, o); if (lane >= (u32)o) incl += x; }
		if (lane == 63) s_w[wave] = incl;
		__syncthreads();
		u32 e = incl - n, tot = 0;
		for (u32 w = 0; w < 4; ++w) { if (w < wave) e += s_w[w]; tot += s_w[w]; }
		if (j < S2) key_off[b0 + j] = run + e;
		run += tot;
	}
	if ((int)p == P - 1 && tid == 0) key_off[(size_t)P * S2] = run;
}

/* keys selected per sub-table = sum over its sub-buckets */
__global__ __launch_bounds__(256)
void k_lc_sum(const u32 *__restrict__ nsel, int s2_bits, int plo, u32 *seg_cnt)
{
	__shared__ u32 s_tot;
	const u32 p = (u32)plo + blockIdx.x, S2 = 1u << s2_bits;
	if (threadIdx.x == 0) s_tot = 0;
	__syncthreads();
	u32 c = 0;
	for (u32 j = threadIdx.x; j < S2; j += 256) c += nsel[(size_t)p * S2 + j];
	for (int o = 32; o; o >>= 1) c += __shfl_down(c, o);
	if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_tot, c);
	__syncthreads();
	if (threadIdx.x == 0) seg_cnt[p] = s_tot;
}

/* The gather for many sub-buckets per sub-table or few sub-tables (a shard of a multi-GPU job: 128 sub-tables x 2^17 sub-buckets): one workgroup per
 * sub-table walking its sub-buckets one after the other (k_lc_compact) would leave most of the chip idle.  k_lc_sum3 reduces what the gather needs per
 * sub-table (keys selected, last put-call, distinct k-mers), k_nsel_scan gives every sub-bucket its place in the list, k_lc_gather copies the
 * fragments, a wave per sub-bucket over the whole grid.  Same list, in the same order, as k_lc_compact writes */
__global__ __launch_bounds__(256)
void k_lc_sum3(LcOut O, int s2_bits, int plo, u64 t_pass0, u32 *seg_cnt, u64 *lastput, u32 *ndist_p)
{
	__shared__ u32 s_red[3];
	const u32 p = (u32)plo + blockIdx.x, S2 = 1u << s2_bits, tid = threadIdx.x;
	const size_t b0 = (size_t)p * S2;
	if (tid < 3) s_red[tid] = 0;
	__syncthreads();
	u32 c = 0, lpm = 0, nds = 0;
	for (u32 j = tid; j < S2; j += 256) { c += O.nsel[b0 + j]; const u32 l = O.lp[b0 + j]; lpm = l > lpm ? l : lpm; nds += O.nd[b0 + j]; }
	for (int o = 32; o; o >>= 1) { c += __shfl_down(c, o); nds += __shfl_down(nds, o); const u32 x = __shfl_down(lpm, o); lpm = x > lpm ? x : lpm; }
	if ((tid & 63) == 0) { if (c) atomicAdd(&s_red[0], c); if (lpm) atomicMax(&s_red[1], lpm); if (nds) atomicAdd(&s_red[2], nds); }
	__syncthreads();
	if (tid == 0) {
		seg_cnt[p] = s_red[0]; ndist_p[p] += s_red[2];
		if (s_red[1]) { const u64 v = t_pass0 + (u64)s_red[1]; if (v > lastput[p]) lastput[p] = v; }
	}
}

__global__ __launch_bounds__(256)
void k_lc_gather(LcOut O, const u64 *__restrict__ sbstart, const u64 *__restrict__ key_off, u32 sb_lo, u32 n_sb, u64 *__restrict__ out_kc, u64 *__restrict__ out_T, Rec *__restrict__ out_kt,
                 u32 *__restrict__ out_c2)
{
	const u32 lane = threadIdx.x & 63, n_waves = gridDim.x * 4;
	/* 64 sub-buckets per step: lane l looks up where sub-bucket j0 + l lies, then the wave copies them one after the other */
	for (u32 j0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; j0 < n_sb; j0 += n_waves * 64) {
		const u32 j = j0 + lane;
		u32 cnt = 0; u64 src = 0, dst = 0;
		if (j < n_sb) { cnt = O.nsel[sb_lo + j]; src = sbstart[sb_lo + j]; dst = key_off[sb_lo + j]; }
		u64 any = __ballot(cnt != 0);
		while (any) {
			const int l = __ffsll((long long)any) - 1;
			any &= any - 1;
			const u32 n = __shfl(cnt, l);
			const u64 a = __shfl(src, l), d = __shfl(dst, l);
			if (out_kt) for (u32 i = lane; i < n; i += 64) out_kt[d + i] = make_ulonglong2(O.kc[a + i], O.T[a + i]);     /* {key, time} pairs for the sort */
			else for (u32 i = lane; i < n; i += 64) { out_kc[d + i] = O.kc[a + i]; out_T[d + i] = O.T[a + i]; }
			if (out_c2) for (u32 i = lane; i < n; i += 64) out_c2[d + i] = O.c2[a + i];                                 /* the count pass's counts, same order */
		}
	}
}

/* {key, time} pairs -> the two arrays the layout stage reads (out_t may be 0) */
__global__ __launch_bounds__(256)
void k_kt_split(const Rec *__restrict__ in, u64 n, u64 *__restrict__ out_kc, u64 *__restrict__ out_t)
{
	for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) { const Rec r = in[i]; out_kc[i] = r.x; if (out_t) out_t[i] = r.y; }
}

/* ------------------------------------------------------------------------------------------
 * The sort by insertion time, second half.  Times are unique inside a sub-table (ranks in its stream, or stream positions), and the partition
 * sweep before this kernel (k_part2<.., TS>) has grouped a sub-table's {key, time} pairs by the top bits of the time: bin j holds the times
 * [j 2^w, (j + 1) 2^w), so it holds at most 2^w keys and -- the bins being in time order -- its keys end up exactly where the bin lies.  Inside a
 * bin the order follows without comparing anything: every key sets bit (time mod 2^w) of a bitmap in LDS, a prefix count of the set bits gives
 * every key its rank.  The keys are put in order in LDS and leave as whole lines; a bin with more keys than the stage holds stores them one by one.
 * A time seen twice raises *fail (the caller then sorts the old way).
 * ------------------------------------------------------------------------------------------ */
#define TSR_R 8                            /* records a lane holds in registers: bins of up to 2048 keys never read their input twice */
/* The partition's bins are 2^w times wide, w <= 11 where the number of bins allows it: such a bin can never hold more than the stage does, however
 * dense the times (first occurrences pile up at the start of a stream of reads: its first bins are full, the later ones nearly empty).  A workgroup
 * takes 2^j neighbouring bins at once -- still one contiguous run of keys and of times -- when together they fit the registers and the stage, and
 * bin after bin from memory when they do not */
__global__ __launch_bounds__(256)
void k_ts_rank(const u64 *__restrict__ binstart, const Rec *__restrict__ in, int w, int j, u32 bin_lo, u32 n_super, u64 *__restrict__ out_kc, u64 *__restrict__ out_t, u32 *fail, u32 cap)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];
	__shared__ u32 s_w[4];
	const int ws = w + j;
	const u32 nW = ws > 6 ? 1u << (ws - 5) : 2u, nWf = w > 6 ? 1u << (w - 5) : 2u, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	u32 *s_bm = s_dyn, *s_pf = s_dyn + nW;
	Rec *s_st = (Rec*)(s_dyn + 2 * nW);
	for (u32 i = tid; i < nW; i += 256) s_bm[i] = 0;
	/* a workgroup walks every gridDim-th group of bins; the NEXT group's keys are requested at the top of an iteration (k_lc2's scheme) */
	u64 na = 0; u32 nc = 0;
	Rec nr[TSR_R];
#pragma unroll
	for (int q = 0; q < TSR_R; ++q) nr[q] = make_ulonglong2(0, 0);
	auto request = [&](u32 g) {
		nc = 0; na = 0;
		if (g < n_super) { na = binstart[bin_lo + ((u64)g << j)]; nc = (u32)(binstart[bin_lo + ((u64)(g + 1) << j)] - na); }
		if (nc <= 256u * TSR_R) {
#pragma unroll
			for (int q = 0; q < TSR_R; ++q) if ((u32)q * 256 + tid < nc) nr[q] = yk_global_rec(in, na + (u32)q * 256 + tid);
		}
	};
	auto scan = [&](const u32 nw) {                            /* exclusive prefix of the words' bit counts: `per` consecutive words per lane */
		const u32 per = (nw + 255) / 256;
		u32 sum = 0;
		for (u32 q = 0; q < per; ++q) { const u32 x = tid * per + q; if (x < nw) sum += __popc(s_bm[x]); }
		u32 incl = sum;
		for (int o = 1; o < 64; o <<= 1) { const u32 y = __shfl_up(incl, o); if (lane >= (u32)o) incl += y; }
		if (lane == 63) s_w[wave] = incl;
		__syncthreads();
		u32 e = incl - sum;
		for (u32 q = 0; q < wave; ++q) e += s_w[q];
		for (u32 q = 0; q < per; ++q) { const u32 x = tid * per + q; if (x < nw) { s_pf[x] = e; e += __popc(s_bm[x]); } }
	};
	u32 g = blockIdx.x;
	request(g);
	__syncthreads();
	while (g < n_super) {
		const u64 a = na;
		const u32 c = nc, nxt = g + gridDim.x;
		Rec r[TSR_R];
#pragma unroll
		for (int q = 0; q < TSR_R; ++q) r[q] = nr[q];
		request(nxt);
		if (c != 0 && c <= 256u * TSR_R && c <= cap) {               /* (uniform) the keys are in registers */
			const u32 tmask = (1u << ws) - 1;
#pragma unroll
			for (int q = 0; q < TSR_R; ++q) if ((u32)q * 256 + tid < c) {
				const u32 t = (u32)r[q].y & tmask;
				const u32 old = atomicOr(&s_bm[t >> 5], 1u << (t & 31));
				if (old >> (t & 31) & 1) *fail = 1;
			}
			__syncthreads();
			scan(nW);
			__syncthreads();
#pragma unroll
			for (int q = 0; q < TSR_R; ++q) if ((u32)q * 256 + tid < c) {
				const u32 t = (u32)r[q].y & tmask;
				s_st[s_pf[t >> 5] + __popc(s_bm[t >> 5] & ((1u << (t & 31)) - 1))] = r[q];
			}
			__syncthreads();
			for (u32 i = tid; i < c; i += 256) { const Rec x = s_st[i]; out_kc[a + i] = x.x; out_t[a + i] = x.y; }
#pragma unroll
			for (int q = 0; q < TSR_R; ++q) if ((u32)q * 256 + tid < c) s_bm[((u32)r[q].y & tmask) >> 5] = 0;   /* a clean bitmap for the next group */
			__syncthreads();
		} else if (c != 0) {
			/* too many keys for one go: bin after bin, from memory; a bin wider than the stage (w > 11: more bins than one partition sweep takes)
			 * fills it window after window, reading its keys once more per window */
			const u32 tmask = (1u << w) - 1;
			for (u32 f = 0; f < (1u << j); ++f) {
				const u64 fa = binstart[bin_lo + ((u64)g << j) + f];
				const u32 fc = (u32)(binstart[bin_lo + ((u64)g << j) + f + 1] - fa);
				if (fc == 0) continue;
				for (u32 i = tid; i < fc; i += 256) {
					const u32 t = (u32)yk_global_rec(in, fa + i).y & tmask;
					const u32 old = atomicOr(&s_bm[t >> 5], 1u << (t & 31));
					if (old >> (t & 31) & 1) *fail = 1;
				}
				__syncthreads();
				scan(nWf);
				__syncthreads();
				for (u32 w0 = 0; w0 < fc; w0 += cap) {
					for (u32 i = tid; i < fc; i += 256) {
						const Rec x = yk_global_rec(in, fa + i);
						const u32 t = (u32)x.y & tmask;
						const u32 rank = s_pf[t >> 5] + __popc(s_bm[t >> 5] & ((1u << (t & 31)) - 1));
						if (rank - w0 < cap) s_st[rank - w0] = x;
					}
					__syncthreads();
					const u32 wn = fc - w0 < cap ? fc - w0 : cap;
					for (u32 i = tid; i < wn; i += 256) { const Rec x = s_st[i]; out_kc[fa + w0 + i] = x.x; out_t[fa + w0 + i] = x.y; }
					__syncthreads();
				}
				for (u32 i = tid; i < nWf; i += 256) s_bm[i] = 0;
				__syncthreads();
			}
		}
		g = nxt;
	}
}

/* gather the fragments of one sub-table into its contiguous list (any order: the sort by insertion time
 * follows); last put-call and distinct k-mers of the sub-table */
__global__ __launch_bounds__(256)
void k_lc_compact(LcOut O, const u64 *__restrict__ sbstart, int s2_bits, int plo, u64 t_pass0, const u64 *__restrict__ seg_base,
                  u64 *__restrict__ out_kc, u64 *__restrict__ out_T, u64 *lastput, u32 *ndist_p, Rec *__restrict__ out_kt, u32 *__restrict__ out_c2)
{
	__shared__ u32 s_off[256], s_red[2];
	const u32 p = (u32)plo + blockIdx.x, S2 = 1u << s2_bits, tid = threadIdx.x, lane = tid & 63;
	const size_t b0 = (size_t)p * S2;
	if (tid < 2) s_red[tid] = 0;
	u64 run = seg_base[p];
	u32 lpm = 0, nds = 0;
	for (u32 j0 = 0; j0 < S2; j0 += 256) {
		__syncthreads();
		const u32 j = j0 + tid, n = j < S2 ? O.nsel[b0 + j] : 0;
		if (j < S2) { const u32 l = O.lp[b0 + j]; lpm = l > lpm ? l : lpm; nds += O.nd[b0 + j]; }
		s_off[tid] = n;
		__syncthreads();
		if (tid < 64) {                                            /* exclusive scan of 256 counts by one wave */
			u32 v[4], t = 0;
			for (int q = 0; q < 4; ++q) { v[q] = s_off[4 * tid + q]; t += v[q]; }
			u32 incl = t;
			for (int o = 1; o < 64; o <<= 1) { const u32 x = __shfl_up(incl, o); if (lane >= (u32)o) incl += x; }
			u32 e = incl - t;
			for (int q = 0; q < 4; ++q) { s_off[4 * tid + q] = e; e += v[q]; }
			if (tid == 63) s_red[1] = incl;
		}
		__syncthreads();
		/* one wave per sub-bucket */
		for (u32 q = tid >> 6; q < 256 && j0 + q < S2; q += 4) {
			const u32 cnt = O.nsel[b0 + j0 + q];
			const u64 src = sbstart[b0 + j0 + q], dst = run + s_off[q];
			if (out_kt) for (u32 i = lane; i < cnt; i += 64) out_kt[dst + i] = make_ulonglong2(O.kc[src + i], O.T[src + i]);
			else for (u32 i = lane; i < cnt; i += 64) { out_kc[dst + i] = O.kc[src + i]; out_T[dst + i] = O.T[src + i]; }
			if (out_c2) for (u32 i = lane; i < cnt; i += 64) out_c2[dst + i] = O.c2[src + i];
		}
		run += s_red[1];
	}
	for (int o = 32; o; o >>= 1) { const u32 x = __shfl_down(lpm, o); lpm = x > lpm ? x : lpm; nds += __shfl_down(nds, o); }
	__syncthreads();
	if (lane == 0) { atomicMax(&s_red[0], lpm); atomicAdd(&ndist_p[p], nds); }
	__syncthreads();
	if (tid == 0 && s_red[0]) { const u64 v = t_pass0 + (u64)s_red[0]; if (v > lastput[p]) lastput[p] = v; }
}

