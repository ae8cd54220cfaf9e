/* kern_layout.inc -- part of kernels.hip (one translation unit, included in this order): per sub-table sort by insertion time; k_replay: exact khashl layout of tables up to 8 Ki slots (placement stages + doublings) */
/* ------------------------------------------------------------------------------------------
 * per sub-table stable LSD radix sort pass (8-bit digit of T), one workgroup per sub-table.
 * Stable ranking: the tile is split wave-major, each wave ranks its 64 elements per round with
 * eight ballots (peers with an equal digit), per-wave digit counters live in LDS.
 * The tile is then laid out by digit in an LDS copy and stored in index order: consecutive lanes
 * write consecutive elements of one digit's run (seg_sort_tile.h has the arithmetic).
 * ------------------------------------------------------------------------------------------ */
template <int BITS, int NT>   /* digit width; threads per workgroup (256, or 1024 for long segments: four times the loads in flight per sub-table).
                               * 8 bits: a tile of 2048 or 4096 keys leaves >= 8 neighbours per digit, i.e. runs of 64 bytes and more that whole groups of lanes write;
                               * 11-bit digits (two passes for 22-bit ranks, the first one fused with the gather of the fragments) were measured and lost: one key per
                               * digit and tile means lone 8-byte stores, and the saved pass does not pay for them.
                               * dig_hist: 256 counters per digit of T and sub-table (sst_hist_row).  The pass with shift 0 counts all n_dig digits in its one
                               * sweep over the times and leaves them there, the later ones take theirs from it (a histogram does not depend on the order).
                               * Without it every pass sweeps for its own digit */
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(NT == 1024 ? 8 : 4)))   /* two workgroups of 1024 per CU (<= 64 VGPRs), four of 256 (eight keys per thread: ~100 VGPRs) */
void k_seg_sort_pass(const u64 *__restrict__ seg_off, const u32 *__restrict__ seg_len, const u64 *__restrict__ src_kc, const u64 *__restrict__ src_t,
                     u64 *__restrict__ dst_kc, u64 *__restrict__ dst_t, int shift, u32 *__restrict__ dig_hist, int n_dig)
{
	constexpr int NBIN = 1 << BITS, NWV = NT / 64, SS_E = sst_per_thread(NT), TILE = sst_tile(NT);
	static_assert(NBIN == 256, "the scans below give four digits to each lane of one wave");
	static_assert(NBIN == SST_NBIN && NT >= NBIN, "one thread per digit");
	__shared__ u32 s_hist[NBIN];                                /* where the digit's next element goes in the segment */
	__shared__ u32 s_start[NBIN];                               /* the tile's count of the digit, then where its run starts in the tile */
	__shared__ u32 s_base[NBIN];                                /* sst_base: s_hist - s_start */
	__shared__ u32 s_wc[NWV][NBIN];
	__shared__ u64 s_stage[TILE];                               /* the tile by digit: its times, then its keys */
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const u64 a = seg_off[blockIdx.x];
	const u32 len = seg_len ? seg_len[blockIdx.x] : (u32)(seg_off[blockIdx.x + 1] - a);   /* (offsets inside a segment are 32-bit throughout) */
	if (len == 0) return;
	if (len == 1) { if (tid == 0) { dst_kc[a] = src_kc[a]; dst_t[a] = src_t[a]; } return; }
	if (dig_hist && shift > 0) {
		for (int q = tid; q < NBIN; q += NT) s_hist[q] = dig_hist[sst_hist_row(blockIdx.x, n_dig, shift / BITS) + q];
	} else if (dig_hist && n_dig > 1) {                         /* (n_dig <= SST_MAX_DIGITS: the rows of the later digits borrow the stage) */
		static_assert(sizeof(s_stage) >= (SST_MAX_DIGITS - 1) * NBIN * sizeof(u32), "rows for the digits behind the first");
		u32 *rows = (u32*)s_stage;
		for (int q = tid; q < NBIN; q += NT) s_hist[q] = 0;
		for (int q = tid; q < (n_dig - 1) * NBIN; q += NT) rows[q] = 0;
		__syncthreads();
		for (u32 i = tid; i < len; i += NT) {
			const u64 t = src_t[a + i];
			atomicAdd(&s_hist[sst_digit(t, 0)], 1u);
			for (int j = 1; j < n_dig; ++j) atomicAdd(&rows[(j - 1) * NBIN + sst_digit(t, j * BITS)], 1u);
		}
		__syncthreads();
		for (int q = tid; q < (n_dig - 1) * NBIN; q += NT) dig_hist[sst_hist_row(blockIdx.x, n_dig, 1) + q] = rows[q];
	} else {
		for (int q = tid; q < NBIN; q += NT) s_hist[q] = 0;
		__syncthreads();
		for (u32 i = tid; i < len; i += NT) atomicAdd(&s_hist[sst_digit(src_t[a + i], shift)], 1u);
	}
	__syncthreads();
	if (tid < 64) {                                              /* exclusive scan of the 256 digit counts by one wave */
		u32 v[4], t = 0;
		for (int q = 0; q < 4; ++q) { v[q] = s_hist[4 * tid + q]; t += v[q]; }
		u32 incl = t;
		for (int o = 1; o < 64; o <<= 1) { const u32 x = __shfl_up(incl, o); if (lane >= o) incl += x; }
		u32 e = incl - t;
		for (int q = 0; q < 4; ++q) { s_hist[4 * tid + q] = e; e += v[q]; }
	}
	for (u32 tile = 0; tile < len; tile += TILE) {
		const u32 n_tile = std::min<u32>(TILE, len - tile);
		for (int q = tid; q < NWV * NBIN; q += NT) (&s_wc[0][0])[q] = 0;
		__syncthreads();                                         /* (and the scan above, and the stores of the tile before) */
		u64 et[SS_E], ek[SS_E];
		u32 erk[SS_E];
#pragma unroll
		for (int r = 0; r < SS_E; ++r) {
			const u32 idx = (u32)sst_src_index(tile, wave, r, lane, SS_E);
			const bool valid = idx < len;
			u64 t = 0;
			if (valid) t = src_t[a + idx];
			const u32 d = sst_digit(t, shift);
			u64 peers = __ballot(valid);
#pragma unroll
			for (int b = 0; b < BITS; ++b) {
				const u64 vb = __ballot(valid && (d >> b & 1));
				peers &= (d >> b & 1) ? vb : ~vb;
			}
			u32 old = 0;
			const int leader = valid ? __ffsll((long long)peers) - 1 : lane;
			if (valid && lane == leader) { old = s_wc[wave][d]; s_wc[wave][d] = old + __popcll(peers); }
			old = __shfl(old, leader);
			et[r] = t;
			erk[r] = valid ? (d << 24 | (old + __builtin_amdgcn_mbcnt_hi((u32)(peers >> 32), __builtin_amdgcn_mbcnt_lo((u32)peers, 0u)))) : 0xffffffffu;   /* + the peers in lower lanes */
		}
#pragma unroll
		for (int r = 0; r < SS_E; ++r)                           /* the keys are not needed before the copy is laid out: their loads run under the scans */
			if (erk[r] != 0xffffffffu) ek[r] = src_kc[a + (u32)sst_src_index(tile, wave, r, lane, SS_E)];
		__syncthreads();
		if (tid < NBIN) s_start[tid] = sst_wave_prefix(&s_wc[0][0], NWV, tid);
		__syncthreads();
		if (tid < 64) {                                          /* the digits' runs inside the tile: exclusive scan of the tile's counts; the running offsets move on */
			u32 v[4], t = 0;
			for (int q = 0; q < 4; ++q) { v[q] = s_start[4 * tid + q]; t += v[q]; }
			u32 incl = t;
#pragma nounroll                                            /* (unrolled, the six source lanes are kept in registers across the whole tile loop) */
			for (int o = 1; o < 64; o <<= 1) { const u32 x = __shfl_up(incl, o); if (lane >= o) incl += x; }
			u32 e = incl - t;
			for (int q = 0; q < 4; ++q) {
				const u32 run = s_hist[4 * tid + q];
				s_start[4 * tid + q] = e; s_base[4 * tid + q] = sst_base(run, e); s_hist[4 * tid + q] = run + v[q];
				e += v[q];
			}
		}
		__syncthreads();
#pragma unroll
		for (int r = 0; r < SS_E; ++r) {
			if (erk[r] != 0xffffffffu) {
				const u32 d = erk[r] >> 24;
				erk[r] = sst_lds_pos(s_start[d], s_wc[wave][d], erk[r] & 0xffffff);
				s_stage[erk[r]] = et[r];
			}
		}
		__syncthreads();
		u32 g[SS_E];                                             /* where the copy's element r x NT + tid goes in the segment */
#pragma unroll
		for (int r = 0; r < SS_E; ++r) {
			const u32 i = r * NT + tid;
			if (i < n_tile) {
				const u64 t = s_stage[i];
				g[r] = (u32)(sst_global(a, s_base[sst_digit(t, shift)], i) - a);
				dst_t[a + g[r]] = t;
			}
		}
		__syncthreads();
#pragma unroll
		for (int r = 0; r < SS_E; ++r) if (erk[r] != 0xffffffffu) s_stage[erk[r]] = ek[r];
		__syncthreads();
#pragma unroll
		for (int r = 0; r < SS_E; ++r) {
			const u32 i = r * NT + tid;
			if (i < n_tile) dst_kc[a + g[r]] = s_stage[i];
		}
	}
}

/* ------------------------------------------------------------------------------------------
 * K5: exact khashl layout replay, one workgroup per sub-table.
 *   * between two doublings every put is a first-come-first-served linear-probing placement of a
 *     NEW key; FCFS in order sigma == ordered probing with priority = rank in sigma, which is
 *     order-free and therefore done in parallel with atomicMin on a per-slot owner rank;
 *   * a doubling is khashl's in-place kick-out rehash (khashl.h:171-189), whose placement order is
 *     data dependent: executed literally by one lane;
 *   * growth happens at the next put-call once count >= 0.75 capacity (khashl.h:202), including a
 *     trailing put-call on an existing key (lastput vs. time of the last new key).
 * ------------------------------------------------------------------------------------------ */
#define RP_U 1
#define RP_PAR_MIN  2048                                 /* doublings from this size on try the exact parallel routine */
#define RP_LDS_WORDS 4096                                 /* doublings up to 131072 slots keep their bitmaps in LDS */
__device__ __forceinline__ bool bm_get(const u32 *u, u32 i) { return u[i >> 5] >> (i & 31) & 1; }

/* khashl's in-place doubling (khashl.h:171-189), executed literally by ONE lane because the order in
 * which keys are re-placed is data dependent.  `cur`/`oth` are the old/new "used" bitmaps (LDS when
 * they fit, else global).  The lane publishes its scan position so that a helper wave can run ahead
 * and pull the cache lines the kick-out chain is about to touch (replay_prefetch). */
__device__ void replay_double(u64 *keys, u32 *cur, u32 *oth, u32 n, u32 N, u32 nbits_new, volatile u32 *progress)
{
	const u32 Nmask = N - 1;
	for (u32 jw = 0; jw < (n + 31) / 32; ++jw) {
		*progress = jw * 32;
		while (cur[jw]) {                                  /* next still-unmoved old slot of this word */
			const u32 j = jw * 32 + (__ffs((int)cur[jw]) - 1);
			if (j >= n) { cur[jw] = 0; break; }
			u64 key = keys[j];
			cur[jw] &= cur[jw] - 1;
			for (;;) {
				u32 i = yk_h2b((u32)(key >> 10), nbits_new);
				u32 wo = oth[i >> 5], wc = i < n ? cur[i >> 5] : 0;     /* both words in flight together */
				while (wo >> (i & 31) & 1) {
					i = (i + 1) & Nmask;
					if ((i & 31) == 0) { wo = oth[i >> 5]; }
					if ((i & 31) == 0 || i == n) wc = i < n ? cur[i >> 5] : 0;
				}
				oth[i >> 5] = wo | 1u << (i & 31);
				if (i < n && (wc >> (i & 31) & 1)) {
					const u64 tmp = keys[i]; keys[i] = key; key = tmp;
					cur[i >> 5] = wc & ~(1u << (i & 31));
				} else { keys[i] = key; break; }
			}
		}
	}
	*progress = 0xffffffffu;
}

/* The same doubling, wave-cooperative.  The ORDER of placements is untouched (lane L of a round
 * commits only after lanes 0..L-1, rounds follow the scan order), but the global-memory latency is
 * taken off the serial path: a round picks the next 64 unmoved slots from the bitmap, all 64 lanes
 * load their key and the 4 slots at its new home at once (an unmoved slot's key never changes before
 * it is moved, so the loads stay valid), then the lanes commit one after the other against the
 * authoritative LDS bitmaps, falling back to a real load only for kicks beyond the first. */
__device__ void replay_double_wave(u64 *keys, u32 *cur, u32 *oth, u32 n, u32 N, u32 nbits_new, volatile u32 *progress, u32 *s_sel)
{
	const u32 lane = threadIdx.x & 63, Nmask = N - 1, nwords = (n + 31) / 32;
	u32 pos = 0;
	while (pos < nwords) {
		if (lane == 0) *progress = pos * 32;
		const u32 w = pos + lane;
		const u32 cw = w < nwords ? cur[w] : 0;
		const u32 c = __popc(cw);
		u32 incl = c;
		for (int o = 1; o < 64; o <<= 1) { const u32 t = __shfl_up(incl, o); if (lane >= (u32)o) incl += t; }
		const u32 total = __shfl(incl, 63), excl = incl - c;
		if (total == 0) { pos += 64; continue; }
		s_sel[lane] = 0xffffffffu;
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		if (excl < 64) {
			u32 bits = cw, r = excl;
			while (bits && r < 64) { s_sel[r++] = w * 32 + (__ffs((int)bits) - 1); bits &= bits - 1; }
		}
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		const u32 j = s_sel[lane];
		const u32 nsel = total < 64 ? total : 64;
		const u32 last = s_sel[nsel - 1];
		pos = total <= 64 ? pos + 64 : last / 32;          /* leftovers of that word are rescanned next round */
		/* speculative loads: own key, then the old keys sitting where it is going to land */
		u64 key0 = 0, win[4] = { 0, 0, 0, 0 };
		u32 h0 = 0;
		if (j != 0xffffffffu) {
			key0 = keys[j];
			h0 = yk_h2b((u32)(key0 >> 10), nbits_new);
#pragma unroll
			for (int q = 0; q < 4; ++q) { const u32 x = (h0 + q) & Nmask; if (x < n) win[q] = keys[x]; }
		}
		for (u32 L = 0; L < nsel; ++L) {
			if (lane == L && (cur[j >> 5] >> (j & 31) & 1)) {      /* still unmoved: its turn in the scan */
				cur[j >> 5] &= ~(1u << (j & 31));
				u64 key = key0;
				bool first = true;
				for (;;) {
					u32 i = yk_h2b((u32)(key >> 10), nbits_new);
					u32 wo = oth[i >> 5], wc = i < n ? cur[i >> 5] : 0;
					while (wo >> (i & 31) & 1) {
						i = (i + 1) & Nmask;
						if ((i & 31) == 0) wo = oth[i >> 5];
						if ((i & 31) == 0 || i == n) wc = i < n ? cur[i >> 5] : 0;
					}
					oth[i >> 5] = wo | 1u << (i & 31);
					if (i < n && (wc >> (i & 31) & 1)) {
						const u32 d = (i - h0) & Nmask;
						u64 kicked;
						if (first && d < 4) kicked = d == 0 ? win[0] : d == 1 ? win[1] : d == 2 ? win[2] : win[3];
						else kicked = keys[i];
						keys[i] = key; key = kicked;
						cur[i >> 5] = wc & ~(1u << (i & 31));
						first = false;
					} else { keys[i] = key; break; }
				}
			}
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		}
	}
	if (lane == 0) *progress = 0xffffffffu;
}

/* LDS variant with the two bitmaps interleaved: bm[w] = old "used" word w (high half) | new "used"
 * word w (low half), so that a placement costs one LDS read and one LDS write on its serial path */
__device__ void replay_double_wave64(u64 *keys, u64 *bm, u32 n, u32 N, u32 nbits_new, volatile u32 *progress, u32 *s_sel)
{
	const u32 lane = threadIdx.x & 63, Nmask = N - 1, nwords = (n + 31) / 32;
	u32 pos = 0;
	while (pos < nwords) {
		if (lane == 0) *progress = pos * 32;
		const u32 w = pos + lane;
		const u32 cw = w < nwords ? (u32)(bm[w] >> 32) : 0;
		const u32 c = __popc(cw);
		u32 incl = c;
		for (int o = 1; o < 64; o <<= 1) { const u32 t = __shfl_up(incl, o); if (lane >= (u32)o) incl += t; }
		const u32 total = __shfl(incl, 63), excl = incl - c;
		if (total == 0) { pos += 64; continue; }
		s_sel[lane] = 0xffffffffu;
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		if (excl < 64) {
			u32 bits = cw, r = excl;
			while (bits && r < 64) { s_sel[r++] = w * 32 + (__ffs((int)bits) - 1); bits &= bits - 1; }
		}
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		const u32 j = s_sel[lane];
		const u32 nsel = total < 64 ? total : 64;
		const u32 last = s_sel[nsel - 1];
		pos = total <= 64 ? pos + 64 : last / 32;
		u64 key0 = 0, win[4] = { 0, 0, 0, 0 };
		u32 h0 = 0;
		if (j != 0xffffffffu) {
			key0 = keys[j];
			h0 = yk_h2b((u32)(key0 >> 10), nbits_new);
#pragma unroll
			for (int q = 0; q < 4; ++q) { const u32 x = (h0 + q) & Nmask; if (x < n) win[q] = keys[x]; }
		}
		for (u32 L = 0; L < nsel; ++L) {
			if (lane == L) {
				u64 b = bm[j >> 5];
				if (b >> (32 + (j & 31)) & 1) {                  /* still unmoved: its turn in the scan */
					u64 key = key0;
					bool first = true;
					u32 i = h0, iw = i >> 5;
					if (iw == (j >> 5)) b &= ~(1ull << (32 + (j & 31)));
					else { bm[j >> 5] = b & ~(1ull << (32 + (j & 31))); b = bm[iw]; }
					for (;;) {
						while (b >> (i & 31) & 1) {                /* linear probing on the new bitmap */
							i = (i + 1) & Nmask;
							if ((i & 31) == 0) { bm[iw] = b; iw = i >> 5; b = bm[iw]; }
						}
						b |= 1ull << (i & 31);
						if (b >> (32 + (i & 31)) & 1) {           /* an unmoved old key sits there: kick it out */
							const u32 d = (i - h0) & Nmask;
							u64 kicked;
							if (first && d < 4) kicked = d == 0 ? win[0] : d == 1 ? win[1] : d == 2 ? win[2] : win[3];
							else kicked = keys[i];
							keys[i] = key; key = kicked;
							b &= ~(1ull << (32 + (i & 31)));
							first = false;
							const u32 i2 = yk_h2b((u32)(key >> 10), nbits_new);
							if ((i2 >> 5) != iw) { bm[iw] = b; iw = i2 >> 5; b = bm[iw]; }
							i = i2;
						} else { keys[i] = key; bm[iw] = b; break; }
					}
				}
			}
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		}
	}
	if (lane == 0) *progress = 0xffffffffu;
}

/* helper wave of the doubling: for old slots a little ahead of the serial lane, touch the line the
 * key will land on and, one level deeper, the line its kicked-out victim will land on */
__device__ void replay_prefetch(const u64 *keys, u32 n, u32 nbits_new, volatile u32 *progress, u32 *sink)
{
	const u32 lane = threadIdx.x & 63;
	u32 acc = 0, last = 0xfffffffeu;
	for (;;) {
		const u32 p = *progress;
		if (p == 0xffffffffu) break;
		if (p == last) { __builtin_amdgcn_s_sleep(8); continue; }
		last = p;
		const u32 j = p + 48 + lane;                       /* window [p+48, p+112) */
		if (j < n) {
			const u64 key = keys[j];
			if (key != YK_EMPTY) {
				const u32 i = yk_h2b((u32)(key >> 10), nbits_new);
				const u64 v = *(volatile const u64*)&keys[i];
				acc ^= (u32)v;
				if (i < n && v != YK_EMPTY) {
					const u32 i2 = yk_h2b((u32)(v >> 10), nbits_new);
					acc ^= (u32)*(volatile const u64*)&keys[i2];
				}
			}
		}
	}
	if (acc == 0x5a5a5a5au) *sink = acc;                   /* keeps the touches alive */
}

/* ------------------------------------------------------------------------------------------
 * Exact PARALLEL doubling.
 * The serial loop above defines, for every key, a processing time sigma = (c, d): c = old slot at
 * which the scan started the kick-out chain that moved the key, d = its depth in that chain; the
 * final layout is first-come-first-served linear probing in sigma order.  Two facts make it
 * parallel:  (1) FCFS in sigma order == ordered probing with priority sigma (atomicMin per slot);
 * (2) the key at old slot s is kicked by the key x that lands on physical slot s iff c(x) < s, and
 * x comes from an old slot <= s/2 + D1 (new home = 2 * old home + 1 bit, D1 = largest old
 * displacement).  So sigma and landing slot become final front to back: once all old slots < F are
 * final, sigma is known up to ~2F and landings up to ~2F - 4 D1.  Each round is a handful of
 * workgroup-wide passes; the first ~8 D1 slots are done by the literal serial rule.
 * The result is VERIFIED against the defining fixed point (sigma of every key follows from its
 * lander; every key sits at the first slot from its home not held by an earlier key).  That fixed
 * point is unique, so a verified layout is the reference's; on any doubt the caller falls back to
 * the serial routine (nothing has been modified until the commit).
 * ------------------------------------------------------------------------------------------ */
__device__ u32 d_par_ok, d_par_fail;      /* doublings done by the parallel routine / sent back to the serial one */
__device__ u64 d_rp_prof[8];              /* debug (dbg & 32): wall-clock ticks of block 0 per phase */
#define RP_TICK(slot) if ((T.dbg & 32) && blockIdx.x == 0 && tid == 0) { const u64 now_ = wall_clock64(); d_rp_prof[slot] += now_ - tick_; tick_ = now_; }
#define PD_U 4
#define PD_EMPTY  0xffffffffffffffffull
#define PD_FINAL  0x8000000000000000ull
#define PD_PACK(c, d, s) ((u64)(c) << 40 | (u64)(d) << 24 | (u64)(s))
#define PD_C(o) ((u32)((o) >> 40) & 0x7fffffu)
#define PD_D(o) ((u32)((o) >> 24) & 0xffffu)
#define PD_S(o) ((u32)(o) & 0xffffffu)

/* one workgroup on one CU: its waves share the L1, so a workgroup barrier (which carries the
 * workgroup-scope fence) orders its own global traffic; the agent-scope write-back + invalidate of
 * block_sync_global() is only needed once, before the result is handed to the rest of the kernel */
__device__ __forceinline__ void pd_sync() { __syncthreads(); }

__device__ bool replay_double_par(u64 *keys, const u32 *cur, u32 *oth, u32 n, u32 N, u32 nb_new,
                                  u64 *OWN, u64 *SIG, u64 *TMP, u32 *s_par /* LDS [8] */, u64 *lds, size_t lds_bytes,
                                  u64 *xtra /* global, N / 2 entries */, bool prof)
{
	u64 tk_ = wall_clock64();
#define PD_TICK(slot) if (prof && threadIdx.x == 0) { const u64 now_ = wall_clock64(); d_rp_prof[slot] += now_ - tk_; tk_ = now_; }
	const u32 tid = threadIdx.x, Nmask = N - 1, nmask = n - 1;
	u32 *s_fail = s_par, *s_d1 = s_par + 1, *s_cnt = s_par + 2;
	if (tid < 8) s_par[tid] = 0;
	__syncthreads();
	/* 0. copies, largest old displacement */
	u32 d1 = 0, nused = 0;
	for (u32 s = tid; s < n; s += blockDim.x) {
		const u64 k = keys[s];
		TMP[s] = k; SIG[s] = PD_EMPTY;
		if (bm_get(cur, s)) { const u32 h = yk_h2b((u32)(k >> 10), nb_new - 1); const u32 d = (s - h) & nmask; d1 = d > d1 ? d : d1; ++nused; }
	}
	for (u32 i = tid; i < N; i += blockDim.x) OWN[i] = PD_EMPTY;
	atomicMax(s_d1, d1); atomicAdd(s_cnt, nused);
	pd_sync();
	const u32 D1 = *s_d1, n_used = *s_cnt;
	PD_TICK(4)
	const u32 F0 = 5 * D1 + 16, B0 = F0 + 2 * D1 + 4;               /* final after the base phase / simulated by it */
	if (B0 * 4 > n || n > (1u << 23)) { if (tid == 0) s_par[7] = 1; return false; }   /* too clustered / too large: serial */
	/* 1. the literal rule for scan positions below B0; a chain is followed only while it stays below
	 * B0 (what it kicks further up lands beyond anything the first F0 slots can reach, and gets its
	 * sigma from the lander rule later); only slots < F0 are kept, the rest is margin.  One lane does
	 * it, on LDS copies of the few hundred entries involved (the chain is a string of dependent
	 * accesses: ~10x faster than on the global arrays). */
	{
		const u32 WA = 2 * B0 + 4 * D1 + 16, WB = 4 * D1 + 16;           /* landings: [0, WA) and, wrapped, [N - WB, N) */
		if (WA + WB > N) { if (tid == 0) s_par[7] = 2; return false; }
		const bool in_lds = (size_t)(2 * B0 + WA + WB) * 8 <= lds_bytes;      /* else the same walk on global scratch */
		if (!in_lds && 2 * B0 + WA + WB > N / 2) { if (tid == 0) s_par[7] = 2; return false; }
		u64 *w_tmp, *w_sig, *w_own;
		if (in_lds) { w_tmp = lds; w_sig = lds + B0; w_own = lds + 2 * B0; }
		else { w_tmp = xtra; w_sig = xtra + B0; w_own = xtra + 2 * B0; }
		for (u32 j = tid; j < B0; j += blockDim.x) { w_tmp[j] = bm_get(cur, j) ? TMP[j] : PD_EMPTY; w_sig[j] = PD_EMPTY; }
		for (u32 i = tid; i < WA + WB; i += blockDim.x) w_own[i] = PD_EMPTY;
		pd_sync();
		if (tid == 0) {
			bool lost = false;
			for (u32 j = 0; j < B0 && !lost; ++j) {
				if (w_tmp[j] == PD_EMPTY || w_sig[j] != PD_EMPTY) continue;
				u32 s = j, d = 0;
				for (;;) {
					const u64 me = PD_PACK(j, d, s);
					w_sig[s] = me | PD_FINAL;
					u32 i = yk_h2b((u32)(w_tmp[s] >> 10), nb_new);
					for (;;) {
						const u32 li = i < WA ? i : i >= N - WB ? WA + (i - (N - WB)) : 0xffffffffu;
						if (li == 0xffffffffu) { lost = true; break; }
						if (w_own[li] == PD_EMPTY) { w_own[li] = me; break; }
						i = (i + 1) & Nmask;
					}
					if (lost) break;
					if (i < B0 && w_tmp[i] != PD_EMPTY && w_sig[i] == PD_EMPTY) { s = i; ++d; } else break;
				}
			}
			if (lost) { *s_fail = 1; s_par[7] = 3; }
		}
		pd_sync();
		if (*s_fail) return false;
		/* keep what concerns old slots < F0 */
		for (u32 j = tid; j < F0; j += blockDim.x) SIG[j] = w_sig[j];
		for (u32 i = tid; i < WA + WB; i += blockDim.x) {
			const u64 o = w_own[i];
			if (o != PD_EMPTY && PD_S(o) < F0) OWN[i < WA ? i : N - WB + (i - WA)] = o;
		}
	}
	pd_sync();
	PD_TICK(5)
	/* 2. rounds */
	u32 F = F0;
	while (F < n) {
		u32 S1 = 2 * (F - D1) - 1;
		if (S1 > n) S1 = n;
		const u32 S2 = S1 == n ? n : S1 - (2 * D1 + 3);
		if (S2 <= F) { if (tid == 0) s_par[7] = 4; return false; }
		/* A: sigma of the keys whose possible landers are all final */
		for (u32 s0 = F + tid; s0 < S1; s0 += PD_U * blockDim.x) {          /* PD_U independent slots per lane in flight */
			u64 g[PD_U], o[PD_U]; bool ok[PD_U];
#pragma unroll
			for (int u = 0; u < PD_U; ++u) {
				const u32 s = s0 + u * blockDim.x;
				ok[u] = s < S1 && bm_get(cur, s);
				g[u] = ok[u] ? SIG[s] : 0; o[u] = ok[u] ? OWN[s] : 0;
			}
#pragma unroll
			for (int u = 0; u < PD_U; ++u) {
				const u32 s = s0 + u * blockDim.x;
				if (ok[u] && g[u] == PD_EMPTY)
					SIG[s] = (o[u] != PD_EMPTY && PD_S(o[u]) != s && PD_C(o[u]) < s) ? PD_PACK(PD_C(o[u]), PD_D(o[u]) + 1, s) : PD_PACK(s, 0, s);
			}
		}
		pd_sync();
		/* B: ordered probing of those keys on top of the final ones */
		for (u32 s0 = F + tid; s0 < S1; s0 += PD_U * blockDim.x) {
			u64 cand[PD_U], old[PD_U]; u32 i[PD_U], act = 0;
#pragma unroll
			for (int u = 0; u < PD_U; ++u) {
				const u32 s = s0 + u * blockDim.x;
				if (s < S1 && bm_get(cur, s)) { cand[u] = SIG[s]; i[u] = yk_h2b((u32)(TMP[s] >> 10), nb_new); if (!(cand[u] & PD_FINAL)) act |= 1u << u; }
			}
			for (u32 guard = 0; act && guard < N; ++guard) {
#pragma unroll
				for (int u = 0; u < PD_U; ++u) if (act >> u & 1) old[u] = atomicMin(&OWN[i[u]], cand[u]);
#pragma unroll
				for (int u = 0; u < PD_U; ++u)
					if (act >> u & 1) {
						if (old[u] == PD_EMPTY) { act &= ~(1u << u); continue; }
						if (old[u] > cand[u]) {
							if (__hip_atomic_load(&SIG[PD_S(old[u])], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & PD_FINAL) { *s_fail = 1; act &= ~(1u << u); continue; }
							cand[u] = old[u];
						}
						i[u] = (i[u] + 1) & Nmask;
					}
			}
		}
		pd_sync();
		if (*s_fail) { if (tid == 0) s_par[7] = 5; return false; }
		/* C: finalise [F, S2); take the not yet final participants [S2, S1) out again */
		for (u32 s = F + tid; s < S2; s += blockDim.x) if (bm_get(cur, s) && !(SIG[s] & PD_FINAL)) SIG[s] |= PD_FINAL;
		if (S2 < S1) {
			const u32 lo = 2 * (S2 > D1 ? S2 - D1 : 0), hi0 = 2 * S1 + 4 * D1 + 16, hi = hi0 < N ? hi0 : N;
			for (u32 i = (lo > 2 ? lo - 2 : 0) + tid; i < hi; i += blockDim.x) {
				const u64 o = OWN[i];
				if (o != PD_EMPTY && PD_S(o) >= S2 && PD_S(o) < S1 && !(SIG[PD_S(o)] & PD_FINAL)) OWN[i] = PD_EMPTY;
			}
			pd_sync();
			for (u32 s = S2 + tid; s < S1; s += blockDim.x) if (bm_get(cur, s) && !(SIG[s] & PD_FINAL)) SIG[s] = PD_EMPTY;
		}
		pd_sync();
		F = S2;
	}
	PD_TICK(6)
	/* 3. verification of the fixed point */
	if (tid < 8 && tid >= 2) s_par[tid] = 0;
	__syncthreads();
	u32 placed = 0, bad = 0;
	for (u32 i0 = tid; i0 < N; i0 += PD_U * blockDim.x) {
		u64 o[PD_U], g[PD_U], k[PD_U];
#pragma unroll
		for (int u = 0; u < PD_U; ++u) { const u32 i = i0 + u * blockDim.x; o[u] = i < N ? OWN[i] : PD_EMPTY; }
#pragma unroll
		for (int u = 0; u < PD_U; ++u) if (o[u] != PD_EMPTY) { g[u] = SIG[PD_S(o[u])]; k[u] = TMP[PD_S(o[u])]; }
#pragma unroll
		for (int u = 0; u < PD_U; ++u) {
			if (o[u] == PD_EMPTY) continue;
			const u32 i = i0 + u * blockDim.x;
			++placed;
			if ((g[u] & ~PD_FINAL) != o[u]) { bad = 1; continue; }
			u32 q = yk_h2b((u32)(k[u] >> 10), nb_new), steps = 0;
			while (q != i) {                                          /* every slot before it holds an earlier key */
				const u64 p = OWN[q];
				if (p == PD_EMPTY || p > o[u] || ++steps > 4 * D1 + 64) { bad = 1; break; }
				q = (q + 1) & Nmask;
			}
		}
	}
	for (u32 s = tid; s < n; s += blockDim.x) {
		if (!bm_get(cur, s)) continue;
		const u64 g = SIG[s], o = OWN[s];
		if (g == PD_EMPTY || !(g & PD_FINAL)) { bad = 1; continue; }
		const u64 want = (o != PD_EMPTY && PD_S(o) != s && PD_C(o) < s) ? PD_PACK(PD_C(o), PD_D(o) + 1, s) : PD_PACK(s, 0, s);
		if ((g & ~PD_FINAL) != want) bad = 1;
	}
	atomicAdd(s_par + 3, placed);
	if (bad) *s_fail = 1;
	__syncthreads();
	if (*s_fail || s_par[3] != n_used) { if (tid == 0) s_par[7] = 6; return false; }
	/* 4. commit: move the keys, publish the new bitmap (one slot per lane: a wave's ballot is two bitmap words) */
	for (u32 i0 = 0; i0 < N; i0 += blockDim.x) {
		const u32 i = i0 + tid;
		const u64 o = i < N ? OWN[i] : PD_EMPTY;
		if (o != PD_EMPTY) keys[i] = TMP[PD_S(o)];
		const u64 b = __ballot(o != PD_EMPTY);
		if ((tid & 63) == 0 && i < N) { oth[i >> 5] = (u32)b; if (i + 32 < N) oth[(i >> 5) + 1] = (u32)(b >> 32); }
	}
	__syncthreads();
	PD_TICK(7)
	return true;
}

__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_replay(const ReplayTask *tasks, const u64 *old_keys, const u32 *old_used, u64 *new_keys, u32 *new_used,
              u32 *scr_used, u32 *scr_owner, u64 *scr_par, const u64 *rec_kc, const u64 *rec_t, const u64 *lastput,
              u32 *out_bits, u32 *out_count, u32 lds_words)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_dyn[];   /* >= 2 * RP_LDS_WORDS words: placement owner ranks, or ... */
	u64 *s_bm = (u64*)s_dyn;                               /* ... doubling: old (high) and new (low) bitmap words, interleaved */
	__shared__ u32 s_progress;
	__shared__ u32 s_sel[64];
	__shared__ u32 s_par[8];
	const ReplayTask T = tasks[blockIdx.x];
	const int tid = threadIdx.x;
	u64 *const gkeys = new_keys + T.new_off;
	/* while the table has <= 8192 slots its keys live in LDS (second half of s_dyn): the doublings of
	 * that phase are the serial routine, whose cost is the latency of its dependent key accesses */
	u64 *const lkeys = (u64*)(s_dyn + 16384);
	u64 *keys = (lds_words >= 32768 && (T.old_bits == YK_NOCAP || T.old_bits <= 12) && (T.init_bits == YK_NOCAP || T.init_bits <= 12) && !(T.dbg & 64)) ? lkeys : gkeys;
	u32 *UA = new_used + (T.new_off >> 5), *UB = scr_used + (T.new_off >> 5);
	u32 *owner = scr_owner + T.new_off;
	u32 *cur = UA, *oth = UB;
	u32 n = T.old_bits == YK_NOCAP ? 0 : 1u << T.old_bits, bits = T.old_bits == YK_NOCAP ? 0 : T.old_bits;
	u32 cnt = T.old_count;

	for (u32 i = tid; i < n; i += blockDim.x) keys[i] = old_keys[T.old_off + i];
	for (u32 w = tid; w < (n + 31) / 32; w += blockDim.x) UA[w] = old_used[(T.old_off >> 5) + w];
	if (n == 0 && T.init_bits != YK_NOCAP) {                 /* yak_ht_resize(f, size) on an empty set (htab.c:186) */
		bits = T.init_bits; n = 1u << bits;
		for (u32 w = tid; w < (n + 31) / 32; w += blockDim.x) UA[w] = 0;
	}
	__syncthreads();

	u32 i0 = 0;
	u64 tick_ = wall_clock64();
	for (;;) {
		const u32 thr = (n >> 1) + (n >> 2);
		bool grow = false;
		if (i0 < T.m) grow = cnt >= thr;
		else {
			/* all new keys are in; one more doubling if a put-call follows the moment the load hit 75 % */
			const u64 lp = lastput ? lastput[blockIdx.x] : 0;
			const bool later_put = lp != 0 && (T.m == 0 || lp - 1 > rec_t[T.rec_off + T.m - 1]);
			grow = later_put && cnt >= thr && i0 != 0xffffffffu;
			if (!grow) break;
			i0 = 0xffffffffu;                              /* at most one trailing doubling */
		}
		if (grow) {
			const u32 N = n ? n << 1 : 4, nb = n ? bits + 1 : 2;
			bool done = false;
			if (scr_par && n >= RP_PAR_MIN && !(T.dbg & 16)) {
				u64 *pb = scr_par + 2 * T.new_off;
				done = replay_double_par(keys, cur, oth, n, N, nb, pb, pb + N, pb + N + n, s_par, (u64*)s_dyn, (size_t)(lds_words < 16384 ? lds_words : 16384) * 4,
				                         (u64*)(scr_owner + T.new_off), (T.dbg & 32) && blockIdx.x == 0);
				if (tid == 0) atomicAdd(done ? &d_par_ok : &d_par_fail, 1u);
				if (!done && (T.dbg & 128) && tid == 0) printf("parfail n=%u code=%u\n", n, s_par[7]);
			}
			if (!done) {
			const bool in_lds = (N + 31) / 32 <= RP_LDS_WORDS && !(T.dbg & 8);
			if (in_lds) {
				for (u32 w = tid; w < (N + 31) / 32; w += blockDim.x) s_bm[w] = w < (n + 31) / 32 ? (u64)cur[w] << 32 : 0ull;
			} else {
				for (u32 w = tid; w < (N + 31) / 32; w += blockDim.x) oth[w] = 0;
			}
			if (tid == 0) s_progress = 0;
			__syncthreads();
			if (T.dbg & 1) { if (tid == 0) s_progress = 0xffffffffu; }
			else if (tid < 64) {
				if (in_lds) replay_double_wave64(keys, s_bm, n, N, nb, &s_progress, s_sel);
				else replay_double_wave(keys, cur, oth, n, N, nb, &s_progress, s_sel);
			} else if (tid < 128 && !(T.dbg & 4) && keys == gkeys) replay_prefetch(keys, n, nb, &s_progress, scr_owner + T.new_off);
			__syncthreads();
			if (in_lds) { for (u32 w = tid; w < (N + 31) / 32; w += blockDim.x) oth[w] = (u32)s_bm[w]; __syncthreads(); }
			}
			u32 *t = cur; cur = oth; oth = t;
			n = N; bits = nb;
			if (keys == lkeys && n >= 8192) {                 /* grown out of LDS */
				for (u32 i = tid; i < n; i += blockDim.x) gkeys[i] = lkeys[i];
				__syncthreads();
				keys = gkeys;
			}
			RP_TICK(n >= 32768 ? 1 : 0)
			if (i0 == 0xffffffffu) break;
			continue;
		}
		/* FCFS placement of the next keys, up to the growth threshold: every key walks from its home
		 * slot and claims a slot with min(rank); a displaced later key is carried on by the claimer.
		 * The owner ranks live in LDS while the table has <= 2 x lds_words slots (32-bit ranks, or
		 * 16-bit ones updated by compare-and-swap), else in global scratch (memory-side atomics). */
		const u32 batch = (T.m - i0 < thr - cnt) ? T.m - i0 : thr - cnt;
		const u32 nmask = n - 1;
		if (T.dbg & 2) { cnt += batch; i0 += batch; continue; }
		const u64 *src = rec_kc + T.rec_off + i0;
#define RP_PLACE(INIT, AMIN, LOAD)                                                                      \
		for (u32 i = tid; i < n; i += blockDim.x) { INIT(i, bm_get(cur, i)); }                              \
		__syncthreads();                                                                                    \
		for (u32 q0 = tid; q0 < batch; q0 += RP_U * blockDim.x) {       /* RP_U independent keys per lane in flight */ \
			u32 r[RP_U], slot[RP_U], old[RP_U], act = 0;                                                    \
			_Pragma("unroll")                                                                               \
			for (int u = 0; u < RP_U; ++u) {                                                                \
				const u32 q = q0 + u * blockDim.x;                                                          \
				if (q < batch) { r[u] = q + 1; slot[u] = yk_h2b((u32)(src[q] >> 10), bits); act |= 1u << u; } \
			}                                                                                               \
			while (act) {                                                                                   \
				_Pragma("unroll")                                                                           \
				for (int u = 0; u < RP_U; ++u) if (act >> u & 1) { AMIN(old[u], slot[u], r[u]); }           \
				_Pragma("unroll")                                                                           \
				for (int u = 0; u < RP_U; ++u)                                                              \
					if (act >> u & 1) {                                                                     \
						if (old[u] == EMPTYV) { act &= ~(1u << u); continue; }                              \
						if (old[u] > r[u]) r[u] = old[u];   /* we took the slot; carry the displaced later key on */ \
						slot[u] = (slot[u] + 1) & nmask;                                                    \
					}                                                                                       \
			}                                                                                               \
		}                                                                                                   \
		__syncthreads();                                                                                    \
		for (u32 i0 = 0; i0 < n; i0 += blockDim.x) {          /* one slot per lane; a wave's ballot is two bitmap words */ \
			const u32 i = i0 + tid;                                                                         \
			u32 o = 0;                                                                                      \
			if (i < n) { LOAD(o, i); }                                                                      \
			const bool fresh = i < n && o != 0 && o != EMPTYV;                                              \
			if (fresh) keys[i] = src[o - 1];                                                                \
			const u64 b = __ballot(fresh);                                                                  \
			if ((tid & 63) == 0 && i < n) { cur[i >> 5] |= (u32)b; if (i + 32 < n) cur[(i >> 5) + 1] |= (u32)(b >> 32); } \
		}                                                                                                   \
		__syncthreads();
		if (n <= lds_words) {
#define EMPTYV 0xffffffffu
#define INIT32(i, used) s_dyn[i] = (used) ? 0u : EMPTYV
#define AMIN32(old, slot, r) old = atomicMin(&s_dyn[slot], r)
#define LOAD32(o, i) o = s_dyn[i]
			RP_PLACE(INIT32, AMIN32, LOAD32)
#undef EMPTYV
		} else if (n <= 2 * lds_words && batch < 0xffffu) {
#define EMPTYV 0xffffu
#define INIT16(i, used) ((unsigned short*)s_dyn)[i] = (used) ? (unsigned short)0 : (unsigned short)0xffff
#define AMIN16(old, slot, r) { u32 *wp = &s_dyn[(slot) >> 1]; const u32 sh = 16 * ((slot) & 1); u32 seen = *(volatile u32*)wp;        \
				for (;;) { old = seen >> sh & 0xffffu; if (old <= (r)) break;                                                            \
				           const u32 got = atomicCAS(wp, seen, (seen & ~(0xffffu << sh)) | (r) << sh); if (got == seen) break; seen = got; } }
#define LOAD16(o, i) o = ((unsigned short*)s_dyn)[i]
			RP_PLACE(INIT16, AMIN16, LOAD16)
#undef EMPTYV
		} else if (scr_par && lds_words >= 1024 && (lds_words & (lds_words - 1)) == 0 && !(T.dbg & 256)) {
			/* larger tables: the same ordered probing, one segment of lds_words slots at a time with the
			 * ranks in LDS; a walk that reaches the end of its segment is parked as (rank, next slot) and
			 * finished afterwards on the written-back global array -- the fixed point of min-rank
			 * probing does not depend on the order in which the walks are made */
			const u32 SEG = lds_words, nseg = n / SEG;
			u64 *spill = scr_par + 2 * T.new_off;                    /* free between doublings; 2 x capacity entries */
			if (tid == 0) s_par[6] = 0;
			for (u32 seg = 0; seg < nseg; ++seg) {
				const u32 base = seg * SEG;
				for (u32 i = tid; i < SEG; i += blockDim.x) s_dyn[i] = bm_get(cur, base + i) ? 0u : 0xffffffffu;
				__syncthreads();
				for (u32 q = tid; q < batch; q += blockDim.x) {
					const u32 home = yk_h2b((u32)(src[q] >> 10), bits);
					if (home / SEG != seg) continue;
					u32 r = q + 1, li = home - base;
					for (;;) {
						const u32 old = atomicMin(&s_dyn[li], r);
						if (old == 0xffffffffu) break;
						if (old > r) r = old;
						if (++li == SEG) { spill[atomicAdd(&s_par[6], 1u)] = (u64)r << 32 | ((base + SEG) & nmask); break; }
					}
				}
				__syncthreads();
				for (u32 i = tid; i < SEG; i += blockDim.x) owner[base + i] = s_dyn[i];
				__syncthreads();
			}
			const u32 ns = s_par[6];
			for (u32 j = tid; j < ns; j += blockDim.x) {
				u32 r = (u32)(spill[j] >> 32), slot = (u32)spill[j];
				for (;;) {
					const u32 old = atomicMin(&owner[slot], r);
					if (old == 0xffffffffu) break;
					if (old > r) r = old;
					slot = (slot + 1) & nmask;
				}
			}
			__syncthreads();
			for (u32 i0 = 0; i0 < n; i0 += blockDim.x) {
				const u32 i = i0 + tid;
				const u32 o = __hip_atomic_load(&owner[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				const bool fresh = o != 0 && o != 0xffffffffu;
				if (fresh) keys[i] = src[o - 1];
				const u64 b = __ballot(fresh);
				if ((tid & 63) == 0) { cur[i >> 5] |= (u32)b; cur[(i >> 5) + 1] |= (u32)(b >> 32); }
			}
			__syncthreads();
		} else {
#define EMPTYV 0xffffffffu
#define INITG(i, used) owner[i] = (used) ? 0u : EMPTYV
#define AMING(old, slot, r) old = atomicMin(&owner[slot], r)
#define LOADG(o, i) o = __hip_atomic_load(&owner[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
			RP_PLACE(INITG, AMING, LOADG)
#undef EMPTYV
		}
		cnt += batch; i0 += batch;
		RP_TICK(n >= 32768 ? 3 : 2)
	}
	__syncthreads();
	if (keys == lkeys) { for (u32 i = tid; i < n; i += blockDim.x) gkeys[i] = lkeys[i]; __syncthreads(); keys = gkeys; }
	/* publish: bitmap in the arena, unused slots normalised to YK_EMPTY */
	if (cur != UA) for (u32 w = tid; w < (n + 31) / 32; w += blockDim.x) UA[w] = cur[w];
	for (u32 i = tid; i < n; i += blockDim.x) if (!bm_get(cur, i)) keys[i] = YK_EMPTY;
	RP_TICK(4)
	if (tid == 0) { out_bits[blockIdx.x] = n ? bits : YK_NOCAP; out_count[blockIdx.x] = cnt; }
}

