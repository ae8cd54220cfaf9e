/* kern_replay2.inc -- part of kernels.hip (one translation unit, included in this order): replay2: the exact layout of large sub-tables (k_r2_*: doubling rounds fused per sub-table, segment placement), shrink */
/* ==========================================================================================
 * K5 for LARGE sub-tables ("replay2").  k_replay gives one sub-table to one workgroup and walks global
 * arrays with random accesses and device atomics; that is fine up to a few thousand slots (everything in
 * LDS) and hopeless at a million (measured 2.7 s for 1024 x 2 Mi slots).  Two facts about khashl make
 * both steps of the replay LOCAL, streaming and free of global atomics:
 *
 * DOUBLING (khashl.h:171-189, n -> 2n slots).  A maximal run of used old slots (e, e') -- slots e and e'
 * unused -- holds keys whose old home lies inside the run, so their new homes lie in [2e + 2, 2e' - 1], and
 * for every h the run has at most e' - h keys with new home >= 2h: the run's keys end up inside the new
 * region [2e + 2, 2e' + 1] whatever the order, and no key of another run ever enters it.  Runs interact
 * only through the ORDER of re-insertion: the key at old slot s is kicked out early iff a key lands on
 * physical slot s before the scan reaches s.  Its processing time is therefore
 *     sigma(s) = (c, d + 1) if the final occupant x of new slot s has sigma(x) = (c, d) with c < s
 *                (s, 0)     otherwise,
 * and the final content of a region is first-come-first-served linear probing of its run's keys in sigma
 * order.  New slot s < 2F belongs to the region of a run below F (when slot F - 1 is unused), so once all
 * runs below F are placed, every run inside [F, 2F) can be placed at once, one lane per run, with plain
 * loads and stores on its own region; `tag` keeps sigma of the occupant of every new slot < n.  The first
 * few slots are done by the literal rule by one lane (chains followed while they stay in that prefix).
 *
 * PLACEMENT of the new keys of a stage (first come first served in rank order, khashl.h:197-221) is
 * ordered probing with the smallest rank winning a slot (order-free), done per segment of R2_SEG slots
 * with the ranks in LDS; the keys of the stage are first grouped by the segment of their home slot.  A walk
 * that leaves its segment is finished afterwards on the first R2_HEAD slots of the next segment, whose
 * ranks are kept in a global array for that purpose (device atomics, but only for these few walks).
 *
 * All sub-tables advance together, one kernel per step; the table of a sub-table alternates between two
 * buffers.  Anything unexpected (a run longer than the round, a walk longer than a head) raises `fail`
 * and the host falls back to k_replay.
 * ========================================================================================== */
#define R2_SEG_LOG 14
#define R2_SEG  (1u << R2_SEG_LOG)
#define R2_HEAD 2048u
#define R2_NONE 0xffffffffu
#define R2_SMALL_F 256u                       /* the single-workgroup kernel runs the doubling rounds up to here */
#define R2_BASE_MAX 4096u
#define R2_LONG 8u                             /* runs longer than this are placed by a whole wave */
#define R2_LMAX 512u
#define R2_RMAX (2 * R2_LMAX + 2 + 256)
#define R2_WS 512u                              /* k_r2_dsmall's LDS windows: old slots [0, R2_WS), new slots [0, R2_WD) */
#define R2_WD (2 * R2_WS + 64)
#define R2_MOVED (YK_EMPTY - 1)                 /* old slot whose key a chain of the prefix has re-inserted: still part of its run, no longer a key */

__device__ __forceinline__ u32 r2_home(u64 key, u32 bits) { return yk_h2b((u32)(key >> 10), bits); }

/* largest g in (F, x] such that old slot g - 1 is unused (g == n is always a boundary); 0 if there is none */
__device__ __forceinline__ u32 r2_boundary(const u64 *S, u32 F, u32 x, u32 n)
{
	if (x >= n) return n;
	u32 g = x;
	while (g > F && S[g - 1] != YK_EMPTY) --g;
	return g > F ? g : 0;
}

/* put `key`, whose processing time is (c, d), into the new table; while it lands on an unmoved key of the run [a, b)
 * that key is kicked out and follows at once with (c, d + 1) (khashl.h:183-187).  A key landing on an unmoved key of
 * ANOTHER run only leaves its tag: that run reads it when its round comes. */
__device__ __forceinline__ void r2_chain(u64 *S, u64 *D, u32 *TG, u32 *UB, u64 key, u32 c, u32 d, u32 a, u32 b, u32 n, u32 nb)
{
	const u32 Nmask = 2 * n - 1;
	for (;;) {
		u32 p = r2_home(key, nb);
		while (D[p] != YK_EMPTY) p = (p + 1) & Nmask;
		D[p] = key;
		if (UB) atomicOr(&UB[p >> 5], 1u << (p & 31));                     /* (global arrays only: the rare path of k_r2_dsmall) */
		if (p >= n) return;
		TG[p] = c << 6 | (d < 63 ? d : 63);
		if (p < a || p >= b) return;
		const u64 v = S[p];
		if (v == YK_EMPTY || v == R2_MOVED) return;
		key = v; S[p] = R2_MOVED; ++d;
	}
}

/* place the run of used old slots starting at a (slot a - 1 is unused).  First the keys kicked out by keys that are
 * already in place (tag with c < slot), in (c, d) order -- c lies below the run, so they all come before the run's own
 * scan positions; then the scan.  COH: the tags were written by other waves of this kernel (in-kernel rounds). */
template <bool COH>
__device__ __forceinline__ bool r2_run(u64 *S, u64 *D, u32 *TG, u32 *UB, u32 a, u32 n, u32 nb)      /* false: a long run, left to a wave */
{
	u32 b = a, nk = 0;
	for (; b < n && S[b] != YK_EMPTY; ++b) {
		if (b - a >= R2_LONG) return false;
		const u32 t = COH ? __hip_atomic_load(&TG[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : TG[b];
		nk += t != R2_NONE && (t >> 6) < b && S[b] != R2_MOVED;
	}
	u32 last = 0;                                                          /* tag + 1 of the last key taken */
	for (u32 it = 0; it < nk; ++it) {
		u32 best = R2_NONE, bs = a;
		for (u32 s = a; s < b; ++s) {
			if (S[s] == R2_MOVED) continue;
			const u32 t = COH ? __hip_atomic_load(&TG[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : TG[s];
			if (t == R2_NONE || (t >> 6) >= s) continue;
			if (t + 1 > last && t < best) { best = t; bs = s; }               /* tags order like (c, d) */
		}
		if (best == R2_NONE) break;                                           /* the others left with a chain */
		last = best + 1;
		const u64 key = S[bs];
		S[bs] = R2_MOVED;
		r2_chain(S, D, TG, UB, key, best >> 6, (best & 63u) + 1, a, b, n, nb);
	}
	for (u32 s = a; s < b; ++s) {
		const u64 key = S[s];
		if (key == R2_MOVED) continue;
		S[s] = R2_MOVED;
		r2_chain(S, D, TG, UB, key, s, 0, a, b, n, nb);
	}
	return true;
}

/* A long run is placed by a whole wave on LDS copies.  In a round all tags a run reads are final, its kicked keys
 * all precede its scan positions, and no chain continues inside it (its region starts at 2a >= b): first come first
 * served in sigma order is then ordered probing with priority = rank in sigma order, all keys at once.  DYN: the run
 * covers [F, 2F] and feeds its own slots (only below R2_SMALL_F): one lane walks it with the literal rule, on LDS. */
template <u32 LM> struct R2WaveT {                     /* LM: longest run the buffers hold; its region + the shared wrap-around head */
	static constexpr u32 LMAX = LM, RMAX = 2 * LM + 2 + 256;
	u64 keys[LM]; u32 sig[LM]; u32 own[2 * LM + 2 + 256]; unsigned short byrank[LM], rk[LM]; u32 mv[LM / 32];
};
typedef R2WaveT<R2_LMAX> R2Wave;
#define R2_MMAX 192u                                  /* "medium" runs: placed by the wave that met them, in the LDS of its chunk (k_r2_double) */
typedef R2WaveT<R2_MMAX> R2WaveM;

__device__ __forceinline__ void r2_wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

/* bitmap words of the 64 consecutive new slots from the 64-aligned slot qa on: `set` = lanes whose slot holds a key, `mine` = lanes whose slot this wave
 * owns (set is a subset of mine).  A 32-bit word that is all ours is stored; one we share with another wave is OR-ed (k_r2_binit zeroed it) */
__device__ __forceinline__ void r2_used_words(u32 *UB, u32 qa, u64 set, u64 mine)
{
	const u32 lane = threadIdx.x & 63;
	if ((lane & 31) == 0) {
		const u32 w = (u32)(lane ? set >> 32 : set), m = (u32)(lane ? mine >> 32 : mine);
		u32 *p = UB + (qa >> 5) + (lane >> 5);
		if (m == 0xffffffffu) *p = w;
		else if (w) atomicOr(p, w);
	}
}

/* COH: S / D / TG are the global arrays, and the run OWNS its region of the new table: nothing has emptied D before (k_r2_dinit is gone), so the slots
 * a prefix chain took come from the OC bitmap instead of D, every slot of the region is written -- key or empty pattern, tag or R2_NONE -- and the
 * region's bits of the occupancy bitmap UB go out with it.  Only the part of the last run's region that wraps around to the first slots of the table
 * (finished by k_r2_dsmall, emptied there) is read from D and left alone where no key lands.  !COH: LDS windows, the old rule (read D, write keys) */
template <bool COH, bool DYN, class WT>
__device__ __forceinline__ void r2_wave_run(WT &W, u64 *S, u64 *D, u32 *TG, const u32 *OC, u32 *UB, u32 a, u32 n, u32 nb, u32 *fail)
{
	constexpr u32 R2_LMAX_ = WT::LMAX, R2_RMAX_ = WT::RMAX;
	const u32 lane = threadIdx.x & 63, Nmask = 2 * n - 1;
	u32 L = 0;
	for (;;) {                                                              /* length of the run */
		const u32 idx = a + L + lane;
		const u64 m = __ballot(idx < n && S[idx] != YK_EMPTY);
		if (m == ~0ull) { L += 64; if (L > R2_LMAX_) break; continue; }
		L += (u32)__ffsll((long long)~m) - 1;
		break;
	}
	u32 wrap = 0;
	if (a + L >= n) {                                                       /* the run that reaches the end of the table shares its region with the table's first run */
		u32 j0 = 0;
		while (j0 < 128 && S[j0] != YK_EMPTY) ++j0;
		wrap = 2 * j0 + 2;
	}
	const u32 R = 2 * L + 2 + wrap;
	if (L > R2_LMAX_ || R > R2_RMAX_) { if (lane == 0) *fail = 6; return; }
	const u32 Rn = 2 * n - 2 * a < R ? 2 * n - 2 * a : R;                   /* entries [0, Rn) lie before the end of the table, [Rn, R) are its first slots */
	for (u32 i = lane; i < L; i += 64) {
		const u32 sl = a + i;
		const u64 k = S[sl];
		const u32 t = COH ? __hip_atomic_load(&TG[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : TG[sl];
		W.keys[i] = k;
		W.sig[i] = k == R2_MOVED ? R2_NONE : (t != R2_NONE && (t >> 6) < sl) ? ((t & ~63u) | ((t & 63u) < 62 ? (t & 63u) + 1 : 63u)) : sl << 6;
	}
	for (u32 i = lane; i < R; i += 64) {
		const u32 slot = (2 * a + i) & Nmask;
		const bool taken = (COH && i < Rn) ? (OC[slot >> 5] >> (slot & 31) & 1) != 0 : D[slot] != YK_EMPTY;
		W.own[i] = taken ? 0u : 0xffffffffu;
	}
	if (lane < R2_LMAX_ / 32) W.mv[lane] = 0;
	r2_wave_sync();
	for (u32 i = lane; i < L; i += 64) {                                    /* rank in sigma order */
		const u32 g = W.sig[i];
		if (g == R2_NONE) continue;
		u32 r = 0;
		for (u32 j = 0; j < L; ++j) r += W.sig[j] < g;
		W.rk[i] = (unsigned short)r; W.byrank[r] = (unsigned short)i;
	}
	r2_wave_sync();
	if (!DYN) {
		for (u32 i = lane; i < L; i += 64) {
			if (W.sig[i] == R2_NONE) continue;
			u32 r = (u32)W.rk[i] + 1, li = (r2_home(W.keys[i], nb) - 2 * a) & Nmask;
			for (;;) {
				if (li >= R) { *fail = 7; break; }
				const u32 old = atomicMin(&W.own[li], r);
				if (old == 0xffffffffu) break;
				if (old > r) r = old;
				++li;
			}
		}
		r2_wave_sync();
		for (u32 i = lane; i < R; i += 64) { const u32 o = W.own[i]; if (o != 0 && o != 0xffffffffu) W.own[i] = (u32)W.byrank[o - 1] + 1; }
	} else if (lane == 0) {
		u32 nv = 0;
		for (u32 i = 0; i < L; ++i) nv += W.sig[i] != R2_NONE;
		auto chain = [&](u32 i, u32 c, u32 d) {
			for (;;) {
				W.mv[i >> 5] |= 1u << (i & 31);
				W.sig[i] = c << 6 | (d < 63 ? d : 63);
				u32 li = (r2_home(W.keys[i], nb) - 2 * a) & Nmask;
				while (li < R && W.own[li] != 0xffffffffu) ++li;
				if (li >= R) { *fail = 7; return; }
				W.own[li] = i + 1;
				const u32 slot = (2 * a + li) & Nmask;
				if (slot < a || slot >= a + L) return;
				const u32 v = slot - a;
				if (W.sig[v] == R2_NONE || (W.mv[v >> 5] >> (v & 31) & 1)) return;
				i = v; ++d;                                                  /* an unmoved key of the run sits there: it follows at once */
			}
		};
		for (u32 r = 0; r < nv; ++r) {                                       /* the keys kicked out from below come first, in sigma order */
			const u32 i = W.byrank[r];
			if (W.mv[i >> 5] >> (i & 31) & 1) continue;                     /* left with a chain already (its time has been overwritten) */
			const u32 g = W.sig[i];
			if ((g & 63u) == 0) break;
			chain(i, g >> 6, g & 63u);
		}
		for (u32 i = 0; i < L; ++i)
			if (W.sig[i] != R2_NONE && !(W.mv[i >> 5] >> (i & 31) & 1)) chain(i, a + i, 0);
	}
	r2_wave_sync();
	if (COH) {
		/* the region before the end of the table, 64 aligned slots at a time: whole-line stores, the bitmap words from ballots */
		const u32 q0 = 2 * a, q1 = 2 * a + Rn;                               /* [q0, q1) */
		for (u32 qa = q0 & ~63u; qa < q1; qa += 64) {
			const u32 q = qa + lane;
			const bool in = q >= q0 && q < q1;
			const u32 o = in ? W.own[q - q0] : 0u;
			const bool put = in && o != 0 && o != 0xffffffffu;
			if (put) { D[q] = W.keys[o - 1]; if (q < n) TG[q] = W.sig[o - 1]; }
			else if (in && o == 0xffffffffu) { D[q] = YK_EMPTY; if (q < n) TG[q] = R2_NONE; }
			r2_used_words(UB, qa, __ballot(put), 0ull);                       /* (always OR-ed: the chunk that met this run leaves its words alone) */
		}
		for (u32 i = Rn + lane; i < R; i += 64) {                            /* the last run's keys among the table's first slots */
			const u32 o = W.own[i];
			if (o == 0 || o == 0xffffffffu) continue;
			const u32 slot = (2 * a + i) & Nmask;
			D[slot] = W.keys[o - 1];
			if (slot < n) TG[slot] = W.sig[o - 1];
			atomicOr(&UB[slot >> 5], 1u << (slot & 31));
		}
	} else {
		for (u32 i = lane; i < R; i += 64) {
			const u32 o = W.own[i];
			if (o == 0 || o == 0xffffffffu) continue;
			const u32 slot = (2 * a + i) & Nmask;
			D[slot] = W.keys[o - 1];
			if (slot < n) TG[slot] = W.sig[o - 1];
		}
	}
	if (DYN) for (u32 i = lane; i < L; i += 64) if (W.sig[i] != R2_NONE) S[a + i] = R2_MOVED;
}

/* R2Tab: first slot in the two buffers, first sorted new key.  R2Act: kind 0 nothing, 1 place, 2 double; bits = log2 capacity before
 * the action; src = buffer (0/1) holding the table; seg0 = first entry of this sub-table in the per-segment arrays (yk_device.h) */

/* The sub-tables that double in this step: no bit in the two bitmaps of the new table -- OC (slots a chain of the prefix took, k_r2_dsmall) and UB
 * (slots that hold a key once the doubling is through: what the placement behind it reads instead of the table).  Until round 6 this kernel also
 * wrote the empty pattern into every slot of the new table and R2_NONE into every tag (k_r2_dinit: 43 GB of fills beside a 1 Gb assembly); the
 * doubling's waves now write whole regions, empties included */
__global__ __launch_bounds__(256)
void k_r2_binit(const R2Tab *tabs, const R2Act *acts, u32 *OCC, u32 *USED)
{
	const R2Act A = acts[blockIdx.y];
	if (A.kind != 2) return;
	const u64 off = tabs[blockIdx.y].off;
	const u64 W = ((2ull << A.bits) + 31) / 32;
	u32 *OC = OCC + (off >> 4), *UB = USED + (off >> 5);                /* (UB is indexed like the table: the placement reads it at (off + slot) / 32) */
	for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < W; i += (u64)gridDim.x * 256) { OC[i] = 0; UB[i] = 0; }
}

/* the doubling rounds [F, G), G <= 2F, of ONE sub-table by one workgroup, until F reaches small_f.  COH: S / D / TG are the global
 * arrays (cross-wave data through L2: fences and agent-scope loads); else they are LDS windows holding slots [0, ws_lim) of the
 * old table and [0, 2 ws_lim + 64) of the new one -- every access of a round stays below 2G + 2 -- and the function returns early
 * (*s_dyn = 2) if a self-feeding run would leave the window */
template <bool COH>
__device__ u32 r2_small_rounds(u64 *S, u64 *D, u32 *TG, const u32 *OC, u32 *UB, u32 F, const u32 n, const u32 nb, const u32 small_f, const u32 ws_lim,
                               R2Wave *waves, const u32 n_waves, u32 *s_long, u32 *s_F, u32 *s_dyn, u32 *s_nlong, u32 *fail)
{
	const u32 tid = threadIdx.x;
	while (F < n && F < small_f) {
		if (tid == 0) {
			u32 g = r2_boundary(S, F, 2 * F < n ? 2 * F : n, n);
			*s_dyn = 0; *s_nlong = 0;
			if (g == 0) {
				/* one run covers [F, 2F]: the keys landing on its slots come from the run itself; it is placed alone, by the
				 * literal rule in sigma order (r2_wave_run<.., true>), up to its own end */
				*s_dyn = 1;
				g = 2 * F;
				while (g < n && S[g] != YK_EMPTY) { ++g; if (!COH && g + 1 >= ws_lim) { *s_dyn = 2; break; } }
				g = g < n ? g + 1 : n;
			}
			*s_F = g;
		}
		__syncthreads();
		const u32 G = *s_F;
		if (*s_dyn == 2) break;                                              /* (uniform) */
		if (*s_dyn) { if (tid < 64) r2_wave_run<COH, true>(waves[0], S, D, TG, OC, UB, F, n, nb, fail); }
		else {
			for (u32 s = F + tid; s < G; s += blockDim.x)
				if (S[s] != YK_EMPTY && (s == F || S[s - 1] == YK_EMPTY) && !r2_run<COH>(S, D, TG, UB, s, n, nb)) {
					const u32 at = atomicAdd(s_nlong, 1u);
					if (at < 256) s_long[at] = s; else *fail = 8;
				}
			__syncthreads();
			const u32 nl = *s_nlong < 256 ? *s_nlong : 256;
			if (tid < 64 * n_waves) for (u32 j = tid >> 6; j < nl; j += n_waves) r2_wave_run<COH, false>(waves[tid >> 6], S, D, TG, OC, UB, s_long[j], n, nb, fail);
		}
		if (COH) __threadfence();
		__syncthreads();
		F = G;
	}
	return F;
}

/* the prefix by the literal rule, then the rounds below R2_SMALL_F; one workgroup per sub-table.  Nothing has emptied the new table (k_r2_binit only
 * zeroes the bitmaps): what this kernel finishes on its LDS windows goes out as whole windows -- slots [0, nd) of D, tags [0, nt), empties included --
 * and k_r2_double writes whole regions from there on.  The rare cases that work on the global arrays instead (a first run or a chain beyond the windows,
 * small_f beyond them: tests) first give the sub-table what k_r2_dinit used to give every one: the empty pattern in every slot, R2_NONE in every tag */
__global__ __launch_bounds__(256)
void k_r2_dsmall(const R2Tab *tabs, const R2Act *acts, u64 *K0, u64 *K1, u32 *TAG, u32 *OCC, u32 *USED, u32 *Fcur, u32 *Gcur, u32 *fail, u32 small_f, int defer)
{
	__shared__ R2Wave s_wave[1];
	__shared__ u64 s_S[R2_WS], s_D[R2_WD];                              /* 31 KB in all: the 1024 workgroups of a launch are resident at once */
	__shared__ u32 s_T[R2_WD];
	__shared__ u32 s_long[256];
	__shared__ u32 s_F, s_dyn, s_nlong;
	const u32 p = blockIdx.x, tid = threadIdx.x;
	const R2Act A = acts[p];
	if (A.kind != 2) return;
	const u64 off = tabs[p].off;
	const u32 n = 1u << A.bits, nb = A.bits + 1, Nmask = 2 * n - 1;
	u64 *S = (A.src ? K1 : K0) + off;
	u64 *D = (A.src ? K0 : K1) + off;
	u32 *TG = TAG + (off >> 1);
	u32 *OC = OCC + (off >> 4);
	u32 *UB = USED + (off >> 5);
	const u32 ns = n < R2_WS ? n : R2_WS, nd = 2 * n < R2_WD ? 2 * n : R2_WD, nt = n < R2_WD ? n : R2_WD;
	__shared__ u32 s_bail;
	/* The literal rule (khashl.h:171-189) for the scan positions below F0.  A kicked-out key leaves a tombstone: its slot still belongs to
	 * its run.  A chain is followed while it stays inside the prefix (whose slots feed each other) and wherever it meets the run that may
	 * touch the end of the table (that run shares its region with the table's first run: its kicked keys must be in place, in the
	 * reference's order, before the first run's later keys).  Anywhere else the key that lands on an unmoved key of another run just leaves
	 * its tag, exactly as in the rounds (r2_chain): that run takes its kicked keys first, in (c, d) order, when its round comes -- the chain's
	 * remaining steps (one dependent global access each, ~log2 n of them) are not walked by this one lane.  defer == 0: every chain to its end.
	 * With deferred chains on a table of >= 2048 slots everything the prefix touches lies in the first few hundred slots of both tables: the
	 * lane walks LDS copies (the new table and its tags start empty: no load), the OC marks are applied afterwards.  An access
	 * that leaves the windows after all (a long first run) drops the copies, nothing global having been written, and the lane starts over
	 * on the arrays */
	bool have_win = false;
	if (defer && n >= 2048) {
		/* A prefix key whose old home lies at the END of the table (the old table's last run wrapped around to slot 0: every third sub-table or so)
		 * has its new home there too: the last R2_WD slots of the new table are emptied here and probed where they lie, by the same lane */
		const u32 tz = 2 * n - R2_WD;                                     /* (2n >= 4096: the two zones are apart) */
		for (u32 i = tid; i < ns; i += 256) s_S[i] = __hip_atomic_load(&S[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		for (u32 i = tid; i < nd; i += 256) s_D[i] = YK_EMPTY;
		for (u32 i = tid; i < nt; i += 256) s_T[i] = R2_NONE;
		for (u32 i = tid; i < R2_WD; i += 256) D[tz + i] = YK_EMPTY;
		if (tid == 0) { s_bail = 0; s_nlong = 0; }
		__threadfence();
		__syncthreads();
		if (tid == 0) {
			u32 F0 = 8, nl = 0;
			bool bail = false;
			while (F0 < ns && s_S[F0 - 1] != YK_EMPTY) ++F0;
			if (F0 >= ns) bail = true;
			for (u32 j = 0; j < F0 && !bail; ++j) {
				u64 key = s_S[j];
				if (key == YK_EMPTY || key == R2_MOVED) continue;
				u32 d = 0;
				s_S[j] = R2_MOVED;
				for (;;) {
					u32 q = r2_home(key, nb);
					for (;;) {
						if (q < nd) { if (s_D[q] == YK_EMPTY) break; }
						else if (q >= tz) { if (__hip_atomic_load(&D[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == YK_EMPTY) break; }
						else { bail = true; break; }
						q = (q + 1) & Nmask;
					}
					if (bail || nl >= 256) { bail = true; break; }              /* (n >= 2048: nt == nd, a slot of the lower window has a tag entry) */
					s_long[nl++] = q;
					if (q >= tz) { D[q] = key; break; }                        /* in the upper half: no tag, nobody to kick out */
					s_D[q] = key;
					s_T[q] = j << 6 | (d < 63 ? d : 63);
					if (q >= F0) break;                                         /* the run of slot q reads the tag in its round (q is far below the table's last run) */
					const u64 v = s_S[q];
					if (v == YK_EMPTY || v == R2_MOVED) break;
					key = v; s_S[q] = R2_MOVED; ++d;                           /* an unmoved key of the prefix sits there: kick it out */
				}
			}
			if (bail) s_bail = 1;
			else {
				for (u32 i = 0; i < nl; ++i) { const u32 q = s_long[i]; OC[q >> 5] |= 1u << (q & 31); if (q >= tz) atomicOr(&UB[q >> 5], 1u << (q & 31)); }
				s_F = F0;
			}
		}
		__syncthreads();
		have_win = s_bail == 0;
	}
	bool on_arrays = !have_win;                                          /* (uniform) the global arrays are worked on: they hold the empty pattern / R2_NONE everywhere first */
	if (!have_win) {
		for (u32 i = tid; i < 2 * n; i += 256) D[i] = YK_EMPTY;
		for (u32 i = tid; i < n; i += 256) TG[i] = R2_NONE;
		__threadfence();
		__syncthreads();
		if (tid == 0) {
			u32 F0 = n < 8 ? n : 8;
			while (F0 < n && S[F0 - 1] != YK_EMPTY) ++F0;               /* slot F0 - 1 unused (or F0 == n) */
			if (F0 > R2_BASE_MAX && F0 < n) *fail = 1;
			const u32 tail0 = n > R2_LMAX + 2 ? n - (R2_LMAX + 2) : 0;     /* a run reaching slot n - 1 starts behind this slot (longer runs are refused) */
			for (u32 j = 0; j < F0; ++j) {
				u64 key = S[j];
				if (key == YK_EMPTY || key == R2_MOVED) continue;
				u32 d = 0;
				S[j] = R2_MOVED;
				for (;;) {
					u32 q = r2_home(key, nb);
					while (D[q] != YK_EMPTY) q = (q + 1) & Nmask;
					D[q] = key;
					OC[q >> 5] |= 1u << (q & 31);
					atomicOr(&UB[q >> 5], 1u << (q & 31));
					if (q >= n) break;
					TG[q] = j << 6 | (d < 63 ? d : 63);
					if (defer && q >= F0 && q < tail0) break;                /* the run of slot q reads the tag in its round */
					const u64 v = S[q];
					if (v == YK_EMPTY || v == R2_MOVED) break;
					key = v; S[q] = R2_MOVED; ++d;                          /* an unmoved key sits there: kick it out */
				}
			}
			s_F = F0;
		}
		__threadfence();
		__syncthreads();
	}
	u32 F = s_F;
	const bool do_small = small_f <= R2_WS / 2 && F < small_f && F < n;
	if (have_win || do_small) {
		/* the rounds below small_f touch old slots < 2 small_f and new slots < 4 small_f + 2 only: they run on LDS copies (a dependent
		 * access costs ~100 cycles there instead of a trip to L2), the windows go back to the arrays afterwards */
		if (!have_win) {
			for (u32 i = tid; i < ns; i += 256) s_S[i] = __hip_atomic_load(&S[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			for (u32 i = tid; i < nd; i += 256) s_D[i] = __hip_atomic_load(&D[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			for (u32 i = tid; i < nt; i += 256) s_T[i] = __hip_atomic_load(&TG[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		__syncthreads();
		if (do_small) F = r2_small_rounds<false>(s_S, s_D, s_T, 0, 0, F, n, nb, small_f, R2_WS, s_wave, 1, s_long, &s_F, &s_dyn, &s_nlong, fail);
		__syncthreads();
		if (!on_arrays && F < n && F < small_f) {                           /* (uniform) rounds on the arrays follow: everything behind the windows empty first */
			on_arrays = true;
			for (u32 i = nd + tid; i < 2 * n; i += 256) D[i] = YK_EMPTY;
			for (u32 i = nt + tid; i < n; i += 256) TG[i] = R2_NONE;
		}
		for (u32 i = tid; i < ns; i += 256) S[i] = s_S[i];
		for (u32 i = tid; i < nd; i += 256) D[i] = s_D[i];
		for (u32 i = tid; i < nt; i += 256) TG[i] = s_T[i];
		/* every key the windows hold is in its final slot (below 2F: the regions of the runs that are through; beyond: a prefix chain's key, OC-marked) */
		for (u32 i0 = 0; i0 < nd; i0 += 256) {
			const u32 i = i0 + tid;
			const u64 b = __ballot(i < nd && s_D[i] != YK_EMPTY);
			if ((tid & 31) == 0 && i < nd) { const u32 w = (u32)((tid & 32) ? b >> 32 : b); if (w) atomicOr(&UB[i >> 5], w); }
		}
		__threadfence();
		__syncthreads();
	}
	F = r2_small_rounds<true>(S, D, TG, OC, UB, F, n, nb, small_f, 0, s_wave, 1, s_long, &s_F, &s_dyn, &s_nlong, fail);   /* whatever is left (a run that left the window; small_f beyond the window) */
	if (tid == 0) Fcur[p] = F;                                                /* k_r2_double goes on from here */
	(void)Gcur;
}

/* ------------------------------------------------------------------------------------------
 * The whole doubling of a sub-table in ONE launch, one workgroup per sub-table (k_r2_double).  Nothing leaves the workgroup, so the
 * rounds [F, G) follow each other behind workgroup barriers instead of kernel boundaries (k_r2_dsmall + ~11 x (k_r2_dround + k_r2_long)
 * took 25 launches per doubling, the big ones bound by the dispatcher, the small ones by launch latency).  Inside a round the waves
 * take the chunks of F2_CH old slots in turn, each on LDS buffers of its own (wave-level synchronisation only): the chunk routine of
 * k_r2_dround with a window for runs of up to F2_CHL slots; a longer run is placed by the wave that met it right after the chunk, in
 * the same LDS (up to R2_MMAX slots), and the few beyond that by wave 0 at the end of the round (up to R2_LMAX).  The boundary of the
 * next round is looked up by wave 0 while the others already place.
 * ------------------------------------------------------------------------------------------ */
#define F2_CH  128u                             /* old slots a wave owns per step */
#define F2_NA  256u                             /* window entries: old slots c0 - 1 ... c0 + 254 (four per lane) */
#define F2_WN  (2 * F2_NA)                      /* new slots 2 c0 ... 2 c0 + 511: the regions of the runs that start in the chunk and end inside the window */
#define F2_NOC (F2_WN / 32 + 2)
#define F2_LST 24u
struct R2Chunk {
	union {
		struct { u64 key[F2_NA]; u64 win[F2_WN + 1]; u32 oc[F2_NOC]; } c;        /* win[F2_WN]: where a walk that leaves the window ends (checked once per chunk) */
		R2WaveM m;                                                             /* the same memory while a medium run is placed */
	} u;
	u32 lst[F2_LST]; u32 nlst, pad;                                            /* runs of this chunk left to the wave routine */
	u32 xr[F2_LST];                                                            /* their regions inside the window (first | last << 16): not the chunk's to write */
};

/* largest g in (F, x] such that old slot g - 1 is unused (g == n is always a boundary); 0 if there is none.  One wave, 64 slots per step */
__device__ __forceinline__ u32 r2_boundary_wave(const u64 *S, u32 F, u32 x, u32 n)
{
	const u32 lane = threadIdx.x & 63;
	if (x >= n) return n;
	for (;;) {
		const u32 g = x - lane;                                                /* candidates x, x - 1, ..., x - 63 */
		const bool hit = x >= lane && g > F && S[g - 1] == YK_EMPTY;
		const u64 m = __ballot(hit);
		if (m) return x - ((u32)__ffsll((long long)m) - 1);
		if (x < 64 + F + 1) return 0;
		x -= 64;
	}
}

/* LDS traffic of ONE wave is served in issue order: a compiler barrier is all that lies between a phase's writes and the next phase's
 * reads -- no s_waitcnt, so the global loads requested for the next chunk stay in flight (a fence or __syncthreads() here waits vmcnt(0):
 * gfx950 counts loads and stores on one counter) */
__device__ __forceinline__ void r2_lds_phase() { __builtin_amdgcn_wave_barrier(); asm volatile("" ::: "memory"); }

/* The part of the round [F, G) that belongs to this wave: the runs behind the unused old slots e in [B0 - 1, B1 - 1), B0 = F + wave * len -- a contiguous
 * share, so that the wave's windows follow each other: a window starts AT an unused slot s0 (entry x <-> old slot s0 + x, lane l holds x = l + 64 j),
 * takes every run that ends inside it, and the next one starts at the last unused slot it saw.  Round 6 rewrote this for instruction count -- the kernel
 * issues, it does not wait (SQ counters at a 1 Gb assembly: 800 VALU + 740 SALU wave-instructions per 128 old slots, both issue ports ~60 % busy):
 *  - before, the waves took chunks of 128 slots in turn and each looked at 201 entries to see the ends of its runs; now ~245 of a window's 256 entries
 *    are its own, and "is this key mine" is one compare (x < up) instead of a search through four ballot masks per lane;
 *  - a key that has found its slot turns into the null entry ~0, which no atomicMin notices: the walks need no flags and no per-step bounds check (a
 *    walk that leaves the window ends on a sentinel entry, looked at once per window);
 *  - the write-back is one predicated store per array and step (key or empty pattern, tag or R2_NONE): EVERY slot of the window's part of the new table
 *    is written (nothing has emptied it), 64 aligned slots per step, and the ballot of "holds a key" is the pair of bitmap words the placement behind
 *    this doubling reads instead of the table;
 *  - only a run longer than a window (or the one that reaches the end of the table and shares its region with the table's first run) goes to the wave
 *    routine (round 5: every run from 64 slots on, 8 % of the kernel's time) */
template <bool PROF, u32 IL>
__device__ __forceinline__ void r2_round_wave(R2Chunk &C, const u64 *S, u64 *D, u32 *TG, const u32 *OC, u32 *UB, const u32 F, const u32 G, const u32 n, const u32 nb,
                                              const u32 wave, const u32 n_waves, u32 *s_big, u32 *s_nbig, u32 *fail, u64 *pf, u64 &tq)
{
	const u32 lane = threadIdx.x & 63;
#define R2W_LAP(i) if (PROF) { const u64 t_ = wall_clock64(); pf[i] += t_ - tq; tq = t_; }
	constexpr u32 PER = F2_NA / 64;
	static_assert(PER == 4, "four 64-bit masks cover the window");
	const u32 len = ((G - F + n_waves - 1) / n_waves + 63) & ~63u;
	const u32 B0 = F + wave * len, B1 = B0 + len < G ? B0 + len : G;
	if (B0 >= G) return;
	u32 s0 = B0 - 1;                                                         /* (wave 0: slot F - 1 is unused) */
	if (wave) {                                                               /* first unused slot at or behind B0 - 1 */
		for (;;) {
			const u32 idx = s0 + lane;
			const u64 m = __ballot(idx >= B1 - 1 || S[idx] == YK_EMPTY);
			if (m) { s0 += (u32)__ffsll((long long)m) - 1; break; }
			s0 += 64;
		}
	}
	u64 rk[PER]; u32 rt[PER], roc = 0;
	auto fetch = [&](const u32 s) {
#pragma unroll
		for (u32 j = 0; j < PER; ++j) {
			const u32 sl = s + lane + 64 * j;
			const u32 cl = sl < n ? sl : n - 1;
			rk[j] = S[cl]; rt[j] = __hip_atomic_load(&TG[cl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		roc = OC[((2 * s + 2) >> 5) + (lane < F2_NOC ? lane : 0)];
	};
	auto run_len = [&](const u32 a) {                                        /* slots of the run that starts at a (beyond R2_LMAX: some larger number) */
		u32 L = 0;
		for (;;) {
			const u32 idx = a + L + lane;
			const u64 m = __ballot(idx < n && S[idx] != YK_EMPTY);
			if (m == ~0ull) { L += 64; if (L > R2_LMAX) break; continue; }
			L += (u32)__ffsll((long long)~m) - 1;
			break;
		}
		return L;
	};
	auto hand_over = [&](const u32 a, const u32 L) {                          /* a run for the wave routine: here and now if this wave's LDS holds it, else wave 0 behind the round */
		if (L <= R2_MMAX) r2_wave_run<true, false>(C.u.m, (u64*)S, D, TG, OC, UB, a, n, nb, fail);
		else if (lane == 0) { const u32 at = atomicAdd(s_nbig, 1u); if (at < 64) s_big[at] = a; else *fail = 8; }
		r2_wave_sync();
	};
	if (s0 < B1 - 1) fetch(s0);
	while (s0 < B1 - 1) {
		const u32 c0 = s0 + 1, w0 = 2 * c0;
		u64 kc[PER], E[PER]; u32 tc[PER];
#pragma unroll
		for (u32 j = 0; j < PER; ++j) {
			const u32 x = lane + 64 * j, sl = s0 + x;
			kc[j] = sl < n ? rk[j] : YK_EMPTY; tc[j] = rt[j];
			C.u.c.key[x] = kc[j];
			E[j] = __ballot(kc[j] == YK_EMPTY);
		}
		const u32 oc_cur = roc;
		const bool any_oc = __ballot(lane < F2_NOC && oc_cur != 0) != 0;      /* slots a chain of the prefix took: only near the two ends of the table */
		if (any_oc && lane < F2_NOC) C.u.c.oc[lane] = oc_cur;
		/* up: the window takes the runs behind its unused entries below `up`, the next window starts at entry `up` (all of this is wave-uniform).
		 * Normally the last unused entry of the window; the first one at or behind `lim` where this wave's share ends; and where the table ends with a
		 * used slot, the last real unused entry -- the run behind it goes to the wave routine (it shares its region with the table's first run) */
		const u32 lim = B1 - 1 - s0;
		u32 hiu = 0;                                                           /* last unused entry (entry 0 is one) */
#pragma unroll
		for (u32 j = 0; j < PER; ++j) if (E[j]) hiu = 64 * j + 63 - (u32)__clzll((long long)E[j]);
		u32 e1 = F2_NA;                                                        /* first unused entry at or behind lim */
#pragma unroll
		for (int j = (int)PER - 1; j >= 0; --j) {
			const u32 lo = 64u * (u32)j;
			u64 m = E[j];
			if (lim > lo) m = lim - lo >= 64 ? 0ull : m & (~0ull << (lim - lo));
			if (m) e1 = lo + (u32)__ffsll((long long)m) - 1;
		}
		u32 up = e1 < F2_NA ? e1 : hiu;
		const bool tail_run = e1 < F2_NA && s0 + e1 >= n;                       /* (only in the table's last round: slot n - 1 is used, the entries from slot n on are no slots) */
		if (tail_run) {
			up = 0;
#pragma unroll
			for (u32 j = 0; j < PER; ++j) {
				const u32 lo = 64u * (u32)j, top = n - s0;                          /* entries below top are slots */
				u64 m = E[j];
				if (top < lo + 64) m = top <= lo ? 0ull : m & ~(~0ull << (top - lo));
				if (m) up = lo + 63 - (u32)__clzll((long long)m);
			}
		}
		const bool giant = up == 0 && !tail_run;                               /* the run behind s0 does not end inside the window */
		const u32 s1 = s0 + up;
		if (!giant && !tail_run && s1 < B1 - 1) fetch(s1);
		r2_lds_phase();
		R2W_LAP(0)
		if (up) {
			if (!any_oc) {
#pragma unroll
				for (u32 t = 0; t < F2_WN / 64; ++t) C.u.c.win[lane + 64 * t] = ~0ull;
			} else {
				for (u32 i = lane; i < F2_WN; i += 64) {
					const u32 q = w0 + i, b = (w0 & 31) + i;
					C.u.c.win[i] = (q < 2 * n && (C.u.c.oc[b >> 5] >> (b & 31) & 1)) ? 0ull : ~0ull;
				}
			}
			if (lane == 0) C.u.c.win[F2_WN] = ~0ull;
			r2_lds_phase();
			R2W_LAP(1)
			u64 pe[PER]; u32 pq[PER];
#pragma unroll
			for (u32 j = 0; j < PER; ++j) {
				const u32 x = lane + 64 * j, sl = s0 + x, t = tc[j];
				const u64 key = kc[j];
				const u32 sig = (t != R2_NONE && (t >> 6) < sl) ? ((t & ~63u) | ((t & 63u) < 62 ? (t & 63u) + 1 : 63u)) : sl << 6;
				pe[j] = (x < up && key != YK_EMPTY && key != R2_MOVED) ? (u64)(sig + 1) << 32 | x : ~0ull;
				const u32 h = r2_home(key, nb) - w0;
				pq[j] = h < F2_WN ? h : F2_WN;
			}
#pragma unroll
			for (u32 j0 = 0; j0 < PER; j0 += IL) {
				for (;;) {
					bool any = false;
#pragma unroll
					for (u32 jl = 0; jl < IL; ++jl) any = any || pe[j0 + jl] != ~0ull;
					if (!__ballot(any)) break;
#pragma unroll
					for (u32 jl = 0; jl < IL; ++jl) {
						const u32 j = j0 + jl;
						if (pe[j] != ~0ull) {
							const u64 old = atomicMin((unsigned long long*)&C.u.c.win[pq[j]], (unsigned long long)pe[j]);
							if (old > pe[j]) pe[j] = old;                              /* we took the slot: the displaced later key walks on -- or nobody, if it was free */
							pq[j] = pq[j] + 1 < F2_WN ? pq[j] + 1 : F2_WN;
						}
					}
				}
			}
			r2_lds_phase();
			R2W_LAP(2)
			if (C.u.c.win[F2_WN] != ~0ull) *fail = 9;                           /* a walk left the window */
			const u32 qhi = w0 + 2 * up - 1 < 2 * n - 1 ? w0 + 2 * up - 1 : 2 * n - 1;   /* the window's part of the new table: [w0, qhi] */
			for (u32 qa = w0 & ~63u; qa <= qhi; qa += 64) {
				const u32 q = qa + lane, i = q - w0;
				const bool in = q - w0 <= qhi - w0;
				const u64 e = C.u.c.win[in ? i : 0];
				const u32 eh = (u32)(e >> 32);
				const bool put = in && eh + 1u >= 2u;                            /* a key of this window (eh == 0: a prefix chain's, k_r2_dsmall wrote it; ~0: nobody) */
				const bool own = in && eh != 0;
				const u64 k = C.u.c.key[(u32)e & (F2_NA - 1)];
				if (own) D[q] = put ? k : YK_EMPTY;
				if (own && q < n) TG[q] = eh - (put ? 1u : 0u);                   /* (R2_NONE is ~0) */
				r2_used_words(UB, qa, __ballot(put), __ballot(own));
			}
			r2_lds_phase();
			R2W_LAP(3)
		}
		if (tail_run) { const u32 a = s1 + 1; hand_over(a, n - a); break; }
		if (giant) {
			const u32 L = run_len(c0);
			hand_over(c0, L);
			if (L > R2_LMAX || c0 + L >= n) break;                                /* refused by the wave routine (fail), or it was the table's last run */
			s0 = c0 + L;
			if (s0 < B1 - 1) fetch(s0);
			R2W_LAP(4)
			continue;
		}
		R2W_LAP(4)
		s0 = s1;
	}
}

template <int NW, bool PROF, int IL>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu((NW == 6 || NW == 5) && !PROF ? NW : 4)))      /* NW = 6: <= 80 VGPRs, four workgroups per CU = 24 waves; NW = 5: <= 96, 20 waves */
void k_r2_double(const R2Tab *tabs, const R2Act *acts, u64 *K0, u64 *K1, u32 *TAG, const u32 *OCC, u32 *USED, const u32 *Fin, u32 *Fout, u32 *fail, u64 *prof)
{
	u64 pf[PROF ? 8 : 1] = { 0 }, tq = PROF ? wall_clock64() : 0;              /* PROF (YAKAMD_VERBOSE > 1): 100 MHz ticks per phase, lane 0 of every wave */
#define R2F_LAP(i) if (PROF) { const u64 t_ = wall_clock64(); pf[i] += t_ - tq; tq = t_; }
	__shared__ union { R2Chunk ch[NW]; R2Wave big; } U;
	__shared__ u32 s_big[64];
	__shared__ u32 s_G, s_F, s_nbig;
	const u32 p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const R2Act A = acts[p];
	if (A.kind != 2) return;
	const u64 off = tabs[p].off;
	const u32 n = 1u << A.bits, nb = A.bits + 1;
	u64 *S = (A.src ? K1 : K0) + off;
	u64 *D = (A.src ? K0 : K1) + off;
	u32 *TG = TAG + (off >> 1);
	const u32 *OC = OCC + (off >> 4);
	u32 *UB = USED + (off >> 5);
	u32 F = Fin[p];                                                           /* k_r2_dsmall did the prefix and the rounds below small_f */
	if (tid == 0) s_nbig = 0;
	if (wave == 0 && F < n) { const u32 g = r2_boundary_wave(S, F, 2 * F < n ? 2 * F : n, n); if (lane == 0) s_G = g; }
	__syncthreads();
	while (F < n) {
		const u32 G = s_G;
		if (G == 0) {
			/* (uniform) no unused slot in (F, 2F]: one run covers [F, 2F] and feeds its own slots.  It is placed alone, by the literal rule in
			 * sigma order on LDS copies (r2_wave_run<.., true>, as in k_r2_dsmall's rounds), up to its own end */
			__syncthreads();
			if (wave == 0) {
				u32 g = 2 * F;
				for (;;) {                                                         /* first unused slot from 2F on */
					const u32 idx = g + lane;
					const u64 m = __ballot(idx >= n || S[idx] == YK_EMPTY);
					if (m) { g += (u32)__ffsll((long long)m) - 1; break; }
					g += 64;
				}
				const u32 G2 = g < n ? g + 1 : n;
				r2_wave_run<true, true>(U.big, S, D, TG, OC, UB, F, n, nb, fail);
				r2_wave_sync();
				const u32 gn = G2 < n ? r2_boundary_wave(S, G2, 2 * G2 < n ? 2 * G2 : n, n) : n;
				if (lane == 0) { s_F = G2; s_G = gn; }
			}
			__syncthreads();
			F = s_F;
			continue;
		}
		__syncthreads();                                                       /* everybody has read s_G */
		if (wave == 0 && G < n) { const u32 g = r2_boundary_wave(S, G, 2 * G < n ? 2 * G : n, n); if (lane == 0) s_G = g; }   /* used slots stay used: the next boundary can be looked up now */
		r2_round_wave<PROF, (u32)IL>(U.ch[wave], S, D, TG, OC, UB, F, G, n, nb, wave, NW, s_big, &s_nbig, fail, pf, tq);
		R2F_LAP(5)
		__syncthreads();                                                       /* workgroup scope is all it takes: the sub-table never leaves this workgroup (an agent-scope fence here writes the L2 back, once per round and workgroup) */
		R2F_LAP(6)
		if (s_nbig) {                                                          /* (uniform) runs beyond R2_MMAX slots: wave 0, one after the other */
			if (wave == 0) {
				const u32 nbg = s_nbig < 64 ? s_nbig : 64;
				for (u32 j = 0; j < nbg; ++j) { r2_wave_run<true, false>(U.big, S, D, TG, OC, UB, s_big[j], n, nb, fail); r2_wave_sync(); }
				if (lane == 0) s_nbig = 0;
			}
			__syncthreads();
			R2F_LAP(7)
		}
		F = G;
	}
	if (tid == 0) { Fout[p] = F; if (F < n) *fail = 10; }                     /* did not reach the end of the table: the host replays with k_replay */
	if (PROF && lane == 0) { for (int i = 0; i < 8; ++i) atomicAdd((unsigned long long*)&prof[i], (unsigned long long)pf[i]); atomicAdd((unsigned long long*)&prof[8], 1ull); }
}

/* The scatter of the grouping kernels below, write-combined through LDS.  A lone 8-byte store costs a whole memory transaction on this chip (mb_scatter: 21 G
 * records/s), and the plain scatter -- every key and its rank stored where its segment's cursor stood -- was just that: k_r2_ppart took 10.8 ms per 1 G
 * keys of an assembly, nine times what its counting pass over the same keys takes.  Now the keys go through tiles of 4096: counted per segment in LDS, laid
 * out by segment in an LDS copy of the tile, and written from there -- consecutive lanes hold consecutive keys of one segment, so a segment's run of the tile
 * (32 keys with 128 segments) leaves as whole lines.  s_cur: where each segment's keys go next (LDS, [1024]); the caller has filled it */
#define PP_TILE 4096u
struct PpartLds { u32 cur[1024], h[1024], o[1024], w[16]; u64 tk[PP_TILE]; u32 tr[PP_TILE]; };   /* 60 KB: two workgroups per CU */
__device__ __forceinline__ void r2_ppart_tiles(PpartLds &S, const u64 *__restrict__ kc, u32 lo, u32 hi, u32 bits, u32 SEGLOG, u64 *__restrict__ pk, u32 *__restrict__ pr)
{
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	for (u32 t0 = lo; t0 < hi; t0 += PP_TILE) {
		const u32 nt = hi - t0 < PP_TILE ? hi - t0 : PP_TILE;
		S.h[tid] = 0;
		__syncthreads();
		u64 key[4]; u32 sg[4], lr[4];
#pragma unroll
		for (u32 j = 0; j < 4; ++j) { const u32 i = tid + 1024 * j; key[j] = i < nt ? kc[t0 + i] : 0; }
#pragma unroll
		for (u32 j = 0; j < 4; ++j) { const u32 i = tid + 1024 * j; sg[j] = r2_home(key[j], bits) >> SEGLOG; lr[j] = i < nt ? atomicAdd(&S.h[sg[j]], 1u) : 0; }
		__syncthreads();
		const u32 c = S.h[tid];                                              /* exclusive scan over the segments: where a segment's keys lie in the tile */
		u32 incl = c;
		for (int o = 1; o < 64; o <<= 1) { const u32 v = __shfl_up(incl, o); if (lane >= (u32)o) incl += v; }
		if (lane == 63) S.w[wave] = incl;
		__syncthreads();
		u32 ex = incl - c;
		for (u32 w = 0; w < wave; ++w) ex += S.w[w];
		S.o[tid] = ex;
		__syncthreads();
#pragma unroll
		for (u32 j = 0; j < 4; ++j) { const u32 i = tid + 1024 * j; if (i < nt) { const u32 at = S.o[sg[j]] + lr[j]; S.tk[at] = key[j]; S.tr[at] = t0 + i + 1; } }
		__syncthreads();
#pragma unroll
		for (u32 j = 0; j < 4; ++j) {
			const u32 i = tid + 1024 * j;
			if (i < nt) {
				const u64 k = S.tk[i];
				const u32 g = r2_home(k, bits) >> SEGLOG, d = S.cur[g] + (i - S.o[g]);
				pk[d] = k; pr[d] = S.tr[i];
			}
		}
		__syncthreads();
		S.cur[tid] += c;
	}
}

/* keys of a stage grouped by the segment of their home slot: pk/pr[rec_off + i0 + ...], seg_start[seg0 + s] relative to the stage's first key */
__global__ __launch_bounds__(1024)
void k_r2_ppart(const R2Tab *tabs, const R2Act *acts, const u64 *__restrict__ kc, u64 *__restrict__ pk, u32 *__restrict__ pr, u32 *seg_start, u32 SEGLOG)
{
	__shared__ PpartLds S;
	const u32 p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const R2Act A = acts[p];
	if (A.kind != 1 || A.bits <= SEGLOG) return;
	const u32 nseg = 1u << (A.bits - SEGLOG);                    /* <= 1024 */
	const u64 base = tabs[p].rec_off + A.i0;
	S.h[tid] = 0;
	__syncthreads();
	for (u32 q = tid; q < A.batch; q += 1024) atomicAdd(&S.h[r2_home(kc[base + q], A.bits) >> SEGLOG], 1u);
	__syncthreads();
	const u32 c = S.h[tid];
	u32 incl = c;
	for (int o = 1; o < 64; o <<= 1) { const u32 t = __shfl_up(incl, o); if (lane >= (u32)o) incl += t; }
	if (lane == 63) S.w[wave] = incl;
	__syncthreads();
	u32 ex = incl - c;
	for (u32 w = 0; w < wave; ++w) ex += S.w[w];
	if (tid < nseg) seg_start[A.seg0 + tid] = ex;
	if (tid == nseg - 1) seg_start[A.seg0 + nseg] = ex + c;
	S.cur[tid] = ex;
	__syncthreads();
	r2_ppart_tiles(S, kc + base, 0, A.batch, A.bits, SEGLOG, pk + base, pr + base);
}

/* the same grouping by G workgroups per sub-table, for the steps in which few sub-tables place (a shard of a multi-GPU job owns 128 of them: one workgroup each
 * left half of the CUs idle, 17 ms per job): count per share of the batch, scan per sub-table, scatter per share.  cnt: [P][G][1024] */
__global__ __launch_bounds__(1024)
void k_r2_ppart_cnt(const R2Tab *tabs, const R2Act *acts, const u64 *__restrict__ kc, u32 *cnt, u32 SEGLOG)
{
	__shared__ u32 s_cnt[1024];
	const u32 g = blockIdx.x, G = gridDim.x, p = blockIdx.y, tid = threadIdx.x;
	const R2Act A = acts[p];
	if (A.kind != 1 || A.bits <= SEGLOG) return;
	const u64 base = tabs[p].rec_off + A.i0;
	const u32 len = ((A.batch + G - 1) / G + 1023) & ~1023u, lo = g * len, hi = lo + len < A.batch ? lo + len : A.batch;
	s_cnt[tid] = 0;
	__syncthreads();
	for (u32 q = lo + tid; q < hi; q += 1024) atomicAdd(&s_cnt[r2_home(kc[base + q], A.bits) >> SEGLOG], 1u);
	__syncthreads();
	cnt[((size_t)p * G + g) * 1024 + tid] = s_cnt[tid];
}

__global__ __launch_bounds__(1024)
void k_r2_ppart_scan(const R2Act *acts, u32 *cnt, u32 *seg_start, u32 SEGLOG, u32 G)
{
	__shared__ u32 s_w[16];
	const u32 p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const R2Act A = acts[p];
	if (A.kind != 1 || A.bits <= SEGLOG) return;
	const u32 nseg = 1u << (A.bits - SEGLOG);
	u32 c = 0;
	for (u32 g = 0; g < G; ++g) c += cnt[((size_t)p * G + g) * 1024 + tid];
	u32 incl = c;
	for (int o = 1; o < 64; o <<= 1) { const u32 t = __shfl_up(incl, o); if (lane >= (u32)o) incl += t; }
	if (lane == 63) s_w[wave] = incl;
	__syncthreads();
	u32 ex = incl - c;
	for (u32 w = 0; w < wave; ++w) ex += s_w[w];
	if (tid < nseg) seg_start[A.seg0 + tid] = ex;
	if (tid == nseg - 1) seg_start[A.seg0 + nseg] = ex + c;
	for (u32 g = 0; g < G; ++g) { u32 *e = &cnt[((size_t)p * G + g) * 1024 + tid]; const u32 v = *e; *e = ex; ex += v; }   /* where share g's keys of this segment start */
}

__global__ __launch_bounds__(1024)
void k_r2_ppart_scat(const R2Tab *tabs, const R2Act *acts, const u64 *__restrict__ kc, u64 *__restrict__ pk, u32 *__restrict__ pr, const u32 *cnt, u32 SEGLOG)
{
	__shared__ PpartLds S;
	const u32 g = blockIdx.x, G = gridDim.x, p = blockIdx.y, tid = threadIdx.x;
	const R2Act A = acts[p];
	if (A.kind != 1 || A.bits <= SEGLOG) return;
	const u64 base = tabs[p].rec_off + A.i0;
	const u32 len = ((A.batch + G - 1) / G + 1023) & ~1023u, lo = g * len, hi = lo + len < A.batch ? lo + len : A.batch;
	S.cur[tid] = cnt[((size_t)p * G + g) * 1024 + tid];
	__syncthreads();
	if (lo < hi) r2_ppart_tiles(S, kc + base, lo, hi, A.bits, SEGLOG, pk + base, pr + base);
}

/* ordered probing of one segment's keys with the ranks in LDS */
__global__ __launch_bounds__(1024)
void k_r2_place(const R2Tab *tabs, const R2Act *acts, u64 *K0, u64 *K1, const u64 *__restrict__ kc, const u64 *__restrict__ pk, const u32 *__restrict__ pr,
                const u32 *__restrict__ seg_start, u32 *head, u64 *spill, u32 *spill_n, u32 spill_cap, u32 *fail, u32 SEGLOG, u32 HEAD, u32 *img_u, u32 p0, const u32 *__restrict__ USED)
{
	extern __shared__ __attribute__((aligned(16))) u32 s_own[];
	/* the segments of ONE sub-table on ONE XCD (the dispatcher deals workgroup b to XCD b % 8; each XCD has an L2 of its own): they all gather their
	 * keys from the same sorted batch of the stage, a few MB that then come from that L2 instead of being fetched by all eight (counters, 1 Gb
	 * assembly: 122 GB fetched by this kernel before).  The grid covers the sub-tables [p0, p0 + gridDim.y) that place in this step, not all P: a shard
	 * owns a contiguous range of them, and dealt over all P its 128 or 512 sub-tables landed on one or four of the eight XCDs (a cfg3 rank's k_r2_place:
	 * 11.2 ms per launch for a quarter of the work a 5 Gb sweep does in 10.7) */
	const u32 bid = blockIdx.x + blockIdx.y * gridDim.x, nwg = gridDim.x * gridDim.y;
	const u32 tile = (nwg & 7) == 0 ? (bid & 7) * (nwg >> 3) + (bid >> 3) : bid;
	const u32 p = p0 + tile / gridDim.x, seg = tile % gridDim.x, tid = threadIdx.x;
	const R2Act A = acts[p];
	if (A.kind != 1) return;
	const u32 n = 1u << A.bits, nseg = A.bits > SEGLOG ? 1u << (A.bits - SEGLOG) : 1;
	if (seg >= nseg) return;
	const u32 L = nseg > 1 ? 1u << SEGLOG : n, start = seg * L;
	u64 *keys = (A.src ? K1 : K0) + tabs[p].off;
	const u64 base = tabs[p].rec_off + A.i0;
	{
		/* which slots are taken: one bit per slot, left by the step before (k_r2_load, or the doubling's write-back: k_r2_double) -- 2 KB per segment
		 * instead of the segment's 128 KB of the table (1 Gb assembly: 32 GB of the 94 this kernel moved) */
		const u32 *ub = USED + ((tabs[p].off + start) >> 5);
		/* (a lane's words are requested eight at a time: one after the other each waited for the one before) */
		for (u32 i0 = 0; i0 < L; i0 += 8 * blockDim.x) {
			u32 w[8];
#pragma unroll
			for (u32 t = 0; t < 8; ++t) { const u32 i = i0 + t * blockDim.x + tid; w[t] = i < L ? ub[i >> 5] : 0; }
#pragma unroll
			for (u32 t = 0; t < 8; ++t) { const u32 i = i0 + t * blockDim.x + tid; if (i < L) s_own[i] = (w[t] >> (i & 31) & 1) ? 0u : 0xffffffffu; }
		}
	}
	__syncthreads();
	const u32 q0 = nseg > 1 ? seg_start[A.seg0 + seg] : 0, q1 = nseg > 1 ? seg_start[A.seg0 + seg + 1] : A.batch;
	if (nseg == 1) {
		for (u32 q = q0 + tid; q < q1; q += blockDim.x) {                   /* a table of one segment: the walk wraps around */
			u32 r = q + 1, li = r2_home(kc[base + q], A.bits);
			for (;;) {
				const u32 old = atomicMin(&s_own[li], r);
				if (old == 0xffffffffu) break;
				if (old > r) r = old;                                      /* we took the slot; carry the displaced later key on */
				li = (li + 1) & (n - 1);
			}
		}
	} else {
		/* The walks are what this kernel issues (SQ counters: ~1000 VALU + 1700 SALU wave-instructions per wave, two thirds of them the loop below in its
		 * old form: a lane's ~6 keys one after the other, every batch of 64 walks running until its LONGEST one ended -- ~25 steps for a mean of 3.7).
		 * Now a lane whose key has its slot takes the next key of its WAVE at once: the wave's keys come 64 at a time through a staging area in LDS
		 * (requested a batch ahead), idle lanes pop from it by ballot + prefix count.  The loop runs ~(atomics of the wave) / 64 steps plus one tail */
		u32 *st_r = s_own + L + (tid >> 6) * 128, *st_l = st_r + 64;        /* this wave's staging area: ranks, home slots */
		const u32 lane = tid & 63, wq0 = q0 + (tid & ~63u);                   /* the wave's batches: keys wq0 + 1024 k + lane */
		const u64 lt = lane ? ~0ull >> (64 - lane) : 0ull;
		u32 rn = 0xffffffffu, ln = 0;
		u32 kb = 0;                                                           /* (uniform) batches requested so far */
		auto request = [&]() {
			const u32 q = wq0 + kb * blockDim.x + lane;
			const bool in = q < q1;
			rn = in ? pr[base + q] : 0xffffffffu;
			ln = r2_home(pk[base + (in ? q : q0)], A.bits) - start;
			++kb;
		};
		if (wq0 < q1) request();
		u32 staged = 0, spos = 0;                                             /* (uniform) keys in the staging area, keys popped */
		bool more = wq0 < q1;                                                 /* (uniform) a requested batch waits in rn / ln */
		u32 r = 0xffffffffu, li = 0;
		for (;;) {
			const u64 idle = __ballot(r == 0xffffffffu);
			if (idle) {
				if (spos == staged && more) {                                   /* staging area drained: the requested batch goes in, the next one is requested */
					st_r[lane] = rn; st_l[lane] = ln;
					const u32 left = q1 - (wq0 + (kb - 1) * blockDim.x);
					staged = left < 64 ? left : 64; spos = 0;
					more = wq0 + kb * blockDim.x < q1;
					if (more) request();
					r2_lds_phase();
				}
				if (spos < staged) {
					const u32 at = spos + (u32)__popcll(idle & lt);
					if (r == 0xffffffffu && at < staged) { r = st_r[at]; li = st_l[at]; }
					const u32 nid = (u32)__popcll(idle);
					spos = spos + nid < staged ? spos + nid : staged;
				}
			}
			if (!__ballot(r != 0xffffffffu)) { if (spos == staged && !more) break; continue; }
			if (r != 0xffffffffu) {
				const u32 old = atomicMin(&s_own[li], r);
				r = old > r ? old : r;                                          /* we took the slot: the displaced later key walks on -- or nobody (~0), if it was free */
				++li;
				if (li == L && r != 0xffffffffu) {                                /* (rare) the walk goes on in the next segment's head */
					const u32 at = atomicAdd(spill_n, 1u);
					if (at < spill_cap) spill[at] = (u64)p << 48 | (u64)((seg + 1) & (nseg - 1)) << 32 | r; else *fail = 4;
					r = 0xffffffffu;
				}
			}
		}
	}
	__syncthreads();
	const u64 *src = kc + base;
	const u32 h0 = nseg > 1 ? HEAD : 0;
	u32 *hd = head + (size_t)(A.seg0 + seg) * HEAD;
	/* A.pad0: this is the sub-table's last step and its buffer becomes the table image -- the "used" bits of the segment go out with the keys (one
	 * slot per lane: a wave's ballot is two bitmap words), so that no pass over the finished table is needed for them */
	u32 *ub = (A.pad0 && img_u) ? img_u + ((tabs[p].off + start) >> 5) : 0;
	for (u32 i0 = 0; i0 < L; i0 += blockDim.x) {
		const u32 i = i0 + tid;
		const bool in = i < L;
		const u32 o = in ? s_own[i] : 0xffffffffu;
		if (in) {
			if (i < h0) hd[i] = o;                                      /* finished by k_r2_spill / k_r2_headfill */
			else if (o != 0 && o != 0xffffffffu) keys[start + i] = src[o - 1];
		}
		if (ub) {
			const u64 b = __ballot(in && o != 0xffffffffu);
			if ((tid & 63) == 0 && in && i >= h0) { ub[i >> 5] = (u32)b; if (i + 32 < L) ub[(i >> 5) + 1] = (u32)(b >> 32); }
		}
	}
}

__global__ __launch_bounds__(256)
void k_r2_spill(const R2Act *acts, const u64 *spill, const u32 *spill_n, u32 spill_cap, u32 *head, u32 *fail, u32 HEAD)
{
	const u32 ns = *spill_n < spill_cap ? *spill_n : spill_cap;
	for (u32 j = blockIdx.x * 256 + threadIdx.x; j < ns; j += gridDim.x * 256) {
		const u64 e = spill[j];
		const u32 p = (u32)(e >> 48), seg = (u32)(e >> 32) & 0xffffu;
		u32 r = (u32)e;
		u32 *hd = head + (size_t)(acts[p].seg0 + seg) * HEAD;
		u32 li = 0;
		for (;;) {
			const u32 old = atomicMin(&hd[li], r);
			if (old == 0xffffffffu) break;
			if (old > r) r = old;
			if (++li == HEAD) { *fail = 5; break; }
		}
	}
}

__global__ __launch_bounds__(256)
void k_r2_headfill(const R2Tab *tabs, const R2Act *acts, u64 *K0, u64 *K1, const u64 *__restrict__ kc, const u32 *head, u32 SEGLOG, u32 HEAD, u32 *img_u, u32 p0)
{
	const u32 bid = blockIdx.x + blockIdx.y * gridDim.x, nwg = gridDim.x * gridDim.y;
	const u32 tile = (nwg & 7) == 0 ? (bid & 7) * (nwg >> 3) + (bid >> 3) : bid;       /* as k_r2_place: a sub-table's segments on one XCD, the grid over the sub-tables that place */
	const u32 p = p0 + tile / gridDim.x, seg = tile % gridDim.x;
	const R2Act A = acts[p];
	if (A.kind != 1 || A.bits <= SEGLOG || seg >= 1u << (A.bits - SEGLOG)) return;
	u64 *keys = (A.src ? K1 : K0) + tabs[p].off + ((u64)seg << SEGLOG);
	const u64 *src = kc + tabs[p].rec_off + A.i0;
	const u32 *hd = head + (size_t)(A.seg0 + seg) * HEAD;
	u32 *ub = (A.pad0 && img_u) ? img_u + ((tabs[p].off + ((u64)seg << SEGLOG)) >> 5) : 0;   /* (as in k_r2_place: the head's "used" bits) */
	for (u32 i0 = 0; i0 < HEAD; i0 += 256) {
		const u32 i = i0 + threadIdx.x;
		const bool in = i < HEAD;
		const u32 o = in ? __hip_atomic_load(&hd[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xffffffffu;
		if (in && o != 0 && o != 0xffffffffu) keys[i] = src[o - 1];
		if (ub) {
			const u64 b = __ballot(in && o != 0xffffffffu);
			if ((threadIdx.x & 63) == 0 && in) { ub[i >> 5] = (u32)b; if (i + 32 < HEAD) ub[(i >> 5) + 1] = (u32)(b >> 32); }
		}
	}
}

/* table of a sub-table into one of the two buffers: a copy of `n` slots of src (unused slots hold YK_EMPTY) or an empty table; its occupancy bitmap
 * for a placement that comes first (one lane per slot; a wave's ballot is two bitmap words) */
__global__ __launch_bounds__(256)
void k_r2_load(const R2Tab *tabs, const R2Load *ld, const u64 *__restrict__ src1, const u64 *__restrict__ src2, u64 *K0, u64 *K1, u32 *USED)
{
	const R2Load Ld = ld[blockIdx.y];
	if (Ld.bits == YK_NOCAP) return;
	u64 *D = (Ld.dst ? K1 : K0) + tabs[blockIdx.y].off;
	u32 *UB = USED + (tabs[blockIdx.y].off >> 5);
	const u64 *src = Ld.from_src == 2 ? src2 : src1;
	const u64 n = 1ull << Ld.bits;
	for (u64 i0 = (u64)blockIdx.x * 256; i0 < n; i0 += (u64)gridDim.x * 256) {
		const u64 i = i0 + threadIdx.x;
		const u64 k = (i < n && Ld.from_src) ? src[Ld.src_off + i] : YK_EMPTY;
		if (i < n) D[i] = k;
		const u64 b = __ballot(k != YK_EMPTY);
		if ((threadIdx.x & 63) == 0 && i < n) { UB[i >> 5] = (u32)b; if (i + 32 < n) UB[(i >> 5) + 1] = (u32)(b >> 32); }
	}
}

/* does a put-call follow the last new key of the sub-table (khashl.h:202 on an existing key: the trailing doubling)? */
__global__ void k_r2_trail(const u64 *lastput, const u64 *rec_t, const u64 *rec_off, const u32 *m, int P, u32 *out)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= P) return;
	const u64 lp = lastput[p];
	out[p] = lp != 0 && (m[p] == 0 || lp - 1 > rec_t[rec_off[p] + m[p] - 1]);
}

/* final table -> arena + bitmap (one lane per slot; a wave's ballot is two bitmap words) */
__global__ __launch_bounds__(256)
void k_r2_publish(const R2Tab *tabs, const R2Pub *pub, const u64 *K0, const u64 *K1, u64 *__restrict__ nk, u32 *__restrict__ nu)
{
	const R2Pub Pb = pub[blockIdx.y];
	if (Pb.bits == YK_NOCAP) return;
	const u64 *S = (Pb.src ? K1 : K0) + tabs[blockIdx.y].off;
	const u64 n = 1ull << Pb.bits;
	for (u64 i0 = (u64)blockIdx.x * 256; i0 < n; i0 += (u64)gridDim.x * 256) {
		const u64 i = i0 + threadIdx.x;
		const u64 k = i < n ? S[i] : YK_EMPTY;
		if (i < n && S != nk + Pb.new_off) nk[Pb.new_off + i] = k;       /* (the buffer that becomes the image: its own tables only get their bitmap) */
		const u64 b = __ballot(k != YK_EMPTY);
		if ((threadIdx.x & 63) == 0 && i < n) { nu[(Pb.new_off + i) >> 5] = (u32)b; if (i + 32 < n) nu[((Pb.new_off + i) >> 5) + 1] = (u32)(b >> 32); }
	}
}

/* ------------------------------------------------------------------------------------------
 * shrink (reference htab.c:180-197): keys with min <= count <= max, in ascending OLD slot order
 * ------------------------------------------------------------------------------------------ */
/* which == 0: count range only (yak_ch_shrink); 1: and absent from `other` (yak_ch_subtract,
 * htab.c:287-316); 2: and present in `other` (yak_ch_isec, htab.c:318-347) */
__device__ __forceinline__ bool shrink_keep(const ImgView &img, u64 a, int cmin, int cmax, int which, const ImgView &other, u32 p)
{
	if (!(img.used[a >> 5] >> (a & 31) & 1)) return false;
	const u64 kc = img.keys[a];
	const int c = (int)(kc & 1023);
	if (c < cmin || c > cmax) return false;
	if (which == 0) return true;
	const bool present = img_find(other, (kc >> 10) << img.pre | p) >= 0;
	return which == 1 ? !present : present;
}

/* A sub-table is walked by gridDim.y workgroups, each over its share of the slots (one workgroup walked 128 Ki slots of a filtered count alone, two
 * barriers per 256 slots: 1.4 ms for the two kernels).  rng_cnt[p * gridDim.y + g] = keys kept in share g; the scatter starts a share behind the
 * shares before it.  A table of fewer than 256 slots per share is share 0's alone */
#define SHR_RG 8
__device__ __forceinline__ void shrink_share(u32 bits, u32 *lo, u32 *hi)
{
	const u32 cap = 1u << bits, per = cap / gridDim.y;
	if (per < 256u) { *lo = 0; *hi = blockIdx.y == 0 ? cap : 0; }
	else { *lo = per * blockIdx.y; *hi = *lo + per; }
}
__global__ __launch_bounds__(256)
void k_shrink_count(ImgView img, int cmin, int cmax, int which, ImgView other, u32 *seg_cnt)
{
	__shared__ u32 s_tot;
	const u32 bits = img.bits[blockIdx.x];
	if (threadIdx.x == 0) s_tot = 0;
	__syncthreads();
	if (bits != YK_NOCAP) {
		const u64 off = img.off[blockIdx.x];
		u32 c = 0, lo, hi;
		shrink_share(bits, &lo, &hi);
		for (u32 i = lo + threadIdx.x; i < hi; i += 256) c += shrink_keep(img, off + i, cmin, cmax, which, other, blockIdx.x);
		for (int o = 32; o; o >>= 1) c += __shfl_down(c, o);
		if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_tot, c);
	}
	__syncthreads();
	if (threadIdx.x == 0) seg_cnt[blockIdx.x * gridDim.y + blockIdx.y] = s_tot;
}

__global__ __launch_bounds__(256)
void k_shrink_scatter(ImgView img, int cmin, int cmax, int which, ImgView other, const u64 *seg_off, u64 *rec_kc, const u32 *rng_cnt)
{
	__shared__ u32 s_w[4];
	const u32 bits = img.bits[blockIdx.x];
	if (bits == YK_NOCAP) return;
	const u64 off = img.off[blockIdx.x];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	u64 out = seg_off[blockIdx.x];
	if (out == ~0ull) return;                                        /* not asked for (a dump of some sub-tables only) */
	for (u32 g = 0; g < blockIdx.y; ++g) out += rng_cnt[blockIdx.x * gridDim.y + g];
	u32 lo, hi;
	shrink_share(bits, &lo, &hi);
	for (u32 base = lo; base < hi; base += 256) {
		const u32 i = base + threadIdx.x;
		const bool keep = i < hi && shrink_keep(img, off + i, cmin, cmax, which, other, blockIdx.x);
		const u64 b = __ballot(keep);
		if (lane == 0) s_w[wave] = __popcll(b);
		__syncthreads();
		u32 pre = 0, tot = 0;
		for (int w = 0; w < 4; ++w) { if (w < wave) pre += s_w[w]; tot += s_w[w]; }
		if (keep) rec_kc[out + pre + __popcll(b & lanemask_lt())] = img.keys[off + i];
		out += tot;
		__syncthreads();
	}
}

/* out[pos[i]] = val[i]: the capacity / size words of a .yak image between its key lists */
__global__ __launch_bounds__(256)
void k_put_u64(const u64 *pos, const u64 *val, u32 n, u64 *out)
{
	const u32 i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) out[pos[i]] = val[i];
}


