/* correct_step.h -- the per-thread steps of the correction of substitution errors (`yak-amd correct`; include/yak_amd_correct.h; DESIGN.md section
 * 30).  No HIP in here: CR_FN is `__host__ __device__` under hipcc and empty otherwise, so that the kernels of correct.hip and the sequential model
 * of tools/correct_model_check.cpp (host compiler, sanitizers) call the very same functions.
 *
 * An array is read through a functor `at(i)` that answers for every i: the kernels give it a tile in LDS, the model the whole array.  Every index
 * that comes from device data -- the place of a record in the image, its run, its sequence -- is checked against its bound before it is used
 * (cr_rec_ok); what does not fit is counted and decides nothing. */
#ifndef YK_CORRECT_STEP_H
#define YK_CORRECT_STEP_H
#include <stdint.h>

#if defined(__HIPCC__)
#define CR_FN __host__ __device__ static inline
#else
#define CR_FN static inline
#endif

#define CR_NONE 0xffffu                                            /* no k-mer ends here */
enum { CR_NOFIT = 0, CR_DONE = 1, CR_AMBIG = 2 };                  /* YAKAMD_FIX_*, include/yak_amd_correct.h */
typedef struct alignas(16) { uint64_t at; uint32_t seq, p, st, en; uint8_t from, to, fit, why; uint32_t reserved; } cr_fix_t;      /* yakamd_fix_t */
typedef struct alignas(16) { uint32_t n_kmer, n_weak, n_cand, n_fixed, n_ambig, n_nofit, n_weak_after, reserved; } cr_tally_t;     /* yakamd_ctally_t */

/* seq_nt4_table (reference misc.c:4-21) without the table: ACGT, acgt, U, u and the bytes 0 .. 3 are bases, everything else is 4 */
CR_FN int cr_nt4(uint8_t b)
{
	if (b < 4) return b;
	switch (b | 0x20) {
	case 'a': return 0;
	case 'c': return 1;
	case 'g': return 2;
	case 't': case 'u': return 3;
	default: return 4;
	}
}

CR_FN int cr_exists(uint32_t v) { return v != CR_NONE; }
CR_FN int cr_weak(uint32_t v, uint32_t c) { return v != CR_NONE && v < c; }

/* the sequence that holds image byte g among [lo, hi) of the ascending, disjoint sequences: the last one that starts at or in front of g, if g lies
 * inside it; -1: none */
CR_FN int64_t cr_seq_of(const uint64_t *off, const uint32_t *len, int64_t lo, int64_t hi, uint64_t g)
{
	while (lo < hi) {                                              /* the first j in [lo, hi) with off[j] > g */
		const int64_t mid = lo + (hi - lo) / 2;
		if (off[mid] <= g) lo = mid + 1; else hi = mid;
	}
	const int64_t j = lo - 1;
	return j >= 0 && g - off[j] < len[j] ? j : -1;
}
/* the number of sequences among [0, n) that start at or in front of g */
CR_FN int64_t cr_seq_upto(const uint64_t *off, int64_t n, uint64_t g)
{
	int64_t lo = 0, hi = n;
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (off[mid] <= g) lo = mid + 1; else hi = mid;
	}
	return lo;
}

/* the same when the first `from` sequences are known to start at or in front of g: a galloping search from there, a few reads when the answer is
 * near -- the next tile's bound from the one before */
CR_FN int64_t cr_seq_upto_from(const uint64_t *off, int64_t n, int64_t from, uint64_t g)
{
	int64_t lo = from, hi = n, step = 1;
	while (lo < n) {
		const int64_t probe = lo + step - 1 < n - 1 ? lo + step - 1 : n - 1;
		if (off[probe] > g) { hi = probe; break; }
		lo = probe + 1; step <<= 1;
	}
	while (lo < hi) {                                              /* the first j in [lo, hi) with off[j] > g; off[hi] > g or hi == n */
		const int64_t mid = lo + (hi - lo) / 2;
		if (off[mid] <= g) lo = mid + 1; else hi = mid;
	}
	return lo;
}

/* Position i of the count array starts a run (it is weak, i - 1 is not): its end, and whether it is a candidate.  `rel` is i relative to its
 * sequence.  At most k entries ahead of i are read.  Returns 1 with *en_rel and *p_rel (relative as well) for a candidate, 0 for a run that is
 * none; *run_len is min(en - st, k + 1) either way */
template <class At>
CR_FN int cr_run(const At &at, int64_t i, uint32_t rel, int k, uint32_t c, int min_run, uint32_t *en_rel, uint32_t *p_rel, int *run_len)
{
	int n = 1;
	while (n <= k && cr_weak(at(i + n), c)) ++n;                   /* n = k + 1: positions i .. i + k are all weak, the run is longer than k */
	*run_len = n;
	if (n > k || n < min_run) return 0;
	const int front = cr_exists(at(i - 1)), back = cr_exists(at(i + n));
	*en_rel = rel + (uint32_t)n;
	if (n == k) { *p_rel = rel; return 1; }
	if (!front && back) {
		if (rel + (uint32_t)n < (uint32_t)k) return 0;             /* en - k in front of the sequence: no lookup wrote this array */
		*p_rel = rel + (uint32_t)n - (uint32_t)k;
		return 1;
	}
	if (front && !back) { *p_rel = rel; return 1; }
	return 0;
}

/* a record as the trials and the decisions may use it: a run of 1 .. k positions with its base at one of the two places the definition allows,
 * the window of its trials inside the image of n_bytes, its sequence among n_seq (n_seq < 0: not asked) */
CR_FN int cr_rec_ok(const cr_fix_t *r, int k, uint64_t n_bytes, int64_t n_seq)
{
	if (r->en <= r->st || r->en - r->st > (uint32_t)k) return 0;
	if (r->p != r->st && (uint64_t)r->p + (uint32_t)k != r->en) return 0;
	if (r->at >= n_bytes || r->at < r->p) return 0;
	const uint64_t off = r->at - r->p;                             /* where the sequence starts */
	if (off + r->st + 1 < (uint64_t)k || off + r->en > n_bytes) return 0;      /* the window [off + st - k + 1, off + en) */
	if (n_seq >= 0 && (int64_t)r->seq >= n_seq) return 0;
	return 1;
}

/* the rank a = 0, 1, 2 of a trial among the three codes that are not o, and the code of a rank */
CR_FN int cr_trial_code(int o, int a) { return a < o ? a : a + 1; }

/* byte j in [0, 6k) of the three trial windows of record r: window a = j / 2k, its byte q = j % 2k.  `base(g)` is image byte g */
template <class Base>
CR_FN uint8_t cr_trial_byte(const Base &base, const cr_fix_t *r, int k, int o, int j)
{
	const int a = j / (2 * k), q = j % (2 * k);
	const uint64_t g0 = r->at - r->p + r->st + 1 - (uint64_t)k;    /* cr_rec_ok: not below 0 */
	const int w = (int)(r->en - r->st) + k - 1;                    /* the window's bytes, at most 2k - 1 */
	if (q >= w) return (uint8_t)'\n';
	if (g0 + (uint64_t)q == r->at) return (uint8_t)"ACGT"[cr_trial_code(o, a)];
	return base(g0 + (uint64_t)q);
}

/* does entry e in [0, en - st) of trial a of candidate i keep the trial alive: the count of the trial image at the k-mer ending at original
 * position st + e */
CR_FN uint64_t cr_trial_entry(uint64_t i, int a, int k, int e) { return (3 * i + (uint64_t)a) * 2 * (uint64_t)k + (uint64_t)(k - 1 + e); }

/* the decision from the three trials: fit has bit b set iff the trial of code b fits.  *to = the byte to write for CR_DONE, else 0 */
CR_FN int cr_decide(int fit, uint8_t from, uint8_t *to)
{
	const int n = (fit & 1) + (fit >> 1 & 1) + (fit >> 2 & 1) + (fit >> 3 & 1);
	*to = 0;
	if (n == 0) return CR_NOFIT;
	if (n > 1) return CR_AMBIG;
	const int b = fit & 1 ? 0 : fit & 2 ? 1 : fit & 4 ? 2 : 3;
	*to = (uint8_t)("ACGT"[b] | (from & 0x20));
	return CR_DONE;
}
#endif
