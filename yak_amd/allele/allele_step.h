/* allele_step.h -- the per-thread steps of the read support of the bubbles' alleles (`yak-amd bubbles -r`; include/yak_amd_allele.h; DESIGN.md
 * section 31).  No HIP in here, as in ../bubble/bubble_step.h: AL_FN is `__host__ __device__` under hipcc and empty otherwise, so that the kernels
 * of allele.hip and the sequential model of tools/allele_model_check.cpp (host compiler, sanitizers) call the very same functions.
 *
 * arm_of[j] = i << 1 | a for the unitig of arm a of bubble i, AL_NONE for every other unitig.  The paths of a chunk tile its steps: path p holds
 * steps[step_off_p .. step_off_p + n_step_p), step_off_0 = 0 and step_off_{p + 1} = step_off_p + n_step_p.  Every index that comes from the caller's
 * device data -- the unitig of an arm, the unitig of a step, the range of a path -- is checked against its bound before it is used; what does not
 * fit is counted in *bad and decides nothing. */
#ifndef YK_ALLELE_STEP_H
#define YK_ALLELE_STEP_H
#include <stdint.h>
#include "../bubble/bubble_step.h"

#define AL_FN BB_FN
#define AL_NONE (~(uint32_t)0)               /* arm_of[j] of a unitig that is no arm */
enum { AL_A = 1, AL_FULL = 2, AL_REV = 4 };  /* the bits of yakamd_aobs_t.flags */

typedef struct alignas(16) { uint64_t step_off, ps; uint32_t seq, n_step, qs, qe; } al_path_t;      /* yakamd_upath_t, include/yak_amd_path.h */
typedef struct alignas(16) { uint32_t seq, bubble, flags, path; } al_obs_t;                         /* yakamd_aobs_t, include/yak_amd_allele.h */
typedef struct alignas(16) { uint64_t full[2], part[2]; } al_sup_t;                                 /* yakamd_asup_t */

/* ---- step 1, arm a (oriented unitig `arm`) of bubble record i claims its unitig.  cas32(p, expected, desired) returns what *p held.  0: it
 * holds it now; AL_BAD_ARM: its unitig is none of the n_unitig, nothing is claimed; AL_DUP_ARM: another arm holds the unitig already ---- */
enum { AL_BAD_ARM = 1, AL_DUP_ARM = 2 };
template <class Cas32> AL_FN int al_claim(uint64_t arm, uint64_t i, unsigned a, uint64_t n_unitig, uint32_t *arm_of, Cas32 cas32)
{
	const uint64_t j = arm >> 1;
	if (j >= n_unitig) return AL_BAD_ARM;
	return cas32(arm_of + j, AL_NONE, (uint32_t)(i << 1 | (uint64_t)a)) != AL_NONE ? AL_DUP_ARM : 0;
}

/* ---- step 2: the last path of paths[lo .. hi] whose step_off is at most t; lo <= hi < n_path.  For lists that do not fit (no order) some path in
 * [lo, hi], which al_find() then refuses ---- */
AL_FN uint64_t al_path_of(const al_path_t *paths, uint64_t lo, uint64_t hi, uint64_t t)
{
	while (lo < hi) {
		const uint64_t mid = lo + ((hi - lo + 1) >> 1);
		if (paths[mid].step_off <= t) lo = mid; else hi = mid - 1;
	}
	return lo;
}

/* step t < n_step of the chunk, whose path lies in paths[lo .. hi]: 0 when it is no observation, else 1 and *obs.  The path's range is checked
 * against n_step and against the path before it, the step's unitig against n_unitig; a misfit is counted in *bad and is no observation.  arm_of[]
 * and rec[] are the library's own: arm_of[j] < 2 n_bubble or AL_NONE */
AL_FN int al_find(const al_path_t *paths, uint64_t lo, uint64_t hi, const uint64_t *steps, uint64_t n_step, uint64_t t, uint64_t n_unitig,
                  const uint32_t *arm_of, const bb_rec_t *rec, al_obs_t *obs, uint64_t *bad)
{
	const uint64_t p = al_path_of(paths, lo, hi, t);
	const al_path_t q = paths[p];
	const uint64_t front = p ? paths[p - 1].step_off + (uint64_t)paths[p - 1].n_step : 0;
	if (q.step_off != front || q.step_off > t || q.n_step > n_step - q.step_off || t - q.step_off >= (uint64_t)q.n_step) { ++*bad; return 0; }
	const uint64_t s = steps[t], j = s >> 1;
	if (j >= n_unitig) { ++*bad; return 0; }
	const uint32_t m = arm_of[j];
	if (m == AL_NONE) return 0;
	const uint32_t i = m >> 1, a = m & 1u;
	const uint32_t full = t != q.step_off && t != q.step_off + (uint64_t)q.n_step - 1;
	const uint32_t rev = (uint32_t)((s ^ rec[i].arm[a]) & 1);
	obs->seq = q.seq; obs->bubble = i; obs->flags = a | full << 1 | rev << 2; obs->path = (uint32_t)p;
	return 1;
}

/* ---- the call of a bubble from its support: 0 het, 1 hom1, 2 hom2, 3 none ---- */
AL_FN int al_call(const al_sup_t *s, uint64_t min_sup)
{
	const int one = s->full[0] >= min_sup, two = s->full[1] >= min_sup;
	return one && two ? 0 : one ? 1 : two ? 2 : 3;
}
#endif
