/* tally.h -- which kernel instances were launched and which host-side decisions were taken, for the tests (tests/paths_util.py).
 *
 * Every kernel launch of the library goes through YK_LAUNCH: one relaxed increment of the counter of that instantiation, then the launch itself,
 * unchanged.  The name of a counter is the instantiation as the launch site writes it, without blanks or the outer parentheses
 * (`k_part2_wc8<false,7>`); two sites that launch the same instantiation share one counter.  The names are registered while the library is
 * loaded -- a kernel that never ran is listed with a count of zero -- so reading them needs no device.
 *
 * The path events (YKE_*) count decisions that are not launches, each where the host learns of it anyway: no device read and no
 * synchronisation is added for them.  Exports: yakamd_tally_names / yakamd_tally_read / yakamd_tally_reset (include/yak_amd.h) */
#ifndef YK_TALLY_H
#define YK_TALLY_H
#include <stdint.h>

enum YkEvent {
	YKE_RANK_REFUSED,        /* slice_sort: the bitmap ranking was refused (or could not be configured), the stable radix passes sort instead */
	YKE_R2_USED,             /* layout.cpp: a replay done by the streaming kernels */
	YKE_R2_REFUSED,          /* ... handed back to k_replay */
	YKE_PAR_OK,              /* yk_par_counters: sub-tables the parallel doubling did / sent back, as of the last yakamd_debug_counters call */
	YKE_PAR_FAIL,
	YKE_LC2_PASSED_ON,       /* slice_count: sub-buckets k_lc2 passed on to the tier behind it (all of the shard's when k_lc2 does not run) */
	YKE_OVF_GROUPS,          /* slice_count: groups the overflow scratch was cut into (launches of k_lds_count_ovf) */
	YKE_OVF_MORE_GROUPS,     /* ... of them, the groups behind the first of their slice (the scratch budget cut the list) */
	YKE_SLICES,              /* slices a pass on the exclusive-ownership path was counted in (fast_finish calls: one for a pass that is not cut) */
	YKE_EARLY_SLICES,        /* ... of them, the slices counted before the pass ended (budget, sub-bucket load, 2^32-position limit) */
	YKE_FAST_ABANDONED,      /* the mid-pass switch from the exclusive-ownership path to the accumulator path */
	YKE_RNG_SWEEPS,          /* extra sweeps of k_img_count_rng after its cross list filled */
	YKE_OWN_SWEEPS,          /* ... of k_img_count_own */
	YKE_PASS2_NONE,          /* yakamd_count_retained: nothing usable was retained (the caller feeds the input again) */
	YKE_PASS2_FUSED,         /* pass2_path 1: the counts of the pass before applied */
	YKE_PASS2_RECOUNT,       /* pass2_path 2: k_cnt2 over the retained sub-bucket records */
	YKE_PASS2_PREFIX,        /* pass2_path 3: the retained level-1 records counted by prefix */
	YKE_N
};

int yk_tally_register(const char *name);       /* the id of `name` (blanks and outer parentheses dropped), a new one if it is not known yet */
void yk_tally_bump(int id, uint64_t by);
static inline void yk_event(YkEvent e, uint64_t by = 1) { yk_tally_bump((int)e, by); }

template<class N> struct YkTallyId { static const int id; };
template<class N> const int YkTallyId<N>::id = yk_tally_register(N::name());

/* (the local type carries the name into the template: its static member is initialised when the library is loaded, wherever the launch stands) */
#define YK_LAUNCH(kern, ...) do { \
		struct YkName_ { static const char *name() { return #kern; } }; \
		yk_tally_bump(YkTallyId<YkName_>::id, 1); \
		hipLaunchKernelGGL(kern, __VA_ARGS__); \
	} while (0)

#endif
