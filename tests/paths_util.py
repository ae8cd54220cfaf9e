"""Which kernels a test case must have run: the library's launch tally (include/yak_amd.h: yakamd_tally_names / _read / _reset) and the
expectation tables that hold the path matrices of test_gpu_parity.py and test_gpu_pass2_fused.py to the paths their ids name.

Every fast path of the engine has an exact fallback behind it, so equal bytes say nothing about which one ran.  A table entry says it:
  ran      kernel instantiations that must have been launched (the names are the launch sites', `k_part2_wc8<false,7>`)
  not_ran  instantiations that must not have been; a trailing `*` stands for every name with that prefix
  events   host decisions that are not launches (`event:...` without the prefix): ">0" or "==0"
Each entry was derived from the branch its switch selects; the comment names the line that decides.  tests/test_paths.py (no GPU) checks the
tables against the parametrize lists and the library's names, and that every instantiation is claimed by some test."""
import contextlib
import ctypes as C


def names(lib):
    p = C.POINTER(C.c_char_p)()
    n = lib.yakamd_tally_names(C.byref(p))
    return [p[i].decode() for i in range(n)]


def read(lib):
    nm = names(lib)
    out = (C.c_uint64 * len(nm))()
    lib.yakamd_tally_read(out, len(nm))
    return {k: int(v) for k, v in zip(nm, out) if v}


@contextlib.contextmanager
def tally(lib, device=True):
    """with tally(L) as t: ...   -- afterwards t is {name: count} of everything launched / decided inside (non-zero entries only).
    device: also take in the doubling counters the device keeps (yakamd_debug_counters synchronises it)"""
    dbg = (C.c_uint32 * 4)()
    if device:
        lib.yakamd_debug_counters(dbg)                     # what the device counted before belongs to nobody here
    lib.yakamd_tally_reset()
    got = {}
    try:
        yield got
    finally:
        if device:
            lib.yakamd_debug_counters(dbg)
        got.update(read(lib))


def expand(pattern, all_names):
    if pattern.endswith("*"):
        return [n for n in all_names if n.startswith(pattern[:-1])]
    return [pattern]


def hold(got, entry, all_names, what=""):
    """assert a tally against a table entry"""
    bad = []
    for n in entry.get("ran", ()):
        if got.get(n, 0) == 0:
            bad.append("%s did not run" % n)
    for pat in entry.get("not_ran", ()):
        for n in expand(pat, all_names):
            if got.get(n, 0) != 0:
                bad.append("%s ran %d times" % (n, got[n]))
    for ev, rel in entry.get("events", {}).items():
        v = got.get("event:" + ev, 0)
        assert rel in (">0", "==0"), rel
        if (rel == ">0") != (v > 0):
            bad.append("event %s is %d, expected %s" % (ev, v, rel))
    assert not bad, "%s: %s\n  tally: %s" % (what, "; ".join(bad), {k: v for k, v in sorted(got.items())})


def E(ran=(), not_ran=(), **events):
    return dict(ran=list(ran), not_ran=list(not_ran), events=events)


# ---- names used below ----
LC2_NOFILTER = "k_lc2<false,false,false,true,false,11>"         # yk_launch_lc2 case 0, cap11, rec8_out
LC2_FILTER = "k_lc2<true,false,false,true,true,10>"             # case 4, rec8_out: the staged filter range
LC2_NOSTAGE_W6 = "k_lc2<true,false,false,true,false,10,6>"      # nostage, YAKAMD_LC2_W6 != 0
LC2_NOSTAGE_W5 = "k_lc2<true,false,false,true,false,10>"        # nostage, YAKAMD_LC2_W6 == 0
WC8_7, WC8_8, WC8_T, WC8_R = "k_part2_wc8<false,7>", "k_part2_wc8<false>", "k_part2_wc8<true>", "k_part2_wc8r"
P2_PLAIN, P2_WC16 = "k_part2<1>", "k_part2_wc<false>"
OWN_H, OWN_HX = "k_img_count_own<1,0>", "k_img_count_own<1,1>"
RNG, RNGX = "k_img_count_rng<0>", "k_img_count_rng<1>"
SORT256, SORT1024 = "k_seg_sort_pass<8,256>", "k_seg_sort_pass<8,1024>"
# the rest of a pass without a switch (feed_image's tagged extraction and its scan, fast_finish, the count pass over bare hashes, the shrink)
DEFAULT_PASS = ["k_xpart<3,31>", "k_xpart_wcs<true,31>", "k_xpart<3>", "k_xpart_wcs<true>", "k_part_sum<true>", "k_part_mid", "k_part_fin<true>", "k_part2<0>", "k_part2_scan",
                "k_lc_sum", "k_lc_compact", "k_seg_sort_pass<8,256>", "k_replay", "k_img_clear", "k_xpart<0>", "k_part_sum<false>", "k_part_fin<false>", "k_xpart_wcs<false>",
                "k_img_count_own<1,0>", "k_img_fold", "k_shrink_count", "k_shrink_scatter", "k_put_u64"]
FAST_ONLY = ["k_part2<0>", "k_lc2*", "k_lds_count_ovf"]        # what only fast_finish launches
FLAT, COMPACT = ["k_lc_sum3", "k_nsel_scan", "k_lc_gather"], ["k_lc_sum", "k_lc_compact"]
R2_SEGMENTED = ["k_r2_place", "k_r2_spill", "k_r2_headfill", "k_r2_publish"]   # yk_r2_place with nseg > 1

# ---- test_gpu_parity.py::test_every_insert_path_is_exact ----
# synth(20000, g=90000): ~2 350 records per sub-table; opts k31 / k31 -b22 / k31 -b28 / k21 -b20, all four inside one tally.  A sub-table's filter
# has 2^nb bits, nb = bf_shift - pre = 12 / 18 / 10, and slice_plan keeps s2 <= nb - 9 = 3 / 9 / 1: a forced YAKAMD_S2_BITS holds without a filter and
# (up to 9) with -b28 only; without a switch s2 = 1 / 1 / 2 / 1, below the write-combining scatters' 4 bits (k_part2<1>).  Tagged 8-byte records in
# and out (k < 32, np_max < 2^(12 + s2)).
EVERY_INSERT_PATH = {
    # engine_pass.cpp pass_begin: c->fast = ... YAKAMD_FAST != 0 -> acc_records per batch; acc_finish at the end of the pass (engine_acc.cpp)
    "general_path": E(["k_acc_init", "k_bf_check", "k_bf_mapfill", "k_bf_resolve", "k_acc_insert", "k_select_count", "k_select_scatter", SORT256, "k_bf_test", "k_bf_set", "k_lastput", "k_xpart_wc<1>"], FAST_ONLY, slices="==0", fast_abandoned="==0"),
    # slice_plan: s2 = 0; with a filter nb - 9 - s2 > 7, so yk_lc2_ok refuses and slice_count sends every sub-bucket on (h_cnt[YKC_NOVF2] = n_all)
    "lds_overflow_to_global": E(["k_lds_count_ovf", P2_PLAIN], [WC8_7, WC8_8], lc2_passed_on=">0", ovf_groups=">0", ovf_more_groups="==0"),   # -b28: nb - 9 - 0 = 9 > 7
    # fast_admit: the first batch's cost (bytes x 12) is over the budget and nothing is kept yet -> fast_abandon
    "budget_exceeded_midpass": E(["k_acc_insert", "k_select_scatter", SORT256], FAST_ONLY, fast_abandoned=">0", slices="==0"),
    # yk_launch_part2: fp.s2_bits >= 4 fails -> k_part2<1>
    "s2_3_multibatch": E([P2_PLAIN, "k_xpart_wcs<true,31>", "k_xpart_wcs<true>"], [WC8_7, WC8_8, WC8_T, P2_WC16], slices=">0", early_slices="==0", fast_abandoned="==0"),
    # pass_begin: nb_bits = 6 != pre -> c->fast = false; count pass: count_plan: key-owning ranges, LDS ranks and home-slot ranges all want nb_bits == pre -> k_img_count_h
    "part6_general": E(["k_acc_insert", "k_xpart_wc<1>", "k_img_count_h"], FAST_ONLY + ["k_img_count_own*", "k_img_count_lds*", "k_img_count_rng*"], slices="==0"),
    # yk_launch_part2: rec8_out, rec8_in, seg = 64 <= 1024, YAKAMD_P2_CAP7 != 0
    "write_combined_level2": E([WC8_7], [WC8_8, WC8_T, WC8_R, P2_WC16]),
    # without a filter seg = WC_SEG = 2048 > 1024 -> the 8-entry stacks (-b28: s2 = 9, 512 segments, the 7-entry ones)
    "write_combined_level2_wide": E([WC8_8], [WC8_T, WC8_R, P2_WC16]),
    "write_combined_level2_segments": E([WC8_8], [WC8_T, WC8_R, P2_WC16]),
    # yk_launch_part2: wc = YAKAMD_P2_WC = 0 -> the last branch
    "plain_scatters": E([P2_PLAIN], [WC8_7, WC8_8, WC8_T, WC8_R, P2_WC16]),
    # count_records: count_plan finds neither key-owning ranges nor LDS ranks -> YK_COUNT_RANGES, count_by_ranges
    "range_count_whole_table": E(["k_hpart2<0>", "k_hpart2<1>", RNG], [RNGX, "k_img_count_own*", "k_img_count_lds*"], rng_sweeps="==0"),
    "range_count_split": E(["k_hpart2<1>", RNG, "k_img_count_h"], [RNGX, "k_img_count_own*", "k_img_count_lds*"], rng_sweeps="==0"),   # xn[0] boundary-crossing instances -> k_img_count_h
    # count_by_ranges (XList::run): xn[1] (list too small) -> the cross sweep
    "range_count_cross_sweep": E([RNG, RNGX], ["k_img_count_own*"], rng_sweeps=">0"),
    "range_count_short_list": E([RNG, RNGX], ["k_img_count_own*"], rng_sweeps=">0"),
    # count_plan: all three refused -> YK_COUNT_ATOMICS, YK_FMT_HASH
    "count_with_device_atomics": E(["k_img_count_h"], ["k_img_count_own*", "k_img_count_lds*", "k_img_count_rng*", "k_hpart2*"]),
    # count_plan: YK_COUNT_LDS -> yk_launch_img_count_lds, YK_FMT_HASH
    "count_lds_rank_kernel": E(["k_img_count_lds<1>"], ["k_img_count_own*", "k_img_count_rng*", "k_img_count_h", "k_img_count_lds<2>"]),
    # count_plan, key-owning ranges: the LDS budget leaves 32-slot ranges (THIN_INPUT: sub-tables of 1024 / 2048 slots; a whole table of up to ~250 keys is cheaper
    # than any range of it, e + e / 8 + 192 keys of room); the list holds every boundary-crossing instance -> XList::run's k_img_count_h over it
    "key_owning_count_32_slot_ranges": E([OWN_H, "k_xpart_wcs<false>", "k_img_count_h"], [OWN_HX, "k_img_count_rng*", "k_img_count_lds*"], own_sweeps="==0"),
    # count_own (XList::run): xn[1] -> the cross sweep
    "key_owning_count_cross_sweep": E([OWN_H, OWN_HX], ["k_img_count_rng*"], own_sweeps=">0"),
    "key_owning_count_short_list": E([OWN_H, OWN_HX], ["k_img_count_rng*"], own_sweeps=">0"),
    # yk_lc2_ok: YAKAMD_LC2 = 0 -> slice_count's !lc2 branch
    "three_tier_lds_kernels": E(["k_lds_count_ovf"], ["k_lc2*"], lc2_passed_on=">0"),
    "three_tier_lds_kernels_crowded": E(["k_lds_count_ovf", WC8_7], ["k_lc2*"], lc2_passed_on=">0"),
    # a grid size only (yk_launch_lc2: wgs): the same instances as without the switch
    "lc2_three_persistent_workgroups": E([LC2_NOFILTER, LC2_FILTER] + DEFAULT_PASS, ["k_lc2<false,false,false,true,false,10>"]),
    # feed_image: the consumed format stays YK_FMT_HASH, no range tag: the same kernels as with the tag (an argument of k_xpart_wcs<false> and k_img_count_own)
    "pass2_plain_hashes": E(["k_xpart_wcs<false>", OWN_H], [OWN_HX, "k_xpart<2>", "k_xpart_wc<2>"], own_sweeps="==0"),
    "pass2_plain_hashes_cross_sweep": E([OWN_H, OWN_HX], [], own_sweeps=">0"),
    # r2_steps: k_r2_dsmall takes YAKAMD_R2_SMALL_F; only a streaming replay launches it (YAKAMD_R2_SMALL_BITS = 5 makes the 1024-slot sub-tables large)
    "replay_prefix_16": E(["k_r2_dsmall", "k_r2_double<5,false,1>", "k_r2_place"], [], r2_used=">0", r2_refused="==0"),
    "replay_prefix_1024": E(["k_r2_dsmall", "k_r2_double<5,false,1>", "k_r2_place"], [], r2_used=">0", r2_refused="==0"),
    # feed_image: kept = YK_FMT_POS -> {hash, position} records; yk_launch_part2's third branch; k_lc2 with R8 = false
    "rec16_records": E(["k_xpart_wc<1>", P2_PLAIN, "k_lc2<false,false,false,false,false,11>", "k_lc2<true,false,false,false,true,10>"], ["k_xpart_wcs<true*", WC8_7, WC8_8, WC8_T, LC2_NOFILTER, LC2_FILTER]),
    # slice_plan: rec8_out = 0 -> yk_launch_part2's second branch (tagged in, {hash, rank} out), which wants s2 >= 4 (YAKAMD_S2_BITS = 6)
    "tagged_in_rec16_out": E([WC8_T, "k_lc2<false,false,false,false,false,11>", "k_lc2<true,false,false,false,true,10>"], [WC8_7, WC8_8, WC8_R, LC2_NOFILTER, LC2_FILTER]),
    "tagged_in_rec16_out_multibatch": E([P2_PLAIN, "k_lc2<false,false,false,false,false,11>", "k_lc2<true,false,false,false,true,10>"], [WC8_7, WC8_8, WC8_R, LC2_NOFILTER, LC2_FILTER]),
    "tagged_multibatch_s2_3": E([P2_PLAIN, "k_xpart_wcs<true,31>"], [WC8_7, WC8_8, WC8_T], early_slices="==0"),
    # r2_plan: classify with SB = 5 -> every sub-table beyond 32 slots is large; r2_publish_commit counts
    "streaming_replay_from_32_slots": E(["k_r2_trail", "k_r2_double<16,false,1>", "k_r2_load", "k_r2_binit", "k_r2_dsmall", "k_r2_double<5,false,1>", "k_r2_place", "k_r2_publish"], [], r2_used=">0", r2_refused="==0"),
    # yk_r2_place: nseg = 2^(bmax - SL) > 1 -> k_r2_ppart, k_r2_spill, k_r2_headfill
    # (THIN_INPUT: sub-tables of 4096 slots, more than one segment)
    "streaming_replay_1k_slot_segments": E(["k_r2_ppart"] + R2_SEGMENTED, ["k_r2_ppart_cnt"], r2_used=">0", r2_refused="==0"),
    "streaming_replay_2k_slot_segments": E(["k_r2_ppart"] + R2_SEGMENTED, ["k_r2_ppart_cnt"], r2_used=">0", r2_refused="==0"),
    # run_replay_v2: YAKAMD_REPLAY2 = 0 -> 1 -> yk_run_replay's k_replay
    "k_replay_only": E(["k_replay"], ["k_r2_*"], r2_used="==0", r2_refused="==0"),
    # yk_r2_place: G > 1 && pcnt -> the three-kernel grouping
    "streaming_replay_keys_grouped_by_3_workgroups": E(["k_r2_ppart_cnt", "k_r2_ppart_scan", "k_r2_ppart_scat"] + R2_SEGMENTED, ["k_r2_ppart"], r2_used=">0", r2_refused="==0"),
    # yk_r2_double: knob 64 -> nw = 6 (more than 256 sub-tables double), il = 4
    "streaming_replay_keys_grouped_by_16_workgroups_6_wave_doubling": E(["k_r2_ppart_cnt", "k_r2_ppart_scat", "k_r2_double<6,false,4>"] + R2_SEGMENTED, ["k_r2_ppart", "k_r2_double<5,*"], r2_used=">0", r2_refused="==0"),
    # fast_admit: the budget holds three batches -> fast_flush_slice; later slices meet a table (img_nonempty: k_lc2 cases 2 and 6)
    "pass_in_slices": E(["k_lc2<false,true,false,true,false,11>", "k_lc2<true,true,false,true,true,10>", LC2_NOFILTER], ["k_acc_insert"], early_slices=">0", fast_abandoned="==0"),
    "pass_in_single_batch_slices": E(["k_lc2<false,true,false,true,false,11>", "k_lc2<true,true,false,true,true,10>"], ["k_acc_insert"], early_slices=">0", fast_abandoned="==0"),
    "pass_in_two_slices": E(["k_lc2<false,true,false,true,false,11>", "k_lc2<true,true,false,true,true,10>"], ["k_acc_insert"], early_slices=">0", fast_abandoned="==0"),
    # slice_count: a sub-bucket's scratch table is 5 x 8192 words, the budget of 200 000 takes four -> many groups
    "lds_overflow_to_global_in_groups": E(["k_lds_count_ovf"], [], lc2_passed_on=">0", ovf_more_groups=">0"),
    # fast_admit: kept_n + n_cap > sub-tables x YAKAMD_SLICE_SB x per_sb -> fast_flush_slice
    "slices_cut_by_sub_bucket_load": E(["k_lc2<false,true,false,true,false,11>"], ["k_acc_insert"], early_slices=">0", fast_abandoned="==0"),
    # slice_plan: three = s2 > p3_min; slice_partition: first sweep rec8_out = 0 (k_part2_wc8<true>), second rec8_in = 0 (k_part2_wc8r)
    "level2_two_sweeps": E([WC8_T, WC8_R], [WC8_7, WC8_8]),
    # s2a = 6, s2b = 3 < 4 -> the second sweep is k_part2<1>
    "level2_two_sweeps_plain_second_multibatch": E([WC8_T, P2_PLAIN], [WC8_R, WC8_7, WC8_8]),
    # second sweep with rec8_out = 0 and rec8_in = 0 -> k_part2_wc<false>
    "level2_two_sweeps_rec16_out": E([WC8_T, P2_WC16], [WC8_R, WC8_7, WC8_8]),
    # {hash, position} records in: both sweeps k_part2_wc<false>
    "level2_two_sweeps_rec16_in": E(["k_xpart_wc<1>", P2_WC16], [WC8_T, WC8_R, WC8_7, WC8_8]),
    # without a filter s2 = 14 > 13 -> two sweeps of 4 and 10 bits (with one, s2 <= nb - 9 <= 13 stays one sweep)
    "level2_two_sweeps_16k_sub_buckets": E([WC8_T, WC8_R], [P2_WC16]),
    # slice_gather: flat
    "flat_gather": E(FLAT, COMPACT),
    "flat_gather_multibatch": E(FLAT + [WC8_7], COMPACT),
    "one_workgroup_per_sub_table_gather": E(COMPACT, FLAT),
    # slice_gather: s.tsort = YAKAMD_TSORT -> slice_sort's !sorted loop only
    "sort_stable_radix_passes": E([SORT256], ["k_ts_rank", "k_part2<0,true>", SORT1024], rank_refused="==0"),
    # s.tsort = 1, tbits = 12 -> ts_b = 1: one partition sweep by time, then k_ts_rank; h_fail == 0 leaves the radix passes out
    "sort_bitmap_ranks": E(["k_ts_rank", "k_part2<0,true>"], [SORT256, SORT1024], rank_refused="==0"),
    # ts_b = 0: no partition sweep
    "sort_one_bin_per_sub_table": E(["k_ts_rank"], ["k_part2<0,true>", "k_part2<1,true>", "k_part2_wc<true>", SORT256, SORT1024], rank_refused="==0"),
    # yk_launch_part2_ts: s2_bits = 3 < 4 -> k_part2<1, true>
    "sort_8_bins_plain_scatter": E(["k_ts_rank", "k_part2<0,true>", "k_part2<1,true>"], ["k_part2_wc<true>", SORT256], rank_refused="==0"),
    "sort_64_bins_multibatch": E(["k_ts_rank", "k_part2<0,true>", "k_part2_wc<true>"], ["k_part2<1,true>", SORT256], rank_refused="==0"),
    "sort_4096_bins_in_segments": E(["k_ts_rank", "k_part2_wc<true>"], ["k_part2<1,true>", SORT256], rank_refused="==0"),
    "sort_bins_joined_by_8": E(["k_ts_rank", "k_part2_wc<true>"], [SORT256], rank_refused="==0"),
    "sort_joined_bins_beyond_the_stage": E(["k_ts_rank", "k_part2_wc<true>"], [SORT256], rank_refused="==0"),
    # k_ts_rank's window loop is a branch inside the kernel (a bin with more keys than the stage's cap = YAKAMD_TS_CAP = 64): the test asserts on its
    # own input that a sub-table of the unfiltered count -- its one bin -- holds more than 64 keys (BIN_OVER_STAGE)
    "sort_one_bin_in_windows": E(["k_ts_rank"], ["k_part2<0,true>", SORT256, SORT1024], rank_refused="==0"),
    # the pool's switches select nothing a launch shows: the pass must still be the default one, on the exclusive-ownership path
    "every_buffer_prefilled_with_0xa5": E([LC2_NOFILTER, LC2_FILTER, "k_replay"], ["k_acc_insert"], fast_abandoned="==0", early_slices="==0"),
    "every_buffer_zeroed_superblocks_only": E([LC2_NOFILTER, LC2_FILTER, "k_replay"], ["k_acc_insert"], fast_abandoned="==0", early_slices="==0"),
    "mapped_ranges_from_1_mib_prefilled": E([LC2_NOFILTER, LC2_FILTER, "k_replay"], ["k_acc_insert"], fast_abandoned="==0", early_slices="==0"),
    "mapped_ranges_from_4_mib_pass_in_slices": E(["k_lc2<false,true,false,true,false,11>", "k_lc2<true,true,false,true,true,10>"], ["k_acc_insert"], fast_abandoned="==0", early_slices=">0"),
    "mapped_ranges_taken_apart_prefilled": E([LC2_NOFILTER, LC2_FILTER, "k_replay"], ["k_acc_insert"], fast_abandoned="==0", early_slices="==0"),
    "mapped_ranges_taken_apart_pass_in_slices": E(["k_lc2<false,true,false,true,false,11>", "k_lc2<true,true,false,true,true,10>"], ["k_acc_insert"], fast_abandoned="==0", early_slices=">0"),
    # yk_launch_part2: YAKAMD_P2_CAP7 = 0 -> tagged records in, segments of 64: the 8-entry stacks
    "level2_8_entry_stacks": E([WC8_8], [WC8_7, WC8_T]),
    # yk_r2_double: more than 256 sub-tables double -> nw and il from the switch
    "doubling_5_waves_2_walks": E(["k_r2_double<5,false,2>"], ["k_r2_double<6,*", "k_r2_double<5,false,1>", "k_r2_double<5,false,4>"], r2_used=">0", r2_refused="==0"),
    "doubling_6_waves_1_walk": E(["k_r2_double<6,false,1>"], ["k_r2_double<5,*", "k_r2_double<6,false,2>", "k_r2_double<6,false,4>"], r2_used=">0", r2_refused="==0"),
    # yk_lc2_per_sb: YAKAMD_LC2_CAPB = 10 -> 600 per sub-bucket, cap11 false: the 1024-slot table; in slices, so that later ones meet a table (I = true)
    "lc2_1024_slot_table_in_slices": E(["k_lc2<false,false,false,true,false,10>", "k_lc2<false,true,false,true,false,10>"], [LC2_NOFILTER, "k_lc2<false,true,false,true,false,11>"], early_slices=">0"),
    "lc2_1024_slot_table_in_slices_rec16_out": E(["k_lc2<false,false,false,false,false,10>", "k_lc2<false,true,false,false,false,10>"], [LC2_NOFILTER, "k_lc2<false,false,false,false,false,11>", "k_lc2<false,false,false,true,false,10>"], early_slices=">0"),
}
# cases of test_every_insert_path_is_exact whose path needs larger sub-tables than synth(20000, g=90000) gives (~540 keys, 1024 slots, without a
# filter; ~100 keys with one): the same reads over a 2 Mb genome, 1.5 x -- ~2 300 keys per sub-table (4096 slots: several segments of 1024 or 2048
# slots for the streaming replay) without a filter, 500-1 400 with one (enough for count_plan to cut ranges)
THIN_INPUT = {"streaming_replay_1k_slot_segments", "streaming_replay_2k_slot_segments", "streaming_replay_keys_grouped_by_3_workgroups",
              "streaming_replay_keys_grouped_by_16_workgroups_6_wave_doubling",
              "key_owning_count_32_slot_ranges", "key_owning_count_cross_sweep", "key_owning_count_short_list", "pass2_plain_hashes_cross_sweep"}

# ---- test_gpu_parity.py::test_replay_variants_on_large_subtables ----
# ~5 800 keys per sub-table without a filter (8 Ki slots), ~1 900 with -b30 (4 Ki slots); the switches of k_replay are arguments of the one kernel
K_REPLAY = E(["k_replay"], [], r2_refused="==0")
REPLAY_VARIANTS = {
    "lds_ranks": K_REPLAY, "global_ranks": K_REPLAY, "lds_16bit_ranks": K_REPLAY,
    # kern_layout.inc: the parallel doubling is skipped under YAKAMD_PAR_REPLAY = 0 (no scratch for it: sp == 0)
    "serial_doubling": E(["k_replay"], [], par_ok="==0", par_fail="==0"),
    # count_plan: bmax = 12 > RNG_LOG = 10 -> rb = 2
    "pass2_by_slot_ranges": E(["k_hpart2<0>", "k_hpart2<1>", RNG], ["k_img_count_own*", "k_img_count_lds*"], rng_sweeps="==0"),
    "pass2_ranges_list_overflow": E([RNG, RNGX], ["k_img_count_own*"], rng_sweeps=">0"),
    "streaming_replay_2k_slot_segments": E(["k_r2_ppart"] + R2_SEGMENTED, ["k_r2_ppart_cnt"], r2_used=">0", r2_refused="==0"),
    "streaming_replay_from_512_slots_1k_slot_segments": E(["k_r2_ppart"] + R2_SEGMENTED, ["k_r2_ppart_cnt"], r2_used=">0", r2_refused="==0"),
    "k_replay_for_16k_slots": E(["k_replay"], ["k_r2_*"], r2_used="==0", r2_refused="==0"),
    "streaming_replay_keys_grouped_by_4_workgroups": E(["k_r2_ppart_cnt", "k_r2_ppart_scan", "k_r2_ppart_scat"] + R2_SEGMENTED, ["k_r2_ppart"], r2_used=">0", r2_refused="==0"),
    # yk_r2_double: more than 256 sub-tables double -> nw from the switch's tens, il from its units
    "doubling_6_waves_2_walks": E(["k_r2_double<6,false,2>"], ["k_r2_double<5,*", "k_r2_double<6,false,1>"], r2_used=">0", r2_refused="==0"),   # (a step in which at most 256 double takes 16 waves)
    "doubling_5_waves_4_walks": E(["k_r2_double<5,false,4>"], ["k_r2_double<6,*", "k_r2_double<5,false,1>"], r2_used=">0", r2_refused="==0"),
    "pass2_key_owning_ranges": E([OWN_H], [OWN_HX, "k_img_count_rng*"], own_sweeps="==0"),
    "pass2_key_owning_ranges_list_overflow": E([OWN_H, OWN_HX], ["k_img_count_rng*"], own_sweeps=">0"),
    "pass2_key_owning_ranges_plain_hashes": E([OWN_H, OWN_HX], ["k_img_count_rng*"], own_sweeps=">0"),
    # (with YAKAMD_R2_SMALL_BITS = 10: at 2^13 slots no sub-table is large for the default 13, and no streaming replay runs)
    "replay_prefix_32": E(["k_r2_dsmall", "k_r2_double<5,false,1>"], [], r2_used=">0", r2_refused="==0"),
    "lds_keys_for_small_stages": K_REPLAY, "segmented_lds_ranks": K_REPLAY, "segmented_lds_ranks_small": K_REPLAY, "global_ranks_for_large_stages": K_REPLAY,
}

# ---- test_gpu_parity.py::test_low_complexity_bursts ----  opts k31 / k31 -b28 / k15 -b27 / k33 ({hash, position} records: k >= 32)
LOW_COMPLEXITY = {
    # ~750 records per sub-table: s2 = 0 without a filter, nb - 9 - 7 = 2 / 1 with -b28 / -b27: below 4 bits, k_part2<1>
    "auto": E(["k_xpart_wcs<true,31>", "k_xpart_wcs<true>", "k_xpart_wc<1>", P2_PLAIN], [WC8_7, WC8_8]),
    "s2_5": E(["k_xpart_wcs<true,31>", "k_xpart_wc<1>", WC8_7, P2_WC16], [P2_PLAIN, WC8_8]),
    "s2_8_multibatch": E(["k_xpart_wcs<true,31>", "k_xpart_wc<1>", WC8_7, P2_WC16], [P2_PLAIN, WC8_8]),
}

# ---- test_gpu_parity.py::test_device_batching_is_invisible ----  the accumulator path (YAKAMD_FAST = 0), the only one that works batch by batch
DEVICE_BATCHING = {
    # acc_reserve: the table grows with the batches -> k_acc_rehash; bloom_phases per batch
    "batch4k": E(["k_acc_insert", "k_acc_rehash", "k_bf_test", "k_bf_set", "k_lastput", "k_lastput_merge"], FAST_ONLY, slices="==0"),
    "batch8k_tail100": E(["k_acc_insert", "k_acc_rehash", "k_lastput", "k_lastput_merge"], FAST_ONLY, slices="==0"),
    "batch64k_tail1": E(["k_acc_insert", "k_lastput", "k_lastput_merge"], FAST_ONLY, slices="==0"),
    # bloom_phases: a `multi` filter of 1024 bits marks something in every batch -> k_bf_check
    "multi10": E(["k_acc_insert", "k_bf_set", "k_bf_check"], FAST_ONLY, slices="==0"),
}

# ---- test_gpu_parity.py::test_second_pass_counts_the_records_the_first_pass_retained ----  keyed by the id of `env`
SECOND_PASS_RETAINED = {
    # slice_plan: nowb_plan (one slice into an empty table, records kept) -> yk_launch_lc2's nostage; yakamd_count_retained's first branch
    "subbucket_records": E([LC2_NOSTAGE_W6, "k_cnt2_apply"], ["k_cnt2<*", LC2_FILTER, LC2_NOSTAGE_W5], pass2_fused=">0", pass2_none="==0"),
    "subbucket_records_many_batches": E([LC2_NOSTAGE_W6, "k_cnt2_apply"], ["k_cnt2<*", LC2_FILTER], pass2_fused=">0", early_slices="==0"),
    # yk_launch_cnt2 (YAKAMD_CNT2_FUSED = 0: slice_count allocates no lo_c2, yakamd_count_retained's second branch): n_keys / n_sb <= small_max
    "subbucket_records_3_workgroups": E(["k_cnt2<512,320>", "k_cnt2_apply"], ["k_cnt2<2048,1280>"], pass2_recount=">0", pass2_fused="==0"),
    # slice_retain: YAKAMD_RETAIN2 = 0 -> the level-1 records; yakamd_count_retained's last branch (consume_records, YK_FMT_TAGGED)
    "prefix_records": E([LC2_FILTER, OWN_H], ["k_cnt2*", LC2_NOSTAGE_W6], pass2_prefix=">0", pass2_none="==0"),
    "prefix_records_many_batches": E([LC2_FILTER, OWN_H], ["k_cnt2*", LC2_NOSTAGE_W6], pass2_prefix=">0", pass2_none="==0"),
    # slice_plan: budget 0 -> nothing kept; yakamd_count_retained returns 1 and the test feeds the input
    "budget_refuses": E([LC2_FILTER, OWN_H], ["k_cnt2*"], pass2_none=">0", pass2_fused="==0", pass2_prefix="==0"),
    # count_plan refuses tagged records -> 1; the feed then counts with k_img_count_lds
    "count_kernel_not_applicable": E(["k_img_count_lds<1>"], ["k_cnt2*", "k_img_count_own*"], pass2_none=">0", pass2_prefix="==0"),
    # small_max = -1 -> the 2048-slot table
    "subbucket_records_big_lds_table": E(["k_cnt2<2048,1280>"], ["k_cnt2<512,320>"], pass2_recount=">0", pass2_fused="==0"),
    "subbucket_records_small_lds_table_overfull": E(["k_cnt2<512,320>"], ["k_cnt2<2048,1280>"], pass2_recount=">0", pass2_fused="==0"),
    "subbucket_records_small_lds_table": E(["k_cnt2<512,320>"], ["k_cnt2<2048,1280>"], pass2_recount=">0", pass2_fused="==0"),
    "subbucket_records_flat_gather": E(FLAT + ["k_cnt2_apply"], ["k_lc_compact", "k_cnt2<*"], pass2_fused=">0"),
    # s2 <= nb - 9 = 5 / 1 / 3 for -b24 / -b20 / -b22: only -b24 is beyond YAKAMD_P3_MIN = 3 and takes two sweeps, of 4 bits (tagged in, {hash, rank}
    # out) and 1 bit (k_part2<1>); the other two filters leave too few sub-buckets for a second sweep
    "subbucket_records_level2_two_sweeps": E(["k_cnt2_apply"], ["k_cnt2<*"], pass2_fused=">0"),
    "k31b24-subbucket_records_level2_two_sweeps": E([WC8_T, P2_PLAIN, "k_cnt2_apply"], [WC8_R, WC8_7, "k_cnt2<*"], pass2_fused=">0"),
    # yk_launch_lc2: nostage and YAKAMD_LC2_W6 = 0 -> the five-wave instance
    "subbucket_records_no_stage_five_waves": E([LC2_NOSTAGE_W5, "k_cnt2_apply"], [LC2_NOSTAGE_W6, LC2_FILTER], pass2_fused=">0"),
}

# ---- test_gpu_pass2_fused.py ----
COUNT_PASS_FROM_FIRST = {   # ::test_count_pass_from_the_first_pass_counts, id of `fused`
    "fused": E([LC2_NOSTAGE_W6, "k_cnt2_apply"], ["k_cnt2<*"], pass2_fused=">0", pass2_recount="==0"),
    "recount": E([LC2_NOSTAGE_W6, "k_cnt2<512,320>", "k_cnt2_apply"], ["k_cnt2<2048,1280>"], pass2_recount=">0", pass2_fused="==0"),
}
FUSED_GATHER_AND_TIER = {   # ::test_fused_counts_on_every_gather_and_tier
    "flat_gather": E(FLAT + ["k_cnt2_apply"], ["k_lc_compact", "k_cnt2<*"], pass2_fused=">0"),
    "compact_gather": E(COMPACT + ["k_cnt2_apply"], ["k_lc_gather", "k_lc_sum3", "k_cnt2<*"], pass2_fused=">0"),
    # slice_gather: tsort -> the gather writes {key, time} pairs, the retained key list is split off them (k_kt_split)
    "gather_to_pairs": E(["k_ts_rank", "k_kt_split", "k_cnt2_apply"], [SORT256, "k_cnt2<*"], pass2_fused=">0", rank_refused="==0"),
    "all_sub_buckets_to_the_scratch_tier": E(["k_lds_count_ovf", "k_cnt2_apply"], ["k_lc2*", "k_cnt2<*"], pass2_fused=">0", lc2_passed_on=">0"),
    # slice_plan: nowb_plan false -> the staged instance, bits kept in LDS and dropped (bf_nowb)
    "filter_stage": E([LC2_FILTER, "k_cnt2_apply"], [LC2_NOSTAGE_W6, LC2_NOSTAGE_W5, "k_cnt2<*"], pass2_fused=">0"),
    "filter_written": E([LC2_FILTER, "k_cnt2_apply"], [LC2_NOSTAGE_W6, LC2_NOSTAGE_W5, "k_cnt2<*"], pass2_fused=">0"),
}
INC_AND_SHRINK = {          # ::test_inc_and_shrink_between_the_passes
    "fused": E(["k_img_inc", "k_shrink_count", "k_shrink_scatter", "k_cnt2_apply"], ["k_cnt2<*"], pass2_fused=">0"),
    "recount": E(["k_img_inc", "k_shrink_count", "k_cnt2<512,320>"], [], pass2_recount=">0", pass2_fused="==0"),
}
SUB_BUCKETS_PASSED_ON = {"": E([LC2_NOSTAGE_W6, "k_lds_count_ovf", "k_cnt2_apply"], [], lc2_passed_on=">0", ovf_groups=">0", pass2_fused=">0")}
# ::test_seg_sort_pass_of_long_segments (test_gpu_parity.py): slice_sort's sort_big = n_sel / (phi - plo) >= 30000
LONG_SEGMENTS = {"": E([SORT1024], [SORT256, "k_ts_rank"], rank_refused="==0")}

# ---- test_gpu_parity.py::test_count_pass_over_hashed_records ----  count_records with YK_FMT_POS: the W = 2 / MODE 2 instances
HASHED_RECORDS = {
    # count_plan: key-owning ranges and LDS ranks refused, the home-slot ranges want hashes alone -> YK_COUNT_ATOMICS, YK_FMT_POS
    "device_atomics": E(["k_rpart<0>", "k_rpart<1>", "k_img_count"], ["k_img_count_own*", "k_img_count_lds*", "k_img_count_rng*", "k_img_count_h"]),
    "lds_rank_kernel": E(["k_img_count_lds<2>"], ["k_img_count_own*", "k_img_count_lds<1>", "k_img_count", "k_img_count_h"]),
    # yk_launch_img_count_own: YK_FMT_POS -> W = 2; the crossing instances of the 32-slot ranges go through the list (k_img_count_h)
    "key_owning_ranges": E(["k_img_count_own<2,0>", "k_img_count_h"], ["k_img_count_own<2,1>", "k_img_count_own<1,*", "k_img_count_lds*"], own_sweeps="==0"),
    "key_owning_ranges_cross_sweep": E(["k_img_count_own<2,0>", "k_img_count_own<2,1>"], ["k_img_count_own<1,*", "k_img_count_lds*"], own_sweeps=">0"),
}

# ---- test_gpu_adversarial.py ----  clustered tables (tests/adversarial_util.py): one sub-table of chosen home slots, blocks and counts per image
# The rows, taken from the matrices above.  An entry's key is "<case>.<row>"; its tally is the count without a filter (k = 31) alone, where the
# put-by-put model speaks for the table: tests/test_adversarial.py derives r2_used / r2_refused of every entry from the model's report and the
# thresholds of kern_replay2.inc (adversarial_util.refusal_codes), so an entry cannot be fitted to a run
ADVERSARIAL_ROWS = {
    "default": dict(),
    "sb5": dict(YAKAMD_R2_SMALL_BITS="5"), "sb5_seg10": dict(YAKAMD_R2_SMALL_BITS="5", YAKAMD_R2_SEG_LOG="10"),
    "sb5_prefix1024": dict(YAKAMD_R2_SMALL_F="1024", YAKAMD_R2_SMALL_BITS="5"),
    "sb5_dbl61": dict(YAKAMD_R2_SMALL_BITS="5", YAKAMD_R2_DBL="61"), "sb5_dbl52": dict(YAKAMD_R2_SMALL_BITS="5", YAKAMD_R2_DBL="52"),
    "replay2_off": dict(YAKAMD_REPLAY2="0"),
    "replay_lds_0": dict(YAKAMD_REPLAY_LDS="0"), "replay_lds_1024": dict(YAKAMD_REPLAY_LDS="1024", YAKAMD_REPLAY_THREADS="256"), "replay_lds_8192": dict(YAKAMD_REPLAY_LDS="8192"),
    "lc2_off": dict(YAKAMD_LC2="0"), "lc2_capb10": dict(YAKAMD_LC2_CAPB="10", YAKAMD_FAST_BUDGET="3000000", YAKAMD_BATCH="65536"),
    "slices": dict(YAKAMD_FAST_BUDGET="1100000", YAKAMD_BATCH="65536"),
    "fast_off": dict(YAKAMD_FAST="0"),
}
R2_ONE = ["k_replay", "k_r2_trail", "k_r2_load", "k_r2_binit", "k_r2_dsmall", "k_r2_double<16,false,1>", "k_r2_place", "k_r2_publish"]   # yk_r2_double: n_dbl <= 256 -> 16 waves, whatever YAKAMD_R2_DBL says
R2_ONE_SEG = R2_ONE + R2_SEGMENTED + ["k_r2_ppart_cnt", "k_r2_ppart_scan", "k_r2_ppart_scat"]        # r2_buffers: n_large = 1 -> ppG = 16 workgroups group the keys
_NOT_LARGE = E(["k_replay"], ["k_r2_*"], r2_used="==0", r2_refused="==0")                            # r2_plan: classify() finds no sub-table beyond 2^SB slots
_USED, _USED_SEG = E(R2_ONE, [], r2_used=">0", r2_refused="==0"), E(R2_ONE_SEG, ["k_r2_ppart"], r2_used=">0", r2_refused="==0")
_REFUSED, _REFUSED_SEG = E(R2_ONE, [], r2_used="==0", r2_refused=">0"), E(R2_ONE_SEG, ["k_r2_ppart"], r2_used="==0", r2_refused=">0")   # r2_publish_commit: h_fail -> 1 -> yk_run_replay's k_replay
_OFF = E(["k_replay"], ["k_r2_*"], r2_used="==0", r2_refused="==0")                                  # run_replay_v2: YAKAMD_REPLAY2 = 0 -> 1
ADVERSARIAL = {
    # ---- one sub-table of 16 Ki slots, streamed from 8 Ki on (SB = 13): the last doubling's old table holds the runs the case lays out ----
    # runs of up to 512 slots: r2_wave_run takes L <= R2_LMAX (kern_replay2.inc:152, :163); 255 and more go to s_big (:577, :621)
    "run_ladder_plain.default": _USED,
    "run_ladder_over.default": _REFUSED,             # a run of 513: L > R2_LMAX -> fail = 6 (:163)
    # the table's last run (100 slots) reaches its end, keys of it go around: wrap = 2 * min(128, 236) + 2 = 258 slots of the new table's start (:157-161)
    "run_ladder_wrap.default": _USED,
    # R2_MMAX: hand_over (:576) places the last run in the wave's own LDS up to 192 slots, R = 2 * 192 + 2 + 12 <= 642; 193 goes to wave 0's (s_big)
    "run_ladder_tail192.default": _USED, "run_ladder_tail193.default": _USED,
    "long_prefix.default": _REFUSED,                 # slots [0, 4100] used: F0 = 4102 > R2_BASE_MAX -> fail = 1 (:417)
    # 32 Ki slots, two segments of 16 Ki: a walk may end on slot HEAD - 1 = 2047 of the next head (k_r2_spill :1030); cluster - 2 is the farthest
    "segment_mid_15_100.default": _USED_SEG, "segment_mid_15_2049.default": _USED_SEG,
    "segment_mid_15_2050.default": _REFUSED_SEG,     # fail = 5
    "segment_end_15_600.default": _USED_SEG,         # the last segment's walks go on in segment 0 (k_r2_place :988: (seg + 1) & (nseg - 1))
    # ---- streamed from 32 slots on (SB = 5); k_r2_dsmall works on the arrays below 2048 slots (:359), its prefix is the whole first run ----
    "one_home_zero_200.sb5": _USED, "one_home_mid_200.sb5": _USED, "one_home_last_200.sb5": _USED,
    "one_home_zero_392.sb5": _USED, "one_home_mid_392.sb5": _USED,
    # the one key of the last run finds the first 258 slots of the new table taken by the 382 keys before it: li >= R -> fail = 7 (:192)
    "one_home_last_392.sb5": _REFUSED, "one_home_last_1544.sb5": _REFUSED, "lastput_growth.sb5": _REFUSED,
    "run_ladder_wrap.sb5": _USED, "segment_mid_12_513.sb5": _USED, "segment_end_12_300.sb5": _USED,
    # segments of 1 Ki slots, HEAD = 512 (kern_launch.inc:498)
    "segment_mid_12_513.sb5_seg10": _USED_SEG, "segment_mid_12_514.sb5_seg10": _REFUSED_SEG, "segment_end_12_300.sb5_seg10": _USED_SEG,
    "one_home_mid_392.sb5_seg10": _USED, "segment_mid_15_2049.sb5_seg10": _REFUSED_SEG,
    # the rounds below YAKAMD_R2_SMALL_F = 1024 run in k_r2_dsmall (r2_small_rounds): r2_run places runs of up to R2_LONG = 8 slots, a wave the longer ones (:84, :309)
    "run_ladder_plain.sb5_prefix1024": _USED, "one_home_zero_392.sb5_prefix1024": _USED,
    "run_ladder_over.replay2_off": _OFF, "one_home_last_392.replay2_off": _OFF,
    # ---- k_replay's rank variants on a table of one cluster (4 Ki slots: not large at SB = 13) ----
    "one_home_last_1544.replay_lds_0": _NOT_LARGE, "one_home_last_1544.replay_lds_1024": _NOT_LARGE, "one_home_last_1544.replay_lds_8192": _NOT_LARGE,
    # ---- the LDS counting table: without a filter s2 = 0 (slice_plan: n_total / P is small), the sub-table is one sub-bucket ----
    # Lc2Cfg::FULL = CAP / 4 * 3 = 1536 distinct keys (kern_count.inc:567, :721); one more is passed on to k_lds_count_ovf
    "hot_block_9.default": E([LC2_NOFILTER], ["k_lds_count_ovf"], lc2_passed_on="==0"), "hot_block_600.default": E([LC2_NOFILTER], ["k_lds_count_ovf"], lc2_passed_on="==0"),
    "hot_block_probes_600.default": E([LC2_NOFILTER], ["k_lds_count_ovf"], lc2_passed_on="==0"),
    "hot_block_1536.default": E(["k_lc2<false,false,false,true,false,11>"], ["k_lds_count_ovf"], lc2_passed_on="==0"),
    "hot_block_1537.default": E(["k_lds_count_ovf"], [], lc2_passed_on=">0", ovf_groups=">0"),
    "hot_block_3000.default": E(["k_lds_count_ovf"], [], lc2_passed_on=">0", ovf_groups=">0"),
    # YAKAMD_LC2_CAPB = 10: 1024 slots, FULL = 768
    "hot_block_768.lc2_capb10": E(["k_lc2<false,false,false,true,false,10>"], ["k_lds_count_ovf", LC2_NOFILTER], lc2_passed_on="==0"),
    "hot_block_769.lc2_capb10": E(["k_lds_count_ovf"], [LC2_NOFILTER], lc2_passed_on=">0", ovf_groups=">0"),
    # one key 2047 ... 70 000 times: more than 2^12 records in a sub-table, so the level-2 records take 16 bytes (slice_plan: np_max)
    "hot_key.default": E(["k_lc2<false,false,false,false,false,11>"], ["k_lds_count_ovf"], lc2_passed_on="==0"),
    "hot_key_among_600.default": E(["k_lc2<false,false,false,false,false,11>"], ["k_lds_count_ovf"], lc2_passed_on="==0"),
    # yk_lc2_ok: YAKAMD_LC2 = 0 -> every sub-bucket to the tiers behind
    "hot_block_769.lc2_off": E(["k_lds_count_ovf"], ["k_lc2*"], lc2_passed_on=">0"), "hot_block_3000.lc2_off": E(["k_lds_count_ovf"], ["k_lc2*"], lc2_passed_on=">0"),
    "hot_key_among_600.lc2_off": E(["k_lds_count_ovf"], ["k_lc2*"], lc2_passed_on=">0"),
    # fast_admit: a batch costs 65536 * 12 bytes, a second one is over the budget -> a slice per batch; the later ones meet the clustered table (I = true)
    "hot_block_3000.slices": E(["k_lds_count_ovf"], ["k_acc_insert"], early_slices=">0", fast_abandoned="==0"),
    "run_ladder_wrap.slices": E(["k_r2_dsmall", "k_r2_place"], ["k_acc_insert"], early_slices=">0", fast_abandoned="==0", r2_used=">0", r2_refused="==0"),
    "long_prefix.slices": E(["k_r2_dsmall"], ["k_acc_insert"], early_slices=">0", fast_abandoned="==0", r2_refused=">0"),
    # pass_begin: YAKAMD_FAST = 0 -> the accumulator path
    "hot_block_625.fast_off": E(["k_acc_insert"], FAST_ONLY, slices="==0"), "hot_key.fast_off": E(["k_acc_insert"], FAST_ONLY, slices="==0"),
    "one_home_last_392.fast_off": E(["k_acc_insert"], FAST_ONLY, slices="==0"),
    # ---- the cases side by side in sub-tables 500 ... 503 of an ordinary read set: more than 256 sub-tables double in a step, so the doubling's waves
    # come from YAKAMD_R2_DBL (yk_r2_double).  tests/test_adversarial.py replays the four sub-tables' actual streams through the model: none refuses ----
    "mixed.default": E(R2_ONE, ["k_r2_double<5,*", "k_r2_double<6,*"], r2_used=">0", r2_refused="==0"),   # (sub-table 502 alone is large: 16 Ki slots)
    "mixed.sb5": E(["k_r2_dsmall", "k_r2_double<5,false,1>", "k_r2_place"], [], r2_used=">0", r2_refused="==0"),
    "mixed.sb5_seg10": E(["k_r2_double<5,false,1>", "k_r2_ppart"] + R2_SEGMENTED, [], r2_used=">0", r2_refused="==0"),
    "mixed.sb5_dbl61": E(["k_r2_double<6,false,1>"], ["k_r2_double<5,*"], r2_used=">0", r2_refused="==0"),
    "mixed.sb5_dbl52": E(["k_r2_double<5,false,2>"], ["k_r2_double<6,*", "k_r2_double<5,false,1>"], r2_used=">0", r2_refused="==0"),
}
# the count with -b22 of the same file (8 blocks per sub-table, s2 = 0: one sub-bucket): the staged instance holds LC2_FULL_BF = 624 distinct keys (kern_count.inc:550)
ADVERSARIAL_B22 = {
    "hot_block_624": E([LC2_FILTER], ["k_lds_count_ovf"], lc2_passed_on="==0"),
    "hot_block_625": E([LC2_FILTER, "k_lds_count_ovf"], [], lc2_passed_on=">0", ovf_groups=">0"),
}
# pass 2 on the clustered tables, keyed by the row; every case of test_gpu_adversarial.PASS2_CASES runs under each, with -b22 (k = 31) and -b20 (k = 21), in one tally.
# `retained`: both passes on one device image with yakamd_retain_input (the protocol of test_second_pass_counts_the_records_the_first_pass_retained);
# else count_protocol_host, whose count pass feeds the input again (feed_image -> consume_records -> count_records: count_own / count_by_ranges / k_img_count_h)
ADVERSARIAL_PASS2_ROWS = {
    "fused": dict(retained=1), "cnt2_unfused": dict(retained=1, YAKAMD_CNT2_FUSED="0"), "retain2_off": dict(retained=1, YAKAMD_RETAIN2="0"),
    "count_atomics": dict(YAKAMD_COUNT_OWN="0", YAKAMD_COUNT_LDS="0", YAKAMD_COUNT_RNG="0"),
    "ranges_32_slots_no_list": dict(YAKAMD_COUNT_OWN="0", YAKAMD_COUNT_LDS="0", YAKAMD_RNG_LOG="5", YAKAMD_XLIST_CAP="0"),
    "own_lds": dict(YAKAMD_OWN_LDS="18700", YAKAMD_OWN_MAXRB="12"), "own_lds_no_list": dict(YAKAMD_OWN_LDS="18700", YAKAMD_OWN_MAXRB="12", YAKAMD_XLIST_CAP="0"),
}
ADVERSARIAL_PASS2 = {
    # slice_plan: nowb_plan (one slice into an empty table, fewer than 2^12 records per sub-table: kept) -> yakamd_count_retained's first branch
    "fused": E(["k_cnt2_apply"], ["k_cnt2<*"], pass2_fused=">0", pass2_none="==0"),
    "cnt2_unfused": E(["k_cnt2_apply"], [], pass2_recount=">0", pass2_fused="==0"),                    # YAKAMD_CNT2_FUSED = 0: k_cnt2 counts again
    "retain2_off": E([OWN_H], ["k_cnt2*"], pass2_prefix=">0", pass2_none="==0"),                       # slice_retain: the level-1 records; consume_records
    # count_plan: key-owning ranges, LDS ranks and home-slot ranges all refused -> every instance walks its chain with device atomics
    "count_atomics": E(["k_img_count_h"], ["k_img_count_own*", "k_img_count_lds*", "k_img_count_rng*", "k_hpart2*"]),
    # count_by_ranges: ranges of 32 slots; a chain that leaves its range is an exception, and a list of no entries sends them all to the cross sweep
    "ranges_32_slots_no_list": E([RNG, RNGX], ["k_img_count_own*"], rng_sweeps=">0"),
    # count_plan: 18700 B leave room for ~228 keys (yk_count_own_lds): ranges of 64 slots and fewer; the instances whose key sits beyond their
    # home slot's range -- all but a few of a cluster's -- go through the list (k_img_count_h), or with no list through the cross sweep
    "own_lds": E([OWN_H, "k_img_count_h"], [OWN_HX, "k_img_count_rng*", "k_img_count_lds*"], own_sweeps="==0"),
    "own_lds_no_list": E([OWN_H, OWN_HX], ["k_img_count_rng*"], own_sweeps=">0"),
}

# test function -> (module, parametrize argument whose ids key the table, table)
TABLES = {
    "test_every_insert_path_is_exact": ("test_gpu_parity", "env", EVERY_INSERT_PATH),
    "test_replay_variants_on_large_subtables": ("test_gpu_parity", "env", REPLAY_VARIANTS),
    "test_low_complexity_bursts": ("test_gpu_parity", "env", LOW_COMPLEXITY),
    "test_device_batching_is_invisible": ("test_gpu_parity", "env", DEVICE_BATCHING),
    "test_second_pass_counts_the_records_the_first_pass_retained": ("test_gpu_parity", "env", SECOND_PASS_RETAINED),
    "test_seg_sort_pass_of_long_segments": ("test_gpu_parity", None, LONG_SEGMENTS),
    "test_count_pass_over_hashed_records": ("test_gpu_parity", "env", HASHED_RECORDS),
    "test_count_pass_from_the_first_pass_counts": ("test_gpu_pass2_fused", "fused", COUNT_PASS_FROM_FIRST),
    "test_fused_counts_on_every_gather_and_tier": ("test_gpu_pass2_fused", "env", FUSED_GATHER_AND_TIER),
    "test_inc_and_shrink_between_the_passes": ("test_gpu_pass2_fused", "fused", INC_AND_SHRINK),
    "test_sub_buckets_k_lc2_passes_on": ("test_gpu_pass2_fused", None, SUB_BUCKETS_PASSED_ON),
    "test_clustered_tables_are_exact": ("test_gpu_adversarial", "case_row", ADVERSARIAL),
    "test_one_block_at_the_staged_table_bound": ("test_gpu_adversarial", "name", ADVERSARIAL_B22),
    "test_pass2_on_clustered_tables": ("test_gpu_adversarial", "row", ADVERSARIAL_PASS2),
}
