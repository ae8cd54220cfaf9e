"""The launch tally's name table against the expectation tables of paths_util.py.  Host data only: loading the library needs no device.

Every kernel instantiation the library can launch is claimed -- by the `ran` of a table entry, or by a test of another GPU file (OTHER_FILES) --
or stands in UNREACHED with a reason, and only the clock-instrumented variants may stand there.  The tables and the parametrize lists they
describe name the same cases; every name a table uses exists; no launch in yak_amd/csrc goes around the tally."""
import glob
import os
import re
import subprocess
import sys

import pytest

import paths_util
from conftest import ROOT

# instantiations that the path matrices do not run: kernel -> a test (file :: id) of another GPU file that does (as the tally of a whole GPU
# run showed: lookup, table commands, depth, cover, graph, hetmers, hpc, inspect, sum, trio and exchange kernels, and two k_lc2 instances that
# only a second create_new pass into a filled table reaches)
OTHER_FILES = {
    "k_lookup<unsignedshort,false>": "test_gpu_lookup.py::test_lookup_equals_oracle[pass-w2-k5-p14]",
    "k_lookup<uint8_t,false>": "test_gpu_lookup.py::test_lookup_equals_oracle[pass-w1-k21-p10]",
    "k_lookup<uint8_t,true>": "test_gpu_lookup.py::test_lookup_equals_oracle[two_pass_fused-w1-k32-p11]",
    "k_lookup<uint8_t,false,true>": "test_gpu_chkerr.py::test_cli_and_library_equal_golden[default-k21]",
    "k_lookup<uint8_t,true,true>": "test_gpu_chkerr.py::test_cli_and_library_equal_golden[default-k41]",
    "k_qv_reduce": "test_gpu_hpc.py::test_yak_qv_counts_on_a_marked_table",
    "k_tb_reduce": "test_gpu_triobin.py::test_cli_and_library_equal_golden[k21-c1d2]",
    "k_te_runs<true,TeMapLow>": "test_gpu_cover.py::test_intervals_through_the_run_finder[2]",
    "k_te_runs<false,TeMapLow>": "test_gpu_cover.py::test_intervals_through_the_run_finder[2]",
    "k_te_runs<true,TeMapTrio>": "test_gpu_trioeval.py::test_cli_and_library_equal_golden[default-asm.fa-k21]",
    "k_te_runs<false,TeMapTrio>": "test_gpu_trioeval.py::test_cli_and_library_equal_golden[default-asm.fa-k21]",
    "k_te_scan": "test_gpu_cover.py::test_intervals_through_the_run_finder[2]",
    "k_te_keep<true,TeMapLow>": "test_gpu_cover.py::test_intervals_through_the_run_finder[2]",
    "k_te_keep<false,TeMapLow>": "test_gpu_cover.py::test_intervals_through_the_run_finder[2]",
    "k_te_keep<true,TeMapTrio>": "test_gpu_trioeval.py::test_cli_and_library_equal_golden[default-asm.fa-k21]",
    "k_te_keep<false,TeMapTrio>": "test_gpu_trioeval.py::test_cli_and_library_equal_golden[default-asm.fa-k21]",
    "k_te_seq": "test_gpu_trioeval.py::test_cli_and_library_equal_golden[default-asm.fa-k21]",
    "k_sc_reduce": "test_gpu_sexchr.py::test_cli_and_library_equal_golden[k21]",
    "k_kmers": "test_gpu_graph.py::test_ranges_of_sub_tables_glue_together",
    "k_print_sizes": "test_gpu_tablecmds.py::test_print_equals_golden[nb_k15_fa]",
    "k_print<true>": "test_gpu_tablecmds.py::test_print_equals_golden[nb_k15_fa]",
    "k_print<false>": "test_gpu_tablecmds.py::test_print_equals_golden[nb_k15_fa]",
    "k_cover<0>": "test_gpu_cover.py::test_sizes_around_16_a_tile_and_a_workgroup[1]",
    "k_cover<1>": "test_gpu_cover.py::test_masks_on_every_byte_value[1]",
    "k_cover<2>": "test_gpu_cover.py::test_masks_on_every_byte_value[2]",
    "k_extract": "test_gpu_exchange.py::test_extract[1]",
    "k_pack": "test_gpu_exchange.py::test_pack[all_bytes]",
    "k_xpart_wc<2>": "test_gpu_inspect.py::test_joint_equals_numpy[41-reads_bf-asm]",
    "k_xpart<2>": "test_gpu_lookup.py::test_lookup_equals_oracle[two_pass_fused-w1-k32-p11]",
    "k_xpart<1>": "test_gpu_lookup.py::test_lookup_equals_oracle[pass-w2-k5-p14]",
    "k_img_hist": "test_gpu_inspect.py::test_default_text_equals_restatement[21-reads-asm]",
    "k_img_setcnt": "test_gpu_lookup.py::test_lookup_equals_oracle[setcnt0-w2-k15-p13]",
    "k_resize": "test_gpu_lookup.py::test_lookup_equals_oracle[triobin_load-w2-k21-p12]",
    "k_keys_to_hashes": "test_gpu_lookup.py::test_lookup_equals_oracle[merge-w2-k15-p11]",
    "k_img_add_counts<false>": "test_gpu_sum.py::test_sum_bytes_equal_the_restated_merge[21-10-0]",
    "k_img_add_counts<true>": "test_gpu_sum.py::test_sum_bytes_equal_the_restated_merge[41-10-0]",
    "k_lc2<false,true,false,false,false,11>": "test_gpu_lookup.py::test_lookup_equals_oracle[triobin_load-w2-k21-p12]",
    "k_lc2<true,true,false,false,true,10>": "test_gpu_api.py::test_insert_list_sequences[21]",
    "k_bf_rebuild": "test_gpu_api.py::test_filter_survives_a_pass_that_kept_it_in_lds[filter_rebuilt_from_retained_records]",
    "k_inspect<false,false>": "test_gpu_inspect.py::test_joint_equals_numpy[21-reads-asm]",
    "k_inspect<true,true>": "test_gpu_inspect.py::test_joint_equals_numpy[41-reads-asm]",
    "k_inspect<true,false>": "test_gpu_inspect.py::test_joint_equals_numpy[21-reads-asm]",
    "k_dp_short": "test_gpu_depth.py::test_reduce_small_windows[0]",
    "k_dp_long": "test_gpu_depth.py::test_reduce_small_windows[0]",
    "k_dp_finish": "test_gpu_depth.py::test_reduce_small_windows[0]",
    "k_hetmer<HM_TALLY>": "test_gpu_hetmers.py::test_tables_equal_restatement[1-planted_k31_p10]",
    "k_hetmer<HM_COUNT>": "test_gpu_hetmers.py::test_tables_equal_restatement[1-planted_k31_p10]",
    "k_hetmer<HM_WRITE>": "test_gpu_hetmers.py::test_tables_equal_restatement[1-planted_k31_p10]",
    "k_graph_rank": "test_gpu_graph.py::test_tables_equal_restatement[1-planted_k31_p10]",
    "k_graph_edges<8>": "test_gpu_graph.py::test_both_probe_schedules_give_the_same",
    "k_graph_edges<4>": "test_gpu_graph.py::test_tables_equal_restatement[1-planted_k31_p10]",
    "k_graph_link<GR_COUNT>": "test_gpu_graph.py::test_tables_equal_restatement[1-planted_k31_p10]",
    "k_graph_link<GR_EMIT>": "test_gpu_graph.py::test_tables_equal_restatement[1-planted_k31_p10]",
    "k_hpc_count<HpPacked>": "test_gpu_hpc.py::test_compaction_of_random_images[1]",
    "k_hpc_count<HpAscii>": "test_gpu_hpc.py::test_compaction_of_random_images[1]",
    "k_hpc_scatter<HpPacked>": "test_gpu_hpc.py::test_compaction_of_random_images[1]",
    "k_hpc_scatter<HpAscii>": "test_gpu_hpc.py::test_compaction_of_random_images[1]",
    "k_hpc_remap": "test_gpu_hpc.py::test_compaction_of_random_images[1]",
}

# kernel -> why no test launches it.  Only the clock-instrumented variants (selected by YAKAMD_DBG / YAKAMD_VERBOSE > 1, timing aids) may be here
UNREACHED = {}
for _i in ("false", "true"):
    for _r8 in ("true", "false"):
        for _c in ("10", "11"):
            UNREACHED["k_lc2<false,%s,true,%s,false,%s>" % (_i, _r8, _c)] = "Pf = true: the phase clocks of YAKAMD_DBG & 128"
        UNREACHED["k_lc2<true,%s,true,%s,true,10>" % (_i, _r8)] = "Pf = true: the phase clocks of YAKAMD_DBG & 128"
UNREACHED["k_lc2<true,false,true,true,false,10>"] = "Pf = true: the phase clocks of YAKAMD_DBG & 128"
for _nw in ("16", "5", "6"):
    UNREACHED["k_r2_double<%s,true,1>" % _nw] = "PROF = true: the phase clocks of YAKAMD_VERBOSE > 1"


def _clock_variant(name):
    m = re.match(r"k_lc2<(\w+),(\w+),(\w+),", name)
    if m:
        return m.group(3) == "true"
    m = re.match(r"k_r2_double<(\d+),(\w+),", name)
    return bool(m) and m.group(2) == "true"


@pytest.fixture(scope="module")
def all_names():
    import yak_amd
    return paths_util.names(yak_amd.lib())


def _entries():
    for fn, (mod, arg, table) in paths_util.TABLES.items():
        for case, e in table.items():
            yield fn, mod, case, e


def test_names_are_unique_and_listed_without_a_device(all_names):
    assert len(all_names) == len(set(all_names)) and len(all_names) > 150
    assert "k_part2_wc8<false,7>" in all_names and "event:rank_refused" in all_names
    assert not [n for n in all_names if " " in n or "(" in n]


def test_every_name_a_table_uses_exists(all_names):
    bad = []
    for fn, mod, case, e in _entries():
        for n in e["ran"]:
            if n not in all_names or n.startswith("event:"):
                bad.append((fn, case, n))
        for pat in e["not_ran"]:
            if not [n for n in paths_util.expand(pat, all_names) if n in all_names]:
                bad.append((fn, case, pat))
        for ev, rel in e["events"].items():
            if "event:" + ev not in all_names or rel not in (">0", "==0"):
                bad.append((fn, case, ev, rel))
        if not (e["ran"] or e["not_ran"] or e["events"]):
            bad.append((fn, case, "an entry with nothing to show"))
        clash = set(e["ran"]) & {n for pat in e["not_ran"] for n in paths_util.expand(pat, all_names)}
        if clash:
            bad.append((fn, case, "both ran and not_ran", sorted(clash)))
    assert not bad, bad


def test_tables_and_parametrize_lists_name_the_same_cases():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import importlib
    for fn, (mod, arg, table) in paths_util.TABLES.items():
        f = getattr(importlib.import_module(mod), fn)
        if arg is None:
            assert list(table) == [""], fn
            continue
        marks = [m for m in getattr(f, "pytestmark", []) if m.name == "parametrize" and m.args[0] == arg]
        assert len(marks) == 1, (fn, arg)
        ids = marks[0].kwargs["ids"]
        assert len(ids) == len(marks[0].args[1]) == len(set(ids)), fn
        cases = {c.split("-")[-1] for c in table}                # (an entry for one combination alone is keyed by the whole id)
        assert sorted(ids) == sorted(cases), (fn, sorted(set(ids) ^ cases))


def test_every_instantiation_is_claimed(all_names):
    kernels = [n for n in all_names if not n.startswith("event:")]
    claimed = {n for _, _, _, e in _entries() for n in e["ran"]}
    both = sorted((claimed | set(OTHER_FILES)) & set(UNREACHED))
    assert not both, both
    nobody = [n for n in kernels if n not in claimed and n not in OTHER_FILES and n not in UNREACHED]
    assert not nobody, nobody
    stale = [n for n in list(OTHER_FILES) + list(UNREACHED) if n not in kernels]
    assert not stale, stale
    assert not [n for n in UNREACHED if not _clock_variant(n)], "only the clock-instrumented variants may go unreached"
    used = {"event:" + ev for _, _, _, e in _entries() for ev in e["events"]}
    assert not [n for n in all_names if n.startswith("event:") and n not in used]


def test_the_tests_of_other_files_exist():
    files = sorted({v.split("::")[0] for v in OTHER_FILES.values()})
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + [os.path.join("tests", f) for f in files],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    have = {ln.strip().split("tests/", 1)[-1] for ln in r.stdout.decode().splitlines() if "::" in ln}
    missing = sorted({v for v in OTHER_FILES.values() if v not in have})
    assert not missing, (missing, r.stdout.decode()[-2000:])


def test_no_launch_goes_around_the_tally():
    word = "hipLaunchKernelGGL"
    hits = []
    for path in sorted(glob.glob(os.path.join(ROOT, "yak_amd", "csrc", "*"))):
        for i, ln in enumerate(open(path, errors="replace").read().splitlines(), 1):
            if word in ln or "<<<" in ln or "hipModuleLaunchKernel" in ln or "hipExtLaunch" in ln:
                hits.append((os.path.basename(path), i))
    assert [h[0] for h in hits] == ["tally.h"], hits           # the macro's definition, once
    src = open(os.path.join(ROOT, "yak_amd", "csrc", "tally.h")).read()
    at = src.index(word)
    assert "#define YK_LAUNCH(" in src[:at] and src.rindex("#define", 0, at) == src.index("#define YK_LAUNCH(")
