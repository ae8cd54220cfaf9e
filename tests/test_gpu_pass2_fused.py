"""The count pass of a filtered count (reference main.c:53-57) over the records the first pass retained by sub-bucket: k_lc2 (and the
global-scratch tier behind it) hands out, next to every key it selects, how often the key occurs in its sub-bucket's records, and the count
pass only adds those (k_cnt2_apply) instead of reading every record again (k_cnt2, still there under YAKAMD_CNT2_FUSED=0).  Both ways give
the oracle's bytes, and the stat `pass2_path` says which one ran."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import paths_util
from conftest import ROOT

pytestmark = pytest.mark.gpu

FUSED, RECOUNT, NONE = 1, 2, 0


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    L = yak_amd.lib()
    assert L.yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


def _keys_of(oracle, o, pre=10):
    """the hashes (as yak_ch_inc takes them) of every key of an oracle table, from its .yak image"""
    d = oracle.dump_bytes(o)
    out, off = [], 16
    for p in range(1 << pre):
        _, n = struct.unpack_from("<II", d, off)
        off += 8
        for e in struct.unpack_from("<%dQ" % n, d, off):
            out.append((e >> 10) << pre | p)
        off += 8 * n
    return out


def _hold(ya, ran, table, request=None):
    """the launch tally of a _protocol run against the entry of the case (tests/paths_util.py)"""
    case = [p for p in request.node.callspec.id.split("-") if p in table] if request is not None else [""]
    assert len(case) == 1
    paths_util.hold(ran, table[case[0]], paths_util.names(ya.lib()), case[0])


def _protocol(ya, oracle, img, opt, img2=None, between=None, ran=None):
    """both passes on the device (the first one retaining its records) and in the oracle; `between(inc, shrink)` runs between the passes on
    both tables.  -> (device bytes, device tot, oracle bytes, oracle tot, stats of the device's count pass); ran: a dict that takes the launch
    tally of the device's part"""
    with paths_util.tally(ya.lib()) as got:
        out = _protocol_body(ya, oracle, img, opt, img2, between)
    if ran is not None:
        ran.update(got)
    return out


def _protocol_body(ya, oracle, img, opt, img2, between):
    L, O = ya.lib(), oracle.lib()
    O.yko_ch_inc.restype = C.c_int; O.yko_ch_inc.argtypes = [C.POINTER(oracle.Ch), C.c_uint64]
    k, nh, bf = opt["k"], opt.get("n_hash", 4), opt["bf_shift"]
    oc = oracle.copt(k, 10, nh, bf)
    o = O.yko_count_mem(img, len(img), C.byref(oc), None)
    O.yko_ch_destroy_bf(o); O.yko_ch_clear(o)
    bufs = [img] + ([img2] if img2 is not None else [])
    d = [L.yakamd_dev_alloc(len(b) + 64) for b in bufs]
    for p, b in zip(d, bufs):
        assert L.yakamd_memcpy_h2d(p, b, len(b)) == 0
    t = ya.Table(k, 10, nh, bf)
    try:
        assert L.yakamd_retain_input(t.h, 1) == 0
        t.count_pass(1, [(d[0], len(img), 0)])
        assert L.yakamd_retained_instances(t.h) > 0
        t.destroy_bf(); t.clear()
        if between:
            keys = _keys_of(oracle, o)

            def inc(x):
                assert L.yak_ch_inc(t.h, x) == O.yko_ch_inc(o, x)

            def shrink(lo, hi):
                t.shrink(lo, hi); O.yko_ch_shrink(o, lo, hi)
            between(keys, inc, shrink)
        second = img2 if img2 is not None else img
        t.count_pass(0, [(d[-1], len(second), 0)], same_input=img2 is None)
        st = t.stats()
        assert L.yakamd_retained_instances(t.h) == 0
        o = O.yko_count_mem(second, len(second), C.byref(oc), o)
        O.yko_ch_shrink(o, 2, 1023); t.shrink(2, 1023)
        return t.dump_bytes(), t.tot, oracle.dump_bytes(o), o.contents.tot, st
    finally:
        t.close(); O.yko_ch_destroy(o)
        for p in d:
            L.yakamd_dev_free(p)


def _repeats(synth):
    """seeded reads + one poly-A run: a key (~2 270 instances) beyond both the count field's clamp (0x800) and the 1023 cap.  (Not much more:
    the records of one sub-table must stay below 2^12 here, or the level-2 records are 16 bytes and pass 1 keeps its level-1 records instead)"""
    return synth(9000, g=40000, s=19) + b"A" * 2300 + b"\n"


INPUTS = {"reads": lambda synth: synth(9000, g=40000, s=19), "repeats": _repeats}
OPTS = [dict(k=31, bf_shift=24), dict(k=21, bf_shift=20), dict(k=31, bf_shift=22, n_hash=7)]


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "recount"])
@pytest.mark.parametrize("opt", OPTS, ids=["k31b24", "k21b20", "k31b22H7"])
@pytest.mark.parametrize("inp", sorted(INPUTS))
def test_count_pass_from_the_first_pass_counts(inp, opt, fused, ya, oracle, synth, knob, request):
    knob("YAKAMD_CNT2_FUSED", fused)
    ran = {}
    got, tot, want, wtot, st = _protocol(ya, oracle, INPUTS[inp](synth), opt, ran=ran)
    assert st["pass2_path"] == (FUSED if fused else RECOUNT)
    assert (got, tot) == (want, wtot)
    _hold(ya, ran, paths_util.COUNT_PASS_FROM_FIRST, request)


@pytest.mark.parametrize("env", [dict(YAKAMD_LC_FLAT="1"), dict(YAKAMD_LC_FLAT="0"), dict(YAKAMD_TSORT="1"), dict(YAKAMD_LC2="0"),
                                 dict(YAKAMD_LC2_NOSTAGE="0"), dict(YAKAMD_BF_DEFER="0")],
                         ids=["flat_gather", "compact_gather", "gather_to_pairs", "all_sub_buckets_to_the_scratch_tier", "filter_stage", "filter_written"])
def test_fused_counts_on_every_gather_and_tier(env, ya, oracle, synth, knob, request):
    """the flat gather (k_lc_gather) and the per-sub-table one (k_lc_compact), into arrays or into {key, time} pairs for the sort, carry the
    counts in the order of the key list; the global-scratch tier (lc_body) emits them as k_lc2 does"""
    for k_, v in env.items():
        knob(k_, v)
    ran = {}
    got, tot, want, wtot, st = _protocol(ya, oracle, _repeats(synth), dict(k=31, bf_shift=24), ran=ran)
    assert st["pass2_path"] == FUSED
    assert (got, tot) == (want, wtot)
    _hold(ya, ran, paths_util.FUSED_GATHER_AND_TIER, request)


def test_sub_buckets_k_lc2_passes_on(ya, oracle, synth, knob, capfd):
    """a thin background of reads (nearly every k-mer once) makes sub-buckets with more distinct k-mers than k_lc2's LDS table holds: those go
    to the tier behind it, which counts them as well, in the same pass as the sub-buckets k_lc2 keeps"""
    knob("YAKAMD_VERBOSE", 1)
    img = synth(20000, g=20000000, s=3) + synth(9000, g=40000, s=19, first=50000)
    ran = {}
    got, tot, want, wtot, st = _protocol(ya, oracle, img, dict(k=31, bf_shift=24), ran=ran)
    err = capfd.readouterr().err
    m = re.search(r"k_lc2: [0-9.]+ ms, (\d+) of (\d+) sub-buckets passed on", err)
    assert m and int(m.group(1)) > 0, err[-2000:]
    assert st["pass2_path"] == FUSED
    assert (got, tot) == (want, wtot)
    assert ran.get("event:lc2_passed_on", 0) == int(m.group(1))      # the event counts what the line reports
    _hold(ya, ran, paths_util.SUB_BUCKETS_PASSED_ON)


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "recount"])
def test_inc_and_shrink_between_the_passes(fused, ya, oracle, synth, knob, request):
    """counts set between the passes (yak_ch_inc) stay under the count pass's saturating add; keys a shrink removed are not found by it"""
    knob("YAKAMD_CNT2_FUSED", fused)

    def between(keys, inc, shrink):
        for x in keys[::7]:
            inc(x)
        for _ in range(40):
            inc(keys[3])
        shrink(1, 1023)
    ran = {}
    got, tot, want, wtot, st = _protocol(ya, oracle, _repeats(synth), dict(k=31, bf_shift=24), between=between, ran=ran)
    assert st["pass2_path"] == (FUSED if fused else RECOUNT)
    assert (got, tot) == (want, wtot)
    _hold(ya, ran, paths_util.INC_AND_SHRINK, request)


def test_count_pass_over_another_input_reads_it(ya, oracle, synth):
    """what the first pass kept is of no use for a second input: that pass reads its own"""
    a, b = synth(9000, g=40000, s=19), synth(6000, g=40000, s=19, e=0.02, first=100000)
    got, tot, want, wtot, st = _protocol(ya, oracle, a, dict(k=31, bf_shift=24), img2=b)
    assert st["pass2_path"] == NONE
    assert (got, tot) == (want, wtot)


def test_cli_takes_the_counts_of_the_first_pass(ya, tmp_path):
    """yak-amd count -b on one file: the count pass applies the first pass's counts (verbose line); on two files it reads the second;
    -X YAKAMD_CNT2_FUSED=0 recounts.  The bytes are the oracle CLI's every time"""
    fq, fq2 = str(tmp_path / "r.fq"), str(tmp_path / "r2.fq")
    yam, yko, syn = (os.path.join(ROOT, *p_) for p_ in (("yak_amd", "yak-amd"), ("oracle", "yko"), ("tools", "yaksynth")))
    subprocess.check_call([syn, "-n", "8000", "-g", "40000", "-s", "8", "-o", fq])
    subprocess.check_call([syn, "-n", "5000", "-g", "40000", "-s", "8", "-o", fq2])
    a, b = str(tmp_path / "a.yak"), str(tmp_path / "b.yak")
    env = dict(os.environ, YAKAMD_VERBOSE="1")
    for files, extra, line in (([fq], [], "the counts of the pass before applied"), ([fq], ["-X", "YAKAMD_CNT2_FUSED=0"], "k_cnt2 over the retained"),
                               ([fq, fq2], [], None)):
        r = subprocess.run([yam, "count", "-k31", "-b24"] + extra + ["-o", a] + files, check=True, stderr=subprocess.PIPE, env=env, timeout=600)
        subprocess.run([yko, "count", "-k31", "-b24", "-o", b] + files, check=True, stderr=subprocess.DEVNULL, timeout=600)
        assert open(a, "rb").read() == open(b, "rb").read()
        err = r.stderr.decode(errors="replace")
        if line:
            assert "[yak_amd] count pass: " + line in err
        else:
            assert "[yak_amd] count pass: " not in err
