"""Counting and table layout on the clustered inputs of tests/adversarial_util.py: keys of one home slot, runs of chosen lengths, walks across
segment ends, one bloom block, one key tens of thousands of times.  The bytes are the oracle's (and, through tests/golden/adversarial.json, the
reference's) for every option set and under every switch row that sends the table through another consumer of probe chains; the launch tally
says which path ran and whether the streaming replay went through or handed the table back to k_replay (paths_util.ADVERSARIAL: derived
from the model's report and the thresholds in the source by tests/test_adversarial.py, not from a run)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import adversarial_util as A
import paths_util
from conftest import GOLD
from test_adversarial import MIXED_SYNTH, OPTS

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(GOLD, "adversarial.json")))["count"]
_want = {}


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def inputs(oracle, synth):
    """(name, option id) -> (image, the oracle's bytes, the oracle's tot); counted once per module, held to the reference's md5"""
    def get(name, oid):
        if (name, oid) not in _want:
            opt = OPTS[oid]
            img = A.mixed(synth(**MIXED_SYNTH), opt["k"])["img"] if name == "mixed" else A.case(name, opt["k"])["img"]
            want, tot = oracle.count_protocol_mem(img, **opt)
            assert dict(md5=hashlib.md5(want).hexdigest(), size=len(want)) == GOLDEN[name][oid], (name, oid)
            _want[name, oid] = (img, want, tot)
        return _want[name, oid]
    return get


def _set(knob, env):
    for k_, v in env.items():
        knob(k_, v)


CASE_ROWS = sorted(paths_util.ADVERSARIAL)


@pytest.mark.parametrize("case_row", CASE_ROWS, ids=CASE_ROWS)
def test_clustered_tables_are_exact(case_row, ya, inputs, knob):
    """bytes and tot for k31, k31 -b22, k31 -b30 and k21 -b20; the tally of the count without a filter -- the one whose table the model describes --
    against the entry: the kernels of the row ran, and the streaming replay was used or refused as the thresholds say"""
    name, row = case_row.split(".")
    _set(knob, paths_util.ADVERSARIAL_ROWS[row])
    ran = None
    for oid, opt in OPTS.items():
        img, want, wtot = inputs(name, oid)
        if oid == "k31":
            with paths_util.tally(ya.lib()) as ran:
                got, tot = ya.count_protocol_host(img, **opt)
        else:
            got, tot = ya.count_protocol_host(img, **opt)
        assert (got == want, tot) == (True, wtot), (name, row, oid)
    paths_util.hold(ran, paths_util.ADVERSARIAL[case_row], paths_util.names(ya.lib()), case_row)


@pytest.mark.parametrize("name", sorted(paths_util.ADVERSARIAL_B22), ids=sorted(paths_util.ADVERSARIAL_B22))
def test_one_block_at_the_staged_table_bound(name, ya, inputs):
    """624 and 625 distinct keys of one bloom block under -b22: the last sub-bucket k_lc2's staged instance keeps, the first it passes on"""
    img, want, wtot = inputs(name, "k31b22")
    with paths_util.tally(ya.lib()) as ran:
        got, tot = ya.count_protocol_host(img, **OPTS["k31b22"])
    assert (got == want, tot) == (True, wtot)
    paths_util.hold(ran, paths_util.ADVERSARIAL_B22[name], paths_util.names(ya.lib()), name)


# fewer than 2^12 records per sub-table: their level-2 records can be kept; and tables of 32 slots or more with either k: count_plan has no key-owning range
# for a smaller one (hot_block_probes_600 has 4 keys at k = 21) and hands it to k_img_count_lds, which test_gpu_parity's count_kernel_not_applicable covers
PASS2_CASES = ("hot_block_769", "one_home_last_1544", "one_home_mid_392", "segment_mid_12_513")


def _retained_protocol(ya, img, opt):
    """both passes on one device image with yakamd_retain_input, as test_second_pass_counts_the_records_the_first_pass_retained does"""
    L = ya.lib()
    d = L.yakamd_dev_alloc(len(img) + 64)
    assert d and L.yakamd_memcpy_h2d(d, img, len(img)) == 0
    t = ya.Table(opt["k"], 10, 4, opt["bf_shift"])
    try:
        assert L.yakamd_retain_input(t.h, 1) == 0
        t.count_pass(1, [(d, len(img), 0)])
        t.destroy_bf(); t.clear()
        assert L.yakamd_pass_begin(t.h, 0) == 0
        r = L.yakamd_count_retained(t.h)
        assert r in (0, 1)
        if r:
            assert L.yakamd_feed_bases_dev(t.h, d, len(img), 0) == 0
        assert L.yakamd_pass_end(t.h) == 0
        t.shrink(2, 1023)
        return t.dump_bytes(), t.tot
    finally:
        t.close()
        L.yakamd_dev_free(d)


@pytest.mark.parametrize("row", sorted(paths_util.ADVERSARIAL_PASS2), ids=sorted(paths_util.ADVERSARIAL_PASS2))
def test_pass2_on_clustered_tables(row, ya, inputs, knob):
    """the count pass over retained records and over the input again, on tables that are one cluster or one block: k_cnt2_apply, k_cnt2,
    k_img_count_own's slot ranges with their exception lists, the range kernel's, the device atomics"""
    env = dict(paths_util.ADVERSARIAL_PASS2_ROWS[row])
    retained = env.pop("retained", None)
    _set(knob, env)
    with paths_util.tally(ya.lib()) as ran:
        for name in PASS2_CASES:
            for oid in ("k31b22", "k21b20"):
                img, want, wtot = inputs(name, oid)
                got, tot = _retained_protocol(ya, img, OPTS[oid]) if retained else ya.count_protocol_host(img, **OPTS[oid])
                assert (got == want, tot) == (True, wtot), (name, row, oid)
    paths_util.hold(ran, paths_util.ADVERSARIAL_PASS2[row], paths_util.names(ya.lib()), row)
    for name in PASS2_CASES:                                             # (-b30: 2^11 blocks in one sub-bucket, no instance of k_lc2 takes them; bytes alone)
        img, want, wtot = inputs(name, "k31b30")
        got, tot = _retained_protocol(ya, img, OPTS["k31b30"]) if retained else ya.count_protocol_host(img, **OPTS["k31b30"])
        assert (got == want, tot) == (True, wtot), (name, row)


def test_second_pass_on_a_clustered_second_file(ya, oracle):
    """test_second_pass_on_a_different_file's shape: the table of one file, counted on another whose keys sit in the same cluster -- half of
    them stored, half absent, all walking the same chain"""
    a = A.case("one_home_last_1544")
    keys = a["xs"][:1544]
    more = A.Picker(a["sub"], 31, seed=3).same_home(4095, 12, 1544 + 700)[1544:]
    assert not set(more) & set(keys)
    first = A.image([x for x in keys for _ in range(2)], a["sub"], 31)
    second = A.image(keys[::2] * 3 + more + keys[1::4], a["sub"], 31)
    for bf in (22, 30):
        got, tot = ya.count_protocol_host(first, bf_shift=bf, buf2=second)
        want, wtot = oracle.count_protocol_mem(first, bf_shift=bf, buf2=second)
        assert (got == want, tot) == (True, wtot), bf
        assert max(n for n in (len(kc) for _, kc in A.sub_tables(want))) > 300      # the filter let a cluster in, and it survived the shrink


def _kmers(xs, sub, k=31):
    return A.hash64_inv_np(np.asarray(xs, dtype=np.uint64) << np.uint64(10) | np.uint64(sub), (1 << 2 * k) - 1)


@pytest.mark.parametrize("name", ["one_home_last_1544", "hot_block_3000"])
def test_readers_on_a_clustered_table(name, ya, oracle, inputs):
    """after the byte check: the lookup kernel and yak_ch_get on every stored k-mer and on absent ones that home at the start, in the middle and at
    the last slot of the cluster (for the block: absent keys of the block); yakamd_ch_sum of two such tables; the het-mer pairs"""
    from hetmer_util import hetmers as restated_hetmers
    from sum_util import expected_sum_bytes
    from test_gpu_lookup import check
    L, O = ya.lib(), oracle.lib()
    c = A.case(name)
    img, want, _ = inputs(name, "k31")
    stored = sorted(set(c["xs"]))
    pk = A.Picker(c["sub"], 31, seed=99)
    pk.taken.update(stored)
    if name.startswith("one_home"):
        n_keys = len(stored)
        absent = pk.same_home(4095, 12, 3) + pk.one_per_slot([4095, n_keys // 2, n_keys - 2, n_keys - 1, n_keys + 5], 12)
    else:
        absent = pk.same_block(stored[0] & ((1 << A.BLOCK_WIDTH) - 1), A.BLOCK_WIDTH, 40)
    assert not set(absent) & set(stored)
    query = A.image(stored + absent + stored[::7], c["sub"], 31)
    t0, t1 = ya.Table(31, 10, 4, 0), ya.Table(31, 10, 4, 0)
    o = O.yko_count_mem(img, len(img), C.byref(oracle.copt(k=31)), None)
    try:
        t0.count_pass_host(1, img); t1.count_pass_host(1, img)
        assert t0.dump_bytes() == want
        res = check(ya, oracle, t0.h, o, query, 2, 31, 10)
        n_hit = int((res[30::32] > 0).sum())
        assert n_hit == len(stored) + len(stored[::7]) and int((res[30::32] == 0).sum()) == len(absent)
        for x in stored[::5] + absent:
            h = x << 10 | c["sub"]
            assert L.yak_ch_get(t0.h, h) == O.yko_ch_get(o, h) == (-1 if x in absent else min(1023, c["xs"].count(x))), hex(x)
        J, g = t0.hetmers(1)
        occ = {}
        for x in c["xs"]:
            occ[x] = occ.get(x, 0) + 1
        wJ, wg, _ = restated_hetmers(31, _kmers(stored, c["sub"]), np.array([min(1023, occ[x]) for x in stored], dtype=np.int64), 1)
        assert (J, g) == (wJ, wg)
        assert L.yakamd_ch_sum(t0.h, t1.h, 0) == 0, ya._err()
        assert t0.dump_bytes() == expected_sum_bytes(want, want, want)
    finally:
        O.yko_ch_destroy(o)
        t0.close(); t1.close()
