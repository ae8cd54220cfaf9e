"""The clustered inputs of tests/adversarial_util.py are what they claim to be (no GPU): every property a case is built for is read off the
put-by-put model, the model's layout is the oracle's dump, the oracle's dump is what the reference wrote for the same image
(tests/golden/adversarial.json, by tests/gen_golden_adversarial.py), and the refusals paths_util.ADVERSARIAL expects are the ones the thresholds of
kern_replay2.inc give on the model's report."""
import hashlib
import json
import os
import random

import pytest

import adversarial_util as A
import paths_util
from conftest import GOLD

OPTS = {"k31": dict(k=31), "k31b22": dict(k=31, bf_shift=22), "k31b30": dict(k=31, bf_shift=30), "k21b20": dict(k=21, bf_shift=20)}
NAMES = sorted(A.CASES)
_models = {}
MIXED_SYNTH = dict(n=8000, g=40000, s=21)


@pytest.fixture(scope="module")
def mixed_case(synth, oracle):
    """adversarial_util.mixed on a small read set, and the model's replay of what really streams into its four sub-tables"""
    c = A.mixed(synth(**MIXED_SYNTH))
    lists = oracle.extract_lists(31, 10, c["img"])
    c["streams"] = {p: [int(h) >> 10 for h in lists[p]] for p in A.MIXED_SUBS}
    c["models"] = {p: A.Model().replay(xs) for p, xs in c["streams"].items()}
    return c


def model(name):
    if name not in _models:
        c = A.case(name)
        _models[name] = [(sub, A.Model().replay(xs)) for sub, xs in c.get("per_sub", [(c["sub"], c["xs"])])]
    return _models[name]


def test_the_inversions():
    from tablecmds_util import hash64_inv
    rnd = random.Random(1)
    for k in (31, 21, 15):
        m = (1 << 2 * k) - 1
        xs = [rnd.getrandbits(2 * k) for _ in range(500)]
        assert [int(v) for v in A.hash64_inv_np(xs, m)] == [hash64_inv(x, m) for x in xs]
    for bits in (2, 9, 14, 16):
        for slot in (0, (1 << bits) - 1, 5 % (1 << bits)):
            for r in (0, 1, (1 << (32 - bits)) - 1):
                lo = A.lo_for(slot, bits, r)
                assert [A.h2b(lo, bits - d) for d in range(bits - 1)] == [slot >> d for d in range(bits - 1)]


def test_the_shortened_probes_are_the_literal_ones():
    """Model (union-find for the first free slot, a dictionary for an existing key) against Kh, the literal put / resize, on uniform keys, on keys of a
    few home slots with repeats, and on the smallest clustered cases"""
    rnd = random.Random(2)
    seqs = []
    for t in range(40):
        mask = [0xFFFFFFFFFF, 0xFF000000FF, 0xF00000000F, 0xFF0000000][t % 4]
        keys = [rnd.getrandbits(40) & mask for _ in range(rnd.choice([5, 40, 300, 700]))]
        seqs.append(keys + keys[:len(keys) // 3])
    seqs += [A.case(n)["xs"] for n in ("one_home_zero_200", "one_home_mid_200", "one_home_last_392", "lastput_growth", "hot_block_600", "segment_end_12_300")]
    for xs in seqs:
        a, b = A.Kh(), A.Model()
        for x in xs:
            a.put(x); b.put(x)
        assert a.layout() == b.layout() and a.count == b.count


@pytest.mark.parametrize("name", NAMES)
def test_model_layout_is_the_oracle_dump(name, oracle):
    """without a filter the table is the put sequence's: capacity, slot order and counts of the case's sub-tables as the model has them, nothing
    anywhere else"""
    c = A.case(name)
    subs = A.sub_tables(oracle.count_protocol_mem(c["img"], k=31)[0])
    mine = dict(model(name))
    seqs = dict(c.get("per_sub", [(c["sub"], c["xs"])]))
    lists = oracle.extract_lists(31, 10, c["img"])                     # the image streams the put sequence it was built from, and nothing else
    assert {p: [int(h) >> 10 for h in lists[p]] for p in seqs} == seqs and sum(len(x) for x in lists) == sum(len(x) for x in seqs.values())
    for p, (cap, keys) in enumerate(subs):
        if p not in mine:
            assert (cap, keys) == (0, []), p
            continue
        m = mine[p]
        occ = {}
        for x in seqs[p]:
            occ[x] = occ.get(x, 0) + 1
        assert cap == m.n_buckets()
        assert keys == [x << 10 | min(occ[x], 1023) for x in m.layout() if x is not None]


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("one_home") or n == "lastput_growth"])
def test_one_home_is_one_cluster_at_every_capacity(name):
    c, m = A.case(name), model(name)[0][1]
    where, n_keys = c["claims"].get("where", "last"), c["claims"]["cluster"]
    assert m.n_buckets() == 1 << c["claims"]["final_bits"] and m.count == n_keys
    assert len(m.doublings) == c["claims"]["final_bits"] - 2
    for d in m.doublings:
        n, cnt = d["n"], d["count"]
        assert cnt == n * 3 // 4 and sum(ln for _, ln in d["runs"]) == cnt
        assert d["walk"] == cnt - 1                                   # the last key put walked past all the others
        if where == "zero":
            assert d["runs"] == [(0, cnt)] and not d["wraps"]
        elif where == "mid":
            assert d["runs"] == [(0, cnt - n // 2), (n // 2, n // 2)] and d["wraps"] and d["tail_far"] == -1
        else:
            assert d["runs"] == [(0, cnt - 1), (n - 1, 1)] and d["wraps"] and (d["tail"], d["head"]) == (1, cnt - 1)
            assert d["tail_far"] in (cnt - 2, cnt - 3)                    # ... and goes around the new table's end as far again (lastput_growth's home is the last slot but one of 1024)
        assert d["cover"] == [F for F in (8, 16, 32, 64, 128, 256, 512, 1024) if (where == "mid" and F == n // 2) or 2 * F <= (cnt - n // 2 if where == "mid" else cnt - (where == "last"))]
    if name == "lastput_growth":                                       # 384 keys in 512 slots would not have grown: the trailing put-call did it
        assert m.n_buckets() == 1024 and m.count == 384 and 10 not in m.stages
    else:
        assert len(m.stages[m.bits]["new"]) == 8                       # 8 keys behind the last doubling, then put-calls on existing keys that grow nothing


@pytest.mark.parametrize("variant", ["plain", "over", "wrap", "tail192", "tail193"])
def test_run_ladder_holds_its_runs(variant):
    name = "run_ladder_" + variant
    c, m = A.case(name), model(name)[0][1]
    d = m.doublings[-1]
    assert m.n_buckets() == 16384 and d["n"] == 8192 and d["count"] == 6144
    lens = [ln for _, ln in d["runs"]]
    for ln in c["claims"]["ladder"]:
        assert lens.count(ln) >= 1, ln
    assert max(lens) == (513 if variant == "over" else 512)
    assert [x for x in lens if x > 193 and x not in (236, 512, 513)] == []   # nothing else is long (236: the head of `wrap`, below)
    if variant == "wrap":
        assert d["wraps"] and d["tail"] == 100 and d["head"] >= 93 and d["tail_far"] >= 0      # keys of the last run do go around the end
        assert d["head"] == 236 and d["tail_far"] < 2 * 128 + 2          # ... and stay inside the `wrap` slots r2_wave_run looks at
    elif variant in ("tail192", "tail193"):
        assert d["wraps"] and (d["tail"], d["head"]) == (int(variant[4:]), 5)
    else:
        assert d["tail"] <= 8 and d["first"] <= 8
    assert A.refusal_codes(m) == ({6} if variant == "over" else set())


def test_long_prefix():
    m = model("long_prefix")[0][1]
    d = m.doublings[-1]
    assert d["n"] == 8192 and d["first"] == 4101 and d["first"] + 1 > A.R2_BASE_MAX and d["walk"] <= 2
    assert 2048 in d["cover"] and A.refusal_codes(m) == {1}


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("segment_")])
def test_segment_edges_spill_as_far_as_they_say(name):
    c, m = A.case(name), model(name)[0][1]
    bits, cluster, B = c["claims"]["final_bits"], c["claims"]["cluster"], c["claims"]["boundary"]
    n = 1 << bits
    assert m.n_buckets() == n
    st = m.stages[bits]
    edge = st["new"][-cluster:]
    assert all(home == (B - 1) % n for home, _, _ in edge)
    assert [w for _, w, _ in edge] == list(range(cluster))               # one at its home slot, the others 0 ... cluster - 2 slots into the next segment
    for seg_log in ([14] if bits == 15 else []) + [10]:
        head = min(A.R2_HEAD, (1 << seg_log) // 2)
        spills, fail5 = A.place_outcome(st, bits, seg_log)
        assert spills >= cluster - 1
        if bits - seg_log == 1 or cluster <= head:                       # (smaller segments: the filler's own walks may spill too; they are short)
            assert fail5 == (cluster - 2 >= head), (seg_log, spills)


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("hot_block")])
def test_hot_block_is_one_block(name):
    c = A.case(name)
    keys = sorted(set(c["xs"]))
    width = c["claims"]["width"]
    assert len(keys) == c["claims"]["block_keys"] and len({x & ((1 << width) - 1) for x in keys}) == 1
    occ = [c["xs"].count(x) for x in keys[:50]]
    assert set(occ) <= {2, 3}
    for bf_shift in (20, 22, 30):                                        # one block, and with `probes` one pair of probe fields (bbf.c:27-30)
        nb = bf_shift - 10
        assert len({x & ((1 << (nb - 9)) - 1) for x in keys}) == 1
        if "probes" in name:
            assert len({(x >> (nb - 9) & 511, x >> nb & 511) for x in keys}) == 1
    if "probes" not in name and len(keys) >= 600:                        # the home slots are uniform: no slot of 1024 is the home of more than a handful
        homes = [A.h2b(x & A.M32, 10) for x in keys]
        assert max(homes.count(h) for h in set(homes)) <= 8 + len(keys) // 256


def test_hot_key_counts():
    for name in ("hot_key", "hot_key_among_600"):
        c = A.case(name)
        for (sub, xs), cnt in zip(c["per_sub"], c["claims"]["counts"]):
            assert xs.count(xs[0]) == cnt and len(set(xs)) == 1 + c["claims"]["others"]
            if c["claims"]["others"]:
                at = [i for i, x in enumerate(xs) if x != xs[0]]
                assert at[0] > 0 and sum(1 for i in at if xs[i + 1:i + 2] == [xs[0]]) >= len(at) // 2   # the others come in between the occurrences


def test_the_fail_codes_the_cases_reach():
    """1, 5, 6 and 7 are each raised by some case under some row; 4, 8, 9 and 10 by none (adversarial_util.refusal_codes says why)"""
    got = set()
    for name in NAMES:
        m = model(name)[0][1]
        for sb, seg in ((13, 14), (5, 14), (5, 10)):
            got |= A.refusal_codes(m, sb, seg)
    assert got == {1, 5, 6, 7}


def test_the_table_expects_the_refusals_the_thresholds_give(mixed_case):
    for key, e in paths_util.ADVERSARIAL.items():
        name, row = key.split(".")
        env = paths_util.ADVERSARIAL_ROWS[row]
        if env.get("YAKAMD_REPLAY2") == "0":
            assert e["events"] == dict(r2_used="==0", r2_refused="==0")
            continue
        if name == "mixed":                                              # (the ordinary sub-tables around: 512 slots, large from SB = 5 on)
            sb = int(env.get("YAKAMD_R2_SMALL_BITS", 13))
            assert all(not A.refusal_codes(m, sb, int(env.get("YAKAMD_R2_SEG_LOG", 14))) for m in mixed_case["models"].values())
            assert e["events"] == dict(r2_used=">0" if any(m.n_buckets() > 1 << sb for m in mixed_case["models"].values()) else "==0", r2_refused="==0")
            continue
        m = model(name)[0][1]
        sb, seg = int(env.get("YAKAMD_R2_SMALL_BITS", 13)), int(env.get("YAKAMD_R2_SEG_LOG", 14))
        codes = A.refusal_codes(m, sb, seg)
        large = m.n_buckets() > 1 << sb
        want = dict(r2_refused=">0" if codes else "==0", r2_used=">0" if large and not codes else "==0")
        if row in ("default", "sb5", "sb5_seg10", "sb5_prefix1024") and not name.startswith("hot_"):
            assert {k_: e["events"].get(k_) for k_ in want} == want, (name, row, codes)
        else:                                                            # rows about something else: what they do say about the replay must still be so
            assert all(want[k_] == v for k_, v in e["events"].items() if k_ in want), (name, row, codes)


def test_mixed_keeps_its_clusters(mixed_case, oracle):
    """the read set adds a few hundred keys to each of the four sub-tables; the clusters are still there, and the model still has the oracle's layout"""
    subs = A.sub_tables(oracle.count_protocol_mem(mixed_case["img"], k=31)[0])
    for p, m in mixed_case["models"].items():
        assert subs[p][0] == m.n_buckets() and [kc >> 10 for kc in subs[p][1]] == [x for x in m.layout() if x is not None]
    m = mixed_case["models"]
    assert m[500].doublings[-1]["first"] >= 128                        # (the reads' own keys grow the tables earlier: less of a cluster is in by a doubling)
    d = m[502].doublings[-1]
    assert m[502].n_buckets() == 16384 and max(ln for _, ln in d["runs"]) >= 256 and d["tail"] >= 32 and d["tail_far"] >= 0
    assert max(w for _, w, _ in m[503].stages[12]["new"]) >= 298
    assert sum(1 for cap, _ in subs if cap >= 64) > 900                # ... among ordinary neighbours that grow as well


def md5_size(data):
    return dict(md5=hashlib.md5(data).hexdigest(), size=len(data))


@pytest.mark.parametrize("name", NAMES + ["mixed"])
def test_oracle_dump_is_the_reference_dump(name, oracle, synth):
    gold = json.load(open(os.path.join(GOLD, "adversarial.json")))["count"]
    for oid, opt in OPTS.items():
        img = A.mixed(synth(**MIXED_SYNTH), opt["k"])["img"] if name == "mixed" else A.case(name, opt["k"])["img"]
        assert md5_size(oracle.count_protocol_mem(img, **opt)[0]) == gold[name][oid], (name, oid)
