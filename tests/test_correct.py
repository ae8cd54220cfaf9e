"""The correction of substitution errors (`yak-amd correct`) without a GPU: the two restatements of tests/correct_util.py -- flat,
in numpy, on the image and a count array made from a .yak dump of the oracle's, and read by read on strings -- held to each other, fix records,
tallies and both texts, on tiny random tables and on hand-derived cases whose S and X lines are written out here, with the invariants
include/yak_amd_correct.h promises (n_weak_after against a fresh lookup of the corrected reads, idempotence, disjoint runs); a planted genome whose
reads must all come back as their sources.  Last, libyak_amd_correct.so itself: its exports, its own launch tally, the sizes of its structs, its
NEEDED entries, its refusals, which need no device, and the CLI's usage."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import correct_util as K
from conftest import ROOT

# k = 5, min_cnt = 2.  G twice and G2 twice: G2 is G with A for T at base 20, so both alleles of that site are solid.  Found by search so that the
# 26 5-mers of G are distinct and every case below meets no chance hit; tests/test_correct_model.py and tests/test_gpu_correct.py share them
G = "TGCCTGGTACATCCGCGAAATGCAGTCAAA"
G2 = G[:20] + "A" + G[21:]
HAND_TABLE = [G, G, G2, G2]
NXT = {"A": "C", "C": "G", "G": "T", "T": "A"}


def mut(r, *ps):
    """the read with the next base of ACGT at each of the places"""
    r = list(r)
    for p in ps:
        r[p] = NXT[r[p]]
    return "".join(r)


# name -> (the read, min_run, the read afterwards, the S line's numbers behind the length, the X lines' fields behind the name)
CASES = {
    # base 12, G for C: the five 5-mers ending at 12 .. 16 hold it, a run of k; only C makes them all solid
    "interior": (mut(G, 12), 1, G, "26\t5\t1\t1\t0\t0\t0", ["12\tG\tC\t5"]),
    # base 0 lies in the first 5-mer alone: the run is [4, 5), nothing ends at 3, p = en - k = 0
    "first_base": (mut(G, 0), 1, G, "26\t1\t1\t1\t0\t0\t0", ["0\tA\tT\t1"]),
    # base 29 lies in the last 5-mer alone: the run is [29, 30), nothing ends at 30, p = st
    "last_base": (mut(G, 29), 1, G, "26\t1\t1\t1\t0\t0\t0", ["29\tC\tA\t1"]),
    # base k - 2 = 3 lies in the 5-mers ending at 4 .. 7: the run [4, 8) of k - 1 at the front, p = 8 - 5
    "base_k_minus_2": (mut(G, 3), 1, G, "26\t4\t1\t1\t0\t0\t0", ["3\tG\tC\t4"]),
    # bases 6 and 12, k bases between them: runs [6, 11) and [12, 17), the 5-mer ending at 11 is solid and parts them; both fixed
    "two_errors_k_between": (mut(G, 6, 12), 1, G, "26\t10\t2\t2\t0\t0\t0", ["6\tT\tG\t5", "12\tG\tC\t5"]),
    # bases 7 and 12: [7, 12) and [12, 17) touch, one run of 2k, no candidate
    "two_errors_runs_touch": (mut(G, 7, 12), 1, mut(G, 7, 12), "26\t10\t0\t0\t0\t0\t10", []),
    # bases 8 and 12, k - 1 apart: the 5-mer ending at 12 holds both, one run [8, 17) of 2k - 1, untouched
    "two_errors_k_minus_1_apart": (mut(G, 8, 12), 1, mut(G, 8, 12), "26\t9\t0\t0\t0\t0\t9", []),
    # N at 14 and the error at 15: of the 5-mers that hold base 15 only the one ending at 19 exists; 10 + 11 5-mers beside the N
    "beside_an_N": (mut(G, 15)[:14] + "N" + mut(G, 15)[15:], 1, G[:14] + "N" + G[15:], "21\t1\t1\t1\t0\t0\t0", ["15\tG\tC\t1"]),
    # 2k - 1 = 9 bases, the error in the middle: all five 5-mers hold it, a run of k with neither neighbour
    "stretch_all_weak": (mut(G, 14)[10:19], 1, G[10:19], "5\t5\t1\t1\t0\t0\t0", ["4\tT\tG\t5"]),
    # 8 bases: four 5-mers, all weak, shorter than k with neither neighbour: no candidate
    "short_stretch_all_weak": (mut(G, 14)[10:18], 1, mut(G, 14)[10:18], "4\t4\t0\t0\t0\t0\t4", []),
    # C at base 20, where A and T are both solid: two trials fit
    "ambiguous": (G[:20] + "C" + G[21:], 1, G[:20] + "C" + G[21:], "26\t5\t1\t0\t1\t0\t5", []),
    # bases 28 and 29: the run [28, 30) at the end names base 28, but the 5-mer ending at 29 holds base 29 as well: no trial fits
    "no_fit": (mut(G, 28, 29), 1, mut(G, 28, 29), "26\t2\t1\t0\t0\t1\t2", []),
    "shorter_than_k": ("ACG", 1, "ACG", "0\t0\t0\t0\t0\t0\t0", []),
    "lower_case": (mut(G, 12).lower(), 1, G.lower(), "26\t5\t1\t1\t0\t0\t0", ["12\tg\tc\t5"]),
    # base 1: the run [4, 6) of two; min_run 3 does not try it
    "end_error_min_run_1": (mut(G, 1), 1, G, "26\t2\t1\t1\t0\t0\t0", ["1\tT\tG\t2"]),
    "end_error_min_run_3": (mut(G, 1), 3, mut(G, 1), "26\t2\t0\t0\t0\t0\t2", []),
}
# (k, seed) at which every planted read comes back as its source
PLANTED = ((21, 1),)


@pytest.fixture(scope="module")
def hand_table(tmp_path_factory):
    return K.oracle_table([s.encode() for s in HAND_TABLE], 5, tmp_path_factory.mktemp("correct") / "hand.yak")


def both(reads, k, c, e, x, cx):
    """the flat restatement and the one on strings, which must agree in everything, with the invariants -> (flat()'s dict, the corrected reads,
    the report with its X lines)"""
    names = ["r%d" % i for i in range(len(reads))]
    img, offs, lens = K.image([r.encode() for r in reads])
    d = K.flat(img, offs, lens, k, c, e, x, cx)
    br = K.by_reads(reads, k, c, e, K.count_dict(k, x, cx))
    out = [d["img"][int(o):int(o) + int(L)].decode() for o, L in zip(offs, lens)]
    assert out == [b[0] for b in br]
    assert [tuple(int(t[f]) for f in K.TALLY_FIELDS) for t in d["tal"]] == [b[1] for b in br]
    assert [(int(r["seq"]), int(r["p"]), int(r["st"]), int(r["en"]), int(r["fit"]), int(r["why"])) for r in d["recs"]] == [(j,) + cnd for j, b in enumerate(br) for cnd in b[3]]
    assert all(int(r["at"]) == int(offs[r["seq"]]) + int(r["p"]) and img[int(r["at"])] == r["from"] for r in d["recs"])
    for lf in (False, True):
        assert K.flat_report(names, d, lens, k, c, e, lf) == K.report(names, lens, [b[1] for b in br], [b[2] for b in br], k, c, e, lf)
    # the runs of two candidates are disjoint, and no k-mer of one's run holds the other's base
    for j in range(len(reads)):
        rs = [r for r in d["recs"] if r["seq"] == j]
        for i, a in enumerate(rs):
            for b in rs[i + 1:]:                                   # the k-mers ending in [st, en) cover the bases st - k + 1 .. en - 1
                assert int(a["en"]) <= int(b["st"])
                assert not int(a["st"]) - k + 1 <= int(b["p"]) <= int(a["en"]) - 1 and not int(b["st"]) - k + 1 <= int(a["p"]) <= int(b["en"]) - 1
    # the corrected image's weak positions are the old ones minus the fixed runs
    t2 = K.counts(d["img"], k, x, cx).astype(np.int64)
    weak2 = (t2 != K.NO) & (t2 < c)
    assert [int(weak2[int(o):int(o) + int(L)].sum()) for o, L in zip(offs, lens)] == [int(t["n_weak_after"]) for t in d["tal"]]
    assert all(int(t["n_weak_after"]) == int(t["n_weak"]) - sum(int(r["en"]) - int(r["st"]) for r in d["recs"] if r["seq"] == j and r["why"] == K.DONE)
               for j, t in enumerate(d["tal"]))
    # a second correction fixes nothing and reports the same ambiguous and no-fit candidates
    d2 = K.flat(d["img"], offs, lens, k, c, e, x, cx)
    assert d2["img"] == d["img"] and not (d2["recs"]["why"] == K.DONE).any()
    left = d["recs"][d["recs"]["why"] != K.DONE]
    assert d2["recs"].tobytes() == left.tobytes()
    return d, out, K.flat_report(names, d, lens, k, c, e, True).decode().splitlines()


def random_case(rng, k):
    """(the strings the table is counted from, reads cut from them and mutated)"""
    src = ["".join(rng.choice("ACGT") for _ in range(rng.randint(3 * k, 8 * k))) for _ in range(rng.randint(1, 3))]
    reads = []
    for _ in range(rng.randint(1, 6)):
        s = rng.choice(src)
        a = rng.randrange(0, len(s) - k)
        r = s[a:a + rng.randint(1, len(s) - a)]
        for _ in range(rng.choice((0, 1, 1, 2, 3))):
            r = K.mutate(rng, r, rng.randrange(len(r)))
        if rng.random() < 0.2:
            p = rng.randrange(len(r))
            r = r[:p] + "N" + r[p + 1:]
        if rng.random() < 0.2:
            r = r.lower()
        reads.append(r)
    if rng.random() < 0.5:                                         # a second allele of one site in the table and a read with a third: ambiguous
        s = src[0]
        p = rng.randrange(k, len(s) - k)
        alt = K.mutate(rng, s, p)
        src.append(alt)
        reads.append(s[:p] + rng.choice([ch for ch in "ACGT" if ch not in (s[p], alt[p])]) + s[p + 1:])
    return src * rng.choice((1, 2)), reads


def test_the_two_restatements_agree_on_tiny_random_tables(tmp_path):
    rng = random.Random(30)
    n = dict(cand=0, fixed=0, ambig=0, nofit=0, front=0, back=0, full=0)
    for it in range(80):
        k = (5, 9)[it % 2]
        src, reads = random_case(rng, k)
        x, cx = K.oracle_table([s.encode() for s in src], k, tmp_path / "t.yak")
        c = rng.choice((1, 2)) if len(src) > 3 or it % 3 else 1
        d = both(reads, k, c, rng.choice((1, 1, 2)), x, cx)[0]
        r = d["recs"]
        n["cand"] += len(r); n["fixed"] += int((r["why"] == K.DONE).sum()); n["ambig"] += int((r["why"] == K.AMBIG).sum()); n["nofit"] += int((r["why"] == K.NOFIT).sum())
        L = r["en"].astype(int) - r["st"].astype(int)
        n["full"] += int((L == k).sum()); n["front"] += int(((L < k) & (r["p"] < r["st"])).sum()); n["back"] += int(((L < k) & (r["p"] == r["st"])).sum())
    assert min(n.values()) >= 5, n                                 # every kind of run and of decision was met


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_derived_case(hand_table, name):
    read, e, after, s_numbers, x_lines = CASES[name]
    d, out, lines = both([read], 5, 2, e, *hand_table)
    assert out == [after]
    want = ["#correct\tk=5\tmin_cnt=2\tmin_run=%d" % e, "S\tr0\t%d\t%s" % (len(read), s_numbers)] + ["X\tr0\t" + ln for ln in x_lines]
    assert lines == want + ["T\t1\t%d\t%s" % (len(read), s_numbers)]


def test_the_hand_cases_as_one_input(hand_table):
    """all of them as the records of one image: the sums of the T line, and no case changes another"""
    names = sorted(n for n in CASES if CASES[n][1] == 1)
    d, out, lines = both([CASES[n][0] for n in names], 5, 2, 1, *hand_table)
    assert out == [CASES[n][2] for n in names]
    sums = [sum(int(CASES[n][3].split("\t")[i]) for n in names) for i in range(7)]
    assert lines[-1] == "T\t%d\t%d\t%s" % (len(names), sum(len(CASES[n][0]) for n in names), "\t".join(map(str, sums)))


@pytest.mark.parametrize("k,seed", PLANTED)
def test_planted_reads_come_back_as_their_sources(tmp_path, k, seed):
    """a condition on the input, asserted here: at this seed every erroneous read is turned back into its source, every other read is left as it is,
    and no candidate is ambiguous or without a fit"""
    clean, bad = K.planted(k, seed)
    x, cx = K.oracle_table([r.encode() for r in clean], k, tmp_path / "p.yak", pre=12)
    d, out, lines = both(bad, k, 3, 1, x, cx)
    assert out == clean[::3]
    n_err = sum(a != b for r, s in zip(bad, clean[::3]) for a, b in zip(r, s))
    assert n_err > 40 and (d["recs"]["why"] == K.DONE).all() and len(d["recs"]) == n_err
    assert sum(r != s for r, s in zip(bad, clean[::3])) > 20 and sum(r == s for r, s in zip(bad, clean[::3])) > 2
    assert all(int(t["n_weak_after"]) == 0 for t in d["tal"])


# ---- the library itself, without a GPU ----
KERNELS = ["k_cor_find<COUNT>", "k_cor_find<EMIT>", "k_cor_tile_scan", "k_cor_trials", "k_cor_decide"]


def test_library_exports_its_header_and_nothing_else():
    import yak_amd.correct as correct
    from test_abi import declared
    want = declared("yak_amd_correct.h")
    assert want == set(correct.CORRECT_H_SYMBOLS) and not want & (declared("yak.h") | declared("yak_amd.h"))
    nm = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", correct.CORRECT_LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines() if ln.strip()}
    assert nm == want
    assert sorted(correct.tally()) == sorted(KERNELS) and not any(correct.tally().values()) and not [b for b in correct.tally() if "cln" in b]
    src = open(os.path.join(ROOT, "yak_amd", "correct", "correct.hip")).read()
    assert "hipLaunchKernelGGL" not in src and "<<<" not in src and len(re.findall(r"YK_LAUNCH\(", src)) == len(KERNELS)
    assert C.sizeof(correct.FixT) == 32 and C.sizeof(correct.CtallyT) == 32 and C.sizeof(correct.CroptT) == 24
    assert K.FIX_DTYPE.itemsize == 32 and [K.FIX_DTYPE.fields[f][1] for f in ("at", "seq", "p", "st", "en", "from", "to", "fit", "why")] == [
        getattr(correct.FixT, f).offset for f in ("at", "seq", "p", "st", "en", "from_", "to", "fit", "why")]
    needed = [ln for ln in subprocess.run(["readelf", "-d", correct.CORRECT_LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
              if "NEEDED" in ln or "RUNPATH" in ln or "RPATH" in ln]
    assert any("[libyak_amd.so]" in ln for ln in needed) and any("$ORIGIN" in ln for ln in needed)
    assert not [ln for ln in needed if re.search(r"libyak_amd_\w+\.so", ln)], "a layer beside it among its NEEDED entries"
    o = correct.options()
    assert (o.min_cnt, o.min_run, o.list, o.stats_only, o.chunk_size) == (3, 1, 0, 0, 1 << 28)


def test_the_base_library_is_untouched():
    """libyak_amd.so gains no export and no kernel: its names are those of tests/golden/libyak_amd_names.txt"""
    import yak_amd
    L = yak_amd.lib()
    nm = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", yak_amd.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines() if ln.strip()}
    names = C.POINTER(C.c_char_p)()
    n = L.yakamd_tally_names(C.byref(names))
    tally = [names[i].decode() for i in range(n)]
    want = open(os.path.join(ROOT, "tests", "golden", "libyak_amd_names.txt")).read().split("\n")
    assert sorted(nm) == want[1:want.index("# tally")] and tally == want[want.index("# tally") + 1:-1] and not [t for t in tally if "k_cor" in t]


def test_refusals_need_no_device(tmp_path):
    import yak_amd.correct as correct
    CL = correct.lib()
    err = CL.yakamd_correct_last_error
    o = correct.options()
    assert CL.yakamd_correct(None, None, None, None, None) == -1 and b"no options" in err()
    assert CL.yakamd_correct(C.byref(o), None, b"x.fq", str(tmp_path / "o.fq").encode(), None) == -1 and b"not an engine table" in err()
    o.chunk_size = 0
    assert CL.yakamd_correct(C.byref(o), None, b"x.fq", str(tmp_path / "o.fq").encode(), None) == -1 and b"chunk_size" in err() and not (tmp_path / "o.fq").exists()
    assert CL.yakamd_correct_image_dev(None, 3, 1, None, 0, None, None, 0, None, 0, None) == -1 and b"not an engine table" in err()
    find = lambda k, c, e, n=0, ns=0, cnt=None: CL.yakamd_correct_find_dev(k, c, e, cnt, n, None, None, ns, None, 0, None)
    assert find(32, 3, 1) == -1 and b"k must be below 32" in err()
    assert find(0, 3, 1) == -1 and b"k must be below 32" in err()
    assert find(21, 0, 1) == -1 and b"min_cnt" in err()
    assert find(21, 1024, 1) == -1 and b"min_cnt" in err()
    assert find(21, 3, 0) == -1 and b"min_run" in err()
    assert find(21, 3, 22) == -1 and b"min_run" in err()
    assert find(21, 3, 1, n=-1) == -1 and find(21, 3, 1, ns=-1) == -1 and b"bad n_bytes or n_seq" in err()
    assert find(21, 3, 1, n=16) == -1 and b"no count array" in err()
    assert find(21, 3, 1, n=16, cnt=8) == -1 and b"16-byte aligned" in err()
    assert find(21, 3, 1, ns=2) == -1 and b"without their offsets" in err()
    assert CL.yakamd_correct_trials_dev(32, None, 0, None, 0, None, 0) == -1 and b"k must be below 32" in err()
    assert CL.yakamd_correct_trials_dev(21, None, 100, None, 3, None, 0) == K.up16(6 * 21 * 3)        # the size query needs no device
    assert CL.yakamd_correct_trials_dev(21, 8, 100, None, 3, None, 0) == -1 and b"16-byte aligned" in err()
    assert CL.yakamd_correct_trials_dev(21, None, 100, None, 101, None, 0) == -1
    assert CL.yakamd_correct_decide_dev(32, 3, None, None, 0, None, 0, None, 0) == -1 and CL.yakamd_correct_decide_dev(21, 0, None, None, 0, None, 0, None, 0) == -1
    assert CL.yakamd_correct_decide_dev(21, 3, None, None, 0, None, 0, None, 0) == 0               # nothing to decide
    ms = (C.c_double * 6)(*[1.0] * 6)
    CL.yakamd_correct_ms(ms)
    assert list(ms) == [0.0] * 6 == correct.ms()


def test_cli_usage_and_no_cpu_fallback(tmp_path, hand_table):
    cli = os.path.join(ROOT, "yak_amd", "yak-amd")
    u = subprocess.run([cli, "correct"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert u.returncode == 1 and u.stderr.startswith(b"usage: yak-amd correct [options] <kmer.yak> <reads.fq>") and u.stdout == b""
    assert all(("    -%s" % ch).encode() in u.stderr for ch in "celsKor")
    top = subprocess.run([cli], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60).stderr.decode()
    assert "      yak-amd correct" in top.split("beyond the reference")[1]
    fn, out = str(tmp_path / "hand.yak"), tmp_path / "out.fa"
    K.oracle_table([s.encode() for s in HAND_TABLE], 5, fn)
    reads = tmp_path / "r.fa"
    reads.write_text(">r\n%s\n" % G)
    for a in (["-c", "0"], ["-c", "1024"], ["-e", "0"], ["-e", "6"], ["-K", "0"]):
        r = subprocess.run([cli, "correct"] + a + ["-o", str(out), fn, str(reads)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and r.stdout == b"" and b"must be in" in r.stderr and not out.exists(), a
    import yak_amd
    if yak_amd.lib().yakamd_device_count() > 0:
        return
    r = subprocess.run([cli, "correct", "-o", str(out), fn, str(reads)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and r.stdout == b"" and b"no MI355X" in r.stderr and not out.exists()
