"""`yak-amd hetmers`, its definition restated twice in tests/hetmer_util.py and held to itself on oracle-counted tables: the
XOR formulation on canonical values against the families of strings that share both flanks, the hand-derived numbers of the planted input, the
order of the pair list; and, without a GPU, the refusal of every new entry point."""
import ctypes as C

import numpy as np
import pytest

import hetmer_util as U


def counted(oracle, tmp_path_factory, img, k, pre=10):
    data, _ = oracle.count_protocol_mem(img, k=k, pre=pre, bf_shift=0)
    fn = str(tmp_path_factory.mktemp("hetmers") / ("k%d.yak" % k))
    open(fn, "wb").write(data)
    kk, x, c = U.members(fn)
    assert kk == k
    return k, x, c


@pytest.fixture(scope="module", params=[5, 21, 31])
def planted(request, oracle, tmp_path_factory):
    return counted(oracle, tmp_path_factory, U.image(U.planted(request.param)), request.param)


@pytest.fixture(scope="module")
def reads(oracle, synth, tmp_path_factory):
    """2000 reads of 150 bases over a 10 kb genome at 0.5 % errors: an error in the middle of a k-mer makes a pair at (1, coverage)"""
    return counted(oracle, tmp_path_factory, synth(2000, 150), 31)


@pytest.mark.parametrize("min_cnt", [1, 3, 1023])
def test_formulations_agree_on_planted(planted, min_cnt):
    J, g, pairs = U.hetmers(*planted, min_cnt)
    assert (J, g) == U.by_families(*planted, min_cnt)
    assert sum(s * g[s] for s in range(5)) == int((planted[2] >= min_cnt).sum())     # every member is in one group
    if min_cnt == 1023:
        assert g == [0] * 5 and not J and not pairs


@pytest.mark.parametrize("min_cnt", [1, 3, 1023])
def test_formulations_agree_on_reads(reads, min_cnt):
    J, g, pairs = U.hetmers(*reads, min_cnt)
    assert (J, g) == U.by_families(*reads, min_cnt)
    if min_cnt == 1:
        assert sum(n for (lo, hi), n in J.items() if lo == 1 and hi >= 10) > 100, "no organic pairs at (1, coverage)"
        assert g[1] > 10000 and g[2] > 100


def test_planted_has_the_hand_derived_numbers(planted):
    k, x, c = planted
    if k == 5:                                          # dense: 4^5 / 2 canonical k-mers, most of them stored
        J, g, _ = U.hetmers(k, x, c, 1)
        assert g[4] > 50 and g[4] > g[1]
        return
    for min_cnt, want in ((1, U.EXPECT[k]), (3, U.EXPECT_MIN3[k])):
        J, g, pairs = U.hetmers(k, x, c, min_cnt)
        assert g == want["n_group"] and J == want["J"], (k, min_cnt, g, J)
    assert U.hetmers(k, x, c, 6)[1][2:] == [0, 0, 0]    # what is left above 5 (shared by G, H and T) has no neighbour
    # the palindromic pair: x = F A rc(F) at count 1, y = F C rc(F) at count 2
    _, _, pairs = U.hetmers(k, x, c, 1)
    (px, py, cx, cy), = [p for p in pairs if (p[2], p[3]) == (1, 2)]
    s, t = U.kmer_str(px, k), U.kmer_str(py, k)
    h = k // 2
    assert s[h] == "A" and t[h] == "C" and s[:h] == t[:h] == U.rc_str(s[h + 1:]) and s[h + 1:] == t[h + 1:]


@pytest.mark.parametrize("min_cnt", [1, 3])
def test_pair_list_is_ordered_and_complete(planted, reads, min_cnt):
    for k, x, c in (planted, reads):
        J, g, pairs = U.hetmers(k, x, c, min_cnt)
        assert len(pairs) == sum(J.values()) == g[2]
        pos = {int(v): i for i, v in enumerate(x)}
        at = [pos[p[0]] for p in pairs]
        assert all(a < b for a, b in zip(at, at[1:])), "not in listing order of x"
        assert all(p[0] < p[1] for p in pairs)
        cnt = {int(v): int(n) for v, n in zip(x, c)}
        assert all(cnt[p[0]] == p[2] and cnt[p[1]] == p[3] for p in pairs)
        ys, xs = np.array([p[1] for p in pairs], np.uint64), np.array([p[0] for p in pairs], np.uint64)
        middle = lambda d: (d >> np.uint64(k - 1) << np.uint64(k - 1) == d) & (d < np.uint64(1 << (k + 1))) & (d > 0)
        assert (middle(xs ^ ys) | middle(xs ^ U.revcomp(ys, k))).all()     # y in one of its orientations differs from x in the middle base alone


def test_text_format():
    J, g = {(1, 2): 1, (3, 5): 27, (3, 3): 2}, [0, 10, 30, 1, 0]
    assert U.text(5, 2, J, g) == b"#hetmers\tk=5\tmin_cnt=2\nG\t1\t10\nG\t2\t30\nG\t3\t1\nG\t4\t0\nP\t1\t2\t1\nP\t3\t3\t2\nP\t3\t5\t27\n"
    assert U.text(3, 1, {}, [0] * 5, [(0b000110, 0b001110, 7, 9)]).split(b"\n")[1] == b"K\tACG\t7\tATG\t9"


def test_no_cpu_fallback_without_gpu(tmp_path):
    """every new entry point refuses without a gfx950 device; the option defaults are pure host code"""
    import yak_amd
    L = yak_amd.lib()
    calls = [L.yakamd_hetmers_dev, L.yakamd_hetmer_pairs_dev, L.yakamd_hetmers]
    o = yak_amd.HmoptT()
    L.yakamd_hmopt_init(C.byref(o))
    assert (o.min_cnt, o.print_pairs, o.batch_keys) == (1, 0, 1 << 24)
    assert C.sizeof(yak_amd.HetpairT) == 24 and C.sizeof(yak_amd.HmoptT) == 16
    if L.yakamd_device_count() > 0:
        return
    out = tmp_path / "o.txt"
    for call in (lambda: calls[0](None, 1, None, None, None), lambda: calls[1](None, 1, None, 0), lambda: calls[2](C.byref(o), None, str(out).encode())):
        assert call() == -1 and b"no gfx950" in L.yakamd_last_error()
    assert not out.exists()
