"""`yak-amd hetmers` restated: the het-mer pairs of a count table -- k-mers that differ in the middle base alone -- twice over.
hetmers() is the XOR formulation of the definition on the canonical values, in numpy; by_families() is independent of it: the stored k-mers as
strings, grouped by their two flanks.  tests/test_hetmers.py holds the two to each other and to the hand-derived numbers of planted(); the device
is held to hetmers() by tests/test_gpu_hetmers.py.  A .yak image is read with tablecmds_util.read_yak and decoded with tablecmds_util.hash64_inv,
which tests/test_tablecmds.py holds to the reference's own `print` output."""
import random
from collections import defaultdict

import numpy as np

import tablecmds_util as T

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def members(fn):
    """(k, x as uint64 array, c as int64 array) of every stored key of a .yak file, in listing order: sub-tables ascending, slots ascending"""
    k, pairs = T.file_order_pairs(fn)
    return k, np.array([x for x, _ in pairs], np.uint64), np.array([c for _, c in pairs], np.int64)


def revcomp(v, k):
    """the reverse complement of 2-bit k-mers (first base highest), base by base"""
    v = np.asarray(v, np.uint64)
    out = np.zeros_like(v)
    for j in range(k):
        out |= (np.uint64(3) - (v >> np.uint64(2 * j) & np.uint64(3))) << np.uint64(2 * (k - 1 - j))
    return out


def hetmers(k, x, c, min_cnt):
    """(J as {(lo, hi): n}, n_group as a list of 5, the pairs [(x, y, cx, cy)] with x < y in listing order of x) by the XOR formulation"""
    assert k % 2 == 1 and k < 32 and 1 <= min_cnt <= 1023
    keep = c >= min_cnt
    x, c = x[keep], c[keep]
    n = len(x)
    order = np.argsort(x, kind="stable")
    sx, sc = x[order], c[order]
    assert n < 2 or (sx[1:] != sx[:-1]).all(), "a k-mer stored twice"
    NONE = np.uint64(2**64 - 1)
    ys, cs, ok = [], [], []
    for d in (1, 2, 3):
        v = x ^ np.uint64(d << (k - 1))
        y = np.minimum(v, revcomp(v, k))
        at = np.minimum(np.searchsorted(sx, y), max(n - 1, 0))
        hit = (sx[at] == y) if n else np.zeros(0, bool)
        good = hit & (y != x)
        for y0, ok0 in zip(ys, ok):                    # equal y's count once
            good &= ~(ok0 & (y0 == y))
        ys.append(y); cs.append(np.where(good, sc[at] if n else 0, 0)); ok.append(good)
    n_part = sum(g.astype(np.int64) for g in ok)
    y_min = np.minimum.reduce([np.where(g, y, NONE) for y, g in zip(ys, ok)]) if n else np.zeros(0, np.uint64)
    reports = x < y_min                                # the member smaller than all its partners (any x without one)
    n_group = [0] + [int((reports & (n_part == s - 1)).sum()) for s in (1, 2, 3, 4)]
    J, pairs = defaultdict(int), []
    for i in np.flatnonzero(reports & (n_part == 1)):
        d = [j for j in range(3) if ok[j][i]][0]
        cx, cy = int(c[i]), int(cs[d][i])
        J[(min(cx, cy), max(cx, cy))] += 1
        pairs.append((int(x[i]), int(ys[d][i]), cx, cy))
    return dict(J), n_group, pairs


def kmer_str(x, k):
    return "".join("ACGT"[int(x) >> 2 * j & 3] for j in range(k - 1, -1, -1))


def rc_str(s):
    return "".join(COMP[ch] for ch in reversed(s))


def by_families(k, x, c, min_cnt):
    """(J, n_group) from strings: every stored k-mer, in both orientations, falls into the family of the strings that share its two flanks; a
    family and its mirror image (the reverse complements) are one group, whose members are the distinct canonical k-mers in it"""
    h = k // 2
    fam = defaultdict(dict)
    for xi, ci in zip(x, c):
        if ci < min_cnt:
            continue
        s = kmer_str(xi, k)
        r = rc_str(s)
        canon = min(s, r)
        keys = [(t[:h], t[h + 1:]) for t in (s, r)]
        fam[min(keys)][canon] = int(ci)
    n_group, J = [0] * 5, defaultdict(int)
    for mem in fam.values():
        n_group[len(mem)] += 1
        if len(mem) == 2:
            a, b = mem.values()
            J[(min(a, b), max(a, b))] += 1
    return dict(J), n_group


def text(k, min_cnt, J, n_group, pairs=None):
    """what yakamd_hetmers writes; pairs: the K lines too"""
    out = ["#hetmers\tk=%d\tmin_cnt=%d\n" % (k, min_cnt)]
    for x, y, cx, cy in (pairs or []):
        out.append("K\t%s\t%d\t%s\t%d\n" % (kmer_str(x, k), cx, kmer_str(y, k), cy))
    out += ["G\t%d\t%d\n" % (s, n_group[s]) for s in (1, 2, 3, 4)]
    out += ["P\t%d\t%d\t%d\n" % (lo, hi, J[(lo, hi)]) for lo, hi in sorted(J)]
    return "".join(out).encode()


# ---- the planted input ----
# G: 3000 random bases, 3 copies.  H: G with another base at the 28 positions 100, 200, .. 2800, 5 copies.  T: G[450:550] with a third base at
# position 500, 2 copies.  Three records F + m + revcomp(F), m = A, C, G, F random of (k - 1) / 2 bases.
# By hand, for k = 21 and 31 (sites at least k apart, no chance repeats among 4^k k-mers):
#   - the k-mer with a site in its middle exists in G's version (count 3: T adds nothing, it lies off T or holds position 500) and in H's (count
#     5): 27 sites give a pair at J[3][5]; at position 500 T's version (count 2) is a third member: one group of three, no pair.
#   - F + A + rc(F) is its own mirror image up to the middle base: its other orientation F + T + rc(F) is the same canonical k-mer (count 1),
#     and F + C + rc(F), F + G + rc(F) are one canonical k-mer in two orientations (count 2): one pair at J[1][2], a family of two members only.
#   - distinct k-mers: 3000 - k + 1 of G, k more per site of H (28 k), k of T through position 500, 2 palindromic ones; 2 * 28 of them are in
#     pairs and 3 in the group of three, the rest are alone: n_group[1] = 3001 - k + 29 k + 2 - 59.
N_SITES = 28
EXPECT = {k: dict(n_group=[0, 3001 - k + 29 * k + 2 - 59, 28, 1, 0], J={(3, 5): 27, (1, 2): 1}) for k in (21, 31)}
assert EXPECT[31]["n_group"] == [0, 3812, 28, 1, 0] and EXPECT[21]["n_group"] == [0, 3532, 28, 1, 0]
# min_cnt = 3 takes T's and the palindromic k-mers away: position 500 is a pair like the other sites, and those k-mers are not counted at all
EXPECT_MIN3 = {k: dict(n_group=[0, 3001 - k + 28 * k - 56, 28, 0, 0], J={(3, 5): 28}) for k in (21, 31)}


def planted(k, seed=17):
    """the records of the planted input (bytes, no names)"""
    rng = random.Random(seed)
    other = lambda b, *no: rng.choice([ch for ch in "ACGT" if ch != b and ch not in no])
    G = [rng.choice("ACGT") for _ in range(3000)]
    H = list(G)
    for p in range(100, 2801, 100):
        H[p] = other(G[p])
    Tr = list(G[450:550])
    Tr[50] = other(G[500], H[500])
    F = "".join(rng.choice("ACGT") for _ in range((k - 1) // 2))
    recs = ["".join(G)] * 3 + ["".join(H)] * 5 + ["".join(Tr)] * 2 + [F + m + rc_str(F) for m in "ACG"]
    return [r.encode() for r in recs]


def image(recs):
    """the memory image of records: each followed by a newline"""
    return b"".join(r + b"\n" for r in recs)


def fasta(recs):
    return b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(recs))
