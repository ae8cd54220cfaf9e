"""`yak-amd cover` restated twice, sharing nothing with the device code and nothing with each other.
(a) flat numpy over the per-position count array t as yakamd_lookup_dev() writes it: element j = the count of the k-mer ENDING at j, 0xffff where
    none ends.  hit(j) = t[j] != 0xffff and lo <= min(t[j], 1023) <= hi; cov(i) = some j in [i, min(i + k - 1, n - 1)] has hit(j).
(b) by strings: every k-mer start of every sequence with a valid window gets its count from a dict, marks its k bases, and the intervals come
    from itertools.groupby."""
import itertools

import numpy as np

from depth_util import image, read_fastx                 # the chunk reader's layout and a FASTA / FASTQ reader: no part of the definition

NOKMER = 0xFFFF
COV_DTYPE = np.dtype([("n_kmer", "<u4"), ("n_hit", "<u4"), ("n_cov", "<u4"), ("n_run", "<u4")])     # yakamd_cov_t
BASES = frozenset(b"ACGTacgt")


# ---- (a) flat numpy ----
def hit(t, lo, hi):
    t = np.asarray(t, np.uint16)
    c = np.minimum(t, 1023)
    return (t != NOKMER) & (c >= lo) & (c <= hi)


def cov(t, k, lo, hi):
    """one byte per position: 1 where the base lies inside a hitting k-mer"""
    h = hit(t, lo, hi)
    c = np.zeros(len(h), bool)
    for d in range(min(k, len(h))):                       # cov(i) |= hit(i + d), as far as the array goes
        c[:len(h) - d] |= h[d:]
    return c.astype(np.uint8)


def tallies(t, offs, lens, k, lo, hi):
    """the yakamd_cov_t array yakamd_cover_dev() must write"""
    t = np.asarray(t, np.uint16)
    h, c = hit(t, lo, hi), cov(t, k, lo, hi)
    out = np.zeros(len(lens), COV_DTYPE)
    for s, (off, L) in enumerate(zip(offs, lens)):
        off, L = int(off), int(L)
        cs = c[off:off + L]
        before = np.concatenate(([0], cs[:-1])) if L else cs
        out[s] = (int((t[off:off + L] != NOKMER).sum()), int(h[off:off + L].sum()), int(cs.sum()), int(((cs == 1) & (before == 0)).sum()))
    return out


def intervals(t, offs, lens, k, lo, hi):
    """per sequence the maximal runs [start, end) of covered bases, in the sequence's own coordinates"""
    c = cov(t, k, lo, hi)
    out = []
    for off, L in zip(offs, lens):
        d = np.diff(np.concatenate(([0], c[int(off):int(off) + int(L)].astype(np.int8), [0])))
        out.append(list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist())))
    return out


def masked(img, c, mode):
    """the masked image: mode 0 the image, 1 covered ASCII letters in lower case, 2 covered bytes as 'N'"""
    b = np.frombuffer(bytes(img), np.uint8).copy()
    on = np.asarray(c[:len(b)], bool)
    if mode == 1:
        low = b | 0x20
        letter = (low >= ord("a")) & (low <= ord("z"))
        b[on & letter] = low[on & letter]
    elif mode == 2:
        b[on] = ord("N")
    return b.tobytes()


# ---- the command ----
def selected(n_hit, n_cov, L, min_hit=0, min_frac=0.0, invert=False):
    return (n_hit >= min_hit and float(n_cov) >= min_frac * float(L)) != bool(invert)


def text(names, t, offs, lens, k, lo=1, hi=1023, intervals_too=False, min_hit=0, min_frac=0.0, invert=False):
    """the bytes of `yak-amd cover` in table mode"""
    tl, iv = tallies(t, offs, lens, k, lo, hi), intervals(t, offs, lens, k, lo, hi)
    out, n_sel = [b"#cover\tk=%d\tlo=%d\thi=%d\n" % (k, lo, hi)], 0
    for name, L, x, runs in zip(names, lens, tl, iv):
        if not selected(int(x["n_hit"]), int(x["n_cov"]), int(L), min_hit, min_frac, invert):
            continue
        n_sel += 1
        out.append(b"S\t%s\t%d\t%d\t%d\t%d\t%d\n" % (name, L, x["n_kmer"], x["n_hit"], x["n_cov"], x["n_run"]))
        if intervals_too:
            out += [b"B\t%s\t%d\t%d\n" % (name, st, en) for st, en in runs]
    out.append(b"T\t%d\t%d\t%d\t%d\t%d\t%d\n" % (len(lens), n_sel, sum(int(L) for L in lens), tl["n_kmer"].astype(np.int64).sum(),
                                                 tl["n_hit"].astype(np.int64).sum(), tl["n_cov"].astype(np.int64).sum()))
    return b"".join(out)


def fasta(names, img, t, offs, lens, k, lo=1, hi=1023, mask=0, min_hit=0, min_frac=0.0, invert=False):
    """the bytes of `yak-amd cover -m none|soft|hard` (mask 0, 1, 2)"""
    tl, m = tallies(t, offs, lens, k, lo, hi), masked(img, cov(t, k, lo, hi), mask)
    out = []
    for name, off, L, x in zip(names, offs, lens, tl):
        if selected(int(x["n_hit"]), int(x["n_cov"]), int(L), min_hit, min_frac, invert):
            out.append(b">%s\n%s\n" % (name, m[int(off):int(off) + int(L)]))
    return b"".join(out)


# ---- (b) by strings ----
def kmers_of(seq, k):
    """(start, the k-mer in upper case) of every start whose window holds bases alone"""
    return [(s, seq[s:s + k].upper()) for s in range(len(seq) - k + 1) if all(ch in BASES for ch in seq[s:s + k])]


def by_strings(seqs, count_of, k, lo, hi):
    """per sequence (n_kmer, n_hit, n_cov, n_run, intervals); count_of: a dict from an upper-case k-mer to its count in the table (0 when absent)"""
    out = []
    for seq in seqs:
        mark, n_kmer, n_hit = [0] * len(seq), 0, 0
        for s, km in kmers_of(seq, k):
            n_kmer += 1
            if lo <= min(count_of[km], 1023) <= hi:
                n_hit += 1
                mark[s:s + k] = [1] * k
        runs, at = [], 0
        for v, g in itertools.groupby(mark):
            n = len(list(g))
            if v:
                runs.append((at, at + n))
            at += n
        out.append((n_kmer, n_hit, sum(mark), len(runs), runs))
    return out


# ---- inputs for the tests ----
def count_dict(oracle, o, seqs, k):
    """the dict of (b): every distinct valid k-mer of seqs -> its count in the oracle's table o, each looked up as a sequence of its own"""
    kms = sorted({km for s in seqs for _, km in kmers_of(s, k)})
    if not kms:
        return {}
    t = oracle.lookup_image(o, b"".join(km + b"\n" for km in kms), 2)
    got = t[k - 1::k + 1]
    assert len(got) == len(kms) and (got != NOKMER).all()
    return dict(zip(kms, got.tolist()))


def variants(seqs, k):
    """[(name, sequence)]: the sequences as they are, then with a stretch in lower case, with Ns, with a planted stretch that no table of random
    sequence holds, and sequences of 1, k - 1 and k bases"""
    out = [(b"s%d" % i, s) for i, s in enumerate(seqs)]
    a, b, c = seqs[0], seqs[1 % len(seqs)], seqs[2 % len(seqs)]
    out.append((b"lower", a[:40] + a[40:90].lower() + a[90:]))
    out.append((b"withN", b[:50] + b"N" + b[51:70] + b"NN" + b[72:]))
    out.append((b"planted", c[:45] + b"A" * 60 + c[105:]))
    out += [(b"one", a[:1]), (b"km1", a[:k - 1]), (b"k", a[:k])]
    return out
