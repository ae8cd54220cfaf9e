"""Independent restatements for the `yak chkerr` and `yak sexchr` tests (no device needed): te_worker's streak rule of chkerr.c:38-67 over
the counts of one sequence's end positions, the run list the device's streak export returns, sexchr.c:57-65's tally, and the hashes of
chkerr.c:28-58 (yak_hash64 at k < 32, yak_hash_long at k >= 32) for hand-written tables."""
import numpy as np

M64 = (1 << 64) - 1
NT4 = {ord(c): i for i, c in enumerate("ACGT")}
NT4.update({ord(c): i for i, c in enumerate("acgt")})


def chkerr_lines(name, cnt, k, min_cnt, min_streak):
    """te_worker (chkerr.c:38-67) over cnt[i] = the count of the k-mer ending at position i (-1 if absent, None if no k-mer ends there)"""
    out, last, streak = [], -1, 0
    for i, c in enumerate(cnt):
        if c is None or not c < min_cnt:
            continue
        if i != last + 1:
            if streak > min_streak:
                out.append(b"%s\t%d\t%d\t%d\n" % (name, last + 1 - k - (streak - 1), last + 1, streak))
            streak = 1
        else:
            streak += 1
        last = i
    if streak > min_streak:
        out.append(b"%s\t%d\t%d\t%d\n" % (name, last + 1 - k - (streak - 1), last + 1, streak))
    return b"".join(out)


def low_runs(low, off, lens, min_streak):
    """the list yakamd_chkerr_streaks_dev returns: (record, st, en, 1) per maximal run of 1 in low[off[j] .. off[j] + len[j]) with
    en - st > min_streak"""
    out = []
    for j, (o, n) in enumerate(zip(off, lens)):
        t = (np.asarray(low[o:o + n]) == 1).astype(np.int8)
        if len(t) == 0:
            continue
        d = np.diff(np.concatenate(([0], t, [0])))
        for s, e in zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()):
            if e - s > min_streak:
                out.append((j, s, e, 1))
    return out


def sexchr_tally(flag, off, lens):
    """sexchr.c:57-65 per record: [n_k, n_sexchr, n_sex1, n_sex2] over the positions whose flag is not 0xff"""
    out = np.zeros((len(off), 4), np.uint64)
    for j, (o, n) in enumerate(zip(off, lens)):
        f = np.asarray(flag[o:o + n]).astype(np.int64)
        f = f[f != 0xFF]
        out[j] = (len(f), int((f > 0).sum()), int((f == 1).sum()), int((f == 2).sum()))
    return out


def hash64_64(key):
    key = (~key + (key << 21)) & M64
    key ^= key >> 24
    key = (key + (key << 3) + (key << 8)) & M64
    key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & M64
    key ^= key >> 28
    return (key + (key << 31)) & M64


def kmer_hash(seq, k):
    """the hash chkerr.c computes for the k-mer seq (k bases of ACGT): yak_hash64 of the canonical 2-bit k-mer at k < 32, yak_hash_long else"""
    assert len(seq) == k
    if k < 32:
        mask, shift = (1 << 2 * k) - 1, 2 * (k - 1)
        x0 = x1 = 0
        for b in seq:
            c = NT4[b]
            x0 = (x0 << 2 | c) & mask
            x1 = x1 >> 2 | (3 - c) << shift
        key = min(x0, x1)
        key = (~key + (key << 21)) & mask
        key ^= key >> 24
        key = (key + (key << 3) + (key << 8)) & mask
        key ^= key >> 14
        key = (key + (key << 2) + (key << 4)) & mask
        key ^= key >> 28
        return (key + (key << 31)) & mask
    mask, shift = (1 << k) - 1, k - 1
    x = [0, 0, 0, 0]
    for b in seq:
        c = NT4[b]
        x[0] = (x[0] << 1 | (c & 1)) & mask
        x[1] = (x[1] << 1 | (c >> 1)) & mask
        x[2] = x[2] >> 1 | (1 - (c & 1)) << shift
        x[3] = x[3] >> 1 | (1 - (c >> 1)) << shift
    j = 0 if x[1] < x[3] else 1
    return (hash64_64(x[j << 1]) + hash64_64(x[j << 1 | 1])) & M64


def h2b(h32, bits):
    """khashl.h:98"""
    return ((h32 * 2654435769) & 0xFFFFFFFF) >> (32 - bits)
