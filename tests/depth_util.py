"""`yak-amd depth` restated in numpy over a per-position count array as yakamd_lookup_dev() writes it: element i = the
count of the k-mer ENDING at position i, 0xffff where none ends.  A sequence of L bases is cut into windows of w k-mer START positions
(w = 0: one window); the k-mer starting at s is element s + k - 1.  Nothing here is shared with the device code: the median comes from a sort."""
import gzip

import numpy as np

NOKMER = 0xFFFF
WIN_DTYPE = np.dtype([("n_kmer", "<u4"), ("n_present", "<u4"), ("median", "<u4"), ("max", "<u4"), ("sum", "<u8")])   # yakamd_win_t
HEADER = b"#name\tstart\tend\tn_kmer\tn_present\tmean\tmedian\tmax\n"


def windows(L, w):
    """the (start, end) bounds in bases of the windows of a sequence of L bases: max(1, ceil(L / w)) of them"""
    if w == 0 or L == 0:
        return [(0, L)]
    return [(s, min(L, s + w)) for s in range(0, L, w)]


def win_off(lens, w):
    """the exclusive scan of the windows per sequence, and their total: len(lens) + 1 words"""
    return np.concatenate(([0], np.cumsum([len(windows(int(L), w)) for L in lens]))).astype(np.uint64)


def window_values(t, off, L, k, st, en):
    """the counts of the k-mers that start in [st, en) of the sequence at t[off : off + L]"""
    v = np.asarray(t[off + st + k - 1: off + min(en + k - 1, L)]) if st + k - 1 < L else np.zeros(0, np.uint16)
    return v[v != NOKMER].astype(np.int64)


def reduce(v):
    """(n_kmer, n_present, sum, lower median, max) of the counts v"""
    if len(v) == 0:
        return 0, 0, 0, 0, 0
    s = np.sort(v)
    return len(v), int((v > 0).sum()), int(v.sum()), int(s[(len(v) - 1) // 2]), int(s[-1])


def depth(t, offs, lens, k, w):
    """per sequence the list of (start, end, n_kmer, n_present, sum, median, max) of its windows"""
    return [[(st, en) + reduce(window_values(t, int(off), int(L), k, st, en)) for st, en in windows(int(L), w)] for off, L in zip(offs, lens)]


def structs(t, offs, lens, k, w):
    """the yakamd_win_t array yakamd_depth_reduce_dev() must write"""
    rows = [r[2:] for seq in depth(t, offs, lens, k, w) for r in seq]
    out = np.zeros(len(rows), WIN_DTYPE)
    for i, (n, p, s, m, x) in enumerate(rows):
        out[i] = (n, p, m, x, s)
    return out


def text(names, t, offs, lens, k, w):
    """the bytes `yak-amd depth` writes"""
    out = [HEADER]
    for name, seq in zip(names, depth(t, offs, lens, k, w)):
        for st, en, n, p, s, m, x in seq:
            out.append(b"%s\t%d\t%d\t%d\t%d\t%s\t%d\t%d\n" % (name, st, en, n, p, (b"%.3f" % (s / n)) if n else b"0.000", m, x))
    return b"".join(out)


def image(seqs):
    """sequences laid out as the chunk reader does: each followed by '\\n' -> (image, offsets, lengths)"""
    offs = np.cumsum([0] + [len(s) + 1 for s in seqs[:-1]]).astype(np.uint64) if seqs else np.zeros(0, np.uint64)
    return b"".join(s + b"\n" for s in seqs), offs, np.array([len(s) for s in seqs], np.uint32)


def read_fastx(path):
    """[(name, sequence)] of a FASTA / FASTQ file, plain or .gz; the name ends at the first blank"""
    data = (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")).read()
    lines, out, i = data.split(b"\n"), [], 0
    while i < len(lines):
        ln = lines[i]
        if ln[:1] not in (b">", b"@"):
            i += 1
            continue
        fastq, name, seq = ln[:1] == b"@", ln[1:].split()[0] if ln[1:].split() else b"", b""
        i += 1
        while i < len(lines) and lines[i][:1] not in (b">", b"@", b"+"):
            seq += lines[i].rstrip(b"\r")
            i += 1
        if fastq and i < len(lines) and lines[i][:1] == b"+":
            i += 1
            q = 0
            while i < len(lines) and q < len(seq):
                q += len(lines[i].rstrip(b"\r"))
                i += 1
        out.append((name, seq))
    return out
