"""`yak-amd correct` restated (the definition at the top of include/yak_amd_correct.h) -- twice over.  flat() is the formulation
on the flat arrays: the base image, the per-position count array as yakamd_lookup_dev() writes it (made here from the stored keys of a .yak dump),
runs from the differences of the weak mask, the trial image and its count array, the decisions; it gives the fix records, the tallies, the trial
image and the corrected image.  by_reads() is independent of it: read by read on strings, itertools.groupby for the runs, string replacement and a
dict of canonical k-mer strings for the trials.  tests/test_correct.py holds the two to each other and to hand-derived cases; the model of the
kernels (tools/correct_model_check.cpp) is held to flat() by tests/test_correct_model.py, the device by tests/test_gpu_correct.py."""
import ctypes as C
import itertools
import random
import struct

import numpy as np

import hetmer_util as H

NO = 0xFFFF
NOFIT, DONE, AMBIG = 0, 1, 2
FIX_DTYPE = np.dtype([("at", "<u8"), ("seq", "<u4"), ("p", "<u4"), ("st", "<u4"), ("en", "<u4"), ("from", "u1"), ("to", "u1"), ("fit", "u1"), ("why", "u1"),
                      ("reserved", "<u4")])
TALLY_FIELDS = ("n_kmer", "n_weak", "n_cand", "n_fixed", "n_ambig", "n_nofit", "n_weak_after")
TALLY_DTYPE = np.dtype([(f, "<u4") for f in TALLY_FIELDS + ("reserved",)])
assert FIX_DTYPE.itemsize == 32 and TALLY_DTYPE.itemsize == 32

CODE = np.full(256, 4, np.uint8)                                   # ACGT, acgt, U, u and the bytes 0 .. 3 are bases
for _b, _v in ((b"Aa\x00", 0), (b"Cc\x01", 1), (b"Gg\x02", 2), (b"TtUu\x03", 3)):
    CODE[list(_b)] = _v


def up16(n):
    return (n + 15) & ~15


def image(seqs):
    """sequences laid out as the chunk reader does: each followed by a newline -> (image, offsets, lengths)"""
    offs = np.cumsum([0] + [len(s) + 1 for s in seqs[:-1]]).astype(np.uint64) if seqs else np.zeros(0, np.uint64)
    return b"".join(bytes(s) + b"\n" for s in seqs), offs, np.array([len(s) for s in seqs], np.uint32)


def oracle_table(recs, k, fn, pre=10):
    """(x, c) of the stored keys of the .yak file the oracle dumps to `fn` after counting the records"""
    from oracle import pyoracle
    L = pyoracle.lib()
    img = b"".join(bytes(r) + b"\n" for r in recs)
    o = pyoracle.copt(k=k, pre=pre)
    t = L.yko_count_mem(img, len(img), C.byref(o), None)
    assert L.yko_ch_dump(t, str(fn).encode()) == 0
    L.yko_ch_destroy(t)
    kk, x, c = H.members(str(fn))
    assert kk == k
    return x, c


def counts(img, k, x, c):
    """the array yakamd_lookup_dev() writes for the image against the table of the stored keys x with counts c: the count of the canonical k-mer
    ending at every byte (0 for an absent one), NO where none ends"""
    b = CODE[np.frombuffer(bytes(img), np.uint8)].astype(np.uint64)
    n = len(b)
    out = np.full(n, NO, np.uint16)
    if n < k:
        return out
    bad = np.concatenate(([0], np.cumsum(b > 3)))
    fw = np.zeros(n - k + 1, np.uint64)
    for j in range(k):                                             # the k-mer starting at s, first base highest
        fw = fw << np.uint64(2) | (b[j:n - k + 1 + j] & np.uint64(3))
    ok = bad[k:] - bad[:n - k + 1] == 0
    y = np.minimum(fw, H.revcomp(fw, k))
    order = np.argsort(x, kind="stable")
    sx, sc = np.asarray(x, np.uint64)[order], np.asarray(c, np.int64)[order]
    v = np.zeros(len(y), np.int64)
    if len(sx):
        at = np.minimum(np.searchsorted(sx, y), len(sx) - 1)
        v = np.where(sx[at] == y, sc[at], 0)
    out[k - 1:] = np.where(ok, np.maximum(v, 0), NO).astype(np.uint16)
    return out


# ---- (a) flat ----
def find(t, offs, lens, k, c, e):
    """(the fix records after the find in image order, the tallies after the find) of the count array t"""
    t = np.asarray(t, np.int64)
    n, ns = len(t), len(lens)
    exists = t != NO
    weak = exists & (t < c)
    tal = np.zeros(ns, TALLY_DTYPE)
    for j in range(ns):
        o, L = int(offs[j]), int(lens[j])
        tal[j]["n_kmer"] = int(exists[o:o + L].sum())
        tal[j]["n_weak"] = tal[j]["n_weak_after"] = int(weak[o:o + L].sum())
    w = np.concatenate(([0], weak.astype(np.int8), [0]))
    d = np.diff(w)
    rows = []
    for st, en in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1)):
        st, en = int(st), int(en)
        j = int(np.searchsorted(np.asarray(offs, np.uint64), st, "right")) - 1
        if j < 0 or st >= int(offs[j]) + int(lens[j]):
            continue                                               # a run in no sequence
        front, back, L = st > 0 and bool(exists[st - 1]), en < n and bool(exists[en]), en - st
        if L < e or L > k:
            continue
        if L == k:
            p = st
        elif not front and back:
            p = en - k
        elif front and not back:
            p = st
        else:
            continue
        o = int(offs[j])
        if p < o:
            continue
        tal[j]["n_cand"] += 1
        rows.append((p, j, p - o, st - o, en - o, 0, 0, 0, 0, 0))
    return np.array(rows, FIX_DTYPE) if rows else np.zeros(0, FIX_DTYPE), tal


def others(o):
    """the three codes that are not o, ascending"""
    return [b for b in range(4) if b != o]


def trial_image(img, recs, k):
    """the trial image of the records: trial 3 cand + a at bytes [2k t, 2k (t + 1)), newlines to a multiple of 16"""
    out = bytearray(b"\n" * up16(6 * k * len(recs)))
    for i, r in enumerate(recs):
        at, off = int(r["at"]), int(r["at"]) - int(r["p"])
        lo, hi = off + int(r["st"]) - k + 1, off + int(r["en"])
        for a, b in enumerate(others(int(CODE[img[at]]))):
            w = bytearray(img[lo:hi])
            w[at - lo] = b"ACGT"[b]
            out[2 * k * (3 * i + a):2 * k * (3 * i + a) + len(w)] = w
    return bytes(out)


def decide(img, recs, tal, tc, k, c):
    """(the records with from, to, fit and why, the tallies completed, the corrected image) from the count array tc of the trial image"""
    img, recs, tal = bytearray(img), recs.copy(), tal.copy()
    for i, r in enumerate(recs):
        at, L = int(r["at"]), int(r["en"]) - int(r["st"])
        frm = img[at]
        fit = 0
        for a, b in enumerate(others(int(CODE[frm]))):
            v = tc[2 * k * (3 * i + a) + k - 1:2 * k * (3 * i + a) + k - 1 + L].astype(np.int64)
            if ((v != NO) & (v >= c)).all():
                fit |= 1 << b
        nfit = bin(fit).count("1")
        why = NOFIT if nfit == 0 else DONE if nfit == 1 else AMBIG
        to = (b"ACGT"[fit.bit_length() - 1] | (frm & 0x20)) if why == DONE else 0
        recs[i]["from"], recs[i]["to"], recs[i]["fit"], recs[i]["why"] = frm, to, fit, why
        t = tal[int(r["seq"])]
        t[("n_nofit", "n_fixed", "n_ambig")[why]] += 1
        if why == DONE:
            t["n_weak_after"] -= L
    for r in recs:                                                 # all decisions on one snapshot, applied together
        if r["why"] == DONE:
            img[int(r["at"])] = int(r["to"])
    return recs, tal, bytes(img)


def flat(img, offs, lens, k, c, e, x, cx):
    """the whole correction of an image against the table (x, cx): dict of t, recs0 (after the find), tal0, trials, tc, recs, tal, img"""
    t = counts(img, k, x, cx)
    recs0, tal0 = find(t, offs, lens, k, c, e)
    tr = trial_image(img, recs0, k)
    tc = counts(tr, k, x, cx)
    recs, tal, out = decide(img, recs0, tal0, tc, k, c)
    return dict(t=t, recs0=recs0, tal0=tal0, trials=tr, tc=tc, recs=recs, tal=tal, img=out)


# ---- (b) read by read, on strings ----
def norm(s):
    return s.upper().replace("U", "T")


def count_dict(k, x, c):
    """{canonical k-mer string: count}"""
    return {H.kmer_str(xi, k): int(ci) for xi, ci in zip(x, c)}


def status(read, k, c, cd):
    """per position of the read: 'n' no k-mer ends, 'w' weak, 's' solid"""
    s, out = norm(read), []
    for i in range(len(s)):
        km = s[i - k + 1:i + 1] if i >= k - 1 else ""
        if len(km) < k or any(ch not in "ACGT" for ch in km):
            out.append("n")
        else:
            out.append("w" if cd.get(min(km, H.rc_str(km)), 0) < c else "s")
    return out


def by_reads(reads, k, c, e, cd):
    """per read (the corrected read, the tally as a tuple in TALLY_FIELDS order, [(p, from, to, run_len)] of the fixed bases,
    [(p, st, en, fit, why)] of all candidates)"""
    out = []
    for read in reads:
        stat = status(read, k, c, cd)
        at, cands = 0, []
        for v, g in itertools.groupby(stat):
            n = len(list(g))
            st, en = at, at + n
            at = en
            if v != "w" or n < e or n > k:
                continue
            front = st > 0 and stat[st - 1] != "n"
            back = en < len(stat) and stat[en] != "n"
            if n == k:
                p = st
            elif not front and back:
                p = en - k
            elif front and not back:
                p = st
            else:
                continue
            cands.append((p, st, en))
        new, fixes, all_c, n_amb, n_no, gone = list(read), [], [], 0, 0, 0
        for p, st, en in cands:
            fits = []
            for b in "ACGT":
                if b == norm(read[p]):
                    continue
                trial = norm(read[:p]) + b + norm(read[p + 1:])
                kms = [trial[i - k + 1:i + 1] for i in range(st, en)]
                assert all(len(km) == k and p - (i - k + 1) in range(k) for i, km in zip(range(st, en), kms))
                if all(cd.get(min(km, H.rc_str(km)), 0) >= c for km in kms):
                    fits.append(b)
            fit = sum(1 << "ACGT".index(b) for b in fits)
            if len(fits) == 1:
                to = fits[0].lower() if ord(read[p]) & 0x20 else fits[0]
                new[p] = to
                fixes.append((p, read[p], to, en - st))
                gone += en - st
            n_amb += len(fits) > 1
            n_no += not fits
            all_c.append((p, st, en, fit, DONE if len(fits) == 1 else AMBIG if fits else NOFIT))
        nw = stat.count("w")
        out.append(("".join(new), (len(stat) - stat.count("n"), nw, len(cands), len(fixes), n_amb, n_no, nw - gone), fixes, all_c))
    return out


# ---- the texts ----
def report(names, lens, tallies, fixes, k, c, e, list_fixed=False):
    """the report: tallies = a tuple in TALLY_FIELDS order per sequence, fixes = [(p, from, to, run_len)] per sequence"""
    out = ["#correct\tk=%d\tmin_cnt=%d\tmin_run=%d\n" % (k, c, e)]
    tot = [0] * 7
    for name, L, t, fx in zip(names, lens, tallies, fixes):
        out.append("S\t%s\t%d\t%s\n" % (name, L, "\t".join(str(int(v)) for v in t)))
        tot = [a + int(b) for a, b in zip(tot, t)]
        if list_fixed:
            out += ["X\t%s\t%d\t%s\t%s\t%d\n" % (name, p, f, to, n) for p, f, to, n in fx]
    out.append("T\t%d\t%d\t%s\n" % (len(names), sum(int(v) for v in lens), "\t".join(str(v) for v in tot)))
    return "".join(out).encode()


def flat_report(names, d, lens, k, c, e, list_fixed=False):
    """the report of a flat() result"""
    tallies = [tuple(int(t[f]) for f in TALLY_FIELDS) for t in d["tal"]]
    fixes = [[(int(r["p"]), chr(r["from"]), chr(r["to"]), int(r["en"]) - int(r["st"])) for r in d["recs"] if r["seq"] == j and r["why"] == DONE] for j in range(len(names))]
    return report(names, lens, tallies, fixes, k, c, e, list_fixed)


def reads_text(records, seqs):
    """the reads output: records = [(name, comment, quality or '')], seqs = the corrected sequences"""
    out = []
    for (name, comment, qual), s in zip(records, seqs):
        head = name + (" " + comment if comment else "")
        out.append("@%s\n%s\n+\n%s\n" % (head, s, qual) if qual else ">%s\n%s\n" % (head, s))
    return "".join(out).encode()


# ---- inputs ----
def mutate(rng, s, p):
    return s[:p] + rng.choice([ch for ch in "ACGT" if ch != s[p]]) + s[p + 1:]


def planted(k, seed, n_genome=3000, n_reads=40, read_len=150):
    """(the error-free reads, one of every three with substitutions that have at least k bases between them -- two errors at p and p + k share no
    k-mer, but their runs [p, p + k) and [p + k, p + 2k) touch and are one run of 2k; from p + k + 1 on a solid position parts them): every read
    of a random genome is there three times, so that each of its k-mers reaches min_cnt 3"""
    rng = random.Random(seed)
    g = "".join(rng.choice("ACGT") for _ in range(n_genome))
    starts = [rng.randrange(0, n_genome - read_len + 1) for _ in range(n_reads)]
    clean = [g[s:s + read_len] for s in starts for _ in range(3)]
    bad = []
    for r in clean[::3]:
        pos, p = [], rng.randrange(0, k)
        while p < read_len:
            pos.append(p)
            p += k + 1 + rng.randrange(0, 2 * k)
        for p in pos[:rng.randrange(1, 4)] if rng.random() < 0.8 else []:
            r = mutate(rng, r, p)
        bad.append(r)
    return clean, bad


def model_file(fn, k, c, e, x, cx):
    """the table tools/correct_model_check.cpp reads: k, min_cnt, min_run, the number of stored keys, then each key with its count"""
    with open(fn, "wb") as f:
        f.write(struct.pack("<IIIQ", k, c, e, len(x)))
        f.write(b"".join(struct.pack("<QI", int(a), int(b)) for a, b in zip(x, cx)))
