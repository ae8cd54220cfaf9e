"""The cleaning of the unitig graph (`yak-amd clean`; include/yak_amd_clean.h) restated twice over, and the command's report.
by_links() applies the definitions to the link list of gfa_util, the descriptors of graph_util's unitigs and the bubble records of
bubble_util.by_links(): unitig by unitig, with the coverage order as integer products.  by_strings() is independent of the link list and of the
records: e -> x holds iff the last k - 1 bases of one oriented unitig are the first k - 1 of the other, all degrees are counted from that relation,
the bubbles are those of bubble_util.by_strings(), the tips are decided anchor by anchor -- among the unitigs that leave one end, every candidate
goes when one of them is no candidate, and all but the strongest go otherwise -- and coverages are compared as fractions.  Both return (records,
stats): a record is (unitig, why, n_node, kc, other) with why 1 for a tip and 2 for a popped arm and other the anchor end or the winning arm's end,
unitig << 1 | (1 for '-'); the records are listed by unitig ascending.
A round's result is the surviving {(k-mer, count)}; the next round restates the graph of that set with graph_util.  rounds() runs them, report()
writes what the command writes.  tests/test_clean.py holds the two to each other and to hand-derived cases, tests/test_clean_model.py the sequential
model of the kernels to them, tests/test_gpu_clean.py the device."""
import random
import struct
from fractions import Fraction

import numpy as np

import bubble_util as B
import gfa_util as G
import graph_util as U

KEEP, TIP, POP = 0, 1, 2
STAT0 = dict(n_tip=0, tip_nodes=0, n_tip_kept=0, n_pop=0, pop_nodes=0, n_pop_kept=0)


def _stats(ug, recs, n_cand, n_bubble):
    tips = [r for r in recs if r[1] == TIP]
    pops = [r for r in recs if r[1] == POP]
    return dict(n_tip=len(tips), tip_nodes=sum(r[2] for r in tips), n_tip_kept=n_cand - len(tips), n_pop=len(pops), pop_nodes=sum(r[2] for r in pops),
                n_pop_kept=n_bubble - len(pops))


def by_links(k, ug, links, bubbles, T, P):
    """the definitions, unitig by unitig and record by record, with integer products"""
    out = {}
    for f, t in links:
        out.setdefault(f, []).append(t)
    deg = lambda e: len(out.get(e, ()))
    n_of, kc_of = [u[1] for u in ug], [u[2] for u in ug]
    stronger = lambda j, i: kc_of[j] * n_of[i] > kc_of[i] * n_of[j] or (kc_of[j] * n_of[i] == kc_of[i] * n_of[j] and j < i)
    tipcand = lambda e: not ug[e >> 1][3] and n_of[e >> 1] < T and deg(e) == 1 and deg(e ^ 1) == 0
    why, n_cand = {}, 0
    for j, u in enumerate(ug):
        es = [e for e in (j << 1, j << 1 | 1) if tipcand(e)]
        if not es:
            continue
        assert len(es) == 1
        n_cand += 1
        e = es[0]
        a = out[e][0]
        if a >> 1 == j:
            continue
        assert e ^ 1 in out[a ^ 1], "a link without its mirror"
        if any(not tipcand(x ^ 1) or stronger(x >> 1, j) for x in out[a ^ 1] if x != e ^ 1):
            why[j] = (TIP, a)
    for s, t, (a1, a2), (n1, n2), (c1, c2), hd, typ in bubbles:
        lo, hi = ((a2, n2, c2), (a1, n1, c1)) if c1 * n2 >= c2 * n1 else ((a1, n1, c1), (a2, n2, c2))
        if P > 0 and 100 * lo[2] * hi[1] <= P * hi[2] * lo[1]:
            assert lo[0] >> 1 not in why, "an arm that is a tip, or an arm of two bubbles"
            why[lo[0] >> 1] = (POP, hi[0])
    recs = [(j, why[j][0], n_of[j], kc_of[j], why[j][1]) for j in sorted(why)]
    assert n_cand <= G.end_deg(ug, links)[0] and all(not ug[r[0]][3] for r in recs)
    return recs, _stats(ug, recs, n_cand, len(bubbles))


def by_strings(k, ug, T, P):
    """from the unitigs' strings alone, anchor by anchor, with fractions"""
    ends = [(e, B.oriented(ug, e)) for e in range(2 * len(ug))]
    head = {}
    for t, b in ends:
        head.setdefault(b[:k - 1], []).append((b[k - 1], t))
    out = {s: [t for _, t in sorted(head.get(a[len(a) - (k - 1):], ()))] for s, a in ends}
    cov = [Fraction(u[2], u[1]) for u in ug]
    cand = lambda e: not ug[e >> 1][3] and ug[e >> 1][1] < T and len(out[e]) == 1 and not out[e ^ 1]
    n_cand = sum(1 for e in range(2 * len(ug)) if cand(e))
    gone = {}
    for y in range(2 * len(ug)):                                 # y = a ^ 1: the end of an anchor that the unitigs of out(y) leave
        if ug[y >> 1][3]:
            continue
        tips = [x for x in out[y] if cand(x ^ 1) and x >> 1 != y >> 1]
        if not tips:
            continue
        if len(tips) == len(out[y]):                             # nothing but candidates: the strongest stays
            best = min(tips, key=lambda x: (-cov[x >> 1], x >> 1))
            tips = [x for x in tips if x != best]
        for x in tips:
            gone[x >> 1] = (TIP, y ^ 1)
    recs_b, bs = B.by_strings(k, ug)
    for r in recs_b:
        a1, a2 = r[2]
        lo, hi = (a2, a1) if cov[a1 >> 1] >= cov[a2 >> 1] else (a1, a2)
        if P > 0 and 100 * cov[lo >> 1] <= P * cov[hi >> 1]:
            assert lo >> 1 not in gone
            gone[lo >> 1] = (POP, hi)
    recs = [(j, gone[j][0], ug[j][1], ug[j][2], gone[j][1]) for j in sorted(gone)]
    return recs, _stats(ug, recs, n_cand, len(recs_b))


def image(k, ug, recs):
    """the drop image: the removed unitigs' strings in record order, each followed by a newline"""
    return "".join(ug[r[0]][0] + "\n" for r in recs).encode()


def as_rows(k, recs):
    """the records as the six words of yakamd_clean_rec_t"""
    rows, off = [], 0
    for j, why, n, kc, other in recs:
        rows.append((j, why, n, kc, other, off))
        off += n + k
    return rows


def kmer_int(s):
    v = 0
    for ch in s:
        v = v << 2 | "ACGT".index(ch)
    return v


def image_kmers(k, img):
    """the canonical k-mers of an image, as integers, every occurrence"""
    out = []
    for line in img.decode().split("\n"):
        out += [kmer_int(U.canon(line[i:i + k])) for i in range(len(line) - k + 1)]
    return out


def one_round(k, x, c, min_cnt, T, P, both=True):
    """a round on the table (x, c) in its listing order: a dict of the graph (st, ug, links, bubbles), the records, the stats, the image, the round's
    nine numbers and `gone`, the set of the removed k-mers.  both: the two restatements, which must agree"""
    recs_g, st = U.graph(k, x, c, min_cnt)
    ug = U.unitigs(k, recs_g, min_cnt)
    links = G.links_by_strings(k, ug)
    bub, bs = B.by_links(k, ug, links)
    recs, cs = by_links(k, ug, links, bub, T, P)
    if both:
        assert (recs, cs) == by_strings(k, ug, T, P)
    img = image(k, ug, recs)
    gone = image_kmers(k, img)
    assert len(set(gone)) == len(gone) == cs["tip_nodes"] + cs["pop_nodes"], "a removed node twice in the image"
    rnd = dict(n_key=len(x), n_unitig=len(ug), n_link=len(links), n_bubble=len(bub), n_tip=cs["n_tip"], tip_nodes=cs["tip_nodes"], n_pop=cs["n_pop"],
               pop_nodes=cs["pop_nodes"], removed=len(gone))
    return dict(st=st, ug=ug, links=links, bubbles=bub, bstats=bs, recs=recs, stats=cs, image=img, round=rnd, gone=set(gone))


def rounds(k, x, c, min_cnt=1, T=None, P=100, max_rounds=8, step=None, both=True):
    """the loop of yakamd_clean on the table (x, c): ([the dict of every round], n_key_in, n_key_after_shrink, (x, c) of the cleaned table).
    step(round, x, c) gives the table of the next round in its listing order; without it the survivors keep their order"""
    T = k if T is None else T
    x, c = np.asarray(x, np.uint64), np.asarray(c, np.int64)
    n_in = len(x)
    if min_cnt > 1:
        x, c = x[c >= min_cnt], c[c >= min_cnt]
    n_shrunk = len(x)
    done = []
    for r in range(max_rounds):
        d = one_round(k, x, c, min_cnt, T, P, both)
        done.append(d)
        if not d["gone"]:
            break
        if step:
            x, c = step(d, x, c)
        else:
            keep = np.array([int(v) not in d["gone"] for v in x], bool)
            x, c = x[keep], c[keep]
    return done, n_in, n_shrunk, (x, c)


def list_lines(r, recs):
    return "".join("%s\t%d\tu%d\t%d\t%d\t%s\n" % ("TP"[why - 1], r, j, n, kc, B.end_name(other)) for j, why, n, kc, other in recs)


def round_line(r, rnd):
    return "R\t%d\t" % r + "\t".join("%d" % rnd[f] for f in ("n_key", "n_unitig", "n_link", "n_bubble", "n_tip", "tip_nodes", "n_pop", "pop_nodes", "removed")) + "\n"


def head_line(k, min_cnt, T, P):
    return "#clean\tk=%d\tmin_cnt=%d\ttip_nodes=%d\tpop_pct=%d\n" % (k, min_cnt, T, P)


def report(k, min_cnt, T, P, done, n_in, n_shrunk, n_out, list_removed=False):
    out = [head_line(k, min_cnt, T, P)]
    for r, d in enumerate(done, 1):
        out.append(round_line(r, d["round"]))
        if list_removed:
            out.append(list_lines(r, d["recs"]))
    out.append("C\t%d\t%d\t%d\t%d\n" % (len(done), n_in, n_shrunk, n_out))
    return "".join(out).encode()


def table_set(k, x, c):
    return {(U.kmer_str(a, k), int(b)) for a, b in zip(x, c)}


def model_file(fn, k, min_cnt, T, P, n_key, desc, bases, links, bubbles):
    """what tests/tools/clean_model_check.cpp reads, all of it little-endian 64-bit words: k, min_cnt, tip_nodes, pop_pct, n_key, the numbers of
    unitigs, bases, links and bubbles; the descriptors (off, n_node, kc, first), the links (from, to), the bubble records (the ten words of
    yakamd_bubble_t); then the bases"""
    words = [k, min_cnt, T, P, n_key, len(desc), len(bases), len(links), len(bubbles)]
    for d in desc:
        words += list(d)
    for l in links:
        words += list(l)
    for b in bubbles:
        words += list(b)
    with open(fn, "wb") as f:
        f.write(struct.pack("<%dQ" % len(words), *words))
        f.write(bases)


# ---- the planted end-to-end case ----
def planted_reads(k, seed, n=2000, n_mid=12, n_end=8, read=150):
    """(the genome, the records): three copies of a random genome of n bases and reads of `read` bases cut from it with one changed base each --
    n_mid of them in the middle of the read (a bubble of k nodes, seen once against three), n_end within k - 1 bases of an end of the read (a tip of
    fewer than k nodes).  The reads are spaced so that no two errors share a k-mer"""
    rng = random.Random(seed)
    g = "".join(rng.choice("ACGT") for _ in range(n))
    recs = [g] * 3
    starts = list(range(k, n - read - k, (n - read - 2 * k) // (n_mid + n_end)))[:n_mid + n_end]
    at = []
    for i, s in enumerate(starts):
        r = list(g[s:s + read])
        d = 1 + (5 * i) % (k - 1)                                # 1 .. k - 1 bases from an end of the read: d nodes hold the error
        p = d - 1 if i < n_end // 2 else read // 2 if i < n_end // 2 + n_mid else read - d
        r[p] = rng.choice([b for b in "ACGT" if b != r[p]])
        recs.append("".join(r))
        at.append(s + p)
    assert all(b - a > k + 1 for a, b in zip(at, at[1:])), "two errors within k bases of each other"
    return g, recs
