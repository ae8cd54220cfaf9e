"""The simple bubbles of the unitig graph (`yak-amd bubbles`; include/yak_amd_bubble.h) restated twice over, and the command's
two texts.  by_links() applies the definition to the link list of gfa_util and the unitigs of graph_util.  by_strings() is independent of the link
list: for every ordered choice of oriented unitigs s -> a holds iff the last k - 1 bases of s are the first k - 1 of a, out(s) is ordered by the base
a appends, and all degrees are counted from that relation.  Both return (records, stats): a record is (src, sink, (a1, a2), (n1, n2), (kc1, kc2), hd,
type) with every end unitig << 1 | (1 for '-'), hd None for arms of two lengths and type one of "SEI"; the records are listed by src ascending.
tests/test_bubble.py holds the two to each other and to hand-derived cases, tests/test_bubble_model.py the sequential model of the kernels to them,
tests/test_gpu_bubble.py the device.  planted() makes the genomes with variants of known types that those tests share."""
import random
import struct

import gfa_util as G
import graph_util as U

NO_HD = (1 << 64) - 1


def oriented(ug, e):
    s = ug[e >> 1][0]
    return U.rc_str(s) if e & 1 else s


def _apply(k, ug, out):
    """the definition, given out(e) for every oriented end e"""
    deg = lambda e: len(out.get(e, ()))
    is_open = lambda e: not ug[e >> 1][3]
    recs = []
    n_fork = n_tip = tip_nodes = max_arm = 0
    for j, u in enumerate(ug):
        if u[3]:
            continue
        n_fork += sum(1 for e in (j << 1, j << 1 | 1) if deg(e) >= 2)
        d0, d1 = deg(j << 1), deg(j << 1 | 1)
        if u[1] < k and (d0 == 0) != (d1 == 0):
            n_tip += 1
            tip_nodes += u[1]
    for s in range(2 * len(ug)):
        if not is_open(s) or deg(s) != 2:
            continue
        a1, a2 = out[s]
        if a1 >> 1 == a2 >> 1 or s >> 1 in (a1 >> 1, a2 >> 1):
            continue
        if any(deg(a ^ 1) != 1 or deg(a) != 1 for a in (a1, a2)):
            continue
        t = out[a1][0]
        if out[a2][0] != t or deg(t ^ 1) != 2 or t >> 1 in (a1 >> 1, a2 >> 1):
            continue
        assert s != t ^ 1
        if not s < (t ^ 1):
            continue
        n1, n2 = ug[a1 >> 1][1], ug[a2 >> 1][1]
        A1, A2 = oriented(ug, a1), oriented(ug, a2)
        hd = sum(1 for x, y in zip(A1, A2) if x != y) if n1 == n2 else None
        typ = "I" if n1 != n2 else "S" if n1 == k else "E"
        recs.append((s, t, (a1, a2), (n1, n2), (ug[a1 >> 1][2], ug[a2 >> 1][2]), hd, typ))
        max_arm = max(max_arm, n1, n2)
    st = dict(n_bubble=len(recs), n_type=[sum(1 for r in recs if r[6] == c) for c in "SEI"], n_tip=n_tip, tip_nodes=tip_nodes, max_arm_nodes=max_arm, n_fork=n_fork)
    return recs, st


def by_links(k, ug, links):
    out = {}
    for f, t in links:                                           # the list is sorted by from, then by the base
        out.setdefault(f, []).append(t)
    return _apply(k, ug, out)


def by_strings(k, ug):
    ends = [(e, oriented(ug, e)) for e in range(2 * len(ug))]
    head = {}
    for t, b in ends:
        head.setdefault(b[:k - 1], []).append((b[k - 1], t))
    out = {}
    for s, a in ends:
        nxt = sorted(head.get(a[len(a) - (k - 1):], ()))
        assert len({b for b, _ in nxt}) == len(nxt), "two links of one end through one base"
        if nxt:
            out[s] = [t for _, t in nxt]
    return _apply(k, ug, out)


def allele(k, ug, a):
    s = oriented(ug, a)[k - 1:ug[a >> 1][1]]
    return s if s else "*"


def end_name(e):
    return "u%d%s" % (e >> 1, "+-"[e & 1])


def text(k, min_cnt, ug, recs):
    out = ["#bubbles\tk=%d\tmin_cnt=%d\n" % (k, min_cnt)]
    for i, (s, t, (a1, a2), (n1, n2), (c1, c2), hd, typ) in enumerate(recs):
        out.append("B\t%d\t%s\t%s\t%s\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%s\t%s\n" % (i, end_name(s), end_name(a1), end_name(a2), end_name(t), typ, n1, n2,
                                                                              "." if hd is None else "%d" % hd, c1, c2, allele(k, ug, a1), allele(k, ug, a2)))
    return "".join(out).encode()


def stats_line(st):
    return ("B\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (st["n_bubble"], st["n_type"][0], st["n_type"][1], st["n_type"][2], st["n_fork"], st["n_tip"], st["tip_nodes"],
                                                      st["max_arm_nodes"])).encode()


def stats_text(k, min_cnt, gst, ug, links, st):
    """the -s text: that of `unitigs -G -s` and the B line"""
    return G.stats_text(k, min_cnt, gst, ug, links) + stats_line(st)


def as_rows(recs):
    """the records as the ten words of yakamd_bubble_t"""
    return [(s, t, a1, a2, n1, n2, c1, c2, NO_HD if hd is None else hd, "SEI".index(typ)) for s, t, (a1, a2), (n1, n2), (c1, c2), hd, typ in recs]


def middle_pairs(k, ug, recs):
    """for every S bubble the two k-mers around the differing base, canonical, as a sorted pair of strings"""
    h = (k - 1) // 2
    return [tuple(sorted(U.canon(oriented(ug, a)[h:h + k]) for a in r[2])) for r in recs if r[6] == "S"]


def check_invariants(k, ug, recs, st):
    assert sum(st["n_type"]) == st["n_bubble"] == len(recs)
    assert [r[0] for r in recs] == sorted(r[0] for r in recs) and len({r[0] for r in recs}) == len(recs)
    seen = {(r[0], r[1]) for r in recs}
    assert not any((t ^ 1, s ^ 1) in seen for s, t in seen), "a bubble listed from both sides"
    for s, t, arms, (n1, n2), kc, hd, typ in recs:
        assert (hd is None) == (typ == "I") and (typ != "S" or hd == 1) and (typ != "E" or hd >= 2), (typ, hd)
        assert typ != "S" or [i for i, (x, y) in enumerate(zip(oriented(ug, arms[0]), oriented(ug, arms[1]))) if x != y] == [k - 1]


def model_file(fn, k, min_cnt, gst, ug, desc, bases, links, end_deg=None):
    """what tests/tools/bubble_model_check.cpp reads, all of it little-endian 64-bit words: k, min_cnt, the numbers of unitigs, bases and links, the
    graph's tallies (n_key, n_node, n_arc, n_linked_side, deg[5][5]), the U line's five numbers, end_deg[5]; the descriptors (off, n_node, kc,
    first), the links (from, to); then the bases.  end_deg: of the list as it was before a test damaged it"""
    u = [int(v) for v in U.u_line(ug).split("\t")[1:]]
    words = [k, min_cnt, len(desc), len(bases), len(links), gst["n_key"], gst["n_node"], gst["n_arc"], gst["n_linked_side"]]
    words += [gst["deg"][l][r] for l in range(5) for r in range(5)] + u + (end_deg or G.end_deg(ug, links))
    for d in desc:
        words += list(d)
    for l in links:
        words += list(l)
    with open(fn, "wb") as f:
        f.write(struct.pack("<%dQ" % len(words), *words))
        f.write(bases)


# ---- planted genomes ----
def planted(k, n, seed, circular=False, kinds="SEI"):
    """(the two haplotypes as strings, the variants [(type, n_node of the two arms sorted)]) of a random genome of about n bases: SNPs (S), pairs of
    SNPs three to k - 1 bases apart (E) and insertions or deletions of 1 to 3 bases (I), more than 2 k apart and from the ends.  A circular genome's
    strings have their first k - 1 bases again behind them.  What a variant must give: S arms of k nodes; E arms of k + d nodes, hd 2; I arms of
    k - 1 and k - 1 + d nodes -- unless a chance repeat hides it, which the caller's seed rules out"""
    rng = random.Random(seed)
    g = [rng.choice("ACGT") for _ in range(n)]
    other = lambda b: rng.choice([c for c in "ACGT" if c != b])
    alt, want = [], []
    step = 2 * k + 4 + 3
    p, i = step, 0
    prev = 0
    while p + step < n:
        kind = kinds[i % len(kinds)]
        alt.append("".join(g[prev:p]))
        if kind == "S":
            alt.append(other(g[p]))
            prev = p + 1
            want.append(("S", (k, k)))
        elif kind == "E":
            d = rng.randint(3, k - 1)
            alt.append(other(g[p]) + "".join(g[p + 1:p + d]) + other(g[p + d]))
            prev = p + d + 1
            want.append(("E", (k + d, k + d)))
        else:                                                    # neither end of what goes or comes repeats its neighbour: the gap cannot shift
            d = rng.randint(1, 3)
            if rng.random() < 0.5:                               # a deletion from the second haplotype
                while g[p] == g[p + d] or g[p + d - 1] == g[p - 1]:
                    alt[-1] += g[p]
                    p += 1
                prev = p + d
            else:
                alt.append("".join([other(g[p])] + [rng.choice("ACGT") for _ in range(d - 2)] + ([other(g[p - 1])] if d > 1 else [])))
                if d == 1 and alt[-1] == g[p - 1]:
                    alt[-1] = [c for c in "ACGT" if c not in (g[p], g[p - 1])][0]
                prev = p
            want.append(("I", (k - 1, k - 1 + d)))
        p = prev + step + rng.randint(0, 5) + (k if kind == "E" else 0)
        i += 1
    alt.append("".join(g[prev:]))
    a, b = "".join(g), "".join(alt)
    if circular:
        a, b = a + a[:k - 1], b + b[:k - 1]
    return [a, b], want


def found(recs):
    return sorted((r[6], tuple(sorted(r[3]))) for r in recs)
