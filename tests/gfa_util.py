"""The links between unitigs (`yak-amd unitigs -G`; include/yak_amd_gfa.h) restated twice over, and the command's two texts.
links_by_map() goes from the graph's records (graph_util.graph()) and the walk's map (walk_util.restate()): for every unlinked side of a node and
every set edge bit of that side, the neighbour's map entry gives the far unitig and its orientation.  links_by_strings() is independent of records
and map: every ordered pair of oriented open unitigs links where the last k - 1 bases of one are the first k - 1 of the other, and a cycle has its
two lines.  Both return [(from, to)] in the defined order -- by j, + before -, then by the base b that the link appends -- with from and to
unitig << 1 | (1 for '-').  tests/test_gfa.py holds the two to each other and to hand-derived cases, tests/test_gfa_model.py the sequential model of
the kernels to them, tests/test_gpu_gfa.py the device."""
import struct

import graph_util as U

NONE = U.NONE


def links_by_map(k, recs, min_cnt, ug, amap):
    n_of = [u[1] for u in ug]
    cyc = [u[3] for u in ug]
    pos = {r[0]: i for i, r in enumerate(recs) if r[3] >= min_cnt}
    mask = (1 << 2 * k) - 1
    rc = lambda z: int(U.H.revcomp([z], k)[0])
    out = []
    for v, (x, lr, ll, c, edges) in enumerate(recs):
        if c < min_cnt:
            continue
        j, at = amap[v]
        p, d = at >> 1, at & 1
        if cyc[j]:
            assert lr != NONE and ll != NONE
            continue
        for s, lk in ((0, lr), (1, ll)):
            if lk != NONE:
                continue
            # the oriented unitig that leaves through side s of v: (j, +) through the read side of its last node, (j, -) through the other side of its first
            if p == n_of[j] - 1 and s == d:
                o = 0
            else:
                assert p == 0 and s == d ^ 1, "an unlinked side inside a unitig"
                o = 1
            for b in range(4):
                if not edges >> (4 * s + b) & 1:
                    continue
                z = (x << 2 | b) & mask if s == 0 else x >> 2 | b << 2 * (k - 1)
                zo = z if s == 0 else rc(z)                      # Z as the oriented unitig reads it: W[1:] + bo
                bo = b if s == 0 else 3 - b
                y = min(z, rc(z))
                jj, att = amap[pos[y]]
                pp, dd = att >> 1, att & 1
                assert not cyc[jj], "an unlinked side next to a cycle"
                fwd = zo == y
                plus = pp == 0 and fwd == (dd == 0)
                minus = pp == n_of[jj] - 1 and fwd == (dd == 1)
                assert plus != minus, "the far side is no unlinked end side"
                out.append((j << 1 | o, bo, jj << 1 | (0 if plus else 1)))
    for j, c in enumerate(cyc):
        if c:
            out += [(j << 1, 0, j << 1), (j << 1 | 1, 0, j << 1 | 1)]
    out.sort()
    return [(f, t) for f, _, t in out]


def links_by_strings(k, ug, all_pairs=False):
    ends = []                                                    # (oriented id, string)
    for j, (s, n, kc, cyc) in enumerate(ug):
        if not cyc:
            ends += [(j << 1, s), (j << 1 | 1, U.rc_str(s))]
    out = []
    if all_pairs:
        for f, a in ends:
            for t, b in ends:
                if a[len(a) - (k - 1):] == b[:k - 1]:
                    out.append((f, "ACGT".index(b[k - 1]), t))
    else:
        head = {}
        for t, b in ends:
            head.setdefault(b[:k - 1], []).append((t, b))
        for f, a in ends:
            for t, b in head.get(a[len(a) - (k - 1):], ()):
                out.append((f, "ACGT".index(b[k - 1]), t))
    for j, u in enumerate(ug):
        if u[3]:
            out += [(j << 1, 0, j << 1), (j << 1 | 1, 0, j << 1 | 1)]
    out.sort()
    assert len({(f, b) for f, b, _ in out}) == len(out), "two links of one end through one base"
    return [(f, t) for f, _, t in out]


def end_deg(ug, links):
    """end_deg[d] = the oriented ends of open unitigs with d links"""
    n = {}
    for f, _ in links:
        n[f] = n.get(f, 0) + 1
    deg = [0] * 5
    for j, u in enumerate(ug):
        if not u[3]:
            deg[n.get(j << 1, 0)] += 1
            deg[n.get(j << 1 | 1, 0)] += 1
    return deg


def check_identities(st, ug, links):
    """what include/yak_amd_gfa.h promises of every list of links; st = the graph's tallies"""
    n_cycle = sum(1 for u in ug if u[3])
    assert len(set(links)) == len(links), "a line twice"
    assert len(links) == st["n_arc"] - st["n_linked_side"] + 2 * n_cycle
    have = set(links)
    assert all((t ^ 1, f ^ 1) in have for f, t in links), "a link without its mirror"
    deg = end_deg(ug, links)                                     # raises IndexError for an end of more than 4 links
    assert sum(deg) == 2 * (len(ug) - n_cycle)
    assert all(f >> 1 < len(ug) and t >> 1 < len(ug) for f, t in links)
    return deg


def gfa_text(k, ug, links):
    out = ["H\tVN:Z:1.0\n"]
    out += ["S\tu%d\t%s\tLN:i:%d\tKC:i:%d\tkm:f:%.1f\tcl:i:%d\n" % (j, s, len(s), kc, kc / n, cyc) for j, (s, n, kc, cyc) in enumerate(ug)]
    out += ["L\tu%d\t%s\tu%d\t%s\t%dM\n" % (f >> 1, "+-"[f & 1], t >> 1, "+-"[t & 1], k - 1) for f, t in links]
    return "".join(out).encode()


def stats_text(k, min_cnt, st, ug, links):
    return U.stats_text(k, min_cnt, st, ug) + ("G\t%d\t" % len(links) + "\t".join("%d" % d for d in end_deg(ug, links)) + "\n").encode()


def parse_gfa(text):
    """(segments [(name, bases)], links [(from, to)]) of a GFA text as written here"""
    seg, links = [], []
    for ln in text.decode().splitlines():
        f = ln.split("\t")
        if f[0] == "S":
            seg.append((f[1], f[2]))
        elif f[0] == "L":
            links.append((int(f[1][1:]) << 1 | (f[2] == "-"), int(f[3][1:]) << 1 | (f[4] == "-")))
    return seg, links


def model_file(fn, k, min_cnt, cap, st, ug, desc, bases):
    """what tests/tools/gfa_model_check.cpp reads, all of it little-endian 64-bit words: k, min_cnt, the capacity of the end table (0: the default),
    the number of unitigs and of bases, the graph's tallies (n_key, n_node, n_arc, n_linked_side, deg[5][5]), the U line's five numbers, the
    descriptors (off, n_node, kc, first); then the bases"""
    u = [int(v) for v in U.u_line(ug).split("\t")[1:]]
    words = [k, min_cnt, cap, len(desc), len(bases), st["n_key"], st["n_node"], st["n_arc"], st["n_linked_side"]]
    words += [st["deg"][l][r] for l in range(5) for r in range(5)] + u
    for d in desc:
        words += list(d)
    with open(fn, "wb") as f:
        f.write(struct.pack("<%dQ" % len(words), *words))
        f.write(bases)


def n_keys(ug):
    """the keys of the end table: the first and, for more than one node, the last node of every open unitig"""
    return sum((2 if u[1] > 1 else 1) for u in ug if not u[3])
