"""`yak-amd unitigs` restated: the de Bruijn graph of a count table's k-mers, its links and its unitigs -- twice over.
graph() / unitigs() are the integer formulation of the definition on hetmer_util.members() of a dump: the records yakamd_graph_nodes_dev writes, the
tallies of yakamd_graph_stats, the unitigs in their defined order and orientation and the command's two texts.  brute() is independent of it: the
k-mers as strings in both orientations, an arc u -> v compactable iff outdeg(u) = indeg(v) = 1 and canon(u) != canon(v); it gives the set of
unitigs as canonical strings, a cycle as the set of its nodes.  tests/test_graph.py holds the two to each other and to hand-derived cases; the
device is held to graph() by tests/test_gpu_graph.py, the host walk of yak_amd/csrc/unitig_walk.h by tests/test_unitig_walk.py."""
import struct

import numpy as np

import hetmer_util as H

NONE = (1 << 64) - 1
members, kmer_str, rc_str, image, fasta = H.members, H.kmer_str, H.rc_str, H.image, H.fasta


def popcount4(v):
    v = np.asarray(v, np.int64)
    return (v & 1) + (v >> 1 & 1) + (v >> 2 & 1) + (v >> 3 & 1)


def extend(x, s, b, k):
    """z: x with base b appended (side 0, R) or prepended (side 1, L)"""
    x = np.asarray(x, np.uint64)
    if s == 0:
        return (x << np.uint64(2) | np.uint64(b)) & np.uint64((1 << 2 * k) - 1)
    return x >> np.uint64(2) | np.uint64(b << 2 * (k - 1))


def graph(k, x, c, min_cnt):
    """(records [(x, link_r, link_l, count, edges)] per stored key in listing order, stats dict) by the integer formulation"""
    assert k % 2 == 1 and k < 32 and 1 <= min_cnt <= 1023
    x, c = np.asarray(x, np.uint64), np.asarray(c, np.int64)
    n = len(x)
    is_node = c >= min_cnt
    ids = np.flatnonzero(is_node)
    order = ids[np.argsort(x[ids], kind="stable")]
    sx = x[order]

    def find(y):
        """the listing index of y where it is a node, else -1"""
        if len(sx) == 0:
            return np.full(len(y), -1, np.int64)
        at = np.minimum(np.searchsorted(sx, y), len(sx) - 1)
        return np.where(sx[at] == y, order[at], -1).astype(np.int64)

    edges = np.zeros(n, np.int64)
    for s in (0, 1):
        for b in range(4):
            z = extend(x, s, b, k)
            y = np.minimum(z, H.revcomp(z, k))
            edges |= ((find(y) >= 0) & is_node).astype(np.int64) << (4 * s + b)
    link = np.full((n, 2), -1, np.int64)
    face = np.zeros((n, 2), np.int64)
    for s in (0, 1):
        nib = edges >> 4 * s & 15
        one = popcount4(nib) == 1
        b = np.where(one, np.log2(np.maximum(nib, 1)).astype(np.int64), 0)
        z = np.where(s == 0, (x << np.uint64(2) | b.astype(np.uint64)) & np.uint64((1 << 2 * k) - 1),
                     x >> np.uint64(2) | b.astype(np.uint64) << np.uint64(2 * (k - 1))).astype(np.uint64)
        y = np.minimum(z, H.revcomp(z, k))
        t = np.where(y == z, 1 - s, s)                           # from R: L if y == z, else R; from L: R if y == z, else L
        at = find(y)
        ok = one & (y != x) & (at >= 0)
        deg_y = popcount4(edges[np.maximum(at, 0)] >> (4 * t) & 15)
        ok &= deg_y == 1
        link[:, s] = np.where(ok, at, -1)
        face[:, s] = t
    recs = []
    for i in range(n):
        lk = [NONE if link[i, s] < 0 else int(link[i, s]) << 1 | int(face[i, s]) for s in (0, 1)]
        recs.append((int(x[i]), lk[0], lk[1], int(c[i]), int(edges[i])))
    deg = [[0] * 5 for _ in range(5)]
    l, r = popcount4(edges >> 4), popcount4(edges & 15)
    for i in ids:
        deg[l[i]][r[i]] += 1
    st = dict(n_key=n, n_node=len(ids), n_arc=int((l + r)[ids].sum()), n_linked_side=int((link[ids] >= 0).sum()), deg=deg)
    return recs, st


def unitigs(k, recs, min_cnt):
    """[(bases, n_node, sum of counts, is a cycle)] in output order: open unitigs ascending by the listing index of their start node -- the end node
    with the smaller index, read away from its unlinked side, a node without links as stored -- then cycles, ascending by their smallest index, from
    that node as stored through R"""
    comp = 3
    seen = set()
    out = []

    def walk(v, d, cyc):
        x = recs[v][0]
        s = kmer_str(x, k) if d == 0 else rc_str(kmer_str(x, k))
        nodes, kc = [v], recs[v][3]
        while True:
            lk = recs[v][1 + d]
            if lk == NONE:
                break
            v, d = lk >> 1, (lk & 1) ^ 1
            if cyc and v == nodes[0]:
                assert d == 0
                break
            assert v not in nodes[-1:] and len(nodes) <= len(recs)
            nodes.append(v)
            kc += recs[v][3]
            xv = recs[v][0]
            s += "ACGT"[xv & 3] if d == 0 else "ACGT"[comp - (xv >> 2 * (k - 1) & 3)]
        return s, nodes, kc

    for i, r in enumerate(recs):
        if r[3] < min_cnt:
            continue
        free = [s for s in (0, 1) if r[1 + s] == NONE]
        if not free:
            continue
        d = 0 if len(free) == 2 else free[0] ^ 1
        s, nodes, kc = walk(i, d, False)
        if nodes[-1] < i:
            continue
        assert len(free) == 2 or nodes[-1] > i
        assert not seen.intersection(nodes)
        seen.update(nodes)
        out.append((s, len(nodes), kc, 0))
    for i, r in enumerate(recs):
        if r[3] < min_cnt or i in seen:
            continue
        s, nodes, kc = walk(i, 0, True)
        assert min(nodes) == i and not seen.intersection(nodes)
        seen.update(nodes)
        out.append((s, len(nodes), kc, 1))
    assert len(seen) == sum(1 for r in recs if r[3] >= min_cnt), "a node in no unitig"
    return out


def fasta_text(ug):
    return "".join(">u%d\tLN:i:%d\tKC:i:%d\tkm:f:%.1f\tCL:i:%d\n%s\n" % (j, len(s), kc, kc / n, cyc, s) for j, (s, n, kc, cyc) in enumerate(ug)).encode()


def u_line(ug):
    lens = sorted((len(u[0]) for u in ug), reverse=True)
    tot, acc, n50 = sum(lens), 0, 0
    for v in lens:
        acc += v
        if 2 * acc >= tot:
            n50 = v
            break
    return "U\t%d\t%d\t%d\t%d\t%d\n" % (sum(1 for u in ug if not u[3]), sum(1 for u in ug if u[3]), tot, lens[0] if lens else 0, n50)


def stats_text(k, min_cnt, st, ug):
    out = ["#unitigs\tk=%d\tmin_cnt=%d\n" % (k, min_cnt), "N\t%d\t%d\t%d\t%d\n" % (st["n_key"], st["n_node"], st["n_arc"], st["n_linked_side"])]
    out += ["D\t%d\t%d\t%d\n" % (l, r, st["deg"][l][r]) for l in range(5) for r in range(5) if st["deg"][l][r]]
    return ("".join(out) + u_line(ug)).encode()


def record_file(fn, k, min_cnt, recs):
    """what tests/tools/unitig_walk_check.cpp reads: k, min_cnt, the number of records, then the 32-byte records"""
    with open(fn, "wb") as f:
        f.write(struct.pack("<IIQ", k, min_cnt, len(recs)))
        f.write(b"".join(struct.pack("<QQQII", x, a, b, c, e) for x, a, b, c, e in recs))


def canon(s):
    return min(s, rc_str(s))


def as_sets(k, ug):
    """the unitigs as brute() gives them: (sorted canonical strings of the open ones, set of frozensets of the cycles' canonical k-mers)"""
    opens = sorted(canon(s) for s, n, kc, cyc in ug if not cyc)
    cycles = {frozenset(canon(s[i:i + k]) for i in range(n)) for s, n, kc, cyc in ug if cyc}
    assert len(cycles) == sum(1 for u in ug if u[3])
    return opens, cycles


def brute(k, x, c, min_cnt):
    """the same two sets from strings alone: every node in both orientations, arcs by overlap of k - 1, maximal paths of compactable arcs"""
    S = set()
    for xi, ci in zip(x, c):
        if ci >= min_cnt:
            s = kmer_str(xi, k)
            S.update((s, rc_str(s)))
    succ = lambda u: [u[1:] + b for b in "ACGT" if u[1:] + b in S]
    pred = lambda v: [b + v[:-1] for b in "ACGT" if b + v[:-1] in S]
    nxt, prv = {}, {}
    for u in S:
        su = succ(u)
        if len(su) == 1 and len(pred(su[0])) == 1 and canon(u) != canon(su[0]):
            nxt[u] = su[0]
            prv[su[0]] = u
    opens, done = set(), set()
    for u in S:
        if u in prv:
            continue
        s, v = u, u
        done.add(u)
        while v in nxt:
            v = nxt[v]
            assert v not in done or v == u
            done.add(v)
            s += v[-1]
        opens.add(canon(s))
    cycles = set()
    for u in S:
        if u in done:
            continue
        nodes, v = [], u
        while v not in done:
            done.add(v)
            nodes.append(canon(v))
            v = nxt[v]
        assert v == u
        cycles.add(frozenset(nodes))
    return sorted(opens), cycles
