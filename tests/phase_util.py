"""The phasing of the bubbles' alleles from read support (`yak-amd bubbles -r -p`; include/yak_amd_phase.h) restated twice
over, and the command's text.  The votes: votes_flat() goes from observation records as allele_util.flat() makes them, votes_from_f_lines() from the F
lines of allele_util's text alone.  The solve: kruskal() takes the edges in the order of the definition with a union-find that carries parity;
by_definition() takes the blocks by flood fill, calls an edge a forest edge iff the edges before it do not join its ends, takes h by a search over
that forest, and then checks the forest by the cycle property.  tests/test_phase.py holds the two to each other and to hand-derived cases,
tests/test_phase_model.py the sequential model of the kernels to them, tests/test_gpu_phase.py the device."""
import struct

import allele_util as A
import bubble_util as B

FULL = A.FULL
NONE = (1 << 32) - 1
X, FOREST, DISC = 1, 2, 4


# ---- the votes ----
def add_votes(votes, frag):
    """the votes of one fragment [(bubble, a)] into {(i, j): [cis, trans]}; returns their number"""
    n = 0
    for (b1, a1), (b2, a2) in zip(frag, frag[1:]):
        if b1 != b2:
            votes.setdefault((min(b1, b2), max(b1, b2)), [0, 0])[a1 != a2] += 1
            n += 1
    return n


def votes_flat(chunks_obs, votes=None):
    """(votes, n_full, n_vote) of the records of chunks [[(seq, bubble, flags, ...)]]: a fragment is the full records of one seq of one chunk"""
    votes = {} if votes is None else votes
    n_full = n_vote = 0
    for obs in chunks_obs:
        per = {}
        for o in obs:
            if o[2] & FULL:
                per.setdefault(o[0], []).append((o[1], o[2] & 1))
                n_full += 1
        for seq in sorted(per):
            n_vote += add_votes(votes, per[seq])
    return votes, n_full, n_vote


def votes_from_f_lines(lines):
    """the same from `F name n i:<1|2><+|-> ...` lines"""
    votes, n_full, n_vote = {}, 0, 0
    for ln in lines:
        f = ln.rstrip("\n").split("\t")
        assert f[0] == "F" and int(f[2]) == len(f) - 3
        frag = [(int(e.split(":")[0]), int(e.split(":")[1][0]) - 1) for e in f[3:]]
        n_full += len(frag)
        n_vote += add_votes(votes, frag)
    return votes, n_full, n_vote


def edges_of(sup, votes, min_sup, min_link):
    """[(w, i, j, x, cis, trans)] in the order of the definition: the larger w first, then the smaller (i, j)"""
    het = [A.call(s, min_sup) == "het" for s in sup]
    out = []
    for (i, j), (c, t) in votes.items():
        if het[i] and het[j] and abs(c - t) >= min_link:
            out.append((abs(c - t), i, j, int(t > c), c, t))
    return sorted(out, key=lambda e: (-e[0], e[1], e[2])), het


def summary(n_bubble, het, edges, forest, h, block):
    """the result in one shape for both solves: nodes [(block, h) or None], edges {(i, j): (w, x, kind, cis, trans)}, blocks [(block, n_bubble,
    n_edge, n_disc, w_sum, w_disc)] of two or more, and the tallies"""
    nodes = [(block[b], h[b]) if het[b] else None for b in range(n_bubble)]
    per = {}
    for b in range(n_bubble):
        if het[b]:
            per.setdefault(block[b], [0, 0, 0, 0, 0])[0] += 1
    ed = {}
    for w, i, j, x, c, t in edges:
        kind = "forest" if (i, j) in forest else "conc" if x == h[i] ^ h[j] else "disc"
        ed[(i, j)] = (w, x, kind, c, t)
        p = per[block[i]]
        p[1] += 1; p[3] += w
        if kind == "disc":
            p[2] += 1; p[4] += w
    blocks = [(nm,) + tuple(p) for nm, p in sorted(per.items()) if p[0] >= 2]
    st = dict(n_het=sum(het), n_edge=len(edges), n_forest=len(forest), n_block=len(blocks), n_single=sum(1 for p in per.values() if p[0] == 1),
              n_disc=sum(b[3] for b in blocks), max_block=max([p[0] for p in per.values()] + [0]))
    assert st["n_forest"] == st["n_het"] - st["n_block"] - st["n_single"]
    return dict(nodes=nodes, edges=ed, blocks=blocks, stats=st)


def kruskal(n_bubble, sup, votes, min_sup=2, min_link=2):
    """restatement 1: Kruskal's algorithm over the ordered edges with a union-find that carries the parity against the root"""
    edges, het = edges_of(sup, votes, min_sup, min_link)
    up, par = list(range(n_bubble)), [0] * n_bubble

    def find(b):
        """(the root of b, the parity of b against it); the path is compressed behind the search"""
        path, p = [], 0
        while up[b] != b:
            path.append(b)
            b = up[b]
        for a in reversed(path):
            p ^= par[a]
            up[a], par[a] = b, p
        return b, p

    forest = set()
    for w, i, j, x, c, t in edges:
        (ri, pi), (rj, pj) = find(i), find(j)
        if ri != rj:
            forest.add((i, j))
            up[ri], par[ri] = rj, pi ^ pj ^ x
    block, h = [None] * n_bubble, [0] * n_bubble
    name = {}
    for b in range(n_bubble):
        if het[b]:
            name.setdefault(find(b)[0], b)
    for b in range(n_bubble):
        if het[b]:
            block[b] = name[find(b)[0]]
            h[b] = find(b)[1] ^ find(block[b])[1]
    return summary(n_bubble, het, edges, forest, h, block)


def by_definition(n_bubble, sup, votes, min_sup=2, min_link=2):
    """restatement 2: the blocks by flood fill over all edges; an edge is a forest edge iff the edges before it in the order do not join its two
    bubbles; h by a search over the forest from the block's name; then the cycle property: a non-forest edge comes behind every edge of the forest
    path between its two bubbles"""
    edges, het = edges_of(sup, votes, min_sup, min_link)

    def reach(start, es):
        adj = {}
        for e in es:
            adj.setdefault(e[1], []).append((e[2], e)); adj.setdefault(e[2], []).append((e[1], e))
        seen, todo = {start: (0, [])}, [start]                    # bubble -> (parity against start, the edges of the path)
        while todo:
            b = todo.pop()
            for nb, e in adj.get(b, []):
                if nb not in seen:
                    seen[nb] = (seen[b][0] ^ e[3], seen[b][1] + [e])
                    todo.append(nb)
        return seen

    block = [None] * n_bubble
    for b in range(n_bubble):
        if het[b] and block[b] is None:
            for nb in reach(b, edges):
                block[nb] = b
    forest = {(e[1], e[2]) for at, e in enumerate(edges) if e[2] not in reach(e[1], edges[:at])}
    fe = [e for e in edges if (e[1], e[2]) in forest]
    h = [0] * n_bubble
    for b in range(n_bubble):
        if het[b] and block[b] == b:
            for nb, (p, path) in reach(b, fe).items():
                h[nb] = p
    rank = {(e[1], e[2]): at for at, e in enumerate(edges)}
    for e in edges:
        if (e[1], e[2]) not in forest:
            p, path = reach(e[1], fe)[e[2]]
            assert all(rank[(f[1], f[2])] < rank[(e[1], e[2])] for f in path), "a non-forest edge before an edge of its cycle"
    return summary(n_bubble, het, edges, forest, h, block)


# ---- the text ----
def lines_of(res, edges):
    out = ["H\t%d\t%d\t%d\n" % (b, n[0], n[1]) for b, n in enumerate(res["nodes"]) if n is not None]
    out += ["K\t%d\t%d\t%d\t%d\t%d\t%d\n" % b for b in res["blocks"]]
    if edges:
        out += ["E\t%d\t%d\t%d\t%d\t%s\n" % (i, j, e[3], e[4], e[2]) for (i, j), e in sorted(res["edges"].items())]
    return out


def text(k, min_cnt, min_sup, min_link, edges, stats_only, recs, sup, head, votes, n_vote, res):
    """the text of the command: head = [n_seq, sum_len, n_path, n_step, n_obs, n_full]; it does not depend on the chunks"""
    out = ["#phase\tk=%d\tmin_cnt=%d\tmin_sup=%d\tmin_link=%d\n" % (k, min_cnt, min_sup, min_link)]
    if not stats_only:
        out += A.allele_lines(recs, sup, min_sup) + lines_of(res, edges)
    st = res["stats"]
    tail = list(head) + [n_vote, len(votes), len(sup), st["n_het"], st["n_edge"], st["n_forest"], st["n_disc"], st["n_block"], st["n_single"], st["max_block"]]
    out.append("T\t%s\n" % "\t".join("%d" % v for v in tail))
    return "".join(out).encode()


def whole(k, ug, recs, reads, min_sup=2, min_link=2, chunk_size=1 << 28):
    """everything the restatement says of reads on the unitigs ug with the bubble records recs, cut into chunks of chunk_size bases"""
    per = [A.flat(k, ug, recs, [reads[i] for i in part]) for part in A.chunks(reads, chunk_size)]
    votes, n_full, n_vote = votes_flat([d["obs"] for d in per])
    sup = [tuple(sum(d["sup"][i][x] for d in per) for x in range(4)) for i in range(len(recs))]
    head = [len(reads), sum(len(r) for r in reads), sum(len(d["paths"]) for d in per), sum(len(d["steps"]) for d in per), sum(len(d["obs"]) for d in per), n_full]
    res = kruskal(len(recs), sup, votes, min_sup, min_link)
    return dict(per=per, votes=votes, n_full=n_full, n_vote=n_vote, sup=sup, head=head, res=res)


# ---- the model of the kernels ----
def model_file(fn, k, min_cnt, min_sup, min_link, edges, stats_only, recs, sup, chunks_obs, chunk_heads):
    """what tools/phase_model_check.cpp reads (little-endian 64-bit words unless stated): k, min_cnt, min_sup, min_link, edges, stats_only, the
    numbers of bubbles, of support entries and of chunks; the bubble records (ten words each); the support (four words each); per chunk n_seq, its
    bases, n_path, n_step, n_obs and the observation records (four 32-bit words each)"""
    rows = B.as_rows(recs)
    out = [struct.pack("<9Q", k, min_cnt, min_sup, min_link, int(edges), int(stats_only), len(recs), len(sup), len(chunks_obs))]
    out += [struct.pack("<10Q", *r) for r in rows]
    out += [struct.pack("<4Q", *s) for s in sup]
    for obs, hd in zip(chunks_obs, chunk_heads):
        out.append(struct.pack("<5Q", *(list(hd) + [len(obs)])))
        out += [struct.pack("<4I", *o[:4]) for o in obs]
    with open(fn, "wb") as f:
        f.write(b"".join(out))


def fake_recs(n_bubble):
    """bubble records for vote tables of the test's own making: bubble i has the arms u<2i>+ and u<2i+1>+; only the arms reach the A lines"""
    return [(0, 0, (4 * i, 4 * i + 2), (1, 1), (1, 1), None, "S") for i in range(n_bubble)]


def obs_of_votes(votes, rng=None):
    """observation records whose votes are `votes` {(i, j): [cis, trans]}: a fragment of two full records per vote, with partial records between"""
    obs, seq = [], 0
    for (i, j), (c, t) in sorted(votes.items()):
        for n, trans in ((c, 0), (t, 1)):
            for _ in range(n):
                a = rng.randrange(2) if rng else 0
                first, second = (i, a), (j, a ^ trans)
                if rng and rng.randrange(2):
                    first, second = second, first
                obs.append((seq, first[0], FULL | first[1] | (4 if rng and rng.randrange(2) else 0), 0))
                if rng and rng.randrange(3) == 0:
                    obs.append((seq, rng.choice((i, j)), rng.randrange(2), 0))       # a partial record between the two
                obs.append((seq, second[0], FULL | second[1], 0))
                seq += 1
    return obs


# ---- planted diploids ----
def diploid(rng, n=3000, gap=400, lo=25, hi=70):
    """(haplotype A, haplotype B, the SNP positions, the first position behind the long gap): SNPs lo to hi bases apart, and once `gap` bases"""
    a = [rng.choice("ACGT") for _ in range(n)]
    b = list(a)
    pos, p, behind = [], 60, None
    while p < n - 60:
        pos.append(p)
        b[p] = rng.choice([c for c in "ACGT" if c != a[p]])
        p += rng.randint(lo, hi)
        if behind is None and p >= n // 2:
            p += gap
            behind = p
    return "".join(a), "".join(b), pos, behind


def diploid_reads(rng, haps, n_reads, length=250):
    """error-free reads of about `length` bases, from the two haplotypes in turn, every third one from the other strand"""
    import graph_util as U
    out = []
    for it in range(n_reads):
        h = haps[it & 1]
        ln = rng.randint(length - 30, length + 30)
        x = rng.randrange(0, len(h) - ln)
        s = h[x:x + ln]
        out.append((U.rc_str(s) if it % 3 == 0 else s).encode())
    return out
