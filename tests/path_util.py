"""`yak-amd paths` (include/yak_amd_path.h) restated twice over, and the command's two texts.  hits_by_strings() goes from the
unitigs' strings alone: a dict from every k-substring of every S_j and of revcomp(S_j) to (j, p, o).  hits_by_ints() goes from the graph's records
(graph_util.graph()) and the walk's map (walk_util.restate()): the canonical value of Q_i is looked for in the listing, the map entry gives
(unitig, p << 1 | d), and o = d ^ (Q_i is not canonical).  Both return hit[] as a list of ints over the bytes of a base image.  chain() forms the
steps and the paths of a hit array with itertools.groupby and the tallies per sequence; check_rules() asserts what the header promises of them.
tests/test_path.py holds the two to each other and to hand-derived cases, tests/test_path_model.py the sequential model of the kernels to them,
tests/test_gpu_path.py the device."""
import bisect
import itertools
import struct

import graph_util as U

NONE, ABSENT = (1 << 64) - 1, (1 << 64) - 2
CODE = {}
for _i, (_a, _b) in enumerate(zip(b"ACGT", b"acgt")):
    CODE[_a] = CODE[_b] = CODE[_i] = _i
CODE[ord("U")] = CODE[ord("u")] = 3


def image(seqs):
    """(image, off, len) of sequences given as bytes: each followed by a newline"""
    off, at = [], 0
    for s in seqs:
        off.append(at)
        at += len(s) + 1
    return b"".join(s + b"\n" for s in seqs), off, [len(s) for s in seqs]


def windows(k, img):
    """per byte i of the image: Q_i as a string over ACGT, or None where no k-mer ends"""
    out, run = [], ""
    for b in img:
        run = run[-(k - 1):] + "ACGT"[CODE[b]] if b in CODE else ""
        out.append(run if len(run) == k else None)
    return out


def hits_by_strings(k, ug, img):
    where = {}
    for j, (s, n, kc, cyc) in enumerate(ug):
        r = U.rc_str(s)
        for p in range(n):
            for key, val in ((s[p:p + k], (j, p, 0)), (r[n - 1 - p:n - 1 - p + k], (j, p, 1))):
                assert key not in where, "a node in two places, or equal to its reverse complement"
                where[key] = val
    out = []
    for q in windows(k, img):
        if q is None:
            out.append(NONE)
        elif q not in where:
            out.append(ABSENT)
        else:
            j, p, o = where[q]
            out.append(j << 32 | p << 1 | o)
    return out


def hits_by_ints(k, recs, min_cnt, amap, img):
    pos = {r[0]: i for i, r in enumerate(recs) if r[3] >= min_cnt}
    mask = (1 << 2 * k) - 1
    out, f, r, n = [], 0, 0, 0
    for b in img:
        if b not in CODE:
            n = 0
            out.append(NONE)
            continue
        c = CODE[b]
        f, r, n = (f << 2 | c) & mask, r >> 2 | (3 - c) << 2 * (k - 1), n + 1
        if n < k:
            out.append(NONE)
            continue
        y = min(f, r)
        if y not in pos:
            out.append(ABSENT)
            continue
        j, at = amap[pos[y]]
        out.append(j << 32 | (at >> 1) << 1 | ((at & 1) ^ (f != y)))
    return out


def chain(k, ug, hits, off, lens):
    """(paths [dict(seq, qs, qe, ps, step_off, n_step)], steps [j << 1 | o], tally [(n_kmer, n_hit, n_path, n_step)] per sequence, spans [(j, o, p_first,
    p_last)] per step) of a hit array"""
    paths, steps, spans = [], [], []
    tally = [[0, 0, 0, 0] for _ in off]
    seq_of = lambda i: bisect.bisect_right(off, i) - 1
    is_hit = lambda h: h < ABSENT
    for s, (o, n) in enumerate(zip(off, lens)):
        tally[s][0] = sum(1 for h in hits[o:o + n] if h != NONE)
        tally[s][1] = sum(1 for h in hits[o:o + n] if is_hit(h))
    i = 0
    for hit, run in itertools.groupby(hits, key=is_hit):
        run = list(run)
        if hit:
            s = seq_of(i)
            assert off[s] <= i - k + 1 and i + len(run) <= off[s] + lens[s], "a path across a sequence boundary"
            # a step: the positions over which (unitig, orientation, p -/+ position) stays what it is
            line = lambda t: (t[1] >> 32, t[1] & 1, (t[1] >> 1 & 0x7fffffff) + (t[0] if t[1] & 1 else -t[0]))
            first = True
            step_off = len(steps)
            for (j, o, _), st in itertools.groupby(enumerate(run), key=line):
                st = [h for _, h in st]
                p0, p1 = st[0] >> 1 & 0x7fffffff, st[-1] >> 1 & 0x7fffffff
                if first:
                    ps = p0 if o == 0 else ug[j][1] - 1 - p0
                    first = False
                steps.append(j << 1 | o)
                spans.append((j, o, p0, p1))
            paths.append(dict(seq=s, qs=i - k + 1 - off[s], qe=i + len(run) - off[s], ps=ps, step_off=step_off, n_step=len(steps) - step_off))
            tally[s][2] += 1
            tally[s][3] += len(steps) - step_off
        i += len(run)
    return paths, steps, [tuple(t) for t in tally], spans


def check_rules(k, ug, paths, steps, spans, links):
    """consecutive steps of a path are a link of yak_amd_gfa.h; only the first step of a path may begin inside its oriented unitig, only the last may
    end inside it"""
    have = set(links)
    for p in paths:
        a, n = p["step_off"], p["n_step"]
        assert n >= 1
        for t in range(a, a + n):
            j, o, p0, p1 = spans[t]
            nn = ug[j][1]
            begins, ends = (p0 == 0, p1 == nn - 1) if o == 0 else (p0 == nn - 1, p1 == 0)
            assert (p1 - p0 if o == 0 else p0 - p1) >= 0
            assert t == a or begins, "a later step begins inside its unitig"
            assert t == a + n - 1 or ends, "an earlier step ends inside its unitig"
            if t > a:
                assert (steps[t - 1], steps[t]) in have, "two consecutive steps without a link"


def gaf_text(k, ug, names, lens, paths, steps, min_len=0):
    out = []
    for p in paths:
        span = p["qe"] - p["qs"]
        if span < min_len:
            continue
        st = steps[p["step_off"]:p["step_off"] + p["n_step"]]
        plen = sum(ug[s >> 1][1] for s in st) + k - 1
        out.append("%s\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t%d\t%d\t255\n" % (names[p["seq"]], lens[p["seq"]], p["qs"], p["qe"], "".join("%su%d" % ("><"[s & 1], s >> 1) for s in st),
                                                                         plen, p["ps"], p["ps"] + span, span, span))
    return "".join(out).encode()


def stats_text(k, min_cnt, names, lens, tally):
    out = ["#paths\tk=%d\tmin_cnt=%d\n" % (k, min_cnt)]
    out += ["S\t%s\t%d\t%d\t%d\t%d\t%d\n" % ((nm, ln) + tuple(t)) for nm, ln, t in zip(names, lens, tally)]
    out.append("T\t%d\t%d\t%s\n" % (len(names), sum(lens), "\t".join("%d" % sum(t[x] for t in tally) for x in range(4))))
    return "".join(out).encode()


def records_text(paths, steps, tally):
    """what path_model_check prints in its `records` mode, without its last line (T table_slots keys max_probe)"""
    out = ["P %d %d %d %d %d %d\n" % (p["seq"], p["qs"], p["qe"], p["ps"], p["step_off"], p["n_step"]) for p in paths]
    out += ["S %d\n" % s for s in steps] + ["Y %d %d %d %d\n" % t for t in tally]
    return "".join(out).encode()


def model_file(fn, k, min_cnt, cap, min_len, desc, bases):
    """what tests/tools/path_model_check.cpp reads, little-endian 64-bit words: k, min_cnt, the capacity of the index (0: the default), min_len, the
    numbers of unitigs and of bases, the descriptors (off, n_node, kc, first); then the bases"""
    words = [k, min_cnt, cap, min_len, len(desc), len(bases)]
    for d in desc:
        words += list(d)
    with open(fn, "wb") as f:
        f.write(struct.pack("<%dQ" % len(words), *words))
        f.write(bases)


def fasta(names, seqs):
    return b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in zip(names, seqs))


def rc_bytes(s):
    return U.rc_str(s.decode()).encode()


def reads_of(rng, sources, n, lo, hi, sub=0.0, n_rate=0.0, mixed_case=False):
    """n reads cut from the source strings on both strands, with substitutions, Ns, and with lower case and U for T"""
    out = []
    for _ in range(n):
        src = rng.choice(sources)
        ln = min(rng.randint(lo, hi), len(src))
        a = rng.randint(0, len(src) - ln)
        r = src[a:a + ln]
        if rng.random() < 0.5:
            r = U.rc_str(r)
        r = list(r)
        for x in range(len(r)):
            u = rng.random()
            if u < sub:
                r[x] = rng.choice([c for c in "ACGT" if c != r[x]])
            elif u < sub + n_rate:
                r[x] = "N"
            if mixed_case and rng.random() < 0.2:
                r[x] = {"T": rng.choice("tUu")}.get(r[x], r[x].lower())
        out.append("".join(r).encode())
    return out
