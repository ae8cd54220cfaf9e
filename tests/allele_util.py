"""The read support of the bubbles' alleles (`yak-amd bubbles -r`; include/yak_amd_allele.h) restated twice over, and the
command's text.  flat() goes from the paths and steps of path_util and the bubble records of bubble_util: the arm map, an observation per step on an
arm, full iff the step is neither the first nor the last of its path.  by_strings() goes from strings alone: with c the base in front of the arm in
the oriented source and d the base behind it in the oriented sink, the full observations of an allele in a read are the occurrences of c + A + d and
of its reverse complement, the partial ones the maximal runs of the arm's nodes that no such occurrence holds.  tests/test_allele.py holds the two
to each other and to hand-derived cases, tests/test_allele_model.py the sequential model of the kernels to them, tests/test_gpu_allele.py the
device."""
import struct

import bubble_util as B
import graph_util as U
import path_util as P

NONE = (1 << 32) - 1
A, FULL, REV = 1, 2, 4
CALLS = ("het", "hom1", "hom2", "none")


def arm_map(n_unitig, recs):
    arm_of = [NONE] * n_unitig
    for i, r in enumerate(recs):
        for a in (0, 1):
            j = r[2][a] >> 1
            assert arm_of[j] == NONE, "a unitig claimed by two arms"
            arm_of[j] = i << 1 | a
    return arm_of


def observe(paths, steps, recs, arm_of):
    """[(seq, bubble, flags, path)] in step order, and beside it the step of each"""
    obs, at = [], []
    for p, pa in enumerate(paths):
        a0, n = pa["step_off"], pa["n_step"]
        for t in range(a0, a0 + n):
            s = steps[t]
            m = arm_of[s >> 1]
            if m == NONE:
                continue
            i, a = m >> 1, m & 1
            full = t not in (a0, a0 + n - 1)
            rev = (s ^ recs[i][2][a]) & 1
            obs.append((pa["seq"], i, a | full << 1 | rev << 2, p))
            at.append(t)
    return obs, at


def support(n_bubble, obs):
    sup = [[0, 0, 0, 0] for _ in range(n_bubble)]                # full1 full2 part1 part2
    for _, i, fl, _ in obs:
        sup[i][(0 if fl & FULL else 2) + (fl & A)] += 1
    return [tuple(s) for s in sup]


def call(s, min_sup):
    one, two = s[0] >= min_sup, s[1] >= min_sup
    return CALLS[0 if one and two else 1 if one else 2 if two else 3]


def flat(k, ug, recs, reads):
    """everything restatement 1 says of reads (bytes) on the unitigs ug with the bubble records recs"""
    img, off, lens = P.image(reads)
    hits = P.hits_by_strings(k, ug, img)
    paths, steps, tally, spans = P.chain(k, ug, hits, off, lens)
    obs, at = observe(paths, steps, recs, arm_map(len(ug), recs))
    return dict(paths=paths, steps=steps, lens=lens, obs=obs, at=at, sup=support(len(recs), obs))


def check_invariants(recs, d):
    """the neighbours of a full observation are src and sink; full + part over the bubbles is n_obs"""
    steps = d["steps"]
    for (seq, i, fl, p), t in zip(d["obs"], d["at"]):
        if fl & FULL:
            src, sink = recs[i][0], recs[i][1]
            assert (steps[t - 1], steps[t + 1]) == ((sink ^ 1, src ^ 1) if fl & REV else (src, sink)), "a full observation without its flanks"
        assert steps[t] >> 1 == recs[i][2][fl & A] >> 1 and d["paths"][p]["seq"] == seq
    assert sum(sum(s) for s in d["sup"]) == len(d["obs"])


def frag_lines(names, obs, min_frag):
    """the F lines of observation records [(seq, bubble, flags, ...)] in read order"""
    out, per = [], {}
    for o in obs:
        if o[2] & FULL:
            per.setdefault(o[0], []).append("%d:%d%s" % (o[1], 1 + (o[2] & A), "-" if o[2] & REV else "+"))
    for seq in sorted(per):
        if len(per[seq]) >= min_frag:
            out.append("F\t%s\t%d\t%s\n" % (names[seq], len(per[seq]), "\t".join(per[seq])))
    return out


def allele_lines(recs, sup, min_sup):
    return ["A\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%s\n" % ((i, B.end_name(r[2][0]), B.end_name(r[2][1])) + tuple(s) + (call(s, min_sup),)) for i, (r, s) in enumerate(zip(recs, sup))]


def text(k, min_cnt, min_sup, min_frag, fragments, stats_only, names, recs, d):
    """the text of the command from flat()'s result over all the reads: it does not depend on the chunks"""
    out = ["#alleles\tk=%d\tmin_cnt=%d\tmin_sup=%d\n" % (k, min_cnt, min_sup)]
    frags = frag_lines(names, d["obs"], min_frag) if fragments else []
    alleles = allele_lines(recs, d["sup"], min_sup)
    if not stats_only:
        out += frags + alleles
    calls = [call(s, min_sup) for s in d["sup"]]
    tail = [len(names), sum(d["lens"]), len(d["paths"]), len(d["steps"]), len(d["obs"]), sum(1 for o in d["obs"] if o[2] & FULL), len(frags), len(recs)]
    out.append("T\t%s\n" % "\t".join("%d" % v for v in tail + [calls.count(c) for c in CALLS]))
    return "".join(out).encode()


# ---- restatement 2: from strings alone ----
def plain(read):
    return "".join("ACGT"[P.CODE[b]] if b in P.CODE else "N" for b in read)


def occurrences(s, w):
    out, at = [], s.find(w)
    while at >= 0:
        out.append(at)
        at = s.find(w, at + 1)
    return out


def by_strings(k, ug, recs, reads):
    """per read [(bubble, a, full, rev)] in read order"""
    arms = []
    for i, r in enumerate(recs):
        for a in (0, 1):
            arm = B.oriented(ug, r[2][a])
            w = B.oriented(ug, r[0])[-k] + arm + B.oriented(ug, r[1])[k - 1]
            rc = U.rc_str(arm)
            nodes = {}
            for p in range(len(arm) - k + 1):
                nodes[arm[p:p + k]] = (0, p)
                nodes[rc[p:p + k]] = (1, p)
            arms.append((i, a, len(arm) - k + 1, w, nodes))
    out = []
    for read in reads:
        s = plain(read)
        got = []
        for i, a, n, w, nodes in arms:
            whole = {}
            for rev, word in ((0, w), (1, U.rc_str(w))):
                for at in occurrences(s, word):
                    whole[at + 1] = rev
                    got.append((at + 1, i, a, 1, rev))
            run = None                                           # (first position, orientation, p of the last node)
            for x in range(len(s) - k + 2):
                hit = nodes.get(s[x:x + k]) if x + k <= len(s) else None
                if run is not None and (hit is None or hit != (run[1], run[2] + 1)):
                    if not (run[0] in whole and x - run[0] == n):
                        got.append((run[0], i, a, 0, run[1]))
                    run = None
                if hit is not None:
                    run = (x if run is None else run[0], hit[0], hit[1])
        out.append([g[1:] for g in sorted(got)])
    return out


def by_strings_lines(names, recs, per_read, min_sup, min_frag):
    """(F lines, A lines) of by_strings()'s result"""
    sup = [[0, 0, 0, 0] for _ in recs]
    frags = []
    for nm, got in zip(names, per_read):
        for i, a, full, rev in got:
            sup[i][(0 if full else 2) + a] += 1
        fr = ["%d:%d%s" % (i, 1 + a, "-+"[rev == 0]) for i, a, full, rev in got if full]
        if len(fr) >= min_frag:
            frags.append("F\t%s\t%d\t%s\n" % (nm, len(fr), "\t".join(fr)))
    return frags, allele_lines(recs, sup, min_sup)


# ---- the model of the kernels ----
def chunks(reads, chunk_size):
    """the reads as the command cuts them: a chunk is full once it holds chunk_size bases; the last may be empty"""
    out, cur, n = [], [], 0
    for i, r in enumerate(reads):
        cur.append(i)
        n += len(r)
        if n >= chunk_size:
            out.append(cur)
            cur, n = [], 0
    return out + [cur]


def model_file(fn, k, min_cnt, min_sup, min_frag, fragments, stats_only, ug, recs, names, reads, chunk_size):
    """what tools/allele_model_check.cpp reads (little-endian 64-bit words unless stated): k, min_cnt, min_sup, min_frag, fragments, stats_only, the
    numbers of unitigs, bubbles and chunks; the bubble records; per chunk n_seq, its bases, n_path, n_step, the path records (yakamd_upath_t),
    the steps, the bytes of the names, the names each with a newline behind it, padded to eight bytes.  Returns flat() per chunk"""
    parts = chunks(reads, chunk_size)
    rows = B.as_rows(recs)
    out = [struct.pack("<9Q", k, min_cnt, min_sup, min_frag, int(fragments), int(stats_only), len(ug), len(recs), len(parts))]
    out += [struct.pack("<10Q", *r) for r in rows]
    per = []
    for part in parts:
        d = flat(k, ug, recs, [reads[i] for i in part])
        per.append(d)
        out.append(struct.pack("<4Q", len(part), sum(len(reads[i]) for i in part), len(d["paths"]), len(d["steps"])))
        out += [struct.pack("<QQIIII", p["step_off"], p["ps"], p["seq"], p["n_step"], p["qs"], p["qe"]) for p in d["paths"]]
        out.append(struct.pack("<%dQ" % len(d["steps"]), *d["steps"]))
        nm = b"".join(names[i].encode() + b"\n" for i in part)
        out.append(struct.pack("<Q", len(nm)) + nm + b"\0" * (-len(nm) % 8))
    with open(fn, "wb") as f:
        f.write(b"".join(out))
    return per


def records_text(per, n_bubble):
    """what allele_model_check prints in its `records` mode"""
    out, sup = [], [[0, 0, 0, 0] for _ in range(n_bubble)]
    for d in per:
        out += ["O %d %d %d %d\n" % o for o in d["obs"]]
        out.append("N %d %d\n" % (len(d["obs"]), sum(1 for o in d["obs"] if o[2] & FULL)))
        for i, s in enumerate(d["sup"]):
            sup[i] = [x + y for x, y in zip(sup[i], s)]
    return ("".join(out) + "".join("S %d %d %d %d\n" % tuple(s) for s in sup)).encode()
