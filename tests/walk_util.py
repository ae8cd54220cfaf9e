"""The results of the device walk (include/yak_amd_walk.h) restated from the unitigs as graph_util.unitigs() gives them -- from
their strings alone, independently of any walk: position p of unitig j is the node whose canonical k-mer equals canon(s[p:p + k]), d = 1 iff that
substring is not canonical (a cycle's string wraps by k - 1, so every p < n_node has its k bases).  tests/test_walk.py holds this to hand-derived
cases and the sequential model of the kernels (tests/tools/uwalk_model_check.cpp) to it; tests/test_gpu_walk.py holds the device to it."""
import graph_util as U

NONE = U.NONE


def restate(k, recs, min_cnt, ug):
    """(map [(unitig, at)] per stored key in listing order, desc [(off, n_node, kc, first)] per unitig, bases as bytes)"""
    pos = {U.kmer_str(r[0], k): i for i, r in enumerate(recs) if r[3] >= min_cnt}      # stored keys are canonical
    assert all(s == U.canon(s) for s in pos)
    amap = [(NONE, 0)] * len(recs)
    desc, off = [], 0
    for j, (s, n, kc, cyc) in enumerate(ug):
        assert len(s) == n + k - 1
        first = None
        for p in range(n):
            sub = s[p:p + k]
            c = U.canon(sub)
            v = pos[c]
            assert amap[v] == (NONE, 0), "a node in two places"
            amap[v] = (j, p << 1 | (1 if sub != c else 0))
            if p == 0:
                first = v
        desc.append((off, n, kc, first << 1 | (1 if cyc else 0)))
        off += len(s)
    assert sum(1 for m in amap if m[0] != NONE) == len(pos)
    return amap, desc, "".join(u[0] for u in ug).encode()


def stats(k, recs, min_cnt, ug):
    """yakamd_uwstat_t without rounds and host_nodes"""
    lens = sorted((len(u[0]) for u in ug), reverse=True)
    tot, acc, n50 = sum(lens), 0, 0
    for v in lens:
        acc += v
        if 2 * acc >= tot:
            n50 = v
            break
    return dict(n_key=len(recs), n_node=sum(1 for r in recs if r[3] >= min_cnt), n_open=sum(1 for u in ug if not u[3]), n_cycle=sum(1 for u in ug if u[3]),
                sum_len=tot, max_len=lens[0] if lens else 0, n50=n50)


def cycle_nodes(ug):
    return sum(u[1] for u in ug if u[3])


def map_text(amap, desc):
    """what uwalk_model_check prints in its `map` mode, without its last line (R rounds cycle_nodes)"""
    return ("".join("%d %d\n" % m for m in amap) + "".join("D %d %d %d %d\n" % d for d in desc)).encode()
