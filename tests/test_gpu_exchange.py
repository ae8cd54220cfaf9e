"""The front of the pipeline, element by element: what yakamd_extract_dev, yakamd_partition_dev / _hashes_dev / _tagged_dev and yakamd_pack_bases_dev
write for an image against what tests/exchange_util.py works out from the oracle's flat extraction (tests/test_exchange.py pins that side without a
GPU), and the owner's side of the tagged format (yakamd_feed_partitioned_tagged_dev) called directly.  Every comparison is exact equality of integers.

Every output buffer is 4 KiB longer than include/yak_amd.h asks for and filled with 0xA5 from the host before the call; the 4 KiB must still hold
0xA5 afterwards (Out.take): a store behind the end of an output buffer fails the test that made it."""
import ctypes as C
import struct

import numpy as np
import pytest

import exchange_util as xu

pytestmark = pytest.mark.gpu

KS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 63]
PRES = [3, 10, 11, 13]             # with k on both sides of 32: k_xpart_wc<1>, k_xpart_wc<2>, k_xpart_wcs<false>, k_xpart<1>, k_xpart<2>
TAGGED = [(31, 10), (30, 8), (21, 10), (27, 3), (1, 3)]      # k_xpart<3, 31> + k_xpart_wcs<true, 31>; the others k_xpart<3> + k_xpart_wcs<true>
IMAGES = ["all_bytes", "random_3wg", "low_complexity"]
SLACK = 4096


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


@pytest.fixture(scope="module")
def images(synth):
    return dict(all_bytes=xu.all_bytes_image(), random_3wg=xu.random_3wg_image(synth), low_complexity=xu.low_complexity_image(synth))


class _Ref:
    """the oracle with its flat extraction computed once per (image, k) and left unchanged"""

    def __init__(self, oracle):
        self.o, self.cache, self.nt4 = oracle, {}, oracle.nt4

    def extract_pos(self, k, img):
        key = (len(img), hash(img), k)
        if key not in self.cache:
            h, t = self.o.extract_pos(k, img)
            h.setflags(write=False); t.setflags(write=False)
            self.cache[key] = (h, t)
        return self.cache[key]


@pytest.fixture(scope="module")
def ref(oracle):
    return _Ref(oracle)


def upload(L, img):
    """a fresh device buffer of exactly len(img) rounded up to 16 bytes (16-byte aligned: hipMalloc) holding img"""
    d = L.yakamd_dev_alloc(max(16, (len(img) + 15) & ~15))
    assert d and d % 16 == 0
    if img:
        assert L.yakamd_memcpy_h2d(d, img, len(img)) == 0
    return d


@pytest.fixture(scope="module")
def dimg(ya, images):
    L = ya.lib()
    d = {name: upload(L, img) for name, img in images.items()}
    yield d
    for p in d.values():
        L.yakamd_dev_free(p)


class Out:
    """a device output buffer of `nbytes` (the documented size) + 4 KiB, all 0xA5"""

    def __init__(self, L, nbytes):
        self.L, self.n = L, int(nbytes)
        self.p = L.yakamd_dev_alloc(self.n + SLACK)
        assert self.p
        fill = np.full(self.n + SLACK, 0xA5, np.uint8)
        assert L.yakamd_memcpy_h2d(self.p, fill.ctypes.data, self.n + SLACK) == 0

    def take(self, dtype, count):
        """the first `count` elements; checks the 4 KiB behind the buffer and frees it"""
        raw = np.empty(self.n + SLACK, np.uint8)
        assert self.L.yakamd_memcpy_d2h(raw.ctypes.data, self.p, self.n + SLACK) == 0
        self.L.yakamd_dev_free(self.p)
        self.p = None
        assert count * np.dtype(dtype).itemsize <= self.n, "more elements than the buffer is documented to hold"
        assert (raw[self.n:] == 0xA5).all(), "a store behind the end of the output buffer"
        return raw[:count * np.dtype(dtype).itemsize].view(dtype).copy()


def err(L):
    return (L.yakamd_last_error() or b"").decode()


# ------------------------------------------------------------------------------------------------------------ yakamd_extract_dev
def check_extract(L, ref, d, img, k, pre=10):
    n = len(img)
    h, t = ref.extract_pos(k, img)
    p = (h & np.uint64((1 << pre) - 1)).astype(np.int64)

    def call(lo, hi):
        oh, ot = Out(L, 8 * n), Out(L, 4 * n)
        m = L.yakamd_extract_dev(k, d, n, oh.p, ot.p, pre, lo, hi, None)
        assert 0 <= m <= n, err(L)
        gh, gt = oh.take(np.uint64, m), ot.take(np.uint32, m)
        o = np.argsort(gt, kind="stable")                  # a global cursor hands out the places: the order is free, the positions are unique
        return gh[o], gt[o]

    def same(got, sel, what):
        assert np.array_equal(got[1], t[sel]) and np.array_equal(got[0], h[sel]), "extract k=%d n=%d %s" % (k, n, what)
    P = 1 << pre
    same(call(0, P), slice(None), "all prefixes")
    same(call(0, 0), slice(0, 0), "no prefix")
    one = int(p[len(p) // 2]) if len(p) else 517
    same(call(one, one + 1), p == one, "prefix %d alone" % one)
    a, b = call(0, 300), call(300, P)
    same(a, p < 300, "lower part")
    same(b, p >= 300, "upper part")
    o = np.argsort(np.concatenate([a[1], b[1]]), kind="stable")
    same((np.concatenate([a[0], b[0]])[o], np.concatenate([a[1], b[1]])[o]), slice(None), "the two parts together")


@pytest.mark.parametrize("k", KS)
def test_extract(k, ya, ref, images, dimg):
    for name in IMAGES:
        check_extract(ya.lib(), ref, dimg[name], images[name], k)


# ------------------------------------------------------------------------------------------------------------ yakamd_partition_dev / _hashes_dev
def check_partition(L, ref, d, img, k, pre):
    n, P = len(img), 1 << pre
    wh, wt, wb = xu.expect_groups(ref, img, k, pre)
    what = "partition k=%d pre=%d n=%d" % (k, pre, n)
    out, bst = Out(L, 16 * n), (C.c_uint64 * (P + 1))(*([0xA5A5A5A5A5A5A5A5] * (P + 1)))
    m = L.yakamd_partition_dev(k, pre, d, n, out.p, bst)
    assert m == len(wh), what + ": " + err(L)
    b = np.frombuffer(bst, np.uint64)
    assert np.array_equal(b, wb), what
    rec = out.take(np.uint64, 2 * m).reshape(m, 2)
    assert not (rec[:, 1] >> np.uint64(32)).any(), what
    gh, gt = xu.sort_groups(b, rec[:, 0], rec[:, 1].astype(np.uint32))
    assert np.array_equal(gt, wt) and np.array_equal(gh, wh), what
    out2, bst2 = Out(L, 8 * n), (C.c_uint64 * (P + 1))(*([0xA5A5A5A5A5A5A5A5] * (P + 1)))
    assert L.yakamd_partition_hashes_dev(k, pre, d, n, out2.p, bst2) == m, what + " (hashes): " + err(L)
    assert np.array_equal(np.frombuffer(bst2, np.uint64), b), what + " (hashes)"
    assert np.array_equal(xu.sort_groups(b, out2.take(np.uint64, m))[0], xu.sort_groups(wb, wh)[0]), what + " (hashes)"


@pytest.mark.parametrize("pre", PRES)
@pytest.mark.parametrize("k", KS)
def test_partition(k, pre, ya, ref, images, dimg):
    for name in IMAGES:
        check_partition(ya.lib(), ref, dimg[name], images[name], k, pre)


def test_partition_of_an_empty_image(ya, ref, images, dimg):
    """n_bytes = 0 is "no chunk": 0 records, every offset 0 -- right after a call that left non-zero offsets in the buffers the next call gets"""
    L = ya.lib()
    for fn, hash_only in ((L.yakamd_partition_dev, 0), (L.yakamd_partition_hashes_dev, 1), (L.yakamd_partition_tagged_dev, 2)):
        for k, pre in ((31, 10), (1, 3)) + (((63, 13),) if hash_only != 2 else ()):
            P = 1 << pre
            out, bst = Out(L, 16 * 5000), (C.c_uint64 * (P + 1))()
            assert fn(k, pre, dimg["random_3wg"], 5000, out.p, bst) == bst[P] > 0
            out.take(np.uint8, 0)
            out, bst = Out(L, 0), (C.c_uint64 * (P + 1))(*([0xA5A5A5A5A5A5A5A5] * (P + 1)))
            assert fn(k, pre, dimg["random_3wg"], 0, out.p, bst) == 0, err(L)
            assert not any(bst)
            out.take(np.uint8, 0)


def test_partition_refusals(ya, dimg):
    L = ya.lib()
    d = dimg["random_3wg"]
    for fn in (L.yakamd_partition_dev, L.yakamd_partition_hashes_dev):
        for k, pre, ptr, msg in ((0, 10, d, "unsupported k / pre"), (64, 10, d, "unsupported k / pre"), (31, 2, d, "unsupported k / pre"),
                                 (31, 14, d, "unsupported k / pre"), (31, 10, d + 8, "16-byte aligned")):
            out, bst = Out(L, 16 * 4096), (C.c_uint64 * ((1 << max(pre, 3)) + 1))()
            assert fn(k, pre, ptr, 4096, out.p, bst) == -1
            assert msg in err(L)
            assert (out.take(np.uint8, 16 * 4096) == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------ yakamd_partition_tagged_dev
def describe_difference(got, want):
    for p in range(int(max(got.prefix.max(initial=0), want.prefix.max(initial=0))) + 1):
        g, w = [s for _, s in got.of(p)], [s for _, s in want.of(p)]
        if g != w:
            i = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            return "prefix %d: %d runs for %d contributing rounds; the first that differs is run %d (round %s)" % (
                p, len(g), len(w), i, want.of(p)[i][0] if i < len(w) else "-")
    return "no difference in the sets (the order of the runs differs)"


def check_tagged(L, ref, d, img, k, pre):
    n, P = len(img), 1 << pre
    want, wb = xu.expect_tagged(ref, img, k, pre)
    what = "tagged partition k=%d pre=%d n=%d" % (k, pre, n)
    out, bst = Out(L, 8 * n), (C.c_uint64 * (P + 1))(*([0xA5A5A5A5A5A5A5A5] * (P + 1)))
    m = L.yakamd_partition_tagged_dev(k, pre, d, n, out.p, bst)
    assert m == int(wb[P]), what + ": " + err(L)
    b = np.frombuffer(bst, np.uint64)
    assert np.array_equal(b, wb), what
    rec = out.take(np.uint64, m)
    assert not (rec & np.uint64(1 << 11)).any(), what + ": bit 11 belongs to no field"
    got = xu.decode_tagged(rec, b)
    assert got.same_runs(want), what + ": " + describe_difference(got, want)
    assert xu.toggles_alternate(got), what


@pytest.mark.parametrize("k,pre", TAGGED)
def test_partition_tagged(k, pre, ya, ref, images, dimg):
    # the inputs do what they are for: a round that overflows the 7-slot stack of the write combining, toggles that cross workgroups
    assert xu.max_per_round(xu.expect_tagged(ref, images["low_complexity"], k, pre)[0]) > 8
    assert xu.crosses_workgroups(xu.expect_tagged(ref, images["random_3wg"], k, pre)[0])
    for name in IMAGES:
        check_tagged(ya.lib(), ref, dimg[name], images[name], k, pre)


def test_tagged_format_applies_where_documented(ya, dimg, knob):
    L = ya.lib()
    for k in range(1, 64):
        for pre in range(0, 15):
            assert bool(L.yakamd_tagged_ok(k, pre)) == (k < 32 and 2 * k - pre <= 52 and 3 <= pre <= 10), (k, pre)

    def refused(k, pre):
        out, bst = Out(L, 8 * 4096), (C.c_uint64 * ((1 << pre) + 1))()
        r = L.yakamd_partition_tagged_dev(k, pre, dimg["random_3wg"], 4096, out.p, bst)
        assert (out.take(np.uint8, 8 * 4096) == 0xA5).all() or r >= 0
        return r == -1 and "tagged records need" in err(L)
    assert refused(31, 9) and refused(32, 10) and not refused(31, 10)
    knob("YAKAMD_REC8", 0)
    assert not L.yakamd_tagged_ok(31, 10) and refused(31, 10)


# ------------------------------------------------------------------------------------------------------------ the length edges
@pytest.mark.parametrize("k", xu.EDGE_K)
def test_length_edges(k, ya, ref, images):
    """prefixes of random_3wg, each in a fresh buffer of exactly its length rounded up to 16: the byte-wise ends of xt_load / xt_put, the last
    partial tile and workgroup, images too short for one k-mer or one bulk load"""
    L = ya.lib()
    for n in xu.edge_lengths(k):
        img = images["random_3wg"][:n]
        d = upload(L, img)
        check_extract(L, ref, d, img, k)
        check_partition(L, ref, d, img, k, 10)
        for pre in (10, 3):
            if L.yakamd_tagged_ok(k, pre):
                check_tagged(L, ref, d, img, k, pre)
        L.yakamd_dev_free(d)


# ------------------------------------------------------------------------------------------------------------ yakamd_pack_bases_dev
def check_pack(ya, oracle, d, img):
    L = ya.lib()
    n = len(img)
    nw = (n + 31) // 32
    oc, ov = Out(L, 8 * nw), Out(L, 4 * nw)
    assert L.yakamd_pack_bases_dev(d, n, oc.p, ov.p, None) == 0 and L.yakamd_device_sync() == 0
    codes, valid = oc.take(np.uint32, 2 * nw), ov.take(np.uint32, nw)
    wc, wv = xu.expect_packed(oracle, img)
    assert np.array_equal(valid, wv) and np.array_equal(codes, wc), "pack n=%d" % n
    hc, hv = xu.split_packed(ya.pack_bases_host(img), n)
    assert np.array_equal(codes, hc) and np.array_equal(valid, hv), "pack n=%d (host)" % n


@pytest.mark.parametrize("name", ["all_bytes", "random_3wg"])
def test_pack(name, ya, oracle, images, dimg):
    check_pack(ya, oracle, dimg[name], images[name])


def test_pack_length_edges(ya, oracle, images):
    L = ya.lib()
    for n in sorted(set(n for k in xu.EDGE_K for n in xu.edge_lengths(k))):
        for src in ("random_3wg", "all_bytes"):
            img = images[src][:n]
            d = upload(L, img)
            check_pack(ya, oracle, d, img)
            L.yakamd_dev_free(d)


# ------------------------------------------------------------------------------------------------------------ the consumer of the tagged format
def test_no_table_takes_a_prefix_below_10_bits(ya):
    """yak_ch_init refuses pre < 10 (htab.c:20) and the tagged format needs pre <= 10: pre = 10 is the only prefix length at which a table can be
    fed tagged records, so the consumer below runs at pre = 10 alone"""
    L = ya.lib()
    for pre in range(3, 10):
        assert L.yakamd_tagged_ok(21, pre) and not L.yak_ch_init(21, pre, 4, 0)


@pytest.mark.parametrize("mode", ["tagged", "fast_off"])
@pytest.mark.parametrize("bf", [0, 23])
@pytest.mark.parametrize("k", [31, 21])
def test_tagged_exchange_on_one_gpu(k, bf, mode, ya, oracle, synth, images, knob):
    """four sources (one of them low_complexity), four owners with yakamd_set_shard: every owner takes each source's slice of
    yakamd_partition_tagged_dev through yakamd_feed_partitioned_tagged_dev, lent and copied alternating, and pass 2 through
    yakamd_count_partitioned_dev; the owners' sub-tables, one behind the other, are the oracle's bytes for the four images one behind the other.
    fast_off: with the exclusive-ownership path switched off the feed refuses tagged records and the same pass takes 16-byte records instead"""
    L = ya.lib()
    world, P, pre = 4, 1024, 10
    per = P // world
    slices = [synth(1200, g=12000, s=5, first=r * 1200) for r in range(3)]
    slices.insert(1, images["low_complexity"])
    t0 = [sum(len(x) for x in slices[:i]) for i in range(world)]
    srcs = []
    for x in slices:                                       # what every source rank prepares
        nb = len(x)
        d = upload(L, x)
        rec8, rec16, hsh = L.yakamd_dev_alloc(nb * 8), L.yakamd_dev_alloc(nb * 16), L.yakamd_dev_alloc(nb * 8)
        bst, b16, b8 = ((C.c_uint64 * (P + 1))() for _ in range(3))
        n = L.yakamd_partition_tagged_dev(k, pre, d, nb, rec8, bst)
        assert n == bst[P] > 0, err(L)
        assert L.yakamd_partition_dev(k, pre, d, nb, rec16, b16) == n and L.yakamd_partition_hashes_dev(k, pre, d, nb, hsh, b8) == n
        assert list(b16) == list(bst) == list(b8)
        srcs.append((rec8, rec16, hsh, list(bst), nb))
        L.yakamd_dev_free(d)
    if mode == "fast_off":
        knob("YAKAMD_FAST", 0)
    parts, tot = [], 0
    for r in range(world):
        lo, hi = r * per, (r + 1) * per
        t = ya.Table(k, pre, 4, bf)
        assert L.yakamd_set_shard(t.h, lo, hi) == 0

        def one_pass(create_new):
            assert L.yakamd_pass_begin(t.h, create_new) == 0
            if create_new:
                assert L.yakamd_pass_fast(t.h) == (1 if mode == "tagged" else 0)
            for src, (rec8, rec16, hsh, bst, nb) in enumerate(srcs):
                m = bst[hi] - bst[lo]
                ob = (C.c_uint64 * (P + 1))(*([0] * lo + [b - bst[lo] for b in bst[lo:hi + 1]] + [m] * (P - hi)))
                if not create_new:                          # count-existing pass: 8-byte hashes, same grouping
                    assert L.yakamd_count_partitioned_dev(t.h, hsh + 8 * bst[lo], m, ob) == 0, err(L)
                    continue
                r8 = L.yakamd_feed_partitioned_tagged_dev(t.h, rec8 + 8 * bst[lo], m, ob, t0[src], nb, (src + r) & 1)
                if mode == "tagged":
                    assert r8 == 0, err(L)
                else:
                    assert r8 == -1 and "tagged records need the exclusive-ownership path" in err(L)
                    assert L.yakamd_feed_partitioned_dev(t.h, rec16 + 16 * bst[lo], m, ob, t0[src], nb) == 0, err(L)
            n_ins = L.yakamd_pass_end(t.h)
            assert n_ins >= 0, err(L)
            t.h.contents.tot += n_ins
        one_pass(1)
        if bf:
            t.destroy_bf(); t.clear(); one_pass(0); t.shrink(2, 1023)
        data = t.dump_bytes(); tot += t.tot; t.close()
        off = 16
        for p in range(P):
            cap, n = struct.unpack_from("<II", data, off)
            if lo <= p < hi:
                parts.append(data[off:off + 8 + 8 * n])
            off += 8 + 8 * n
    for rec8, rec16, hsh, _, _ in srcs:
        L.yakamd_dev_free(rec8); L.yakamd_dev_free(rec16); L.yakamd_dev_free(hsh)
    want, wtot = oracle.count_protocol_mem(b"".join(slices), k=k, bf_shift=bf)
    assert want[:16] + b"".join(parts) == want and tot == wtot
