"""The lookup kernel (k_lookup, behind yakamd_lookup_dev and yakamd_triobin_lookup_dev) against the oracle's restatement of the same
operation (yko_lookup_image, pinned on the reference's own library by tests/test_oracle_lookup.py), on every kind of table it can be given:
every sub-table directory path (pre 10-12 staged in LDS, pre 13-14 read from global memory), every operation that writes the table image
(a count pass as it left the table, the two-pass protocol fused and not, the loads, shrink, clear, setcnt, inc, subtract, isec, merge,
tighten), every shape of query stream, and every refusal.  Each case first asserts that the library's .yak bytes are the oracle's, so a
mismatch after that is the lookup's."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENT = 0xA5                                    # every byte of an output buffer before the call
FUSED, RECOUNT = 1, 2
MOTIF = bytes(np.random.default_rng(0).choice(list(b"ACGT"), 200).tolist())     # counted 1100 times: its k-mers saturate at 1023
SEEN = {"cases": 0, "cap0": 0, "dense": 0, "zero": 0, "max": 0, "absent": 0, "kmers": 0, "flags": set(), "dirs": set()}


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


# ------------------------------------------------------------------------------------------ helpers
class Dev:
    def __init__(self, L):
        self.L, self.bufs = L, []

    def alloc(self, nbytes):
        p = self.L.yakamd_dev_alloc(max(nbytes, 16))
        assert p
        self.bufs.append(p)
        return p

    def put(self, data, nbytes=None):
        p = self.alloc(nbytes or len(data))
        if len(data):
            assert self.L.yakamd_memcpy_h2d(p, bytes(data), len(data)) == 0
        return p

    def get(self, p, nbytes):
        out = np.empty(nbytes, np.uint8)
        if nbytes:
            assert self.L.yakamd_memcpy_d2h(out.ctypes.data, p, nbytes) == 0
        return out

    def free(self):
        for p in self.bufs:
            self.L.yakamd_dev_free(p)
        self.bufs = []


def lib_dump(L, h):
    out = C.POINTER(C.c_uint8)()
    n = L.yakamd_dump_mem(h, C.byref(out))
    assert n > 0
    data = C.string_at(out, n)
    C.CDLL(None).free(out)
    return data


NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    NT4[_c] = NT4[_c + 32] = _i
NT4[[ord("U"), ord("u")]] = 3
NT4[:4] = np.arange(4)


def kmer_hash(O, seq, k):
    """the hash of the k-mer seq (k bases, all ACGT), as count.c:28-60 computes it"""
    if k < 32:
        mask, fw, rv = (1 << 2 * k) - 1, 0, 0
        for b in seq:
            c = int(NT4[b])
            fw = (fw << 2 | c) & mask
            rv = rv >> 2 | (3 - c) << 2 * (k - 1)
        return O.yko_hash64(min(fw, rv), mask)
    mask, x = (1 << k) - 1, [0, 0, 0, 0]
    for b in seq:
        c = int(NT4[b])
        x = [(x[0] << 1 | c & 1) & mask, (x[1] << 1 | c >> 1) & mask, x[2] >> 1 | (1 - (c & 1)) << k - 1, x[3] >> 1 | (1 - (c >> 1)) << k - 1]
    return O.yko_hash_long((C.c_uint64 * 4)(*x))


def describe(O, img, k, pre, want, got, bad):
    """position, record (0-based, records end at '\\n'), hash, prefix, expected, actual of the first mismatches"""
    out = []
    for i in bad[:6]:
        i = int(i)
        w = img[i - k + 1:i + 1] if i >= k - 1 else b""
        h = kmer_hash(O, w, k) if len(w) == k and all(NT4[b] < 4 for b in w) else None
        out.append(dict(pos=i, record=img.count(b"\n", 0, i), hash=None if h is None else hex(h),
                        prefix=None if h is None else h & ((1 << pre) - 1), want=int(want[i]), got=int(got[i])))
    return out


def lookup(ya, dev, h, img, width, slack=4096, offset=0):
    """the export of `width` on img; the device buffers are larger than n_bytes, the bases past it ACGT, the output pre-filled with SENT.
    -> (return value, the whole output buffer as elements)"""
    L = ya.lib()
    n = len(img)
    cap = (n + slack + 15) // 16 * 16 + offset
    tail = bytes(np.random.default_rng(n).choice(list(b"ACGT"), cap - n - offset).tolist())
    d_img = dev.put(b"A" * offset + img + tail, cap)
    d_out = dev.put(bytes([SENT]) * (cap * width))
    fn = L.yakamd_lookup_dev if width == 2 else L.yakamd_triobin_lookup_dev
    r = fn(h, d_img + offset, n, d_out)
    raw = dev.get(d_out, cap * width)
    return r, raw.view(np.uint16 if width == 2 else np.uint8)


def check(ya, oracle, h, o, img, width, k, pre):
    """the tables' bytes equal, then the whole device output equal to yko_lookup_image and nothing written at or past n_bytes"""
    L, O = ya.lib(), oracle.lib()
    assert lib_dump(L, h) == oracle.dump_bytes(o), "the library's table is not the oracle's: the lookup is not what is wrong"
    want = oracle.lookup_image(o, img, width)
    dev = Dev(L)
    try:
        r, out = lookup(ya, dev, h, img, width)
    finally:
        dev.free()
    assert r == 0, ya._err()
    got, rest = out[:len(img)], out[len(img):]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, describe(O, img, k, pre, want, got, bad))
    sent = 0xA5A5 if width == 2 else SENT
    assert (rest == sent).all(), ("written past n_bytes", np.flatnonzero(rest != sent)[:8])
    return want


def account(ya, oracle, h, o, img, want, width, tmp_path):
    """what the case contributes to the guards of test_matrix_reached_every_edge.  Which k-mers the table holds is read from a copy of the
    oracle's table whose counts are all set to 1"""
    L, O, pre = ya.lib(), oracle.lib(), o.contents.pre
    nok = 0xFFFF if width == 2 else 0xFF
    cap, size = C.c_uint32(), C.c_uint32()
    for p in range(1 << pre):
        assert L.yakamd_subtable(h, p, C.byref(cap), C.byref(size)) == 0
        SEEN["cap0"] += cap.value == 0
        SEEN["dense"] += cap.value > 0 and size.value > 0.7 * cap.value
    fn = str(tmp_path / "present.yak")
    open(fn, "wb").write(oracle.dump_bytes(o))
    ones = O.yko_ch_restore(fn.encode())
    O.yko_ch_setcnt(ones, 1)
    present = oracle.lookup_image(ones, img, 2) == 1
    O.yko_ch_destroy(ones)
    kmer = want != nok
    SEEN["cases"] += 1
    SEEN["dirs"].add("lds" if pre <= 12 else "global")
    SEEN["kmers"] += int(kmer.sum())
    SEEN["absent"] += int((kmer & ~present).sum())
    SEEN["zero"] += int((present & (want == 0)).sum())
    SEEN["max"] += int((present & (want == 1023)).sum())
    if width == 1:
        SEEN["flags"] |= set(np.unique(want[kmer]).tolist())


# ------------------------------------------------------------------------------------------ inputs
def reads(synth, width, seed, second=False):
    """width 2: ~15x of a 40 kb genome and MOTIF 1100 times (counts up to 1023); width 1: ~3x (counts of at most 15, asserted per case).
    second: the other table of subtract / isec / merge -- the same genome, other reads, and a second genome"""
    if second:
        return synth(1500 if width == 2 else 400, 150, 40000, s=seed, e=0.01, first=200000) + synth(600, 150, 40000, s=seed + 50)
    if width == 2:
        return synth(4000, 150, 40000, s=seed, e=0.005) + (MOTIF + b"\n") * 1100
    return synth(800, 150, 40000, s=seed, e=0.005)


def query(synth, seed):
    """~70 kb: reads of the counted genome (present and absent k-mers), of another genome, MOTIF, one record of ~9 kb across tiles, and
    every kind of byte that breaks a k-mer or does not"""
    rng = np.random.default_rng(seed)
    a = synth(250, 150, 40000, s=seed, e=0.01, first=100000)
    b = synth(60, 150, 40000, s=seed + 50, e=0.005)
    long_rec = synth(60, 150, 40000, s=seed, e=0.002, first=300000).replace(b"\n", b"")
    img = bytearray(a + b + MOTIF + b"\n" + long_rec + b"\n" + b"ACGTU" * 8 + b"\n")
    odd = b"NnRYKMSWBDHVrykmswbdhv-.*\r\0\t @xX\x80\xff" + bytes([4, 5, 6, 7])
    for p in rng.integers(0, len(img), 150):
        img[p] = odd[rng.integers(0, len(odd))]
    for p in rng.integers(0, len(img), 1500):
        if img[p] in b"ACGT":
            img[p] = b"acgtUu\0\1\2\3"[rng.integers(0, 10)]
    return bytes(img)


# ------------------------------------------------------------------------------------------ a. b. table shapes x table histories
# (k, pre) pairs of the width-2 export (k < 32) and of the width-1 export; history j takes Q[j % len(Q)] and T[j % len(T)]: every pre meets
# both a k < 32 and a k >= 32 case, k = 5 meets pre 14
Q = [(5, 14), (11, 10), (15, 11), (21, 12), (27, 13), (31, 14), (21, 10), (31, 12), (15, 13), (27, 11), (11, 14), (5, 12)]
T = [(21, 10), (32, 11), (33, 12), (41, 13), (47, 14), (63, 10), (31, 11), (41, 12), (32, 13), (63, 14), (33, 10), (47, 11), (21, 14)]
# (the library's flag-mode loads take pre <= 13 only -- they need the exclusive-ownership path of the count pass: the two load histories sit where
# Q and T have no pre 14)
HISTORIES = ["pass", "two_pass_fused", "two_pass_recount", "triobin_load", "restore", "shrink_narrow", "clear", "sexchr_load",
             "setcnt0", "setcnt15", "setcnt1023", "inc", "subtract", "isec", "merge", "merge_pre_resize", "tighten"]
CASES = []
for _j, _hist in enumerate(HISTORIES):
    CASES.append((_hist, 2) + Q[_j % len(Q)])
    if _hist != "setcnt1023":                  # counts of 1023 are refused by the one-byte lookup (test_over_15_refusals)
        CASES.append((_hist, 1) + T[_j % len(T)])
CASES += [("two_pass_fused", 2, 21, 10), ("two_pass_recount", 2, 21, 10)]     # where the suite pins which way pass 2 goes (test_gpu_pass2_fused.py)


def build(ya, oracle, synth, knob, tmp_path, hist, width, k, pre):
    """the same table on both sides after `hist` -> (library yak_ch_t *, oracle yko_ch_t *, owners to release)"""
    L, O = ya.lib(), oracle.lib()
    seed = 7 + k + pre
    if hist in ("triobin_load", "sexchr_load"):
        fns = []
        for j in range(2 if hist == "triobin_load" else 3):
            buf = [reads(synth, 2, seed), reads(synth, 2, seed, second=True), synth(2000, 150, 40000, s=seed, e=0.01, first=400000)][j]
            o = O.yko_count_mem(buf, len(buf), C.byref(oracle.copt(k=k, pre=pre)), None)
            fns.append(str(tmp_path / ("p%d.yak" % j)))
            assert O.yko_ch_dump(o, fns[-1].encode()) == 0
            O.yko_ch_destroy(o)
        modes = [(2, fns[0]), (3, fns[1])] if hist == "triobin_load" else [(4, fns[0]), (5, fns[1]), (6, fns[2])]
        h, o = None, None
        for mode, fn in modes:
            h = L.yak_ch_restore_core(h, fn.encode(), mode, C.c_int(2), C.c_int(6))
            o = O.yko_ch_restore_core(o, fn.encode(), mode, 2, 6)
            assert h and o
        return h, o, []
    if hist == "restore":
        buf = reads(synth, width, seed)
        o = O.yko_count_mem(buf, len(buf), C.byref(oracle.copt(k=k, pre=pre)), None)
        fn = str(tmp_path / "t.yak")
        assert O.yko_ch_dump(o, fn.encode()) == 0
        O.yko_ch_destroy(o)
        h, o = L.yak_ch_restore(fn.encode()), O.yko_ch_restore(fn.encode())      # restored in file order: not the counted layout
        assert h and o
        return h, o, []
    buf = reads(synth, width, seed)
    if hist.startswith("two_pass"):
        knob("YAKAMD_CNT2_FUSED", int(hist == "two_pass_fused"))
        bf = pre + 12                            # 4 kb of filter per sub-table
        oc = oracle.copt(k=k, pre=pre, bf_shift=bf)
        o = O.yko_count_protocol_mem(buf, len(buf), None, 0, C.byref(oc))
        dev = Dev(L)
        d = dev.put(buf, len(buf) + 64)
        t = ya.Table(k, pre, 4, bf)
        try:
            assert L.yakamd_retain_input(t.h, 1) == 0
            t.count_pass(1, [(d, len(buf), 0)])
            t.destroy_bf(); t.clear()
            t.count_pass(0, [(d, len(buf), 0)], same_input=True)
            if (k, pre) == (21, 10):
                assert t.stats()["pass2_path"] == (FUSED if hist == "two_pass_fused" else RECOUNT)
            t.shrink(2, 1023)
        finally:
            dev.free()
        return t.h, o, [t]
    t = ya.Table(k, pre, 4, 0)
    t.count_pass_host(1, buf)
    h = t.h
    o = O.yko_count_mem(buf, len(buf), C.byref(oracle.copt(k=k, pre=pre)), None)
    owners = [t]
    if hist == "shrink_narrow":
        lo, hi = (2, 3) if width == 1 else (9, 14)
        L.yak_ch_shrink(h, lo, hi, 1); O.yko_ch_shrink(o, lo, hi)
    elif hist == "clear":
        L.yak_ch_clear(h, 1); O.yko_ch_clear(o)
    elif hist.startswith("setcnt"):
        c = int(hist[6:])
        L.yak_ch_setcnt(h, c, 1); O.yko_ch_setcnt(o, c)
    elif hist == "inc":
        rng = np.random.default_rng(k)
        keys = [kmer_hash(O, buf[i:i + k], k) for i in rng.integers(0, 600 * 151, 300) if all(NT4[b] < 4 for b in buf[i:i + k])]
        keys += [int(x) for x in rng.integers(0, 1 << 62, 40, dtype=np.uint64)]     # mostly absent: -1 on both sides
        for x in keys + (keys[:50] * 3 if width == 2 else []):
            assert L.yak_ch_inc(h, x) == O.yko_ch_inc(o, x)
    elif hist in ("subtract", "isec", "merge", "merge_pre_resize"):
        buf2 = reads(synth, width, seed, second=True)
        t2 = ya.Table(k, pre, 4, 0)
        t2.count_pass_host(1, buf2)
        o2 = O.yko_count_mem(buf2, len(buf2), C.byref(oracle.copt(k=k, pre=pre)), None)
        if hist == "subtract":
            L.yak_ch_subtract(h, t2.h, 1); O.yko_ch_subtract(o, o2)
        elif hist == "isec":
            L.yak_ch_isec(h, t2.h, 1); O.yko_ch_isec(o, o2)
        else:
            pr = int(hist == "merge_pre_resize")
            L.yak_ch_merge(h, t2.h, 1, 1023, 1, pr); O.yko_ch_merge(o, o2, 1, 1023, pr)
            t2.h = o2 = None                         # both merges destroy their second table
        if o2 is not None:
            O.yko_ch_destroy(o2)
        owners.append(t2)
    elif hist == "tighten":
        L.yak_ch_shrink(h, 2, 1023, 1); O.yko_ch_shrink(o, 2, 1023)     # most keys go: tighten then shrinks the sub-tables
        L.yak_ch_tighten(h); O.yko_ch_tighten(o)
    return h, o, owners


@pytest.mark.parametrize("hist,width,k,pre", CASES, ids=["%s-w%d-k%d-p%d" % c for c in CASES])
def test_lookup_equals_oracle(hist, width, k, pre, ya, oracle, synth, knob, tmp_path):
    L, O = ya.lib(), oracle.lib()
    h, o, owners = build(ya, oracle, synth, knob, tmp_path, hist, width, k, pre)
    try:
        if width == 1:
            hist_ = (C.c_int64 * 1024)()
            O.yko_ch_hist(o, hist_)
            assert sum(hist_[16:]) == 0, "the fixture of a one-byte case holds counts above 15"
        img = query(synth, 7 + k + pre)
        want = check(ya, oracle, h, o, img, width, k, pre)
        if hist == "clear":
            assert (want == 0).sum() > 100 and ((want != 0) & (want != (0xFFFF if width == 2 else 0xFF))).sum() == 0
        account(ya, oracle, h, o, img, want, width, tmp_path)
    finally:
        if not owners:
            L.yak_ch_destroy(h)
        for t in owners:
            t.close()
        if o is not None:
            O.yko_ch_destroy(o)


# ------------------------------------------------------------------------------------------ c. query shapes
@pytest.fixture(scope="module")
def shape_tables(ya, oracle, synth, tmp_path_factory):
    """width 2: k = 21 counted at pre 13 (global directory); width 1: the two triobin loads at k = 41, pre 11 (LDS directory)"""
    L, O = ya.lib(), oracle.lib()
    d = tmp_path_factory.mktemp("shapes")
    buf = reads(synth, 2, 5)
    t = ya.Table(21, 13, 4, 0)
    t.count_pass_host(1, buf)
    o2 = O.yko_count_mem(buf, len(buf), C.byref(oracle.copt(k=21, pre=13)), None)
    fns = []
    for j, b in enumerate((reads(synth, 2, 5), reads(synth, 2, 5, second=True))):
        o = O.yko_count_mem(b, len(b), C.byref(oracle.copt(k=41, pre=11)), None)
        fns.append(str(d / ("p%d.yak" % j)))
        assert O.yko_ch_dump(o, fns[-1].encode()) == 0
        O.yko_ch_destroy(o)
    h1 = ya.triobin_table(fns[0], fns[1], 2, 6)
    o1 = O.yko_ch_restore_core(None, fns[0].encode(), 2, 2, 6)
    o1 = O.yko_ch_restore_core(o1, fns[1].encode(), 3, 2, 6)
    yield {2: (t.h, o2, 21, 13), 1: (h1, o1, 41, 11)}
    t.close(); L.yak_ch_destroy(h1); O.yko_ch_destroy(o1); O.yko_ch_destroy(o2)


def long_image(synth):
    """~1.3 Mb: the query image, one record of 1.1 Mb, then reads; every record crosses tile (4096) and workgroup (65536) boundaries somewhere"""
    big = synth(7400, 150, 40000, s=5, e=0.003, first=500000).replace(b"\n", b"")
    return query(synth, 5) + big + b"\n" + synth(400, 150, 40000, s=5, first=600000) + b"N\r\0"


@pytest.mark.parametrize("width", [2, 1])
def test_query_lengths(width, ya, oracle, synth, shape_tables):
    h, o, k, pre = shape_tables[width]
    img = long_image(synth)
    assert len(img) > 1200000
    lengths = [1, 15, 16, k - 1, k, 4095, 4096, 4097, 65535, 65536, 65537, 3 * 65536 + 4097 + 7, len(img)]
    for n in lengths:
        check(ya, oracle, h, o, img[:n], width, k, pre)
    # n_bytes = 0: 0, and nothing written
    dev = Dev(ya.lib())
    try:
        r, out = lookup(ya, dev, h, b"", width)
    finally:
        dev.free()
    assert r == 0 and (out == (0xA5A5 if width == 2 else SENT)).all()


@pytest.mark.parametrize("width", [2, 1])
def test_nothing_written_past_n_bytes_sentinel(width, ya, oracle, synth, shape_tables):
    """the output buffer is 4 kb + longer than n_bytes and the bases past n_bytes are ACGT (k-mers would end there): every element at or past
    n_bytes keeps the sentinel"""
    h, o, k, pre = shape_tables[width]
    img = long_image(synth)
    for n in (k, 4097, 65536 + 13, 200000 + 1):
        check(ya, oracle, h, o, img[:n], width, k, pre)


# ------------------------------------------------------------------------------------------ d. refusals and state
def refused(ya, h, width, img, what, offset=0, untouched=True):
    dev = Dev(ya.lib())
    try:
        r, out = lookup(ya, dev, h, img, width, offset=offset)
    finally:
        dev.free()
    assert r != 0 and what in ya._err(), ya._err()
    assert not untouched or (out == (0xA5A5 if width == 2 else SENT)).all(), "a refused lookup wrote its output"


@pytest.mark.parametrize("width", [2, 1])
def test_misaligned_base_image_is_refused(width, ya, synth, shape_tables):
    h = shape_tables[width][0]
    for off in (1, 8):
        refused(ya, h, width, query(synth, 5)[:5000], "16-byte aligned", offset=off)


def test_lookup_during_an_open_pass_is_refused(ya, synth):
    L = ya.lib()
    buf = reads(synth, 1, 9)
    t = ya.Table(21, 10, 4, 0)
    try:
        t.count_pass_host(1, buf)
        assert L.yakamd_pass_begin(t.h, 0) == 0
        for width in (2, 1):
            refused(ya, t.h, width, buf[:3000], "open pass")
        assert L.yakamd_pass_end(t.h) >= 0
    finally:
        t.close()


def test_qv_lookup_refuses_k_32_and_above(ya, synth):
    buf = reads(synth, 1, 9)
    for k in (32, 41):
        t = ya.Table(k, 10, 4, 0)
        try:
            t.count_pass_host(1, buf)
            refused(ya, t.h, 2, buf[:3000], "k must be below 32")
        finally:
            t.close()


def test_sharded_tables_are_refused(ya, oracle, synth, knob, tmp_path):
    """a yakamd_set_shard range (then the whole range again: the lookup is the oracle's) and several GPUs' table (yak_count with two
    ranks on one device)"""
    L, O = ya.lib(), oracle.lib()
    buf = reads(synth, 1, 9)
    o = O.yko_count_mem(buf, len(buf), C.byref(oracle.copt(k=21, pre=10)), None)
    t = ya.Table(21, 10, 4, 0)
    try:
        t.count_pass_host(1, buf)
        assert L.yakamd_set_shard(t.h, 0, 512) == 0
        for width in (2, 1):
            refused(ya, t.h, width, buf[:3000], "sharded")
        assert L.yakamd_set_shard(t.h, 0, 1024) == 0
        check(ya, oracle, t.h, o, query(synth, 9), 2, 21, 10)
    finally:
        t.close(); O.yko_ch_destroy(o)
    fq = str(tmp_path / "r.fa")
    open(fq, "wb").write(b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(buf.split(b"\n")[:-1])))
    knob("YAKAMD_GPUS", 2)
    knob("YAKAMD_GPU_LIST", "0,0")
    co = ya.CoptT()
    L.yak_copt_init(C.byref(co))
    co.k = 21
    h = L.yak_count(fq.encode(), C.byref(co), None)
    assert h
    try:
        assert L.yakamd_last_sweeps() == 2
        for width in (2, 1):
            refused(ya, h, width, buf[:3000], "sharded")
    finally:
        L.yak_ch_destroy(h)


def _only_over_15(ya, oracle, shape_tables, synth):
    """the width-1 shape table (on both sides) with one key raised above 15, and a query in which that k-mer ends exactly once"""
    L, O = ya.lib(), oracle.lib()
    h, o, k, pre = shape_tables[1]
    src = reads(synth, 2, 5)
    for i in range(0, 20000, 151):
        w = src[i:i + k]
        if all(NT4[b] < 4 for b in w) and O.yko_ch_get(o, kmer_hash(O, w, k)) == 10:
            x = kmer_hash(O, w, k)
            break
    else:
        raise AssertionError("no k-mer of both parents' class 2 in the fixture")
    return h, o, k, pre, x, w


def test_over_15_refusals(ya, oracle, synth, shape_tables, tmp_path):
    """a query meeting the only key above 15 once is refused; the next lookup on a valid flag table succeeds and equals the oracle (the
    over-15 flag of one call does not carry into the next)"""
    L, O = ya.lib(), oracle.lib()
    h, o, k, pre = shape_tables[1]
    fn = str(tmp_path / "t.yak")
    open(fn, "wb").write(lib_dump(L, h))
    h2, o2 = L.yak_ch_restore(fn.encode()), O.yko_ch_restore(fn.encode())
    try:
        _, _, _, _, x, w = _only_over_15(ya, oracle, shape_tables, synth)
        for _ in range(6):
            assert L.yak_ch_inc(h2, x) == O.yko_ch_inc(o2, x)
        assert O.yko_ch_get(o2, x) == 16
        img = query(synth, 77)
        over = lambda v: ((v > 15) & (v != 0xFFFF)).sum()
        assert over(oracle.lookup_image(o2, img, 2)) == 0
        img = img[:30000] + b"\n" + w + b"\n" + img[30000:]
        assert over(oracle.lookup_image(o2, img, 2)) == 1
        refused(ya, h2, 1, img, "above 15", untouched=False)      # the flags are written before the check
        check(ya, oracle, h, o, img, 1, k, pre)
        refused(ya, h2, 1, img, "above 15", untouched=False)      # the flags are written before the check
        check(ya, oracle, h, o, query(synth, 78), 1, k, pre)
    finally:
        L.yak_ch_destroy(h2); O.yko_ch_destroy(o2)


# ------------------------------------------------------------------------------------------ e. the matrix was not degenerate
def test_matrix_reached_every_edge():
    """runs after the cases above (file order): a fixture that shrinks must fail here, not pass vacuously"""
    if SEEN["cases"] < len(CASES):
        pytest.skip("only %d of the %d table cases ran: the guards need the whole file" % (SEEN["cases"], len(CASES)))
    assert SEEN["dirs"] == {"lds", "global"}
    assert SEEN["cap0"] > 0, "no sub-table of capacity 0"
    assert SEEN["dense"] > 0, "no sub-table above 70 % load"
    assert SEEN["zero"] > 0, "no present k-mer with value 0"
    assert SEEN["max"] > 0, "no present k-mer with value 1023"
    assert SEEN["absent"] >= 0.05 * SEEN["kmers"], (SEEN["absent"], SEEN["kmers"])
    assert SEEN["flags"] >= {0, 1, 2, 4, 5, 6, 8, 9, 10}, SEEN["flags"]
