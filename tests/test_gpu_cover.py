"""`yak-amd cover` on the device (kern_cover.inc behind yakamd_cover_dev, yakamd_cover, the CLI and yak_amd.cover) against the numpy restatement
of DESIGN.md section 19 (tests/cover_util.py, held to the reference's numbers and to a second restatement by tests/test_cover.py): the cover bytes
and the masked image byte by byte and the tallies struct by struct on hand-built arrays around every edge of the kernel's tiling, the intervals
through chkerr's run finder, the command byte for byte on the oracle's lookups in any chunking, the refusals, and no host mirror."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import cover_util as U

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
YKO = os.path.join(ROOT, "oracle", "yko")
SYN = os.path.join(ROOT, "tools", "yaksynth")
NO = U.NOKMER
TILE = 4096                                    # positions per tile of k_cover: 256 threads of 16
WAVE = 1024                                    # positions per wave of a tile
GROUP = 16 * TILE                              # positions per workgroup
PAD = 4096                                     # bytes behind every output buffer that must stay as they were
FILL = 0xA5


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


class Dev:
    def __init__(self, L):
        self.L, self.bufs = L, []

    def put(self, arr):
        data = np.ascontiguousarray(arr).tobytes()
        p = self.L.yakamd_dev_alloc(max(len(data), 16))
        assert p
        self.bufs.append(p)
        if data:
            assert self.L.yakamd_memcpy_h2d(p, data, len(data)) == 0
        return p

    def get(self, p, n):
        raw = np.empty(n, np.uint8)
        assert self.L.yakamd_memcpy_d2h(raw.ctypes.data, p, n) == 0
        return raw

    def free(self):
        for p in self.bufs:
            self.L.yakamd_dev_free(p)
        self.bufs = []


def up16(n):
    return (n + 15) & ~15


def cover_dev(ya, t, k, lo, hi, offs=(), lens=(), bases=None, mask=0, n=None, want_rc=0):
    """yakamd_cover_dev on t[0 .. n) -> (cov, masked or None, tallies); the room behind n up to the next multiple of 16 holds a valid count that must
    not be read as part of the array, every output is pre-filled and checked behind its end"""
    L = ya.lib()
    n = len(t) if n is None else n
    offs, lens = np.asarray(offs, np.uint64), np.asarray(lens, np.uint32)
    ns, room = len(lens), up16(n)
    tt = np.full(room, 5, np.uint16)
    tt[:n] = t[:n]
    dev = Dev(L)
    try:
        d_cov = dev.put(np.full(room + PAD, FILL, np.uint8))
        d_msk = dev.put(np.full(room + PAD, FILL, np.uint8)) if mask else None
        d_tal = dev.put(np.full(ns * 16 + PAD, FILL, np.uint8))
        d_img = None
        if bases is not None:
            b = np.full(room, ord("G"), np.uint8)
            b[:n] = np.frombuffer(bytes(bases), np.uint8)[:n]
            d_img = dev.put(b)
        r = L.yakamd_cover_dev(k, lo, hi, dev.put(tt), n, dev.put(offs), dev.put(lens), ns, d_img, mask, d_cov, d_msk, d_tal, None)
        assert r == want_rc, ya._err()
        cov = dev.get(d_cov, room + PAD)
        msk = dev.get(d_msk, room + PAD) if mask else None
        tal = dev.get(d_tal, ns * 16 + PAD)
    finally:
        dev.free()
    if want_rc != 0:
        assert (cov == FILL).all() and (tal == FILL).all() and (msk is None or (msk == FILL).all()), "a refused call wrote"
        return None
    assert (cov[room:] == FILL).all() and (tal[ns * 16:] == FILL).all(), "written behind the end"
    if n > 0:
        assert (cov[n:room] == 0).all()
    if mask:
        assert (msk[room:] == FILL).all(), "written behind the end"
        assert (msk[n:room] == ord("\n")).all()
        msk = msk[:n]
    return cov[:n], msk, tal[:ns * 16].view(U.COV_DTYPE)


def check(ya, t, k, lo=1, hi=1023, offs=(), lens=(), bases=None, mask=0, n=None):
    n = len(t) if n is None else n
    cov, msk, tal = cover_dev(ya, t, k, lo, hi, offs, lens, bases, mask, n)
    want = U.cov(t[:n], k, lo, hi)
    bad = np.flatnonzero(cov != want)
    assert bad.size == 0, (k, lo, hi, n, bad[:8], cov[bad[:8]], want[bad[:8]])
    if mask:
        wm = np.frombuffer(U.masked(bytes(bases[:n]), want, mask), np.uint8)
        bad = np.flatnonzero(msk != wm)
        assert bad.size == 0, (k, mask, bad[:8], msk[bad[:8]], wm[bad[:8]])
    wt = U.tallies(t[:n], offs, lens, k, lo, hi)
    bad = np.flatnonzero(tal != wt)
    assert bad.size == 0, (k, lo, hi, bad[:8], tal[bad[:8]], wt[bad[:8]])
    return cov, tal


def sparse(rng, n, k):
    """counts 0 with hits (a count of 1 .. 1023) at density 1 / k, so that runs merge and split, and 5 % positions without a k-mer"""
    t = np.zeros(n, np.uint16)
    h = rng.random(n) < 1.0 / k
    t[h] = rng.integers(1, 1024, int(h.sum()))
    t[rng.random(n) < 0.05] = NO
    return t


# ---- the cover bytes ----
@pytest.mark.parametrize("k", [1, 2, 21, 31])
def test_sizes_around_16_a_tile_and_a_workgroup(ya, k):
    rng = np.random.default_rng(190 + k)
    for n in (1, 15, 16, 17, TILE - 1, TILE, TILE + 1, GROUP - 1, GROUP, GROUP + 1):
        t = sparse(rng, n, k)
        t[0] = t[n - 1] = 3                                # a hit at element 0 and at n - 1
        check(ya, t, k, offs=[0], lens=[n])
        t[:] = 0
        t[n - 1] = 3                                        # the only hit is the last element
        cov, tal = check(ya, t, k, offs=[0], lens=[n])
        assert int(cov.sum()) == min(k, n) and tuple(tal[0]) == (n, 1, min(k, n), 1)


@pytest.mark.parametrize("k", [1, 2, 21, 31])
def test_isolated_hits_at_every_offset_around_tile_and_wave_edges(ya, k):
    """edge e of the array gets one hit at offset d_e from it, every d in [-(k - 1), k - 1]: tile edges (every 16th a workgroup edge) and, a
    quarter, a half and three quarters of a tile further, wave edges"""
    ds = list(range(-(k - 1), k))
    n = (len(ds) + 2) * TILE
    t = np.zeros(n, np.uint16)
    for e, d in enumerate(ds):
        t[(e + 1) * TILE + d] = 9
        t[(e + 1) * TILE + WAVE * (1 + e % 3) + d] = 9
    cov, tal = check(ya, t, k, offs=[0], lens=[n])
    assert int(cov.sum()) == 2 * len(ds) * k and tuple(tal[0]) == (n, 2 * len(ds), 2 * len(ds) * k, 2 * len(ds))
    for d in sorted({-(k - 1), -1, 0, 1 if k > 1 else 0, k - 1}):      # one hit alone in the array, around the edge between two workgroups
        n2 = GROUP + TILE
        t2 = np.zeros(n2, np.uint16)
        t2[GROUP + d] = 9
        cov, _ = check(ya, t2, k, offs=[0], lens=[n2])
        assert np.flatnonzero(cov).tolist() == list(range(GROUP + d - k + 1, GROUP + d + 1))


@pytest.mark.parametrize("k", [1, 2, 21, 31])
def test_all_none_and_random(ya, k):
    rng = np.random.default_rng(200 + k)
    n = 3 * GROUP + 1234                                   # about three workgroups, not a multiple of anything
    cov, _ = check(ya, np.full(n, 8, np.uint16), k, offs=[0], lens=[n])
    assert cov.all()
    cov, _ = check(ya, np.full(n, NO, np.uint16), k, offs=[0], lens=[n])
    assert not cov.any()
    cov, _ = check(ya, np.zeros(n, np.uint16), k, offs=[0], lens=[n])
    assert not cov.any()
    cov, tal = check(ya, sparse(rng, n, k), k, offs=[0], lens=[n])
    assert 0 < cov.sum() < n and tal["n_run"][0] > 1000
    check(ya, sparse(rng, n, k), k)                        # no sequence: no tally


def test_predicates_with_elements_above_1023(ya):
    rng = np.random.default_rng(210)
    n = TILE + 700
    t = rng.choice(np.array([0, 0, 0, 1, 7, 8, 999, 1000, 1023, 1024, 4000, 0xFFFE, NO, NO], np.uint16), n)
    seen = []
    for lo, hi in ((1, 1023), (0, 0), (7, 7), (1000, 1023), (0, 1023)):
        cov, tal = check(ya, t, 5, lo, hi, offs=[0], lens=[n])
        seen.append(int(tal["n_hit"][0]))
    assert seen[3] == int(np.isin(t, [1000, 1023, 1024, 4000, 0xFFFE]).sum()) and seen[4] == int((t != NO).sum()) and len(set(seen)) == 5


# ---- the masks ----
@pytest.mark.parametrize("mask", [0, 1, 2])
def test_masks_on_every_byte_value(ya, mask):
    rng = np.random.default_rng(220 + mask)
    n = TILE + 256 * 3 + 5
    bases = np.concatenate([np.arange(256, dtype=np.uint8)] * ((n + 255) // 256))[:n]
    t = sparse(rng, n, 3)                                  # k = 3: every byte value meets covered and uncovered positions
    check(ya, t, 3, bases=bases.tobytes(), mask=mask, offs=[0], lens=[n])
    check(ya, np.full(n, 8, np.uint16), 3, bases=bases.tobytes(), mask=mask)
    if mask:
        _, msk, _ = cover_dev(ya, np.full(n, 8, np.uint16), 3, 1, 1023, bases=bases.tobytes(), mask=mask)
        assert bytes(msk[:5]) == (b"\x00\x01\x02\x03\x04" if mask == 1 else b"NNNNN") and bytes(msk[65:68]) == (b"abc" if mask == 1 else b"NNN")


# ---- the tallies ----
def records(rng, k, lens, real):
    """sequences of the given lengths, each followed by one separator element -> (t, offs, lens).  real: the separators and the first k - 1
    elements of every sequence hold no k-mer, as on an image; else they are elements like any other, which the flat definition must bear"""
    offs = np.concatenate(([0], np.cumsum(np.asarray(lens, np.int64) + 1)))[:-1]
    n = int(offs[-1] + lens[-1] + 1)
    t = sparse(rng, n, k)
    if real:
        for o, L in zip(offs, lens):
            t[o:o + min(k - 1, L)] = NO
            t[o + L] = NO
    return t, offs.astype(np.uint64), np.asarray(lens, np.uint32)


@pytest.mark.parametrize("k", [2, 21, 31])
@pytest.mark.parametrize("real", [False, True], ids=["flat", "image"])
def test_tallies_of_many_short_records_and_a_long_one(ya, k, real):
    rng = np.random.default_rng(230 + k)
    short = [0, 1, k - 1, k]
    lens = [short[i % 4] for i in range(3000)] + [3 * GROUP + 77] + [short[(i + 1) % 4] for i in range(3000)] + [150] * 200
    t, offs, lens = records(rng, k, lens, real)
    _, tal = check(ya, t, k, offs=offs, lens=lens)
    assert tal["n_cov"][3000] > GROUP and tal["n_run"][3000] > 100
    check(ya, t, k, 0, 0, offs=offs, lens=lens)


def test_records_that_leave_gaps_and_start_late(ya):
    """positions before the first sequence, between two and behind the last belong to nobody"""
    rng = np.random.default_rng(240)
    n = 2 * TILE + 99
    t = sparse(rng, n, 4)
    check(ya, t, 4, offs=[37, 100, TILE - 3, TILE + 600], lens=[20, 0, 300, TILE - 700])
    check(ya, t, 4, offs=[n - 1], lens=[1])


# ---- the intervals: chkerr's run finder on the cover bytes ----
@pytest.mark.parametrize("k", [2, 21])
def test_intervals_through_the_run_finder(ya, k):
    L = ya.lib()
    rng = np.random.default_rng(250 + k)
    lens = [0, 1, k - 1, k, 150, 999] * 40 + [GROUP + 5000] + [150] * 50
    t, offs, lens = records(rng, k, lens, real=True)
    n, room = len(t), up16(len(t))
    want = U.intervals(t, offs, lens, k, 1, 1023)
    dev = Dev(L)
    try:
        tt = np.full(room, NO, np.uint16)
        tt[:n] = t
        d_cov, d_tal, d_off = dev.put(np.full(room, FILL, np.uint8)), dev.put(np.zeros(len(lens) * 16, np.uint8)), dev.put(offs)
        assert L.yakamd_cover_dev(k, 1, 1023, dev.put(tt), n, d_off, dev.put(lens), len(lens), None, 0, d_cov, None, d_tal, None) == 0, ya._err()
        d_sk, n_sk = C.c_void_p(), C.c_int64()
        assert L.yakamd_chkerr_streaks_dev(-1, d_cov, d_off, len(lens), n, C.byref(d_sk), C.byref(n_sk), None) == 0, ya._err()
        sk = np.empty((n_sk.value, 4), np.uint32)
        if n_sk.value:
            assert L.yakamd_memcpy_d2h(sk.ctypes.data, d_sk, sk.nbytes) == 0
            L.yakamd_dev_free(d_sk)
        tal = dev.get(d_tal, len(lens) * 16).view(U.COV_DTYPE)
    finally:
        dev.free()
    got = [[] for _ in lens]
    for s, st, en, ty in sk.tolist():
        assert ty == 1
        got[s].append((st, en))
    assert got == want and sum(len(g) for g in got) > 1000
    assert [len(g) for g in got] == tal["n_run"].tolist()


# ---- the empty image and the refusals ----
def test_empty_image_and_refusals(ya):
    L = ya.lib()
    t = np.full(64, 3, np.uint16)
    img = b"ACGT" * 16
    cov, msk, tal = cover_dev(ya, t, 21, 1, 1023, bases=img, mask=1, n=0)              # nothing to do, nothing written
    assert len(cov) == 0 and len(tal) == 0
    for kw, what in ((dict(k=0), b"below 32"), (dict(k=32), b"below 32"), (dict(lo=-1), b"1023"), (dict(lo=8, hi=7), b"1023"), (dict(hi=1024), b"1023"),
                     (dict(mask=3), b"mask"), (dict(mask=-1), b"mask"), (dict(mask=1, bases=None), b"image"), (dict(n=-1), b"n_bytes")):
        a = dict(k=21, lo=1, hi=1023, mask=1, bases=img, n=64)
        a.update(kw)
        n = a.pop("n")
        if n < 0:                                                                     # cover_dev sizes its buffers by n
            dev = Dev(L)
            try:
                p = dev.put(np.full(64 + PAD, FILL, np.uint8))
                assert L.yakamd_cover_dev(21, 1, 1023, dev.put(t), -1, None, None, 0, None, 0, p, None, None, None) == -1
                assert L.yakamd_cover_dev(21, 1, 1023, dev.put(t), 64, None, None, -1, None, 0, p, None, None, None) == -1
                assert (dev.get(p, 64 + PAD) == FILL).all()
            finally:
                dev.free()
        else:
            assert cover_dev(ya, t, a["k"], a["lo"], a["hi"], offs=[0], lens=[64], bases=a["bases"], mask=a["mask"], n=n, want_rc=-1) is None
        assert what in L.yakamd_last_error(), (kw, L.yakamd_last_error())
    dev = Dev(L)
    try:
        d_t, d_cov, d_msk, d_img, d_tal = dev.put(t), dev.put(np.full(64 + PAD, FILL, np.uint8)), dev.put(np.full(64 + PAD, FILL, np.uint8)), dev.put(np.zeros(80, np.uint8)), dev.put(np.full(64, FILL, np.uint8))
        d_off, d_len = dev.put(np.zeros(1, np.uint64)), dev.put(np.full(1, 32, np.uint32))
        for a in ((d_t + 2, d_img, d_cov, d_msk), (d_t, d_img + 1, d_cov, d_msk), (d_t, d_img, d_cov + 8, d_msk), (d_t, d_img, d_cov, d_msk + 4)):
            assert L.yakamd_cover_dev(21, 1, 1023, a[0], 32, d_off, d_len, 1, a[1], 1, a[2], a[3], d_tal, None) == -1
            assert b"aligned" in L.yakamd_last_error()
        assert (dev.get(d_cov, 64 + PAD) == FILL).all() and (dev.get(d_msk, 64 + PAD) == FILL).all() and (dev.get(d_tal, 64) == FILL).all()
        assert L.yakamd_cover_dev(21, 1, 1023, d_t, 32, d_off, d_len, 1, d_img + 1, 0, d_cov, None, d_tal, None) == 0      # mask 0 does not look at the image
    finally:
        dev.free()


# ---- the command, end to end ----
@pytest.fixture(scope="module", params=[(21, 10), (31, 12)], ids=["k21p10", "k31p12"])
def e2e(request, oracle, tmp_path_factory):
    """30 x 1000 bp of a 2.5 kb genome with errors and Ns, their variants (lower case, a planted stretch the table lacks, sequences of 1, k - 1 and k
    bases, an empty one) and 4 x 1000 bp of another genome, against the table of 150 bp reads of the first genome"""
    k, pre = request.param
    O = oracle.lib()
    d = tmp_path_factory.mktemp("cover")
    fq, fa0, fa1, fa, tab = str(d / "r.fq"), str(d / "a0.fa"), str(d / "a1.fa"), str(d / "a.fa"), str(d / "t.yak")
    subprocess.check_call([SYN, "-n", "600", "-l", "150", "-g", "2500", "-s", "5", "-o", fq])
    subprocess.check_call([SYN, "-a", "-n", "30", "-l", "1000", "-g", "2500", "-s", "5", "-e", "0.01", "-N", "0.001", "-o", fa0])
    subprocess.check_call([SYN, "-a", "-n", "4", "-l", "1000", "-g", "2500", "-s", "77", "-o", fa1])
    subprocess.run([YKO, "count", f"-k{k}", f"-p{pre}", "-b0", "-o", tab, fq], check=True, stderr=subprocess.DEVNULL)
    recs = U.variants([s for _, s in U.read_fastx(fa0)], k) + [(b"other%d" % i, s) for i, (_, s) in enumerate(U.read_fastx(fa1))] + [(b"empty", b"")]
    with open(fa, "wb") as f:
        for i, (nm, s) in enumerate(recs):                                            # every third record folded into lines of 60
            body = b"\n".join(s[j:j + 60] for j in range(0, len(s), 60)) if i % 3 == 0 and s else s
            f.write(b">" + nm + b" a comment\n" + body + b"\n")
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    assert U.read_fastx(fa) == recs and any(b"N" in s for s in seqs)
    img, offs, lens = U.image(seqs)
    o = O.yko_ch_restore(tab.encode())
    assert o
    t = oracle.lookup_image(o, img, 2)
    O.yko_ch_destroy(o)
    return dict(k=k, fa=fa, tab=tab, dir=d, names=names, img=img, t=t, offs=offs, lens=lens, total=int(lens.sum()),
                text=lambda **kw: U.text(names, t, offs, lens, k, **kw), fasta=lambda **kw: U.fasta(names, img, t, offs, lens, k, **kw))


def cli(args, **kw):
    return subprocess.run([CLI, "cover"] + args, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600, **kw).stdout


def test_table_in_any_chunking(ya, e2e):
    plain, with_b = e2e["text"](), e2e["text"](intervals_too=True)
    assert plain.count(b"\nS\t") == len(e2e["names"]) and with_b.count(b"\nB\t") > 40 and plain.endswith(b"\n") and b"\nT\t%d\t%d\t" % ((len(e2e["names"]),) * 2) in plain
    for chunk in (None, e2e["total"] // 3, 1):                                        # one chunk, about three, one sequence per chunk
        assert ya.cover(e2e["tab"], e2e["fa"], chunk=chunk) == plain, chunk
        assert ya.cover(e2e["tab"], e2e["fa"], intervals=True, chunk=chunk) == with_b, chunk


def test_fasta_masks_and_selection(ya, e2e):
    soft, hard = e2e["fasta"](mask=1), e2e["fasta"](mask=2)
    assert soft != hard and soft.upper() != soft and hard.count(b"N") > 20000
    for chunk in (None, e2e["total"] // 3, 1):
        assert ya.cover(e2e["tab"], e2e["fa"], mask="soft", chunk=chunk) == soft, chunk
        assert ya.cover(e2e["tab"], e2e["fa"], mask="hard", chunk=chunk) == hard, chunk
    keep, drop = e2e["fasta"](mask=0, min_frac=0.5), e2e["fasta"](mask=0, min_frac=0.5, invert=True)
    assert ya.cover(e2e["tab"], e2e["fa"], mask="none", min_frac=0.5, chunk=e2e["total"] // 3) == keep
    assert ya.cover(e2e["tab"], e2e["fa"], mask="none", min_frac=0.5, invert=True) == drop
    heads = lambda b: [ln for ln in b.split(b"\n") if ln[:1] == b">"]
    assert sorted(heads(keep) + heads(drop)) == sorted(b">" + n for n in e2e["names"]) and len(heads(keep)) >= 30 and len(heads(drop)) >= 4
    assert ya.cover(e2e["tab"], e2e["fa"], min_hit=900, intervals=True) == e2e["text"](min_hit=900, intervals_too=True)


def test_the_stretch_the_table_lacks(ya, e2e):
    got = ya.cover(e2e["tab"], e2e["fa"], lo=0, hi=0, intervals=True)
    assert got == e2e["text"](lo=0, hi=0, intervals_too=True)
    b = [tuple(int(x) for x in ln.split(b"\t")[2:]) for ln in got.split(b"\n") if ln.startswith(b"B\tplanted\t")]
    assert any(st <= 45 and en >= 105 for st, en in b)
    assert ya.cover(e2e["tab"], e2e["fa"], lo=2, hi=40) == e2e["text"](lo=2, hi=40)


def test_gzip_cli_and_python(ya, e2e):
    gz = str(e2e["dir"] / "a.fa.gz")
    with gzip.open(gz, "wb") as f:
        f.write(open(e2e["fa"], "rb").read())
    tab, fa = e2e["tab"], e2e["fa"]
    assert ya.cover(tab, gz, intervals=True) == e2e["text"](intervals_too=True)
    assert cli([tab, fa]) == e2e["text"]()
    assert cli(["-b", tab, gz]) == e2e["text"](intervals_too=True)
    assert cli(["-b", "-c", "0:0", "-K", "10k", tab, "-"], input=open(fa, "rb").read()) == e2e["text"](lo=0, hi=0, intervals_too=True)
    assert cli(["-c30", "-n", "5", tab, fa]) == e2e["text"](lo=30, hi=1023, min_hit=5)
    assert cli(["-m", "soft", tab, fa]) == e2e["fasta"](mask=1)
    assert cli(["-mhard", "-K1", tab, gz]) == e2e["fasta"](mask=2)
    assert cli(["-m", "none", "-f", "0.5", tab, fa]) == e2e["fasta"](mask=0, min_frac=0.5)
    assert cli(["-m", "none", "-f", "0.5", "-v", tab, fa]) == e2e["fasta"](mask=0, min_frac=0.5, invert=True)
    out = str(e2e["dir"] / "o.txt")
    assert cli(["-b", "-o", out, tab, fa]) == b"" and open(out, "rb").read() == e2e["text"](intervals_too=True)
    usage = subprocess.run([CLI], stderr=subprocess.PIPE).stderr.decode()
    assert "yak-amd cover" in usage.split("beyond the reference")[1]
    usage = subprocess.run([CLI, "cover"], stderr=subprocess.PIPE).stderr.decode()
    assert "<kmer.yak> <seq.fa>" in usage and "qualities" in usage


def test_no_host_mirror(ya, e2e):
    """across yakamd_cover itself, on a table restored before (yak_ch_init, behind the restore, takes the empty table's mirror once)"""
    L = ya.lib()
    h = L.yak_ch_restore(e2e["tab"].encode())
    assert h, ya._err()
    try:
        o = ya.CvoptT()
        L.yakamd_cvopt_init(C.byref(o))
        o.intervals = 1
        out = str(e2e["dir"] / "mirror.txt")
        before = L.yakamd_host_syncs()
        assert L.yakamd_cover(C.byref(o), h, e2e["fa"].encode(), out.encode()) == 0, ya._err()
        o.mask = 1
        assert L.yakamd_cover(C.byref(o), h, e2e["fa"].encode(), out.encode()) == 0, ya._err()
        assert L.yakamd_host_syncs() == before
        assert open(out, "rb").read() == e2e["fasta"](mask=1)
    finally:
        L.yak_ch_destroy(h)


# ---- refusals: a message, and nothing written ----
def refused(ya, h, fa, out, capfd, what, **opts):
    L = ya.lib()
    o = ya.CvoptT()
    L.yakamd_cvopt_init(C.byref(o))
    assert (o.lo, o.hi, o.intervals, o.mask, o.invert, o.min_hit, o.min_frac, o.n_threads, o.chunk_size) == (1, 1023, 0, -1, 0, 0, 0.0, 8, 1000000000)
    for name, v in opts.items():
        setattr(o, name, v)
    capfd.readouterr()
    assert L.yakamd_cover(C.byref(o), h, fa.encode(), out.encode()) == -1
    err = capfd.readouterr().err + L.yakamd_last_error().decode()
    assert what in err and "yakamd_cover" in err, err
    assert not os.path.exists(out), "a refused call created its output"


def test_refusals(ya, e2e, synth, knob, capfd, tmp_path):
    L = ya.lib()
    out = str(tmp_path / "o.txt")
    buf = synth(300, 150, 2500, s=5)
    t = ya.Table(32, 10, 4, 0)
    try:
        t.count_pass_host(1, buf)
        refused(ya, t.h, e2e["fa"], out, capfd, "below 32")
    finally:
        t.close()
    t = ya.Table(21, 10, 4, 0)
    try:
        t.count_pass_host(1, buf)
        refused(ya, t.h, e2e["fa"], out, capfd, "1023", lo=5, hi=4)
        refused(ya, t.h, e2e["fa"], out, capfd, "1023", lo=-1)
        refused(ya, t.h, e2e["fa"], out, capfd, "1023", hi=1024)
        refused(ya, t.h, e2e["fa"], out, capfd, "fraction", min_frac=1.5)
        refused(ya, t.h, e2e["fa"], out, capfd, "fraction", min_frac=-0.1)
        refused(ya, t.h, e2e["fa"], out, capfd, "hits", min_hit=-1)
        refused(ya, t.h, e2e["fa"], out, capfd, "mask", mask=3)
        refused(ya, t.h, str(tmp_path / "missing.fa"), out, capfd, "cannot open")
        assert L.yakamd_pass_begin(t.h, 0) == 0
        refused(ya, t.h, e2e["fa"], out, capfd, "open pass")
        assert L.yakamd_pass_end(t.h) >= 0
        assert L.yakamd_ch_set_hpc(t.h, 1) == 0
        refused(ya, t.h, e2e["fa"], out, capfd, "homopolymer")
    finally:
        t.close()
    fq = str(tmp_path / "r.fa")
    open(fq, "wb").write(b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(buf.split(b"\n")[:-1])))
    knob("YAKAMD_GPUS", 2)
    knob("YAKAMD_GPU_LIST", "0,0")
    co = ya.CoptT()
    L.yak_copt_init(C.byref(co))
    co.k = 21
    h = L.yak_count(fq.encode(), C.byref(co), None)
    assert h, ya._err()
    try:
        assert L.yakamd_last_sweeps() == 2
        refused(ya, h, e2e["fa"], out, capfd, "sharded")
    finally:
        L.yak_ch_destroy(h)
    k32 = os.path.join(GOLD, "nb_k32.yak")
    for a in (["-o", out, k32, e2e["fa"]], ["-c", "9:3", "-o", out, e2e["tab"], e2e["fa"]], ["-c", "x", "-o", out, e2e["tab"], e2e["fa"]],
              ["-m", "medium", "-o", out, e2e["tab"], e2e["fa"]], ["-f", "2", "-o", out, e2e["tab"], e2e["fa"]], ["-n", "-3", "-o", out, e2e["tab"], e2e["fa"]],
              ["-o", out, e2e["tab"], str(tmp_path / "missing.fa")]):
        r = subprocess.run([CLI, "cover"] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr and not os.path.exists(out), a
