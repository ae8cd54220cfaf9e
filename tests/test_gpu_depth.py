"""`yak-amd depth` on the device (kern_depth.inc behind yakamd_depth_reduce_dev, yakamd_depth, the CLI and yak_amd.depth) against the numpy
restatement of DESIGN.md section 16 (tests/depth_util.py, held to the reference's numbers by tests/test_depth.py): the reduction struct by struct on
hand-written arrays through every path (values in registers, read again, histograms over many workgroups, groups and batches), the command byte
for byte on the oracle's lookups in any chunking and from .gz, the refusals, and no host mirror."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD, ROOT
import depth_util as U

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
YKO = os.path.join(ROOT, "oracle", "yko")
SYN = os.path.join(ROOT, "tools", "yaksynth")
NO = U.NOKMER
K = 21
POISON = 1000                                  # a valid count where no window may look: separators and the k - 1 lead-in elements


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


class Dev:
    def __init__(self, L):
        self.L, self.bufs = L, []

    def put(self, arr, nbytes=None):
        data = np.ascontiguousarray(arr).tobytes()
        p = self.L.yakamd_dev_alloc(max(nbytes or len(data), 16))
        assert p
        self.bufs.append(p)
        if data:
            assert self.L.yakamd_memcpy_h2d(p, data, len(data)) == 0
        return p

    def free(self):
        for p in self.bufs:
            self.L.yakamd_dev_free(p)
        self.bufs = []


def counts(rng, n):
    """skewed counts with heavy ties: mostly a narrow peak, a tail up to 1023, zeros, and 5 % positions without a k-mer"""
    v = np.minimum(rng.geometric(0.08, n) + 20, 1023)
    v[rng.random(n) < 0.15] = 0
    tail = rng.random(n) < 0.04
    v[tail] = rng.integers(900, 1024, int(tail.sum()))
    v[rng.random(n) < 0.05] = NO
    return v.astype(np.uint16)


def layout(rng, n_pos, fill=None, k=K):
    """sequences whose whole-sequence windows have n_pos[j] positions (0: alternately an empty sequence and one of k - 1 bases) -> (t, offs, lens);
    fill[j]: the window's values instead of random ones"""
    parts, offs, lens, at = [], [], [], 0
    for j, n in enumerate(n_pos):
        L = n + k - 1 if n else (0 if j % 2 == 0 else k - 1)
        v = np.full(L + 1, POISON, np.uint16)
        if n:
            v[k - 1:L] = counts(rng, n) if fill is None or fill[j] is None else fill[j]
        parts.append(v); offs.append(at); lens.append(L)
        at += L + 1
    t = np.concatenate(parts + [np.full(16 - at % 16, POISON, np.uint16)])       # the allocation: a multiple of 16 bytes
    return t, np.array(offs, np.uint64), np.array(lens, np.uint32), at


def reduce_dev(ya, t, offs, lens, n_bytes, w, k=K):
    L = ya.lib()
    woff = U.win_off(lens, w)
    n_win = int(woff[-1])
    dev = Dev(L)
    try:
        d_win = dev.put(np.full(n_win * 24 + 64, 0xA5, np.uint8))
        r = L.yakamd_depth_reduce_dev(k, w, dev.put(t), dev.put(offs), dev.put(lens), dev.put(woff), len(lens), n_bytes, d_win, None)
        assert r == 0, ya._err()
        raw = np.empty(n_win * 24 + 64, np.uint8)
        assert L.yakamd_memcpy_d2h(raw.ctypes.data, d_win, len(raw)) == 0
    finally:
        dev.free()
    assert (raw[n_win * 24:] == 0xA5).all(), "written past the last window"
    return raw[:n_win * 24].view(U.WIN_DTYPE)


def check(ya, t, offs, lens, n_bytes, w, k=K):
    got, want = reduce_dev(ya, t, offs, lens, n_bytes, w, k), U.structs(t, offs, lens, k, w)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (w, bad[:5], got[bad[:5]], want[bad[:5]])
    return got


@pytest.fixture(scope="module")
def small():
    """window lengths around every boundary of the short path (64 lanes, 512 values in registers, the default threshold of 2048), an all-0xffff
    window, an all-1023 one, one of equal values, empty sequences in between"""
    rng = np.random.default_rng(16)
    n_pos = [0, 1, 63, 0, 64, 65, 255, 256, 257, 0, 0, 511, 512, 513, 300, 300, 300, 2047, 2048, 2049, 5000, 2, 0]
    fill = [None] * len(n_pos)
    fill[14], fill[15], fill[16] = np.full(300, NO, np.uint16), np.full(300, 1023, np.uint16), np.full(300, 37, np.uint16)
    return layout(rng, n_pos, fill)


@pytest.fixture(scope="module")
def large():
    """511, 512, 513 positions and one window of 300 000: many tiles and workgroups of the histogram kernel"""
    return layout(np.random.default_rng(17), [511, 300000, 512, 0, 513, 40000])


@pytest.mark.parametrize("w", [0, 1, 7, 1000])
def test_reduce_small_windows(ya, small, w):
    got = check(ya, *small, w)
    if w == 0:
        assert got["n_kmer"][14] == 0 and tuple(got[15]) == (300, 300, 1023, 1023, 300 * 1023) and got["median"][16] == 37
        assert (got["n_kmer"][[0, 3, 9, 10, 22]] == 0).all()


@pytest.mark.parametrize("w", [0, 1000, 100000])
def test_reduce_long_windows_at_both_thresholds(ya, large, knob, w):
    at_default = check(ya, *large, w)
    knob("YAKAMD_DEPTH_LONG", 512)
    at_512 = check(ya, *large, w)
    assert np.array_equal(at_default, at_512)
    if w == 0:
        assert at_512["n_kmer"][1] > 280000


def test_reduce_small_windows_at_threshold_512_and_0(ya, small, knob):
    want = check(ya, *small, 0)
    for T in (512, 0):                        # 0: every window that has a position through the histogram kernels
        knob("YAKAMD_DEPTH_LONG", T)
        assert np.array_equal(check(ya, *small, 0), want)
        assert np.array_equal(check(ya, *small, 1000), U.structs(*small[:3], K, 1000))


def test_reduce_in_batches(ya, small, large, knob):
    """the second test switch lowers the batch from 2^24 windows: short windows in many batches, long ones in several"""
    knob("YAKAMD_DEPTH_BATCH", 1000)
    assert len(check(ya, *small, 1)) > 10000
    check(ya, *small, 7)
    knob("YAKAMD_DEPTH_BATCH", 64)
    knob("YAKAMD_DEPTH_LONG", 512)
    assert len(check(ya, *large, 1000)) > 5 * 64


def test_reduce_more_long_windows_than_one_group(ya, knob):
    """more than 16384 long windows in one batch: their histograms are held group after group"""
    rng = np.random.default_rng(18)
    n = 513 * 16500 + 100
    t, offs, lens, nb = layout(rng, [n, 700])
    knob("YAKAMD_DEPTH_LONG", 512)
    got = check(ya, t, offs, lens, nb, 513)
    assert len(got) > 16384 + 100


def test_reduce_other_k_and_arguments(ya):
    L = ya.lib()
    rng = np.random.default_rng(19)
    for k in (1, 5, 31):
        t, offs, lens, nb = layout(rng, [0, 3, 700, 64, 0, 2100], k=k)
        for w in (0, 50):
            check(ya, t, offs, lens, nb, w, k)
    t, offs, lens, nb = layout(rng, [10])
    dev = Dev(L)
    try:
        args = [dev.put(t), dev.put(offs), dev.put(lens), dev.put(U.win_off(lens, 0))]
        d_win = dev.put(np.zeros(64, np.uint8))
        assert L.yakamd_depth_reduce_dev(K, 0, *args, 0, nb, d_win, None) == 0             # no sequence: nothing to do
        assert L.yakamd_depth_reduce_dev(32, 0, *args, 1, nb, d_win, None) == -1 and b"below 32" in L.yakamd_last_error()
        assert L.yakamd_depth_reduce_dev(K, -1, *args, 1, nb, d_win, None) == -1 and b"window" in L.yakamd_last_error()
        assert L.yakamd_depth_reduce_dev(K, 0, *args, -1, nb, d_win, None) == -1
        assert L.yakamd_depth_reduce_dev(K, 0, args[0] + 2, *args[1:], 1, nb, d_win, None) == -1 and b"aligned" in L.yakamd_last_error()
    finally:
        dev.free()


# ---- the command, end to end ----
@pytest.fixture(scope="module", params=[(21, 10), (31, 12)], ids=["k21p10", "k31p12"])
def e2e(request, oracle, tmp_path_factory):
    """30 x 1000 bp of a 2.5 kb genome with errors and Ns, and the table of 150 bp reads of the same genome; the expected lines per window size
    from the oracle's lookups"""
    k, pre = request.param
    O = oracle.lib()
    d = tmp_path_factory.mktemp("depth")
    fq, fa, tab = str(d / "r.fq"), str(d / "a.fa"), str(d / "t.yak")
    subprocess.check_call([SYN, "-n", "600", "-l", "150", "-g", "2500", "-s", "5", "-o", fq])
    subprocess.check_call([SYN, "-a", "-n", "30", "-l", "1000", "-g", "2500", "-s", "5", "-e", "0.01", "-N", "0.001", "-o", fa])
    subprocess.run([YKO, "count", f"-k{k}", f"-p{pre}", "-b0", "-o", tab, fq], check=True, stderr=subprocess.DEVNULL)
    recs = U.read_fastx(fa)
    assert len(recs) == 30 and any(b"N" in s for _, s in recs)
    img, offs, lens = U.image([s for _, s in recs])
    o = O.yko_ch_restore(tab.encode())
    assert o
    t = oracle.lookup_image(o, img, 2)
    O.yko_ch_destroy(o)
    want = {w: U.text([n for n, _ in recs], t, offs, lens, k, w) for w in (0, 100)}
    assert want[0].count(b"\n") == 31 and want[100].count(b"\n") == 301 and b"\t0\t0\t0.000\t0\t0\n" not in want[0]
    return dict(k=k, fa=fa, tab=tab, want=want, dir=d)


@pytest.mark.parametrize("w", [0, 100])
def test_depth_equals_restatement_in_any_chunking(ya, e2e, w):
    one = ya.depth(e2e["tab"], e2e["fa"], window=w)
    assert one == e2e["want"][w]
    assert ya.depth(e2e["tab"], e2e["fa"], window=w, chunk=10000) == one          # three chunks of ten sequences


def test_depth_gzip_cli_and_batches(ya, e2e, knob):
    gz = str(e2e["dir"] / "a.fa.gz")
    with gzip.open(gz, "wb") as f:
        f.write(open(e2e["fa"], "rb").read())
    assert ya.depth(e2e["tab"], gz, window=100) == e2e["want"][100]
    knob("YAKAMD_DEPTH_BATCH", 7)
    assert ya.depth(e2e["tab"], e2e["fa"], window=100) == e2e["want"][100]
    run = lambda a, **kw: subprocess.run([CLI, "depth"] + a, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600, **kw).stdout
    assert run(["-w", "100", e2e["tab"], e2e["fa"]]) == e2e["want"][100]
    assert run([e2e["tab"], gz]) == e2e["want"][0]
    assert run(["-K", "10k", e2e["tab"], "-"], input=open(e2e["fa"], "rb").read()) == e2e["want"][0]
    out = str(e2e["dir"] / "o.txt")
    assert run(["-w100", "-o", out, e2e["tab"], e2e["fa"]]) == b"" and open(out, "rb").read() == e2e["want"][100]
    usage = subprocess.run([CLI], stderr=subprocess.PIPE).stderr.decode()
    assert "beyond the reference" in usage and "yak-amd depth" in usage.split("beyond the reference")[1]


def test_no_host_mirror(ya, e2e):
    """across yakamd_depth itself, on a table restored before (yak_ch_init, behind the restore, takes the empty table's mirror once)"""
    L = ya.lib()
    h = L.yak_ch_restore(e2e["tab"].encode())
    assert h, ya._err()
    try:
        o = ya.DpoptT()
        L.yakamd_dpopt_init(C.byref(o))
        o.window = 100
        out = str(e2e["dir"] / "mirror.txt")
        before = L.yakamd_host_syncs()
        assert L.yakamd_depth(C.byref(o), h, e2e["fa"].encode(), out.encode()) == 0, ya._err()
        assert L.yakamd_host_syncs() == before
        assert open(out, "rb").read() == e2e["want"][100]
        L.yak_ch_get.restype = C.c_int
        L.yak_ch_get(h, 12345)
        assert L.yakamd_host_syncs() == before + 1                # the counter does see a mirror being built
    finally:
        L.yak_ch_destroy(h)


# ---- refusals: a message, and nothing written ----
def refused(ya, h, fa, out, capfd, what, window=0):
    L = ya.lib()
    o = ya.DpoptT()
    L.yakamd_dpopt_init(C.byref(o))
    assert (o.window, o.n_threads, o.chunk_size) == (0, 8, 1000000000)
    o.window = window
    capfd.readouterr()
    assert L.yakamd_depth(C.byref(o), h, fa.encode(), out.encode()) == -1
    err = capfd.readouterr().err
    assert what in err and "yakamd_depth" in err, err
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
        refused(ya, t.h, e2e["fa"], out, capfd, "window", window=-1)
        refused(ya, t.h, str(tmp_path / "missing.fa"), out, capfd, "cannot open")
        assert L.yakamd_pass_begin(t.h, 0) == 0
        refused(ya, t.h, e2e["fa"], out, capfd, "open pass")
        assert L.yakamd_pass_end(t.h) >= 0
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
    for a in (["-o", out, k32, e2e["fa"]], ["-w", "-5", "-o", out, e2e["tab"], e2e["fa"]], ["-o", out, e2e["tab"], str(tmp_path / "missing.fa")]):
        r = subprocess.run([CLI, "depth"] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode != 0 and r.stdout == b"" and r.stderr and not os.path.exists(out), a
