"""Homopolymer compression on the device: the compaction kernels (ASCII and packed input, the sequence remap) against tests/hpc_util.py, counting in
compressed space over every route of yak_count() against plain counting of the host-compressed FASTA and against the oracle on the compressed
image, `yak qv` on a marked table, the command line and the refusals.  Every comparison is exact."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import hpc_util as H

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "yak_amd", "yak-amd")
T = 600


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    assert yak_amd.lib().yakamd_device_count() >= 1
    return yak_amd


class Dev:
    """device buffers of one test, freed at its end"""

    def __init__(self, L):
        self.L, self.bufs = L, []

    def alloc(self, nbytes, fill=0xA5):
        nbytes = max((nbytes + 15) // 16 * 16, 16)
        p = self.L.yakamd_dev_alloc(nbytes)
        assert p
        self.bufs.append(p)
        assert self.L.yakamd_memcpy_h2d(p, bytes([fill]) * nbytes, nbytes) == 0
        return p

    def put(self, data):
        data = bytes(data)
        p = self.alloc(len(data))
        if data:
            assert self.L.yakamd_memcpy_h2d(p, data, len(data)) == 0
        return p

    def get(self, p, nbytes):
        out = C.create_string_buffer(max(nbytes, 1))
        if nbytes:
            assert self.L.yakamd_memcpy_d2h(out, p, nbytes) == 0
        return out.raw[:nbytes]

    def close(self):
        for p in self.bufs:
            self.L.yakamd_dev_free(p)


@pytest.fixture
def dev(ya):
    d = Dev(ya.lib())
    yield d
    d.close()


def records(img):
    """offsets and lengths of the '\\n'-separated records of an image (a last record without its '\\n' too), and a few arbitrary slices"""
    off, ln, p = [], [], 0
    for r in img.split(b"\n"):
        off.append(p); ln.append(len(r)); p += len(r) + 1
    n = len(img)
    r = np.random.default_rng(len(img))
    for _ in range(8):
        o = int(r.integers(0, n + 1))
        off.append(o); ln.append(int(r.integers(0, n - o + 1)))
    off += [0, n, n // 2]; ln += [n, 0, n - n // 2]
    return np.array(off, np.uint64), np.array(ln, np.uint32)


def check_image(ya, dev, img):
    L = ya.lib()
    n = len(img)
    want = H.padded(H.compress(img))
    n_want = len(H.compress(img))
    room = (n + 15) // 16 * 16
    # ASCII, with the remap
    off, ln = records(img)
    ns = len(off)
    d_in, d_out = dev.put(img), dev.alloc(room + 16)
    d_off, d_len, d_oo, d_lo = dev.put(off.tobytes()), dev.put(ln.tobytes()), dev.alloc(8 * ns), dev.alloc(4 * ns)
    got_n = L.yakamd_hpc_dev(d_in, n, d_out, d_off, d_len, ns, d_oo, d_lo, None)
    assert got_n == n_want, ya._err()
    raw = dev.get(d_out, room + 16)
    assert raw[:len(want)] == want
    assert raw[len(want):] == b"\xa5" * (room + 16 - len(want))         # nothing behind the fill
    woff, wlen = H.remap(img, off, ln)
    assert np.array_equal(np.frombuffer(dev.get(d_oo, 8 * ns), np.uint64), woff)
    assert np.array_equal(np.frombuffer(dev.get(d_lo, 4 * ns), np.uint32), wlen)
    assert L.yakamd_hpc_dev(d_in, n, d_out, None, None, 0, None, None, None) == n_want      # the arrays may be NULL
    # packed: the last code word and the last validity word may be partial
    codes, valid = H.pack(img)
    d_c, d_v, d_out2 = dev.put(codes.tobytes()), dev.put(valid.tobytes()), dev.alloc(room + 16)
    assert L.yakamd_hpc_packed_dev(d_c, d_v, n, d_out2, None) == n_want, ya._err()
    raw = dev.get(d_out2, room + 16)
    assert raw[:len(want)] == want and raw[len(want):] == b"\xa5" * (room + 16 - len(want))


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, (1 << 20) + 3])
def test_compaction_of_random_images(n, ya, dev):
    check_image(ya, dev, H.random_image(n, 100 + n % 97))


def boundary_image():
    """runs that end exactly at, one before and one behind the multiples of 16, 32, 64, 256, 1024 and 4096 -- the lanes', waves' and tiles' edges of
    both input forms (a tile is 4096 positions of ASCII, 16384 packed) -- in an image of five packed tiles and a bit"""
    n = 5 * 16384 + 7
    a = np.frombuffer(H.random_image(n, 7, p_repeat=0.2), np.uint8).copy()
    r = np.random.default_rng(8)
    for B, ms in ((16, (1, 2, 255, 256, 257)), (32, (1, 3, 127)), (64, (1, 5, 63, 64)), (256, (1, 2, 15, 17)), (1024, (1, 3, 4, 15, 17)), (4096, (1, 2, 3, 4, 5, 8, 12, 16, 20))):
        for m in ms:
            for d in (-1, 0, 1):
                e = B * m + d                                        # the run is [e - l, e)
                l = int(r.integers(2, 12))
                a[e - l:e] = b"ACGT"[int(r.integers(0, 4))]
    a[16384 - 3:16384 + 5] = ord("T")                               # and runs that cross them
    a[4096 * 6 - 40:4096 * 6 + 40] = ord("c")
    return a.tobytes()


PLANTED_GPU = H.PLANTED + [
    boundary_image(),
    H.random_image(9000, 3)[:4090] + b"A" * 70001 + H.random_image(5000, 4),           # a run longer than any tile
    b"ACGT" * 1024 + b"\n" + b"G" * 4096 + b"\n" + b"G" * 4096,                           # tiles that keep one byte, or none
    b"".join(bytes([c]) * (i % 37 + 1) for i, c in enumerate(b"ACGTNacgtn\nTU" * 700)),     # every length of run up to 37
    b"N" * 5000 + b"A" * 5000 + b"\n" * 5000,
    bytes(range(256)) * 40,
]


@pytest.mark.parametrize("i", range(len(PLANTED_GPU)))
def test_compaction_of_planted_images(i, ya, dev):
    check_image(ya, dev, PLANTED_GPU[i])


# ---- counting in compressed space ----
def fasta(recs, fn):
    with open(fn, "wb") as f:
        for i, r in enumerate(recs):
            f.write(b">r%d\n%s\n" % (i, r))
    return fn


@pytest.fixture(scope="module")
def reads(synth, tmp_path_factory):
    """about 20 k reads with homopolymer runs of up to 40 written over a third of them: the raw FASTA (plain and .gz), the host-compressed FASTA and
    the compressed image"""
    d = tmp_path_factory.mktemp("hpc")
    img = H.plant_runs(synth(20000, g=100000, s=21), 3)
    recs = img.split(b"\n")[:-1]
    raw = fasta(recs, str(d / "raw.fa"))
    with open(raw, "rb") as f, gzip.open(str(d / "raw.fa.gz"), "wb", compresslevel=1) as g:
        g.write(f.read())
    comp = fasta([H.compress_seq(r) for r in recs], str(d / "comp.fa"))
    return dict(img=img, raw=raw, gz=str(d / "raw.fa.gz"), comp=comp, cimg=H.compress(img), dir=str(d))


CASES = {"k31_b0": dict(k=31, bf=0), "k31_filtered": dict(k=31, bf=24), "k21_b0": dict(k=21, bf=0)}


def protocol(ya, count, fn, k, bf, count2=None):
    """`yak count` (reference main.c:53-61) with `count` for the first pass and count2 (default: the same) for the second -> .yak bytes"""
    L = ya.lib()
    o = ya.CoptT(); L.yak_copt_init(C.byref(o)); o.k, o.bf_shift = k, bf
    h = count(fn.encode(), C.byref(o), None)
    assert h, ya._err()
    t = ya.Table(ptr=h)
    try:
        if bf:
            t.destroy_bf(); t.clear()
            assert (count2 or count)(fn.encode(), C.byref(o), t.h), ya._err()
            t.shrink(2, 1023)
        return t.dump_bytes()
    finally:
        t.close()


_want = {}


def want_bytes(ya, oracle, reads, case):
    """plain yak_count of the host-compressed FASTA, which is also the oracle's count of the compressed image; computed once per case"""
    if case not in _want:
        c = CASES[case]
        plain = protocol(ya, ya.lib().yak_count, reads["comp"], c["k"], c["bf"])
        assert plain == oracle.count_protocol_mem(reads["cimg"], k=c["k"], bf_shift=c["bf"])[0]
        _want[case] = plain
    return _want[case]


ROUTES = {
    "plain_file": ("raw", {}),
    "no_host_pack": ("raw", {"YAKAMD_NO_HOST_PACK": 1}),
    "gz": ("gz", {}),
    "pipe": ("pipe", {}),
    "batch_4096": ("raw", {"YAKAMD_BATCH": 4096}),
    "no_retain": ("raw", {"YAKAMD_NO_RETAIN": 1}),
    "two_ranks": ("raw", {"YAKAMD_GPUS": 2}),
}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", list(CASES))
def test_count_hpc_equals_plain_count_of_the_compressed_file(case, route, ya, oracle, reads, knob):
    src, knobs = ROUTES[route]
    for name, v in knobs.items():
        knob(name, v)
    fn = reads["raw"] if src == "pipe" else reads[src]
    c = CASES[case]
    if src == "pipe":                                               # a named pipe: nothing to map, nothing to stat, one pass per open
        fifo = os.path.join(reads["dir"], "fifo_%s" % case)
        if not os.path.exists(fifo):
            os.mkfifo(fifo)

        def count(_, o, h):
            p = subprocess.Popen(["sh", "-c", 'cat "$0" > "$1"', reads["raw"], fifo])   # the writer's open waits in the child for the reader
            try:
                return ya.lib().yakamd_count_hpc(fifo.encode(), o, h)
            finally:
                p.wait(timeout=T)
        got = protocol(ya, count, fifo, c["k"], c["bf"])
    else:
        got = protocol(ya, ya.lib().yakamd_count_hpc, fn, c["k"], c["bf"])
    assert got == want_bytes(ya, oracle, reads, case)


@pytest.mark.parametrize("case", ["k31_filtered"])
def test_yak_count_on_a_marked_table_compresses_too(case, ya, oracle, reads):
    c = CASES[case]
    L = ya.lib()
    assert protocol(ya, L.yakamd_count_hpc, reads["raw"], c["k"], c["bf"], count2=L.yak_count) == want_bytes(ya, oracle, reads, case)


def test_plain_count_of_the_raw_file_differs(ya, oracle, reads):
    """the negative control: the input tells the two spaces apart"""
    assert protocol(ya, ya.lib().yak_count, reads["raw"], 31, 0) != want_bytes(ya, oracle, reads, "k31_b0")


@pytest.mark.parametrize("packed", [0, 1])
def test_direct_feeds_into_a_marked_table(packed, ya, oracle, reads, dev):
    L = ya.lib()
    img = reads["img"][:151 * 6000]
    cut = 151 * 2500                                                # two feeds: the second one's t0 is its uncompressed stream position
    t = ya.Table(21, 10, 4, 0)
    try:
        assert L.yakamd_ch_hpc(t.h) == 0 and L.yakamd_ch_set_hpc(t.h, 1) == 0 and L.yakamd_ch_hpc(t.h) == 1
        parts = [(img[:cut], 0), (img[cut:], cut)]
        if packed:
            feeds = []
            for b, t0 in parts:
                codes, valid = H.pack(b)
                feeds.append((dev.put(codes.tobytes()), dev.put(valid.tobytes()), len(b), t0))
            t.count_pass_packed(1, feeds)
        else:
            t.count_pass(1, [(dev.put(b), len(b), t0) for b, t0 in parts])
        assert t.dump_bytes() == oracle.count_protocol_mem(H.compress(img), k=21)[0]
        assert L.yakamd_ch_set_hpc(t.h, 0) == 0 and L.yakamd_ch_hpc(t.h) == 0
    finally:
        t.close()


def test_a_sequence_longer_than_a_multi_rank_chunk(ya, oracle, knob, tmp_path):
    """two ranks and chunks of 8192 bases: a sequence of 60 k bases is cut inside, and in compressed space the next chunk opens with the last k - 1
    KEPT positions of the one before"""
    seq = H.random_image(60000, 31, p_repeat=0.6, p_n=0.0005, p_lower=0.0, p_nl=0.0)
    raw = fasta([seq, seq[100:30000]], str(tmp_path / "long.fa"))
    comp = fasta([H.compress_seq(seq), H.compress_seq(seq[100:30000])], str(tmp_path / "long_c.fa"))
    want = protocol(ya, ya.lib().yak_count, comp, 31, 0)
    assert want == oracle.count_protocol_mem(H.compress(seq + b"\n" + seq[100:30000] + b"\n"), k=31)[0]
    knob("YAKAMD_GPUS", 2); knob("YAKAMD_MGPU_CHUNK", 8192)
    assert protocol(ya, ya.lib().yakamd_count_hpc, raw, 31, 0) == want


# ---- qv, the command line, the refusals ----
@pytest.fixture(scope="module")
def qv_inputs(ya, reads, synth):
    """a table counted in compressed space, and sequences to evaluate: raw, and host-compressed under the same names"""
    L = ya.lib()
    d = reads["dir"]
    o = ya.CoptT(); L.yak_copt_init(C.byref(o)); o.k, o.bf_shift = 21, 0
    h = L.yakamd_count_hpc(reads["raw"].encode(), C.byref(o), None)
    assert h, ya._err()
    tab = os.path.join(d, "hpc21.yak")
    assert L.yak_ch_dump(h, tab.encode()) == 0
    L.yak_ch_destroy(h)
    recs = H.plant_runs(synth(600, g=100000, s=21, e=0.02), 2, seed=4).split(b"\n")[:-1]
    recs += [b"", b"AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA", recs[0] * 40, b"ACGTNNNNNNACGT" * 9]
    raw = fasta(recs, os.path.join(d, "q_raw.fa"))
    comp = fasta([H.compress_seq(r) for r in recs], os.path.join(d, "q_comp.fa"))
    return tab, raw, comp


def run_cli(args):
    r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=T)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r.stdout


@pytest.mark.parametrize("flags", [["-p", "-E"], ["-p", "-l", "100"], []], ids=["p_E", "p_min_len", "parallel_reader"])
def test_qv_on_a_marked_table_prints_what_the_compressed_file_gives(flags, qv_inputs):
    tab, raw, comp = qv_inputs
    want = run_cli(["qv"] + flags + [tab, comp])
    assert want.count(b"\n") > 1000 or not flags
    for K in ("1g", "20000", "700"):
        assert run_cli(["qv", "-c", "-K", K] + flags + [tab, raw]) == want
    assert run_cli(["qv"] + flags + [tab, raw]) != want                # the negative control


def test_yak_qv_counts_on_a_marked_table(ya, qv_inputs):
    L = ya.lib()
    tab, raw, comp = qv_inputs
    want = ya.qv_counts(tab, comp)
    h = L.yak_ch_restore(tab.encode())
    assert h and L.yakamd_ch_set_hpc(h, 1) == 0
    o = ya.QoptT(); L.yak_qopt_init(C.byref(o))
    cnt = (C.c_int64 * 1024)()
    L.yak_qv(C.byref(o), raw.encode(), h, cnt)
    L.yak_ch_destroy(h)
    assert list(cnt) == want and sum(want) > 0
    assert ya.qv_counts(tab, raw) != want


@pytest.mark.parametrize("case", ["k31_b0", "k31_filtered"])
def test_cli_count_c_equals_the_library(case, ya, oracle, reads, tmp_path):
    c = CASES[case]
    out = str(tmp_path / "cli.yak")
    run_cli(["count", "-c", "-k%d" % c["k"], "-b%d" % c["bf"], "-o", out, reads["raw"]])
    assert open(out, "rb").read() == want_bytes(ya, oracle, reads, case)


def test_refusals(ya, reads, tmp_path, capfd):
    L = ya.lib()
    o = ya.CoptT(); L.yak_copt_init(C.byref(o)); o.k = 21
    plain = ya.Table(21, 10, 4, 0)
    marked = ya.Table(21, 10, 4, 0)
    try:
        # yakamd_count_hpc on an unmarked table
        assert not L.yakamd_count_hpc(reads["raw"].encode(), C.byref(o), plain.h)
        assert b"not marked" in L.yakamd_last_error() and plain.tot == 0
        # the mark inside an open pass
        assert L.yakamd_pass_begin(marked.h, 1) == 0
        assert L.yakamd_ch_set_hpc(marked.h, 1) == -1 and b"open pass" in L.yakamd_last_error() and L.yakamd_ch_hpc(marked.h) == 0
        assert L.yakamd_pass_end(marked.h) == 0
        assert L.yakamd_ch_set_hpc(marked.h, 1) == 0
        # the lookup commands that read uncompressed sequence
        fn = reads["raw"].encode()
        tb, te, ce, sc, dp = ya.TboptT(), ya.TeoptT(), ya.CeoptT(), ya.ScoptT(), ya.DpoptT()
        L.yakamd_tbopt_init(C.byref(tb)); L.yakamd_teopt_init(C.byref(te)); L.yakamd_ceopt_init(C.byref(ce)); L.yakamd_scopt_init(C.byref(sc)); L.yakamd_dpopt_init(C.byref(dp))
        calls = {
            "yakamd_triobin": lambda out: L.yakamd_triobin(C.byref(tb), marked.h, fn, out),
            "yakamd_trioeval": lambda out: L.yakamd_trioeval(C.byref(te), marked.h, fn, out),
            "yakamd_chkerr": lambda out: L.yakamd_chkerr(C.byref(ce), marked.h, fn, out),
            "yakamd_sexchr": lambda out: L.yakamd_sexchr(C.byref(sc), marked.h, fn, fn, out),
            "yakamd_depth": lambda out: L.yakamd_depth(C.byref(dp), marked.h, fn, out),
        }
        for name, call in calls.items():
            out = str(tmp_path / (name + ".out"))
            assert call(out.encode()) == -1, name
            assert name.encode() in L.yakamd_last_error() and b"homopolymer" in L.yakamd_last_error()
            assert not os.path.exists(out), name
        assert b"homopolymer" in capfd.readouterr().err.encode()
    finally:
        plain.close(); marked.close()
