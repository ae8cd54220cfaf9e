"""yak_ch_clear is deferred (engine_table.cpp yk_ctx_clear: k_img_clear runs when the image is next read or written), and the count pass over the
input of the pass before takes a pending clear over: one sweep raises every count by one and k_cnt2_apply probes only the keys whose count is
something else (engine_count.cpp yakamd_count_retained; the rule itself: tests/test_pass2_bump.py).  Against the oracle, byte for byte: the
protocol with that branch on and off (YAKAMD_PASS2_BUMP), everything that can look at a table between a clear and the next pass, the retained sets
that must not take the branch, and a count pass without a clear in front."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import paths_util
from test_pass2_bump import BOUNDARY, SATURATION, table_counts

pytestmark = pytest.mark.gpu

FUSED = 1
SHAPES = {"k31b22": (lambda synth: synth(20000, g=90000, s=21), dict(k=31, bf_shift=22)),
          "k21b20": (lambda synth: synth(20000, g=90000, s=21), dict(k=21, bf_shift=20)),
          "saturation": (lambda synth: SATURATION + BOUNDARY, dict(k=31, bf_shift=20))}
shapes = pytest.mark.parametrize("shape", sorted(SHAPES))


@pytest.fixture(scope="module")
def ya():
    import yak_amd
    L = yak_amd.lib()
    assert L.yakamd_device_count() >= 1, "GPU tests need an MI355X; the engine has no CPU fallback"
    return yak_amd


def _keys_of(oracle, o):
    """the hashes (as yak_ch_inc and yak_ch_get take them) of every key of an oracle table"""
    return list(table_counts(oracle.dump_bytes(o)))


def _create_pass(oracle, o, img, opt):
    """a create pass of the oracle over `img` on top of what the table holds (yko_count_mem only counts into an existing table)"""
    O = oracle.lib()
    for a in oracle.extract_lists(opt["k"], 10, img):
        if len(a):
            o.contents.tot += O.yko_ch_insert_list(o, 1, len(a), np.ascontiguousarray(a).ctypes.data_as(C.POINTER(C.c_uint64)))


@contextlib.contextmanager
def _after_pass1(ya, oracle, img, opt, before=None, others=()):
    """the device table (retaining its input) and the oracle's after the first pass over `img` -- on top of a create pass over `before`, if given.
    -> (t, o, feed(buf) -> the feeds of count_pass for a buffer of `img`, `before` or `others`)"""
    L, O = ya.lib(), oracle.lib()
    bufs = [b for b in (img, before) + tuple(others) if b is not None]
    d = [L.yakamd_dev_alloc(len(b) + 64) for b in bufs]
    for p, b in zip(d, bufs):
        assert p and L.yakamd_memcpy_h2d(p, b, len(b)) == 0

    def feed(buf):
        return [(d[[b is buf for b in bufs].index(True)], len(buf), 0)]
    t = ya.Table(opt["k"], 10, 4, opt["bf_shift"])
    o = O.yko_ch_init(opt["k"], 10, 4, opt["bf_shift"])
    try:
        assert L.yakamd_retain_input(t.h, 1) == 0
        for b in (before, img):
            if b is not None:
                t.count_pass(1, feed(b))
                _create_pass(oracle, o, b, opt)
        yield t, o, feed
    finally:
        t.close(); O.yko_ch_destroy(o)
        for p in d:
            L.yakamd_dev_free(p)


def _count(oracle, o, img, opt):
    oc = oracle.copt(opt["k"], 10, 4, opt["bf_shift"])
    assert oracle.lib().yko_count_mem(img, len(img), C.byref(oc), o)


def _same(t, oracle, o):
    assert (t.dump_bytes(), t.tot) == (oracle.dump_bytes(o), o.contents.tot)


@pytest.mark.parametrize("bump", [1, 0], ids=["bump", "clear_then_add"])
@shapes
def test_protocol(shape, bump, ya, oracle, synth, knob, capfd):
    make, opt = SHAPES[shape]
    img = make(synth)
    O = oracle.lib()
    knob("YAKAMD_PASS2_BUMP", bump)
    knob("YAKAMD_VERBOSE", 1)
    with _after_pass1(ya, oracle, img, opt) as (t, o, feed):
        with paths_util.tally(ya.lib()) as ran:
            t.destroy_bf(); t.clear()
            t.count_pass(0, feed(img), same_input=True)
        st = t.stats()
        O.yko_ch_destroy_bf(o); O.yko_ch_clear(o); _count(oracle, o, img, opt)
        t.shrink(2, 1023); O.yko_ch_shrink(o, 2, 1023)
        _same(t, oracle, o)
    assert st["pass2_path"] == FUSED
    assert ran.get("k_img_clear", 0) == 1 and ran.get("k_cnt2_apply", 0) == 1 and ran.get("event:pass2_fused", 0) == 1, ran
    line = [l for l in capfd.readouterr().err.splitlines() if "count pass: the counts of the pass before applied" in l]
    assert len(line) == 1 and ("with the pending clear, in one sweep" in line[0]) == bool(bump), line


def _dump(ya, oracle, t, o, env):
    pass


def _hist(ya, oracle, t, o, env):
    got, want = (C.c_int64 * 1024)(), (C.c_int64 * 1024)()
    ya.lib().yak_ch_hist(t.h, got, 1); oracle.lib().yko_ch_hist(o, want)
    assert list(got) == list(want) and want[0] == o.contents.tot > 0


def _lookup(ya, oracle, t, o, env):
    L, img = ya.lib(), env["img"]
    if env["opt"]["k"] < 32:
        d_out = L.yakamd_dev_alloc(2 * len(img) + 64)
        try:
            assert L.yakamd_lookup_dev(t.h, env["feed"](img)[0][0], len(img), d_out) == 0
            got = np.empty(len(img), np.uint16)
            assert L.yakamd_memcpy_d2h(got.ctypes.data, d_out, 2 * len(img)) == 0
        finally:
            L.yakamd_dev_free(d_out)
        assert (got == oracle.lookup_image(o, img, 2)).all()
    keys = _keys_of(oracle, o)
    for x in keys[::97] + [keys[0] ^ (1 << 40)]:
        assert L.yak_ch_get(t.h, x) == oracle.lib().yko_ch_get(o, x)


def _inc(ya, oracle, t, o, env):
    keys = _keys_of(oracle, o)
    for x in keys[::53] + [keys[5]] * 3 + [keys[0] ^ (1 << 40)]:
        assert ya.lib().yak_ch_inc(t.h, x) == oracle.lib().yko_ch_inc(o, x)


def _other_input(ya, oracle, t, o, env):
    t.count_pass(0, env["feed"](env["other"]))
    _count(oracle, o, env["other"], env["opt"])
    assert t.stats()["pass2_path"] == 0


def _shrink(ya, oracle, t, o, env):
    t.shrink(0, 5); oracle.lib().yko_ch_shrink(o, 0, 5)
    assert o.contents.tot > 0


def _clear_again(ya, oracle, t, o, env):
    t.clear(); oracle.lib().yko_ch_clear(o)


def _shrink_to_nothing(ya, oracle, t, o, env):
    t.shrink(1, 1023); oracle.lib().yko_ch_shrink(o, 1, 1023)
    assert o.contents.tot == 0


LOOKS = {"dump": _dump, "hist": _hist, "lookup": _lookup, "inc_dump": _inc, "pass_over_other_input": _other_input, "shrink": _shrink,
         "second_clear": _clear_again, "shrink_to_nothing": _shrink_to_nothing}


@pytest.mark.parametrize("look", sorted(LOOKS))
@shapes
def test_deferred_clear_is_invisible(shape, look, ya, oracle, synth):
    """whatever comes first behind a clear meets a cleared table; the dump behind it says what that something left"""
    make, opt = SHAPES[shape]
    img, other = make(synth), synth(6000, g=90000, s=21, e=0.02, first=100000)
    with _after_pass1(ya, oracle, img, opt, others=(other,)) as (t, o, feed):
        t.destroy_bf(); t.clear()
        oracle.lib().yko_ch_destroy_bf(o); oracle.lib().yko_ch_clear(o)
        LOOKS[look](ya, oracle, t, o, dict(img=img, other=other, opt=opt, feed=feed))
        _same(t, oracle, o)


def _in_slices(knob, img):
    """the budget of the kept batches (12 bytes per position) holds three batches of the reads (tests/test_gpu_parity.py: pass_in_slices), one of the
    short saturation input: fast_admit counts the batches before as a slice of their own"""
    if len(img) > 1 << 20:
        knob("YAKAMD_FAST_BUDGET", 3000000); knob("YAKAMD_BATCH", 65536)
    else:
        assert len(img) > 2 * 4096
        knob("YAKAMD_FAST_BUDGET", 60000); knob("YAKAMD_BATCH", 4096)


@pytest.mark.parametrize("why", ["pass_in_slices", "inc_before_the_clear", "table_not_empty_before"])
@shapes
def test_retained_set_that_is_not_the_image_takes_the_old_path(shape, why, ya, oracle, synth, knob, capfd):
    make, opt = SHAPES[shape]
    img = make(synth)
    before = synth(3000, g=90000, s=21, first=100000) if why == "table_not_empty_before" else None
    O = oracle.lib()
    knob("YAKAMD_VERBOSE", 1)
    if why == "pass_in_slices":
        _in_slices(knob, img)
    with _after_pass1(ya, oracle, img, opt, before=before) as (t, o, feed):
        if why == "pass_in_slices":
            assert "slice of the pass counted early" in capfd.readouterr().err
        if why == "inc_before_the_clear":
            _inc(ya, oracle, t, o, None)
        t.destroy_bf(); t.clear()
        t.count_pass(0, feed(img), same_input=True)
        O.yko_ch_destroy_bf(o); O.yko_ch_clear(o); _count(oracle, o, img, opt)
        _same(t, oracle, o)
        t.shrink(2, 1023); O.yko_ch_shrink(o, 2, 1023)
        _same(t, oracle, o)
    assert "with the pending clear, in one sweep" not in capfd.readouterr().err


@shapes
def test_count_pass_without_a_clear_adds_to_the_first_pass_counts(shape, ya, oracle, synth, knob, capfd):
    make, opt = SHAPES[shape]
    img = make(synth)
    O = oracle.lib()
    knob("YAKAMD_VERBOSE", 1)
    with _after_pass1(ya, oracle, img, opt) as (t, o, feed):
        t.destroy_bf()
        t.count_pass(0, feed(img), same_input=True)
        assert t.stats()["pass2_path"] == FUSED
        O.yko_ch_destroy_bf(o); _count(oracle, o, img, opt)
        _same(t, oracle, o)
        t.shrink(2, 1023); O.yko_ch_shrink(o, 2, 1023)
        _same(t, oracle, o)
    assert "with the pending clear, in one sweep" not in capfd.readouterr().err
