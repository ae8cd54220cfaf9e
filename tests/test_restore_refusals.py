"""What yak_ch_restore refuses before it touches a device -- a body that ends early, a wrong magic, wrong counter bits, a sub-table header that no
table writes -- and yakamd_yak_header, the header alone (yak_amd/csrc/yak_file.cpp over yak_file.h).  None of it makes a device call, so all of it
runs without a GPU."""
import ctypes as C
import glob
import os
import struct

import pytest

from conftest import ROOT

GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.yak")))


def _image():
    """a golden table, and the index and offset of its first sub-table with two keys or more"""
    img = open(os.path.join(ROOT, "tests", "golden", "nb_k31.yak"), "rb").read()
    pre = struct.unpack_from("<I", img, 8)[0]
    off = 16
    for p in range(1 << pre):
        size = struct.unpack_from("<I", img, off + 4)[0]
        if size >= 2:
            return img, p, off
        off += 8 + 8 * size
    raise AssertionError("no sub-table with two keys")


def _refused(tmp_path, capfd, name, data):
    import yak_amd
    fn = tmp_path / name
    fn.write_bytes(data)
    capfd.readouterr()
    assert not yak_amd.lib().yak_ch_restore(str(fn).encode())
    err = capfd.readouterr().err
    assert "gfx950" not in err and "[E::" not in err, err        # refused by the file alone, before any table was asked for
    return err, str(fn)


def test_restore_refuses_a_body_that_ends_early(tmp_path, capfd):
    img, p, off = _image()
    err, fn = _refused(tmp_path, capfd, "keys.yak", img[:off + 8 + 8 + 3])       # inside the second key of sub-table p
    assert "ERROR: '%s' is truncated at sub-table %d\n" % (fn, p) in err
    err, fn = _refused(tmp_path, capfd, "key_end.yak", img[:off + 8 + 8])        # between two keys
    assert "ERROR: '%s' is truncated at sub-table %d\n" % (fn, p) in err
    err, fn = _refused(tmp_path, capfd, "head.yak", img[:off + 4])               # inside its header
    assert "ERROR: '%s' is truncated at sub-table %d\n" % (fn, p) in err
    err, fn = _refused(tmp_path, capfd, "last.yak", img[:-1])                    # the last byte of the file
    assert "is truncated at sub-table" in err


def test_restore_refuses_bad_headers(tmp_path, capfd):
    img, p, off = _image()
    err, _ = _refused(tmp_path, capfd, "magic.yak", b"YAK\x01" + img[4:])
    assert "ERROR: wrong file magic.\n" in err
    err, _ = _refused(tmp_path, capfd, "bits.yak", img[:12] + struct.pack("<I", 8) + img[16:])
    assert "ERROR: saved counter bits: 8; compile-time counter bits: 10\n" in err
    size = struct.unpack_from("<I", img, off + 4)[0]
    err, fn = _refused(tmp_path, capfd, "cap.yak", img[:off] + struct.pack("<I", 3) + img[off + 4:])
    assert "ERROR: corrupt sub-table header in '%s' (capacity 3, size %d)\n" % (fn, size) in err


def test_yak_header_of_every_golden_table_and_its_refusals(tmp_path):
    import yak_amd
    L = yak_amd.lib()
    assert len(GOLDEN) >= 10
    for fn in GOLDEN:
        want = struct.unpack("<2I", open(fn, "rb").read(16)[4:12])
        k, pre = C.c_int(-1), C.c_int(-1)
        assert L.yakamd_yak_header(fn.encode(), C.byref(k), C.byref(pre)) == 0
        assert (k.value, pre.value) == want
        assert yak_amd.yak_header(fn) == want
    head = open(GOLDEN[0], "rb").read(16)
    short, magic, missing = tmp_path / "short.yak", tmp_path / "magic.yak", tmp_path / "none.yak"
    short.write_bytes(head[:15])
    magic.write_bytes(b"YAK\x01" + head[4:])
    for fn, what in ((missing, "cannot open"), (short, "truncated header"), (magic, "wrong file magic")):
        k, pre = C.c_int(-1), C.c_int(-1)
        assert L.yakamd_yak_header(str(fn).encode(), C.byref(k), C.byref(pre)) == -1
        assert what in L.yakamd_last_error().decode() and str(fn) in L.yakamd_last_error().decode()
        assert (k.value, pre.value) == (-1, -1)
    for fn in (short, magic):
        with pytest.raises(ValueError):
            yak_amd.yak_header(str(fn))
    with pytest.raises(OSError):                                   # as open() raised it before
        yak_amd.yak_header(str(missing))
