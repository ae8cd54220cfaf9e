"""Homopolymer compression without a device: the two restatements of tests/hpc_util.py against each other, yakamd_hpc_host against them byte for
byte, a case derived by hand, and the oracle's count of a compressed image against the reference's own count of the host-compressed FASTA."""
import ctypes as C
import numpy as np
import pytest

import hpc_util as H

PLANTED = H.PLANTED
plant_runs = H.plant_runs


def host(img):
    import yak_amd
    L = yak_amd.lib()
    out = C.create_string_buffer((len(img) + 15) // 16 * 16 + 16)
    C.memset(out, 0x5a, len(out))
    n = L.yakamd_hpc_host(img, len(img), out)
    assert n >= 0
    assert out.raw[(n + 15) // 16 * 16:] == b"\x5a" * (len(out) - (n + 15) // 16 * 16)      # nothing behind the fill
    return out.raw[:(n + 15) // 16 * 16], n


def test_hand_derived_case():
    """AAACCCGTTNNAAT: the runs AAA CCC G TT collapse, each N stays and cuts, AA T follow -> ACGT N N AT; its 3-mers are those of ACGT alone"""
    img = b"AAACCCGTTNNAAT\n"
    want = b"ACGT\n\nAT\n"
    assert H.compress(img) == want
    assert H.compress_seq(b"AAACCCGTTNNAAT") == b"ACGTNNAT"
    kmers = [w[i:i + 3] for w in want.split(b"\n") for i in range(len(w) - 2)]
    assert kmers == [b"ACG", b"CGT"]
    got, n = host(img)
    assert n == len(want) and got == H.padded(want)


@pytest.mark.parametrize("i", range(len(PLANTED)))
def test_restatements_and_host_agree_on_planted_inputs(i):
    img = PLANTED[i]
    want = H.compress(img)
    if img.endswith(b"\n"):
        assert H.as_image(H.compress_records(img)) == want
    got, n = host(img)
    assert n == len(want) and got == H.padded(want)
    assert all(a != b or a == 10 for a, b in zip(want, want[1:]))      # no base twice in a row


@pytest.mark.parametrize("n,seed", [(1, 1), (15, 2), (16, 3), (17, 4), (4095, 5), (4096, 6), (4097, 7), (200003, 8)])
def test_restatements_and_host_agree_on_random_images(n, seed):
    img = H.random_image(n, seed)[:-1] + b"\n"
    want = H.compress(img)
    assert H.as_image(H.compress_records(img)) == want
    got, m = host(img)
    assert m == len(want) and got == H.padded(want)
    assert len(want) < 0.75 * n or n < 100
    kept, prev = [], 4                                                 # the definition once more, position by position
    for b in img:
        c = int(H.NT4[b])
        kept.append(not (c < 4 and c == prev))
        prev = c
    off = np.array([0, n // 3, n - 1, n, n // 2], np.int64)
    ln = np.array([n // 3, n // 2, 1, 0, n], np.int64)
    oo, lo = H.remap(img, off, ln)
    for o, l, a, b in zip(off, ln, oo, lo):
        assert a == sum(kept[:o]) and b == sum(kept[o:o + l])


def test_pack_restatement_round_trips():
    img = H.random_image(1000, 11)
    codes, valid = H.pack(img)
    code = H.NT4[np.frombuffer(img, np.uint8)]
    for j in (0, 1, 15, 16, 31, 32, 999):
        assert (valid[j // 32] >> (j % 32)) & 1 == (code[j] < 4)
        if code[j] < 4:
            assert (codes[j // 16] >> (2 * (j % 16))) & 3 == code[j]


def test_oracle_on_the_compressed_image_equals_the_reference_on_the_compressed_fasta(oracle, synth, tmp_path):
    """what the GPU tests compare the device with: oracle.count_protocol_mem of the compressed image.  Where the reference itself is built, its CLI's
    count of the host-compressed FASTA gives the same bytes"""
    if not oracle.have_ref():
        pytest.skip("reference binary not built")
    img = plant_runs(synth(3000, g=20000, s=5), 3)
    fa = tmp_path / "c.fa"
    with open(fa, "wb") as f:
        for i, r in enumerate(img.split(b"\n")[:-1]):
            f.write(b">r%d\n%s\n" % (i, H.compress_seq(r)))
    for args, kw in ((["-k31", "-b0"], dict(k=31)), (["-k21", "-b24"], dict(k=21, bf_shift=24))):
        out = str(tmp_path / "ref.yak")
        oracle.ref_count_cli(args + ["-t1", "-o", out, str(fa)])
        want = open(out, "rb").read()
        got, _ = oracle.count_protocol_mem(H.compress(img), **kw)
        assert got == want
