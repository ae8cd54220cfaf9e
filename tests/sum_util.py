"""What yakamd_ch_sum must leave in a table, restated with numpy on .yak images (tests/test_sum.py checks the restatement against the oracle
alone; tests/test_gpu_sum.py checks the device against it).

A .yak image is a 16-byte header {"YAK\\2", k, pre, counter bits}, then per sub-table {u32 capacity, u32 size} and `size` 8-byte keys in slot
order, a key = (hash >> pre) << 10 | count.  A k-mer is named by (sub-table, key >> 10)."""
import struct

import numpy as np


def parse(img):
    """(k, pre, sub, keys, heads): per key its sub-table index and its 8-byte word, in image order; heads[p] = byte offset of sub-table p's
    {capacity, size} word"""
    assert img[:4] == b"YAK\x02" and len(img) >= 16, "not a .yak image"
    k, pre, cbits = struct.unpack("<3I", img[4:16])
    assert cbits == 10
    P = 1 << pre
    heads, sizes, parts = np.empty(P, np.int64), np.empty(P, np.int64), []
    off = 16
    for p in range(P):
        heads[p] = off
        _, size = struct.unpack_from("<2I", img, off)
        off += 8
        parts.append(np.frombuffer(img, np.uint64, size, off))
        sizes[p] = size
        off += 8 * size
    assert off == len(img), "bytes behind the last sub-table"
    keys = np.concatenate(parts) if parts else np.empty(0, np.uint64)
    return k, pre, np.repeat(np.arange(P, dtype=np.int64), sizes), keys, heads


def counts(img):
    """{(sub-table, key >> 10): count} of a .yak image"""
    _, _, sub, keys, _ = parse(img)
    kid, c = keys >> np.uint64(10), keys & np.uint64(1023)
    d = dict(zip(zip(sub.tolist(), kid.tolist()), c.tolist()))
    assert len(d) == len(keys), "a k-mer is stored twice"
    return d


def _labels(subs, kids):
    """one integer per distinct (sub-table, key >> 10) over several tables: the tables' label arrays and the number of labels"""
    sub, kid = np.concatenate(subs), np.concatenate(kids)
    order = np.lexsort((kid, sub))
    s, q = sub[order], kid[order]
    new = np.ones(len(s), bool)
    new[1:] = (s[1:] != s[:-1]) | (q[1:] != q[:-1])
    lab = np.empty(len(s), np.int64)
    lab[order] = np.cumsum(new) - 1
    cuts = np.cumsum([len(x) for x in subs])[:-1]
    return np.split(lab, cuts), int(new.sum())


def expected_sum_bytes(merged, a, b):
    """the image yakamd_ch_sum(a, b) must dump: `merged` -- what yko_ch_merge(a, copy of b, 1, 1023, pre_resize) dumps -- with every header,
    capacity, size and key position kept and each key's low 10 bits replaced by min(1023, its count in a + its count in b), 0 where absent"""
    km, pm, sub_m, keys_m, heads = parse(merged)
    tabs = [parse(x) for x in (a, b)]
    assert all((t[0], t[1]) == (km, pm) for t in tabs), "different k or pre"
    (lm, la, lb), n = _labels([sub_m, tabs[0][2], tabs[1][2]], [keys_m >> np.uint64(10), tabs[0][3] >> np.uint64(10), tabs[1][3] >> np.uint64(10)])
    tot = np.zeros(n, np.int64)
    for lab, t in ((la, tabs[0]), (lb, tabs[1])):
        assert len(np.unique(lab)) == len(lab), "a k-mer is stored twice"
        tot[lab] += (t[3] & np.uint64(1023)).astype(np.int64)
    new = (keys_m & ~np.uint64(1023)) | np.minimum(tot[lm], 1023).astype(np.uint64)
    out = bytearray(merged)
    at = 0
    for h in heads.tolist():
        size = struct.unpack_from("<I", merged, h + 4)[0]
        out[h + 8:h + 8 + 8 * size] = new[at:at + size].tobytes()
        at += size
    return bytes(out)


def tandem(unit, copies, flank=b""):
    """one record: `unit` repeated `copies` times -- every k-mer of the repeat (k <= len(unit) apart from self-overlaps) occurs about `copies` times"""
    return flank + unit * copies + flank + b"\n"


U1 = b"ACGGTCATTAGCCTGAATCGTTAGGCATCCGATTACA"          # 37 bases
U2 = b"TTGACCGTAAGCTAGGCTTACGATCAGTCCATGGA"            # 35 bases
U3 = b"GATTCACGTTGCAAGCTTGGACTCATGCAATCGGTAC"          # 37 bases


def operand_images(synth):
    """the two inputs of the sum tests, of unequal size, as base images (every record followed by a newline, so A + B is `A ++ B` with a record
    break between them): reads of one genome, so that most k-mers are in both with different counts, plus tandem repeats whose k-mers
    (a) pass 1023 only in the sum -- about 700 copies in each --, (b) are at 1023 in A already and present in B, (c) are at 1023 in B alone"""
    a = synth(3000, g=20000, s=11) + tandem(U1, 700) + tandem(U2, 1500)
    b = synth(1200, g=20000, s=11, first=3000) + tandem(U1, 700) + tandem(U2, 5) + tandem(U3, 1300)
    return a, b
