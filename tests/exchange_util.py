"""What the extraction, packing and exchange exports must write, element by element, worked out with numpy from the oracle's flat extraction
(yko_extract_pos: every k-mer of an image with the index of its last base, in stream order) and its base table yko_nt4 -- and the images the
tests of those exports share.  The formats are the ones include/yak_amd.h states:

  * yakamd_extract_dev: (hash, position) of the k-mers whose prefix hash & (2^pre - 1) lies in a range, in no particular order;
  * yakamd_partition_dev / _hashes_dev: the same records (or the bare hashes) grouped by prefix, 2^pre + 1 group offsets, free order inside a group;
  * yakamd_partition_tagged_dev: (hash >> pre) << 12 | toggle << 10 | position & 1023; inside a group the records of one 1024-position round
    are contiguous, the rounds follow each other in stream order, the toggle flips between consecutive rounds that contributed to the group;
  * yakamd_pack_bases_dev / _host: 2-bit codes, 16 positions per 32-bit word, and one validity bit per position, zero behind the last one.
"""
import numpy as np

ROUND = 1024                       # stream positions per round of the tagged format
WG = 65536                         # stream positions per workgroup of the partition kernels
TAG_BITS, TOGGLE_BIT = 12, 10


# ---------------------------------------------------------------------------------------------- expected outputs
def flat(oracle, img, k):
    """(hashes, positions) of the image's k-mers in stream order, from the oracle"""
    return oracle.extract_pos(k, img)


def expect_groups(oracle, img, k, pre):
    """-> (hash, pos, bstart): the records sorted by (prefix, position, hash) and the 2^pre + 1 offsets of the prefix groups"""
    h, t = flat(oracle, img, k)
    P = 1 << pre
    p = (h & np.uint64(P - 1)).astype(np.int64)
    order = np.lexsort((h, t, p))
    bstart = np.zeros(P + 1, np.uint64)
    bstart[1:] = np.cumsum(np.bincount(p, minlength=P))
    return h[order], t[order], bstart


def group_ids(bstart):
    """the prefix of every record of a partition, from its offsets"""
    b = np.asarray(bstart, np.int64)
    return np.repeat(np.arange(len(b) - 1, dtype=np.int64), np.diff(b))


def sort_groups(bstart, h, t=None):
    """a partition's records sorted inside every prefix group by (position, hash) -- by hash alone without positions"""
    g = group_ids(bstart)
    order = np.lexsort((h, g)) if t is None else np.lexsort((h, t, g))
    return (h[order],) if t is None else (h[order], t[order])


class Runs:
    """the records of a tagged partition as runs: run i belongs to prefix[i], holds payload[start[i]:start[i + 1]] -- (hash >> pre) << 10 | position
    in the round, sorted, so a run is its set of records -- and carries key[i]: the round (expected) or the toggle (decoded)"""

    def __init__(self, prefix, key, start, payload):
        self.prefix, self.key, self.start, self.payload = prefix, key, start, payload

    def of(self, p):
        """prefix p's runs in order: [(key, frozenset of (hash >> pre, position in the round))]"""
        out = []
        for i in np.flatnonzero(self.prefix == p):
            x = self.payload[self.start[i]:self.start[i + 1]]
            out.append((int(self.key[i]), frozenset(zip((x >> np.uint64(10)).tolist(), (x & np.uint64(1023)).tolist()))))
        return out

    def same_runs(self, other):
        """run for run: the same prefixes in the same order, the same records in each (the keys are of different kinds and not compared)"""
        return (np.array_equal(self.prefix, other.prefix) and np.array_equal(self.start, other.start)
                and np.array_equal(self.payload, other.payload))


def _runs(run_id, prefix_of_rec, key_of_rec, payload):
    """records -> Runs; run_id is non-decreasing along the records"""
    n = len(payload)
    first = np.flatnonzero(np.r_[True, run_id[1:] != run_id[:-1]]) if n else np.empty(0, np.int64)
    order = np.lexsort((payload, run_id))
    return Runs(prefix_of_rec[first], key_of_rec[first], np.r_[first, n].astype(np.int64), payload[order])


def expect_tagged(oracle, img, k, pre):
    """-> (Runs, bstart): per prefix the contributing rounds R = pos >> 10 in ascending order, each with its set of (hash >> pre, pos & 1023)"""
    h, t = flat(oracle, img, k)
    P = 1 << pre
    p = (h & np.uint64(P - 1)).astype(np.int64)
    R = (t >> np.uint32(10)).astype(np.int64)
    order = np.lexsort((R, p))                                   # stable: stream order inside a round
    p, R = p[order], R[order]
    payload = (h[order] >> np.uint64(pre)) << np.uint64(10) | (t[order] & np.uint32(ROUND - 1)).astype(np.uint64)
    bstart = np.zeros(P + 1, np.uint64)
    bstart[1:] = np.cumsum(np.bincount(p, minlength=P))
    return _runs(p * (int(R.max()) + 1 if len(R) else 1) + R, p, R, payload), bstart


def decode_tagged(rec8, bstart):
    """a tagged partition as it came from the device -> Runs: every prefix group cut into maximal runs of equal toggle (bit 10), key = the toggle"""
    rec8 = np.asarray(rec8, np.uint64)
    g = group_ids(bstart)
    assert len(g) == len(rec8), "the offsets do not cover the records"
    tg = (rec8 >> np.uint64(TOGGLE_BIT) & np.uint64(1)).astype(np.int64)
    new = np.r_[True, (g[1:] != g[:-1]) | (tg[1:] != tg[:-1])] if len(g) else np.empty(0, bool)
    payload = (rec8 >> np.uint64(TAG_BITS)) << np.uint64(10) | (rec8 & np.uint64(ROUND - 1))
    return _runs(np.cumsum(new) - 1, g, tg, payload)


def toggles_alternate(runs):
    """consecutive runs of one prefix carry different toggles (by construction of decode_tagged; stated on its own for the reader of a failure)"""
    same_prefix = runs.prefix[1:] == runs.prefix[:-1]
    return bool(np.all(runs.key[1:][same_prefix] != runs.key[:-1][same_prefix]))


def max_per_round(runs):
    """the largest number of records one prefix has in one round"""
    return int(np.diff(runs.start).max()) if len(runs.prefix) else 0


def crosses_workgroups(runs):
    """some prefix has two consecutive contributing rounds in different workgroups (runs = expect_tagged's: key = round)"""
    same_prefix = runs.prefix[1:] == runs.prefix[:-1]
    wg = runs.key // (WG // ROUND)
    return bool(np.any(same_prefix & (wg[1:] != wg[:-1])))


def expect_packed(oracle, img):
    """-> (code words, validity words) of the whole image, numpy uint32: position j at bits 2 (j % 16) of code word j / 16 and at bit j % 32 of
    validity word j / 32; (n + 31) / 32 validity words and twice as many code words, zero for every position that holds no base and behind n"""
    n = len(img)
    nw = (n + 31) // 32
    c = np.full(32 * nw, 4, np.uint8)
    c[:n] = oracle.nt4()[np.frombuffer(bytes(img), np.uint8)]
    ok = c < 4
    code = np.where(ok, c, 0).astype(np.uint32).reshape(2 * nw, 16)
    codes = (code << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)      # disjoint bit fields: the sum is the OR
    valid = (ok.astype(np.uint32).reshape(nw, 32) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
    return codes, valid


def split_packed(pk, n):
    """the bytes yakamd_pack_bases_host wrote for n positions -> (code words, validity words)"""
    nw = (n + 31) // 32
    cb = (8 * nw + 15) & ~15
    assert len(pk) == cb + 4 * nw
    return np.frombuffer(pk[:8 * nw], np.uint32), np.frombuffer(pk[cb:cb + 4 * nw], np.uint32)


# ---------------------------------------------------------------------------------------------- the images
def _acgt(rnd, n):
    return bytes(rnd.choice(b"ACGT") for _ in range(n))


SPECIAL_AT = {4096: bytes([ord("u"), ord("\r"), 2, 0xff]), 65536: bytes([1, ord(">"), ord("U"), ord("y")])}   # at T - 2 .. T + 1


def all_bytes_image():
    """every byte value 0..255 between ACGT runs of 64..80 bases -- the raw codes 0..3, U / u, lower case, IUPAC letters, '>', CR, 0xff among them --
    over more than one workgroup, with rare bases and non-bases on both sides of positions 4096 and 65536; its length is no multiple of 16"""
    import random
    rnd = random.Random(20240607)
    out = bytearray()
    while len(out) < WG + 3000:
        vals = list(range(256))
        rnd.shuffle(vals)
        for v in vals:
            out += _acgt(rnd, rnd.randrange(64, 81))
            out.append(v)
    out += _acgt(rnd, 70)
    for T, s in SPECIAL_AT.items():
        out[T - 2:T + 2] = s
    while len(out) % 16 != 5:
        out.append(rnd.choice(b"ACGT"))
    return bytes(out)


def isolated_values(img):
    """the byte values that occur somewhere in img with 64 bases A / C / G / T directly before and directly behind them"""
    a = np.frombuffer(img, np.uint8)
    base = np.isin(a, np.frombuffer(b"ACGT", np.uint8)).astype(np.int64)
    cs = np.r_[0, np.cumsum(base)]
    i = np.arange(64, len(a) - 64)
    ok = (cs[i] - cs[i - 64] == 64) & (cs[i + 65] - cs[i + 1] == 64)
    return set(np.unique(a[i[ok]]).tolist())


RANDOM_READ_LEN = 175              # 176 positions per read: reads 372 and 744 lie across positions 65536 and 131072


def random_3wg_image(synth):
    """about 140 000 positions of synthetic reads -- three workgroups of the partition kernels, the last one partial; the length is no multiple of 16"""
    img = synth(800, l=RANDOM_READ_LEN, g=30000, s=4242, N=0.002)
    return img[:140003]


def low_complexity_image(synth):
    """runs that put thousands of records of one prefix into one 1024-position round -- poly-A, ACGT and AATT repeated, a 2-periodic run -- each
    between random reads that share its first and last round, so other prefixes sit beside them"""
    reads = synth(120, l=150, g=6000, s=777)
    rd = [reads[i * 151:(i + 1) * 151] for i in range(120)]
    parts = [b"".join(rd[0:20]), b"A" * 3000 + b"\n", b"".join(rd[20:30]), b"ACGT" * 800 + b"\n", b"".join(rd[30:40]),
             b"AATT" * 800 + b"\n", b"".join(rd[40:55]), b"AC" * 1500 + b"\n", b"".join(rd[55:120])]
    return b"".join(parts)


EDGE_K = (1, 31, 32, 63)


def edge_lengths(k):
    """the lengths at which a prefix of random_3wg ends: nothing, one position, one k-mer short of / exactly one k-mer, around the 16 positions of a
    bulk load, around a tile of 4096, the last k-mer that starts in the first tile's halo, around a workgroup of 65536"""
    return sorted({0, 1, k - 1, k, 15, 16, 17, 4095, 4096, 4097, 4096 + k - 2, 65535, 65536, 65537})
