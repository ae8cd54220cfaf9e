"""Clustered, adversarial count inputs and an independent put-by-put model of khashl to say what they are.

Every other count and layout input of the suite is uniform after yak_hash64 in the three places where the kernels' hard cases live: the khashl home
slot h2b((u32)(hash >> pre), bits), the bloom block (low bits of hash >> pre) and the level-2 sub-bucket.  yak_hash64 is invertible
(tablecmds_util.hash64_inv) and so is khashl's Fibonacci multiply (2654435769 is odd), so chosen values of x = hash >> pre are turned back into
one-k-mer records here.  Three parts:

  builders   canonical k-mers for chosen x: keys of one home slot, of consecutive home slots, of one bloom block; the record writer
  the model  Kh, the literal put / resize of khashl.h:152-221 (the third restatement, beside oracle/yko_core.c and the reference), and Model, the same
             with reports: per doubling the runs of used old slots, whether the last run wraps, whether one run covers [F, 2F], the longest walk of
             a put; and predictions of what the streaming replay's thresholds (kern_replay2.inc) make of them
  CASES      name -> case(k): the image, its put sequence and the properties it claims; tests/test_adversarial.py asserts every claim from the model
             and from the oracle's dump, tests/test_gpu_adversarial.py counts the images on the device
"""
import random
import struct

import numpy as np

M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
FIB = 2654435769
FIB_INV = pow(FIB, -1, 1 << 32)
PRE = 10
SUB = 37                                        # the sub-table of the single-table cases (any would do)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------------------------
def hash64_inv_np(x, m):
    """tablecmds_util.hash64_inv (reference yak-priv.h:41-68) on a numpy uint64 array"""
    u = np.uint64
    x = np.asarray(x, dtype=np.uint64)
    m = u(m)
    t = x - (x << u(31)); x = (x - (t << u(31))) & m
    t = x ^ x >> u(28); x = x ^ t >> u(28)
    x = (x * u(14933078535860113213)) & m
    t = x ^ x >> u(14); t = x ^ t >> u(14); t = x ^ t >> u(14); x = x ^ t >> u(14)
    x = (x * u(15244667743933553977)) & m
    t = x ^ x >> u(24); x = x ^ t >> u(24)
    t = ~x; t = ~(x - (t << u(21))); t = ~(x - (t << u(21))); x = ~(x - (t << u(21))) & m
    return x


def revcomp(xs, k):
    """reverse complement of 2-bit packed k-mers (numpy uint64)"""
    xs = np.asarray(xs, dtype=np.uint64)
    rc = np.zeros_like(xs)
    for j in range(k):
        rc |= (np.uint64(3) - (xs >> np.uint64(2 * j) & np.uint64(3))) << np.uint64(2 * (k - 1 - j))
    return rc


def records(xs, k):
    """one record per 2-bit packed k-mer: its k letters and '\\n', a (len, k + 1) uint8 array"""
    xs = np.asarray(xs, dtype=np.uint64)
    seq = np.empty((len(xs), k + 1), dtype=np.uint8)
    for j in range(k):
        seq[:, j] = np.frombuffer(b"ACGT", dtype=np.uint8)[(xs >> np.uint64(2 * (k - 1 - j)) & np.uint64(3)).astype(np.int64)]
    seq[:, k] = ord("\n")
    return seq


def canonical_kmers(hashes, k, n=None):
    """the k-mers of the given hashes that are their own canonical form (the others would be counted as their reverse complement, somewhere
    else), in the order given; n: exactly the first n of them"""
    xs = hash64_inv_np(np.asarray(hashes, dtype=np.uint64), (1 << 2 * k) - 1)
    xs = xs[xs < revcomp(xs, k)]
    if n is not None:
        assert len(xs) >= n, (len(xs), n)
        xs = xs[:n]
    return xs


def is_canonical(xs, sub, k, pre=PRE):
    """per x = hash >> pre: is the k-mer of hash x << pre | sub its own canonical form?"""
    h = np.asarray(xs, dtype=np.uint64) << np.uint64(pre) | np.uint64(sub)
    z = hash64_inv_np(h, (1 << 2 * k) - 1)
    return z < revcomp(z, k)


def image(xs, sub, k, pre=PRE):
    """the image of the put sequence xs (values of hash >> pre, repeats and all) into sub-table `sub`: one canonical k-mer per record"""
    if len(xs) == 0:
        return b""
    h = np.asarray(xs, dtype=np.uint64) << np.uint64(pre) | np.uint64(sub)
    z = hash64_inv_np(h, (1 << 2 * k) - 1)
    assert bool(np.all(z < revcomp(z, k)))
    return records(z, k).tobytes()


def h2b(h, bits):
    """khashl's __kh_h2b"""
    return ((h * FIB) & M32) >> (32 - bits)


def lo_for(slot, bits, r=0):
    """the low 32 bits of hash >> pre whose home slot is `slot` at 2^bits slots (and slot >> d at 2^(bits - d)); r < 2^(32 - bits) picks among them"""
    assert 0 <= slot < 1 << bits and 0 <= r < 1 << (32 - bits)
    return (((slot << (32 - bits)) | r) * FIB_INV) & M32


def hi_bits(k, pre=PRE):
    """bits of hash >> pre above the 32 that khashl hashes: 20 at k = 31, none at k = 21 (2k - pre = 32: nothing hides above the slot hash)"""
    return max(0, 2 * k - pre - 32)


class Picker:
    """hands out distinct x = hash >> pre whose k-mers are canonical.  A candidate that is not is dropped and the next free high bits are taken
    instead (k = 31: 20 of them); where there are none (k = 21) the next free r below the slot bits"""
    def __init__(self, sub, k, pre=PRE, seed=1):
        self.sub, self.k, self.pre, self.hb = sub, k, pre, hi_bits(k, pre)
        self.rnd = random.Random(seed)
        self.taken = set()

    def _first_ok(self, cands):
        ok = is_canonical(cands, self.sub, self.k, self.pre)
        out = []
        for x, o in zip(cands, ok):
            if o and x not in self.taken:
                out.append(x)
        return out

    def same_home(self, slot, bits, n):
        """n keys whose home slot is `slot` at 2^bits slots and slot >> d at every smaller capacity.  With high bits (k = 31) they share ALL 32
        hashed bits: one home slot at every capacity whatsoever"""
        out, nxt = [], 0
        while len(out) < n:
            m = 2 * (n - len(out)) + 16
            if self.hb:
                assert nxt + m <= 1 << self.hb
                cands = [(hi << 32) | lo_for(slot, bits) for hi in range(nxt, nxt + m)]
            else:
                assert nxt + m <= 1 << (32 - bits)
                cands = [lo_for(slot, bits, r) for r in range(nxt, nxt + m)]
            nxt += m
            for x in self._first_ok(cands):
                if len(out) < n:
                    out.append(x); self.taken.add(x)
        return out

    def one_per_slot(self, slots, bits):
        """one key for each of `slots` (repeats allowed: several keys of that home), random below and above the slot bits"""
        out = []
        todo = list(slots)
        while todo:
            cands = [(self.rnd.getrandbits(self.hb) << 32 if self.hb else 0) | lo_for(s, bits, self.rnd.getrandbits(32 - bits)) for s in todo]
            ok = is_canonical(cands, self.sub, self.k, self.pre)
            nxt = []
            for s, x, o in zip(todo, cands, ok):
                if o and x not in self.taken:
                    out.append((s, x)); self.taken.add(x)
                else:
                    nxt.append(s)
            todo = nxt
        order = {}
        for s, x in out:
            order.setdefault(s, []).append(x)
        return [order[s].pop() for s in slots]

    def same_block(self, low_bits, width, n):
        """n keys that agree in the low `width` bits of hash >> pre (one bloom block for every filter of up to 2^(width + 9) bits per sub-table);
        everything above is random, so the home slots are uniform while width leaves hashed bits free"""
        out, top = [], 2 * self.k - self.pre - width
        assert top > 0
        if top <= 12:                                               # few bits left: every candidate, and as many keys as there are (up to n)
            out = self._first_ok([t << width | low_bits for t in range(1 << top)])[:n]
            self.taken.update(out)
            return out
        assert n <= 1 << (top - 1)
        while len(out) < n:
            cands = [self.rnd.getrandbits(top) << width | low_bits for _ in range(2 * (n - len(out)) + 16)]
            for x in self._first_ok(cands):
                if len(out) < n:
                    out.append(x); self.taken.add(x)
        return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Kh:
    """khashl set (khashl.h:152-221), literally: keys are x = hash >> pre, hashed by their low 32 bits (yak_ch_hash = key >> 10 as khint_t)"""
    def __init__(self):
        self.bits, self.count, self.used, self.keys = 0, 0, None, None

    def n_buckets(self):
        return (1 << self.bits) if self.keys is not None else 0

    def resize(self, new_n):
        j, x = 0, new_n
        while x > 1:
            x >>= 1; j += 1
        if new_n & (new_n - 1):
            j += 1
        nb = max(j, 2)
        new_n = 1 << nb
        if self.count > (new_n >> 1) + (new_n >> 2):
            return
        new_used = [False] * new_n
        n = self.n_buckets()
        if self.keys is None:
            self.keys, self.used = [None] * new_n, [False] * 0
        if n < new_n:
            self.keys = self.keys + [None] * (new_n - n)
        mask = new_n - 1
        for j in range(n):
            if not self.used[j]:
                continue
            key = self.keys[j]
            self.used[j] = False
            while True:
                i = h2b(key & M32, nb)
                while new_used[i]:
                    i = (i + 1) & mask
                new_used[i] = True
                if i < n and self.used[i]:
                    self.keys[i], key = key, self.keys[i]
                    self.used[i] = False
                else:
                    self.keys[i] = key
                    break
        self.used, self.bits = new_used, nb

    def put(self, key):
        n = self.n_buckets()
        if self.count >= (n >> 1) + (n >> 2):
            self.resize(n + 1)
            n = self.n_buckets()
        mask = n - 1
        i = last = h2b(key & M32, self.bits)
        while self.used[i] and self.keys[i] != key:
            i = (i + 1) & mask
            if i == last:
                break
        if not self.used[i]:
            self.keys[i], self.used[i] = key, True
            self.count += 1

    def layout(self):
        return [self.keys[i] if self.used[i] else None for i in range(self.n_buckets())]


class _NextFree:
    """first unused slot at or behind i, cyclically (a table is never full): union-find with path halving"""
    def __init__(self, n):
        self.n, self.nx = n, list(range(n))

    def find(self, i):
        nx = self.nx
        while nx[i] != i:
            nx[i] = nx[nx[i]]
            i = nx[i]
        return i

    def take(self, i):
        self.nx[i] = (i + 1) % self.n


def runs_of(used):
    """[(start, length)] of the maximal runs of used slots of a table, not joined around its end"""
    out, n, i = [], len(used), 0
    while i < n:
        if not used[i]:
            i += 1
            continue
        j = i
        while j < n and used[j]:
            j += 1
        out.append((i, j - i))
        i = j
    return out


class Model(Kh):
    """Kh with the probe sequences shortened (the first free slot by union-find, an existing key by a dictionary: the same slots, checked against Kh by
    tests/test_adversarial.py) and reports.  doublings: one dict per doubling of a table that holds keys --
      n        old capacity                         runs   [(start, length)] of the used old slots
      wraps    the run that reaches slot n - 1 goes on at slot 0          tail, head   its lengths before the end and from slot 0 on (0: none)
      cover    every power of two F >= 8 such that no slot of [F, 2F) is unused: one run covers [F, 2F]
      first    the used slots from slot 0 on (k_r2_dsmall's literal prefix is max(8, first + 1) slots)
      walk     the longest walk (slots past the home slot) of a put at the old capacity
      tail_far the last new slot, counted from slot 0, that a key of the old table's last run takes behind the new table's end (-1: none goes around)
    stages: per capacity the new keys put there as [(home, walk, x)] in put order, and `before`, the used slots when the first of them came"""
    def __init__(self):
        Kh.__init__(self)
        self.doublings, self.stages = [], {}
        self.pos, self.nf, self.walk = {}, None, 0

    def resize(self, new_n):
        n = self.n_buckets()
        assert new_n == n + 1
        nb = max(self.bits + 1, 2) if n else 2
        new_n = 1 << nb
        if n:
            runs = runs_of(self.used)
            tail = runs[-1][1] if runs and runs[-1][0] + runs[-1][1] == n else 0
            first = runs[0][1] if runs and runs[0][0] == 0 else 0
            cover, F = [], 8
            while 2 * F <= n:
                if all(self.used[F:2 * F]):
                    cover.append(F)
                F *= 2
            tail_keys = [self.keys[i] for i in range(n - tail, n)]
            self.doublings.append(dict(n=n, count=self.count, runs=runs, wraps=bool(tail and first), tail=tail, head=first if tail else 0, first=first, cover=cover, walk=self.walk))
        new_used, nf = [False] * new_n, _NextFree(new_n)
        if self.keys is None:
            self.keys, self.used = [None] * new_n, []
        if n < new_n:
            self.keys = self.keys + [None] * (new_n - n)
        for j in range(n):
            if not self.used[j]:
                continue
            key = self.keys[j]
            self.used[j] = False
            while True:
                i = nf.find(h2b(key & M32, nb))
                new_used[i] = True; nf.take(i)
                if i < n and self.used[i]:
                    self.keys[i], key = key, self.keys[i]
                    self.used[i] = False
                else:
                    self.keys[i] = key
                    break
        self.used, self.bits, self.nf, self.walk = new_used, nb, nf, 0
        self.pos = {self.keys[i]: i for i in range(new_n) if new_used[i]}
        if n:                                                       # the keys of the old table's last run that went around the new table's end
            far = [self.pos[x] for x in tail_keys if self.pos[x] < 2 * (n - tail)]
            self.doublings[-1]["tail_far"] = max(far) if far else -1

    def put(self, key):
        n = self.n_buckets()
        if self.count >= (n >> 1) + (n >> 2):
            self.resize(n + 1)
            n = self.n_buckets()
        home = h2b(key & M32, self.bits)
        i = self.pos.get(key)
        if i is None:
            st = self.stages.get(self.bits)
            if st is None:
                st = self.stages[self.bits] = dict(before=list(self.used), new=[])
            i = self.nf.find(home)
            self.keys[i], self.used[i] = key, True
            self.nf.take(i); self.pos[key] = i
            self.count += 1
            st["new"].append((home, (i - home) & (n - 1), key))
        self.walk = max(self.walk, (i - home) & (n - 1))

    def replay(self, xs):
        for x in xs:
            self.put(x)
        return self


# ---- what the streaming replay makes of a model's report (kern_replay2.inc, layout.cpp, replay_plan.h) -----------------------------------------
R2_BASE_MAX, R2_LMAX, R2_MMAX, R2_HEAD, R2_SEG_LOG, R2_WIN = 4096, 512, 192, 2048, 14, 256        # kern_replay2.inc:34-39, 121; F2_NA :488


def streamed(model, sb=13):
    """the doublings and placement stages the streaming kernels do: those of capacities from 2^sb on, if the table outgrows 2^sb slots at all
    (replay_plan.h classify: large = final capacity > 2^SB; schedule: k_replay fills the table of 2^SB slots)"""
    if model.n_buckets() <= 1 << sb:
        return [], []
    return [d for d in model.doublings if d["n"] >= 1 << sb], [b for b in sorted(model.stages) if b > sb]


def place_outcome(stage, bits, seg_log=R2_SEG_LOG):
    """k_r2_place / k_r2_spill on one stage (kern_replay2.inc:897-1033): ordered probing per segment of 2^seg_log slots, a walk that leaves its
    segment finishes on the first HEAD slots of the next one (kern_launch.inc:498: HEAD = min(2048, segment / 2)).  Only which slots are taken
    matters for where a walk ends, so the keys go in put order.  Returns (walks that spill, does one run past the head: fail = 5)"""
    n = 1 << bits
    if bits <= seg_log:
        return 0, False                                             # one segment: the walk wraps around inside k_r2_place
    L = 1 << seg_log
    head = min(R2_HEAD, L // 2)
    used = list(stage["before"])
    spill = {}
    for home, _, _ in stage["new"]:
        seg, i = home >> seg_log, home
        while i < (seg + 1) * L and used[i]:
            i += 1
        if i < (seg + 1) * L:
            used[i] = True
        else:
            nxt = (seg + 1) & ((n >> seg_log) - 1)
            spill[nxt] = spill.get(nxt, 0) + 1
    fail5 = False
    for seg, cnt in spill.items():
        free = sum(1 for i in range(seg * L, seg * L + head) if not used[i])
        fail5 = fail5 or cnt > free
    return sum(spill.values()), fail5


def refusal_codes(model, sb=13, seg_log=R2_SEG_LOG):
    """the `fail` codes the thresholds of kern_replay2.inc raise on this table (a set; empty: the streaming replay goes through, r2_refused == 0)
      1  k_r2_dsmall: the literal prefix F0 (8, then on to the first unused slot) has F0 > R2_BASE_MAX and F0 < n (:417; the LDS windows of :359-407
         hold 512 old slots and hand a longer prefix to the arrays)
      6  r2_wave_run: a run of more than LMAX used old slots behind the prefix, or a region 2 L + 2 + wrap beyond RMAX = 2 LMAX + 2 + 256 (:152, :163).
         wrap = 2 min(128, used slots from slot 0 on) + 2 for the run that reaches the table's end (:157-161), whose LMAX is R2_MMAX = 192 when the run
         has that many slots or fewer (:576: the wave's own LDS) and R2_LMAX = 512 beyond
      7  r2_wave_run: a key of the last run needs a slot beyond the `wrap` first slots of the new table (:192)
      5  k_r2_spill: a walk reaches the end of the next segment's head (:1030)
    fail = 8 needs more runs in one round than a table of this file's sizes holds (many_big_runs' note below), 4 more spilling walks than a test of
    these sizes has keys (layout.cpp:154: the list has at least 2^20 entries), 9 a walk that leaves a window that the run's region lies inside by
    construction, and 10 a loop that ends before F reaches n, which k_r2_double's `while (F < n)` does not: none of them is predicted, none is claimed"""
    dbl, stages = streamed(model, sb)
    codes = set()
    for d in dbl:
        n = d["n"]
        used = [False] * n
        for s, ln in d["runs"]:
            used[s:s + ln] = [True] * ln
        F0 = min(n, 8)
        while F0 < n and used[F0 - 1]:
            F0 += 1
        if R2_BASE_MAX < F0 < n:
            codes.add(1)
        for s, ln in d["runs"]:
            if s >= F0 and ln > R2_LMAX:
                codes.add(6)
        tail = d["tail"] if n - d["tail"] >= F0 else 0
        if tail:
            j0 = 0
            while j0 < 128 and used[j0]:
                j0 += 1
            wrap = 2 * j0 + 2
            lmax = R2_MMAX if tail <= R2_MMAX else R2_LMAX
            if 2 * tail + 2 + wrap > 2 * lmax + 2 + 256:
                codes.add(6)
            if d["tail_far"] >= wrap:
                codes.add(7)
    for b in stages:
        if place_outcome(model.stages[b], b, seg_log)[1]:
            codes.add(5)
    return codes


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the dump of one sub-table
# ---------------------------------------------------------------------------------------------------------------------------------------------
def sub_tables(yak_bytes, pre=PRE):
    """[(capacity, [key << 10 | count in slot order])] of a .yak image (htab.c:373-394)"""
    out, off = [], 16
    for _ in range(1 << pre):
        cap, n = struct.unpack_from("<II", yak_bytes, off)
        out.append((cap, list(struct.unpack_from("<%dQ" % n, yak_bytes, off + 8))))
        off += 8 + 8 * n
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _case(name, k, xs, sub=SUB, **claims):
    return dict(name=name, k=k, sub=sub, xs=list(xs), img=image(xs, sub, k), claims=claims)


def _shuffled(xs, seed):
    xs = list(xs)
    random.Random(seed).shuffle(xs)
    return xs


def one_home(where, n_keys, k=31, sub=SUB):
    """n_keys keys of ONE home slot -- slot 0, the middle slot or the last slot (the cluster wraps) of every capacity up to the final one -- then the
    first five again.  The sizes used are 192 * 2^j + 8: every doubling finds the table at 75 % load, one run (two around the end) of 0.75 n slots,
    and 8 keys are placed behind the last one.  The ~7000 keys of a 16 Ki-slot table are not built: a cluster is walked key by key wherever one
    lane follows the literal rule (k_r2_dsmall's prefix, k_replay), 7000^2 / 2 dependent accesses -- tens of seconds of one lane.  Every branch
    such a table takes is taken by 392 keys under YAKAMD_R2_SMALL_BITS = 5 (the model's reports have the same shape at every capacity), and the
    prefix beyond R2_BASE_MAX by long_prefix, whose walks are short"""
    cap = 4
    while cap * 3 // 4 < n_keys:
        cap *= 2
    bits = cap.bit_length() - 1
    slot = dict(zero=0, mid=1 << (bits - 1), last=(1 << bits) - 1)[where]
    keys = Picker(sub, k, seed=3).same_home(slot, bits, n_keys)
    return _case("one_home_%s_%d" % (where, n_keys), k, keys + keys[:5], sub, final_bits=bits, cluster=n_keys, where=where)


def lastput_growth(k=31):
    """the `lastput` rule on a clustered table: exactly 0.75 x 512 keys of one home slot, then one of them again -- the trailing put-call on an
    existing key doubles the table (khashl.h:202), with nothing to place behind the doubling"""
    keys = Picker(SUB, k, seed=4).same_home(511, 9, 384)
    return _case("lastput_growth", k, keys + keys[100:101], final_bits=10, cluster=384)


def _ladder_layout(n_old, blocks, seed, n_keys, picker, extra=()):
    """keys with pairwise distinct home slots at n_old slots (so each sits in its home slot there, whatever the order): the given blocks of
    consecutive slots [(start, length)], guarded by an unused slot on either side, and uniform filler over the rest up to n_keys keys in all"""
    bits = n_old.bit_length() - 1
    taken, guard = set(), set()
    for s, ln in blocks:
        for i in range(s, s + ln):
            taken.add(i % n_old)
        guard.add((s - 1) % n_old); guard.add((s + ln) % n_old)
    assert not (taken & guard), "blocks touch"
    free = [i for i in range(n_old) if i not in taken and i not in guard]
    rnd = random.Random(seed)
    fill = rnd.sample(free, n_keys - len(taken) - len(extra))
    slots = sorted(taken) + fill + list(extra)
    return picker.one_per_slot(slots, bits)


LADDER = (8, 9, 64, 65, 160, 192, 193, 512)


def run_ladder(variant="plain", k=31, sub=SUB):
    """One sub-table that ends at 16 Ki slots.  Its 6144 first keys have pairwise distinct home slots at 8 Ki slots, so the old table of the last
    doubling holds exactly the runs laid out here -- 8, 9, 64, 65, 160, 192, 193 and 512 used slots between unused ones -- among uniform filler;
    put order shuffled; 200 more keys behind the doubling.
      plain    as said                                   over     a run of 513 as well: one past R2_LMAX
      wrap     the 193-slot run lies around the table's end, 100 slots before it and 93 from slot 0 on, and 30 further keys of the last 10 home
               slots make keys of the last run wrap: its region in the new table goes on at slot 0 (r2_wave_run's `wrap`)
      tail192 / tail193   the run that reaches the end of the table has 192 / 193 slots before it (R2_MMAX: the wave's own LDS, or wave 0's)"""
    n_old, n1 = 8192, 6144
    pk = Picker(sub, k, seed=5)
    ladder = list(LADDER) + ([513] if variant == "over" else [])
    blocks, at = [], 600
    for ln in ladder:
        if variant != "plain" and variant != "over" and ln == 193:
            continue
        blocks.append((at, ln)); at += ln + 37
    extra = []
    if variant == "wrap":
        blocks.append((n_old - 100, 193))
        extra = [n_old - 1 - (i % 10) for i in range(30)]
    elif variant in ("tail192", "tail193"):
        t = int(variant[4:])
        blocks.append((n_old - t, t + 5))
    first = _ladder_layout(n_old, blocks, 6, n1, pk, extra)
    more = pk.one_per_slot(random.Random(7).sample(range(2 * n_old), 200), 14)
    want = sorted(ladder if variant in ("plain", "over") else [l for l in ladder if l != 193])
    return _case("run_ladder_" + variant, k, _shuffled(first, 8) + more, sub, final_bits=14, ladder=want, variant=variant)


# fail = 8, the full list of long runs.  k_r2_double's s_big has 64 entries for the runs that do not end inside a 256-entry window -- 255 used slots or
# more (kern_replay2.inc:621, :577), not R2_MMAX + 1: the shorter ones are placed in the window.  A round [F, G) has G <= 2F <= n, so it holds at most
# n / 2 / 256 of them: 64 at 32 Ki old slots, the largest doubling of a sub-table that ends at 64 Ki -- the list is never too short there, and 65 take
# an old table of 64 Ki slots, beyond this file's sizes.  k_r2_dsmall's list has 256 entries for runs of 9 slots or more in a round below
# YAKAMD_R2_SMALL_F <= 4096: at most 2048 / 10 of them.  No case for either


def long_prefix(k=31):
    """the literal prefix of k_r2_dsmall beyond R2_BASE_MAX (fail = 1) without long walks: the old table of the last doubling (8 Ki slots) holds one
    run over slots [0, 4100], keys of pairwise distinct home slots"""
    n_old, n1 = 8192, 6144
    pk = Picker(SUB, k, seed=13)
    first = _ladder_layout(n_old, [(0, 4101)], 14, n1, pk)
    more = pk.one_per_slot(random.Random(15).sample(range(2 * n_old), 50), 14)
    return _case("long_prefix", k, _shuffled(first, 16) + more, final_bits=14, first=4101)


def segment_edge(where, cluster, final_bits=15, k=31, sub=SUB):
    """A sub-table of 2^final_bits slots filled to 75 % of half of that with keys of distinct home slots, then -- behind the last doubling, in the
    placement the streaming kernels do -- `cluster` keys whose home is the last slot before a segment boundary (`mid`: the middle of the table,
    a boundary of 16 Ki- and 1 Ki-slot segments alike) or before the table's end (`end`: the walks go on at slot 0).  All but one leave their
    segment; the last one ends `cluster - 2` slots into the next segment's head, which the filler leaves free"""
    n = 1 << final_bits
    pk = Picker(sub, k, seed=17)
    B = n // 2 if where == "mid" else 0
    keep_free = set((B + i) % n for i in range(-1, cluster + 40))
    rnd = random.Random(18)
    n1 = n // 2 * 3 // 4
    fill = rnd.sample([i for i in range(n) if i not in keep_free], n1 + 30)
    first = pk.one_per_slot(fill, final_bits)
    edge = pk.same_home((B - 1) % n, final_bits, cluster) if hi_bits(k) else pk.one_per_slot([(B - 1) % n] * cluster, final_bits)
    return _case("segment_%s_%d_%d" % (where, final_bits, cluster), k, first + edge, sub, final_bits=final_bits, cluster=cluster, boundary=B)


BLOCK_WIDTH = 11      # block bits of the largest filter the tests use: -b30 at pre 10 is 2^20 bits per sub-table, 2^11 blocks of 512 bits
PROBE_WIDTH = 29      # ... and bits [nb - 9, nb + 9) above them hold h1 and h2 of bbf.c:29-30: [1, 19) for -b20, [3, 21) for -b22, [11, 29) for -b30


def hot_block(n_keys, k=31, probes=False, sub=SUB):
    """n_keys distinct keys of ONE bloom block, each two or three times so that it survives the filter (bbf.c:25-42: an occurrence passes once all its
    probe bits are set).  The keys agree in the low 11 bits of hash >> pre -- the block index of every filter the tests use (-b20, -b22, -b30 at
    pre = 10: 1, 3 and 11 block bits; 31 shared bits, enough for any filter up to -b50, would leave one hashed bit free and two home slots) --
    and are random above, so the home slots are uniform.  probes: the low 29 bits agree, and with them both probe fields h1 and h2 of all three filters: every key
    probes the same bits.  At k = 21 only 3 bits are left above them: 8 keys at the most"""
    pk = Picker(sub, k, seed=19 + n_keys)
    width = PROBE_WIDTH if probes else BLOCK_WIDTH
    low = 0x155D5A5B & ((1 << width) - 1)
    keys = pk.same_block(low, width, n_keys)
    n_keys = len(keys)
    rnd = random.Random(20)
    seq = [x for x in keys for _ in range(2 + (rnd.random() < 0.3))]
    rnd.shuffle(seq)
    return _case("hot_block_%s%d" % ("probes_" if probes else "", n_keys), k, seq, sub, block_keys=n_keys, width=width)


def hot_key(counts=(2047, 2048, 2049, 4095, 4096, 65535, 65536, 70000), k=31, others=0):
    """one key per count, each in a sub-table of its own (SUB, SUB + 1, ...), `count` times in a row; others: interleaved with that many other keys of
    its bloom block -- and so of its level-2 sub-bucket, the top bits of the block index -- each twice"""
    recs, per_sub = [], []
    for j, c in enumerate(counts):
        sub = SUB + j
        pk = Picker(sub, k, seed=23 + j)
        keys = pk.same_block(0x2A5 + j, BLOCK_WIDTH, 1 + others)
        seq = [keys[0]] * c
        if others:
            step = max(1, c // (2 * others))
            for i, x in enumerate(keys[1:] * 2):
                seq.insert(min(len(seq), (i + 1) * step + i), x)
        per_sub.append((sub, seq))
        h = np.asarray(seq, dtype=np.uint64) << np.uint64(PRE) | np.uint64(sub)
        recs.append(records(hash64_inv_np(h, (1 << 2 * k) - 1), k))
    return dict(name="hot_key%s" % ("_among_%d" % others if others else ""), k=k, sub=SUB, xs=per_sub[0][1], per_sub=per_sub,
                img=np.concatenate(recs).tobytes(), claims=dict(counts=list(counts), others=others))


MIXED_SUBS = (500, 501, 502, 503)


def mixed(synth_img, k=31):
    """four cases in neighbouring sub-tables of one image with an ordinary read set around them (and a few of its k-mers inside them): every sub-table
    grows, more than 256 of them in a step.  The model speaks for sub-tables 500 ... 503 through their actual streams (oracle.extract_lists)"""
    parts = [one_home("zero", 200, k, 500), hot_block(769, k, sub=501), run_ladder("wrap", k, 502), segment_edge("mid", 300, 12, k, 503)]
    half = len(synth_img) // 2
    return dict(name="mixed", k=k, sub=500, xs=[], img=synth_img[:half] + b"".join(c["img"] for c in parts) + synth_img[half:], claims={})


# name -> builder(k).  The sizes of one_home are 192 * 2^j + 8: see its docstring
CASES = {
    "one_home_zero_200": lambda k: one_home("zero", 200, k), "one_home_mid_200": lambda k: one_home("mid", 200, k), "one_home_last_200": lambda k: one_home("last", 200, k),
    "one_home_zero_392": lambda k: one_home("zero", 392, k), "one_home_mid_392": lambda k: one_home("mid", 392, k), "one_home_last_392": lambda k: one_home("last", 392, k),
    "one_home_last_1544": lambda k: one_home("last", 1544, k),
    "lastput_growth": lastput_growth,
    "run_ladder_plain": lambda k: run_ladder("plain", k), "run_ladder_over": lambda k: run_ladder("over", k), "run_ladder_wrap": lambda k: run_ladder("wrap", k),
    "run_ladder_tail192": lambda k: run_ladder("tail192", k), "run_ladder_tail193": lambda k: run_ladder("tail193", k),
    "long_prefix": long_prefix,
    "segment_mid_15_100": lambda k: segment_edge("mid", 100, 15, k), "segment_mid_15_2049": lambda k: segment_edge("mid", 2049, 15, k), "segment_mid_15_2050": lambda k: segment_edge("mid", 2050, 15, k),
    "segment_end_15_600": lambda k: segment_edge("end", 600, 15, k),
    "segment_mid_12_513": lambda k: segment_edge("mid", 513, 12, k), "segment_mid_12_514": lambda k: segment_edge("mid", 514, 12, k), "segment_end_12_300": lambda k: segment_edge("end", 300, 12, k),
    "hot_block_9": lambda k: hot_block(9, k), "hot_block_600": lambda k: hot_block(600, k), "hot_block_624": lambda k: hot_block(624, k), "hot_block_625": lambda k: hot_block(625, k),
    "hot_block_768": lambda k: hot_block(768, k), "hot_block_769": lambda k: hot_block(769, k), "hot_block_1536": lambda k: hot_block(1536, k), "hot_block_1537": lambda k: hot_block(1537, k), "hot_block_3000": lambda k: hot_block(3000, k), "hot_block_probes_600": lambda k: hot_block(600, k, probes=True),
    "hot_key": lambda k: hot_key(k=k), "hot_key_among_600": lambda k: hot_key(k=k, others=600),
}
_built = {}


def case(name, k=31):
    """the case, built once per process"""
    if (name, k) not in _built:
        _built[name, k] = CASES[name](k)
    return _built[name, k]
