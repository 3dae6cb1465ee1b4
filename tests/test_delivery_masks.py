"""Random delivery's per-receiver masks: a plain restatement with a path census, the case list, and what can be
checked without a device.

delivery_mask_model restates, in Python integers over oracle.philox4x32_10, the definition in the comment above
oracle_delivery_mask (oracle/benor_oracle.c): the delivered-sender mask of one receiver in one phase.  Next to the
mask it returns a census: which path of the kernels (csrc/benor_kernels.hip random_tally, csrc/benor_random.hip
bern_tally) this very mask takes, by the kernels' control flow.

Floyd census (random_tally): `fast` aligned four-draw blocks; `screen` aligned blocks sent to the exact path because
lmin < jj + 4 (`screen_clean`: the screen hits of a mask that rejects no word at all, the screen's false alarms);
`redraws`, one (position of the rejected word in
its block, whether a further draw follows) per Lemire rejection; `misaligned` exact steps taken only because the
stream position is no multiple of four; `collisions` (t already in T, so jj joins); `short_last`, the length n < 4 of
a fast last block; `deliver_T`.

Bernoulli census (bern_tally<NW, B>): `direction` remove, add or none (c = q); `blocks`, the fix-up's Philox blocks;
fields refused before the quota is met because idx >= m (`pad`), because an earlier field of the same block flipped
that very sender (`repeat`), or by the mask's own state (`state`); `undone`, flips the kernel's speculative block
makes past the quota and takes back (`max_undone`: the most in one block).

cases() is a seeded list (case i reads np.random.default_rng(BASE + i) and SHAPES, nothing else): every reachable
<NW, B> instantiation at its smallest shape, the other shapes at which the code takes another path (m = 2^b, the most
padding, W32 mod 4 for the three- and one-word comparators' partial super-blocks, m mod 32 in {0, 1, 31}, a = 3 and
14, 16 q divisible by m), both sides of the sampler boundary, the Floyd shapes, scattered crashed nodes, trial ids
on both sides of 2^32, rounds up to 1024, both phases, and one N = 4096 network whose few live ids include 4095.
The Floyd sampler's rare paths come from a search (floyd_rare_pairs) over trial ids at (600, 525) and (600, 75).
tests/test_delivery_masks_gpu.py compares the device's masks with the model for every receiver of every case.  Here:

 (a) the model's mask equals oracle.delivery_mask (the C oracle) bit for bit, every receiver of every case;
 (b) popcount = q and no bit >= m;
 (c) the census conditions of test_census_*: the list reaches the paths it is there for.

Conditions that the definition rules out at a shape, and are therefore not asked there:
 * m = 2^(b-1) + 1 at b = 7 is m = 65, where k = min(q, m - q) <= 32 < 64: Floyd.  b = 7 has one Bernoulli shape,
   (128, 64), which is also its m = 2^b;
 * padding refusals need a field >= m: none at m = 2^b.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import benor
import oracle

M32 = 0xFFFFFFFF
RD = benor.BO_MODE_RANDOM_DELIVERY
STREAM_DELIVERY = 2


# ------------------------------------------------------------------------------------------------ the model
class Stream:
    """Philox stream 2 of one receiver-phase: word i = element i & 3 of block i >> 2."""

    def __init__(self, seed, trial, node, rnd, phase):
        self.key = (seed & M32, (seed >> 32) & M32)
        self.ctr = (trial & M32, (trial >> 32) & M32, ((rnd & 0x7FFF) << 16) | ((phase & 1) << 31),
                    (node & 0xFFF) | (STREAM_DELIVERY << 24))
        self.widx = 0
        self._i, self._blk = -1, None

    def word_at(self, i):
        if i >> 2 != self._i:
            self._i = i >> 2
            self._blk = oracle.philox4x32_10(self.key, (self.ctr[0], self.ctr[1], self.ctr[2] | self._i, self.ctr[3]))
        return self._blk[i & 3]

    def next(self):
        self.widx += 1
        return self.word_at(self.widx - 1)


def sampler_of(m, q):
    """None for Floyd (k < 64 or 8 k <= m), else (a, b) of the Bernoulli mask + fix-up."""
    k = min(q, m - q)
    if k < 64 or 8 * k <= m:
        return None
    return min(15, max(1, -(-16 * q // m))), max(1, (m - 1).bit_length())


def _floyd(s, m, q):
    e = m - q
    deliver_T = q <= e
    k = q if deliver_T else e
    cen = dict(sampler="floyd", fast=0, screen=0, screen_clean=0, redraws=[], misaligned=0, collisions=0, short_last=0,
               deliver_T=deliver_T)
    T, fast_left = 0, 0
    for j in range(m - k, m):
        pos, kind = s.widx, "fast"
        if fast_left == 0:
            if pos & 3:
                kind = "misaligned"
            elif min((s.word_at(pos + i) * (j + 1 + i)) & M32 for i in range(4)) >= j + 4:   # the kernel's screen
                fast_left = min(4, m - j)
                cen["fast"] += 1
                if fast_left < 4:
                    cen["short_last"] = fast_left
            else:
                kind = "screen"
        # t = uniform[0, j]: Lemire's multiply-shift, a word rejected when its low product is below 2^32 mod (j + 1)
        r, rejected = j + 1, []
        x = s.next() * r
        if x & M32 < r:
            thr = (1 << 32) % r
            while x & M32 < thr:
                rejected.append((s.widx - 1) & 3)
                x = s.next() * r
        t = x >> 32
        if kind == "fast":
            assert not rejected, "the screen let a rejection into the fast path"
            fast_left -= 1
        elif kind == "screen":
            cen["screen"] += 1
        else:
            cen["misaligned"] += 1
        cen["redraws"] += [(p, j < m - 1) for p in rejected]
        if (T >> t) & 1:
            cen["collisions"] += 1
            t = j
        T |= 1 << t
    if not cen["redraws"]:                               # (a rejection of any word of the mask makes its hits true ones)
        cen["screen_clean"] = cen["screen"]
    return (T if deliver_T else ((1 << m) - 1) & ~T), cen


def _bernoulli(s, m, q, a, b):
    tz = (a & -a).bit_length() - 1
    mask = 0
    for w in range((m + 31) // 32):
        r = 0
        for i in range(tz, 4):                       # bit = (u < a), u's bits tz .. 3 from one stream word each
            u = s.next()
            r = ((~u | r) if (a >> i) & 1 else (~u & r)) & M32
        mask |= r << (32 * w)
    mask &= (1 << m) - 1
    c = bin(mask).count("1")
    rm = c > q
    cen = dict(sampler="bernoulli", nw=4 - tz, b=b, direction="remove" if rm else ("add" if c < q else "none"), blocks=0,
               pad=0, repeat=0, state=0, undone=0, max_undone=0)
    per = 32 // b
    s.widx = (s.widx + 3) & ~3                       # the fields start at a fresh block
    while c != q:
        cen["blocks"] += 1
        flipped, spec, undone = set(), None, 0       # spec: the kernel's state of this block past the quota
        for _ in range(4):
            word = s.next()
            for _ in range(per):
                idx, word = word & ((1 << b) - 1), word >> b
                if spec is None:                     # the definition: fields are read while c != q
                    if idx >= m:
                        cen["pad"] += 1
                    elif (mask >> idx) & 1 == rm:
                        mask ^= 1 << idx
                        flipped.add(idx)
                        c += -1 if rm else 1
                        if c == q:
                            spec = mask
                    else:
                        cen["repeat" if idx in flipped else "state"] += 1
                elif idx < m and (spec >> idx) & 1 == rm:   # the rest of the block: flipped, counted, taken back
                    spec ^= 1 << idx
                    undone += 1
        cen["undone"] += undone
        cen["max_undone"] = max(cen["max_undone"], undone)
    return mask, cen


def delivery_mask_model(seed, trial, node, rnd, phase, m, q, sampler="defined"):
    """(mask over compact sender indices as an int, census).  sampler: "defined" picks by (m, q) as the definition
    does; "floyd" / "bernoulli" force one (the boundary test: the two give different masks)."""
    s = Stream(seed, trial, node, rnd, phase)
    ab = sampler_of(m, q)
    if sampler == "floyd" or (sampler == "defined" and ab is None):
        return _floyd(s, m, q)
    if ab is None:
        ab = min(15, max(1, -(-16 * q // m))), max(1, (m - 1).bit_length())
    return _bernoulli(s, m, q, *ab)


def mask_words(mask, m):
    return [(mask >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range((m + 63) // 64)]


# ------------------------------------------------------------------------------------------------ the shapes
# The smallest (m, q) of each reachable <NW, B> (b = 7 only with a = 8: NW = 1), enumerated over 2 <= m <= 4096.
BERN_TABLE = {
    1: {7: (128, 64), 8: (129, 64), 9: (257, 113), 10: (513, 225), 11: (1025, 449), 12: (2049, 897)},
    2: {8: (205, 141), 9: (257, 64), 10: (513, 97), 11: (1025, 193), 12: (2049, 385)},
    3: {8: (147, 83), 9: (257, 81), 10: (513, 161), 11: (1025, 321), 12: (2049, 641)},
    4: {8: (129, 65), 9: (257, 65), 10: (513, 65), 11: (1025, 129), 12: (2049, 257)},
}
SHAPES = [(m, q, f"bern<{nw},{b}> smallest") for nw, row in BERN_TABLE.items() for b, (m, q) in row.items()]
SHAPES += [
    # m = 2^b: no padding, rows == W32 (b = 7: (128, 64) above)
    (256, 170, "bern m=2^8"), (512, 380, "bern m=2^9"), (1024, 683, "bern m=2^10"), (2048, 1229, "bern m=2^11"),
    (4096, 2048, "bern m=2^12, 16q|m"),
    # m mod 32 = 31 with W32 odd and even (mod 32 = 1: the 2^(b-1) + 1 shapes; = 0: the powers of two)
    (159, 80, "bern m%32=31 W32=5"), (191, 96, "bern m%32=31 W32=6"),
    # the partial super-blocks of the three-word (4 mask words per 3 blocks) and one-word (4 per block) comparators,
    # W32 mod 4 = 2, 3, 0 (= 1: the smallest shapes), and the two-word one (2 per block) at an even W32
    (180, 108, "bern NW=3 W32%4=2"), (220, 132, "bern NW=3 W32%4=3"), (256, 156, "bern NW=3 W32%4=0"),
    (180, 90, "bern NW=1 W32%4=2"), (220, 110, "bern NW=1 W32%4=3"), (256, 180, "bern NW=2 W32 even"),
    (400, 70, "bern a=3"), (400, 336, "bern a=14"), (256, 176, "bern 16q|m a=11"),
    # a smallest shape has 16 q / m just above a - 1: its masks start some m / 16 above q (four standard deviations
    # at b >= 10) and only remove.  Balanced shapes, 16 q just below a m, for the instantiations that lack an add mask
    (1025, 512, "bern<1,11> balanced"), (513, 128, "bern<2,10> balanced"), (1025, 256, "bern<2,11> balanced"),
    (2049, 512, "bern<2,12> balanced"), (2049, 768, "bern<3,12> balanced"), (1025, 192, "bern<4,11> balanced"),
    (2049, 384, "bern<4,12> balanced"),
    # the sampler boundary from both sides: k = 63 | 64, and 8k = m | 8k = m + 8
    (200, 63, "floyd k=63"), (200, 64, "bern k=64"), (600, 525, "floyd 8k=m"), (600, 524, "bern 8k=m+8"),
    (600, 75, "floyd 8k=m deliver_T"),
    # Floyd: m <= 32, 64, 65, above 2048 with k < 64; k = 0, k = 1 in both senses; k mod 4 = 3, 3, 1, 2
    (20, 13, "floyd m<=32 k=7"), (64, 31, "floyd m=64 k=31 deliver_T"), (65, 40, "floyd m=65 k=25"),
    (2100, 2050, "floyd m>2048 k=50"), (50, 50, "floyd k=0"), (37, 36, "floyd k=1 complement"),
    (37, 1, "floyd k=1 deliver_T"),
]
TRIALS = (0, 2**32 - 1, 2**32, 2**40 + 12345)
ROUNDS = (1, 2, 255, 256, 1024)
BASE = 26000
RARE_SHAPES = ((600, 525), (600, 75))


@dataclasses.dataclass(frozen=True)
class Case:
    tag: str
    N: int
    F: int
    faulty: tuple
    seed: int
    trial: int
    rnd: int
    phase: int

    @property
    def live(self):
        return [i for i in range(self.N) if not self.faulty[i]]

    @property
    def m(self):
        return self.N - sum(self.faulty)

    @property
    def q(self):
        return self.N - self.F

    def __str__(self):
        return (f"{self.tag}: N={self.N} F={self.F} m={self.m} q={self.q} seed={self.seed:#x} trial={self.trial} "
                f"round={self.rnd} phase={self.phase}")


def network(rng, m, q, N=None):
    """(N, F, faulty): m live nodes scattered over N ids (N = m + f, 2 <= f <= 6 crashed, unless given), quorum q."""
    if N is None:
        N = min(4096, m + int(rng.integers(2, 7)))
    faulty = [False] * N
    for i in rng.choice(N - 1 if N == 4096 else N, N - m, replace=False):    # (N = 4096: id 4095 stays live)
        faulty[int(i)] = True
    return N, N - q, tuple(faulty)


def _cases():
    out = []
    for m, q, tag in SHAPES:
        for _ in range(3 if m <= 300 else (2 if m <= 600 else 1)):
            rng = np.random.default_rng(BASE + len(out))
            N, F, fl = network(rng, m, q)
            out.append(Case(tag, N, F, fl, int(rng.integers(0, 2**63)), TRIALS[int(rng.integers(0, 4))],
                            ROUNDS[int(rng.integers(0, 5))], int(rng.integers(0, 2))))
    for phase in (0, 1):                                 # few live nodes among 4096 ids, 4095 one of them
        rng = np.random.default_rng(BASE + len(out))
        N, F, fl = network(rng, 200, 100, N=4096)
        assert not fl[4095] and F == 3996
        out.append(Case("bern N=4096 m=200", N, F, fl, int(rng.integers(0, 2**63)), 2**32 + phase, 256 - phase, phase))
    return out


# ------------------------------------------------------------------------------------------------ the rare paths
K0, K1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85


def philox_np(key, c0, c1, c2, c3):
    """Philox4x32-10 over uint64 arrays holding 32-bit words (checked against the oracle's in test_philox_np)."""
    lo = np.uint64(M32)
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k0, k1 = key
    for _ in range(10):
        p0, p1 = np.uint64(K0) * c[0], np.uint64(K1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + W0) & M32, (k1 + W1) & M32
    return c


def floyd_candidates(seed, live, q, rnd, trials):
    """(trial, phase, c) whose mask may leave the fast path: some word i of the receiver's stream, taken as draw i, has
    a low product below its range + 3.  That holds for every screen hit and every first rejection of a mask (the
    screen compares a block's smallest low product with its first range + 3, and up to the first rejection word i is
    draw i); the model then says what each candidate is."""
    m = len(live)
    k = min(q, m - q)
    nb = (k + 3) // 4
    key = (seed & M32, seed >> 32)
    tr = np.asarray(trials, dtype=np.uint64)[:, None, None, None]
    ph = np.arange(2, dtype=np.uint64)[None, :, None, None]
    nd = np.asarray(live, dtype=np.uint64)[None, None, :, None]
    bl = np.arange(nb, dtype=np.uint64)[None, None, None, :]
    shape = (len(trials), 2, m, nb)
    words = philox_np(key, np.broadcast_to(tr & np.uint64(M32), shape), np.broadcast_to(tr >> np.uint64(32), shape),
                      np.broadcast_to(bl | np.uint64((rnd & 0x7FFF) << 16) | (ph << np.uint64(31)), shape),
                      np.broadcast_to(nd | np.uint64(STREAM_DELIVERY << 24), shape))
    hit = np.zeros(shape[:3], dtype=bool)
    for e in range(4):
        i = np.arange(nb, dtype=np.uint64) * np.uint64(4) + np.uint64(e)
        rng_ = np.uint64(m - k + 1) + i
        low = (words[e] * rng_) & np.uint64(M32)
        hit |= ((low < rng_ + np.uint64(3)) & (i < np.uint64(k))).any(axis=3)
    return [(int(trials[t]), int(p), int(c)) for t, p, c in zip(*np.nonzero(hit))]


RARE_WANT = dict(redraw_masks=8, first=1, last=1, screen_clean=4)
RARE_CHUNK, RARE_MAX_CHUNKS = 50, 80


@functools.lru_cache(maxsize=None)
def floyd_rare_pairs():
    """The (trial, phase) pairs, per rare shape, whose masks meet RARE_WANT between them, redraws and clean screen hits each over both shapes: trial ids are scanned
    upward from just below 2^32 (first shape) and from 2^40 (second) in chunks, alternating between the shapes, the
    candidates classified by the model, until the counts are met (or the scan's cap: the census test then fails).
    Returns ([Case], counts)."""
    cfg = []
    for s, (m, q) in enumerate(RARE_SHAPES):
        rng = np.random.default_rng(BASE + 900 + s)
        N, F, fl = network(rng, m, q)
        cfg.append((N, F, fl, int(rng.integers(0, 2**63)), (255, 1024)[s], (2**32 - 150, 2**40)[s]))
    got = dict(redraw_masks=0, first=0, last=0, screen_clean=0)
    per_shape, clean_per_shape = [0] * len(RARE_SHAPES), [0] * len(RARE_SHAPES)
    pairs = []
    for chunk in range(RARE_MAX_CHUNKS):
        s = chunk % len(cfg)
        N, F, fl, seed, rnd, t0 = cfg[s]
        live = [i for i in range(N) if not fl[i]]
        trials = [t0 + (chunk // len(cfg)) * RARE_CHUNK + i for i in range(RARE_CHUNK)]
        for trial, phase, c in floyd_candidates(seed, live, N - F, rnd, trials):
            _, cen = delivery_mask_model(seed, trial, live[c], rnd, phase, len(live), N - F)
            further = [p for p, more in cen["redraws"] if more]
            need = bool(further) and (got["redraw_masks"] < RARE_WANT["redraw_masks"] or not per_shape[s] or
                                      (0 in further and not got["first"]) or (3 in further and not got["last"]))
            need_clean = cen["screen_clean"] and (got["screen_clean"] < RARE_WANT["screen_clean"] or
                                                  not clean_per_shape[s])
            if not need and not need_clean:
                continue                                  # nothing the list still lacks
            got["redraw_masks"] += bool(further)
            got["first"] += 0 in further
            got["last"] += 3 in further
            got["screen_clean"] += cen["screen_clean"]
            per_shape[s] += bool(further)
            clean_per_shape[s] += cen["screen_clean"]
            case = Case(f"floyd rare {RARE_SHAPES[s]}", N, F, fl, seed, trial, rnd, phase)
            if case not in pairs:
                pairs.append(case)
        if all(got[k] >= v for k, v in RARE_WANT.items()) and all(per_shape) and all(clean_per_shape):
            break
    return pairs, dict(got, per_shape=tuple(per_shape), clean_per_shape=tuple(clean_per_shape))


@functools.lru_cache(maxsize=None)
def cases():
    return _cases() + floyd_rare_pairs()[0]


@functools.lru_cache(maxsize=None)
def case_masks(i):
    """The model's (masks, censuses) of every receiver of case i, in compact order."""
    c = cases()[i]
    live = c.live
    res = [delivery_mask_model(c.seed, c.trial, node, c.rnd, c.phase, c.m, c.q) for node in live]
    return [r[0] for r in res], [r[1] for r in res]


def census_table():
    """One line per case: what its masks reach (printed when a census condition fails)."""
    lines = []
    for i, c in enumerate(cases()):
        cens = case_masks(i)[1]
        if cens[0]["sampler"] == "floyd":
            s = dict(fast=sum(x["fast"] for x in cens), screen=sum(x["screen"] for x in cens),
                     screen_clean=sum(x["screen_clean"] for x in cens), redraws=[r for x in cens for r in x["redraws"]],
                     misaligned=sum(x["misaligned"] for x in cens), collisions=sum(x["collisions"] for x in cens),
                     short_last=sorted({x["short_last"] for x in cens}), deliver_T=cens[0]["deliver_T"])
        else:
            s = dict(nw=cens[0]["nw"], b=cens[0]["b"], remove=sum(x["direction"] == "remove" for x in cens),
                     add=sum(x["direction"] == "add" for x in cens), none=sum(x["direction"] == "none" for x in cens),
                     blocks2=sum(x["blocks"] >= 2 for x in cens), pad=sum(x["pad"] for x in cens),
                     repeat=sum(x["repeat"] for x in cens), state=sum(x["state"] for x in cens),
                     undone=sum(x["undone"] > 0 for x in cens), max_undone=max(x["max_undone"] for x in cens))
        lines.append(f"{i:3d} {c}\n      {s}")
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ the tests
def test_philox_np():
    rng = np.random.default_rng(BASE - 1)
    key = (int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32)))
    ctr = rng.integers(0, 2**32, size=(4, 50), dtype=np.uint64)
    got = philox_np(key, *ctr)
    for j in range(50):
        assert [int(g[j]) for g in got] == oracle.philox4x32_10(key, [int(ctr[e][j]) for e in range(4)])


def test_shapes_are_what_their_tags_say():
    """The table's shapes reach their instantiation by the definition's rule and by the oracle's, they are the
    smallest that do, and every boundary of the sampler choice is taken from both sides."""
    for m, q, tag in SHAPES:
        ab = sampler_of(m, q)
        assert ab == oracle.delivery_bernoulli(m, q), (m, q)
        assert (ab is None) == tag.startswith("floyd"), (m, q, tag)
    first = {}
    for m in range(2, 4097):                              # (vectorised over q: sampler_of's rule again)
        q = np.arange(1, m + 1)
        k = np.minimum(q, m - q)
        a = np.clip(-(-16 * q // m), 1, 15)
        nw = 4 - np.log2(a & -a).astype(int)
        for i in np.nonzero((k >= 64) & (8 * k > m))[0]:
            first.setdefault((int(nw[i]), (m - 1).bit_length()), (m, int(q[i])))
    assert first == {(nw, b): mq for nw, row in BERN_TABLE.items() for b, mq in row.items()}
    assert len(first) == 21
    assert sampler_of(200, 63) is None and sampler_of(200, 64) and sampler_of(600, 525) is None and sampler_of(600, 524)
    assert 8 * 75 == 600 and 8 * 76 == 600 + 8


def test_case_list_covers_the_inputs():
    cs = cases()
    for t in TRIALS:
        assert sum(c.trial == t for c in cs) >= 3, t
    for r in ROUNDS:
        assert sum(c.rnd == r for c in cs) >= 3, r
    assert sum(c.phase for c in cs) >= 10 and sum(1 - c.phase for c in cs) >= 10
    assert all(0 < sum(c.faulty) and c.faulty != tuple(sorted(c.faulty, reverse=True)) for c in cs if c.m < 4096)
    assert any(c.N == 4096 and not c.faulty[4095] and c.m == 200 for c in cs)
    assert any(c.trial >= 2**32 for c in cs if c.tag.startswith("floyd rare"))
    for c in cs:                                          # the host plans every case on the random-delivery kernel
        assert benor.kernel_for(c.N, c.F, list(c.faulty), mode=RD, k_max=16) == benor.BO_KERNEL_RANDOM, str(c)


def _model_is_the_oracle(i):
    c = cases()[i]
    masks, _ = case_masks(i)
    for node, mask in zip(c.live, masks):
        assert mask_words(mask, c.m) == oracle.delivery_mask(c.seed, c.trial, node, c.rnd, c.phase, c.m, c.q), (str(c), node)
        assert bin(mask).count("1") == c.q and mask >> c.m == 0, (str(c), node)


N_LISTED = len(_cases())                                  # (the searched cases follow them in cases())


@pytest.mark.parametrize("i", range(N_LISTED))
def test_model_is_the_oracle(i):
    """(a) and (b): two independent statements of one definition agree, and the mask is a q-subset of [0, m)."""
    _model_is_the_oracle(i)


def test_model_is_the_oracle_on_the_rare_paths():
    assert len(cases()) > N_LISTED
    for i in range(N_LISTED, len(cases())):
        _model_is_the_oracle(i)


def test_boundary_sides_draw_different_masks():
    """Across the sampler boundary the two samplers give different masks from the same stream, so a plan that ran
    the other kernel could not pass the device comparison: that comparison is how a plan reports its sampler."""
    for i, c in enumerate(cases()):
        if "k=63" in c.tag or "k=64" in c.tag or "8k=m" in c.tag:
            other = "bernoulli" if sampler_of(c.m, c.q) is None else "floyd"
            for node, a in zip(c.live, case_masks(i)[0]):       # every receiver: one equal row would hide there
                b = delivery_mask_model(c.seed, c.trial, node, c.rnd, c.phase, c.m, c.q, sampler=other)[0]
                assert a != b, (str(c), node)


def _floyd_census():
    return [(cases()[i], x) for i in range(len(cases())) for x in case_masks(i)[1] if x["sampler"] == "floyd"]


def _bern_census():
    return [(cases()[i], x) for i in range(len(cases())) for x in case_masks(i)[1] if x["sampler"] == "bernoulli"]


def test_census_floyd():
    """(c) The Floyd paths the list must reach."""
    cen = _floyd_census()
    table = census_table
    redraw = [(c, x) for c, x in cen if any(more for _, more in x["redraws"])]
    assert len(redraw) >= 8, table()
    assert len({(c.m, c.q) for c, _ in redraw}) >= 2, table()
    pos = {p for _, x in redraw for p, more in x["redraws"] if more}
    assert 0 in pos and 3 in pos, table()       # a rejected first word, and a last one: its redraw is the next block's
    clean = [(c, x) for c, x in cen if x["screen_clean"]]
    assert all(not x["redraws"] for _, x in clean), table()
    assert sum(x["screen_clean"] for _, x in clean) >= 4, table()     # the screen's false alarms: no word rejected
    assert len({(c.m, c.q) for c, _ in clean}) >= 2, table()
    assert sum(x["collisions"] for _, x in cen) >= 50, table()
    assert {x["short_last"] for _, x in cen} >= {1, 2, 3}, table()
    assert {x["deliver_T"] for _, x in cen} == {True, False}, table()
    assert sum(x["misaligned"] for _, x in cen) >= 12, table()     # three after every clean screen hit
    assert sum(x["fast"] for _, x in cen) >= 1000, table()
    ks = {min(c.q, c.m - c.q) for c, _ in cen}
    assert {0, 1} <= ks and {k % 4 for k in ks} == {0, 1, 2, 3}, table()
    ms = {c.m for c, _ in cen}
    assert any(m <= 32 for m in ms) and {64, 65} <= ms and any(m > 2048 for m in ms), table()


def test_census_bernoulli():
    """(c) The Bernoulli paths: per instantiation a remove and an add mask, a mask with two fix-up blocks or more and
    one with a flip taken back; over the list a block with two flips taken back, five masks with c = q, five
    same-block repeats, and padding refusals at every m that is no power of two."""
    cen = _bern_census()
    table = census_table
    inst = {}
    for _, x in cen:
        inst.setdefault((x["nw"], x["b"]), []).append(x)
    assert sorted(inst) == sorted((nw, b) for nw, row in BERN_TABLE.items() for b in row), table()
    for key, xs in inst.items():
        assert any(x["direction"] == "remove" for x in xs), (key, table())
        assert any(x["direction"] == "add" for x in xs), (key, table())
        assert any(x["blocks"] >= 2 for x in xs), (key, table())
        assert any(x["undone"] >= 1 for x in xs), (key, table())
    assert max(x["max_undone"] for _, x in cen) >= 2, table()
    assert sum(x["direction"] == "none" for _, x in cen) >= 5, table()
    assert sum(x["repeat"] for _, x in cen) >= 5, table()
    for m in sorted({c.m for c, _ in cen}):
        pad = sum(x["pad"] for c, x in cen if c.m == m)
        assert (pad == 0) if m & (m - 1) == 0 else (pad > 0), (m, table())
    a_of = {sampler_of(c.m, c.q)[0] for c, _ in cen}
    assert {3, 14} <= a_of, table()
    assert any(16 * c.q % c.m == 0 for c, _ in cen), table()
    for b in range(8, 13):                                   # m = 2^b and m = 2^(b-1) + 1 (b = 7: the docstring)
        assert {1 << b, (1 << (b - 1)) + 1} <= {c.m for c, _ in cen}, b
    assert {c.m % 32 for c, _ in cen} >= {0, 1, 31} and {((c.m + 31) // 32) % 2 for c, _ in cen} == {0, 1}
    for nw, per in ((3, 4), (1, 4), (2, 2)):                 # every remainder of the comparator's super-block
        assert {((c.m + 31) // 32) % per for c, x in cen if x["nw"] == nw} == set(range(per)), (nw, table())


def test_entry_refuses_what_it_cannot_answer():
    """bo_plan_delivery_masks without a plan: an argument error, as bo_plan_rule's; a plan itself needs a device."""
    L = benor.lib()
    out = (ctypes.c_uint64 * 4)()
    assert L.bo_plan_delivery_masks(None, 0, 1, 0, out) == benor.BO_ERR_INVALID_ARGUMENT
    assert "NULL" in benor.last_error()
    assert L.bo_abi_version() == 8                          # an added entry: no struct changed
