"""BO_MODE_CRASH_SUBSET, crashes during the run whose last broadcast reaches an
arbitrary subset of the receivers (CPU suite).

The definition, restated here in plain Python over
tests/test_crash_tally.py's schedule and tests/test_tally3.py's draw3 -- nothing
from the kernel; tests/test_crash_subset_gpu.py checks the kernel against it bit
for bit.  It is BO_MODE_CRASH_PARTIAL's definition (tests/test_crash_partial.py)
with one change:

* Reach.  The configuration word that mode 6 reads as crash_cut is crash_reach, a
  probability in units of 2^-32; every 32-bit value is valid.  Crasher p's step-s
  message reaches receiver c (compact indices) iff crash_reach == UINT32_MAX or
  word(p, c) < crash_reach, word(p, c) = element c & 3 of the Philox4x32-10 block
  ctr = {trial_lo, trial_hi, p | (c >> 2) << 12, 9 << 24}, key = seed (stream 9).
  The word is keyed by trial, crasher and receiver only.  crash_reach = 0 reaches
  nobody, UINT32_MAX everybody; neither draws a stream-9 word.
* Step s: C_s = the alive nodes scheduled at s, A_s the alive set without them.
  p in C_s does not receive at step s; its step-s message (its x at an R-step,
  the proposal it formed at step s - 1 at a P-step) reaches the receivers it
  reaches.  Receiver c in A_s draws draw3 with m = m_s + |H_c| and class sizes
  over A_s + H_c, H_c = {p in C_s : p reaches c}; stream-5 block of (trial, c, r),
  stream-6 walk, the m = q shortcut per receiver.

The law is checked against a mask-level simulation written here with numpy
(explicit Bernoulli reach per crasher and receiver, explicit pools A_s + H_c and
a uniform q-subset of each), which shares nothing with the count-level argument.
"""
import functools

import numpy as np
import pytest

import benor
import oracle
import test_crash_partial as m6
import test_crash_tally as m5
import test_tally3 as t3
from test_crash_tally import at, schedule, table_bytes
from test_tally import chi2_two_sample, first, philox
from test_tally3 import Q, draw3

M5 = benor.BO_MODE_CRASH_TALLY
M6 = benor.BO_MODE_CRASH_PARTIAL
M7 = getattr(benor, "BO_MODE_CRASH_SUBSET", None)           # absent before the mode: every test fails
ALL = 0xFFFFFFFF
STREAM_TALLY, STREAM_REACH = 5, 9
SEED = t3.SEED
MIB = 1 << 20
HALF, QUARTER = 1 << 31, 1 << 30


# ------------------------------------------------------------ restatement
def reach(seed, trial, p, c, crash_reach):
    """Whether crasher p's last message reaches receiver c (compact indices): stream 9."""
    if crash_reach == ALL:
        return True
    if crash_reach == 0:
        return False
    return philox(seed, (trial & 0xFFFFFFFF, trial >> 32, p | (c >> 2) << 12, STREAM_REACH << 24))[c & 3] < crash_reach


def subset_trial(N, F, faulty, seed, trial, k_max, initial_values=None, crash_at=None, crash_count=0, crash_window=0,
                 crash_reach=0):
    """One trial: (histogram bins it increments, rounds, per-node states)."""
    live = [i for i in range(N) if not faulty[i]]
    m0, q = len(live), N - F
    states = [{"killed": True, "x": None, "decided": None, "k": None} if faulty[i] else None for i in range(N)]
    if m0 == 0:
        return [2], 0, states
    assert 0 <= crash_reach <= ALL
    sched = schedule(seed, trial, live, crash_at, crash_count, crash_window)
    assert (N - m0) + sum(s is not None for s in sched) <= F
    if initial_values is None:
        x = [oracle.random_init(seed, trial, c, m0) for c in range(m0)]
    else:
        x = [2 if initial_values[i] == Q else initial_values[i] for i in live]
    alive = [True] * m0
    dec = [False] * m0
    tlo, thi = trial & 0xFFFFFFFF, trial >> 32

    def step(s, r, phase, vals, blocks):
        """Step s: its crashers leave; {receiver: (c0, c1)} over the alive set, None if it is empty."""
        C = [c for c in range(m0) if alive[c] and sched[c] == s]
        for c in C:
            alive[c] = False
            states[live[c]] = {"killed": True, "x": Q if x[c] == 2 else x[c], "decided": dec[c], "k": r}
        A = [c for c in range(m0) if alive[c]]
        if not A:
            return None
        assert len(A) >= q
        out = {}
        for c in A:
            H = [p for p in C if reach(seed, trial, p, c, crash_reach)]
            sizes = tuple(sum(vals[a] == v for a in A + H) for v in (0, 1, 2))   # the class sizes over the pool A + H
            b = blocks[c]
            u = b[1] << 32 | b[0] if phase == 0 else b[3] << 32 | b[2]
            out[c] = draw3(len(A) + len(H), q, sizes, seed, trial, c, r, phase, u)
        return out

    R = 0
    prop = [2] * m0
    for r in range(1, k_max + 1):
        blocks = {c: philox(seed, (tlo, thi, c, (r - 1) | STREAM_TALLY << 24)) for c in range(m0) if alive[c]}
        cnt = step(2 * (r - 1), r, 0, x, blocks)
        if cnt is None:
            return [2], 0, states
        for c, (c0, c1) in cnt.items():
            prop[c] = 0 if c0 > c1 else 1 if c1 > c0 else 2
        cnt = step(2 * (r - 1) + 1, r, 1, prop, blocks)        # a P-step crasher proposed; it does not vote
        if cnt is None:
            return [2], 0, states
        for c, (c0, c1) in cnt.items():
            if c0 > F:
                x[c], dec[c] = 0, True
            elif c1 > F:
                x[c], dec[c] = 1, True
            elif c0 != c1:
                x[c] = 1 if c1 > c0 else 0
            else:
                x[c] = oracle.coin(seed, trial, c, r)
        R = r
        if all(dec[c] for c in cnt):
            break
    A = [c for c in range(m0) if alive[c]]
    ones = sum(x[c] for c in A)
    v = 2 if 0 < ones < len(A) else (1 if ones else 0)
    all_dec = all(dec[c] for c in A)
    bins = [R * 3 + v] if all_dec else [v]
    if all_dec and v == 2:
        bins.append((k_max + 1) * 3)
    for c in A:
        states[live[c]] = {"killed": False, "x": x[c], "decided": dec[c], "k": R + 1}
    return bins, (R if all_dec else 0), states


def subset_hist(N, F, faulty, seed, trial_begin, trial_count, k_max, initial_values=None, **sched):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in subset_trial(N, F, faulty, seed, t, k_max, initial_values, **sched)[0]:
            h[b] += 1
    return h


# ------------------------------------------- mask-level simulation (numpy)
def mask_sim_hist(N, F, faulty, k_max, trials, rng, initial_values=None, crash_at=None, crash_count=0,
                  crash_window=0, crash_reach=0, chunk=10000):
    """The same model at the level of inboxes: at every step each alive receiver c
    hears a uniform q-subset (the q smallest of iid uniform keys) of its pool,
    the alive senders and the step's crashers that reach c -- an independent
    Bernoulli(crash_reach / 2^32) per (crasher, receiver), drawn explicitly;
    schedules, reach, initial values and coins from `rng`."""
    live = [i for i in range(N) if not faulty[i]]
    m0, q = len(live), N - F
    hist = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    never = 1 << 30
    prob = 1.0 if crash_reach == ALL else crash_reach / 2.0 ** 32

    def counts(vals, alive, going, hears):
        n = len(vals)
        if q == 0:
            return np.zeros((n, m0), dtype=np.int64), np.zeros((n, m0), dtype=np.int64)
        pool = alive[:, None, :] | (going[:, None, :] & hears)                     # [trial, receiver, sender]
        keys = rng.random((n, m0, m0))
        keys[~pool] = 2.0
        inbox = np.argpartition(keys, q - 1, axis=2)[:, :, :q]
        assert (np.take_along_axis(keys, inbox, axis=2) < 1.5).all(axis=2)[alive].all()   # a receiver's pool holds a quorum
        heard = np.take_along_axis(np.broadcast_to(vals[:, None, :], keys.shape), inbox, axis=2)
        return (heard == 0).sum(axis=2), (heard == 1).sum(axis=2)

    def finish(x, alive, dec, R):
        n_alive = alive.sum(axis=1)
        ones = ((x == 1) & alive).sum(axis=1)
        v = np.where((ones > 0) & (ones < n_alive), 2, np.where(ones > 0, 1, 0))
        all_dec = (dec | ~alive).all(axis=1)
        np.add.at(hist, np.where(all_dec, R * 3 + v, v), 1)
        hist[-1] += int((all_dec & (v == 2)).sum())

    for lo in range(0, trials, chunk):
        n = min(chunk, trials - lo)
        if initial_values is None:
            x = rng.integers(0, 2, size=(n, m0)).astype(np.int8)
        else:
            x = np.tile(np.array([2 if initial_values[i] == Q else initial_values[i] for i in live], dtype=np.int8), (n, 1))
        sched = np.full((n, m0), never, dtype=np.int64)
        if crash_at is not None:
            sched[:] = [never if crash_at[i] in (None, benor.NEVER) else crash_at[i] for i in live]
        elif crash_count:
            who = np.argsort(rng.random((n, m0)), axis=1)[:, :crash_count]
            np.put_along_axis(sched, who, rng.integers(0, crash_window, size=(n, crash_count)), axis=1)
        hears = rng.random((n, m0, m0)) < prob               # [trial, receiver, sender]: a node crashes once
        alive = np.ones((n, m0), dtype=bool)
        dec = np.zeros((n, m0), dtype=bool)
        if m0 == 0:
            hist[2] += n
            continue
        for r in range(1, k_max + 1):
            going = alive & (sched == 2 * (r - 1))
            alive &= ~going
            gone = ~alive.any(axis=1)
            c0, c1 = counts(x, alive, going, hears)
            prop = np.where(c0 > c1, 0, np.where(c1 > c0, 1, 2)).astype(np.int8)
            going = alive & (sched == 2 * (r - 1) + 1)
            alive &= ~going
            gone |= ~alive.any(axis=1)
            c0, c1 = counts(prop, alive, going, hears)
            coin = rng.integers(0, 2, size=(len(x), m0))
            new = np.where(c0 > F, 0, np.where(c1 > F, 1, np.where(c1 > c0, 1, np.where(c0 > c1, 0, coin))))
            x = np.where(alive, new, x).astype(np.int8)
            dec |= alive & ((c0 > F) | (c1 > F))
            hist[2] += int(gone.sum())                      # nobody left: bin[2]
            halted = (dec | ~alive).all(axis=1) & ~gone
            if r == k_max:
                halted = ~gone
            finish(x[halted], alive[halted], dec[halted], r)
            keep = ~halted & ~gone
            x, alive, dec, sched, hears = x[keep], alive[keep], dec[keep], sched[keep], hears[keep]
            if not len(x):
                break
    return hist


# ---------------------------------------------------------------- the tests
def test_the_mode_exists():
    assert M7 == 7 and benor.REACH_ALL == ALL
    assert benor.BO_KERNEL_TALLY_SUBSET == 13 and benor.BO_KERNEL_TALLY_SUBSET in benor.KERNEL_NAMES
    assert benor.lib().bo_abi_version() == 8                # the struct layout is unchanged
    assert [n for n, _ in benor.TrialsCfgC._fields_][5] == "crash_cut"      # ... crash_reach fills the same word
    assert benor.reach_word(0.0) == 0 and benor.reach_word(1.0) == ALL
    assert benor.reach_word(0.5) == HALF and benor.reach_word(0.25) == QUARTER
    with pytest.raises(ValueError):
        benor.kernel_for(10, 4, first(0, 10), mode=M7, crash_count=1, crash_window=2, crash_cut=3, crash_reach=HALF)
    with pytest.raises(ValueError):
        benor.kernel_for(10, 4, first(0, 10), mode=M7, crash_count=1, crash_window=2, crash_reach=ALL + 1)


EXTREME_SHAPES = [
    (10, 4, 0, None, dict(crash_at=at(10, {2: 1, 5: 2, 9: 3}))),
    (10, 4, 1, None, dict(crash_count=3, crash_window=6)),
    (12, 4, 0, [Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1, 0], dict(crash_at=at(12, {0: 0, 6: 1}))),
    (70, 24, 5, None, dict(crash_count=8, crash_window=5)),
]


@pytest.mark.parametrize("N,F,f,init,sched", EXTREME_SHAPES)
def test_reach_0_is_mode_5(N, F, f, init, sched):
    """Histogram bins, rounds and per-node states, trial by trial."""
    assert M7 == 7
    faulty = first(f, N)
    for t in range(150 if N < 20 else 25):
        assert subset_trial(N, F, faulty, SEED, t, 16, init, crash_reach=0, **sched) \
            == m5.crash_trial(N, F, faulty, SEED, t, 16, init, **sched), t


@pytest.mark.parametrize("N,F,f,init,sched", EXTREME_SHAPES)
def test_reach_all_is_mode_6_with_a_full_cut(N, F, f, init, sched):
    """... and through it mode 6's own even-step equivalence with mode 5."""
    assert M7 == 7
    faulty = first(f, N)
    killed = 0
    for t in range(150 if N < 20 else 25):
        got = subset_trial(N, F, faulty, SEED, t, 16, init, crash_reach=ALL, **sched)
        assert got == m6.partial_trial(N, F, faulty, SEED, t, 16, init, crash_cut=N - f, **sched), t
        killed += sum(s["killed"] for s in got[2]) - f
    assert killed > 0


@pytest.mark.parametrize("N,F,f", [(10, 4, 0), (11, 4, 2), (69, 24, 5)])
def test_empty_or_unreached_schedule_equals_mode_4(N, F, f):
    assert M7 == 7
    faulty, k_max = first(f, N), 16
    sched = at(N, {f: 2 * k_max, N - 1: 2 * k_max + 7}) if F - f >= 2 else at(N, {N - 1: 2 * k_max})
    for r in (0, HALF, ALL):
        for t in range(40):
            assert subset_trial(N, F, faulty, SEED, t, k_max, crash_at=sched, crash_reach=r) \
                == t3.tally3_trial(N, F, faulty, SEED, t, k_max), (r, t)
        assert subset_trial(N, F, faulty, SEED, 5, k_max, crash_reach=r) == t3.tally3_trial(N, F, faulty, SEED, 5, k_max)


def test_a_partial_reach_differs_from_both_ends():
    assert M7 == 7
    N, F, faulty, sched = 10, 4, first(0, 10), at(10, {3: 0, 8: 2})
    mid = [subset_trial(N, F, faulty, SEED, t, 16, crash_at=sched, crash_reach=HALF)[0] for t in range(300)]
    assert mid != [subset_trial(N, F, faulty, SEED, t, 16, crash_at=sched, crash_reach=0)[0] for t in range(300)]
    assert mid != [subset_trial(N, F, faulty, SEED, t, 16, crash_at=sched, crash_reach=ALL)[0] for t in range(300)]


def test_stream_9_word_depends_on_seed_trial_crasher_and_receiver_only():
    assert M7 == 7
    for trial in (0, 7, (1 << 32) + 5):
        for p in (0, 3, 4095):
            for c in (0, 1, 6, 4095):
                w = philox(SEED, (trial & 0xFFFFFFFF, trial >> 32, p | (c >> 2) << 12, STREAM_REACH << 24))[c & 3]
                assert (p | (c >> 2) << 12) < 1 << 22                       # the counter word fits
                for r in (1, w, w + 1, HALF, ALL - 1):
                    assert reach(SEED, trial, p, c, r) == (w < r)
                assert reach(SEED, trial, p, c, 0) is False and reach(SEED, trial, p, c, ALL) is True
    pattern = lambda seed, trial: [[reach(seed, trial, p, c, HALF) for c in range(12)] for p in range(12)]  # noqa: E731
    assert pattern(SEED, 0) == pattern(SEED, 0)
    assert pattern(SEED, 0) != pattern(SEED, 1) and pattern(SEED, 0) != pattern(SEED + 1, 0)
    assert pattern(SEED, 0) != pattern(SEED, 1 << 32)                       # the trial's high word counts
    rows = pattern(SEED, 0)
    assert len({tuple(r) for r in rows}) == 12                              # a pattern per crasher ...
    assert len({tuple(r[c] for r in rows) for c in range(12)}) == 12        # ... and per receiver


def test_the_reach_pattern_does_not_depend_on_the_schedule_order():
    """A trial's random schedule (drawn in Floyd's order) and the same schedule given explicitly (a list
    in node order) give the same trial: only (trial, p, c) enters a word, no position in a list."""
    assert M7 == 7
    N, F, f = 12, 4, 1
    faulty = first(f, N)
    live = [i for i in range(N) if not faulty[i]]
    for t in range(60):
        sched = schedule(SEED, t, live, None, 3, 5)
        explicit = at(N, {live[c]: s for c, s in enumerate(sched) if s is not None})
        assert sum(s is not None for s in explicit) == 3
        assert subset_trial(N, F, faulty, SEED, t, 16, crash_count=3, crash_window=5, crash_reach=HALF) \
            == subset_trial(N, F, faulty, SEED, t, 16, crash_at=explicit, crash_reach=HALF), t


def test_reach_frequency():
    """crash_reach = 2^30: the reach frequency over 20 * 20 * 256 = 102400 (p, c, trial) triples within
    5 sigma of 1/4, sigma = sqrt(n / 4 * 3 / 4) the binomial value."""
    assert M7 == 7
    n = hits = 0
    for trial in range(256):
        for p in range(20):
            for c in range(20):
                hits += reach(SEED, trial, 3 * p, 5 * c + 1, QUARTER)
                n += 1
    assert n >= 10 ** 5
    sigma = (n * 0.25 * 0.75) ** 0.5
    print(f"reach frequency {hits} / {n} = {hits / n:.5f}, sigma {sigma:.1f}")
    assert abs(hits - n / 4) < 5 * sigma, (hits, n, sigma)


def test_validation_and_kernel_choice():
    assert M7 == 7
    N, F = 10, 4
    none = first(0, N)
    S = benor.BO_KERNEL_TALLY_SUBSET
    for r in (0, 1, 5, 11, QUARTER, HALF, ALL - 1, ALL):    # every reach value is one
        assert benor.kernel_for(N, F, none, mode=M7, crash_count=3, crash_window=6, crash_reach=r) == S
        assert benor.kernel_for(N, F, none, mode=M7, crash_at=at(N, {3: 1}), crash_reach=r) == S
    assert benor.kernel_for(N, F, first(2, N), mode=M7, crash_count=2, crash_window=6, crash_reach=9) == S
    # mode 5's validation
    with pytest.raises(benor.Error, match="BO_MODE_CRASH_SUBSET needs at most F"):        # BO_ERR_FAULTY_COUNT
        benor.kernel_for(N, F, first(2, N), mode=M7, crash_count=3, crash_window=6, crash_reach=HALF)
    with pytest.raises(benor.Error, match="BO_MODE_CRASH_SUBSET needs at most F"):
        benor.kernel_for(N, F, none, mode=M7, crash_at=at(N, {i: 1 for i in range(5)}), crash_reach=HALF)
    with pytest.raises(RuntimeError, match="libbenor error 3.*crash_window"):
        benor.kernel_for(N, F, none, mode=M7, crash_count=3, crash_window=0, crash_reach=HALF)
    # an empty schedule is mode 4's plan
    for r in (0, HALF, ALL - 1, ALL):
        assert benor.kernel_for(N, F, none, mode=M7, crash_reach=r) == benor.BO_KERNEL_TALLY3
        assert benor.kernel_for(N, F, none, mode=M7, crash_at=at(N, {}), crash_reach=r) == benor.BO_KERNEL_TALLY3
        assert benor.kernel_for(11, 4, first(0, 11), mode=M7, crash_reach=r) == benor.BO_KERNEL_TALLY
    assert benor.kernel_for(3, 3, first(3, 3), mode=M7) == benor.BO_KERNEL_NONE
    # a non-empty one runs the subset kernel, reached or not
    assert benor.kernel_for(N, F, none, mode=M7, crash_at=at(N, {3: 10 ** 6}), crash_reach=HALF) == S
    assert benor.kernel_for(1024, 392, first(0, 1024), mode=M7, crash_count=392, crash_window=6, crash_reach=HALF) == S
    # mode 6 still reads the word as a cut: values in (m0, UINT32_MAX) are no cut
    assert benor.kernel_for(N, F, none, mode=M6, crash_count=3, crash_window=6, crash_cut=10) == benor.BO_KERNEL_TALLY_PARTIAL
    for cut in (11, HALF, ALL - 1):
        with pytest.raises(RuntimeError, match="libbenor error 3.*crash_cut"):
            benor.kernel_for(N, F, none, mode=M6, crash_count=3, crash_window=6, crash_cut=cut)
    # the other modes ignore the word
    assert benor.kernel_for(N, F, none, mode=M5, crash_count=3, crash_window=6, crash_reach=HALF) == benor.BO_KERNEL_TALLY_CRASH
    assert benor.kernel_for(N, F, none, mode=benor.BO_MODE_RANDOM_TALLY3, crash_reach=HALF) == benor.BO_KERNEL_TALLY3


def test_table_limit():
    """A table per m0 - j, j = 0 .. the scheduled crashes below step 2 k_max, at every reach; a table of
    (m', q) holds q (m' - q) thresholds of 8 bytes."""
    assert M7 == 7
    limit = 512 * MIB
    N, F = 4096, 1366
    q = N - F
    none = first(0, N)
    S = benor.BO_KERNEL_TALLY_SUBSET
    assert all(table_bytes(N - j, q) == 8 * q * (F - j) for j in (0, 1, 16, 32))
    t17 = sum(8 * q * (F - j) for j in range(17))
    t33 = sum(8 * q * (F - j) for j in range(33))
    assert 480 * MIB < t17 <= limit < t33
    assert 927 * MIB < t33 < 928 * MIB
    for r in (0, HALF, ALL):
        assert benor.kernel_for(N, F, none, mode=M7, crash_count=16, crash_window=4, crash_reach=r) == S
        assert benor.kernel_for(N, F, none, mode=M7, crash_at=at(N, {i: i % 2 for i in range(16)}), crash_reach=r) == S
        with pytest.raises(RuntimeError, match="libbenor error 7.*BO_MODE_CRASH_SUBSET.*512 MiB"):
            benor.kernel_for(N, F, none, mode=M7, crash_count=32, crash_window=4, crash_reach=r)
        with pytest.raises(RuntimeError, match="libbenor error 7.*512 MiB"):
            benor.kernel_for(N, F, none, mode=M7, crash_at=at(N, {i: i % 2 for i in range(32)}), crash_reach=r)
    # ... over the crashes below step 2 k_max only
    late = at(N, {i: (i % 2 if i < 16 else 1000) for i in range(32)})
    assert benor.kernel_for(N, F, none, mode=M7, crash_at=late, crash_reach=HALF, k_max=16) == S


LAW_SHAPES = {
    "even-quorum-steps-0-1-2": dict(N=10, F=4, f=0, init=None, sched=dict(crash_at=at(10, {2: 0, 5: 1, 9: 2}))),
    "odd-quorum-random-4-of-4": dict(N=11, F=4, f=0, init=None, sched=dict(crash_count=4, crash_window=4)),
    "question-marks-steps-0-0-1": dict(N=12, F=4, f=0, init=[Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1, 0],
                                       sched=dict(crash_at=at(12, {0: 0, 3: 0, 6: 1}))),
}
LAW_TRIALS, LAW_K_MAX = 20000, 16


@functools.lru_cache(maxsize=None)
def law_restatement(name, crash_reach):
    s = LAW_SHAPES[name]
    return subset_hist(s["N"], s["F"], first(s["f"], s["N"]), SEED, 0, LAW_TRIALS, LAW_K_MAX, s["init"],
                       crash_reach=crash_reach, **s["sched"])


@functools.lru_cache(maxsize=None)
def law_simulation(name, crash_reach):
    s = LAW_SHAPES[name]
    return mask_sim_hist(s["N"], s["F"], first(s["f"], s["N"]), LAW_K_MAX, LAW_TRIALS, np.random.default_rng(SEED + 1),
                         s["init"], crash_reach=crash_reach, **s["sched"])


@pytest.mark.parametrize("crash_reach", [HALF, QUARTER])
@pytest.mark.parametrize("name", sorted(LAW_SHAPES))
def test_law_matches_mask_level_simulation(name, crash_reach):
    """The restatement's histogram against the mask-level simulation, 2 * 10^4
    trials a side, k_max 16: two-sample chi^2 over bins pooled to >= 20,
    p > 10^-3 at fixed seeds."""
    assert M7 == 7
    got, ref = law_restatement(name, crash_reach), law_simulation(name, crash_reach)
    assert int(got[:-1].sum()) == LAW_TRIALS == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"{name}, reach {crash_reach / 2 ** 32}: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}, "
          f"agreement violations {int(got[-1])} / {int(ref[-1])}")
    assert p > 1e-3, (p, stat, df)


def test_the_gate_tells_reach_0_from_reach_one_half():
    """The same gate with the restatement at reach 0 against the simulation at reach 1/2 fails on at
    least one shape: it can see the reach."""
    assert M7 == 7
    ps = {}
    for name in sorted(LAW_SHAPES):
        ps[name] = chi2_two_sample(law_restatement(name, 0), law_simulation(name, HALF))[0]
        if ps[name] <= 1e-3:
            break                                           # one shape is enough (5 * 10^-34 on the first)
    print(ps)
    assert min(ps.values()) <= 1e-3, ps
