"""BO_MODE_CRASH_PARTIAL, crashes during the run that cut a broadcast short (CPU suite).

The definition, restated here in plain Python over
tests/test_crash_tally.py's schedule and tests/test_tally3.py's WordStream /
draw3 -- nothing from the kernel; tests/test_crash_partial_gpu.py checks the
kernel against it bit for bit.  It is BO_MODE_CRASH_TALLY's definition
(tests/test_crash_tally.py) with one change:

* Every scheduled crasher p has a cut, cut_p in [0, m0], counted over the
  initially-live nodes in ascending node id (the compact index).  crash_cut <= m0:
  every cut is that value.  crash_cut = CUT_RANDOM: cut_p = below(m0 + 1) from the
  word stream of the Philox blocks {trial_lo, trial_hi, c | b << 12, 8 << 24},
  b = 0, 1, .., c the crasher's compact index -- the multiply-shift with exact
  rejection of stream 6, from word 0.
* Step s: C_s = the alive nodes scheduled at s, A_s the alive set without them.
  p in C_s does not receive at step s; its step-s message (its x at an R-step,
  the proposal it formed at step s - 1 at a P-step) reaches exactly the
  receivers with compact index c < cut_p.  Receiver c in A_s draws draw3 with
  m = m_s + |H_c| and class sizes over A_s + H_c, H_c = {p in C_s : c < cut_p}.

The law is checked against a mask-level simulation written here with numpy
(explicit pools A_s + H_c and a uniform q-subset of each), which shares nothing
with the count-level argument.
"""
import numpy as np
import pytest

import benor
import oracle
import test_crash_tally as m5
import test_tally3 as t3
from test_crash_tally import at, schedule, table_bytes
from test_tally import chi2_two_sample, first, philox
from test_tally3 import Q, WordStream, draw3

M5 = benor.BO_MODE_CRASH_TALLY
M6 = getattr(benor, "BO_MODE_CRASH_PARTIAL", None)          # absent before the mode: every test fails
RANDOM = 0xFFFFFFFF
STREAM_TALLY, STREAM_CUT = 5, 8
SEED = t3.SEED
MIB = 1 << 20


# ------------------------------------------------------------ restatement
def cut_of(seed, trial, c, m0, crash_cut):
    """Crasher c's cut: the plan's, or one draw below m0 + 1 from stream 8."""
    if crash_cut != RANDOM:
        return crash_cut
    return WordStream(seed, trial & 0xFFFFFFFF, trial >> 32, c, STREAM_CUT << 24).below(m0 + 1)


def partial_trial(N, F, faulty, seed, trial, k_max, initial_values=None, crash_at=None, crash_count=0, crash_window=0,
                  crash_cut=0):
    """One trial: (histogram bins it increments, rounds, per-node states)."""
    live = [i for i in range(N) if not faulty[i]]
    m0, q = len(live), N - F
    states = [{"killed": True, "x": None, "decided": None, "k": None} if faulty[i] else None for i in range(N)]
    if m0 == 0:
        return [2], 0, states
    assert crash_cut == RANDOM or 0 <= crash_cut <= m0
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
        cuts = {p: cut_of(seed, trial, p, m0, crash_cut) for p in C}
        A = [c for c in range(m0) if alive[c]]
        if not A:
            return None
        assert len(A) >= q
        out, sizes = {}, {}
        for c in A:
            H = tuple(p for p in C if c < cuts[p])
            if H not in sizes:                             # the class sizes over the pool A + H
                sizes[H] = tuple(sum(vals[a] == v for a in A + list(H)) for v in (0, 1, 2))
            b = blocks[c]
            u = b[1] << 32 | b[0] if phase == 0 else b[3] << 32 | b[2]
            out[c] = draw3(len(A) + len(H), q, sizes[H], seed, trial, c, r, phase, u)
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


def partial_hist(N, F, faulty, seed, trial_begin, trial_count, k_max, initial_values=None, **sched):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in partial_trial(N, F, faulty, seed, t, k_max, initial_values, **sched)[0]:
            h[b] += 1
    return h


# ------------------------------------------- mask-level simulation (numpy)
def mask_sim_hist(N, F, faulty, k_max, trials, rng, initial_values=None, crash_at=None, crash_count=0,
                  crash_window=0, crash_cut=0, chunk=10000):
    """The same model at the level of inboxes: at every step each alive receiver c
    hears a uniform q-subset (the q smallest of iid uniform keys) of its pool,
    the alive senders and the step's crashers whose cut is above c, drawn
    explicitly; schedules, cuts, initial values and coins from `rng`."""
    live = [i for i in range(N) if not faulty[i]]
    m0, q = len(live), N - F
    hist = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    never = 1 << 30
    recv = np.arange(m0)[None, :, None]

    def counts(vals, alive, going, cut):
        n = len(vals)
        if q == 0:
            return np.zeros((n, m0), dtype=np.int64), np.zeros((n, m0), dtype=np.int64)
        pool = alive[:, None, :] | (going[:, None, :] & (recv < cut[:, None, :]))   # [trial, receiver, sender]
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
        if crash_cut == RANDOM:
            cut = rng.integers(0, m0 + 1, size=(n, m0))
        else:
            cut = np.full((n, m0), crash_cut, dtype=np.int64)
        alive = np.ones((n, m0), dtype=bool)
        dec = np.zeros((n, m0), dtype=bool)
        if m0 == 0:
            hist[2] += n
            continue
        for r in range(1, k_max + 1):
            going = alive & (sched == 2 * (r - 1))
            alive &= ~going
            gone = ~alive.any(axis=1)
            c0, c1 = counts(x, alive, going, cut)
            prop = np.where(c0 > c1, 0, np.where(c1 > c0, 1, 2)).astype(np.int8)
            going = alive & (sched == 2 * (r - 1) + 1)
            alive &= ~going
            gone |= ~alive.any(axis=1)
            c0, c1 = counts(prop, alive, going, cut)
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
            x, alive, dec, sched, cut = x[keep], alive[keep], dec[keep], sched[keep], cut[keep]
            if not len(x):
                break
    return hist


# ---------------------------------------------------------------- the tests
def test_the_mode_exists():
    assert M6 == 6 and benor.CUT_RANDOM == RANDOM
    assert benor.BO_KERNEL_TALLY_PARTIAL == 12 and benor.BO_KERNEL_TALLY_PARTIAL in benor.KERNEL_NAMES
    assert benor.lib().bo_abi_version() == 8                # the struct layout is unchanged
    assert [n for n, _ in benor.TrialsCfgC._fields_][5] == "crash_cut"


@pytest.mark.parametrize("N,F,f", [(10, 4, 0), (11, 4, 2), (69, 24, 5)])
def test_empty_or_unreached_schedule_equals_mode_4(N, F, f):
    assert M6 == 6
    faulty, k_max = first(f, N), 16
    sched = at(N, {f: 2 * k_max, N - 1: 2 * k_max + 7}) if F - f >= 2 else at(N, {N - 1: 2 * k_max})
    for cut in (0, N - f, RANDOM):
        for t in range(60):
            assert partial_trial(N, F, faulty, SEED, t, k_max, crash_at=sched, crash_cut=cut) \
                == t3.tally3_trial(N, F, faulty, SEED, t, k_max), (cut, t)
        assert partial_trial(N, F, faulty, SEED, 5, k_max, crash_cut=cut) == t3.tally3_trial(N, F, faulty, SEED, 5, k_max)


@pytest.mark.parametrize("N,F,f,init,sched", [
    (10, 4, 0, None, dict(crash_at=at(10, {2: 1, 5: 2, 9: 3}))),
    (10, 4, 1, None, dict(crash_count=3, crash_window=6)),
    (12, 4, 0, [Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1, 0], dict(crash_at=at(12, {0: 0, 6: 1}))),
    (69, 24, 5, None, dict(crash_count=8, crash_window=5)),
])
def test_cut_0_is_mode_5(N, F, f, init, sched):
    assert M6 == 6
    faulty = first(f, N)
    for t in range(150 if N < 20 else 25):
        assert partial_trial(N, F, faulty, SEED, t, 16, init, crash_cut=0, **sched) \
            == m5.crash_trial(N, F, faulty, SEED, t, 16, init, **sched), t


@pytest.mark.parametrize("N,F,f,init,steps", [
    (10, 4, 0, None, {3: 0}),
    (10, 4, 1, None, {2: 0, 5: 2, 9: 2}),
    (12, 4, 0, [Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1, 0], {0: 0, 6: 2, 7: 4}),
    (69, 24, 5, None, {6 + 7 * i: 2 * (i % 3) for i in range(9)}),
])
def test_even_steps_with_a_full_cut_are_mode_5_one_step_later(N, F, f, init, steps):
    """The crasher's x reaches everyone at the R-step; crashing at the P-step instead it
    also proposes, but it does not vote, and its x, decided and k as of the crash agree."""
    assert M6 == 6
    faulty = first(f, N)
    later = {i: s + 1 for i, s in steps.items()}
    reached = 0
    for t in range(150 if N < 20 else 25):
        got = partial_trial(N, F, faulty, SEED, t, 16, init, crash_at=at(N, steps), crash_cut=N - f)
        assert got == m5.crash_trial(N, F, faulty, SEED, t, 16, init, crash_at=at(N, later)), t
        reached += sum(s["killed"] for s in got[2]) - f
    assert reached > 0


def test_a_partial_cut_differs_from_both_ends():
    """A cut strictly inside (0, m0) is neither mode 5 nor mode 5 one step later somewhere."""
    assert M6 == 6
    N, F, faulty, sched = 10, 4, first(0, 10), at(10, {3: 0, 8: 2})
    mid = [partial_trial(N, F, faulty, SEED, t, 16, crash_at=sched, crash_cut=5)[0] for t in range(300)]
    assert mid != [partial_trial(N, F, faulty, SEED, t, 16, crash_at=sched, crash_cut=0)[0] for t in range(300)]
    assert mid != [partial_trial(N, F, faulty, SEED, t, 16, crash_at=sched, crash_cut=10)[0] for t in range(300)]


def test_stream_8_cut_depends_on_seed_trial_and_compact_index_only():
    assert M6 == 6
    m0 = 12
    for trial in (0, 7, (1 << 32) + 5):
        for c in (0, 3, 11):
            w = philox(SEED, (trial & 0xFFFFFFFF, trial >> 32, c, STREAM_CUT << 24))[0]
            if (w * (m0 + 1) & 0xFFFFFFFF) >= (2 ** 32 - (m0 + 1)) % (m0 + 1):      # word 0 accepted
                assert cut_of(SEED, trial, c, m0, RANDOM) == w * (m0 + 1) >> 32
            assert cut_of(SEED, trial, c, m0, RANDOM) == cut_of(SEED, trial, c, m0, RANDOM)
            assert cut_of(SEED, trial, c, m0, 7) == 7
    cuts = [[cut_of(SEED, t, c, m0, RANDOM) for c in range(m0)] for t in range(400)]
    assert all(0 <= v <= m0 for row in cuts for v in row)
    assert len({tuple(r) for r in cuts}) == 400             # a draw per trial ...
    assert all(len({r[c] for r in cuts}) == m0 + 1 for c in range(m0))      # ... and every cut 0..m0 occurs
    assert cuts[0] != [cut_of(SEED + 1, 0, c, m0, RANDOM) for c in range(m0)]
    hits = np.bincount(np.array(cuts).ravel(), minlength=m0 + 1)
    assert all(abs(h - 4800 / 13) < 5 * 18.5 for h in hits), hits         # Binomial(4800, 1/13): sd 18.5


def test_validation_and_kernel_choice():
    assert M6 == 6
    N, F = 10, 4
    none = first(0, N)
    P = benor.BO_KERNEL_TALLY_PARTIAL
    for cut in (0, 5, 10, RANDOM):
        assert benor.kernel_for(N, F, none, mode=M6, crash_count=3, crash_window=6, crash_cut=cut) == P
        assert benor.kernel_for(N, F, none, mode=M6, crash_at=at(N, {3: 1}), crash_cut=cut) == P
    assert benor.kernel_for(N, F, first(2, N), mode=M6, crash_count=2, crash_window=6, crash_cut=8) == P   # m0 = 8
    with pytest.raises(RuntimeError, match="libbenor error 3.*crash_cut"):
        benor.kernel_for(N, F, first(2, N), mode=M6, crash_count=2, crash_window=6, crash_cut=9)
    with pytest.raises(RuntimeError, match="libbenor error 3.*crash_cut"):
        benor.kernel_for(N, F, none, mode=M6, crash_count=2, crash_window=6, crash_cut=RANDOM - 1)
    with pytest.raises(RuntimeError, match="libbenor error 3.*crash_cut"):                # ... an empty schedule too
        benor.kernel_for(N, F, none, mode=M6, crash_cut=11)
    # mode 5's validation
    with pytest.raises(benor.Error):
        benor.kernel_for(N, F, first(2, N), mode=M6, crash_count=3, crash_window=6)
    with pytest.raises(RuntimeError, match="libbenor error 3.*crash_window"):
        benor.kernel_for(N, F, none, mode=M6, crash_count=3, crash_window=0)
    # an empty schedule is mode 4's plan
    assert benor.kernel_for(N, F, none, mode=M6, crash_cut=RANDOM) == benor.BO_KERNEL_TALLY3
    assert benor.kernel_for(N, F, none, mode=M6, crash_at=at(N, {}), crash_cut=3) == benor.BO_KERNEL_TALLY3
    assert benor.kernel_for(11, 4, first(0, 11), mode=M6) == benor.BO_KERNEL_TALLY
    assert benor.kernel_for(3, 3, first(3, 3), mode=M6) == benor.BO_KERNEL_NONE
    # a non-empty one runs the partial kernel, reached or not
    assert benor.kernel_for(N, F, none, mode=M6, crash_at=at(N, {3: 10 ** 6}), crash_cut=RANDOM) == P
    assert benor.kernel_for(1024, 392, first(0, 1024), mode=M6, crash_count=392, crash_window=6, crash_cut=RANDOM) == P
    # the other modes ignore the field
    assert benor.kernel_for(N, F, none, mode=M5, crash_count=3, crash_window=6, crash_cut=77) == benor.BO_KERNEL_TALLY_CRASH
    assert benor.kernel_for(N, F, none, mode=benor.BO_MODE_RANDOM_TALLY3, crash_cut=77) == benor.BO_KERNEL_TALLY3


def test_table_limit():
    """One table per pool size; a table of (m', q) holds q (m' - q) thresholds of 8 bytes."""
    assert M6 == 6
    limit = 512 * MIB
    N, F = 4096, 1366
    q = N - F
    none = first(0, N)
    P = benor.BO_KERNEL_TALLY_PARTIAL
    assert all(table_bytes(N - j, q) == 8 * q * (F - j) for j in (0, 1, 16, 32))
    t3_ = sum(8 * q * (F - j) for j in (0, 16, 32))          # 32 crashes at two steps, a fixed cut: mode 5's three
    t17 = sum(8 * q * (F - j) for j in range(17))
    t33 = sum(8 * q * (F - j) for j in range(33))
    assert 84 * MIB < t3_ < 85 * MIB and 480 * MIB < t17 <= limit
    assert 927 * MIB < t33 < 928 * MIB                      # 33 tables: 8 * 2730 * 44550 bytes = 927.9 MiB
    two_steps = at(N, {i: i % 2 for i in range(32)})
    # a fixed cut with an explicit schedule needs no more tables than mode 5: pools m_s and m_s + |C_s|
    assert benor.kernel_for(N, F, none, mode=M5, crash_at=two_steps) == benor.BO_KERNEL_TALLY_CRASH
    for cut in (0, 1000, N):
        assert benor.kernel_for(N, F, none, mode=M6, crash_at=two_steps, crash_cut=cut) == P
    # random cuts: any number of a step's crashers may reach a receiver, every m0 - j
    with pytest.raises(RuntimeError, match="libbenor error 7.*512 MiB"):
        benor.kernel_for(N, F, none, mode=M6, crash_at=two_steps, crash_cut=RANDOM)
    # ... over the crashes below step 2 k_max only
    late = at(N, {i: (i % 2 if i < 16 else 1000) for i in range(32)})
    assert benor.kernel_for(N, F, none, mode=M6, crash_at=late, crash_cut=RANDOM, k_max=16) == P
    # a random schedule already has every m0 - j
    assert benor.kernel_for(N, F, none, mode=M6, crash_count=16, crash_window=4, crash_cut=RANDOM) == P
    with pytest.raises(RuntimeError, match="libbenor error 7.*512 MiB"):
        benor.kernel_for(N, F, none, mode=M6, crash_count=32, crash_window=4, crash_cut=5)


LAW_SHAPES = {
    "steps-1-2-3-random-cuts": dict(N=10, F=4, f=0, init=None, seed=SEED + 1,
                                    sched=dict(crash_at=at(10, {2: 1, 5: 2, 9: 3}), crash_cut=RANDOM)),
    "random-3-of-6-cut-4": dict(N=10, F=4, f=1, init=None, seed=SEED + 1,
                                sched=dict(crash_count=3, crash_window=6, crash_cut=4)),
    "question-marks-random-cuts": dict(N=12, F=4, f=0, init=[Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1, 0], seed=SEED + 1,
                                       sched=dict(crash_at=at(12, {0: 0, 6: 1}), crash_cut=RANDOM)),
}


@pytest.mark.parametrize("name", sorted(LAW_SHAPES))
def test_law_matches_mask_level_simulation(name):
    """The restatement's histogram against the mask-level simulation, 2 * 10^4
    trials a side, k_max 16: two-sample chi^2 over bins pooled to >= 20,
    p > 10^-3 at fixed seeds."""
    assert M6 == 6
    s = LAW_SHAPES[name]
    N, F, T, k_max = s["N"], s["F"], 20000, 16
    faulty = first(s["f"], N)
    ref = mask_sim_hist(N, F, faulty, k_max, T, np.random.default_rng(s["seed"]), s["init"], **s["sched"])
    got = partial_hist(N, F, faulty, SEED, 0, T, k_max, s["init"], **s["sched"])
    assert int(got[:-1].sum()) == T == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"{name}: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}, agreement violations {int(got[-1])} / {int(ref[-1])}")
    assert p > 1e-3, (p, stat, df)
