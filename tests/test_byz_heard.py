"""BO_BYZ_BALANCE and BO_BYZ_SPLIT: Byzantine senders that see each receiver's inbox (CPU suite).

Two strategies of BO_MODE_BYZ_TALLY (include/benor.h), restated here in
plain Python over test_tally3.draw3 and its WordStream, test_tally.philox,
oracle.random_init and oracle.coin -- nothing from the kernel;
tests/test_byz_heard_gpu.py checks the kernel against it bit for bit.  Who is
Byzantine, f + b <= F, compact indices, senders and receivers, rule, coins, k, halting
over the honest nodes, the histogram and the per-node states are mode 8's
(tests/test_byz_tally.py).  What differs is the draw, two stages per (receiver c,
round r, phase), with (H0, H1, Hq) the honest senders' class sizes at the step:

* Stage 1: (h0, h1) = test_tally3.draw3 among m senders with the class sizes
  (H0, H1, Hq + b), from c's stream-5 uniform and stream-6 walk as in mode 4;
  rest = q - h0 - h1 messages come from the merged class of Hq + b senders.
* Stage 2: nB ~ Hypergeometric(Hq + b, b, rest) of them are Byzantine.  Hq = 0: nB =
  rest; rest = 0: nB = 0; neither draws.  Else selection sampling over the smaller
  sub-class (KW = min(b, Hq), the Byzantine one on a tie): member i is in the inbox iff
  v_i < rest - taken, v_i uniform below Hq + b - i (draw3's multiply-shift with exact
  rejection) from the word stream of blocks {trial_lo, trial_hi, c | blk << 12,
  (r - 1) | phase << 16 | 11 << 24}, blk = 0, 1, ..; nB is the number taken if the
  Byzantine class was walked, else rest minus it.
* The nB liars see (h0, h1); l1 of them say 1, the others 0:
    BYZ_BALANCE  d = h0 + nB - h1; l1 = 0 if d <= 0, else min(nB, d // 2);
    BYZ_SPLIT    l1 = nB if c is odd, else 0.
  (c0, c1) = (h0 + nB - l1, h1 + l1).  byz_one is not read.
"""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import benor
import oracle
import test_byz_tally as mode8
import test_tally3
from test_tally import chi2_two_sample, first, philox
from test_tally3 import WordStream, draw3

M8 = getattr(benor, "BO_MODE_BYZ_TALLY", None)
BYZ = getattr(benor, "BO_KERNEL_TALLY_BYZ", None)
BALANCE = getattr(benor, "BO_BYZ_BALANCE", None)             # absent before the strategies: every test fails
SPLIT = getattr(benor, "BO_BYZ_SPLIT", None)
RANDOM = mode8.RANDOM
STREAM_TALLY, STREAM_HEARD = 5, 11
SEED = mode8.SEED
HALF, ALL = mode8.HALF, mode8.ALL
Q = "?"
marks = mode8.marks


def strategies_exist():
    assert (BALANCE, SPLIT) == (3, 4)


# ------------------------------------------------------------ restatement
def heard_byz(Hq, b, rest, seed, trial, c, r, phase):
    """Stage 2: how many of the `rest` messages from the merged class are Byzantine."""
    if Hq == 0:
        return rest
    if rest == 0:
        return 0
    walk_byz = b <= Hq
    ws = WordStream(seed, trial & 0xFFFFFFFF, trial >> 32, c, (r - 1) | phase << 16 | STREAM_HEARD << 24)
    taken = 0
    for i in range(b if walk_byz else Hq):
        if ws.below(Hq + b - i) < rest - taken:
            taken += 1
    return taken if walk_byz else rest - taken


def heard_lies(strategy, c, h0, h1, nB):
    """l1: how many of the nB Byzantine messages in receiver c's inbox say 1."""
    if strategy == SPLIT:
        return nB if c % 2 else 0
    assert strategy == BALANCE
    d = h0 + nB - h1
    return 0 if d <= 0 else min(nB, d // 2)


def heard_trial(N, F, faulty, byzantine, seed, trial, k_max, initial_values=None, byz_one=0, byz_strategy=None):
    """One trial: (histogram bins it increments, rounds, per-node states).  byz_one is not read."""
    strategies_exist()
    live = [i for i in range(N) if not faulty[i]]
    honest = [c for c, i in enumerate(live) if not byzantine[i]]
    m, q, b = len(live), N - F, len(live) - len(honest)
    assert not any(faulty[i] and byzantine[i] for i in range(N)) and (N - m) + b <= F
    states = [{"killed": bool(faulty[i]), "x": None, "decided": None, "k": None} for i in range(N)]
    if not honest:
        return [2], 0, states
    if initial_values is None:
        x = {c: oracle.random_init(seed, trial, c, m) for c in honest}
    else:
        x = {c: 2 if initial_values[live[c]] == Q else initial_values[live[c]] for c in honest}
    dec = {c: False for c in honest}
    tlo, thi = trial & 0xFFFFFFFF, trial >> 32
    R = 0
    for r in range(1, k_max + 1):
        blocks = {c: philox(seed, (tlo, thi, c, (r - 1) | STREAM_TALLY << 24)) for c in honest}

        def sizes(vals):
            return [sum(1 for v in vals.values() if v == k) for k in (0, 1, 2)]

        def counts(H, c, phase):
            s = blocks[c]
            h0, h1 = draw3(m, q, (H[0], H[1], H[2] + b), seed, trial, c, r, phase,
                           s[3] << 32 | s[2] if phase else s[1] << 32 | s[0])
            nB = heard_byz(H[2], b, q - h0 - h1, seed, trial, c, r, phase)
            assert max(0, q - h0 - h1 - H[2]) <= nB <= min(b, q - h0 - h1)
            l1 = heard_lies(byz_strategy, c, h0, h1, nB)
            return h0 + nB - l1, h1 + l1

        prop, H = {}, sizes(x)
        for c in honest:
            c0, c1 = counts(H, c, 0)
            prop[c] = 0 if c0 > c1 else 1 if c1 > c0 else 2
        new, H = {}, sizes(prop)
        for c in honest:
            c0, c1 = counts(H, c, 1)
            if c0 > F:
                new[c], dec[c] = 0, True
            elif c1 > F:
                new[c], dec[c] = 1, True
            elif c0 != c1:
                new[c] = 1 if c1 > c0 else 0
            else:
                new[c] = oracle.coin(seed, trial, c, r)
        x = new
        R = r
        if all(dec.values()):
            break
    ones = sum(x.values())
    v = 2 if 0 < ones < len(honest) else (1 if ones else 0)
    all_dec = all(dec.values())
    bins = [R * 3 + v] if all_dec else [v]
    if all_dec and v == 2:
        bins.append((k_max + 1) * 3)
    for c in honest:
        states[live[c]] = {"killed": False, "x": x[c], "decided": dec[c], "k": R + 1}
    return bins, (R if all_dec else 0), states


def heard_hist(N, F, faulty, byzantine, seed, trial_begin, trial_count, k_max, initial_values=None, **lie):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in heard_trial(N, F, faulty, byzantine, seed, t, k_max, initial_values, **lie)[0]:
            h[b] += 1
    return h


# ------------------------------------------------- mask-level simulation
def mask_sim_hist(N, F, byzantine, k_max, trials, rng, strategy, initial_values=None, chunk=10000):
    """The same model at the level of inboxes (f = 0): at every step each honest receiver
    hears an explicit uniform q-subset of the m senders (the q smallest of iid uniform
    keys); the Byzantine senders inside it read the honest messages beside them in that
    very inbox and then choose what to say.  Initial values (unless given), inboxes and
    coins from `rng`."""
    is_byz = np.array([bool(v) for v in byzantine])
    m, q = N, N - F
    odd = (np.arange(m) % 2 == 1)[None, :]
    hist = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)

    def counts(vals):
        n = len(vals)
        inbox = np.argpartition(rng.random((n, m, m)), q - 1, axis=2)[:, :, :q]        # [trial, receiver, slot] -> sender
        got = np.take_along_axis(np.broadcast_to(vals[:, None, :], (n, m, m)), inbox, axis=2)
        liar = is_byz[inbox]
        h0 = ((got == 0) & ~liar).sum(axis=2)
        h1 = ((got == 1) & ~liar).sum(axis=2)
        nB = liar.sum(axis=2)
        if strategy == SPLIT:
            l1 = np.where(odd, nB, 0)
        else:
            d = h0 + nB - h1
            l1 = np.where(d <= 0, 0, np.minimum(nB, d // 2))
        return h0 + nB - l1, h1 + l1

    def finish(x, dec, R):
        ones = ((x == 1) & ~is_byz).sum(axis=1)
        v = np.where((ones > 0) & (ones < (~is_byz).sum()), 2, np.where(ones > 0, 1, 0))
        all_dec = (dec | is_byz).all(axis=1)
        np.add.at(hist, np.where(all_dec, R * 3 + v, v), 1)
        hist[-1] += int((all_dec & (v == 2)).sum())

    for lo in range(0, trials, chunk):
        n = min(chunk, trials - lo)
        if initial_values is None:
            x = rng.integers(0, 2, size=(n, m)).astype(np.int8)
        else:
            x = np.tile(np.array([2 if v == Q else v for v in initial_values], dtype=np.int8), (n, 1))
        dec = np.zeros((n, m), dtype=bool)
        for r in range(1, k_max + 1):
            c0, c1 = counts(x)
            prop = np.where(c0 > c1, 0, np.where(c1 > c0, 1, 2)).astype(np.int8)
            c0, c1 = counts(prop)
            coin = rng.integers(0, 2, size=(len(x), m))
            x = np.where(c0 > F, 0, np.where(c1 > F, 1, np.where(c1 > c0, 1, np.where(c0 > c1, 0, coin)))).astype(np.int8)
            dec |= (c0 > F) | (c1 > F)
            halted = (dec | is_byz).all(axis=1)
            if r == k_max:
                halted[:] = True
            finish(x[halted], dec[halted], r)
            x, dec = x[~halted], dec[~halted]
            if not len(x):
                break
    return hist


# ------------------------------------------------- shared restatement runs
T_LAW, K_MAX = 1500, 16
INIT_12 = [Q, 1, 0, Q, 1, Q, 0, 1, Q, 0, Q, 1]               # six "?", two of them (nodes 0 and 3) liars'
SHAPES = {"10,4,2": (10, 4, {2, 7}, None), "10,4,4": (10, 4, {0, 4, 5, 9}, None), "12,4,4?": (12, 4, {0, 3, 6, 9}, INIT_12)}


@functools.lru_cache(maxsize=None)
def shared_hist(shape, strategy):
    """1500 trials from trial 0, k_max 16, f = 0: computed once, read by the law and the effect tests."""
    N, F, ids, init = SHAPES[shape]
    if strategy == "random":
        h = mode8.byz_hist(N, F, first(0, N), marks(ids, N), SEED, 0, T_LAW, K_MAX, init, byz_one=HALF, byz_strategy=RANDOM)
    else:
        h = heard_hist(N, F, first(0, N), marks(ids, N), SEED, 0, T_LAW, K_MAX, init, byz_strategy=strategy)
    h.setflags(write=False)
    return h


def undecided(h):
    return int(h[:3].sum())


def mean_rounds(h, k_max=K_MAX):
    """Rounds per trial, k_max for an undecided one."""
    n = sum(R * int(h[R * 3:R * 3 + 3].sum()) for R in range(1, k_max + 1)) + k_max * undecided(h)
    return n / int(h[:-1].sum())


# ---------------------------------------------------------------- the tests
def test_the_strategies_exist():
    strategies_exist()
    assert (benor.BYZ_BALANCE, benor.BYZ_SPLIT) == (3, 4)
    assert benor.lib().bo_abi_version() == 8                # the struct layout is unchanged


def test_validation_and_kernel_choice():
    """Through bo_kernel_for: no device needed."""
    strategies_exist()
    one = dict(mode=M8, byz_one=HALF)
    for bad in (2, 5, 6, 0xFFFFFFFF):                        # 2 was invalid before these strategies and stays so
        with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}"):
            benor.kernel_for(10, 4, first(0, 10), byzantine=marks({1}, 10), byz_strategy=bad, **one)
    for strategy in (BALANCE, SPLIT):
        for w in (0, HALF, ALL):                             # every byz_one is valid
            kw = dict(mode=M8, byz_one=w, byz_strategy=strategy)
            for N, F, f, ids in ((10, 4, 0, {0}), (10, 4, 2, {5, 6}), (11, 4, 0, {3, 9}),
                                 (1024, 340, 0, set(range(0, 1000, 10))), (4096, 1366, 0, {7})):
                assert benor.kernel_for(N, F, first(f, N), byzantine=marks(ids, N), **kw) == BYZ
            with pytest.raises(benor.Error, match="at most F nodes crashed or Byzantine"):
                benor.kernel_for(10, 4, first(2, 10), byzantine=marks({5, 6, 7}, 10), **kw)
            # b = 0 is mode 4's plan
            assert benor.kernel_for(10, 4, first(0, 10), byzantine=marks(set(), 10), **kw) == benor.BO_KERNEL_TALLY3
            assert benor.kernel_for(11, 4, first(0, 11), byzantine=marks(set(), 11), **kw) == benor.BO_KERNEL_TALLY


@pytest.mark.parametrize("name", ["BALANCE", "SPLIT"])
def test_restatement_without_byzantine_nodes_is_mode_4(name):
    strategies_exist()
    strategy = {"BALANCE": BALANCE, "SPLIT": SPLIT}[name]
    for N, F, f, init in ((10, 4, 0, None), (10, 4, 2, None), (11, 4, 1, None), (10, 4, 0, test_tally3.INIT_10)):
        got = heard_hist(N, F, first(f, N), marks(set(), N), SEED, 0, 300, 16, init, byz_strategy=strategy)
        assert np.array_equal(got, test_tally3.tally3_hist(N, F, first(f, N), SEED, 0, 300, 16, init))


@pytest.mark.parametrize("name", ["BALANCE", "SPLIT"])
def test_byz_one_is_not_read(name):
    strategies_exist()
    strategy = {"BALANCE": BALANCE, "SPLIT": SPLIT}[name]
    N, F, byz = 12, 4, marks({0, 3, 6, 9}, 12)
    a = heard_hist(N, F, first(0, N), byz, SEED, 0, 200, 16, INIT_12, byz_one=0, byz_strategy=strategy)
    c = heard_hist(N, F, first(0, N), byz, SEED, 0, 200, 16, INIT_12, byz_one=ALL, byz_strategy=strategy)
    assert np.array_equal(a, c) and int(a[:-1].sum()) == 200


@pytest.mark.parametrize("Hq,b,rest", [(5, 2, 3), (3, 3, 4), (2, 5, 4), (6, 1, 6), (1, 4, 2)])
def test_stage_2_is_hypergeometric(Hq, b, rest):
    """The walk's nB over 24 000 receivers (compact indices 0..3999 of six trials, round 3, both
    phases alternating) covers exactly the support max(0, rest - Hq) .. min(b, rest) of
    Hypergeometric(Hq + b, b, rest), and its counts pass the two-sample chi^2 against the exact
    pmf (Fractions) scaled to 10^7 draws, p > 10^-3 as the tally tests.  b < Hq walks the
    Byzantine class, b = Hq too (the tie), b > Hq the honest "?" one."""
    strategies_exist()
    lo, hi = max(0, rest - Hq), min(b, rest)
    got = np.zeros(b + 2, dtype=np.uint64)                   # (a last bin that chi2_two_sample leaves out)
    for t in range(6):
        for c in range(4000):
            got[heard_byz(Hq, b, rest, SEED, (1 << 33) + t, c, 3, c & 1)] += 1
    assert [k for k in range(b + 1) if got[k]] == list(range(lo, hi + 1))
    pmf = [Fraction(math.comb(b, k) * math.comb(Hq, rest - k), math.comb(Hq + b, rest)) if lo <= k <= hi else Fraction(0)
           for k in range(b + 1)]
    assert sum(pmf) == 1
    ref = np.array([round(p * 10 ** 7) for p in pmf] + [0], dtype=np.uint64)
    p, stat, df = chi2_two_sample(got, ref)
    print(f"(Hq, b, rest) = ({Hq}, {b}, {rest}): counts {[int(v) for v in got[:-1]]}, chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}")
    assert p > 1e-3, (p, stat, df)


def test_stage_2_draws_nothing_at_its_edges():
    strategies_exist()
    assert heard_byz(0, 4, 3, SEED, 0, 1, 1, 0) == 3          # no honest "?": the rest is Byzantine
    assert heard_byz(5, 4, 0, SEED, 0, 1, 1, 0) == 0
    assert heard_byz(5, 0, 3, SEED, 0, 1, 1, 0) == 0          # b = 0: an empty walk
    assert heard_byz(2, 3, 5, SEED, 0, 1, 1, 1) == 3          # the whole merged class is in the inbox
    assert [heard_lies(BALANCE, 0, h0, h1, nB) for h0, h1, nB in ((3, 3, 0), (1, 5, 2), (3, 3, 2), (3, 2, 3), (6, 0, 2), (0, 0, 5))] \
        == [0, 0, 1, 2, 2, 2]
    assert [heard_lies(SPLIT, c, 2, 1, 3) for c in (0, 1, 2, 7)] == [0, 3, 0, 3]


@pytest.mark.parametrize("name", ["BALANCE", "SPLIT"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_law_matches_the_mask_level_simulation(shape, name):
    """The restatement's histogram (1500 trials) against the mask-level simulation (2 * 10^4
    trials, explicit q-subsets, liars that read the actual inbox), k_max 16: two-sample chi^2
    over bins pooled to >= 20, p > 10^-3 at fixed seeds."""
    strategies_exist()
    strategy = {"BALANCE": BALANCE, "SPLIT": SPLIT}[name]
    N, F, ids, init = SHAPES[shape]
    got = shared_hist(shape, strategy)
    ref = mask_sim_hist(N, F, marks(ids, N), K_MAX, 20000, np.random.default_rng(SEED + 2), strategy, init)
    assert int(got[:-1].sum()) == T_LAW and int(ref[:-1].sum()) == 20000
    p, stat, df = chi2_two_sample(got, ref)
    print(f"({shape}) {name}: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}; violations {int(got[-1])} of {T_LAW} (restatement) / "
          f"{int(ref[-1])} of 20000 (simulation); undecided {undecided(got)} / {undecided(ref)}; "
          f"mean rounds {mean_rounds(got):.2f} / {mean_rounds(ref):.2f}")
    assert p > 1e-3, (p, stat, df)


@pytest.mark.parametrize("name", ["BALANCE", "SPLIT"])
def test_three_liars_cannot_move_unanimous_ones(name):
    """N = 10, F = 3, b = 3, every honest node starts at 1: q = 7 and nB <= 3, so a receiver hears
    h1 = 7 - nB >= 4 honest ones and no honest zero; under either strategy c1 >= h1 >= 4 > c0 (at
    most 3) and c1 >= 4 > F in both phases: every trial decides 1 in round 1."""
    strategies_exist()
    strategy = {"BALANCE": BALANCE, "SPLIT": SPLIT}[name]
    N, F, byz = 10, 3, marks({1, 4, 8}, 10)
    h = heard_hist(N, F, first(0, N), byz, SEED, 0, 300, 16, [1] * N, byz_strategy=strategy)
    assert int(h[1 * 3 + 1]) == 300 and int(h.sum()) == 300
    _, rounds, st = heard_trial(N, F, first(0, N), byz, SEED, 7, 16, [1] * N, byz_strategy=strategy)
    assert rounds == 1
    assert all(s == ({"killed": False, "x": None, "decided": None, "k": None} if i in (1, 4, 8) else
                     {"killed": False, "x": 1, "decided": True, "k": 2}) for i, s in enumerate(st))


def test_split_breaks_agreement_at_least_twice_as_often_as_random():
    """(10, 4), b = 4, 1500 trials, k_max 16, random starts.  The restatement's counts: SPLIT
    1330 violations and 146 undecided; RANDOM 1/2 on the same trials 284 violations and 6 undecided."""
    strategies_exist()
    split, rnd = shared_hist("10,4,4", SPLIT), shared_hist("10,4,4", "random")
    print(f"violations: SPLIT {int(split[-1])}, RANDOM 1/2 {int(rnd[-1])}; undecided {undecided(split)}, {undecided(rnd)}")
    assert int(rnd[-1]) > 0 and int(split[-1]) >= 2 * int(rnd[-1])


def test_balance_keeps_the_run_undecided():
    """(10, 4), b = 4, 1500 trials, k_max 16, random starts.  The restatement's count:
    1500 of 1500 undecided, no violation."""
    strategies_exist()
    bal = shared_hist("10,4,4", BALANCE)
    print(f"BALANCE: {undecided(bal)} of {T_LAW} undecided, {int(bal[-1])} violations")
    assert undecided(bal) >= 0.9 * T_LAW


def test_balance_slows_two_liars_down():
    """(10, 4), b = 2, 1500 trials, k_max 16, random starts.  The restatement's figures:
    BALANCE 5.232 rounds per trial, RANDOM 1/2 2.706; no violation and no undecided trial under either."""
    strategies_exist()
    bal, rnd = shared_hist("10,4,2", BALANCE), shared_hist("10,4,2", "random")
    print(f"mean rounds: BALANCE {mean_rounds(bal):.3f}, RANDOM 1/2 {mean_rounds(rnd):.3f}; violations {int(bal[-1])}, {int(rnd[-1])}")
    assert mean_rounds(bal) >= mean_rounds(rnd) + 1
