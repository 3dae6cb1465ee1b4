"""BO_MODE_BYZ_TALLY, count-level random delivery with Byzantine senders (CPU suite).

The definition (include/benor.h), restated here in plain Python
over test_tally3.draw3, philox, oracle.random_init, oracle.coin and
benor.byz_cdf -- nothing from the kernel; tests/test_byz_tally_gpu.py checks the
kernel against it bit for bit:

* `faulty[i]` crashed from the start (f of them), `byzantine[i]` Byzantine (b of
  them), f + b <= F.  The m = N - f live nodes, honest and Byzantine together,
  carry compact indices c in ascending node id; q = N - F, so m >= q + b.
* All m live nodes send at every step; only the h = m - b honest ones receive
  and run the rule.  (H0, H1, Hq) are the class sizes over the honest senders: x
  at an R-step, the proposal at a P-step; decided nodes keep sending.
* B1 of the b Byzantine messages that could reach receiver c carry 1:
    BYZ_RANDOM  byz_one = 0: 0; 2^32 - 1: b; else #{j : thr[j] <= u}, thr =
                benor.byz_cdf(b, byz_one), u from the Philox block {trial_lo,
                trial_hi, c, (r - 1) | 10 << 24}: R-phase out[1] << 32 | out[0],
                P-phase out[3] << 32 | out[2];
    BYZ_OPPOSE  0 if H1 > H0, b if H0 > H1, for every receiver; on H0 == H1 the
                step is BYZ_RANDOM's.
* Receiver c's (c0, c1) = test_tally3.draw3 among m senders with the class sizes
  (H0 + b - B1, H1 + B1, Hq) and mode 4's stream-5 uniform.  Rule, coins, k and
  the histogram layout are mode 4's (tests/test_tally3.py), halting and the
  common value over the honest nodes.
* A Byzantine node's state is {killed False, x None, decided None, k None}.
"""
import bisect
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import benor
import oracle
from test_tally import chi2_two_sample, first, philox
from test_tally3 import draw3

M8 = getattr(benor, "BO_MODE_BYZ_TALLY", None)               # absent before the mode: every test fails
BYZ = getattr(benor, "BO_KERNEL_TALLY_BYZ", None)
RANDOM, OPPOSE = 0, 1
STREAM_TALLY, STREAM_LIE = 5, 10
SEED = 0x243F6A8885A308D3
ALL, HALF, QUARTER = 2 ** 32 - 1, 2 ** 31, 2 ** 30
Q = "?"


def marks(ids, N):
    return [i in ids for i in range(N)]


# ------------------------------------------------------------ restatement
@functools.lru_cache(maxsize=None)
def lie_thresholds(b, byz_one):
    return benor.byz_cdf(b, byz_one)


def lies(b, byz_one, strategy, H0, H1, u):
    """B1: how many of the b Byzantine messages carry 1 for a receiver whose stream-10 uniform is u()."""
    if strategy == OPPOSE and H0 != H1:
        return b if H0 > H1 else 0
    if byz_one == 0:
        return 0
    if byz_one == ALL:
        return b
    return bisect.bisect_right(lie_thresholds(b, byz_one), u())


def byz_trial(N, F, faulty, byzantine, seed, trial, k_max, initial_values=None, byz_one=0, byz_strategy=RANDOM):
    """One trial: (histogram bins it increments, rounds, per-node states)."""
    live = [i for i in range(N) if not faulty[i]]
    honest = [c for c, i in enumerate(live) if not byzantine[i]]
    m, q, b = len(live), N - F, len(live) - len(honest)
    assert not any(faulty[i] and byzantine[i] for i in range(N)) and (N - m) + b <= F
    states = [{"killed": True, "x": None, "decided": None, "k": None} if faulty[i] else
              {"killed": False, "x": None, "decided": None, "k": None} for i in range(N)]
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
        lie = {}

        def sizes(vals):
            return [sum(1 for v in vals.values() if v == k) for k in (0, 1, 2)]

        def counts(H, c, phase):

            def u():
                if c not in lie:
                    lie[c] = philox(seed, (tlo, thi, c, (r - 1) | STREAM_LIE << 24))
                w = lie[c]
                return w[3] << 32 | w[2] if phase else w[1] << 32 | w[0]
            B1 = lies(b, byz_one, byz_strategy, H[0], H[1], u)
            s = blocks[c]
            return draw3(m, q, (H[0] + b - B1, H[1] + B1, H[2]), seed, trial, c, r, phase,
                         s[3] << 32 | s[2] if phase else s[1] << 32 | s[0])

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


def byz_hist(N, F, faulty, byzantine, seed, trial_begin, trial_count, k_max, initial_values=None, **lie):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in byz_trial(N, F, faulty, byzantine, seed, t, k_max, initial_values, **lie)[0]:
            h[b] += 1
    return h


# ------------------------------------------------- mask-level simulation
def mask_sim_hist(N, F, faulty, byzantine, k_max, trials, rng, byz_one=0, byz_strategy=RANDOM, chunk=10000):
    """The same model at the level of inboxes: at every step each honest receiver
    hears a uniform q-subset (the q smallest of iid uniform keys) of the m live
    senders; an honest sender's message is its value, a Byzantine sender's an
    explicit Bernoulli(byz_one / 2^32) lie per (sender, receiver, step) -- or, under
    BYZ_OPPOSE off a tie, the value fewer honest senders hold.  Initial values,
    inboxes, lies and coins from `rng`."""
    live = [i for i in range(N) if not faulty[i]]
    is_byz = np.array([bool(byzantine[i]) for i in live])
    m, q = len(live), N - F
    prob = 1.0 if byz_one == ALL else byz_one / 2.0 ** 32
    hist = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)

    def counts(vals):
        n = len(vals)
        H0 = ((vals == 0) & ~is_byz).sum(axis=1)
        H1 = ((vals == 1) & ~is_byz).sum(axis=1)
        lie = (rng.random((n, m, m)) < prob).astype(np.int8)                        # [trial, receiver, sender]
        if byz_strategy == OPPOSE:
            fewer = np.where(H0 > H1, 1, 0).astype(np.int8)
            lie = np.where((H0 == H1)[:, None, None], lie, fewer[:, None, None])
        heard = np.where(is_byz[None, None, :], lie, vals[:, None, :])
        keys = rng.random((n, m, m))
        inbox = np.argpartition(keys, q - 1, axis=2)[:, :, :q]
        got = np.take_along_axis(heard, inbox, axis=2)
        return (got == 0).sum(axis=2), (got == 1).sum(axis=2)

    def finish(x, dec, R):
        ones = ((x == 1) & ~is_byz).sum(axis=1)
        v = np.where((ones > 0) & (ones < (~is_byz).sum()), 2, np.where(ones > 0, 1, 0))
        all_dec = (dec | is_byz).all(axis=1)
        np.add.at(hist, np.where(all_dec, R * 3 + v, v), 1)
        hist[-1] += int((all_dec & (v == 2)).sum())

    for lo in range(0, trials, chunk):
        n = min(chunk, trials - lo)
        x = rng.integers(0, 2, size=(n, m)).astype(np.int8)
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


# ---------------------------------------------------------------- the tests
def test_the_mode_exists():
    assert M8 == 8 and BYZ == 14 and BYZ in benor.KERNEL_NAMES
    assert (benor.BYZ_RANDOM, benor.BYZ_OPPOSE) == (RANDOM, OPPOSE)
    assert benor.lib().bo_abi_version() == 8                # the struct layout is unchanged
    with pytest.raises(ValueError):                         # byz_one fills crash_cut's word
        benor.kernel_for(10, 4, first(0, 10), mode=M8, byzantine=marks({1}, 10), byz_one=HALF, crash_cut=3)
    with pytest.raises(ValueError):
        benor.kernel_for(10, 4, first(0, 10), mode=M8, byzantine=marks({1}, 10), byz_one=ALL + 1)
    with pytest.raises(ValueError):                         # a node is crashed or Byzantine, not both
        benor.kernel_for(10, 4, first(2, 10), mode=M8, byzantine=marks({1}, 10))
    with pytest.raises(ValueError):
        benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_RANDOM_TALLY3, byzantine=marks({1}, 10))


def test_byz_cdf_arguments():
    L = benor.lib()
    n = ctypes.c_uint32()
    thr = (ctypes.c_uint64 * 8)()
    assert L.bo_byz_cdf(5, HALF, thr, 4, ctypes.byref(n)) == benor.BO_ERR_INVALID_ARGUMENT      # a short cap
    assert L.bo_byz_cdf(5, HALF, thr, 5, ctypes.byref(n)) == benor.BO_OK
    assert n.value == 5
    assert [thr[j] for j in range(5)] == benor.byz_cdf(5, HALF)
    assert benor.byz_cdf(0, HALF) == []


@pytest.mark.parametrize("b", [1, 2, 70, 340])
@pytest.mark.parametrize("byz_one", [1, QUARTER, HALF, ALL - 1])
def test_byz_cdf_accuracy(b, byz_one):
    """|T[j] / 2^64 - CDF(j)| <= 2^-40 against the exact rational Binomial(b, byz_one / 2^32).

    The bound the double construction allows: p and 1 - p are exact, and so are the
    products (b - j) p and (j + 1)(1 - p) (12 + 32 bits); a weight is at most b steps
    from the mode's, two roundings a step (the ratio's division, the product), so its
    relative error is below 2 b 2^-53 (1 + o(1)); the running sums and the total add at
    most b 2^-53 each, the final division one rounding: below (4 b + 8) 2^-53 on a
    CDF <= 1, under 2^-42 for b <= 340, and the floor to 2^-64 units adds 2^-64."""
    thr = benor.byz_cdf(b, byz_one)
    assert len(thr) == b
    assert all(t0 <= t1 for t0, t1 in zip(thr, thr[1:]))
    assert all(0 <= t < 2 ** 64 for t in thr)
    p = Fraction(byz_one, 2 ** 32)
    run, worst = Fraction(0), 0.0
    for j, t in enumerate(thr):
        run += math.comb(b, j) * p ** j * (1 - p) ** (b - j)
        err = abs(Fraction(t, 2 ** 64) - run)
        assert err <= Fraction(1, 2 ** 40), (j, float(err))
        assert err <= Fraction(4 * b + 8, 2 ** 53) + Fraction(1, 2 ** 64), (j, float(err))
        worst = max(worst, float(err))
    print(f"b = {b}, byz_one = {byz_one}: worst |T/2^64 - CDF| = {worst:.3g}")


def test_byz_draw_covers_the_support():
    assert M8 == 8
    for b in (1, 2, 40):                                    # CDF(0) = 2^-b >= 2^-64: the least count is 0
        thr = lie_thresholds(b, HALF)
        assert bisect.bisect_right(thr, 0) == 0
        assert bisect.bisect_right(thr, 2 ** 64 - 1) == b
    assert abs(lie_thresholds(2, HALF)[0] - 2 ** 62) <= 2 ** 24 and abs(lie_thresholds(2, HALF)[1] - 3 * 2 ** 62) <= 2 ** 24
    assert lies(7, 0, RANDOM, 3, 3, None) == 0 and lies(7, ALL, RANDOM, 3, 3, None) == 7     # no stream-10 word
    assert lies(7, HALF, OPPOSE, 4, 3, None) == 7 and lies(7, HALF, OPPOSE, 3, 4, None) == 0
    assert lies(7, HALF, OPPOSE, 3, 3, lambda: 2 ** 64 - 1) == 7


def test_validation_and_kernel_choice():
    """Through bo_kernel_for: no device needed."""
    assert M8 == 8
    one = dict(mode=M8, byz_one=HALF)
    with pytest.raises(benor.Error, match="at most F nodes crashed or Byzantine"):                  # f + b > F: BO_ERR_FAULTY_COUNT
        benor.kernel_for(10, 4, first(2, 10), byzantine=marks({5, 6, 7}, 10), **one)
    assert benor.kernel_for(10, 4, first(2, 10), byzantine=marks({5, 6}, 10), **one) == BYZ          # f + b = F
    with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}"):       # faulty value 3
        benor.kernel_for(10, 4, [0, 3] + [0] * 8, **one)
    with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}"):       # strategy 2
        benor.kernel_for(10, 4, first(0, 10), byzantine=marks({1}, 10), byz_strategy=2, **one)
    assert benor.kernel_for(10, 4, [0, 2] + [0] * 8, **one) == BYZ                                   # the raw value 2
    # every other mode keeps reading non-zero as faulty
    assert benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_RANDOM_TALLY3) == benor.BO_KERNEL_TALLY3
    # b = 0 is mode 4's plan, at every byz_one and strategy
    for strategy in (RANDOM, OPPOSE):
        for w in (0, HALF, ALL):
            kw = dict(mode=M8, byzantine=marks(set(), 10), byz_one=w, byz_strategy=strategy)
            assert benor.kernel_for(10, 4, first(0, 10), **kw) == benor.BO_KERNEL_TALLY3
            kw["byzantine"] = marks(set(), 11)
            assert benor.kernel_for(11, 4, first(0, 11), **kw) == benor.BO_KERNEL_TALLY
    for N, F, ids in ((10, 4, {0}), (11, 4, {3, 9}), (1024, 340, set(range(0, 1000, 10))), (4096, 1366, {7})):
        assert benor.kernel_for(N, F, first(0, N), byzantine=marks(ids, N), byz_strategy=OPPOSE, **one) == BYZ
    assert benor.lib().bo_abi_version() == 8


def test_restatement_without_byzantine_nodes_is_mode_4():
    import test_tally3
    assert M8 == 8

    for N, F, f in ((10, 4, 0), (10, 4, 2), (11, 4, 1)):
        got = byz_hist(N, F, first(f, N), marks(set(), N), SEED, 0, 300, 16, byz_one=HALF, byz_strategy=OPPOSE)
        assert np.array_equal(got, test_tally3.tally3_hist(N, F, first(f, N), SEED, 0, 300, 16))


def test_law_matches_the_mask_level_simulation():
    """The restatement's histogram against the mask-level simulation, (26, 8), b = 4,
    byz_one 1/2, 2 * 10^4 trials a side, k_max 16: two-sample chi^2 over bins pooled
    to >= 20, p > 10^-3 at fixed seeds."""
    assert M8 == 8
    N, F, T, k_max = 26, 8, 20000, 16
    faulty, byz = first(0, N), marks({2, 9, 17, 25}, N)
    got = byz_hist(N, F, faulty, byz, SEED, 0, T, k_max, byz_one=HALF)
    ref = mask_sim_hist(N, F, faulty, byz, k_max, T, np.random.default_rng(SEED + 1), byz_one=HALF)
    assert int(got[:-1].sum()) == T == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"(N, F, b) = ({N}, {F}, 4), byz_one 1/2: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}, "
          f"agreement violations {int(got[-1])} (restatement) / {int(ref[-1])} (simulation)")
    assert p > 1e-3, (p, stat, df)


def test_oppose_is_random_never_when_every_honest_node_starts_at_1():
    """Every honest x = 1 and q - b > b: every honest receiver proposes 1 and keeps 1, so H1 > H0 at
    every step and BYZ_OPPOSE sends 0 to everybody -- BYZ_RANDOM's step with byz_one = 0."""
    assert M8 == 8
    N, F, byz = 10, 4, marks({3, 8}, 10)
    init = [1] * N
    a = byz_hist(N, F, first(0, N), byz, SEED, 0, 300, 16, init, byz_one=HALF, byz_strategy=OPPOSE)
    c = byz_hist(N, F, first(0, N), byz, SEED, 0, 300, 16, init, byz_one=0, byz_strategy=RANDOM)
    assert np.array_equal(a, c) and int(a[:-1].sum()) == 300
    for t in range(5):
        assert byz_trial(N, F, first(0, N), byz, SEED, t, 16, init, byz_one=HALF, byz_strategy=OPPOSE) == \
               byz_trial(N, F, first(0, N), byz, SEED, t, 16, init, byz_one=0, byz_strategy=RANDOM)


@pytest.mark.parametrize("strategy,byz_one", [(RANDOM, HALF), (RANDOM, ALL), (OPPOSE, HALF)])
def test_one_liar_cannot_make_0_voters_decide_1(strategy, byz_one):
    """(10, 4), b = 1, every honest x = 0: c1 <= 1 <= F at every step, so nobody decides 1 or holds it."""
    assert M8 == 8
    N, F, k_max = 10, 4, 16
    h = byz_hist(N, F, first(0, N), marks({4}, N), SEED, 0, 300, k_max, [0] * N, byz_one=byz_one, byz_strategy=strategy)
    assert int(h[:-1].sum()) == 300
    assert all(int(h[R * 3 + v]) == 0 for R in range(k_max + 1) for v in (1, 2)) and int(h[-1]) == 0
    _, _, st = byz_trial(N, F, first(0, N), marks({4}, N), SEED, 0, k_max, [0] * N, byz_one=byz_one, byz_strategy=strategy)
    assert st[4] == {"killed": False, "x": None, "decided": None, "k": None}
    assert all(s == {"killed": False, "x": 0, "decided": True, "k": 2} for i, s in enumerate(st) if i != 4)
