"""BO_MODE_RANDOM_TALLY3, count-level random delivery with three vote classes (CPU suite).

The definition, restated here in plain Python over
benor.tally_cdf, oracle.philox4x32_10, oracle.coin and oracle.random_init --
nothing from the kernel; tests/test_tally3_gpu.py checks the kernel against it
bit for bit:

* Trial set-up, histogram layout, "common value" rule, halting and k = R + 1 as
  in BO_MODE_RANDOM_TALLY (tests/test_tally.py); any quorum q = N - F, initial
  values may be "?".
* A phase's votes are K0 zeros, K1 ones and Kq "?" (K0 + K1 + Kq = m).  Classes:
  S = the smallest (ties: "?", then 0, then 1), A = the ones unless S is the
  ones, then the zeros; T = the third.  Receiver c:
    cA = lo + #{j : T[j] <= u} from row K_A of the (m, q) table, u = u_R or u_P
         of the block {trial_lo, trial_hi, c, (r - 1) | 5 << 24} as in mode 3;
    cS : for i = 0..Ks-1, member i of S is in the inbox iff v_i < q - cA - taken,
         v_i uniform below m - K_A - i (multiply-shift with exact rejection) from
         the word stream of blocks {trial_lo, trial_hi, c | b << 12,
         (r - 1) | phase << 16 | 6 << 24}, b = 0, 1, ..; words in order;
    cT = q - cA - cS.
* R-phase: c0 > c1 -> propose 0, c1 > c0 -> 1, else "?".  P-phase: c0 > F ->
  x = 0 decided, else c1 > F -> x = 1 decided, else the strict majority of
  (c0, c1), else oracle.coin(seed, trial, c, r).  `decided` is sticky.
"""
import bisect

import numpy as np
import pytest

import benor
import oracle
import test_tally as model
from test_tally import chi2_two_sample, first, philox, row

STREAM_TALLY, STREAM_WALK = 5, 6
SEED = model.SEED
Q = "?"
INIT_10 = [0, 1, 0, Q, 1, Q, 0, 1, 1, 0]


# ------------------------------------------------------------ restatement
class WordStream:
    """Words of the Philox blocks {c0, c1, c2 | b << 12, c3}, b = 0, 1, ..., in order."""

    def __init__(self, seed, c0, c1, c2, c3):
        self.seed, self.ctr, self.buf, self.i = seed, (c0, c1, c2, c3), None, 0

    def next(self):
        if self.i % 4 == 0:
            c0, c1, c2, c3 = self.ctr
            self.buf = philox(self.seed, (c0, c1, c2 | (self.i // 4) << 12, c3))
        w = self.buf[self.i % 4]
        self.i += 1
        return w

    def below(self, d):
        """Uniform integer in [0, d): Lemire's multiply-shift with exact rejection."""
        mm = self.next() * d
        if (mm & 0xFFFFFFFF) < d:
            t = (2 ** 32 - d) % d
            while (mm & 0xFFFFFFFF) < t:
                mm = self.next() * d
        return mm >> 32


def classes(K0, K1, Kq):
    """(S, A, T) as indices into (0, 1, "?") = (0, 1, 2)."""
    if Kq <= K0 and Kq <= K1:
        return 2, 1, 0
    if K0 <= K1:
        return 0, 1, 2
    return 1, 0, 2


def draw3(m, q, K, seed, trial, c, r, phase, u):
    """Receiver c's (c0, c1) over class sizes K = (K0, K1, Kq)."""
    S, A, T = classes(*K)
    lo, thr = row(m, q, K[A])
    cA = lo + bisect.bisect_right(thr, u)
    cS = 0
    if K[S]:
        ws = WordStream(seed, trial & 0xFFFFFFFF, trial >> 32, c, (r - 1) | phase << 16 | STREAM_WALK << 24)
        for i in range(K[S]):
            if ws.below(m - K[A] - i) < q - cA - cS:
                cS += 1
    cnt = [0, 0, 0]
    cnt[A], cnt[S], cnt[T] = cA, cS, q - cA - cS
    assert min(cnt) >= 0 and all(n <= k for n, k in zip(cnt, K))
    return cnt[0], cnt[1]


def tally3_trial(N, F, faulty, seed, trial, k_max, initial_values=None):
    """One trial: (histogram bins it increments, rounds, per-node states)."""
    live = [i for i in range(N) if not faulty[i]]
    m, q = len(live), N - F
    states = [{"killed": True, "x": None, "decided": None, "k": None} if faulty[i] else None for i in range(N)]
    if m == 0:
        return [2], 0, states
    if initial_values is None:
        x = [oracle.random_init(seed, trial, c, m) for c in range(m)]
    else:
        x = [2 if initial_values[i] == Q else initial_values[i] for i in live]
    assert m >= q and all(v in (0, 1, 2) for v in x)
    dec = [False] * m
    tlo, thi = trial & 0xFFFFFFFF, trial >> 32
    R = 0
    for r in range(1, k_max + 1):
        blocks = [philox(seed, (tlo, thi, c, (r - 1) | STREAM_TALLY << 24)) for c in range(m)]
        K = tuple(x.count(v) for v in (0, 1, 2))
        prop = []
        for c, b in enumerate(blocks):
            c0, c1 = draw3(m, q, K, seed, trial, c, r, 0, b[1] << 32 | b[0])
            prop.append(0 if c0 > c1 else 1 if c1 > c0 else 2)
        K2 = tuple(prop.count(v) for v in (0, 1, 2))
        for c, b in enumerate(blocks):
            c0, c1 = draw3(m, q, K2, seed, trial, c, r, 1, b[3] << 32 | b[2])
            if c0 > F:
                x[c], dec[c] = 0, True
            elif c1 > F:
                x[c], dec[c] = 1, True
            elif c0 != c1:
                x[c] = 1 if c1 > c0 else 0
            else:
                x[c] = oracle.coin(seed, trial, c, r)
        R = r
        if all(dec):
            break
    ones = sum(x)
    v = 2 if 0 < ones < m else (1 if ones else 0)
    all_dec = all(dec)
    bins = [R * 3 + v] if all_dec else [v]
    if all_dec and v == 2:
        bins.append((k_max + 1) * 3)
    for c, i in enumerate(live):
        states[i] = {"killed": False, "x": x[c], "decided": dec[c], "k": R + 1}
    return bins, (R if all_dec else 0), states


def tally3_hist(N, F, faulty, seed, trial_begin, trial_count, k_max, initial_values=None):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in tally3_trial(N, F, faulty, seed, t, k_max, initial_values)[0]:
            h[b] += 1
    return h


# ---------------------------------------------------------------- the tests
def test_word_stream_draw_is_in_range_and_rejects():
    ws = WordStream(SEED, 7, 0, 3, STREAM_WALK << 24)
    assert all(0 <= ws.below(d) < d for d in (1, 2, 3, 7, 4096, 2 ** 31 + 1) for _ in range(50))
    assert ws.i >= 300                                  # at least one word per draw, in order


def test_classes():
    assert classes(3, 4, 0) == (2, 1, 0)                # no "?": the ones from the table, as mode 3
    assert classes(3, 3, 3) == (2, 1, 0)                # ties: "?" first
    assert classes(2, 2, 5) == (0, 1, 2)                # ... then the zeros
    assert classes(5, 1, 3) == (1, 0, 2)                # S = ones: the zeros from the table
    assert classes(0, 0, 9) == (0, 1, 2)


@pytest.mark.parametrize("N,F,f", [(11, 4, 0), (11, 4, 2), (69, 24, 5)])
def test_restatement_equals_mode_3_in_its_scope(N, F, f):
    faulty = first(f, N)
    for t in range(200):
        assert tally3_trial(N, F, faulty, SEED, t, 16) == model.tally_trial(N, F, faulty, SEED, t, 16), t


def test_kernel_choice_and_validation():
    T3 = benor.BO_MODE_RANDOM_TALLY3
    assert T3 == 4 and benor.BO_KERNEL_TALLY3 == 10 and benor.BO_KERNEL_TALLY3 in benor.KERNEL_NAMES
    for N, F in ((10, 4), (1024, 340), (4096, 1366)):
        assert benor.kernel_for(N, F, first(0, N), mode=T3) == benor.BO_KERNEL_TALLY3, (N, F)
    init = [1, 0, Q] + [1] * 8
    assert benor.kernel_for(11, 4, first(0, 11), mode=T3, initial_values=init) == benor.BO_KERNEL_TALLY3
    # inside mode 3's scope: that mode's kernel (a "?" held by a crashed node is no initial value of the run)
    assert benor.kernel_for(11, 4, first(0, 11), mode=T3) == benor.BO_KERNEL_TALLY
    assert benor.kernel_for(1024, 341, first(0, 1024), mode=T3) == benor.BO_KERNEL_TALLY
    assert benor.kernel_for(11, 4, first(1, 11), mode=T3, initial_values=[Q] + [1, 0] * 5) == benor.BO_KERNEL_TALLY
    assert benor.kernel_for(3, 3, first(3, 3), mode=T3) == benor.BO_KERNEL_NONE
    with pytest.raises(benor.Error) as e_t3:
        benor.kernel_for(10, 4, first(5, 10), mode=T3)
    with pytest.raises(benor.Error) as e_mask:
        benor.kernel_for(10, 4, first(5, 10), mode=benor.BO_MODE_RANDOM_DELIVERY)
    assert str(e_t3.value) == str(e_mask.value)
    with pytest.raises(RuntimeError, match="libbenor error 7.*BO_MODE_RANDOM_DELIVERY"):     # mode 3 as before
        benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_RANDOM_TALLY)


@pytest.mark.parametrize("N,F,f,init", [(10, 4, 0, None), (10, 4, 2, None), (10, 4, 1, INIT_10)])
def test_law_matches_random_delivery(N, F, f, init):
    """The restatement's histogram against the CPU oracle's mask-level random
    delivery, 2 * 10^4 trials a side, k_max 16: two-sample chi^2 over bins pooled
    to >= 20, p > 10^-3 at fixed seeds."""
    T, k_max = 20000, 16
    faulty = first(f, N)
    ref = oracle.run_trials(N, F, faulty, seed=SEED + 1, trial_count=T, k_max=k_max, initial_values=init,
                            mode=oracle.MODE_RANDOM_DELIVERY).hist
    got = tally3_hist(N, F, faulty, SEED, 0, T, k_max, init)
    assert int(got[:-1].sum()) == T == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"(N, F, f) = ({N}, {F}, {f}){' fixed init' if init else ''}: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}")
    assert p > 1e-3, (p, stat, df)
