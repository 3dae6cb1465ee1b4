"""BO_MODE_RANDOM_TALLY, the count-level random-delivery mode (CPU suite).

The definition, restated here in plain Python over
benor.tally_cdf, oracle.philox4x32_10 and oracle.random_init -- nothing from the
kernel; tests/test_tally_gpu.py checks the kernel against it bit for bit:

* Trial set-up, histogram layout, "common value" rule and k = R + 1 as in the
  other batch modes (oracle/benor_oracle.c run_one); m = 0 and m < q land in
  bin 2.  q = N - F is odd and no initial value is "?".
* Round r = 1..k_max, live nodes by compact index c, m live, q = N - F:
    R-phase  K = live nodes with x = 1; receiver c draws c1 from row K with u_R,
             c0 = q - c1; it proposes 1 if c1 > c0, else 0.
    P-phase  K' = live nodes proposing 1; receiver c draws c1 from row K' with
             u_P, c0 = q - c1; c0 > F: x = 0, decided; else c1 > F: x = 1,
             decided; else x = the majority.  `decided` is sticky.
    Halt when every live node has decided.
* Philox4x32-10 keyed by the seed, counter {trial_lo, trial_hi, c,
  (r - 1) | 5 << 24}: u_R = out[1] << 32 | out[0], u_P = out[3] << 32 | out[2].
* Row K of the table for (m, q): lo = max(0, q - (m - K)), hi = min(K, q), and
  hi - lo thresholds T[j] = min(2^64 - 1, floor(CDF_K(lo + j) 2^64)), CDF_K the
  CDF of Hypergeometric(m, K, q); the draw is c1 = lo + #{j : T[j] <= u}.  The
  table holds every row K = 0..m in full (no use of the K <-> m - K symmetry).
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

STREAM_TALLY = 5
SEED = 0x243F6A8885A308D3


# ------------------------------------------------------------ restatement
@functools.lru_cache(maxsize=None)
def row(m, q, K):
    return benor.tally_cdf(m, q, K)


_KEY = (ctypes.c_uint32 * 2)()
_CTR = (ctypes.c_uint32 * 4)()
_OUT = (ctypes.c_uint32 * 4)()


def philox(seed, ctr):
    """oracle.philox4x32_10 on reused buffers (one call per receiver-round)."""
    _KEY[0], _KEY[1] = seed & 0xFFFFFFFF, seed >> 32
    _CTR[0], _CTR[1], _CTR[2], _CTR[3] = ctr
    oracle.lib().oracle_philox4x32_10(_KEY, _CTR, _OUT)
    return _OUT[0], _OUT[1], _OUT[2], _OUT[3]


def draw(m, q, K, u):
    lo, thr = row(m, q, K)
    return lo + bisect.bisect_right(thr, u)


def tally_trial(N, F, faulty, seed, trial, k_max, initial_values=None):
    """One trial: (histogram bins it increments, rounds, per-node states)."""
    live = [i for i in range(N) if not faulty[i]]
    m, q = len(live), N - F
    states = [{"killed": True, "x": None, "decided": None, "k": None} if faulty[i] else None for i in range(N)]
    if m == 0:
        return [2], 0, states
    if initial_values is None:
        x = [oracle.random_init(seed, trial, c, m) for c in range(m)]
    else:
        x = [initial_values[i] for i in live]
    assert all(v in (0, 1) for v in x) and q % 2 == 1
    if m < q:                                       # no trigger ever fires
        for c, i in enumerate(live):
            states[i] = {"killed": False, "x": x[c], "decided": False, "k": 1}
        return [2], 0, states
    dec = [False] * m
    tlo, thi = trial & 0xFFFFFFFF, trial >> 32
    R = 0
    for r in range(1, k_max + 1):
        blocks = [philox(seed, (tlo, thi, c, (r - 1) | STREAM_TALLY << 24)) for c in range(m)]
        K = sum(x)
        prop = [1 if 2 * draw(m, q, K, b[1] << 32 | b[0]) > q else 0 for b in blocks]
        K2 = sum(prop)
        for c, b in enumerate(blocks):
            c1 = draw(m, q, K2, b[3] << 32 | b[2])
            c0 = q - c1
            if c0 > F:
                x[c], dec[c] = 0, True
            elif c1 > F:
                x[c], dec[c] = 1, True
            else:
                x[c] = 1 if c1 > c0 else 0
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


def tally_hist(N, F, faulty, seed, trial_begin, trial_count, k_max, initial_values=None):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in tally_trial(N, F, faulty, seed, t, k_max, initial_values)[0]:
            h[b] += 1
    return h


# ---------------------------------------------------------- two-sample chi^2
def _gamma_q(a, x):
    """Regularised upper incomplete gamma Q(a, x) (series / Lentz continued fraction)."""
    if x <= 0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1:
        term = s = 1.0 / a
        n = a
        for _ in range(10000):
            n += 1
            term *= x / n
            s += term
            if abs(term) < abs(s) * 1e-15:
                break
        return 1.0 - s * math.exp(-x + a * math.log(x) - lg)
    tiny = 1e-300
    b = x + 1 - a
    c = 1 / tiny
    d = 1 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        delta = d * c
        h *= delta
        if abs(delta - 1) < 1e-15:
            break
    return math.exp(-x + a * math.log(x) - lg) * h


def chi2_two_sample(ha, hb, min_pooled=20):
    """p-value of the two-sample chi^2 test over the outcome bins of two
    histograms (the last bin, agreement violations, repeats bin (R, 2) and is left
    out).  Bins whose pooled count is below min_pooled are merged into one
    cell; if that cell is still short it joins the smallest kept one."""
    a = np.asarray(ha[:-1], dtype=np.float64)
    b = np.asarray(hb[:-1], dtype=np.float64)
    pooled = a + b
    keep = pooled >= min_pooled
    cells = [(x, y) for x, y in zip(a[keep], b[keep])]
    ra, rb = a[~keep].sum(), b[~keep].sum()
    if ra + rb > 0:
        if ra + rb >= min_pooled or not cells:
            cells.append((ra, rb))
        else:
            i = min(range(len(cells)), key=lambda j: cells[j][0] + cells[j][1])
            cells[i] = (cells[i][0] + ra, cells[i][1] + rb)
    na, nb = a.sum(), b.sum()
    stat = sum((math.sqrt(nb / na) * x - math.sqrt(na / nb) * y) ** 2 / (x + y) for x, y in cells)
    df = len(cells) - 1
    return (_gamma_q(df / 2, stat / 2) if df > 0 else 1.0), stat, df


def test_chi2_helper():
    assert abs(_gamma_q(0.5, 3.841458820694124 / 2) - 0.05) < 1e-9          # chi^2_1 95 %
    assert abs(_gamma_q(5.0, 18.307038053275146 / 2) - 0.05) < 1e-9         # chi^2_10 95 %
    assert abs(_gamma_q(2.0, 0.5) - 1.5 * math.exp(-0.5)) < 1e-12
    p, stat, df = chi2_two_sample([100, 50, 3, 2, 0], [90, 60, 1, 4, 0])
    assert df == 1 and abs(stat - (10 ** 2 / 190 + 10 ** 2 / 120)) < 1e-9   # the short cell joined (50, 60)


# ------------------------------------------------- kernel choice, validation
def first(f, N):
    return [i < f for i in range(N)]


def test_kernel_choice():
    assert benor.BO_MODE_RANDOM_TALLY == 3 and benor.BO_KERNEL_TALLY == 9
    assert benor.BO_KERNEL_TALLY in benor.KERNEL_NAMES
    for N, F in ((1024, 341), (11, 4), (256, 85), (4096, 1365)):
        assert benor.kernel_for(N, F, first(0, N), mode=benor.BO_MODE_RANDOM_TALLY) == benor.BO_KERNEL_TALLY
    assert benor.kernel_for(11, 4, first(4, 11), mode=benor.BO_MODE_RANDOM_TALLY) == benor.BO_KERNEL_TALLY


def test_validation():
    T = benor.BO_MODE_RANDOM_TALLY
    with pytest.raises(RuntimeError, match="libbenor error 7.*BO_MODE_RANDOM_DELIVERY"):      # even quorum
        benor.kernel_for(10, 4, first(0, 10), mode=T)
    with pytest.raises(RuntimeError, match="libbenor error 7.*BO_MODE_RANDOM_DELIVERY"):      # "?" initial value
        benor.kernel_for(11, 4, first(0, 11), mode=T, initial_values=[1, 0, "?"] + [1] * 8)
    # f > F: BO_MODE_RANDOM_DELIVERY's error
    with pytest.raises(benor.Error) as e_tally:
        benor.kernel_for(11, 4, first(5, 11), mode=T)
    with pytest.raises(benor.Error) as e_mask:
        benor.kernel_for(11, 4, first(5, 11), mode=benor.BO_MODE_RANDOM_DELIVERY)
    assert str(e_tally.value) == str(e_mask.value)
    # a "?" held by a crashed node is no initial value of the run
    init = ["?", "?"] + [1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert benor.kernel_for(11, 4, first(2, 11), mode=T, initial_values=init) == benor.BO_KERNEL_TALLY
    # no live node: outcomes need no kernel (bin 2, as in the other modes)
    assert benor.kernel_for(3, 3, first(3, 3), mode=T) == benor.BO_KERNEL_NONE


def test_tally_cdf_arguments():
    L = benor.lib()
    lo, n = ctypes.c_uint32(), ctypes.c_uint32()
    thr = (ctypes.c_uint64 * 8)()
    assert L.bo_tally_cdf(11, 7, 12, ctypes.byref(lo), thr, 8, ctypes.byref(n)) == benor.BO_ERR_INVALID_ARGUMENT
    assert L.bo_tally_cdf(11, 12, 3, ctypes.byref(lo), thr, 8, ctypes.byref(n)) == benor.BO_ERR_INVALID_ARGUMENT
    assert L.bo_tally_cdf(11, 7, 5, ctypes.byref(lo), thr, 3, ctypes.byref(n)) == benor.BO_ERR_INVALID_ARGUMENT
    assert L.bo_tally_cdf(11, 7, 5, ctypes.byref(lo), thr, 4, ctypes.byref(n)) == benor.BO_OK
    assert (lo.value, n.value) == (1, 4)


# ------------------------------------------------------------ table accuracy
@pytest.mark.parametrize("m,q", [(11, 7), (65, 45), (129, 83), (1024, 683), (4096, 2731)])
def test_table_accuracy(m, q):
    """|T[j] / 2^64 - CDF| <= 2^-40 against exact binomial fractions (the
    recurrence's worst case is ~4 width 2^-53, width <= 2049)."""
    worst = 0.0
    for K in sorted({0, 1, q // 2, m // 2, m // 2 + 1, q, m - q, m - 1, m}):
        lo, thr = benor.tally_cdf(m, q, K)
        elo, ehi = max(0, q - (m - K)), min(K, q)
        assert lo == elo and len(thr) == ehi - elo, (K, lo, len(thr))
        assert all(t0 <= t1 for t0, t1 in zip(thr, thr[1:])), K
        assert all(0 <= t < 2 ** 64 for t in thr)
        total = math.comb(m, q)
        run = 0
        for j, t in enumerate(thr):
            c = elo + j
            run += math.comb(K, c) * math.comb(m - K, q - c)
            err = abs(Fraction(t, 2 ** 64) - Fraction(run, total))
            assert err <= Fraction(1, 2 ** 40), (K, j, float(err))
            worst = max(worst, float(err))
    print(f"(m, q) = ({m}, {q}): worst |T/2^64 - CDF| = {worst:.3g}")


def test_rows_of_m_equal_q_are_empty():
    for m in (7, 65, 683):
        for K in (0, 1, m // 2, m - 1, m):
            assert benor.tally_cdf(m, m, K) == (K, [])


def test_draw_covers_the_support():
    lo, thr = benor.tally_cdf(11, 7, 5)
    assert draw(11, 7, 5, 0) == lo == 1                      # P(c1 = 1) = C(5,1) C(6,6) / C(11,7) > 2^-64
    assert draw(11, 7, 5, 2 ** 64 - 1) == 5
    assert abs(thr[0] - (5 * 2 ** 64) // 330) <= 2 ** 24     # CDF(1) = 5 / 330, built in double (2^-40 of 2^64)


# --------------------------------------------------------------------- law
@pytest.mark.parametrize("f", [0, 2])
def test_law_matches_random_delivery(f):
    """The restatement's histogram against the CPU oracle's mask-level random
    delivery, (11, 4, f), 2 * 10^4 trials a side, k_max 16: two-sample chi^2
    over bins pooled to >= 20, p > 10^-3 at fixed seeds."""
    N, F, T, k_max = 11, 4, 20000, 16
    faulty = first(f, N)
    ref = oracle.run_trials(N, F, faulty, seed=SEED + 1, trial_count=T, k_max=k_max,
                            mode=oracle.MODE_RANDOM_DELIVERY).hist
    got = tally_hist(N, F, faulty, SEED, 0, T, k_max)
    assert int(got[:-1].sum()) == T == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"(N, F, f) = ({N}, {F}, {f}): chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}")
    assert p > 1e-3, (p, stat, df)
