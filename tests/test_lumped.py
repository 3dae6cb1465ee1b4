"""The lumped API: the adversarial scheduler at the level of classes (CPU suite).

The definition (include/benor.h), restated here in plain Python over test_tally.philox,
test_byz_coin.common_coin, test_byz_sched.counts and the tables of bo_binom_half_cdf -- nothing from the kernel;
tests/test_lumped_gpu.py checks the kernel against it bit for bit.  Modes 12 and 13 with nodes replaced by the
two receiver parities: a trial is a Markov chain on (a_0, a_1, dec_0, dec_1).

* h_0 = ceil(m / 2) - byz_even, h_1 = floor(m / 2) - (b - byz_even), h = h_0 + h_1, q = N - F;
* R-phase: class sizes (H0, H1, Hq) -- round 1: the initial values'; later (h - A, A, 0), A = a_0 + a_1 -- give
  parity pi the counts of a receiver c with c & 1 = pi, and its proposal by the rule;
* P-phase: class sizes from the two proposals weighted by h_pi, the same counts, the rule's P-step: a_pi = v h_pi,
  or the round's common bit times h_pi, or Binomial(h_pi, 1/2);
* the draw: n by its set bits in ascending k, the j-th set bit takes the j-th 64-bit word of the blocks
  philox(seed, (t_lo, t_hi, 16 pi + (j >> 1), r | 13 << 24)); k <= 6 a popcount, k >= 7 lo_k + #{thr_k <= u}.

Also here: the exact law of the chain by a DP with Binomial weights, validated against mode 12/13's restatement
(test_byz_sched.sched_hist) independently of the feature, and then the reference for the lumped restatement and,
in the GPU suite, for both devices' histograms.
"""
import bisect
import functools
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import benor
import oracle
import test_byz_coin as coin_model
import test_byz_rule_b as mode9
import test_byz_sched as sched
import test_byz_tally as mode8
from conftest import PKG, ROOT
from test_tally import first, philox

BALANCE, SPLIT = sched.BALANCE, sched.SPLIT
STRATEGIES = sched.STRATEGIES
SEED = mode8.SEED
ALL, HALF = mode8.ALL, mode8.HALF
marks = mode8.marks
STREAM_BINOM = 13
CSRC = os.path.join(PKG, "csrc")
both_strategies = sched.both_strategies
both_rules = pytest.mark.parametrize("rule", ["ref", "b"])


def api_exists():
    for name in ("LumpedPlan", "lumped_trials", "lumped_trial", "byz_even", "binom_half_cdf"):
        assert hasattr(benor, name), name              # absent before the feature: every test that needs it fails


# ------------------------------------------------------------ restatement
@functools.lru_cache(maxsize=None)
def table(k):
    api_exists()
    lo, thr = benor.binom_half_cdf(k)
    return lo, tuple(thr)


def binom_half(n, seed, trial, pi, r):
    """Binomial(n, 1/2) from parity pi's words of round r."""
    total, j, blk = 0, 0, None
    for k in range(25):
        if not (n >> k) & 1:
            continue
        if j % 2 == 0:
            blk = philox(seed, (trial & 0xFFFFFFFF, trial >> 32, 16 * pi + (j >> 1), r | STREAM_BINOM << 24))
        u = (blk[1] << 32 | blk[0]) if j % 2 == 0 else (blk[3] << 32 | blk[2])
        j += 1
        if k <= 6:
            total += bin(u & ((1 << (1 << k)) - 1)).count("1")
        else:
            lo, thr = table(k)
            total += lo + bisect.bisect_right(thr, u)
    assert n < 1 << 25
    return total


def sizes(N, F, f, b, byz_even):
    m = N - f
    h0, h1 = (m + 1) // 2 - byz_even, m // 2 - (b - byz_even)
    return N - F, (h0, h1)


def r_step(rule, c0, c1, N, F):
    if rule == "b":
        return 0 if 2 * c0 > N + F else 1 if 2 * c1 > N + F else 2
    return 0 if c0 > c1 else 1 if c1 > c0 else 2


def p_step(rule, c0, c1, N, F):
    """(the new x or 2 for "takes the coin", whether the counts decide)."""
    if rule == "b":
        cv = max(c0, c1)
        if c0 != c1 and cv > F:
            return (1 if c1 > c0 else 0), 2 * cv > N + F
        return 2, False
    if c0 > F:
        return 0, True
    if c1 > F:
        return 1, True
    return (1 if c1 > c0 else 0 if c0 > c1 else 2), False


def class_round(rule, N, F, b, strategy, h, H):
    """One round's deterministic part from the class sizes H: per parity (action, decides)."""
    q = N - F
    P = [0, 0, 0]
    for pi in (0, 1):
        P[r_step(rule, *sched.counts(strategy, pi, q, H, b), N, F)] += h[pi]
    return [p_step(rule, *sched.counts(strategy, pi, q, P, b), N, F) for pi in (0, 1)]


def lumped_trial(rule, N, F, seed, trial, k_max, *, f=0, b=0, byz_even=0, byz_strategy=BALANCE, coin_common=0, init=None):
    """One trial of the lumped chain: (histogram bins it increments, rounds, a, dec).  init: None (random) or the
    counts (init0, init1, initq)."""
    q, h = sizes(N, F, f, b, byz_even)
    hh = h[0] + h[1]
    assert hh >= q >= 1 and min(h) >= 0
    if init is None:
        H1 = binom_half(hh, seed, trial, 0, 0)
        H = [hh - H1, H1, 0]
    else:
        assert sum(init) == hh
        H = list(init)
    a, dec, R = [0, 0], [False, False], 0
    for r in range(1, k_max + 1):
        acts = class_round(rule, N, F, b, byz_strategy, h, H)
        for pi in (0, 1):
            if h[pi] and acts[pi][1]:
                dec[pi] = True
        bit = None
        if any(h[pi] and acts[pi][0] == 2 for pi in (0, 1)):  # the round's word is drawn only if a parity takes the coin
            bit = coin_model.common_coin(seed, trial, r, coin_common)
        for pi in (0, 1):
            if h[pi] == 0:
                a[pi] = 0
            elif acts[pi][0] != 2:
                a[pi] = acts[pi][0] * h[pi]
            elif bit is not None:
                a[pi] = bit * h[pi]
            else:
                a[pi] = binom_half(h[pi], seed, trial, pi, r)
        H = [hh - a[0] - a[1], a[0] + a[1], 0]
        R = r
        if all(dec[pi] or not h[pi] for pi in (0, 1)):
            break
    all_dec = all(dec[pi] or not h[pi] for pi in (0, 1))
    K = a[0] + a[1]
    v = 2 if 0 < K < hh else (1 if K else 0)
    bins = [R * 3 + v] if all_dec else [v]
    if all_dec and v == 2:
        bins.append((k_max + 1) * 3)
    return bins, (R if all_dec else 0), tuple(a), tuple(dec)


def lumped_hist(rule, N, F, seed, trial_begin, trial_count, k_max, **kw):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for bn in lumped_trial(rule, N, F, seed, t, k_max, **kw)[0]:
            h[bn] += 1
    return h


# ------------------------------------------------------------ the exact law
@functools.lru_cache(maxsize=None)
def binom_pmf(n):
    return np.array([math.comb(n, k) / (1 << n) for k in range(n + 1)])    # (int / int: correctly rounded)


def exact_law(rule, N, F, b, h, strategy, k_max, coin_common=0, init=None):
    """The probability of every histogram bin (the last, the violations, is a marginal of the bins R * 3 + 2), by a
    DP over (A, dec_0, dec_1) with exact Binomial weights, A = a_0 + a_1: the next round reads A and the flags alone.
    h = (h_0, h_1); init None: H1 ~ Binomial(h, 1/2), else the three fixed counts."""
    hh = h[0] + h[1]
    pc = 1.0 if coin_common == ALL else coin_common / 2.0 ** 32
    p = np.zeros(oracle.hist_len(k_max))
    pmf = {n: binom_pmf(n) for n in (h[0], h[1], hh)}
    # a state: ((H0, H1, Hq) of the next R-phase, dec_0, dec_1) -> probability
    dist = {}
    if init is None:
        for H1, w in enumerate(pmf[hh]):
            dist[((hh - H1, H1, 0), False, False)] = float(w)
    else:
        dist[(tuple(init), False, False)] = 1.0
    for r in range(1, k_max + 1):
        nxt = {}
        for (H, d0, d1), w in dist.items():
            acts = class_round(rule, N, F, b, strategy, h, list(H))
            dec = (d0 or bool(h[0] and acts[0][1]), d1 or bool(h[1] and acts[1][1]))
            fixed = sum(acts[pi][0] * h[pi] for pi in (0, 1) if h[pi] and acts[pi][0] != 2)
            takers = [pi for pi in (0, 1) if h[pi] and acts[pi][0] == 2]
            out = {}                                             # A after the round -> probability
            if not takers:
                out[fixed] = 1.0
            else:
                n = sum(h[pi] for pi in takers)
                if pc > 0.0:
                    for v in (0, 1):
                        out[fixed + v * n] = out.get(fixed + v * n, 0.0) + pc / 2
                if pc < 1.0:                                    # independent coins: the takers' ones add up to Binomial(n, 1/2)
                    for k, wk in enumerate(np.convolve(pmf[h[takers[0]]], pmf[h[takers[1]]]) if len(takers) == 2
                                           else pmf[n]):
                        out[fixed + k] = out.get(fixed + k, 0.0) + (1.0 - pc) * float(wk)
            all_dec = all(dec[pi] or not h[pi] for pi in (0, 1))
            for A, wa in out.items():
                v = 2 if 0 < A < hh else (1 if A else 0)
                if all_dec:
                    p[r * 3 + v] += w * wa
                    if v == 2:
                        p[-1] += w * wa
                elif r == k_max:
                    p[v] += w * wa
                else:
                    key = ((hh - A, A, 0), dec[0], dec[1])
                    nxt[key] = nxt.get(key, 0.0) + w * wa
        dist = nxt
    assert abs(p[:-1].sum() - 1.0) < 1e-9
    return p


def gate(obs, p, label=""):
    """The law check: every bin within 6 sigma + 1 of its expectation, the bins with n p < 10 pooled into one.  The
    outcome bins partition the trials; the last bin is a marginal and is gated on its own."""
    obs = np.asarray(obs, dtype=np.float64)
    n = float(obs[:-1].sum())
    small = n * p[:-1] < 10.0
    cells = [(f"bin {i}", obs[i], p[i]) for i in np.flatnonzero(~small)]
    cells.append(("pooled", obs[:-1][small].sum(), p[:-1][small].sum()))
    cells.append(("violations", obs[-1], p[-1]))
    for name, o, pr in cells:
        pr = min(max(pr, 0.0), 1.0)
        bound = 6.0 * math.sqrt(n * pr * (1.0 - pr)) + 1.0
        print(f"{label} {name}: observed {o:.0f}, expected {n * pr:.2f}, bound {bound:.2f}")
        assert abs(o - n * pr) <= bound, (label, name, o, n * pr, bound)


def honest_sizes(N, faulty, byz):
    """(h_0, h_1) straight from a marking: the honest nodes by the parity of their compact index."""
    live = [i for i in range(N) if not faulty[i]]
    return tuple(sum(1 for c, i in enumerate(live) if not byz[i] and c & 1 == pi) for pi in (0, 1))


LAW_SHAPES = [(10, 4, 0, 0, 3000), (11, 2, 0, 2, 3000), (64, 12, 3, 9, 500)]     # (N, F, f, b, node-level trials)


def marking(N, f, b):
    return first(f, N), marks(set(range(f, f + b)), N)


@both_rules
@both_strategies
@pytest.mark.parametrize("N,F,f,b,trials", LAW_SHAPES)
def test_dp_is_the_law_of_modes_12_and_13(N, F, f, b, trials, name, rule):
    """Passes without the feature: mode 12/13's restatement, node by node with local coins, against the DP."""
    faulty, byz = marking(N, f, b)
    got = sched.sched_hist(rule, N, F, faulty, byz, SEED, 0, trials, 8, byz_strategy=STRATEGIES[name])
    gate(got, exact_law(rule, N, F, b, honest_sizes(N, faulty, byz), STRATEGIES[name], 8), f"{rule} {name} ({N}, {F})")


@both_rules
@both_strategies
@pytest.mark.parametrize("N,F,f,b,trials", LAW_SHAPES)
def test_lumped_restatement_has_the_same_law(N, F, f, b, trials, name, rule):
    api_exists()
    faulty, byz = marking(N, f, b)
    be = benor.byz_even(faulty, byz)
    h = honest_sizes(N, faulty, byz)
    assert sizes(N, F, f, b, be)[1] == h
    got = lumped_hist(rule, N, F, SEED, 0, 6000, 8, f=f, b=b, byz_even=be, byz_strategy=STRATEGIES[name])
    gate(got, exact_law(rule, N, F, b, h, STRATEGIES[name], 8), f"{rule} {name} ({N}, {F})")


@both_rules
def test_lumped_restatement_law_with_a_weak_coin_and_fixed_starts(rule):
    api_exists()
    got = lumped_hist(rule, 11, 2, SEED, 0, 6000, 8, b=2, byz_even=1, coin_common=HALF, init=(4, 4, 1))
    gate(got, exact_law(rule, 11, 2, 2, (5, 4), BALANCE, 8, coin_common=HALF, init=(4, 4, 1)), f"{rule} weak coin")


# ------------------------------------------------------------ exact coincidences with modes 12 and 13, per trial
def fixed_values(N, faulty, byz, init):
    """Per-node initial values that give the honest nodes the counts init = (zeros, ones, "?")."""
    vals = [0] * init[0] + [1] * init[1] + ["?"] * init[2]
    it = iter(vals)
    return [next(it) if not faulty[i] and not byz[i] else 0 for i in range(N)]


@both_rules
@both_strategies
@pytest.mark.parametrize("N,F,f,b,init", [(10, 4, 0, 0, (5, 5, 0)), (11, 2, 0, 2, (4, 4, 1)), (11, 2, 1, 1, (3, 6, 0)),
                                          (64, 12, 3, 9, (26, 26, 0)), (12, 2, 0, 2, (1, 1, 8))])
def test_shared_stream_gives_the_same_trials(N, F, f, b, init, name, rule):
    """Fixed starts and a coin common in every round: stream 12 is shared and no stream-13 word is drawn, so every
    trial's bins and rounds are mode 12/13's."""
    api_exists()
    faulty, byz = marking(N, f, b)
    be = benor.byz_even(faulty, byz)
    values = fixed_values(N, faulty, byz, init)
    for t in range(100):
        node = sched.sched_trial(rule, N, F, faulty, byz, SEED, t, 16, values, byz_strategy=STRATEGIES[name], coin_common=ALL)
        cls = lumped_trial(rule, N, F, SEED, t, 16, f=f, b=b, byz_even=be, byz_strategy=STRATEGIES[name], coin_common=ALL,
                           init=init)
        assert node[:2] == cls[:2], (t, node[:2], cls)
        honest = [s for i, s in enumerate(node[2]) if not faulty[i] and not byz[i]]
        assert sum(s["x"] for s in honest) == sum(cls[2])


@both_strategies
@pytest.mark.parametrize("coin", [0, ALL])
@pytest.mark.parametrize("v", [0, 1])
@pytest.mark.parametrize("N,F,f,b", sched.RULE_B_SHAPES + [(1 << 20, 209715, 0, 16)])
def test_rule_b_unanimous_start_decides_in_round_1(N, F, f, b, v, coin, name):
    api_exists()
    hh = N - f - b
    init = (0, hh, 0) if v else (hh, 0, 0)
    h = lumped_hist("b", N, F, SEED, 0, 50, 16, f=f, b=b, byz_even=(b + 1) // 2, byz_strategy=STRATEGIES[name],
                    coin_common=coin, init=init)
    assert int(h[3 + v]) == 50 and int(h.sum()) == 50


@both_strategies
@pytest.mark.parametrize("coin", [0, HALF])
@pytest.mark.parametrize("N,F,f,b", sched.RULE_B_SHAPES + [(1 << 16, 13000, 100, 12000)])
def test_rule_b_is_safe(N, F, f, b, coin, name):
    """Rule B with N > 5F: the last bin and every bin R * 3 + 2 are zero."""
    api_exists()
    h = lumped_hist("b", N, F, SEED, 0, 300, 16, f=f, b=b, byz_even=b // 2, byz_strategy=STRATEGIES[name], coin_common=coin)
    assert int(h[:-1].sum()) == 300 and mode9.forbidden_bins(h) == 0


# ------------------------------------------------------------ the tables
def exact_thresholds(k):
    """floor(CDF(x) 2^64) of Binomial(2^k, 1/2) for every x, in integers."""
    n = 1 << k
    out, run = [], 0
    for x in range(n + 1):
        run += math.comb(n, x)
        out.append(min((1 << 64) - 1, (run << 64) >> n))
    return out


TABLE_BOUND = 1 << 16        # a double leaves 2^11 units at CDF ~ 1/2; five more bits for accumulation


@pytest.mark.parametrize("k", range(7, 13))
def test_tables_against_exact_integers(k):
    lo, thr = table(k)
    exact = exact_thresholds(k)
    assert all(t == 0 for t in exact[:lo]) or max(exact[:lo]) <= TABLE_BOUND        # trimmed where the threshold is 0
    worst = max(abs(t - exact[lo + i]) for i, t in enumerate(thr))
    print(f"k = {k}: {len(thr)} thresholds from {lo}, largest deviation {worst}")
    assert worst <= TABLE_BOUND
    assert thr[0] > 0 and thr[-1] < (1 << 64) - 1
    assert all(t >= (1 << 64) - 1 - TABLE_BOUND for t in exact[lo + len(thr):])       # ... or saturated


@pytest.mark.parametrize("k", range(7, 25))
def test_tables_structure(k):
    lo, thr = table(k)
    n, full = 1 << k, 1 << 64
    assert len(thr) > 0 and all(a <= b for a, b in zip(thr, thr[1:]))               # nondecreasing
    assert 0 < thr[0] and thr[-1] < full - 1                                       # trimmed
    cdf = {lo + i: v for i, v in enumerate(thr)}

    def at(x):
        return 0 if x < lo else cdf.get(x, full)

    # (bo_binom_half_cdf builds the upper half as the mirror image of the lower, so the symmetry and the mean hold by
    # construction up to the floor / ceil of each entry; the variance is what constrains the pmf's shape here, and
    # test_tables_against_exact_integers the values themselves for k <= 12)
    for x in range(lo, lo + len(thr)):                                             # symmetric: CDF(x) + CDF(n - 1 - x) = 1
        assert abs(at(x) + at(n - 1 - x) - full) <= TABLE_BOUND, x
    # the implied pmf: mean 2^(k-1), variance 2^(k-2), to relative 2^-40 (integers over 2^64)
    xs = list(range(lo, lo + len(thr) + 1))
    pm = [at(x) - at(x - 1) for x in xs]
    assert sum(pm) == full
    mean_num = sum(x * w for x, w in zip(xs, pm))
    var_num = sum((2 * x - n) ** 2 * w for x, w in zip(xs, pm))                     # 4 Var, around n / 2
    assert abs(mean_num - (n // 2) * full) * (1 << 40) <= (n // 2) * full
    assert abs(var_num - n * full) * (1 << 40) <= n * full


def test_binom_half_cdf_arguments():
    api_exists()
    L = benor.lib()
    import ctypes

    lo, n = ctypes.c_uint32(), ctypes.c_uint32()
    thr = (ctypes.c_uint64 * 8)()
    for k in (0, 6, 25, 64):
        assert L.bo_binom_half_cdf(k, ctypes.byref(lo), thr, 8, ctypes.byref(n)) == benor.BO_ERR_INVALID_ARGUMENT
        assert "7 <= k <= 24" in benor.last_error()
    assert L.bo_binom_half_cdf(7, ctypes.byref(lo), thr, 8, ctypes.byref(n)) == benor.BO_ERR_INVALID_ARGUMENT
    assert "too short" in benor.last_error()
    assert L.bo_binom_half_cdf(7, None, thr, 8, ctypes.byref(n)) == benor.BO_ERR_INVALID_ARGUMENT


def test_draw_restatement_small_bits_are_popcounts():
    """k <= 6 against popcounts of the words, and the word order: n = 75 takes words 0..3 of blocks 0 and 1."""
    api_exists()
    t, r, pi = 2 ** 32 + 5, 3, 1
    b0 = philox(SEED, (t & 0xFFFFFFFF, t >> 32, 16, r | 13 << 24))
    b1 = philox(SEED, (t & 0xFFFFFFFF, t >> 32, 17, r | 13 << 24))
    w = [b0[1] << 32 | b0[0], b0[3] << 32 | b0[2], b1[1] << 32 | b1[0], b1[3] << 32 | b1[2]]
    want = sum(bin(w[j] & ((1 << (1 << k)) - 1)).count("1") for j, k in enumerate((0, 1, 3, 6)))
    assert binom_half(75, SEED, t, pi, r) == want
    assert binom_half(0, SEED, t, pi, r) == 0


def test_diagram_agrees_with_the_node_level():
    """results/r21_sweep_lumped_balance.csv (the class level, N = 2^6 .. 2^24) against results/r20_sweep_sched_balance.csv
    (mode 12, another stream) at the cells they share: the undecided counts within the two-sample 6 sigma gate."""
    import csv

    def rows(name):
        with open(os.path.join(ROOT, "results", name)) as f:
            return {(int(r["N"]), int(r["F"])): r for r in csv.DictReader(f)}

    cls, node = rows("r21_sweep_lumped_balance.csv"), rows("r20_sweep_sched_balance.csv")
    assert {N for N, _ in cls} == {4 ** k for k in range(3, 13)} and all(r["level"] == "class" for r in cls.values())
    shared = sorted(set(cls) & set(node))
    assert {N for N, _ in shared} == {64, 256, 1024} and len(shared) >= 36
    for key in shared:
        n = int(cls[key]["trials"])
        assert n == int(node[key]["trials"]) == 20000
        u1, u2 = int(cls[key]["undecided"]), int(node[key]["undecided"])
        p = (u1 + u2) / (2 * n)
        assert abs(u1 - u2) <= 6.0 * math.sqrt(2 * n * p * (1 - p)) + 1.0, (key, u1, u2)


# ------------------------------------------------------------ the host program, validation, ABI, CLI
def test_lumped_header_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "lumped_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "lumped_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.split()[0]) >= 100 and " 0 failures" in r.stdout, r.stdout


GOOD = dict(b=2, byz_even=1, rule=0, byz_strategy=BALANCE, k_max=16)


def test_validation_needs_no_device():
    api_exists()
    benor.LumpedPlan(11, 2, **GOOD)
    benor.LumpedPlan(1 << 24, 3355443, k_max=32)                                  # the top of the admitted range
    benor.LumpedPlan(5000, 1000, b=16, byz_even=8, byz_strategy=SPLIT, rule=1)
    bad = [
        (dict(N=0), "N must be"), (dict(N=(1 << 24) + 1), "N must be"), (dict(F=11), "F must be below N"),
        (dict(byz_even=3), "byz_even must be"), (dict(N=3, F=2, byz_even=0), "b - byz_even must be"),
        (dict(byz_strategy=0), "strategy must be"), (dict(byz_strategy=1), "strategy must be"),
        (dict(byz_strategy=2), "strategy must be"), (dict(byz_strategy=5), "strategy must be"),
        (dict(rule=2), "rule must be"), (dict(k_max=0), "k_max must be"), (dict(k_max=1025), "k_max must be"),
        (dict(initial_values=(4, 4, 0)), r"init0 \+ init1 \+ initq must be"),
        (dict(initial_values=(0xFFFFFFFF, 10, 0)), r"init0 \+ init1 \+ initq must be"),
    ]
    for change, text in bad:
        kw = dict(GOOD, N=11, F=2)
        kw.update(change)
        N, F = kw.pop("N"), kw.pop("F")
        with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}: bo_lumped.*{text}"):
            benor.LumpedPlan(N, F, **kw)
    with pytest.raises(benor.Error, match="bo_lumped needs at most F nodes crashed or Byzantine"):
        benor.LumpedPlan(11, 2, **dict(GOOD, f=1))
    with pytest.raises(ValueError, match="three counts"):
        benor.LumpedPlan(11, 2, initial_values=(1, 2))
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        benor.LumpedPlan(11, 2, coin_common=ALL + 1)
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        benor.LumpedPlan(11, -1)
    assert benor.lib().bo_lumped_check(None) == benor.BO_ERR_INVALID_ARGUMENT
    assert benor.lib().bo_abi_version() == 8                                      # bo_trials_cfg is as it was
    assert benor.BO_MAX_N == 4096 and benor.LUMPED_MAX_N == 1 << 24


def test_byz_even_of_a_marking():
    api_exists()
    assert benor.byz_even(first(0, 11), marks({3}, 11)) == 0
    assert benor.byz_even(first(0, 11), marks({4}, 11)) == 1
    assert benor.byz_even(first(0, 11), marks({3, 8}, 11)) == 1
    assert benor.byz_even(first(3, 64), marks(set(range(3, 12)), 64)) == 5         # compact 0..8
    assert benor.byz_even(first(1, 11), marks({3}, 11)) == 1                       # node 3 is compact index 2
    assert benor.byz_even([0, 2, 1, 2, 0, 2]) == 2                              # raw bytes: compact 1, 2 and 4 lie
    assert benor.byz_even([False] * 200, marks(set(range(64, 128)), 200)) == 32


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                          env=env, cwd=ROOT)


def test_cli_class_level_lifts_the_size_limit():
    api_exists()
    big = ("trials", "--N", "5000", "--F", "1000", "--trials", "10", "--crashed", "0", "--mode", "byz", "--delivery",
           "adversarial", "--byz-strategy", "balance")
    p = _cli(*big, "--level", "class")                    # accepted: it runs, or gets as far as the missing device
    assert "N must be" not in p.stderr
    assert p.returncode == 0 or "libbenor error 4" in p.stderr, p.stderr


def test_cli_argument_errors_need_no_device():
    api_exists()
    big = ("trials", "--N", "5000", "--F", "1000", "--trials", "10", "--crashed", "0", "--mode", "byz", "--delivery",
           "adversarial", "--byz-strategy", "balance")
    for level in ((), ("--level", "node")):               # rejected as before
        p = _cli(*big, *level)
        assert p.returncode != 0 and "N must be in [1, 4096]" in p.stderr
    p = _cli(*big[:2], str((1 << 24) + 1), *big[3:], "--level", "class")
    assert p.returncode != 0 and "bo_lumped: N must be" in p.stderr
    base = ("trials", "--N", "11", "--F", "2", "--trials", "10", "--crashed", "0")
    p = _cli(*base, "--level", "class")
    assert p.returncode != 0 and "--level class needs --mode byz or --mode byzb with --delivery adversarial" in p.stderr
    p = _cli(*base, "--mode", "byz", "--byz-strategy", "split", "--level", "class")
    assert p.returncode != 0 and "--level class needs" in p.stderr
    p = _cli(*base, "--mode", "tally3", "--delivery", "adversarial", "--level", "class")
    assert p.returncode != 0 and "--delivery adversarial needs --mode byz or --mode byzb" in p.stderr
    adv = (*base, "--mode", "byzb", "--delivery", "adversarial", "--level", "class")
    p = _cli(*adv, "--byz-strategy", "oppose")
    assert p.returncode != 0 and "--delivery adversarial needs --byz-strategy balance" in p.stderr
    p = _cli(*adv, "--byz-strategy", "split", "--byzantine", "12")
    assert p.returncode != 0 and "--byzantine counts live nodes" in p.stderr
    p = _cli(*adv, "--byz-strategy", "split", "--byzantine", "3")
    assert p.returncode != 0 and "bo_lumped needs at most F nodes crashed or Byzantine" in p.stderr
    p = _cli(*adv, "--byz-strategy", "split", "--coin-common", "1.5")
    assert p.returncode != 0 and "--coin-common is a probability in [0, 1]" in p.stderr
    p = _cli(*adv, "--byz-strategy", "split", "--level", "group")
    assert p.returncode != 0 and "invalid choice" in p.stderr
    sweep = ("sweep", "--N", "16", "--steps", "2", "--trials", "10")
    p = _cli(*sweep, "--level", "class")
    assert p.returncode != 0 and "--level class needs" in p.stderr
    p = _cli(*sweep, "--mode", "byz", "--byz-strategy", "balance", "--level", "class")
    assert p.returncode != 0 and "--level class needs" in p.stderr
