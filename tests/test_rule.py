"""Threshold rules on the count-level modes: Protocol A and any rule of three words (CPU suite).

The definition (include/benor.h), restated here in plain Python over the existing restatements'
helpers -- test_byz_sched.counts, test_byz_coin.common_coin, the draws of test_byz_coin.coin_trial, test_lumped's
binom_half -- and nothing from the kernel; tests/test_rule_gpu.py checks the kernels against it bit for bit.  A
rule is three words (propose_gt2, adopt_gt, decide_gt2).  With v the value of the strictly larger count (none on
c0 == c1, an empty tally included):

    R-phase: propose v iff v exists and 2 c_v > propose_gt2, else "?";
    P-phase: if v exists and c_v > adopt_gt: x = v, decided iff also 2 c_v > decide_gt2; else the node's coin.

Presets: Protocol A (N, 0, 2F); Protocol B (N + F, F, N + F), mode 9's rule at every count; (0, 0, 2F), the
reference's rule whenever N <= 3F + 1.  The _rule entries run modes 9, 11 and 13 and the lumped chain with the
rule replaced and everything else -- strategies, streams, coins, states, bins -- as it is.
"""
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
import test_byz_heard as heard
import test_byz_rule_b as mode9
import test_byz_sched as sched
import test_byz_tally as mode8
import test_lumped as lumped_model
from conftest import PKG, ROOT
from test_tally import first, philox
from test_tally3 import draw3

RANDOM, OPPOSE, BALANCE, SPLIT = 0, 1, 3, 4
SCHED_STRATEGIES = sched.STRATEGIES
ALL_STRATEGIES = coin_model.STRATEGIES
SEED = mode8.SEED
ALL, HALF = mode8.ALL, mode8.HALF
Q = "?"
marks = mode8.marks
CSRC = os.path.join(PKG, "csrc")
both_strategies = sched.both_strategies
every_strategy = coin_model.every_strategy
both_coins = pytest.mark.parametrize("coin", [0, ALL])


def api_exists():
    for name in ("Rule", "rule_protocol_a", "rule_protocol_b"):
        assert hasattr(benor, name), name              # absent before the feature: every test that needs it fails


# ------------------------------------------------------------ the rule, from the header's text
def protocol_a(N, F):
    return (N, 0, 2 * F)


def protocol_b(N, F):
    return (N + F, F, N + F)


def reference(N, F):
    return (0, 0, 2 * F)


def larger(c0, c1):
    """(v, c_v) of the strictly larger count, or (None, 0)."""
    return (1, c1) if c1 > c0 else (0, c0) if c0 > c1 else (None, 0)


def r_step(words, c0, c1):
    v, cv = larger(c0, c1)
    return v if v is not None and 2 * cv > words[0] else 2


def p_step(words, c0, c1):
    """(the new x or 2 for "takes the coin", whether the counts decide)."""
    v, cv = larger(c0, c1)
    if v is not None and cv > words[1]:
        return v, 2 * cv > words[2]
    return 2, False


# ------------------------------------------------------------ restatement, node level
def node_trial(words, N, F, faulty, byzantine, seed, trial, k_max, initial_values, coin_common, counts_of):
    """One trial of a Byzantine mode's plan with its rule replaced: (histogram bins it increments, rounds, per-node
    states).  counts_of(r, H, c, phase) gives honest receiver c its (c0, c1) from the honest class sizes H."""
    live = [i for i in range(N) if not faulty[i]]
    honest = [c for c, i in enumerate(live) if not byzantine[i]]
    m, b = len(live), len(live) - len(honest)
    assert not any(faulty[i] and byzantine[i] for i in range(N)) and (N - m) + b <= F
    states = [{"killed": bool(faulty[i]), "x": None, "decided": None, "k": None} for i in range(N)]
    if not honest:
        return [2], 0, states
    if initial_values is None:
        x = {c: oracle.random_init(seed, trial, c, m) for c in honest}
    else:
        x = {c: 2 if initial_values[live[c]] == Q else initial_values[live[c]] for c in honest}
    dec = {c: False for c in honest}
    R = 0

    def sizes(vals):
        H = [0, 0, 0]
        for v in vals.values():
            H[v] += 1
        return H

    for r in range(1, k_max + 1):
        H = sizes(x)
        prop = {c: r_step(words, *counts_of(r, H, c, 0)) for c in honest}
        H = sizes(prop)
        new, took = {}, []
        for c in honest:
            act, decides = p_step(words, *counts_of(r, H, c, 1))
            if act == 2:
                took.append(c)
            else:
                new[c] = act
                dec[c] = dec[c] or decides
        if took:                                             # the round's word is drawn only if somebody takes a coin
            bit = coin_model.common_coin(seed, trial, r, coin_common)
            for c in took:
                new[c] = oracle.coin(seed, trial, c, r) if bit is None else bit
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


def sched_trial(words, N, F, faulty, byzantine, seed, trial, k_max, initial_values=None, byz_strategy=BALANCE,
                coin_common=0):
    """Mode 13's plan with the rule `words`: the adversarial scheduler's closed forms (test_byz_sched.counts)."""
    assert byz_strategy in (BALANCE, SPLIT)
    q = N - F
    b = sum(1 for i in range(N) if byzantine[i] and not faulty[i])
    cache = {}

    def counts_of(r, H, c, phase):
        key = (r, phase, c & 1)                              # a step's counts: one pair per parity of c
        if key not in cache:
            cache[key] = sched.counts(byz_strategy, c & 1, q, H, b)
        return cache[key]

    return node_trial(words, N, F, faulty, byzantine, seed, trial, k_max, initial_values, coin_common, counts_of)


def coin_trial(words, N, F, faulty, byzantine, seed, trial, k_max, initial_values=None, byz_one=0, byz_strategy=RANDOM,
               coin_common=0):
    """Mode 9's plan (coin_common 0) or mode 11's with the rule `words`: random delivery, the draws of
    test_byz_coin.coin_trial word for word."""
    live = [i for i in range(N) if not faulty[i]]
    m, q = len(live), N - F
    b = sum(1 for i in live if byzantine[i])
    tlo, thi = trial & 0xFFFFFFFF, trial >> 32
    blocks, lie = {}, {}

    def counts_of(r, H, c, phase):
        if (r, c) not in blocks:
            blocks[r, c] = philox(seed, (tlo, thi, c, (r - 1) | coin_model.STREAM_TALLY << 24))
        s = blocks[r, c]
        u5 = s[3] << 32 | s[2] if phase else s[1] << 32 | s[0]
        if b == 0:                                           # nobody lies: mode 4's draw, no stream-10 or stream-11 word
            return draw3(m, q, (H[0], H[1], H[2]), seed, trial, c, r, phase, u5)
        if byz_strategy in (BALANCE, SPLIT):                 # the liars see the inbox
            h0, h1 = draw3(m, q, (H[0], H[1], H[2] + b), seed, trial, c, r, phase, u5)
            nB = heard.heard_byz(H[2], b, q - h0 - h1, seed, trial, c, r, phase)
            l1 = heard.heard_lies(byz_strategy, c, h0, h1, nB)
            return h0 + nB - l1, h1 + l1

        def u():
            if (r, c) not in lie:
                lie[r, c] = philox(seed, (tlo, thi, c, (r - 1) | coin_model.STREAM_LIE << 24))
            w = lie[r, c]
            return w[3] << 32 | w[2] if phase else w[1] << 32 | w[0]
        B1 = mode8.lies(b, byz_one, byz_strategy, H[0], H[1], u)
        return draw3(m, q, (H[0] + b - B1, H[1] + B1, H[2]), seed, trial, c, r, phase, u5)

    return node_trial(words, N, F, faulty, byzantine, seed, trial, k_max, initial_values, coin_common, counts_of)


def hist_of(trial_fn, k_max, trial_begin, trial_count):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in trial_fn(t)[0]:
            h[b] += 1
    return h


def sched_hist(words, N, F, faulty, byzantine, seed, trial_begin, trial_count, k_max, initial_values=None, **kw):
    return hist_of(lambda t: sched_trial(words, N, F, faulty, byzantine, seed, t, k_max, initial_values, **kw), k_max,
                   trial_begin, trial_count)


# ------------------------------------------------------------ restatement, class level
def class_round(words, N, F, b, strategy, h, H):
    """One round's deterministic part from the class sizes H: per parity (action, decides)."""
    q = N - F
    P = [0, 0, 0]
    for pi in (0, 1):
        P[r_step(words, *sched.counts(strategy, pi, q, H, b))] += h[pi]
    return [p_step(words, *sched.counts(strategy, pi, q, P, b)) for pi in (0, 1)]


def lumped_trial(words, N, F, seed, trial, k_max, *, f=0, b=0, byz_even=0, byz_strategy=BALANCE, coin_common=0, init=None):
    """One trial of the lumped chain under the rule `words`: (bins, rounds, a, dec); test_lumped.lumped_trial with
    the rule's two steps replaced."""
    q, h = lumped_model.sizes(N, F, f, b, byz_even)
    hh = h[0] + h[1]
    assert hh >= q >= 1 and min(h) >= 0
    if init is None:
        H1 = lumped_model.binom_half(hh, seed, trial, 0, 0)
        H = [hh - H1, H1, 0]
    else:
        assert sum(init) == hh
        H = list(init)
    a, dec, R = [0, 0], [False, False], 0
    for r in range(1, k_max + 1):
        acts = class_round(words, N, F, b, byz_strategy, h, H)
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
                a[pi] = lumped_model.binom_half(h[pi], seed, trial, pi, r)
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


def lumped_hist(words, N, F, seed, trial_begin, trial_count, k_max, **kw):
    return hist_of(lambda t: lumped_trial(words, N, F, seed, t, k_max, **kw), k_max, trial_begin, trial_count)


# ------------------------------------------------------------ the exact law (test_lumped.exact_law over three words)
def exact_law(words, N, F, b, h, strategy, k_max, coin_common=0, init=None):
    """The probability of every histogram bin by the DP over (A, dec_0, dec_1) with exact Binomial weights."""
    hh = h[0] + h[1]
    pc = 1.0 if coin_common == ALL else coin_common / 2.0 ** 32
    p = np.zeros(oracle.hist_len(k_max))
    pmf = {n: lumped_model.binom_pmf(n) for n in (h[0], h[1], hh)}
    dist = {}
    if init is None:
        for H1, w in enumerate(pmf[hh]):
            dist[((hh - H1, H1, 0), False, False)] = float(w)
    else:
        dist[(tuple(init), False, False)] = 1.0
    for r in range(1, k_max + 1):
        nxt = {}
        for (H, d0, d1), w in dist.items():
            acts = class_round(words, N, F, b, strategy, h, list(H))
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


@functools.lru_cache(maxsize=None)
def shared_hist(words, N, F, f, b, name, coin_common, k_max=32, trials=300):
    """`trials` node-level trials from trial 0 at SEED under the scheduler, the first f nodes crashed and the next b
    Byzantine: computed once."""
    h = sched_hist(words, N, F, first(f, N), marks(set(range(f, f + b)), N), SEED, 0, trials, k_max,
                   byz_strategy=SCHED_STRATEGIES[name], coin_common=coin_common)
    h.setflags(write=False)
    return h


# ---------------------------------------------------------------- the tests
# ---- the host program over csrc/benor_rule.h
def test_rule_header_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "rule_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "rule_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.split()[0]) >= 10000 and " 0 failures" in r.stdout, r.stdout


# ---- the rule's text against the existing restatements' two rules
def test_presets_restate_the_two_rules_at_every_count():
    """Protocol B's words against test_lumped's rule "b" at every (c0, c1) with c0 + c1 <= N, N <= 24; (0, 0, 2F)
    against rule "ref" for N <= 3F + 1, and the count at which they part above it."""
    for N in range(1, 25):
        for F in range(N):
            for c0 in range(N + 1):
                for c1 in range(N + 1 - c0):
                    wb = protocol_b(N, F)
                    assert r_step(wb, c0, c1) == lumped_model.r_step("b", c0, c1, N, F)
                    assert p_step(wb, c0, c1) == lumped_model.p_step("b", c0, c1, N, F)
                    if N <= 3 * F + 1 and c0 + c1 <= N - F:
                        wr = reference(N, F)
                        assert r_step(wr, c0, c1) == lumped_model.r_step("ref", c0, c1, N, F)
                        assert p_step(wr, c0, c1) == lumped_model.p_step("ref", c0, c1, N, F), (N, F, c0, c1)
    N, F = 5, 1                                               # N = 3F + 2: q = 4 holds F + 1 of both values
    assert lumped_model.p_step("ref", 2, 2, N, F) == (0, True) and p_step(reference(N, F), 2, 2) == (2, False)


# ---- per-node equality with the existing restatements
B_SHAPES = [(10, 4, 0, 0, 40), (11, 2, 0, 2, 40), (64, 12, 3, 9, 12)]        # (N, F, f, b, trials)
REF_SHAPES = [(10, 4, 0, 2, 40), (64, 21, 0, 4, 12)]                         # N <= 3F + 1


def marking(N, f, b):
    return first(f, N), marks(set(range(f, f + b)), N)


@both_coins
@both_strategies
@pytest.mark.parametrize("N,F,f,b,trials", B_SHAPES)
def test_protocol_b_words_are_mode_13(N, F, f, b, trials, name, coin):
    faulty, byz = marking(N, f, b)
    kw = dict(byz_strategy=SCHED_STRATEGIES[name], coin_common=coin)
    for t in range(trials):
        assert sched_trial(protocol_b(N, F), N, F, faulty, byz, SEED, t, 16, **kw) == \
            sched.sched_trial("b", N, F, faulty, byz, SEED, t, 16, **kw), t


@both_coins
@both_strategies
@pytest.mark.parametrize("N,F,f,b,trials", REF_SHAPES)
def test_reference_words_are_mode_12(N, F, f, b, trials, name, coin):
    faulty, byz = marking(N, f, b)
    kw = dict(byz_strategy=SCHED_STRATEGIES[name], coin_common=coin)
    for t in range(trials):
        assert sched_trial(reference(N, F), N, F, faulty, byz, SEED, t, 16, **kw) == \
            sched.sched_trial("ref", N, F, faulty, byz, SEED, t, 16, **kw), t


@both_coins
@every_strategy
@pytest.mark.parametrize("N,F,f,b,trials", B_SHAPES)
def test_protocol_b_words_are_modes_9_and_11(N, F, f, b, trials, name, coin):
    faulty, byz = marking(N, f, b)
    kw = dict(byz_one=HALF, byz_strategy=ALL_STRATEGIES[name], coin_common=coin)
    for t in range(trials):
        assert coin_trial(protocol_b(N, F), N, F, faulty, byz, SEED, t, 16, **kw) == \
            coin_model.coin_trial("b", N, F, faulty, byz, SEED, t, 16, **kw), t


@both_coins
@every_strategy
@pytest.mark.parametrize("N,F,f,b,trials", REF_SHAPES)
def test_reference_words_are_modes_8_and_10(N, F, f, b, trials, name, coin):
    faulty, byz = marking(N, f, b)
    kw = dict(byz_one=HALF, byz_strategy=ALL_STRATEGIES[name], coin_common=coin)
    for t in range(trials):
        assert coin_trial(reference(N, F), N, F, faulty, byz, SEED, t, 16, **kw) == \
            coin_model.coin_trial("ref", N, F, faulty, byz, SEED, t, 16, **kw), t


@both_coins
@both_strategies
@pytest.mark.parametrize("rule,N,F,f,b", [("b", N, F, f, b) for N, F, f, b, _ in B_SHAPES] +
                         [("ref", N, F, f, b) for N, F, f, b, _ in REF_SHAPES])
def test_preset_words_are_the_lumped_chain(rule, N, F, f, b, name, coin):
    words = protocol_b(N, F) if rule == "b" else reference(N, F)
    kw = dict(f=f, b=b, byz_even=(b + 1) // 2, byz_strategy=SCHED_STRATEGIES[name], coin_common=coin)
    for t in range(60):
        assert lumped_trial(words, N, F, SEED, t, 16, **kw) == lumped_model.lumped_trial(rule, N, F, SEED, t, 16, **kw), t


# ---- Protocol A proposes one value
def test_protocol_a_proposes_a_single_value():
    """Every N <= 10, F < N / 2, f <= F and honest class sizes with b = 0: over every feasible inbox
    (test_byz_sched.inboxes), no two receivers can be made to propose different values."""
    checked = 0
    for N in range(1, 11):
        for F in range((N + 1) // 2):                        # 2F < N
            for f in range(F + 1):
                q, h = N - F, N - f
                for H in sched.class_sizes(h):
                    props = {r_step(protocol_a(N, F), c0, c1) for c0, c1 in sched.inboxes(q, H, 0)} - {2}
                    assert len(props) <= 1, (N, F, f, H, props)
                    checked += 1
    assert checked > 1000
    # the bare majority, the reference's R-step, has no such property: (10, 4) with five of each
    assert {r_step(reference(10, 4), c0, c1) for c0, c1 in sched.inboxes(6, (5, 5, 0), 0)} >= {0, 1}


# ---- safety under SPLIT
@pytest.mark.parametrize("N,F", [(10, 4), (64, 20), (64, 31)])
def test_protocol_a_is_safe_under_split_without_a_byzantine_node(N, F):
    """b = 0, 300 trials, k_max 32: no trial in the violation bin (a theorem for N > 2F: it holds on any stream),
    where the reference's rule breaks agreement (test_byz_sched)."""
    h = shared_hist(protocol_a(N, F), N, F, 0, 0, "SPLIT", 0)
    ref = shared_hist(reference(N, F), N, F, 0, 0, "SPLIT", 0)
    print(f"({N}, {F}) split: Protocol A {int(h[-1])} violations of 300, (0, 0, 2F) {int(ref[-1])}, "
          f"undecided {heard.undecided(h)} and {heard.undecided(ref)}")
    assert int(h[:-1].sum()) == 300 and int(h[-1]) == 0 and mode9.forbidden_bins(h, 32) == 0
    assert int(ref[-1]) > 150


def test_protocol_a_is_not_built_for_byzantine_nodes():
    """(64, 12, b = 12) under SPLIT: Protocol A violates agreement in more than half the trials, Protocol B in none."""
    a = shared_hist(protocol_a(64, 12), 64, 12, 0, 12, "SPLIT", 0)
    b = shared_hist(protocol_b(64, 12), 64, 12, 0, 12, "SPLIT", 0)
    print(f"(64, 12, 12) split: Protocol A {int(a[-1])} violations of 300, Protocol B {int(b[-1])}")
    assert int(a[:-1].sum()) == 300 and int(a[-1]) > 150
    assert int(b[-1]) == 0 and mode9.forbidden_bins(b, 32) == 0


# ---- the boundary under BALANCE
@pytest.mark.parametrize("N,F", [(64, 8), (256, 16)])
def test_balance_stalls_protocol_a_at_half_the_f(N, F):
    """F = sqrt N, b = 0, local coins, 300 trials, k_max 32: more than 40 trials undecided under Protocol A, fewer than
    5 under (0, 0, 2F) -- the scheduler hides a majority from Protocol A while the deviation from h / 2 is at most F,
    from the bare-majority rule while it is at most F / 2."""
    a = shared_hist(protocol_a(N, F), N, F, 0, 0, "BALANCE", 0)
    ref = shared_hist(reference(N, F), N, F, 0, 0, "BALANCE", 0)
    print(f"({N}, {F}) balance: undecided {heard.undecided(a)} of 300 under Protocol A, {heard.undecided(ref)} under (0, 0, 2F)")
    assert int(a[:-1].sum()) == 300 and int(ref[:-1].sum()) == 300
    assert heard.undecided(a) > 40
    assert heard.undecided(ref) < 5
    assert int(a[-1]) == 0


# ---- the exact law
LAW_SHAPES = [(10, 4, 0, 0, 3000), (11, 5, 0, 0, 3000), (64, 12, 3, 9, 500)]   # (N, F, f, b, node-level trials)
law_coins = pytest.mark.parametrize("coin", [0, HALF])


@law_coins
@both_strategies
@pytest.mark.parametrize("N,F,f,b,trials", LAW_SHAPES)
def test_node_level_restatement_has_the_exact_law(N, F, f, b, trials, name, coin):
    faulty, byz = marking(N, f, b)
    words = protocol_a(N, F)
    got = sched_hist(words, N, F, faulty, byz, SEED, 0, trials, 8, byz_strategy=SCHED_STRATEGIES[name], coin_common=coin)
    law = exact_law(words, N, F, b, lumped_model.honest_sizes(N, faulty, byz), SCHED_STRATEGIES[name], 8, coin_common=coin)
    lumped_model.gate(got, law, f"A {name} ({N}, {F})")


@law_coins
@both_strategies
@pytest.mark.parametrize("N,F,f,b,trials", LAW_SHAPES)
def test_lumped_restatement_has_the_exact_law(N, F, f, b, trials, name, coin):
    faulty, byz = marking(N, f, b)
    words = protocol_a(N, F)
    h = lumped_model.honest_sizes(N, faulty, byz)
    be = (b + 1) // 2                                         # compact indices 0 .. b - 1 lie
    assert lumped_model.sizes(N, F, f, b, be)[1] == h
    got = lumped_hist(words, N, F, SEED, 0, 6000, 8, f=f, b=b, byz_even=be, byz_strategy=SCHED_STRATEGIES[name],
                      coin_common=coin)
    lumped_model.gate(got, exact_law(words, N, F, b, h, SCHED_STRATEGIES[name], 8, coin_common=coin), f"A {name} ({N}, {F})")


def test_exact_law_at_the_preset_words_is_test_lumpeds():
    for rule, words in (("b", protocol_b(11, 2)), ("ref", reference(10, 4))):
        N, F = (11, 2) if rule == "b" else (10, 4)
        for strategy in (BALANCE, SPLIT):
            assert np.array_equal(exact_law(words, N, F, 0, (5, N - 5), strategy, 8, coin_common=HALF),
                                  lumped_model.exact_law(rule, N, F, 0, (5, N - 5), strategy, 8, coin_common=HALF))


# ---- plumbing: presets, validation, ABI, CLI
def test_presets_and_the_rule_type():
    api_exists()
    assert benor.rule_protocol_a(64, 20).words == protocol_a(64, 20) == (64, 0, 40)
    assert benor.rule_protocol_b(64, 12).words == protocol_b(64, 12) == (76, 12, 76)
    assert benor.rule_protocol_a(1 << 24, 3355443).words == (1 << 24, 0, 6710886)
    assert benor.rule_protocol_a(10, 4) == benor.Rule(10, 0, 8, 0) and benor.rule_protocol_a(10, 4) != benor.Rule(10, 0, 8, 1)
    with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}: bo_rule"):
        benor.rule_protocol_b((1 << 31) - 1, 1)
    assert benor.lib().bo_rule_protocol_a(10, 4, None) == benor.BO_ERR_INVALID_ARGUMENT
    assert benor.lib().bo_abi_version() == 8                  # bo_trials_cfg and bo_lumped_cfg are as they were
    assert benor.BO_MODE_SCHED_RULE_B == 13 and max(benor.KERNEL_NAMES) == 21   # no mode, no kernel value added


BIG = 1 << 31


def test_validation_needs_no_device():
    api_exists()
    bad = [((BIG, 0, 0), "propose_gt2"), ((0, BIG, 0), "adopt_gt"), ((0, 0, BIG), "decide_gt2"),
           ((0xFFFFFFFF, 0, 0), "propose_gt2"), (benor.Rule(10, 0, 8, 1), "reserved")]
    byz = dict(byzantine=marks({3}, 11), byz_strategy=SPLIT)
    for thresholds, word in bad:
        want = f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}: bo_rule: {word} must be"
        for mode in (benor.BO_MODE_BYZ_RULE_B, benor.BO_MODE_BYZ_RULE_B_COIN, benor.BO_MODE_SCHED_RULE_B):
            with pytest.raises(RuntimeError, match=want):
                benor.TrialsPlan(11, 2, first(0, 11), mode=mode, thresholds=thresholds, **byz)
            with pytest.raises(RuntimeError, match=want):
                benor.run_trial_states(11, 2, first(0, 11), mode=mode, thresholds=thresholds, **byz)
        with pytest.raises(RuntimeError, match=want):
            benor.LumpedPlan(11, 2, thresholds=thresholds)
    # a wrong base mode: the rule replaces Protocol B's, on the three modes that run it
    for mode in (benor.BO_MODE_LOCKSTEP, benor.BO_MODE_RANDOM_TALLY3, benor.BO_MODE_BYZ_TALLY, benor.BO_MODE_BYZ_COIN,
                 benor.BO_MODE_SCHED_TALLY, 14):
        kw = byz if mode in (8, 10, 12) else {}
        with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}: a threshold rule needs mode"):
            benor.TrialsPlan(11, 2, first(0 if kw else 2, 11), mode=mode, thresholds=protocol_a(11, 2), **kw)
        with pytest.raises(RuntimeError, match="a threshold rule needs mode"):
            benor.run_trial_states(11, 2, first(0 if kw else 2, 11), mode=mode, thresholds=protocol_a(11, 2), **kw)
    # the base mode's own validation stays
    with pytest.raises(RuntimeError, match="byz_strategy must be BO_BYZ_BALANCE or BO_BYZ_SPLIT under an adversarial"):
        benor.TrialsPlan(11, 2, first(0, 11), mode=benor.BO_MODE_SCHED_RULE_B, byz_strategy=RANDOM, thresholds=protocol_a(11, 2))
    with pytest.raises(benor.Error, match="BO_MODE_BYZ_RULE_B needs at most F nodes crashed or Byzantine"):
        benor.TrialsPlan(11, 2, first(1, 11), mode=benor.BO_MODE_BYZ_RULE_B, byzantine=marks({3, 4}, 11), thresholds=protocol_a(11, 2))
    with pytest.raises(RuntimeError, match="bo_lumped: strategy must be"):
        benor.LumpedPlan(11, 2, byz_strategy=RANDOM, thresholds=protocol_a(11, 2))
    # Python's own argument errors
    with pytest.raises(ValueError, match="three words"):
        benor.LumpedPlan(11, 2, thresholds=(1, 2))
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        benor.LumpedPlan(11, 2, thresholds=(1, -2, 3))
    # cfg->rule is not read by the _rule entries; without thresholds= it is checked as before
    plan = benor.LumpedPlan(11, 2, rule=7, thresholds=benor.rule_protocol_a(11, 2))
    assert plan.rule.words == (11, 0, 4)
    with pytest.raises(RuntimeError, match="rule must be"):
        benor.LumpedPlan(11, 2, rule=2)
    L = benor.lib()
    assert L.bo_lumped_check_rule(None, None) == benor.BO_ERR_INVALID_ARGUMENT
    assert L.bo_plan_create_rule(None, None, None) == benor.BO_ERR_INVALID_ARGUMENT
    assert L.bo_plan_rule(None, None) == -benor.BO_ERR_INVALID_ARGUMENT
    assert L.bo_abi_version() == 8


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                          env=env, cwd=ROOT)


def test_cli_argument_errors_need_no_device():
    api_exists()
    base = ("trials", "--N", "11", "--F", "2", "--trials", "10", "--crashed", "0")
    for mode in ((), ("--mode", "tally3"), ("--mode", "byz", "--byz-strategy", "split")):
        p = _cli(*base, *mode, "--rule", "a")
        assert p.returncode != 0 and "--rule needs --mode byzb" in p.stderr, p.stderr
    p = _cli(*base, "--mode", "byz", "--delivery", "adversarial", "--byz-strategy", "split", "--rule", "a")
    assert p.returncode != 0 and "--rule needs --mode byzb" in p.stderr
    for text in ("c", "1:2", "1:2:3:4", "1:x:3", "1:2:-3"):
        p = _cli(*base, "--mode", "byzb", "--rule", text)
        assert p.returncode != 0 and "--rule is a, b or three words P:A:D" in p.stderr, (text, p.stderr)
    for level in ((), ("--delivery", "adversarial", "--byz-strategy", "split"),
                  ("--delivery", "adversarial", "--byz-strategy", "split", "--level", "class")):
        p = _cli(*base, "--mode", "byzb", *level, "--rule", f"{BIG}:0:4")
        assert p.returncode != 0 and "bo_rule: propose_gt2 must be" in p.stderr, p.stderr
    sweep = ("sweep", "--N", "16", "--steps", "2", "--trials", "10")
    p = _cli(*sweep, "--rule", "a")
    assert p.returncode != 0 and "--rule needs --mode byzb" in p.stderr
    p = _cli(*sweep, "--mode", "byz", "--rule", "a")
    assert p.returncode != 0 and "--rule needs --mode byzb" in p.stderr
    p = _cli(*sweep, "--mode", "byzb", "--rule", "1:2")
    assert p.returncode != 0 and "--rule is a, b or three words P:A:D" in p.stderr
    p = _cli(*sweep, "--mode", "byzb", "--rule", f"0:{BIG}:4")
    assert p.returncode != 0 and "bo_rule: adopt_gt must be" in p.stderr
