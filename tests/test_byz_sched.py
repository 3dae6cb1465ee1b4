"""BO_MODE_SCHED_TALLY and BO_MODE_SCHED_RULE_B, count-level delivery under an adversarial scheduler (CPU suite).

The definition (include/benor.h), restated here in plain Python over oracle.random_init,
oracle.coin and test_byz_coin.common_coin -- nothing from the kernel; tests/test_byz_sched_gpu.py checks the
kernels against it bit for bit.  Mode 12 is mode 10 and mode 13 is mode 11, word for word, except for how a
receiver's inbox is composed: the adversary delivers q = N - F messages of its choice from distinct senders, and
chooses what each delivered Byzantine message says.  With (H0, H1, Hq) the class sizes over the honest senders:

    push(v):  c_v = min(q, H_v + b), rest = q - c_v, c_{1-v} = rest - min(rest, Hq)
    even():   hq = min(q, Hq), r = q - hq, lo = r - min(r, H1 + b), hi = min(r, H0 + b),
              c0 = clamp((r + (c & 1)) >> 1, lo, hi), c1 = r - c0

BO_BYZ_SPLIT is push(c & 1) in both phases, BO_BYZ_BALANCE even() in both.  No stream 5, 6, 10 or 11 word.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import benor
import oracle
import test_byz_coin as coin_model
import test_byz_heard as heard
import test_byz_rule_b as mode9
import test_byz_tally as mode8
from conftest import PKG, ROOT
from test_tally import first

M12 = getattr(benor, "BO_MODE_SCHED_TALLY", None)            # absent before the modes: every test fails
M13 = getattr(benor, "BO_MODE_SCHED_RULE_B", None)
K18 = getattr(benor, "BO_KERNEL_TALLY_SCHED", None)
K19 = getattr(benor, "BO_KERNEL_TALLY_SCHED_B", None)
K20 = getattr(benor, "BO_KERNEL_TALLY_SCHED_COIN", None)
K21 = getattr(benor, "BO_KERNEL_TALLY_SCHED_B_COIN", None)
RANDOM, OPPOSE, BALANCE, SPLIT = 0, 1, 3, 4
STRATEGIES = {"BALANCE": BALANCE, "SPLIT": SPLIT}
SEED = mode8.SEED
ALL, HALF = mode8.ALL, mode8.HALF
Q = "?"
marks = mode8.marks
both_strategies = pytest.mark.parametrize("name", list(STRATEGIES))
both_modes = pytest.mark.parametrize("rule", ["ref", "b"])
both_coins = pytest.mark.parametrize("coin", [0, ALL])


def modes_exist():
    assert (M12, M13, K18, K19, K20, K21) == (12, 13, 18, 19, 20, 21)


def mode_of(rule):
    return M13 if rule == "b" else M12


def kernel_of(rule, coin_common):
    return (K21 if rule == "b" else K20) if coin_common else (K19 if rule == "b" else K18)


# ------------------------------------------------------------ the two closed forms
def push(v, q, H, b):
    """(c0, c1): the most v that any inbox allows, and then the least 1 - v."""
    cv = min(q, H[v] + b)
    rest = q - cv
    co = rest - min(rest, H[2])
    return (co, cv) if v else (cv, co)


def even_bounds(q, H, b):
    r = q - min(q, H[2])
    return r, r - min(r, H[1] + b), min(r, H[0] + b)


def even(c, q, H, b):
    """(c0, c1): "?" messages first, then the rest as level as the senders allow."""
    r, lo, hi = even_bounds(q, H, b)
    c0 = min(max((r + (c & 1)) >> 1, lo), hi)
    return c0, r - c0


def counts(strategy, c, q, H, b):
    return push(c & 1, q, H, b) if strategy == SPLIT else even(c, q, H, b)


# ------------------------------------------------------------ restatement
def sched_trial(rule, N, F, faulty, byzantine, seed, trial, k_max, initial_values=None, byz_strategy=BALANCE,
                coin_common=0):
    """One trial of mode 12 (rule "ref") or 13 (rule "b"): (histogram bins it increments, rounds, per-node states).
    test_byz_coin.coin_trial with counts(H, c, phase) replaced by the two closed forms."""
    modes_exist()
    assert byz_strategy in (BALANCE, SPLIT)
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
    R = 0

    def sizes(vals):
        H = [0, 0, 0]
        for v in vals.values():
            H[v] += 1
        return H

    for r in range(1, k_max + 1):
        H = sizes(x)
        by_parity = [counts(byz_strategy, par, q, H, b) for par in (0, 1)]   # a step's counts: one pair per parity of c
        prop = {}
        for c in honest:
            c0, c1 = by_parity[c & 1]
            if rule == "b":
                prop[c] = 0 if 2 * c0 > N + F else 1 if 2 * c1 > N + F else 2
            else:
                prop[c] = 0 if c0 > c1 else 1 if c1 > c0 else 2
        H = sizes(prop)
        by_parity = [counts(byz_strategy, par, q, H, b) for par in (0, 1)]
        new, took = {}, []
        for c in honest:
            c0, c1 = by_parity[c & 1]
            if rule == "b":
                cv = max(c0, c1)
                if c0 != c1 and cv > F:
                    new[c] = 1 if c1 > c0 else 0
                    if 2 * cv > N + F:
                        dec[c] = True
                    continue
            elif c0 > F:
                new[c], dec[c] = 0, True
                continue
            elif c1 > F:
                new[c], dec[c] = 1, True
                continue
            elif c0 != c1:
                new[c] = 1 if c1 > c0 else 0
                continue
            took.append(c)
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


def sched_hist(rule, N, F, faulty, byzantine, seed, trial_begin, trial_count, k_max, initial_values=None, **kw):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in sched_trial(rule, N, F, faulty, byzantine, seed, t, k_max, initial_values, **kw)[0]:
            h[b] += 1
    return h


@functools.lru_cache(maxsize=None)
def shared_hist(rule, N, F, f, b, name, coin_common, k_max=16, trials=150, init=None):
    """`trials` trials from trial 0 at SEED, the first f nodes crashed and the next b Byzantine: computed once."""
    h = sched_hist(rule, N, F, first(f, N), marks(set(range(f, f + b)), N), SEED, 0, trials, k_max,
                   None if init is None else [init] * N, byz_strategy=STRATEGIES[name], coin_common=coin_common)
    h.setflags(write=False)
    return h


# ---------------------------------------------------------------- the tests
def test_the_modes_exist():
    modes_exist()
    for k in (K18, K19, K20, K21):
        assert k in benor.KERNEL_NAMES
    assert benor.BO_MODE_BYZ_COIN == 10 and benor.BO_MODE_BYZ_RULE_B_COIN == 11
    assert benor.BO_KERNEL_TALLY_BYZ_COIN == 16 and benor.BO_KERNEL_TALLY_BYZ_B_COIN == 17
    assert benor.lib().bo_abi_version() == 8                # the struct layout is unchanged


def test_kernel_choice():
    """Through bo_kernel_for: no device needed.  b = 0 and coin_common = 0 keep the mode."""
    modes_exist()
    for strategy in STRATEGIES.values():
        for N, F, f, ids in ((10, 4, 0, set()), (10, 4, 4, set()), (10, 4, 2, {5, 6}), (11, 2, 0, {3, 9}), (64, 20, 0, set()),
                             (1024, 204, 0, set(range(0, 160, 10))), (4096, 819, 0, {7}), (4096, 819, 0, set())):
            for rule in ("ref", "b"):
                kw = dict(mode=mode_of(rule), byzantine=marks(ids, N), byz_strategy=strategy)
                assert benor.kernel_for(N, F, first(f, N), **kw) == kernel_of(rule, 0)
                assert benor.kernel_for(N, F, first(f, N), coin_common=0, **kw) == kernel_of(rule, 0)
                for coin in (1, HALF, ALL):
                    assert benor.kernel_for(N, F, first(f, N), coin_common=coin, **kw) == kernel_of(rule, coin)
                assert benor.kernel_for(N, F, first(f, N), byz_one=HALF, **kw) == kernel_of(rule, 0)   # byz_one is not read
    # without byzantine= at all, and the raw words
    assert benor.kernel_for(10, 4, first(0, 10), mode=M12, byz_strategy=SPLIT) == K18
    assert benor.kernel_for(10, 4, first(0, 10), mode=M13, crash_count=BALANCE, crash_window=HALF) == K21
    # no honest node: outcomes need no kernel
    assert benor.kernel_for(3, 3, first(3, 3), mode=M12, byz_strategy=SPLIT) == benor.BO_KERNEL_NONE
    assert benor.kernel_for(4, 4, first(1, 4), byzantine=marks({1, 2, 3}, 4), mode=M13, byz_strategy=BALANCE,
                            coin_common=ALL) == benor.BO_KERNEL_NONE
    # modes 10 and 11 are as they were
    assert benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_COIN, byz_strategy=SPLIT, coin_common=ALL) == 16
    assert benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_RULE_B_COIN, byz_strategy=SPLIT, coin_common=0) == 15
    assert benor.lib().bo_abi_version() == 8


@both_coins
@both_modes
def test_validation(rule, coin):
    """Every validation error of modes 10 and 11, and the strategy: BALANCE or SPLIT."""
    modes_exist()
    M = mode_of(rule)
    name = "BO_MODE_SCHED_RULE_B" if rule == "b" else "BO_MODE_SCHED_TALLY"
    one = dict(mode=M, byz_strategy=SPLIT, coin_common=coin)
    for bad in (RANDOM, OPPOSE, 2, 5, 0xFFFFFFFF):            # 0 and 1 are strategies of the random-delivery modes only
        with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}.*byz_strategy must be"):
            benor.kernel_for(10, 4, first(0, 10), byzantine=marks({1}, 10), mode=M, byz_strategy=bad, coin_common=coin)
    with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}.*byz_strategy must be"):
        benor.kernel_for(10, 4, first(0, 10), mode=M, coin_common=coin)               # the default word is BYZ_RANDOM
    with pytest.raises(ValueError):                         # byz_one fills crash_cut's word
        benor.kernel_for(10, 4, first(0, 10), byzantine=marks({1}, 10), crash_cut=3, **one)
    with pytest.raises(ValueError):                         # a node is crashed or Byzantine, not both
        benor.kernel_for(10, 4, first(2, 10), byzantine=marks({1}, 10), **one)
    with pytest.raises(benor.Error, match=f"{name} needs at most F nodes crashed or Byzantine"):   # f + b > F
        benor.kernel_for(10, 4, first(2, 10), byzantine=marks({5, 6, 7}, 10), **one)
    with pytest.raises(benor.Error, match="at most F"):                                              # f > F
        benor.kernel_for(10, 4, first(5, 10), **one)
    with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}.*{name}: a faulty entry"):
        benor.kernel_for(10, 4, [0, 3] + [0] * 8, **one)
    with pytest.raises(RuntimeError, match="k_max must be"):
        benor.kernel_for(10, 4, first(0, 10), byzantine=marks({1}, 10), k_max=0, **one)
    with pytest.raises(RuntimeError, match="N must be"):
        benor.kernel_for(4097, 4, first(0, 4097), **one)
    with pytest.raises(ValueError, match="crash_window"):   # one word
        benor.kernel_for(10, 4, first(0, 10), mode=M, byz_strategy=SPLIT, coin_common=HALF, crash_window=4)
    with pytest.raises(ValueError, match="coin_common is a probability"):
        benor.kernel_for(10, 4, first(0, 10), mode=M, byz_strategy=SPLIT, coin_common=ALL + 1)
    assert benor.kernel_for(10, 4, first(2, 10), byzantine=marks({5, 6}, 10), **one) == kernel_of(rule, coin)   # f + b = F
    assert benor.kernel_for(10, 4, [0, 2] + [0] * 8, **one) == kernel_of(rule, coin)                            # the raw value 2


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                          env=env, cwd=ROOT)


def test_cli_argument_errors_need_no_device():
    modes_exist()
    base = ("trials", "--N", "11", "--F", "2", "--trials", "10", "--crashed", "0")
    p = _cli(*base, "--delivery", "adversarial")
    assert p.returncode != 0 and "--delivery adversarial needs --mode byz or --mode byzb" in p.stderr
    p = _cli(*base, "--mode", "tally3", "--delivery", "adversarial")
    assert p.returncode != 0 and "--delivery adversarial needs --mode byz or --mode byzb" in p.stderr
    for mode in ("byz", "byzb"):
        p = _cli(*base, "--mode", mode, "--delivery", "adversarial")                  # the default strategy is random
        assert p.returncode != 0 and "--delivery adversarial needs --byz-strategy balance or --byz-strategy split" in p.stderr
        p = _cli(*base, "--mode", mode, "--delivery", "adversarial", "--byz-strategy", "oppose")
        assert p.returncode != 0 and "--delivery adversarial needs --byz-strategy balance" in p.stderr
        p = _cli(*base, "--mode", mode, "--delivery", "adversarial", "--byz-strategy", "split", "--byzantine", "12")
        assert p.returncode != 0 and "--byzantine counts live nodes" in p.stderr
        p = _cli(*base, "--mode", mode, "--delivery", "adversarial", "--byz-strategy", "split", "--coin-common", "1.5")
        assert p.returncode != 0 and "--coin-common is a probability in [0, 1]" in p.stderr
    p = _cli(*base, "--mode", "byz", "--delivery", "sideways")
    assert p.returncode != 0 and "invalid choice" in p.stderr
    sweep = ("sweep", "--N", "16", "--steps", "2", "--trials", "10")
    p = _cli(*sweep, "--delivery", "adversarial")
    assert p.returncode != 0 and "--delivery adversarial needs --mode byz or --mode byzb" in p.stderr
    p = _cli(*sweep, "--mode", "tally3", "--delivery", "adversarial")
    assert p.returncode != 0 and "--delivery adversarial needs --mode byz or --mode byzb" in p.stderr
    p = _cli(*sweep, "--mode", "byzb", "--delivery", "adversarial")
    assert p.returncode != 0 and "--delivery adversarial needs --byz-strategy balance" in p.stderr


# ---- the closed forms against every inbox
def class_sizes(h):
    return [(H0, H1, h - H0 - H1) for H0 in range(h + 1) for H1 in range(h + 1 - H0)]


def shapes(n_max):
    """(N, F, f, b) with f + b <= F and an honest node."""
    for N in range(1, n_max + 1):
        for F in range(N + 1):
            for f in range(F + 1):
                for b in range(F - f + 1):
                    if N - f - b >= 1:
                        yield N, F, f, b


def inboxes(q, H, b):
    """Every (c0, c1) that an inbox of q messages from distinct senders can give: h0, h1, hq of the honest classes
    and nB Byzantine senders, l1 of which say 1."""
    out = set()
    for h0 in range(min(H[0], q) + 1):
        for h1 in range(min(H[1], q - h0) + 1):
            for hq in range(min(H[2], q - h0 - h1) + 1):
                nB = q - h0 - h1 - hq
                if nB <= b:
                    for l1 in range(nB + 1):
                        out.add((h0 + nB - l1, h1 + l1))
    return out


def test_closed_forms_are_feasible_and_extreme():
    """Brute force over every inbox for N <= 8, all F, f, b and all class sizes: the counts are realisable, push is
    lexicographically extreme (the most v, then the least 1 - v), even attains the minimum of max(c0, c1), lo <= hi."""
    checked = 0
    for N, F, f, b in shapes(8):
        q, h = N - F, N - f - b
        assert h >= q
        for H in class_sizes(h):
            can = inboxes(q, H, b)
            assert can
            for v in (0, 1):
                got = push(v, q, H, b)
                assert got in can, (N, F, f, b, H, v, got)
                most = max(c[v] for c in can)
                assert got[v] == most and got[1 - v] == min(c[1 - v] for c in can if c[v] == most), (N, F, f, b, H, v, got)
            r, lo, hi = even_bounds(q, H, b)
            assert 0 <= lo <= hi <= r, (N, F, f, b, H)
            best = min(max(c) for c in can)
            for c in (0, 1):
                got = even(c, q, H, b)
                assert got in can and max(got) == best, (N, F, f, b, H, c, got, best)
            if r & 1 and lo <= r >> 1 and (r + 1) >> 1 <= hi:  # an odd rest the senders can level: the parities differ
                assert even(0, q, H, b) == (r >> 1, (r + 1) >> 1) and even(1, q, H, b) == ((r + 1) >> 1, r >> 1)
            checked += 1
    assert checked == sum(len(class_sizes(N - f - b)) for N, F, f, b in shapes(8)) > 0   # (every case ran)


# ---- an explicit inbox, sender by sender
def explicit_inbox(strategy, c, q, values, liars):
    """Receiver c's (c0, c1) from q concrete sender ids: `values` maps an honest sender id to 0, 1 or 2 ("?"),
    `liars` lists the Byzantine ids.  SPLIT: the holders of v = c & 1, then the liars (who say v), then "?", then the
    rest.  BALANCE: the "?" holders, then one sender at a time for the smaller tally (on a tie 0 for an odd c, 1 for
    an even one): an honest holder of that value, else a liar who says it, else whoever is left."""
    pool = {k: [s for s, v in sorted(values.items()) if v == k] for k in (0, 1, 2)}
    free = list(liars)
    heard, said = [], []
    if strategy == SPLIT:
        v = c & 1
        order = [(s, v) for s in pool[v]] + [(s, v) for s in free] + [(s, 2) for s in pool[2]] + [(s, 1 - v) for s in pool[1 - v]]
        for s, w in order[:q]:
            heard.append(s), said.append(w)
    else:
        for s in pool[2][:q]:
            heard.append(s), said.append(2)
        tally = [0, 0]
        while len(heard) < q:
            want = (0 if c & 1 else 1) if tally[0] == tally[1] else (0 if tally[0] < tally[1] else 1)
            for w in (want, 1 - want):
                if pool[w]:
                    s = pool[w].pop(0)
                elif free:
                    s = free.pop(0)
                else:
                    continue
                heard.append(s), said.append(w)
                tally[w] += 1
                break
            else:
                raise AssertionError("fewer than q senders")
    assert len(heard) == q and len(set(heard)) == q         # exactly q messages from distinct senders
    for s, w in zip(heard, said):
        assert s in liars and w in (0, 1) or values[s] == w  # honest senders carry their true value, liars 0 or 1
    return said.count(0), said.count(1)


@both_strategies
def test_explicit_inboxes_give_the_closed_forms(name):
    """N <= 12: at every class size an explicit inbox of q sender ids, built from the words of the strategy, counts
    what the closed form says, for a receiver of either parity."""
    strategy = STRATEGIES[name]
    checked = 0
    for N, F, f, b in shapes(12):
        q, h = N - F, N - f - b
        liars = list(range(h, h + b))
        for H in class_sizes(h):
            values = dict(enumerate([0] * H[0] + [1] * H[1] + [2] * H[2]))
            for c in (0, 1):
                assert explicit_inbox(strategy, c, q, values, liars) == counts(strategy, c, q, H, b), (N, F, f, b, H, c)
                checked += 1
    assert checked == 2 * sum(len(class_sizes(N - f - b)) for N, F, f, b in shapes(12)) > 0   # (every case ran)


# ---- exact properties of the restatement
@both_coins
@both_strategies
@both_modes
@pytest.mark.parametrize("N,F", [(10, 4), (11, 2), (64, 12)])
def test_no_choice_is_random_delivery(N, F, rule, name, coin):
    """f = F, b = 0: m == q, the scheduler has no choice, and every trial is test_byz_coin.coin_trial's, per node
    (mode 4's and mode 9's at coin_common 0, mode 10's and mode 11's with a coin), 150 trials."""
    faulty, byz = first(F, N), marks(set(), N)
    for t in range(150):
        assert sched_trial(rule, N, F, faulty, byz, SEED, t, 16, byz_strategy=STRATEGIES[name], coin_common=coin) == \
            coin_model.coin_trial(rule, N, F, faulty, byz, SEED, t, 16, coin_common=coin), t


RULE_B_SHAPES = [(11, 2, 0, 0), (11, 2, 0, 1), (11, 2, 0, 2), (11, 2, 1, 1), (64, 12, 0, 12), (64, 12, 3, 9)]   # N > 5F


@both_coins
@both_strategies
@pytest.mark.parametrize("N,F,f,b", RULE_B_SHAPES)
def test_rule_b_is_safe_under_the_scheduler(N, F, f, b, name, coin):
    """Rule B with N > 5F, 150 trials: the last bin and every bin R * 3 + 2 are zero."""
    h = shared_hist("b", N, F, f, b, name, coin)
    assert int(h[:-1].sum()) == 150
    assert mode9.forbidden_bins(h) == 0, {i: int(v) for i, v in enumerate(h) if v}


@both_coins
@both_strategies
@pytest.mark.parametrize("v", [0, 1])
@pytest.mark.parametrize("N,F,f,b", RULE_B_SHAPES)
def test_rule_b_unanimous_start_decides_in_round_1(N, F, f, b, v, name, coin):
    """Every honest node starts at v: every trial lands in bin[3 + v]."""
    h = shared_hist("b", N, F, f, b, name, coin, trials=150, init=v)
    assert int(h[3 + v]) == 150 and int(h.sum()) == 150, {i: int(n) for i, n in enumerate(h) if n}


# ---- what the adversary achieves (the CPU model's figures in the docstrings)
def test_split_breaks_the_reference_rule_without_a_byzantine_node():
    """ref / SPLIT / (64, 20, b = 0), 300 trials, k_max 32: more than half end in the agreement-violation bin."""
    h = shared_hist("ref", 64, 20, 0, 0, "SPLIT", 0, k_max=32, trials=300)
    print(f"(64, 20) split: {int(h[-1])} of 300 trials violate agreement")
    assert int(h[:-1].sum()) == 300 and int(h[-1]) > 150
    h = shared_hist("ref", 10, 4, 0, 0, "SPLIT", 0, k_max=32, trials=300)
    print(f"(10, 4) split: {int(h[-1])} of 300 trials violate agreement")
    assert int(h[-1]) > 0


def test_balance_draws_the_sqrt_n_boundary():
    """ref / BALANCE, even quorum, N = 64, b = 0, 300 trials, k_max 32: the undecided share at F = 20 exceeds that at F = 2."""
    far = shared_hist("ref", 64, 20, 0, 0, "BALANCE", 0, k_max=32, trials=300)
    near = shared_hist("ref", 64, 2, 0, 0, "BALANCE", 0, k_max=32, trials=300)
    print(f"balance, N = 64: undecided {heard.undecided(far)} of 300 at F = 20, {heard.undecided(near)} of 300 at F = 2 "
          f"({heard.mean_rounds(near, 32):.2f} rounds)")
    assert int(far[:-1].sum()) == 300 and int(near[:-1].sum()) == 300
    assert heard.undecided(far) > heard.undecided(near)


def test_balance_stalls_rule_b_until_the_coin_is_shared():
    """b / BALANCE / (64, 12, b = 12), 300 trials, k_max 32: at least 90 % undecided with local coins, none with a coin
    common in every round; no violation either way."""
    local = shared_hist("b", 64, 12, 0, 12, "BALANCE", 0, k_max=32, trials=300)
    shared = shared_hist("b", 64, 12, 0, 12, "BALANCE", ALL, k_max=32, trials=300)
    print(f"(64, 12, 12) balance: undecided {heard.undecided(local)} of 300 with local coins, {heard.undecided(shared)} with "
          f"a common coin ({heard.mean_rounds(shared, 32):.2f} rounds)")
    assert heard.undecided(local) >= 270
    assert heard.undecided(shared) == 0 and int(shared[:-1].sum()) == 300
    assert mode9.forbidden_bins(local, 32) == 0 and mode9.forbidden_bins(shared, 32) == 0
