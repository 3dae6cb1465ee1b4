"""BO_MODE_BYZ_COIN and BO_MODE_BYZ_RULE_B_COIN, a shared coin in the Byzantine modes (CPU suite).

The definition (include/benor.h), restated here in plain Python over
test_byz_tally.lies, test_byz_heard.heard_byz and heard_lies, test_tally3.draw3, philox,
oracle.random_init and oracle.coin -- nothing from the kernel; tests/test_byz_coin_gpu.py
checks the kernels against it bit for bit.  Mode 10 is mode 8 and mode 11 is mode 9, word
for word, except for the coin a P-phase takes:

* the word other modes call crash_window is coin_common, a probability in units of 2^-32;
* round r of trial t has the block philox(seed, (t_lo, t_hi, 0, (r - 1) | 12 << 24));
  it is common iff coin_common == 2^32 - 1 or out[0] < coin_common, its value out[1] & 1;
* in a common round every honest node whose rule takes a coin (the reference rule's tie,
  Protocol B's "otherwise") gets that bit; in any other round its own oracle.coin;
* coin_common == 0 draws no stream-12 word and is the parent mode's plan.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import benor
import oracle
import test_byz_heard as heard
import test_byz_rule_b as mode9
import test_byz_tally as mode8
from conftest import PKG, ROOT
from test_tally import chi2_two_sample, first, philox
from test_tally3 import draw3

M10 = getattr(benor, "BO_MODE_BYZ_COIN", None)               # absent before the modes: every test fails
M11 = getattr(benor, "BO_MODE_BYZ_RULE_B_COIN", None)
K16 = getattr(benor, "BO_KERNEL_TALLY_BYZ_COIN", None)
K17 = getattr(benor, "BO_KERNEL_TALLY_BYZ_B_COIN", None)
RANDOM, OPPOSE, BALANCE, SPLIT = 0, 1, 3, 4
STRATEGIES = {"RANDOM": RANDOM, "OPPOSE": OPPOSE, "BALANCE": BALANCE, "SPLIT": SPLIT}
STREAM_TALLY, STREAM_LIE, STREAM_COMMON = 5, 10, 12
SEED = mode8.SEED
ALL, HALF = mode8.ALL, mode8.HALF
Q = "?"
marks = mode8.marks
every_strategy = pytest.mark.parametrize("name", list(STRATEGIES))
both_modes = pytest.mark.parametrize("rule", ["ref", "b"])


def modes_exist():
    assert (M10, M11, K16, K17) == (10, 11, 16, 17)


def mode_of(rule):
    return M11 if rule == "b" else M10


# ------------------------------------------------------------ restatement
def common_coin(seed, trial, r, coin_common):
    """The shared bit of round r, or None where the round is not common.  coin_common == 0 draws no word."""
    if coin_common == 0:
        return None
    w = philox(seed, (trial & 0xFFFFFFFF, trial >> 32, 0, (r - 1) | STREAM_COMMON << 24))
    return (w[1] & 1) if coin_common == ALL or w[0] < coin_common else None


def coin_trial(rule, N, F, faulty, byzantine, seed, trial, k_max, initial_values=None, byz_one=0, byz_strategy=RANDOM,
               coin_common=0, takers=None):
    """One trial of mode 10 (rule "ref") or 11 (rule "b"): (histogram bins it increments, rounds, per-node
    states).  `takers`, a list, receives (round, the shared bit or None, [x of every node that took a coin])."""
    modes_exist()
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
        lie = {}

        def sizes(vals):
            return [sum(1 for v in vals.values() if v == k) for k in (0, 1, 2)]

        def counts(H, c, phase):
            s = blocks[c]
            u5 = s[3] << 32 | s[2] if phase else s[1] << 32 | s[0]
            if b == 0:                                       # nobody lies: mode 4's draw, no stream-10 or stream-11 word
                return draw3(m, q, (H[0], H[1], H[2]), seed, trial, c, r, phase, u5)
            if byz_strategy in (BALANCE, SPLIT):             # the liars see the inbox
                h0, h1 = draw3(m, q, (H[0], H[1], H[2] + b), seed, trial, c, r, phase, u5)
                nB = heard.heard_byz(H[2], b, q - h0 - h1, seed, trial, c, r, phase)
                l1 = heard.heard_lies(byz_strategy, c, h0, h1, nB)
                return h0 + nB - l1, h1 + l1

            def u():
                if c not in lie:
                    lie[c] = philox(seed, (tlo, thi, c, (r - 1) | STREAM_LIE << 24))
                w = lie[c]
                return w[3] << 32 | w[2] if phase else w[1] << 32 | w[0]
            B1 = mode8.lies(b, byz_one, byz_strategy, H[0], H[1], u)
            return draw3(m, q, (H[0] + b - B1, H[1] + B1, H[2]), seed, trial, c, r, phase, u5)

        prop, H = {}, sizes(x)
        for c in honest:
            c0, c1 = counts(H, c, 0)
            if rule == "b":
                prop[c] = 0 if 2 * c0 > N + F else 1 if 2 * c1 > N + F else 2
            else:
                prop[c] = 0 if c0 > c1 else 1 if c1 > c0 else 2
        new, H, took = {}, sizes(prop), []
        for c in honest:
            c0, c1 = counts(H, c, 1)
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
            bit = common_coin(seed, trial, r, coin_common)
            for c in took:
                new[c] = oracle.coin(seed, trial, c, r) if bit is None else bit
            if takers is not None:
                takers.append((r, bit, [new[c] for c in took]))
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


def coin_hist(rule, N, F, faulty, byzantine, seed, trial_begin, trial_count, k_max, initial_values=None, **kw):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in coin_trial(rule, N, F, faulty, byzantine, seed, t, k_max, initial_values, **kw)[0]:
            h[b] += 1
    return h


# ------------------------------------------------- mask-level simulation
def mask_sim_hist(rule, N, F, byzantine, k_max, trials, rng, strategy, byz_one=0, coin_common=0, chunk=5000):
    """The same model at the level of inboxes (f = 0, random starts): at every step each honest receiver
    hears an explicit uniform q-subset of the m senders (the q smallest of iid uniform keys).  A Byzantine
    sender inside it says 1 with probability byz_one / 2^32 per (sender, receiver, step) under BYZ_RANDOM,
    and under BYZ_SPLIT 1 to a receiver of odd index and 0 to one of even index.  Per (trial, round) the
    coin is common with probability coin_common / 2^32, and then one fair bit for every node that takes
    a coin; otherwise a fair bit per node.  Initial values, inboxes, lies and coins from `rng`."""
    is_byz = np.array([bool(v) for v in byzantine])
    m, q = N, N - F
    prob = 1.0 if byz_one == ALL else byz_one / 2.0 ** 32
    p_common = 1.0 if coin_common == ALL else coin_common / 2.0 ** 32
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
            assert strategy == RANDOM
            l1 = (liar & (rng.random((n, m, q)) < prob)).sum(axis=2)
        return h0 + nB - l1, h1 + l1

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
            if rule == "b":
                prop = np.where(2 * c0 > N + F, 0, np.where(2 * c1 > N + F, 1, 2)).astype(np.int8)
            else:
                prop = np.where(c0 > c1, 0, np.where(c1 > c0, 1, 2)).astype(np.int8)
            c0, c1 = counts(prop)
            common = rng.random(len(x)) < p_common
            shared = rng.integers(0, 2, size=len(x))
            coin = np.where(common[:, None], shared[:, None], rng.integers(0, 2, size=(len(x), m)))
            if rule == "b":
                cv = np.maximum(c0, c1)
                adopt = (c0 != c1) & (cv > F)
                x = np.where(adopt, c1 > c0, coin).astype(np.int8)
                dec |= adopt & (2 * cv > N + F)
            else:
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
K_MAX = 16
COINS = {"half": HALF, "all": ALL}
# N > 5F, f + b <= F: (N, F, Byzantine ids)
PROPERTY_SHAPES = {"11,2,b2": (11, 2, {3, 8}), "16,3,b3": (16, 3, {0, 7, 15}), "26,5,b4": (26, 5, {2, 9, 17, 25})}
T_PROP = 100


@functools.lru_cache(maxsize=None)
def shared_run(shape, name, coin, init=None, trials=T_PROP):
    """`trials` trials of mode 11 from trial 0, k_max 16, byz_one 1/2, of a PROPERTY_SHAPES entry: computed
    once, read by the property tests.  Returns (histogram, the coin records of every trial)."""
    N, F, ids = PROPERTY_SHAPES[shape]
    h = np.zeros(oracle.hist_len(K_MAX), dtype=np.uint64)
    records = []
    for t in range(trials):
        took = []
        for b in coin_trial("b", N, F, first(0, N), marks(ids, N), SEED, t, K_MAX, None if init is None else [init] * N,
                            byz_one=HALF, byz_strategy=STRATEGIES[name], coin_common=COINS[coin], takers=took)[0]:
            h[b] += 1
        records.append(tuple(took))
    h.setflags(write=False)
    return h, tuple(records)


# ---------------------------------------------------------------- the tests
def test_the_modes_exist():
    modes_exist()
    assert K16 in benor.KERNEL_NAMES and K17 in benor.KERNEL_NAMES
    assert benor.BO_MODE_BYZ_TALLY == 8 and benor.BO_MODE_BYZ_RULE_B == 9
    assert benor.BO_KERNEL_TALLY_BYZ == 14 and benor.BO_KERNEL_TALLY_BYZ_B == 15
    assert benor.lib().bo_abi_version() == 8                # the struct layout is unchanged


def test_kernel_choice_and_plan_collapse():
    """Through bo_kernel_for: no device needed."""
    modes_exist()
    for strategy in STRATEGIES.values():
        for w in (0, HALF, ALL):
            lie = dict(byz_one=w, byz_strategy=strategy)
            for N, F, f, ids in ((10, 4, 0, {0}), (10, 4, 2, {5, 6}), (11, 2, 0, {3, 9}), (1024, 204, 0, set(range(0, 160, 10))),
                                 (4096, 819, 0, {7}), (9, 3, 0, {1})):
                kw = dict(byzantine=marks(ids, N), **lie)
                # 0: the parent mode's kernel
                assert benor.kernel_for(N, F, first(f, N), mode=M10, coin_common=0, **kw) == benor.BO_KERNEL_TALLY_BYZ
                assert benor.kernel_for(N, F, first(f, N), mode=M11, coin_common=0, **kw) == benor.BO_KERNEL_TALLY_BYZ_B
                assert benor.kernel_for(N, F, first(f, N), mode=M10, **kw) == benor.BO_KERNEL_TALLY_BYZ
                for coin in (1, HALF, ALL):
                    assert benor.kernel_for(N, F, first(f, N), mode=M10, coin_common=coin, **kw) == K16
                    assert benor.kernel_for(N, F, first(f, N), mode=M11, coin_common=coin, **kw) == K17
            # b = 0: mode 10 at 0 is mode 4's plan (mode 3's inside that mode's scope), mode 11 at 0 mode 9's
            for N, F, f in ((10, 4, 0), (11, 2, 2), (26, 5, 0)):
                none = dict(byzantine=marks(set(), N), **lie)
                assert benor.kernel_for(N, F, first(f, N), mode=M10, coin_common=0, **none) == \
                    benor.kernel_for(N, F, first(f, N), mode=benor.BO_MODE_RANDOM_TALLY3)
                assert benor.kernel_for(N, F, first(f, N), mode=M11, coin_common=0, **none) == benor.BO_KERNEL_TALLY_BYZ_B
                for coin in (1, HALF, ALL):                  # non-zero runs the new kernels without a Byzantine node too
                    assert benor.kernel_for(N, F, first(f, N), mode=M10, coin_common=coin, **none) == K16
                    assert benor.kernel_for(N, F, first(f, N), mode=M11, coin_common=coin, **none) == K17
                    assert benor.kernel_for(N, F, first(f, N), mode=M10, coin_common=coin) == K16
    assert benor.kernel_for(10, 4, first(0, 10), mode=M10, coin_common=0, byzantine=marks(set(), 10)) == benor.BO_KERNEL_TALLY3
    # no honest node: outcomes need no kernel
    assert benor.kernel_for(3, 3, first(3, 3), mode=M10, coin_common=ALL) == benor.BO_KERNEL_NONE
    assert benor.kernel_for(4, 4, first(1, 4), byzantine=marks({1, 2, 3}, 4), mode=M11, coin_common=ALL) == benor.BO_KERNEL_NONE
    # modes 8 and 9 are as they were, and do not read the word
    assert benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_TALLY, byzantine=marks({1}, 10)) == benor.BO_KERNEL_TALLY_BYZ
    assert benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_TALLY, byzantine=marks({1}, 10),
                            crash_window=7) == benor.BO_KERNEL_TALLY_BYZ
    assert benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_RULE_B, crash_window=7) == benor.BO_KERNEL_TALLY_BYZ_B
    assert benor.lib().bo_abi_version() == 8


@pytest.mark.parametrize("coin", [0, ALL])
@both_modes
def test_validation_is_mode_8s(rule, coin):
    """Every mode-8 validation error, in modes 10 and 11, at coin_common 0 and non-zero."""
    modes_exist()
    M = mode_of(rule)
    name = "BO_MODE_BYZ_RULE_B_COIN" if rule == "b" else "BO_MODE_BYZ_COIN"
    one = dict(mode=M, byz_one=HALF, coin_common=coin)
    with pytest.raises(ValueError):                         # byz_one fills crash_cut's word
        benor.kernel_for(10, 4, first(0, 10), byzantine=marks({1}, 10), crash_cut=3, **one)
    with pytest.raises(ValueError):
        benor.kernel_for(10, 4, first(0, 10), mode=M, byzantine=marks({1}, 10), byz_one=ALL + 1, coin_common=coin)
    with pytest.raises(ValueError):                         # a node is crashed or Byzantine, not both
        benor.kernel_for(10, 4, first(2, 10), byzantine=marks({1}, 10), **one)
    with pytest.raises(benor.Error, match=f"{name} needs at most F nodes crashed or Byzantine"):   # BO_ERR_FAULTY_COUNT
        benor.kernel_for(10, 4, first(2, 10), byzantine=marks({5, 6, 7}, 10), **one)
    with pytest.raises(benor.Error, match="at most F"):                                              # f > F
        benor.kernel_for(10, 4, first(5, 10), **one)
    with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}.*{name}: a faulty entry"):   # faulty value 3
        benor.kernel_for(10, 4, [0, 3] + [0] * 8, **one)
    for bad in (2, 5, 6, 0xFFFFFFFF):
        with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}.*byz_strategy must be"):
            benor.kernel_for(10, 4, first(0, 10), byzantine=marks({1}, 10), byz_strategy=bad, **one)
    with pytest.raises(RuntimeError, match="k_max must be"):
        benor.kernel_for(10, 4, first(0, 10), byzantine=marks({1}, 10), k_max=0, **one)
    with pytest.raises(RuntimeError, match="N must be"):
        benor.kernel_for(4097, 4, first(0, 4097), **one)
    want = (K17 if rule == "b" else K16) if coin else (benor.BO_KERNEL_TALLY_BYZ_B if rule == "b" else benor.BO_KERNEL_TALLY_BYZ)
    assert benor.kernel_for(10, 4, first(2, 10), byzantine=marks({5, 6}, 10), **one) == want          # f + b = F
    assert benor.kernel_for(10, 4, [0, 2] + [0] * 8, **one) == want                                   # the raw value 2


def test_python_argument_errors():
    modes_exist()
    with pytest.raises(ValueError, match="coin_common needs mode"):
        benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_RULE_B, coin_common=HALF)
    with pytest.raises(ValueError, match="coin_common needs mode"):
        benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_RANDOM_TALLY3, coin_common=0)
    with pytest.raises(ValueError, match="coin_common needs mode"):
        benor.kernel_for(10, 4, coin_common=1)
    with pytest.raises(ValueError, match="crash_window"):   # one word
        benor.kernel_for(10, 4, first(0, 10), mode=M11, coin_common=HALF, crash_window=4)
    for bad in (-1, ALL + 1):
        with pytest.raises(ValueError, match="coin_common is a probability"):
            benor.kernel_for(10, 4, first(0, 10), mode=M10, coin_common=bad)
    # the same checks on the two other entry points, before any device work
    with pytest.raises(ValueError, match="coin_common needs mode"):
        benor.TrialsPlan(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_TALLY, coin_common=HALF)
    with pytest.raises(ValueError, match="coin_common needs mode"):
        benor.run_trial_states(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_TALLY, coin_common=HALF)
    with pytest.raises(ValueError, match="crash_window"):
        benor.run_trial_states(10, 4, first(0, 10), mode=M10, coin_common=HALF, crash_window=1)
    # the raw word works too: crash_window's word is coin_common
    assert benor.kernel_for(10, 4, first(0, 10), mode=M10, crash_window=HALF) == K16


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                          env=env, cwd=ROOT)


def test_cli_argument_errors_need_no_device():
    modes_exist()
    base = ("trials", "--N", "11", "--F", "2", "--trials", "10", "--crashed", "0")
    for mode in ("byz", "byzb"):
        p = _cli(*base, "--mode", mode, "--byzantine", "2", "--coin-common", "1.5")
        assert p.returncode != 0 and "--coin-common is a probability in [0, 1]" in p.stderr
        p = _cli(*base, "--mode", mode, "--byzantine", "2", "--coin-common", "-0.1")
        assert p.returncode != 0 and "--coin-common is a probability in [0, 1]" in p.stderr
        p = _cli(*base, "--mode", mode, "--byzantine", "12", "--coin-common", "1")
        assert p.returncode != 0 and "--byzantine counts live nodes" in p.stderr
    p = _cli(*base, "--mode", "tally3", "--coin-common", "0.5")
    assert p.returncode != 0 and "--coin-common needs --mode byz or --mode byzb" in p.stderr
    p = _cli(*base, "--coin-common", "0.5")
    assert p.returncode != 0 and "--coin-common needs --mode byz or --mode byzb" in p.stderr


@every_strategy
@pytest.mark.parametrize("N,F,ids", [(11, 2, {3, 8}), (10, 4, {6})])
def test_coin_common_0_is_the_parent_modes_restatement(N, F, ids, name):
    """coin_common = 0: histograms and per-node states of test_byz_tally's / test_byz_heard's restatement
    (mode 8) and of test_byz_rule_b's (mode 9)."""
    strategy = STRATEGIES[name]
    faulty, byz, T = first(0, N), marks(ids, N), 60
    lie = dict(byz_one=HALF, byz_strategy=strategy)
    parent8 = heard.heard_trial if strategy in (BALANCE, SPLIT) else mode8.byz_trial
    for t in range(T):
        assert coin_trial("ref", N, F, faulty, byz, SEED, t, K_MAX, **lie) == parent8(N, F, faulty, byz, SEED, t, K_MAX, **lie)
        assert coin_trial("b", N, F, faulty, byz, SEED, t, K_MAX, coin_common=0, **lie) == \
            mode9.rule_b_trial(N, F, faulty, byz, SEED, t, K_MAX, **lie)


@every_strategy
@pytest.mark.parametrize("coin", list(COINS))
@pytest.mark.parametrize("shape", list(PROPERTY_SHAPES))
def test_no_disagreement_for_n_above_5f(shape, name, coin):
    """Mode 11, random starts, k_max 16: not one entry in the last bin or in a bin R * 3 + 2, and in every
    common round all the nodes that took a coin hold the same x afterwards."""
    h, records = shared_run(shape, name, coin)
    assert int(h[:-1].sum()) == T_PROP
    assert mode9.forbidden_bins(h) == 0, {i: int(v) for i, v in enumerate(h) if v}
    common_rounds = 0
    for took in records:
        for r, bit, xs in took:
            if coin == "all":
                assert bit is not None
            if bit is not None:
                common_rounds += 1
                assert xs and all(v == bit for v in xs)
    assert common_rounds > 0


@every_strategy
@pytest.mark.parametrize("coin", list(COINS))
@pytest.mark.parametrize("v", [0, 1])
@pytest.mark.parametrize("shape", list(PROPERTY_SHAPES))
def test_unanimous_start_decides_in_round_1(shape, v, name, coin):
    """Every honest node starts at v: every trial lands in bin[1 * 3 + v], and nobody takes a coin."""
    h, records = shared_run(shape, name, coin, init=v, trials=40)
    assert int(h[3 + v]) == 40 and int(h.sum()) == 40, {i: int(n) for i, n in enumerate(h) if n}
    assert all(not took for took in records)


def test_the_shared_coin_ends_the_exponential_wait():
    """(64, 12, b = 12), Rule B, RANDOM 1/2, random starts, k_max 32, 60 trials from trial 0 at SEED_64: with local
    coins (mode 9's restatement) no trial decides; with a coin common in every round all of them do.  In a common
    round the adopters all adopt one v (N > 5F) and the coin equals v with probability 1/2, so a trial stays
    undecided after 32 rounds with probability below 2^-30.  That side holds at every seed.  Local coins do decide
    now and then, about one trial in a hundred within 32 rounds (of SEED + 0 .. SEED + 11 five seeds leave all 60
    undecided, six leave 59 and one 58), so the seed of this test was checked on this restatement: SEED + 3."""
    N, F, T = 64, 12, 60
    SEED = SEED_64
    faulty, byz = first(0, N), marks({(5 * i) % 64 for i in range(12)}, N)
    assert sum(byz) == 12
    lie = dict(byz_one=HALF, byz_strategy=RANDOM)
    local = mode9.rule_b_hist(N, F, faulty, byz, SEED, 0, T, 32, **lie)
    shared = coin_hist("b", N, F, faulty, byz, SEED, 0, T, 32, coin_common=ALL, **lie)
    print(f"undecided of {T}: local coins {heard.undecided(local)}, common coin {heard.undecided(shared)}, "
          f"{heard.mean_rounds(shared, 32):.2f} rounds")
    assert heard.undecided(local) == T
    assert heard.undecided(shared) == 0 and int(shared[:-1].sum()) == T and mode9.forbidden_bins(shared, 32) == 0


@both_modes
@pytest.mark.parametrize("name", ["RANDOM", "SPLIT"])
def test_coin_common_1_is_the_parent_mode_where_no_word_is_0(rule, name):
    """coin_common = 1: a round is common iff its stream-12 out[0] is 0.  Where none is, the histogram is the
    parent mode's: the shape of the A/B measurement."""
    N, F, ids, T = (11, 2, {3, 8}, 80) if rule == "b" else (10, 4, {2, 7}, 80)   # (an even quorum: the reference rule ties)
    for t in range(T):
        for r in range(1, K_MAX + 1):
            assert philox(SEED, (t, 0, 0, (r - 1) | STREAM_COMMON << 24))[0] != 0
    lie = dict(byz_one=HALF, byz_strategy=STRATEGIES[name])
    got = coin_hist(rule, N, F, first(0, N), marks(ids, N), SEED, 0, T, K_MAX, coin_common=1, **lie)
    ref = coin_hist(rule, N, F, first(0, N), marks(ids, N), SEED, 0, T, K_MAX, coin_common=0, **lie)
    assert np.array_equal(got, ref)
    assert not np.array_equal(ref, coin_hist(rule, N, F, first(0, N), marks(ids, N), SEED, 0, T, K_MAX, coin_common=ALL, **lie))


def test_the_word_depends_on_trial_and_round_only():
    """One block per (trial, round): nodes, strategy and the nodes that take a coin do not enter its counter."""
    for t in (0, 5, (1 << 32) + 7):
        for r in (1, 2, 17):
            w = philox(SEED, (t & 0xFFFFFFFF, t >> 32, 0, (r - 1) | STREAM_COMMON << 24))
            assert common_coin(SEED, t, r, ALL) == w[1] & 1
            assert common_coin(SEED, t, r, 0) is None
            assert (common_coin(SEED, t, r, HALF) is not None) == (w[0] < HALF)
    took = []
    coin_trial("b", 16, 3, first(0, 16), marks({0, 7, 15}, 16), SEED, 3, K_MAX, byz_one=HALF, coin_common=ALL, takers=took)
    for r, bit, xs in took:
        assert bit == common_coin(SEED, 3, r, ALL)


SEED_64 = SEED + 3                                           # test_the_shared_coin_ends_the_exponential_wait


LAW = {  # rule: (N, F, Byzantine ids, restatement trials, simulated trials)
    "b": (26, 5, {2, 9, 17, 25}, 600, 10000),
    "ref": (10, 4, {2, 7}, 1500, 20000),
}


@pytest.mark.parametrize("name", ["RANDOM", "SPLIT"])
@both_modes
def test_law_matches_the_mask_level_simulation(rule, name):
    """The restatement's histogram against the mask-level simulation with a shared coin, f = 0, byz_one 1/2,
    coin_common 1/2 (both kinds of round occur), k_max 16: two-sample chi^2 over bins pooled to >= 20,
    p > 10^-3 at fixed seeds."""
    N, F, ids, T, T_sim = LAW[rule]
    strategy = STRATEGIES[name]
    got = coin_hist(rule, N, F, first(0, N), marks(ids, N), SEED, 0, T, K_MAX, byz_one=HALF, byz_strategy=strategy,
                    coin_common=HALF)
    ref = mask_sim_hist(rule, N, F, marks(ids, N), K_MAX, T_sim, np.random.default_rng(SEED + 12), strategy, byz_one=HALF,
                        coin_common=HALF)
    assert int(got[:-1].sum()) == T and int(ref[:-1].sum()) == T_sim
    p, stat, df = chi2_two_sample(got, ref)
    print(f"{rule} ({N}, {F}, b = {len(ids)}) {name}: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}; violations "
          f"{int(got[-1])} / {int(ref[-1])}; undecided {heard.undecided(got)} of {T} / {heard.undecided(ref)} of {T_sim}; "
          f"mean rounds {heard.mean_rounds(got):.2f} / {heard.mean_rounds(ref):.2f}")
    assert p > 1e-3, (p, stat, df)
    assert df >= 2
    if rule == "b":
        assert mode9.forbidden_bins(got) == 0 and mode9.forbidden_bins(ref) == 0
