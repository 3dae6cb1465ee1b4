"""BO_MODE_BYZ_RULE_B, Byzantine senders under Ben-Or's Byzantine-tolerant rule (CPU suite).

The definition (include/benor.h), restated here in plain Python over
test_byz_tally.lies, test_byz_heard.heard_byz and heard_lies, test_tally3.draw3, philox,
oracle.random_init and oracle.coin -- nothing from the kernel;
tests/test_byz_rule_b_gpu.py checks the kernel against it bit for bit.  Who is
Byzantine, f + b <= F, compact indices, senders and receivers, the four strategies with
their draws, coins, k, halting over the honest nodes, the histogram and the per-node
states are mode 8's (tests/test_byz_tally.py, tests/test_byz_heard.py).  What differs is
the rule applied to a receiver's counts (c0, c1), with F as the paper's t:

* R-phase: propose 0 if 2 c0 > N + F, else 1 if 2 c1 > N + F, else "?".
* P-phase: v = the value with the strictly larger count (none on c0 == c1).  If v exists
  and c_v > F: x = v, decided iff 2 c_v > N + F (sticky).  Otherwise x = oracle.coin.
* b = 0 keeps the rule (it is not mode 4's plan): B1 = 0 at every step, no stream-10 or
  stream-11 word, the same at every strategy and byz_one.

For N > 5F and f + b <= F (DESIGN §4.3.9 has the argument) no trial ends in the
agreement-violation bin or in a bin R * 3 + 2, and a unanimous honest start v lands in
bin[1 * 3 + v]: hard conditions, checked below on the restatement.
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
import test_byz_tally as mode8
from conftest import PKG, ROOT
from test_tally import chi2_two_sample, first, philox
from test_tally3 import draw3

M9 = getattr(benor, "BO_MODE_BYZ_RULE_B", None)              # absent before the mode: every test fails
BYZ_B = getattr(benor, "BO_KERNEL_TALLY_BYZ_B", None)
RANDOM, OPPOSE, BALANCE, SPLIT = 0, 1, 3, 4
STRATEGIES = {"RANDOM": RANDOM, "OPPOSE": OPPOSE, "BALANCE": BALANCE, "SPLIT": SPLIT}
STREAM_TALLY, STREAM_LIE = 5, 10
SEED = mode8.SEED
ALL, HALF = mode8.ALL, mode8.HALF
Q = "?"
marks = mode8.marks
every_strategy = pytest.mark.parametrize("name", list(STRATEGIES))


def mode_exists():
    assert (M9, BYZ_B) == (9, 15)


# ------------------------------------------------------------ restatement
def rule_b_trial(N, F, faulty, byzantine, seed, trial, k_max, initial_values=None, byz_one=0, byz_strategy=RANDOM):
    """One trial: (histogram bins it increments, rounds, per-node states)."""
    mode_exists()
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
            if byz_strategy in (BALANCE, SPLIT):             # the liars see the inbox (tests/test_byz_heard.py)
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
            assert not (2 * c0 > N + F and 2 * c1 > N + F)
            prop[c] = 0 if 2 * c0 > N + F else 1 if 2 * c1 > N + F else 2
        new, H = {}, sizes(prop)
        for c in honest:
            c0, c1 = counts(H, c, 1)
            cv = max(c0, c1)
            if c0 != c1 and cv > F:
                new[c] = 1 if c1 > c0 else 0
                if 2 * cv > N + F:
                    dec[c] = True
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


def rule_b_hist(N, F, faulty, byzantine, seed, trial_begin, trial_count, k_max, initial_values=None, **lie):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in rule_b_trial(N, F, faulty, byzantine, seed, t, k_max, initial_values, **lie)[0]:
            h[b] += 1
    return h


# ------------------------------------------------- mask-level simulation
def mask_sim_hist(N, F, byzantine, k_max, trials, rng, strategy, byz_one=0, chunk=5000):
    """The same model at the level of inboxes (f = 0, random starts): at every step each honest
    receiver hears an explicit uniform q-subset of the m senders (the q smallest of iid uniform
    keys).  A Byzantine sender inside it says 1 with probability byz_one / 2^32 per (sender,
    receiver, step) under BYZ_RANDOM, and under BYZ_SPLIT 1 to a receiver of odd index and 0 to
    one of even index.  The rule is Protocol B's.  Initial values, inboxes, lies and coins from `rng`."""
    is_byz = np.array([bool(v) for v in byzantine])
    m, q = N, N - F
    prob = 1.0 if byz_one == ALL else byz_one / 2.0 ** 32
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
            prop = np.where(2 * c0 > N + F, 0, np.where(2 * c1 > N + F, 1, 2)).astype(np.int8)
            c0, c1 = counts(prop)
            coin = rng.integers(0, 2, size=(len(x), m))
            cv = np.maximum(c0, c1)
            adopt = (c0 != c1) & (cv > F)
            x = np.where(adopt, c1 > c0, coin).astype(np.int8)
            dec |= adopt & (2 * cv > N + F)
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
BYZ_ONES = {"0": 0, "half": HALF, "all": ALL}
# N > 5F, f + b <= F: (N, F, crashed, Byzantine ids)
PROPERTY_SHAPES = {"11,2,b2": (11, 2, 0, {3, 8}), "11,2,f1,b1": (11, 2, 1, {6}), "16,3,b3": (16, 3, 0, {0, 7, 15})}
T_PROP = 150


@functools.lru_cache(maxsize=None)
def shared_hist(shape, name, one, init=None, trials=T_PROP):
    """`trials` trials from trial 0, k_max 16, of a PROPERTY_SHAPES entry: computed once, read by the property tests.
    init: None (random starts) or the value every node starts with."""
    N, F, f, ids = PROPERTY_SHAPES[shape]
    h = rule_b_hist(N, F, first(f, N), marks(ids, N), SEED, 0, trials, K_MAX, None if init is None else [init] * N,
                    byz_one=BYZ_ONES[one], byz_strategy=STRATEGIES[name])
    h.setflags(write=False)
    return h


def forbidden_bins(h, k_max=K_MAX):
    """What N > 5F rules out: the agreement-violation bin and every bin R * 3 + 2 of a decided trial."""
    return int(h[-1]) + sum(int(h[R * 3 + 2]) for R in range(1, k_max + 1))


# ---------------------------------------------------------------- the tests
def test_the_mode_exists():
    mode_exists()
    assert BYZ_B in benor.KERNEL_NAMES and benor.BO_KERNEL_TALLY_BYZ == 14 and benor.BO_MODE_BYZ_TALLY == 8
    assert benor.lib().bo_abi_version() == 8                # the struct layout is unchanged


def test_validation_and_kernel_choice():
    """Through bo_kernel_for: no device needed.  Every mode-8 validation error, in mode 9."""
    mode_exists()
    one = dict(mode=M9, byz_one=HALF)
    with pytest.raises(ValueError):                         # byz_one fills crash_cut's word
        benor.kernel_for(10, 4, first(0, 10), mode=M9, byzantine=marks({1}, 10), byz_one=HALF, crash_cut=3)
    with pytest.raises(ValueError):
        benor.kernel_for(10, 4, first(0, 10), mode=M9, byzantine=marks({1}, 10), byz_one=ALL + 1)
    with pytest.raises(ValueError):                         # a node is crashed or Byzantine, not both
        benor.kernel_for(10, 4, first(2, 10), mode=M9, byzantine=marks({1}, 10))
    with pytest.raises(ValueError):                         # byzantine= with mode 4 still raises
        benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_RANDOM_TALLY3, byzantine=marks({1}, 10))
    with pytest.raises(benor.Error, match="BO_MODE_BYZ_RULE_B needs at most F nodes crashed or Byzantine"):   # BO_ERR_FAULTY_COUNT
        benor.kernel_for(10, 4, first(2, 10), byzantine=marks({5, 6, 7}, 10), **one)
    with pytest.raises(benor.Error, match="at most F"):                                              # f > F
        benor.kernel_for(10, 4, first(5, 10), **one)
    assert benor.kernel_for(10, 4, first(2, 10), byzantine=marks({5, 6}, 10), **one) == BYZ_B        # f + b = F
    with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}.*BO_MODE_BYZ_RULE_B"):   # faulty value 3
        benor.kernel_for(10, 4, [0, 3] + [0] * 8, **one)
    for bad in (2, 5, 6, 0xFFFFFFFF):
        with pytest.raises(RuntimeError, match=f"libbenor error {benor.BO_ERR_INVALID_ARGUMENT}"):
            benor.kernel_for(10, 4, first(0, 10), byzantine=marks({1}, 10), byz_strategy=bad, **one)
    assert benor.kernel_for(10, 4, [0, 2] + [0] * 8, **one) == BYZ_B                                 # the raw value 2
    for strategy in STRATEGIES.values():
        for w in (0, HALF, ALL):                             # every byz_one is valid
            kw = dict(mode=M9, byz_one=w, byz_strategy=strategy)
            for N, F, f, ids in ((10, 4, 0, {0}), (10, 4, 2, {5, 6}), (11, 2, 0, {3, 9}), (11, 2, 2, set()),
                                 (1024, 204, 0, set(range(0, 160, 10))), (4096, 819, 0, {7}), (9, 3, 0, {1})):
                assert benor.kernel_for(N, F, first(f, N), byzantine=marks(ids, N), **kw) == BYZ_B
            # b = 0 is this mode's plan, not mode 4's: odd and even quorums alike
            assert benor.kernel_for(10, 4, first(0, 10), byzantine=marks(set(), 10), **kw) == BYZ_B
            assert benor.kernel_for(11, 4, first(0, 11), byzantine=marks(set(), 11), **kw) == BYZ_B
            assert benor.kernel_for(11, 4, first(0, 11), **kw) == BYZ_B
    # no honest node: outcomes need no kernel
    assert benor.kernel_for(3, 3, first(3, 3), **one) == benor.BO_KERNEL_NONE
    assert benor.kernel_for(4, 4, first(1, 4), byzantine=marks({1, 2, 3}, 4), **one) == benor.BO_KERNEL_NONE
    # mode 8 is as it was
    assert benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_TALLY, byzantine=marks({1}, 10)) == benor.BO_KERNEL_TALLY_BYZ
    assert benor.kernel_for(10, 4, first(0, 10), mode=benor.BO_MODE_BYZ_TALLY, byzantine=marks(set(), 10)) == benor.BO_KERNEL_TALLY3
    assert benor.lib().bo_abi_version() == 8


@every_strategy
@pytest.mark.parametrize("one", list(BYZ_ONES))
@pytest.mark.parametrize("shape", list(PROPERTY_SHAPES))
def test_no_disagreement_for_n_above_5f(shape, name, one):
    """Random starts, 150 trials, k_max 16: not one entry in the last bin or in a bin R * 3 + 2."""
    h = shared_hist(shape, name, one)
    assert int(h[:-1].sum()) == T_PROP
    assert forbidden_bins(h) == 0, {i: int(v) for i, v in enumerate(h) if v}


@every_strategy
@pytest.mark.parametrize("one", list(BYZ_ONES))
@pytest.mark.parametrize("v", [0, 1])
@pytest.mark.parametrize("shape", list(PROPERTY_SHAPES))
def test_unanimous_start_decides_in_round_1(shape, v, name, one):
    """Every honest node starts at v: every trial lands in bin[1 * 3 + v]."""
    h = shared_hist(shape, name, one, init=v, trials=60)
    assert int(h[3 + v]) == 60 and int(h.sum()) == 60, {i: int(n) for i, n in enumerate(h) if n}
    N, F, f, ids = PROPERTY_SHAPES[shape]
    _, rounds, st = rule_b_trial(N, F, first(f, N), marks(ids, N), SEED, 5, K_MAX, [v] * N, byz_one=BYZ_ONES[one],
                                 byz_strategy=STRATEGIES[name])
    assert rounds == 1
    for i, s in enumerate(st):
        assert s == ({"killed": True, "x": None, "decided": None, "k": None} if i < f else
                     {"killed": False, "x": None, "decided": None, "k": None} if i in ids else
                     {"killed": False, "x": v, "decided": True, "k": 2})


def test_split_breaks_the_reference_rule_on_the_same_trials():
    """(11, 2), b = 2, SPLIT, random starts, 150 trials, k_max 16.  The restatements' counts on
    these trials (seed SEED, trials 0..149): mode 8's rule 32 agreement violations, all 150 decided
    in round 1; this rule none, all 150 decided, 3.81 rounds per trial."""
    N, F, ids = PROPERTY_SHAPES["11,2,b2"][0], PROPERTY_SHAPES["11,2,b2"][1], PROPERTY_SHAPES["11,2,b2"][3]
    ref = heard.heard_hist(N, F, first(0, N), marks(ids, N), SEED, 0, T_PROP, K_MAX, byz_strategy=SPLIT)
    got = shared_hist("11,2,b2", "SPLIT", "0")
    print(f"violations: reference rule {int(ref[-1])}, Protocol B {int(got[-1])}; undecided {heard.undecided(ref)}, "
          f"{heard.undecided(got)}; mean rounds {heard.mean_rounds(ref):.2f}, {heard.mean_rounds(got):.2f}")
    assert int(ref[-1]) > 0
    assert int(got[-1]) == 0 and heard.undecided(got) == 0
    assert heard.mean_rounds(got) > heard.mean_rounds(ref)   # what the tolerance costs


@every_strategy
def test_without_byzantine_nodes_strategy_and_byz_one_are_not_read(name):
    """b = 0: one histogram for all four strategies and three byz_one values, at an even and an odd
    quorum, with crashed nodes up to f = F (m == q), and with "?" starts."""
    init = [Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1]
    for N, F, f, ini in ((11, 2, 0, None), (11, 2, 2, None), (10, 2, 1, None), (11, 2, 1, init)):
        ref = rule_b_hist(N, F, first(f, N), marks(set(), N), SEED, 0, 60, K_MAX, ini, byz_one=0, byz_strategy=RANDOM)
        assert int(ref[:-1].sum()) == 60 and forbidden_bins(ref) == 0
        for one in (0, HALF, ALL):
            got = rule_b_hist(N, F, first(f, N), marks(set(), N), SEED, 0, 60, K_MAX, ini, byz_one=one,
                              byz_strategy=STRATEGIES[name])
            assert np.array_equal(got, ref)


def test_the_rule_differs_from_mode_4_without_byzantine_nodes():
    """(10, 4), b = 0: N <= 5F, a proposal needs 2 c > 14, more than the 6 messages heard -- nobody ever
    proposes or decides, while mode 4's rule decides nearly every trial."""
    import test_tally3
    got = rule_b_hist(10, 4, first(0, 10), marks(set(), 10), SEED, 0, 100, 8)
    ref = test_tally3.tally3_hist(10, 4, first(0, 10), SEED, 0, 100, 8)
    assert int(got[:3].sum()) == 100 and int(ref[:3].sum()) < 50


def test_n_at_most_3f_never_proposes():
    """(9, 3), b = 3: 2 c > 12 needs 7 > q = 6 messages; every trial ends in bin 0..2 after k_max rounds."""
    for name in ("RANDOM", "SPLIT"):
        h = rule_b_hist(9, 3, first(0, 9), marks({0, 4, 8}, 9), SEED, 0, 40, 4, byz_one=HALF, byz_strategy=STRATEGIES[name])
        assert int(h[:3].sum()) == 40 and int(h.sum()) == 40


LAW = {  # (N, F, Byzantine ids, restatement trials, simulated trials)
    "26,8,4": (26, 8, {2, 9, 17, 25}, 100, 2000),
    "26,5,4": (26, 5, {2, 9, 17, 25}, 600, 10000),
}


@pytest.mark.parametrize("name", ["RANDOM", "SPLIT"])
@pytest.mark.parametrize("shape", list(LAW))
def test_law_matches_the_mask_level_simulation(shape, name):
    """The restatement's histogram against the mask-level simulation with the same rule, b = 4, f = 0,
    byz_one 1/2, k_max 16: two-sample chi^2 over bins pooled to >= 20, p > 10^-3 at fixed seeds.

    (26, 8) is mode 8's law-test shape.  Under this rule it is degenerate: a proposal needs
    2 c > 34, all q = 18 messages equal, and adopting a value 9 equal proposals, so every x is a
    coin in every round; both sides put every trial, run to k_max, in bin 2 (22 fair coins agree
    with probability 2^-21), and the chi^2 has one cell.  Hence few trials there, and (26, 5),
    inside N > 5F where the rule decides, carries the comparison: 600 trials against 10^4."""
    N, F, ids, T, T_sim = LAW[shape]
    strategy = STRATEGIES[name]
    got = rule_b_hist(N, F, first(0, N), marks(ids, N), SEED, 0, T, K_MAX, byz_one=HALF, byz_strategy=strategy)
    ref = mask_sim_hist(N, F, marks(ids, N), K_MAX, T_sim, np.random.default_rng(SEED + 9), strategy, byz_one=HALF)
    assert int(got[:-1].sum()) == T and int(ref[:-1].sum()) == T_sim
    p, stat, df = chi2_two_sample(got, ref)
    print(f"({shape}) {name}: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}; violations {int(got[-1])} / {int(ref[-1])}; "
          f"undecided {heard.undecided(got)} of {T} / {heard.undecided(ref)} of {T_sim}; "
          f"mean rounds {heard.mean_rounds(got):.2f} / {heard.mean_rounds(ref):.2f}")
    assert p > 1e-3, (p, stat, df)
    if shape == "26,8,4":
        assert int(got[2]) == T and int(ref[2]) == T_sim
    else:
        assert df >= 3 and forbidden_bins(got) == 0 and forbidden_bins(ref) == 0


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                          env=env, cwd=ROOT)


def test_cli_argument_errors_need_no_device():
    mode_exists()
    base = ("trials", "--N", "11", "--F", "2", "--trials", "10", "--mode", "byzb", "--crashed", "0")
    p = _cli(*base, "--byzantine", "2", "--byz-one", "1.5")
    assert p.returncode != 0 and "--byz-one is a probability in [0, 1]" in p.stderr
    p = _cli(*base, "--byzantine", "12")
    assert p.returncode != 0 and "--byzantine counts live nodes" in p.stderr
    p = _cli(*base, "--byzantine", "2", "--byz-strategy", "both")
    assert p.returncode != 0 and "invalid choice" in p.stderr
    p = _cli(*base, "--byzantine", "2", "--crash-count", "1")
    assert p.returncode != 0 and "--crash-at / --crash-count need" in p.stderr
    p = _cli("trials", "--N", "11", "--F", "2", "--trials", "10", "--mode", "tally3", "--crashed", "0", "--byzantine", "2")
    assert p.returncode != 0 and "--byzantine needs --mode byz or --mode byzb" in p.stderr
