"""Threshold rules on the device: the RuleT entries of csrc/benor_tally_sched.hip,
csrc/benor_tally_byz.hip and csrc/benor_lumped.hip, bit-exact against the plain-Python restatement in
tests/test_rule.py (histograms, per-node states, bo_lumped_trial_rule states), device against device with the
compile-time rules' entries at Protocol B's and the reference's words, both levels against the exact DP, and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import oracle
import test_lumped as lumped_model
import test_rule as model
from conftest import PKG, ROOT
from test_tally import first

pytestmark = pytest.mark.gpu

BALANCE, SPLIT = model.BALANCE, model.SPLIT
SCHED = model.SCHED_STRATEGIES
EVERY = model.ALL_STRATEGIES
ALL, HALF = model.ALL, model.HALF
SEED = model.SEED
marks = model.marks
Q = "?"
M8, M9, M10, M11, M12, M13 = 8, 9, 10, 11, 12, 13
both_strategies = model.both_strategies
every_strategy = model.every_strategy
every_coin = pytest.mark.parametrize("coin", [0, HALF, ALL])


def a_words(N, F):
    model.api_exists()
    words = benor.rule_protocol_a(N, F).words
    assert words == model.protocol_a(N, F)
    return words


def base_kernel(mode, coin):
    return {M9: 15, M11: 17 if coin else 15, M13: 21 if coin else 19}[mode]


def plan_of(words, mode, N, F, faulty, byz, *, seed=SEED, k_max=16, init=None, coin_common=0, **kw):
    coin_kw = {} if mode == M9 else {"coin_common": coin_common}
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=mode, byzantine=byz,
                            thresholds=words, **coin_kw, **kw)
    assert plan.kernel == base_kernel(mode, coin_common)      # the base plan's variant: no kernel value of its own
    assert plan.rule.words == tuple(words)
    return plan


def check_exact(words, mode, N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, coin_common=0, **kw):
    """The launch's histogram, and the per-node states of its first two and last trials, against the restatement
    (each trial restated once)."""
    plan = plan_of(words, mode, N, F, faulty, byz, seed=seed, k_max=k_max, init=init, coin_common=coin_common, **kw)
    got = plan.run(begin, trials)
    plan.check()                                              # no overflow or deferral state
    restate = model.sched_trial if mode == M13 else model.coin_trial
    ref = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    restated = {}
    for t in range(begin, begin + trials):
        restated[t] = restate(words, N, F, faulty, byz, seed, t, k_max, init, coin_common=coin_common, **kw)
        for b in restated[t][0]:
            ref[b] += 1
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    coin_kw = {} if mode == M9 else {"coin_common": coin_common}
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init, mode=mode,
                                            byzantine=byz, thresholds=words, **coin_kw, **kw)
        _, ref_rounds, ref_st = restated[t]
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
    return got


# ------------------------------------------------------------ the scheduler, Protocol A
@both_strategies
@every_coin
def test_sched_bit_exact_small(coin, name):
    """(10, 4, b = 0) and (11, 5, b = 0), where Protocol A is safe, and (11, 2) with one and two liars."""
    s = SCHED[name]
    for N, F in ((10, 4), (11, 5)):
        h = check_exact(a_words(N, F), M13, N, F, first(0, N), marks(set(), N), 300, byz_strategy=s, coin_common=coin)
        assert int(h[:-1].sum()) == 300 and int(h[-1]) == 0
    for ids in ({3}, {3, 8}):
        check_exact(a_words(11, 2), M13, 11, 2, first(0, 11), marks(ids, 11), 300, byz_strategy=s, coin_common=coin)


@both_strategies
def test_sched_k_max_one_and_question_mark_starts(name):
    s = SCHED[name]
    check_exact(a_words(11, 2), M13, 11, 2, first(0, 11), marks({2, 7}, 11), 300, k_max=1, byz_strategy=s)
    check_exact(a_words(10, 4), M13, 10, 4, first(1, 10), marks({5}, 10), 300, k_max=1, byz_strategy=s, coin_common=ALL)
    init = [Q, 1, 0, 0, Q, 1, 0, 0, 1, Q, 1, 0]
    for ids in ({4}, {0, 4}):
        check_exact(a_words(12, 2), M13, 12, 2, first(0, 12), marks(ids, 12), 200, init=init, byz_strategy=s, coin_common=HALF)
    check_exact(a_words(12, 2), M13, 12, 2, first(0, 12), marks({4}, 12), 100, init=[Q] * 9 + [1, 0, Q], byz_strategy=s)


@both_strategies
def test_sched_groups(name):
    """(64, 12, b = 12): one full group; (65, 12) and (130, 46) with liars {0, 63, 64}: the group edges; (200, 70) with
    liars 64 .. 127: a group with no honest lane."""
    s = SCHED[name]
    ids = {(5 * i) % 64 for i in range(12)}
    check_exact(a_words(64, 12), M13, 64, 12, first(0, 64), marks(ids, 64), 60, k_max=32, byz_strategy=s)
    check_exact(a_words(65, 12), M13, 65, 12, first(0, 65), marks({0, 63, 64}, 65), 60, byz_strategy=s, coin_common=HALF)
    check_exact(a_words(130, 46), M13, 130, 46, first(0, 130), marks({0, 63, 64}, 130), 40, byz_strategy=s)
    check_exact(a_words(200, 70), M13, 200, 70, first(0, 200), marks(set(range(64, 128)), 200), 30, byz_strategy=s,
                coin_common=HALF)


@both_strategies
def test_sched_large_networks(name):
    """(1024, 204, b = 16), 60 trials, and (4096, 819, b = 16), all 64 groups, 8 trials."""
    s = SCHED[name]
    ids = {(41 * i) % 1024 for i in range(16)}
    check_exact(a_words(1024, 204), M13, 1024, 204, first(0, 1024), marks(ids, 1024), 60, k_max=8, byz_strategy=s)
    ids = {(163 * i) % 4096 for i in range(16)}
    check_exact(a_words(4096, 819), M13, 4096, 819, first(0, 4096), marks(ids, 4096), 8, k_max=4, byz_strategy=s,
                coin_common=HALF)


@both_strategies
def test_sched_trial_ids_and_launch_split(name):
    """trial_begin = 2^32 + 12345, and one launch against three."""
    s = SCHED[name]
    check_exact(a_words(10, 4), M13, 10, 4, first(1, 10), marks({5}, 10), 150, begin=(1 << 32) + 12345, byz_strategy=s,
                coin_common=HALF)
    N, F, trials, a, c = 100, 40, 9000, 3333, 5000
    plan = plan_of(a_words(N, F), M13, N, F, first(2, N), marks({2 + (7 * i) % 98 for i in range(12)}, N),
                   byz_strategy=s, coin_common=HALF)
    whole = plan.run(0, trials)
    assert np.array_equal(whole, plan.run(0, a) + plan.run(a, c - a) + plan.run(c, trials - c))
    assert int(whole[:-1].sum()) == trials


# ------------------------------------------------------------ random delivery, Protocol A on modes 9 and 11
@every_strategy
@pytest.mark.parametrize("mode,coin", [(M9, 0), (M11, HALF), (M11, ALL)])
def test_random_delivery_bit_exact(mode, coin, name):
    """All four strategies at byz_one 1/2: both trial loops of csrc/benor_tally_byz.hip under both coins."""
    s = EVERY[name]
    kw = dict(byz_one=HALF, byz_strategy=s, coin_common=coin)
    h = check_exact(a_words(10, 4), mode, 10, 4, first(0, 10), marks({0, 4, 5, 9}, 10), 500, **kw)
    assert int(h[:-1].sum()) == 500
    check_exact(a_words(11, 2), mode, 11, 2, first(0, 11), marks({3, 8}, 11), 300, **kw)
    check_exact(a_words(70, 13), mode, 70, 13, first(5, 70), marks({8, 45}, 70), 50, **kw)
    check_exact(a_words(26, 5), mode, 26, 5, first(0, 26), marks(set(), 26), 200, **kw)       # b = 0: every step wave-uniform


# ------------------------------------------------------------ device against device
def twins(base, twin, N, F, f, ids, words, *, trials=2000, coin=0, states=(0, 7), **kw):
    """The plan of mode `base` with `words` against the plain plan of mode `twin`: histograms and states bit-equal, on
    different kernel entries."""
    faulty, byz = first(f, N), marks(ids, N)
    coin_of = lambda mode: {"coin_common": coin} if mode >= M10 else {}                      # noqa: E731
    common = dict(seed=SEED, k_max=16, byzantine=byz, **kw)
    mine = benor.TrialsPlan(N, F, faulty, mode=base, thresholds=words, **coin_of(base), **common)
    other = benor.TrialsPlan(N, F, faulty, mode=twin, **coin_of(twin), **common)
    assert mine.rule is not None and other.rule is None
    got, want = mine.run(7, trials), other.run(7, trials)
    assert np.array_equal(got, want), ({i: int(v) for i, v in enumerate(got) if v}, {i: int(v) for i, v in enumerate(want) if v})
    for t in states:
        _, st = benor.run_trial_states(N, F, faulty, trial=t, mode=base, thresholds=words, **coin_of(base), **common)
        assert st == benor.run_trial_states(N, F, faulty, trial=t, mode=twin, **coin_of(twin), **common)[1]


B_TWINS = [(64, 12, 0, {(5 * i) % 64 for i in range(12)}, 2000), (130, 46, 0, {0, 63, 64}, 1000),
           (200, 70, 0, set(range(64, 128)), 600), (1024, 204, 0, {(41 * i) % 1024 for i in range(16)}, 200)]
REF_TWINS = [(10, 4, 0, {2, 7}, 3000), (64, 21, 0, {1, 20, 40, 63}, 2000), (130, 46, 0, {0, 63, 64}, 1000)]   # N <= 3F + 1


@pytest.mark.parametrize("N,F,f,ids,trials", B_TWINS)
def test_protocol_b_words_equal_the_plain_plans(N, F, f, ids, trials):
    """thresholds=rule_protocol_b against modes 9, 11 and 13: the RuleT entries against the RuleB entries."""
    model.api_exists()
    words = benor.rule_protocol_b(N, F)
    for strategy in (SPLIT, BALANCE):
        twins(M13, M13, N, F, f, ids, words, trials=trials, byz_strategy=strategy)
        twins(M13, M13, N, F, f, ids, words, trials=trials, coin=HALF, byz_strategy=strategy)
    for strategy in EVERY.values():
        twins(M9, M9, N, F, f, ids, words, trials=trials // 2, byz_one=HALF, byz_strategy=strategy)
        twins(M11, M11, N, F, f, ids, words, trials=trials // 2, coin=HALF, byz_one=HALF, byz_strategy=strategy)


@pytest.mark.parametrize("N,F,f,ids,trials", REF_TWINS)
def test_reference_words_equal_modes_8_10_and_12(N, F, f, ids, trials):
    """(0, 0, 2F) on modes 9, 11 and 13 against modes 8, 10 and 12, where a quorum cannot hold F + 1 of both values."""
    model.api_exists()
    words = model.reference(N, F)
    for strategy in (SPLIT, BALANCE):
        twins(M13, M12, N, F, f, ids, words, trials=trials, byz_strategy=strategy)
        twins(M13, M12, N, F, f, ids, words, trials=trials, coin=ALL, byz_strategy=strategy)
    for strategy in EVERY.values():
        twins(M9, M8, N, F, f, ids, words, trials=trials // 2, byz_one=HALF, byz_strategy=strategy)
        twins(M11, M10, N, F, f, ids, words, trials=trials // 2, coin=HALF, byz_one=HALF, byz_strategy=strategy)


# ------------------------------------------------------------ the lumped chain
def lumped_exact(words, N, F, trials, *, seed=SEED, k_max=16, begin=0, init=None, **kw):
    plan = benor.LumpedPlan(N, F, seed=seed, k_max=k_max, initial_values=init, thresholds=words, **kw)
    got = plan.run(begin, trials)
    ref = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    restated = {}
    for t in range(begin, begin + trials):
        restated[t] = model.lumped_trial(words, N, F, seed, t, k_max, init=init, **kw)
        for b in restated[t][0]:
            ref[b] += 1
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        _, rounds, a, dec = restated[t]
        assert plan.trial(t) == {"a": a, "dec": dec, "rounds": rounds}, t
    return got


@both_strategies
@every_coin
def test_lumped_bit_exact(coin, name):
    s = SCHED[name]
    h = lumped_exact(a_words(10, 4), 10, 4, 400, byz_strategy=s, coin_common=coin)
    assert int(h[:-1].sum()) == 400 and int(h[-1]) == 0
    lumped_exact(a_words(64, 12), 64, 12, 100, b=12, byz_even=6, k_max=32, byz_strategy=s, coin_common=coin)
    lumped_exact(a_words(4096, 819), 4096, 819, 200, b=16, byz_even=8, k_max=8, byz_strategy=s, coin_common=coin)
    lumped_exact(a_words(1 << 24, 3355443), 1 << 24, 3355443, 200, k_max=8, byz_strategy=s, coin_common=coin)
    lumped_exact(a_words((1 << 23) - 1, 1677721), (1 << 23) - 1, 1677721, 200, k_max=8, byz_strategy=s, coin_common=coin)


@both_strategies
@every_coin
def test_lumped_protocol_b_words_equal_rule_1(coin, name):
    model.api_exists()
    for N, F, b in ((64, 12, 12), (4096, 819, 16), (1 << 20, 209715, 16)):
        kw = dict(b=b, byz_even=(b + 1) // 2, byz_strategy=SCHED[name], coin_common=coin, seed=SEED, k_max=16)
        got = benor.lumped_trials(N, F, 5, 3000, rule=0, thresholds=benor.rule_protocol_b(N, F), **kw)   # rule is not read
        assert np.array_equal(got, benor.lumped_trials(N, F, 5, 3000, rule=1, **kw))
        assert benor.lumped_trial(N, F, 9, thresholds=benor.rule_protocol_b(N, F), **kw) == benor.lumped_trial(N, F, 9, rule=1, **kw)


@both_strategies
@pytest.mark.parametrize("N,F,ids,init", [(64, 12, range(12), (26, 26, 0)), (4096, 819, range(16), (2040, 2040, 0))])
def test_lumped_equals_the_node_level_where_the_streams_coincide(N, F, ids, init, name):
    """Fixed starts and a coin common in every round: stream 12 is shared, no stream-13 word is drawn."""
    faulty, byz = [False] * N, marks(set(ids), N)
    words = a_words(N, F)
    values = lumped_model.fixed_values(N, faulty, byz, init)
    node = plan_of(words, M13, N, F, faulty, byz, init=values, byz_strategy=SCHED[name], coin_common=ALL).run(0, 2000)
    cls = benor.lumped_trials(N, F, 0, 2000, b=len(ids), byz_even=benor.byz_even(faulty, byz), byz_strategy=SCHED[name],
                              coin_common=ALL, seed=SEED, k_max=16, initial_values=init, thresholds=words)
    assert np.array_equal(node, cls), ({i: int(v) for i, v in enumerate(node) if v}, {i: int(v) for i, v in enumerate(cls) if v})


@both_strategies
def test_both_levels_have_the_exact_law(name):
    """Protocol A with local coins at (10, 4), 2 * 10^5 trials: the node level's device histogram and the lumped one
    both pass the 6 sigma gate against the DP; no trial violates agreement."""
    words = a_words(10, 4)
    law = model.exact_law(words, 10, 4, 0, (5, 5), SCHED[name], 16)
    node = plan_of(words, M13, 10, 4, [False] * 10, [False] * 10, byz_strategy=SCHED[name]).run(0, 200000)
    lumped_model.gate(node, law, f"node level A {name}")
    cls = benor.lumped_trials(10, 4, 0, 200000, byz_strategy=SCHED[name], seed=SEED, k_max=16, thresholds=words)
    lumped_model.gate(cls, law, f"class level A {name}")
    assert int(node[-1]) == 0 and int(cls[-1]) == 0


# ------------------------------------------------------------ the CLI
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=300,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_cli_trials_rule_a():
    N, F, trials = 64, 20, 3000
    base = ("trials", "--N", str(N), "--F", str(F), "--trials", str(trials), "--mode", "byzb", "--crashed", "0",
            "--byz-strategy", "split", "--k-max", "32", "--delivery", "adversarial")
    row = json.loads(_cli(*base, "--rule", "a").strip().splitlines()[-1])
    assert row["rule"] == "a" and row["rule_words"] == [64, 0, 40] and row["delivery"] == "adversarial"
    assert row["kernel"] == benor.KERNEL_NAMES[19]
    h = plan_of(a_words(N, F), M13, N, F, first(0, N), marks(set(), N), k_max=32, byz_strategy=SPLIT).run(0, trials)
    assert row["hist"] == [int(v) for v in h] and row["agreement_violations"] == 0
    words = json.loads(_cli(*base, "--rule", "64:0:40").strip().splitlines()[-1])
    assert words["rule"] == "64:0:40" and words["hist"] == row["hist"]
    plain = json.loads(_cli(*base).strip().splitlines()[-1])
    assert "rule" not in plain and "rule_words" not in plain            # without --rule the row is what it was
    b = json.loads(_cli(*base, "--rule", "b").strip().splitlines()[-1])
    assert b["hist"] == plain["hist"] and b["rule_words"] == [84, 20, 84]


@pytest.mark.parametrize("level", ["node", "class"])
def test_cli_sweep_rule_a(level):
    from benor import cli

    cells, per_cell = [(64, 8, 0), (256, 16, 0), (130, 46, 4)], 1000
    out = _cli("sweep", "--mode", "byzb", "--delivery", "adversarial", "--byz-strategy", "balance", "--k-max", "16",
               "--cells", ",".join(f"{N}:{F}:{b}" for N, F, b in cells), "--per-cell", str(per_cell), "--rule", "a",
               "--level", level)
    lines = out.strip().splitlines()
    keys = lines[0].split(",")
    assert keys[-1] == "rule" and len(lines) == 1 + len(cells)
    for line, (N, F, b) in zip(lines[1:], cells):
        row = dict(zip(keys, line.split(",")))
        seed = SEED ^ (N << 20) ^ F ^ (b << 44)
        if level == "class":
            h = benor.lumped_trials(N, F, 0, per_cell, b=b, byz_even=(b + 1) // 2, byz_strategy=BALANCE, seed=seed, k_max=16,
                                    thresholds=a_words(N, F))
        else:
            h = plan_of(a_words(N, F), M13, N, F, first(0, N), marks(set(range(b)), N), seed=seed,
                        byz_strategy=BALANCE).run(0, per_cell)
        want = cli.summarize(h, N, F, 16, 0)
        assert (int(row["N"]), int(row["F"]), int(row["b"]), row["rule"], row["mode"]) == (N, F, b, "a", "byzb")
        assert int(row["trials"]) == per_cell and int(row["undecided"]) == want["undecided"]
        assert int(row["agreement_violations"]) == want["agreement_violations"]
