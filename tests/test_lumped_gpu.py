"""The lumped API on the device (csrc/benor_lumped.hip): bit-exact against the plain-Python restatement in
tests/test_lumped.py (histograms and bo_lumped_trial states), independence of the launch split and the grid, device
against device with modes 12 and 13 where the streams coincide, both devices' laws against the exact DP, and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import oracle
import test_byz_sched as sched
import test_lumped as model
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

BALANCE, SPLIT = model.BALANCE, model.SPLIT
STRATEGIES = model.STRATEGIES
ALL, HALF = model.ALL, model.HALF
SEED = model.SEED
RULES = {"ref": 0, "b": 1}
both_strategies = model.both_strategies
both_rules = model.both_rules
every_coin = pytest.mark.parametrize("coin", [0, HALF, ALL])


def plan_of(rule, N, F, *, seed=SEED, k_max=16, init=None, **kw):
    model.api_exists()
    return benor.LumpedPlan(N, F, rule=RULES[rule], seed=seed, k_max=k_max, initial_values=init, **kw)


def check_exact(rule, N, F, trials, *, seed=SEED, k_max=16, begin=0, init=None, **kw):
    """The launch's histogram, and the states of its first two and last trials, against the restatement (each trial
    restated once)."""
    plan = plan_of(rule, N, F, seed=seed, k_max=k_max, init=init, **kw)
    got = plan.run(begin, trials)
    ref = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    restated = {}
    for t in range(begin, begin + trials):
        restated[t] = model.lumped_trial(rule, N, F, seed, t, k_max, init=init, **kw)
        for b in restated[t][0]:
            ref[b] += 1
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        _, rounds, a, dec = restated[t]
        assert plan.trial(t) == {"a": a, "dec": dec, "rounds": rounds}, t
    return got


@both_rules
@both_strategies
@every_coin
def test_bit_exact_small(coin, name, rule):
    """(10, 4, b = 0), and (11, 2) with one and two liars of either parity: byz_even 0, 1 and 2."""
    s = STRATEGIES[name]
    h = check_exact(rule, 10, 4, 400, byz_strategy=s, coin_common=coin)
    assert int(h[:-1].sum()) == 400
    for b, even in ((1, 0), (1, 1), (2, 0), (2, 1), (2, 2)):
        h = check_exact(rule, 11, 2, 200, b=b, byz_even=even, byz_strategy=s, coin_common=coin)
        assert int(h[:-1].sum()) == 200
        if rule == "b":
            assert model.mode9.forbidden_bins(h) == 0


@both_rules
@both_strategies
@every_coin
def test_bit_exact_shapes(coin, name, rule):
    """A parity without an honest node, all liars on one parity, and h_0 != h_1."""
    s = STRATEGIES[name]
    check_exact(rule, 3, 2, 200, b=2, byz_even=2, byz_strategy=s, coin_common=coin)          # h = (0, 1)
    check_exact(rule, 64, 12, 100, b=12, byz_even=12, k_max=32, byz_strategy=s, coin_common=coin)   # h = (20, 32)
    check_exact(rule, 64, 12, 100, b=12, byz_even=6, k_max=8, byz_strategy=s, coin_common=coin)
    check_exact(rule, 65, 12, 100, byz_strategy=s, coin_common=coin)                          # h = (33, 32)
    check_exact(rule, 130, 46, 100, f=3, b=20, byz_even=3, byz_strategy=s, coin_common=coin)  # h = (61, 46)


@both_rules
@both_strategies
@every_coin
def test_fixed_starts(coin, name, rule):
    """Round 1's class sizes: "?" starts, balanced starts that take coins, and Hq >= q."""
    s = STRATEGIES[name]
    check_exact(rule, 12, 2, 200, b=2, byz_even=1, init=(2, 5, 3), byz_strategy=s, coin_common=coin)
    check_exact(rule, 12, 2, 200, b=2, byz_even=2, init=(4, 3, 3), byz_strategy=s, coin_common=coin)
    check_exact(rule, 12, 4, 100, b=2, byz_even=0, init=(1, 1, 8), byz_strategy=s, coin_common=coin)   # q = 8 = Hq
    check_exact(rule, 12, 4, 100, init=(0, 0, 12), byz_strategy=s, coin_common=coin)


@both_rules
@both_strategies
@every_coin
def test_round_cap(coin, name, rule):
    """k_max 1 and k_max 1024 at (10, 5)."""
    s = STRATEGIES[name]
    h = check_exact(rule, 10, 5, 400, k_max=1, byz_strategy=s, coin_common=coin)
    assert int(h[:-1].sum()) == 400
    h = check_exact(rule, 10, 5, 100, k_max=1024, byz_strategy=s, coin_common=coin)
    assert int(h[:-1].sum()) == 100 and len(h) == 1025 * 3 + 1


@both_rules
@both_strategies
@every_coin
def test_bit_exact_large(coin, name, rule):
    """(2^20 + 1, 209715, b = 16), 2000 trials (with local coins at coin 0; the start is random at every coin): h = 0xFFFF1 and h_pi = 0x7FFF9, 0x7FFF8 read every
    table from k = 7 to 19 and up to 17 words; (2^23 - 1, 1677721): h = 0x7FFFFF reads the tables to k = 22 and 23
    words; (2^24, 3355443): the top of the admitted range, k = 24 and 23."""
    s = STRATEGIES[name]
    check_exact(rule, (1 << 20) + 1, 209715, 2000, b=16, byz_even=8, k_max=8, byz_strategy=s, coin_common=coin)
    check_exact(rule, (1 << 23) - 1, 1677721, 300, k_max=8, byz_strategy=s, coin_common=coin)
    check_exact(rule, 1 << 24, 3355443, 200, k_max=8, byz_strategy=s, coin_common=coin)
    check_exact(rule, 1 << 24, 3355443, 200, f=1, b=3355442, byz_even=1677721, k_max=4, byz_strategy=s, coin_common=coin)


@both_rules
def test_results_do_not_depend_on_the_launch_split_or_the_grid(rule, monkeypatch):
    """Trial ids above 2^32; one launch against three; two trial counts with different grids; a grid so small
    that every lane runs several trials, against the default."""
    begin = 2 ** 32 + 12345
    plan = plan_of(rule, 1000, 30, b=7, byz_even=4, k_max=32)
    check_exact(rule, 1000, 30, 300, begin=begin, b=7, byz_even=4, k_max=32)
    whole = plan.run(begin, 100000)                                       # 391 workgroups
    parts = plan.run(begin, 300) + plan.run(begin + 300, 70000) + plan.run(begin + 70300, 29700)   # 2, 274 and 117
    assert np.array_equal(whole, parts) and int(whole[:-1].sum()) == 100000
    big = plan.run(begin, 200000)
    assert np.array_equal(big - whole, plan.run(begin + 100000, 100000))
    monkeypatch.setenv("BENOR_BLOCKS_PER_CU", "1")                        # a lane's next trial in the same loop
    assert np.array_equal(big, plan.run(begin, 200000))
    assert plan.trial(begin + 7) == plan_of(rule, 1000, 30, b=7, byz_even=4, k_max=32).trial(begin + 7)


@both_rules
def test_a_lane_starts_its_next_trial_bit_exact(rule, monkeypatch):
    """One workgroup per CU: 256 CUs of 256 lanes are 65536 lanes, and 70000 trials make 4464 of them end a trial and
    start their next id in the same loop iteration, with random starts and a coin common in half the rounds.  Against
    the restatement (a few seconds of it: the trial count is what the grid needs), so the path stays tested however
    the grid comes to be chosen."""
    monkeypatch.setenv("BENOR_BLOCKS_PER_CU", "1")
    h = check_exact(rule, 10, 4, 70000, k_max=8, coin_common=HALF)
    assert int(h[:-1].sum()) == 70000


# ------------------------------------------------------------ device against device, modes 12 and 13
@both_rules
@both_strategies
@pytest.mark.parametrize("N,F,ids,init", [(64, 12, range(12), (26, 26, 0)), (200, 70, range(64, 128), (68, 60, 8)),
                                          (4096, 819, range(16), (2040, 2040, 0))])
def test_same_histogram_as_the_node_level_where_the_streams_coincide(N, F, ids, init, name, rule):
    """Fixed starts and a coin common in every round: stream 12 is shared, no stream-13 word is drawn."""
    faulty, byz = [False] * N, sched.marks(set(ids), N)
    values = model.fixed_values(N, faulty, byz, init)
    node = benor.TrialsPlan(N, F, faulty, seed=SEED, k_max=16, initial_values=values, mode=sched.mode_of(rule),
                            byzantine=byz, byz_strategy=STRATEGIES[name], coin_common=ALL).run(0, 2000)
    cls = plan_of(rule, N, F, b=len(ids), byz_even=benor.byz_even(faulty, byz), byz_strategy=STRATEGIES[name],
                  coin_common=ALL, init=init).run(0, 2000)
    assert np.array_equal(node, cls), ({i: int(v) for i, v in enumerate(node) if v}, {i: int(v) for i, v in enumerate(cls) if v})


@both_rules
@both_strategies
def test_both_levels_have_the_exact_law(name, rule):
    """Local coins at (10, 4), 2 * 10^5 trials: mode 12/13's device histogram and the lumped one both pass the
    6 sigma gate against the DP."""
    law = model.exact_law(rule, 10, 4, 0, (5, 5), STRATEGIES[name], 16)
    node = benor.TrialsPlan(10, 4, [False] * 10, seed=SEED, k_max=16, mode=sched.mode_of(rule), byzantine=[False] * 10,
                            byz_strategy=STRATEGIES[name]).run(0, 200000)
    model.gate(node, law, f"node level {rule} {name}")
    model.gate(plan_of(rule, 10, 4, byz_strategy=STRATEGIES[name]).run(0, 200000), law, f"class level {rule} {name}")


def test_law_with_table_draws():
    """(600, 40, b = 4): h_pi = 298 draws from the k = 8 table; the DP over 596 honest nodes, 50000 trials."""
    law = model.exact_law("ref", 600, 40, 4, (298, 298), BALANCE, 8)
    model.gate(plan_of("ref", 600, 40, b=4, byz_even=2, k_max=8).run(0, 50000), law, "(600, 40, 4)")


# ------------------------------------------------------------ the CLI
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=300,
                          env=env, cwd=ROOT)


def test_cli_trials_class_level():
    p = _cli("trials", "--N", "5000", "--F", "100", "--trials", "3000", "--crashed", "2", "--byzantine", "7", "--mode", "byzb",
             "--delivery", "adversarial", "--byz-strategy", "split", "--level", "class", "--coin-common", "0.5", "--begin", "17")
    assert p.returncode == 0, p.stderr
    row = json.loads(p.stdout)
    want = benor.lumped_trials(5000, 100, 17, 3000, f=2, b=7, byz_even=4, rule=1, byz_strategy=SPLIT, coin_common=HALF,
                               seed=SEED, k_max=16)
    assert row["hist"] == [int(v) for v in want]
    assert row["level"] == "class" and row["delivery"] == "adversarial" and row["m"] == 4998 and row["byz_even"] == 4
    # the node level's row has no level field, as before
    p = _cli("trials", "--N", "64", "--F", "12", "--trials", "100", "--crashed", "0", "--mode", "byz", "--delivery",
             "adversarial", "--byz-strategy", "split")
    assert p.returncode == 0 and "level" not in json.loads(p.stdout)


def test_cli_sweep_class_level():
    from benor import cli

    cells = [(64, 8, 0), (256, 20, 4), (5000, 100, 10)]
    p = _cli("sweep", "--cells", ",".join(":".join(map(str, c)) for c in cells), "--per-cell", "2000", "--mode", "byz",
             "--delivery", "adversarial", "--byz-strategy", "balance", "--level", "class", "--k-max", "16")
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    keys = lines[0].split(",")
    assert keys[-2:] == ["delivery", "level"] and len(lines) == 4
    for line, (N, F, b) in zip(lines[1:], cells):
        row = dict(zip(keys, line.split(",")))
        h = benor.lumped_trials(N, F, 0, 2000, b=b, byz_even=(b + 1) // 2, byz_strategy=BALANCE,
                                seed=SEED ^ (N << 20) ^ F ^ (b << 44), k_max=16)
        want = cli.summarize(h, N, F, 16, 0)
        assert (int(row["N"]), int(row["F"]), int(row["b"]), row["level"]) == (N, F, b, "class")
        assert int(row["trials"]) == 2000 and int(row["undecided"]) == want["undecided"]
        assert float(row["decided_frac"]) == want["decided_frac"] and int(row["agreement_violations"]) == want["agreement_violations"]
