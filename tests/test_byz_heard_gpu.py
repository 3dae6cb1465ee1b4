"""BO_BYZ_BALANCE and BO_BYZ_SPLIT on the device (benor_tally_heard_kernel in
csrc/benor_tally_byz.hip): bit-exact against the plain-Python restatement of their
definition in tests/test_byz_heard.py (histograms and per-node states), equality
with BO_MODE_RANDOM_TALLY3 without a Byzantine node, the provable N = 10, F = 3
outcome, and the JS and CLI surfaces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import test_byz_heard as model
from conftest import PKG, ROOT
from test_js_api import needs_node
from test_tally import first

pytestmark = pytest.mark.gpu

M8, BYZ = model.M8, model.BYZ
BALANCE, SPLIT = model.BALANCE, model.SPLIT                   # None before the strategies: every test fails
HALF, ALL = model.HALF, model.ALL
SEED = model.SEED
marks = model.marks
Q = "?"
both = pytest.mark.parametrize("name", ["BALANCE", "SPLIT"])


def strategy_of(name):
    model.strategies_exist()
    return {"BALANCE": BALANCE, "SPLIT": SPLIT}[name]


def gpu_hist(N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, kernel=None, **lie):
    model.strategies_exist()
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=M8, byzantine=byz, **lie)
    assert plan.kernel == (BYZ if kernel is None else kernel)
    h = plan.run(begin, trials)
    plan.check()                                              # no overflow or deferral state
    return h


def check_exact(N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, **lie):
    got = gpu_hist(N, F, faulty, byz, trials, seed=seed, k_max=k_max, begin=begin, init=init, **lie)
    ref = model.heard_hist(N, F, faulty, byz, seed, begin, trials, k_max, init, **lie)
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init,
                                            mode=M8, byzantine=byz, **lie)
        _, ref_rounds, ref_st = model.heard_trial(N, F, faulty, byz, seed, t, k_max, init, **lie)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
    return got


def minority_init(N):
    """Mostly 1s: every 23rd node starts at 0 and every 31st at "?"."""
    return [Q if i % 31 == 5 else 0 if i % 23 == 0 else 1 for i in range(N)]


@both
def test_bit_exact_one_liar(name):
    """(10, 4, f = 0), node 3 Byzantine."""
    h = check_exact(10, 4, first(0, 10), marks({3}, 10), 2000, byz_strategy=strategy_of(name))
    assert int(h[:-1].sum()) == 2000


@both
def test_bit_exact_as_many_liars_as_the_rule_tolerates_crashes(name):
    """(10, 4, f = 0), b = 4 = F: m = q + b.  SPLIT reaches the agreement-violation bin here."""
    h = check_exact(10, 4, first(0, 10), marks({0, 4, 5, 9}, 10), 2000, byz_strategy=strategy_of(name))
    assert int(h[-1]) > 1000 if name == "SPLIT" else int(h[:3].sum()) >= 1800   # (BALANCE: hardly anybody decides)


@both
def test_bit_exact_rows_at_the_edge_of_their_support(name):
    """(10, 4, f = 1), b = 3: f + b = F, m = q + b = 9."""
    check_exact(10, 4, first(1, 10), marks({1, 5, 9}, 10), 2000, byz_strategy=strategy_of(name))


@both
def test_k_max_one(name):
    h = check_exact(10, 4, first(0, 10), marks({2, 7}, 10), 2000, k_max=1, byz_strategy=strategy_of(name))
    assert int(h[:3].sum()) > 0


@both
@pytest.mark.parametrize("ids", [{4, 7}, {0, 1, 4, 7}])
def test_fixed_init_with_question_marks(name, ids):
    """(12, 4) with "?" starts: stage 2 runs in round 1's R-phase.  With two liars the three
    honest "?" outnumber them and the Byzantine class is walked; with four liars two honest "?"
    are left and the walk is theirs."""
    init = [Q, 1, 0, 1, Q, 0, 1, 0, 1, Q, 1, Q]               # nodes 0 and 4 may be liars: no initial value of the run
    check_exact(12, 4, first(0, 12), marks(ids, 12), 1000, init=init, byz_strategy=strategy_of(name))


@both
@pytest.mark.parametrize("ids", [{5 + 64}, {5 + 3, 5 + 40}])
def test_bit_exact_second_group_of_one_lane(name, ids):
    """(70, 24, f = 5), m = 65: compact index 64 is node 69.  Byzantine: group 1 has no
    receiver and draws nothing; honest with liars inside group 0: group 1 is one lane."""
    check_exact(70, 24, first(5, 70), marks(ids, 70), 300, byz_strategy=strategy_of(name))


@both
def test_bit_exact_three_groups(name):
    check_exact(130, 46, first(0, 130), marks({(13 * i) % 130 for i in range(10)}, 130), 100, byz_strategy=strategy_of(name))


@both
def test_bit_exact_walk_over_many_blocks(name):
    """(200, 70), b = 70: a P-phase with "?" proposals walks up to 70 members, many Philox blocks.
    (k_max 6 keeps BALANCE's long runs, and with them the restatement's time, short; some end undecided.)"""
    ids = {(17 * i) % 200 for i in range(70)}
    assert len(ids) == 70
    check_exact(200, 70, first(0, 200), marks(ids, 200), 50, k_max=6, byz_strategy=strategy_of(name))


@both
def test_bit_exact_large_network(name):
    """(1024, 340), b = 100, sixteen groups.  Fixed starts with few 0s and fewer "?" than liars: round 1's
    R-phase walks the 0s in stage 1 and the honest "?" in stage 2 at every receiver (random starts would
    walk a hundred members per receiver and step, half a minute of restatement)."""
    ids = {(41 * i) % 1024 for i in range(100)}
    assert len(ids) == 100
    check_exact(1024, 340, first(0, 1024), marks(ids, 1024), 30, init=minority_init(1024), byz_strategy=strategy_of(name))


@both
def test_bit_exact_thirty_two_groups(name):
    """(2048, 682), b = 300, with the same kind of starts."""
    ids = {(7 * i) % 2048 for i in range(300)}
    assert len(ids) == 300
    check_exact(2048, 682, first(0, 2048), marks(ids, 2048), 4, init=minority_init(2048), byz_strategy=strategy_of(name))


@both
def test_trial_begin_beyond_32_bits(name):
    check_exact(10, 4, first(1, 10), marks({1, 5, 9}, 10), 500, begin=(1 << 32) + 12345, byz_strategy=strategy_of(name))
    check_exact(70, 24, first(5, 70), marks({8, 45}, 70), 100, begin=(7 << 32) - 50, byz_strategy=strategy_of(name))


@both
def test_byz_one_is_not_read(name):
    a = gpu_hist(10, 4, first(0, 10), marks({2, 7}, 10), 2000, byz_one=0, byz_strategy=strategy_of(name))
    for w in (HALF, ALL):
        assert np.array_equal(a, gpu_hist(10, 4, first(0, 10), marks({2, 7}, 10), 2000, byz_one=w, byz_strategy=strategy_of(name)))


@both
def test_no_byzantine_node_is_mode_4(name):
    T3 = benor.BO_MODE_RANDOM_TALLY3
    for N, F, kernel in ((10, 4, benor.BO_KERNEL_TALLY3), (11, 4, benor.BO_KERNEL_TALLY)):
        ref = benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=16, mode=T3).run(0, 2000)
        got = gpu_hist(N, F, first(0, N), marks(set(), N), 2000, kernel=kernel, byz_one=HALF, byz_strategy=strategy_of(name))
        assert np.array_equal(got, ref)
        for t in (0, 1, 1999):
            a = benor.run_trial_states(N, F, first(0, N), seed=SEED, trial=t, k_max=16, mode=M8,
                                       byzantine=marks(set(), N), byz_strategy=strategy_of(name))
            assert a == benor.run_trial_states(N, F, first(0, N), seed=SEED, trial=t, k_max=16, mode=T3)


@both
def test_three_liars_cannot_move_unanimous_ones(name):
    """N = 10, F = 3, b = 3, every honest node starts at 1: every trial decides 1 in round 1
    (tests/test_byz_heard.py has the argument)."""
    h = gpu_hist(10, 3, first(0, 10), marks({1, 4, 8}, 10), 5000, init=[1] * 10, byz_strategy=strategy_of(name))
    assert int(h[1 * 3 + 1]) == 5000 and int(h.sum()) == 5000


@needs_node
@both
def test_js_run_trials(name, tmp_path):
    N, F, trials = 10, 4, 1000
    strategy = strategy_of(name)
    script = tmp_path / "heard.js"
    script.write_text(
        "const b = require(%s);\n"
        "if (b.BYZ_BALANCE !== 3 || b.BYZ_SPLIT !== 4) process.exit(2);\n"
        "const byz = new Array(%d).fill(false); byz[2] = true; byz[7] = true;\n"
        "b.runTrials({N: %d, F: %d, faultyList: new Array(%d).fill(false), seed: %dn, kMax: 16,\n"
        "             trialCount: %d, mode: b.MODE_BYZ_TALLY, byzantineList: byz, byzStrategy: b.BYZ_%s})\n"
        "  .then((h) => { console.log(JSON.stringify(Array.from(h, Number))); })\n"
        "  .catch((e) => { console.error(e); process.exit(1); });\n"
        % (json.dumps(os.path.join(PKG, "js", "index.js")), N, N, F, N, SEED, trials, name))
    p = subprocess.run(["node", str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array(json.loads(p.stdout.strip().splitlines()[-1]), dtype=np.uint64)
    assert np.array_equal(got, gpu_hist(N, F, first(0, N), marks({2, 7}, N), trials, byz_strategy=strategy))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


@both
def test_cli_trials_mode_byz(name):
    N, F, trials = 100, 36, 5000
    strategy = strategy_of(name)
    out = _cli("trials", "--N", str(N), "--F", str(F), "--trials", str(trials), "--mode", "byz", "--crashed", "2",
               "--byzantine", "12", "--byz-strategy", name.lower(), "--k-max", "16")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["mode"] == "byz" and row["crashed"] == 2 and row["m"] == N - 2 and row["trials"] == trials
    assert row["byzantine"] == 12 and row["byz_strategy"] == name.lower()
    byz = marks(set(range(2, 14)), N)                         # the 12 live nodes after the crashed ones
    h = gpu_hist(N, F, first(2, N), byz, trials, byz_one=HALF, byz_strategy=strategy)   # the CLI's default seed is SEED
    assert row["hist"] == [int(v) for v in h]
