"""BO_MODE_BYZ_RULE_B on the device (the RuleB entries of csrc/benor_tally_byz.hip): bit-exact
against the plain-Python restatement of its definition in tests/test_byz_rule_b.py
(histograms and per-node states), launch mechanics, the plans without a Byzantine node,
the properties that N > 5F guarantees, and the JS and CLI surfaces.  The mode-8 GPU tests
(tests/test_byz_tally_gpu.py, tests/test_byz_heard_gpu.py) are the check that variant 14,
which shares the trial loops, computes what it did."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import oracle
import test_byz_rule_b as model
from conftest import PKG, ROOT
from test_js_api import needs_node
from test_tally import first

pytestmark = pytest.mark.gpu

M9, BYZ_B = model.M9, model.BYZ_B                             # None before the mode: every test fails
RANDOM, OPPOSE, BALANCE, SPLIT = model.RANDOM, model.OPPOSE, model.BALANCE, model.SPLIT
STRATEGIES = model.STRATEGIES
ALL, HALF = model.ALL, model.HALF
SEED = model.SEED
marks = model.marks
Q = "?"
every_strategy = pytest.mark.parametrize("name", list(STRATEGIES))
every_byz_one = pytest.mark.parametrize("byz_one", [0, HALF, ALL])


def gpu_hist(N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, mode=None, kernel=None, **lie):
    model.mode_exists()
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=M9 if mode is None else mode,
                            byzantine=byz, **lie)
    assert plan.kernel == (BYZ_B if kernel is None else kernel)
    h = plan.run(begin, trials)
    plan.check()                                              # no overflow or deferral state
    return h


def check_exact(N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, **lie):
    """The launch's histogram, and the per-node states of its first two and last trials, against the restatement
    (each trial restated once)."""
    got = gpu_hist(N, F, faulty, byz, trials, seed=seed, k_max=k_max, begin=begin, init=init, **lie)
    ref = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    restated = {}
    for t in range(begin, begin + trials):
        restated[t] = model.rule_b_trial(N, F, faulty, byz, seed, t, k_max, init, **lie)
        for b in restated[t][0]:
            ref[b] += 1
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init,
                                            mode=M9, byzantine=byz, **lie)
        _, ref_rounds, ref_st = restated[t]
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
    return got


def minority_init(N):
    """Mostly 1s: every 23rd node starts at 0 and every 31st at "?"."""
    return [Q if i % 31 == 5 else 0 if i % 23 == 0 else 1 for i in range(N)]


@every_strategy
@every_byz_one
@pytest.mark.parametrize("ids", [{3}, {3, 8}])
def test_bit_exact_11_2(ids, byz_one, name):
    """(11, 2, f = 0), one and two liars, 300 trials: N > 5F, so nothing lands in a forbidden bin either."""
    h = check_exact(11, 2, first(0, 11), marks(ids, 11), 300, byz_one=byz_one, byz_strategy=STRATEGIES[name])
    assert int(h[:-1].sum()) == 300 and model.forbidden_bins(h) == 0


@every_strategy
def test_bit_exact_a_crashed_node_and_a_liar(name):
    """(11, 2, f = 1), b = 1: f + b = F, m = q + b = 10."""
    check_exact(11, 2, first(1, 11), marks({6}, 11), 300, byz_one=HALF, byz_strategy=STRATEGIES[name])


@every_strategy
def test_outside_the_bound(name):
    """(10, 4), b = 4, N <= 5F: a proposal needs 2 c > 14 of q = 6 messages; no validation, nothing decides."""
    h = check_exact(10, 4, first(0, 10), marks({0, 4, 5, 9}, 10), 200, k_max=32, byz_one=HALF, byz_strategy=STRATEGIES[name])
    assert int(h[:3].sum()) == 200


@every_strategy
def test_k_max_one(name):
    h = check_exact(11, 2, first(0, 11), marks({2, 7}, 11), 500, k_max=1, byz_one=HALF, byz_strategy=STRATEGIES[name])
    assert int(h[:3].sum()) > 0 and int(h[3:6].sum()) > 0


@every_strategy
@pytest.mark.parametrize("ids", [{4}, {0, 4}])
def test_fixed_init_with_question_marks(name, ids):
    """(12, 2) with "?" starts: under BALANCE and SPLIT stage 2 runs in round 1's R-phase."""
    init = [Q, 1, 0, 1, Q, 1, 1, 0, 1, Q, 1, 1]               # nodes 0 and 4 may be liars: no initial value of the run
    check_exact(12, 2, first(0, 12), marks(ids, 12), 300, init=init, byz_one=HALF, byz_strategy=STRATEGIES[name])


@every_strategy
@every_byz_one
def test_no_byzantine_node_with_every_crash_the_rule_allows(name, byz_one):
    """(11, 2, f = 2, b = 0): m == q, every live sender is in every inbox."""
    h = check_exact(11, 2, first(2, 11), marks(set(), 11), 300, byz_one=byz_one, byz_strategy=STRATEGIES[name])
    assert model.forbidden_bins(h) == 0


def test_no_byzantine_node_26_5():
    """(26, 5), b = 0, with and without crashed nodes: one histogram for every strategy and byz_one, the
    restatement's, and not mode 4's (the rule differs)."""
    for f in (0, 3):
        ref = check_exact(26, 5, first(f, 26), marks(set(), 26), 300, byz_one=0, byz_strategy=RANDOM)
        for strategy in STRATEGIES.values():
            for w in (0, HALF, ALL):
                assert np.array_equal(ref, gpu_hist(26, 5, first(f, 26), marks(set(), 26), 300, byz_one=w, byz_strategy=strategy))
        assert np.array_equal(ref, gpu_hist(26, 5, first(f, 26), None, 300))          # no byzantine= at all
        mode4 = benor.TrialsPlan(26, 5, first(f, 26), seed=SEED, k_max=16, mode=benor.BO_MODE_RANDOM_TALLY3).run(0, 300)
        assert not np.array_equal(ref, mode4)


@every_strategy
def test_group_boundary_liar_in_lane_0_of_group_1(name):
    """(70, 13, f = 0): compact index 64 is Byzantine, group 1 has five receivers."""
    check_exact(70, 13, first(0, 70), marks({64}, 70), 100, byz_one=HALF, byz_strategy=STRATEGIES[name])


@every_strategy
def test_group_boundary_three_groups(name):
    """(130, 25, f = 0): liars in all three groups; group 2 is nodes 128 (a liar) and 129, one honest lane."""
    ids = {0, 63, 64, 100, 128}
    check_exact(130, 25, first(0, 130), marks(ids, 130), 40, byz_one=HALF, byz_strategy=STRATEGIES[name])


@every_strategy
def test_more_liars_than_lanes(name):
    """(400, 70), b = 70 = F: N > 5F at its edge (5F = 350), nearly every lane has class sizes of its own."""
    ids = {(17 * i) % 400 for i in range(70)}
    assert len(ids) == 70
    h = check_exact(400, 70, first(0, 400), marks(ids, 400), 3, byz_one=HALF, byz_strategy=STRATEGIES[name])
    assert model.forbidden_bins(h) == 0


@every_strategy
@pytest.mark.parametrize("starts,trials", [("minority", 30), ("random", 4)])
def test_bit_exact_large_network(name, starts, trials):
    """(1024, 204), b = 16, sixteen groups, both entries.  With 95 % ones at the start every trial decides in
    round 1; random starts run k_max rounds of proposals of "?" and coins."""
    ids = {(41 * i) % 1024 for i in range(16)}
    assert len(ids) == 16
    init = minority_init(1024) if starts == "minority" else None
    check_exact(1024, 204, first(0, 1024), marks(ids, 1024), trials, init=init, byz_one=HALF, byz_strategy=STRATEGIES[name])


@pytest.mark.parametrize("name", ["RANDOM", "OPPOSE"])
def test_bit_exact_thresholds_searched_in_global_memory(name):
    """(2048, 682), b = 300: variant 14's LDS layout, so as in tests/test_byz_tally_gpu.py the 2400 B of
    thresholds would cost a resident workgroup and are searched in global memory.  N <= 5F: every trial runs
    all k_max rounds, 55 936 receiver-steps that the restatement walks one by one, so two trials."""
    ids = {(7 * i) % 2048 for i in range(300)}
    assert len(ids) == 300
    check_exact(2048, 682, first(0, 2048), marks(ids, 2048), 2, byz_one=HALF, byz_strategy=STRATEGIES[name])


@every_strategy
def test_trial_begin_beyond_32_bits(name):
    strategy = STRATEGIES[name]
    check_exact(11, 2, first(1, 11), marks({5}, 11), 200, begin=(1 << 32) + 12345, byz_one=HALF, byz_strategy=strategy)
    check_exact(70, 13, first(5, 70), marks({8, 45}, 70), 50, begin=(7 << 32) - 25, byz_one=HALF, byz_strategy=strategy)


@every_strategy
def test_split_invariance(name):
    N, F, trials, a, c = 100, 19, 9000, 3333, 5000
    model.mode_exists()
    plan = benor.TrialsPlan(N, F, first(2, N), seed=SEED, k_max=16, mode=M9,
                            byzantine=marks({2 + (7 * i) % 98 for i in range(12)}, N), byz_one=HALF,
                            byz_strategy=STRATEGIES[name])
    assert plan.kernel == BYZ_B
    whole = plan.run(0, trials)
    parts = plan.run(0, a) + plan.run(a, c - a) + plan.run(c, trials - c)
    assert np.array_equal(whole, parts)
    assert int(whole[:-1].sum()) == trials and model.forbidden_bins(whole) == 0


@pytest.mark.parametrize("N,F,f,ids,init,name", [
    (10, 4, 1, {1, 5, 9}, None, "RANDOM"),
    (10, 4, 0, {0, 9}, [Q, 1, 0, Q, 1, 1, 0, 0, 1, 0], "SPLIT"),
    (130, 25, 1, {1, 64, 65, 100, 129}, None, "RANDOM"),
    (130, 25, 0, {0, 63, 64}, [Q if i % 9 == 0 else 1 if i % 7 else 0 for i in range(130)], "OPPOSE"),
    (130, 25, 2, {2, 66, 129}, None, "BALANCE"),
])
def test_per_node_states(N, F, f, ids, init, name):
    """bo_run_trial_states over 30 trials with crashed, Byzantine and honest nodes."""
    model.mode_exists()
    faulty, byz, strategy = first(f, N), marks(ids, N), STRATEGIES[name]
    for t in range(30):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, initial_values=init, mode=M9,
                                            byzantine=byz, byz_one=HALF, byz_strategy=strategy)
        _, ref_rounds, ref_st = model.rule_b_trial(N, F, faulty, byz, SEED, t, 16, init, byz_one=HALF, byz_strategy=strategy)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
        for i in ids:
            assert st[i] == {"killed": False, "x": None, "decided": None, "k": None}
        for i in range(f):
            assert st[i] == {"killed": True, "x": None, "decided": None, "k": None}


def test_properties_on_the_device():
    """(11, 2), b = 2, SPLIT, 10^5 trials, k_max 32: this rule never violates agreement where mode 8's rule
    does on the same trials, and a unanimous honest start v decides v in round 1."""
    N, F, trials, byz = 11, 2, 100000, marks({3, 8}, 11)
    got = gpu_hist(N, F, first(0, N), byz, trials, k_max=32, byz_strategy=SPLIT)
    ref = gpu_hist(N, F, first(0, N), byz, trials, k_max=32, byz_strategy=SPLIT, mode=benor.BO_MODE_BYZ_TALLY,
                   kernel=benor.BO_KERNEL_TALLY_BYZ)
    print(f"(11, 2), b = 2, SPLIT, {trials} trials: agreement violations {int(ref[-1])} under the reference rule, "
          f"{int(got[-1])} under Protocol B; undecided {int(ref[:3].sum())}, {int(got[:3].sum())}")
    assert int(got[:-1].sum()) == trials == int(ref[:-1].sum())
    assert model.forbidden_bins(got, 32) == 0 and int(ref[-1]) > 0
    for v in (0, 1):
        for strategy in STRATEGIES.values():
            h = gpu_hist(N, F, first(0, N), byz, trials, k_max=32, init=[v] * N, byz_one=HALF, byz_strategy=strategy)
            assert int(h[3 + v]) == trials and int(h.sum()) == trials


@needs_node
@pytest.mark.parametrize("name", ["OPPOSE", "SPLIT"])
def test_js_run_trials_mode_9(name, tmp_path):
    N, F, trials = 11, 2, 1000
    script = tmp_path / "byzb.js"
    script.write_text(
        "const b = require(%s);\n"
        "if (b.MODE_BYZ_RULE_B !== 9 || b.MODE_BYZ_TALLY !== 8) process.exit(2);\n"
        "const byz = new Array(%d).fill(false); byz[2] = true; byz[7] = true;\n"
        "b.runTrials({N: %d, F: %d, faultyList: new Array(%d).fill(false), seed: %dn, kMax: 16,\n"
        "             trialCount: %d, mode: b.MODE_BYZ_RULE_B, byzantineList: byz, byzOne: 0x80000000,\n"
        "             byzStrategy: b.BYZ_%s})\n"
        "  .then((h) => { console.log(JSON.stringify(Array.from(h, Number))); })\n"
        "  .catch((e) => { console.error(e); process.exit(1); });\n"
        % (json.dumps(os.path.join(PKG, "js", "index.js")), N, N, F, N, SEED, trials, name))
    p = subprocess.run(["node", str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array(json.loads(p.stdout.strip().splitlines()[-1]), dtype=np.uint64)
    assert np.array_equal(got, gpu_hist(N, F, first(0, N), marks({2, 7}, N), trials, byz_one=HALF, byz_strategy=STRATEGIES[name]))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


@pytest.mark.parametrize("name", ["random", "balance"])
def test_cli_trials_mode_byzb(name):
    N, F, trials = 100, 19, 5000
    out = _cli("trials", "--N", str(N), "--F", str(F), "--trials", str(trials), "--mode", "byzb", "--crashed", "2",
               "--byzantine", "12", "--byz-one", "0.5", "--byz-strategy", name, "--k-max", "16")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["mode"] == "byzb" and row["crashed"] == 2 and row["m"] == N - 2 and row["trials"] == trials
    assert row["byzantine"] == 12 and row["byz_one"] == 0.5 and row["byz_one_word"] == HALF
    assert row["byz_strategy"] == name and row["kernel"] == benor.KERNEL_NAMES[BYZ_B]
    byz = marks(set(range(2, 14)), N)                         # the 12 live nodes after the crashed ones
    h = gpu_hist(N, F, first(2, N), byz, trials, byz_one=HALF, byz_strategy=STRATEGIES[name.upper()])   # the CLI's default seed is SEED
    assert row["hist"] == [int(v) for v in h] and row["agreement_violations"] == 0
