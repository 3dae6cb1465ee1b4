"""BO_MODE_BYZ_TALLY on the device (csrc/benor_tally_byz.hip): bit-exact against
the plain-Python restatement of its definition in tests/test_byz_tally.py
(histograms and per-node states), launch mechanics, equality with
BO_MODE_RANDOM_TALLY3 without a Byzantine node, the law against that file's
mask-level simulation, the reachable agreement violations, and the JS and CLI
surfaces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import test_byz_tally as model
from conftest import PKG, ROOT
from test_js_api import needs_node
from test_tally import chi2_two_sample, first

pytestmark = pytest.mark.gpu

M8 = getattr(benor, "BO_MODE_BYZ_TALLY", None)               # absent before the mode: every test fails
BYZ = getattr(benor, "BO_KERNEL_TALLY_BYZ", None)
RANDOM, OPPOSE = model.RANDOM, model.OPPOSE
ALL, HALF, QUARTER = model.ALL, model.HALF, model.QUARTER
SEED = model.SEED
marks = model.marks
Q = "?"


def gpu_hist(N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, kernel=None, **lie):
    assert M8 == 8
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=M8, byzantine=byz, **lie)
    assert plan.kernel == (BYZ if kernel is None else kernel)
    h = plan.run(begin, trials)
    plan.check()                                              # no overflow or deferral state
    return h


def check_exact(N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, **lie):
    got = gpu_hist(N, F, faulty, byz, trials, seed=seed, k_max=k_max, begin=begin, init=init, **lie)
    ref = model.byz_hist(N, F, faulty, byz, seed, begin, trials, k_max, init, **lie)
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init,
                                            mode=M8, byzantine=byz, **lie)
        _, ref_rounds, ref_st = model.byz_trial(N, F, faulty, byz, seed, t, k_max, init, **lie)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
    return got


@pytest.mark.parametrize("byz_one", [0, HALF, ALL])
def test_bit_exact_one_liar(byz_one):
    """(10, 4, f = 0), node 3 Byzantine: always 0, a fair coin per receiver and step, always 1."""
    h = check_exact(10, 4, first(0, 10), marks({3}, 10), 2000, byz_one=byz_one)
    assert int(h[:-1].sum()) == 2000


@pytest.mark.parametrize("byz_one", [HALF, QUARTER])
def test_bit_exact_as_many_liars_as_the_rule_tolerates_crashes(byz_one):
    """(10, 4, f = 0), b = 4 = F: m = q + b."""
    check_exact(10, 4, first(0, 10), marks({0, 4, 5, 9}, 10), 2000, byz_one=byz_one)


def test_bit_exact_oppose():
    check_exact(10, 4, first(0, 10), marks({2, 7}, 10), 2000, byz_one=HALF, byz_strategy=OPPOSE)


def test_k_max_one():
    h = check_exact(10, 4, first(0, 10), marks({2, 7}, 10), 2000, k_max=1, byz_one=HALF)
    assert int(h[:3].sum()) > 0


def test_bit_exact_rows_at_the_edge_of_their_support():
    """(10, 4, f = 1), b = 3: f + b = F, m = q + b = 9."""
    check_exact(10, 4, first(1, 10), marks({1, 5, 9}, 10), 2000, byz_one=HALF)


@pytest.mark.parametrize("strategy", [RANDOM, OPPOSE])
def test_fixed_init_with_question_marks(strategy):
    init = [Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1, 0]
    byz = marks({4, 7}, 12)                                   # one of the "?" is a liar's: no initial value of the run
    check_exact(12, 4, first(0, 12), byz, 1000, init=init, byz_one=HALF, byz_strategy=strategy)


@pytest.mark.parametrize("ids", [{5 + 64}, {5 + 3, 5 + 40}])
def test_bit_exact_second_group_of_one_lane(ids):
    """(70, 24, f = 5), m = 65: compact index 64 is node 69.  Byzantine: group 1 has no
    receiver and draws nothing; honest with liars inside group 0: group 1 is one lane."""
    check_exact(70, 24, first(5, 70), marks(ids, 70), 300, byz_one=HALF)


def test_bit_exact_three_groups():
    check_exact(130, 46, first(0, 130), marks({(13 * i) % 130 for i in range(10)}, 130), 100, byz_one=HALF)


def test_bit_exact_more_liars_than_lanes():
    """(200, 70), b = 70: nearly every lane has class sizes of its own."""
    ids = {(17 * i) % 200 for i in range(70)}
    assert len(ids) == 70
    check_exact(200, 70, first(0, 200), marks(ids, 200), 50, byz_one=HALF)


@pytest.mark.parametrize("strategy", [RANDOM, OPPOSE])
def test_bit_exact_large_network(strategy):
    ids = {(41 * i) % 1024 for i in range(100)}
    assert len(ids) == 100
    check_exact(1024, 340, first(0, 1024), marks(ids, 1024), 30, byz_one=HALF, byz_strategy=strategy)


@pytest.mark.parametrize("strategy", [RANDOM, OPPOSE])
def test_bit_exact_thresholds_searched_in_global_memory(strategy):
    """(2048, 682), b = 300: a workgroup's LDS is 208 B of histogram and 4 x (4 x 32 + 682) x 8 B,
    26128 B, six workgroups per CU in 512-byte granules of 160 KiB; the 2400 B of thresholds would
    leave five, so the kernel searches them where they lie in global memory (every smaller shape
    above keeps them in LDS)."""
    ids = {(7 * i) % 2048 for i in range(300)}
    assert len(ids) == 300
    check_exact(2048, 682, first(0, 2048), marks(ids, 2048), 4, byz_one=HALF, byz_strategy=strategy)


def test_trial_begin_beyond_32_bits():
    check_exact(10, 4, first(1, 10), marks({1, 5, 9}, 10), 500, begin=(1 << 32) + 12345, byz_one=HALF)
    check_exact(70, 24, first(5, 70), marks({8, 45}, 70), 100, begin=(7 << 32) - 50, byz_one=HALF)


def test_split_invariance():
    N, F, trials, a = 100, 36, 10000, 3333
    assert M8 == 8
    plan = benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=16, mode=M8,
                            byzantine=marks({(7 * i) % N for i in range(12)}, N), byz_one=HALF)
    assert plan.kernel == BYZ
    whole = plan.run(0, trials)
    parts = plan.run(0, a) + plan.run(a, trials - a)
    assert np.array_equal(whole, parts)
    assert int(whole[:-1].sum()) == trials


def test_no_byzantine_node_is_mode_4():
    T3 = benor.BO_MODE_RANDOM_TALLY3
    for N, F, kernel in ((10, 4, benor.BO_KERNEL_TALLY3), (11, 4, benor.BO_KERNEL_TALLY)):
        ref = benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=16, mode=T3).run(0, 2000)
        for strategy, w in ((RANDOM, 0), (RANDOM, HALF), (OPPOSE, ALL)):
            got = gpu_hist(N, F, first(0, N), marks(set(), N), 2000, kernel=kernel, byz_one=w, byz_strategy=strategy)
            assert np.array_equal(got, ref)
        for t in (0, 1, 1999):
            a = benor.run_trial_states(N, F, first(0, N), seed=SEED, trial=t, k_max=16, mode=M8,
                                       byzantine=marks(set(), N), byz_one=HALF)
            assert a == benor.run_trial_states(N, F, first(0, N), seed=SEED, trial=t, k_max=16, mode=T3)


@pytest.mark.parametrize("N,F,f,ids,init,strategy", [
    (10, 4, 1, {1, 5, 9}, None, RANDOM),
    (10, 4, 0, {0, 9}, [Q, 1, 0, Q, 1, 1, 0, 0, 1, 0], OPPOSE),
    (130, 46, 1, {1, 64, 65, 100, 129}, None, RANDOM),
    (130, 46, 0, {0, 63, 64}, [Q if i % 9 == 0 else i % 2 for i in range(130)], OPPOSE),
])
def test_per_node_states(N, F, f, ids, init, strategy):
    """bo_run_trial_states over 40 trials: a Byzantine node is alive and has no protocol state."""
    assert M8 == 8
    faulty, byz = first(f, N), marks(ids, N)
    for t in range(40):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, initial_values=init, mode=M8,
                                            byzantine=byz, byz_one=HALF, byz_strategy=strategy)
        _, ref_rounds, ref_st = model.byz_trial(N, F, faulty, byz, SEED, t, 16, init, byz_one=HALF, byz_strategy=strategy)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
        for i in ids:
            assert st[i] == {"killed": False, "x": None, "decided": None, "k": None}
        for i in range(f):
            assert st[i] == {"killed": True, "x": None, "decided": None, "k": None}


def test_law_on_device():
    """GPU histogram against the mask-level simulation of tests/test_byz_tally.py,
    (26, 8), b = 4, byz_one 1/2, 5 * 10^4 trials a side: two-sample chi^2 over bins
    pooled to >= 20, p > 10^-3, fixed seeds."""
    N, F, trials = 26, 8, 50000
    faulty, byz = first(0, N), marks({2, 9, 17, 25}, N)
    got = gpu_hist(N, F, faulty, byz, trials, byz_one=HALF)
    ref = model.mask_sim_hist(N, F, faulty, byz, 16, trials, np.random.default_rng(SEED + 1), byz_one=HALF)
    assert int(got[:-1].sum()) == trials == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"(N, F, b) = ({N}, {F}, 4), byz_one 1/2: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}, "
          f"agreement violations {int(got[-1])} (device) / {int(ref[-1])} (simulation)")
    assert p > 1e-3, (p, stat, df)


def test_agreement_violations_are_reachable():
    """(10, 4), b = 4, byz_one 1/2, m = 10 even: the histogram's last bin, unreachable in the
    crash modes, equals the restatement's."""
    N, F, trials = 10, 4, 3000
    byz = marks({0, 4, 5, 9}, N)
    got = gpu_hist(N, F, first(0, N), byz, trials, byz_one=HALF)
    ref = model.byz_hist(N, F, first(0, N), byz, SEED, 0, trials, 16, byz_one=HALF)
    print(f"(10, 4), b = 4, byz_one 1/2: {int(got[-1])} agreement violations in {trials} trials "
          f"(restatement: {int(ref[-1])})")
    assert int(got[-1]) == int(ref[-1])
    assert np.array_equal(got, ref)


@needs_node
def test_js_run_trials_mode_8(tmp_path):
    N, F, trials = 10, 4, 1000
    script = tmp_path / "byz.js"
    script.write_text(
        "const b = require(%s);\n"
        "if (b.MODE_BYZ_TALLY !== 8 || b.BYZ_RANDOM !== 0 || b.BYZ_OPPOSE !== 1) process.exit(2);\n"
        "const byz = new Array(%d).fill(false); byz[2] = true; byz[7] = true;\n"
        "b.runTrials({N: %d, F: %d, faultyList: new Array(%d).fill(false), seed: %dn, kMax: 16,\n"
        "             trialCount: %d, mode: b.MODE_BYZ_TALLY, byzantineList: byz, byzOne: 0x80000000,\n"
        "             byzStrategy: b.BYZ_OPPOSE})\n"
        "  .then((h) => { console.log(JSON.stringify(Array.from(h, Number))); })\n"
        "  .catch((e) => { console.error(e); process.exit(1); });\n"
        % (json.dumps(os.path.join(PKG, "js", "index.js")), N, N, F, N, SEED, trials))
    p = subprocess.run(["node", str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array(json.loads(p.stdout.strip().splitlines()[-1]), dtype=np.uint64)
    assert np.array_equal(got, gpu_hist(N, F, first(0, N), marks({2, 7}, N), trials, byz_one=HALF, byz_strategy=OPPOSE))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


@pytest.mark.parametrize("name,strategy", [("random", RANDOM), ("oppose", OPPOSE)])
def test_cli_trials_mode_byz(name, strategy):
    N, F, trials = 100, 36, 5000
    out = _cli("trials", "--N", str(N), "--F", str(F), "--trials", str(trials), "--mode", "byz", "--crashed", "2",
               "--byzantine", "12", "--byz-one", "0.5", "--byz-strategy", name, "--k-max", "16")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["mode"] == "byz" and row["crashed"] == 2 and row["m"] == N - 2 and row["trials"] == trials
    assert row["byzantine"] == 12 and row["byz_one"] == 0.5 and row["byz_one_word"] == HALF
    assert row["byz_strategy"] == name
    byz = marks(set(range(2, 14)), N)                         # the 12 live nodes after the crashed ones
    h = gpu_hist(N, F, first(2, N), byz, trials, byz_one=HALF, byz_strategy=strategy)   # the CLI's default seed is SEED
    assert row["hist"] == [int(v) for v in h]
