"""BO_MODE_RANDOM_TALLY on the device (csrc/benor_tally.hip): bit-exact against
the plain-Python restatement of its definition in tests/test_tally.py, split
invariance, equality with BO_MODE_LOCKSTEP at f = F, the law against the CPU
oracle's mask-level random delivery, and the JS and CLI surfaces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import benor
import oracle
import test_tally as model
from conftest import PKG, ROOT
from test_js_api import needs_node

pytestmark = pytest.mark.gpu

T = benor.BO_MODE_RANDOM_TALLY
SEED = model.SEED


def gpu_hist(N, F, faulty, trials, *, seed=SEED, k_max=16, begin=0, init=None):
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=T)
    assert plan.kernel == benor.BO_KERNEL_TALLY
    return plan.run(begin, trials)


def check_exact(N, F, faulty, trials, *, seed=SEED, k_max=16, begin=0, init=None, state_trials=None):
    got = gpu_hist(N, F, faulty, trials, seed=seed, k_max=k_max, begin=begin, init=init)
    ref = model.tally_hist(N, F, faulty, seed, begin, trials, k_max, init)
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in state_trials if state_trials is not None else (begin, begin + 1, begin + trials - 1):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init,
                                            mode=T)
        _, ref_rounds, ref_st = model.tally_trial(N, F, faulty, seed, t, k_max, init)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, t
    return got


@pytest.mark.parametrize("N,F,f,trials", [
    (11, 4, 0, 2000),        # multi-round
    (11, 4, 2, 2000),        # multi-round, f > 0
    (69, 24, 5, 500),        # m = 64: one full receiver group
    (70, 25, 5, 500),        # m = 65: one lane in group 2
    (130, 47, 1, 200),       # m = 129
    (300, 111, 0, 100),
    (1024, 393, 0, 20),      # multi-round, 16 receiver groups
    (4096, 1365, 0, 3),      # largest rows, LDS sizing, 64 receiver groups
])
def test_bit_exact(N, F, f, trials):
    h = check_exact(N, F, model.first(f, N), trials)
    assert int(h[:-1].sum()) == trials


def test_multi_round_shapes_take_more_than_one_round():
    """F < q <= 2F: not every trial halts in round 1 (the cases above do cover the round loop)."""
    h = gpu_hist(11, 4, model.first(0, 11), 2000)
    assert int(h[6:-1].sum()) > 0


def test_fixed_init_faulty_interleaved():
    N, F = 11, 4
    faulty = [i in (1, 4, 8) for i in range(N)]
    init = [1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0]
    check_exact(N, F, faulty, 500, init=init)
    N, F = 140, 49                                            # m = 131: three groups, faulty nodes spread out
    faulty = [i % 16 == 3 for i in range(N)]
    init = [(i * 7 // 3) & 1 for i in range(N)]
    assert sum(faulty) == 9
    check_exact(N, F, faulty, 100, init=init)


def test_fixed_all_ones_is_degenerate():
    """K = m: every row is a point, every receiver counts q ones and decides 1 in round 1."""
    N, F = 11, 4
    h = check_exact(N, F, model.first(1, N), 300, init=[1] * N)
    assert int(h[1 * 3 + 1]) == 300
    N, F = 130, 47
    h = check_exact(N, F, model.first(1, N), 50, init=[0] * N)
    assert int(h[1 * 3 + 0]) == 50


def test_k_max_one_fills_the_undecided_bins():
    h = check_exact(11, 4, model.first(0, 11), 2000, k_max=1)
    assert int(h[:3].sum()) > 0


def test_trial_begin_beyond_32_bits():
    check_exact(11, 4, model.first(2, 11), 500, begin=(1 << 32) + 12345)
    check_exact(70, 25, model.first(5, 70), 100, begin=(7 << 32) - 50)     # the launch crosses a 2^32 boundary


def test_split_invariance():
    N, F, trials, a = 100, 37, 10000, 3333
    plan = benor.TrialsPlan(N, F, model.first(0, N), seed=SEED, k_max=16, mode=T)
    whole = plan.run(0, trials)
    parts = plan.run(0, a) + plan.run(a, trials - a)
    assert np.array_equal(whole, parts)
    assert int(whole[:-1].sum()) == trials


@pytest.mark.parametrize("N,F,trials", [(11, 4, 2000), (257, 86, 500), (1024, 341, 200)])
def test_f_equal_F_is_lockstep(N, F, trials):
    """m = q: every row is a single point (c1 = K) and m is odd, so the mode
    equals BO_MODE_LOCKSTEP bit for bit for the same seed."""
    faulty = model.first(F, N)
    got = gpu_hist(N, F, faulty, trials)
    ref = benor.TrialsPlan(N, F, faulty, seed=SEED, k_max=16, mode=benor.BO_MODE_LOCKSTEP).run(0, trials)
    assert np.array_equal(got, ref)
    for t in (0, 1, trials - 1):
        a = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, mode=T)
        b = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, mode=benor.BO_MODE_LOCKSTEP)
        assert a == b, t


@pytest.mark.parametrize("N,F,trials", [(26, 9, 100000), (100, 37, 50000)])
def test_law_on_device(N, F, trials):
    """GPU tally histogram against the CPU oracle's mask-level random delivery
    (f = 0): two-sample chi^2 over bins pooled to >= 20, p > 10^-3, fixed seeds."""
    faulty = model.first(0, N)
    got = gpu_hist(N, F, faulty, trials)
    ref = oracle.run_trials(N, F, faulty, seed=SEED + 1, trial_count=trials, k_max=16,
                            mode=oracle.MODE_RANDOM_DELIVERY).hist
    assert int(got[:-1].sum()) == trials
    p, stat, df = model.chi2_two_sample(got, ref)
    print(f"(N, F) = ({N}, {F}): chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}")
    assert p > 1e-3, (p, stat, df)


def test_popc_unit_and_live_nodes():
    plan = benor.TrialsPlan(1024, 341, model.first(0, 1024), seed=SEED, k_max=16, mode=T)
    assert plan.live_nodes == 1024 and plan.popc_words_per_node_round == 4 * 32
    plan.check()                                              # no overflow or deferral state


@needs_node
def test_js_run_trials_mode_3(tmp_path):
    N, F, trials = 11, 4, 1000
    script = tmp_path / "tally.js"
    script.write_text(
        "const b = require(%s);\n"
        "b.runTrials({N: %d, F: %d, faultyList: new Array(%d).fill(false), seed: %dn, kMax: 16,\n"
        "             trialCount: %d, mode: b.MODE_RANDOM_TALLY})\n"
        "  .then((h) => { console.log(JSON.stringify(Array.from(h, Number))); })\n"
        "  .catch((e) => { console.error(e); process.exit(1); });\n"
        % (json.dumps(os.path.join(PKG, "js", "index.js")), N, F, N, SEED, trials))
    p = subprocess.run(["node", str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array(json.loads(p.stdout.strip().splitlines()[-1]), dtype=np.uint64)
    assert np.array_equal(got, gpu_hist(N, F, model.first(0, N), trials))


def test_cli_trials_mode_tally():
    N, F, trials = 100, 37, 5000
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", "trials", "--N", str(N), "--F", str(F), "--trials",
                        str(trials), "--mode", "tally", "--crashed", "0", "--k-max", "16"],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    row = json.loads(p.stdout.strip().splitlines()[-1])
    assert row["mode"] == "tally" and row["crashed"] == 0 and row["m"] == N and row["trials"] == trials
    h = gpu_hist(N, F, model.first(0, N), trials)              # the CLI's default seed is SEED
    assert row["hist"] == [int(v) for v in h]
