"""BO_MODE_CRASH_TALLY on the device (csrc/benor_tally_crash.hip): bit-exact
against the plain-Python restatement of its definition in
tests/test_crash_tally.py (histograms and per-node states), launch mechanics,
equality with BO_MODE_RANDOM_TALLY3 when no crash is reached, the law against
that file's mask-level simulation, and the JS and CLI surfaces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import test_crash_tally as model
from conftest import PKG, ROOT
from test_crash_tally import at
from test_js_api import needs_node
from test_tally import chi2_two_sample, first

pytestmark = pytest.mark.gpu

M5 = benor.BO_MODE_CRASH_TALLY
T3 = benor.BO_MODE_RANDOM_TALLY3
SEED = model.SEED
Q = "?"


def gpu_hist(N, F, faulty, trials, *, seed=SEED, k_max=16, begin=0, init=None, kernel=benor.BO_KERNEL_TALLY_CRASH,
             **sched):
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=M5, **sched)
    assert plan.kernel == kernel
    h = plan.run(begin, trials)
    plan.check()                                              # no overflow or deferral state
    return h


def check_exact(N, F, faulty, trials, *, seed=SEED, k_max=16, begin=0, init=None, **sched):
    got = gpu_hist(N, F, faulty, trials, seed=seed, k_max=k_max, begin=begin, init=init, **sched)
    ref = model.crash_hist(N, F, faulty, seed, begin, trials, k_max, init, **sched)
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init,
                                            mode=M5, **sched)
        _, ref_rounds, ref_st = model.crash_trial(N, F, faulty, seed, t, k_max, init, **sched)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
    return got


@pytest.mark.parametrize("steps", [{3: 0}, {1: 1, 4: 1}, {0: 2, 5: 3, 9: 5}, {2: 0, 3: 1, 6: 4, 7: 4}])
def test_bit_exact_explicit_small(steps):
    """(10, 4, f = 0): steps 0-5, 1-4 crashes, two at one step included."""
    h = check_exact(10, 4, first(0, 10), 2000, crash_at=at(10, steps))
    assert int(h[:-1].sum()) == 2000


def test_bit_exact_random_schedule_reaches_the_quorum():
    """(10, 4, f = 1) with 3 random crashes: f + crashes = F, so m_s reaches q."""
    check_exact(10, 4, first(1, 10), 2000, crash_count=3, crash_window=6)


@pytest.mark.parametrize("N,F,f,trials,steps", [
    (70, 24, 5, 300, {i: 1 for i in range(64, 70)}),          # compact 59..64: the one node of group 2 goes
    (70, 24, 0, 300, {i: 1 for i in range(64, 70)}),          # m0 = 70: group 2 (c = 64..69) empties
    (68, 22, 4, 300, {10 + 9 * s: s for s in range(6)}),      # m0 = 64, one crash per step: 7 tables
    (1024, 392, 0, 5, {i: 1 + i // 60 for i in range(300)}),  # 60 crashes at each of steps 1..5: rounds 1-3
    (4096, 1366, 0, 2, {**{100 * i: 1 for i in range(5)}, **{4095 - 64 * i: 2 for i in range(7)}}),   # three ~28 MiB tables
])
def test_bit_exact_explicit(N, F, f, trials, steps):
    h = check_exact(N, F, first(f, N), trials, crash_at=at(N, steps))
    assert int(h[:-1].sum()) == trials


def test_bit_exact_random_schedule_two_groups():
    check_exact(130, 46, first(1, 130), 100, crash_count=10, crash_window=8)


def test_bit_exact_random_schedule_words_in_the_row_region():
    """(400, 133): W = 7 and a row cap of 133, so a pass of stream-7 words fits the row region and
    the schedule is drawn there, in the batch launch and in the state launches (at N = 10 and 130
    above the words have a region of their own)."""
    check_exact(400, 133, first(0, 400), 300, crash_count=8, crash_window=4)


def test_fixed_init_with_question_marks():
    init = [Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1, 0]
    check_exact(12, 4, first(0, 12), 1000, init=init, crash_at=at(12, {0: 0, 6: 1}))   # a "?" holder goes at step 0
    _, st = benor.run_trial_states(12, 4, first(0, 12), seed=SEED, trial=0, k_max=16, initial_values=init, mode=M5,
                                   crash_at=at(12, {0: 0, 6: 1}))
    assert st[0] == {"killed": True, "x": Q, "decided": False, "k": 1}
    assert st[6] == {"killed": True, "x": 1, "decided": False, "k": 1}
    check_exact(10, 4, first(1, 10), 1000, init=model.t3.INIT_10, crash_count=2, crash_window=3)


def test_k_max_one():
    h = check_exact(10, 4, first(0, 10), 2000, k_max=1, crash_at=at(10, {2: 0, 7: 1, 8: 2}))   # step 2 is never reached
    assert int(h[:3].sum()) > 0


def test_trial_begin_beyond_32_bits():
    check_exact(10, 4, first(1, 10), 500, begin=(1 << 32) + 12345, crash_count=3, crash_window=6)
    check_exact(70, 24, first(5, 70), 100, begin=(7 << 32) - 50, crash_count=6, crash_window=4)   # across 2^32


def test_split_invariance():
    N, F, trials, a = 100, 36, 10000, 3333
    plan = benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=16, mode=M5, crash_count=12, crash_window=5)
    assert plan.kernel == benor.BO_KERNEL_TALLY_CRASH
    whole = plan.run(0, trials)
    parts = plan.run(0, a) + plan.run(a, trials - a)
    assert np.array_equal(whole, parts)
    assert int(whole[:-1].sum()) == trials


@pytest.mark.parametrize("N,F,trials", [(10, 4, 2000), (100, 36, 2000), (1024, 340, 100)])
def test_unreached_schedule_equals_mode_4_on_the_crash_kernel(N, F, trials):
    faulty, k_max = first(0, N), 16
    sched = at(N, {0: 2 * k_max, N - 1: 2 * k_max + 5})
    got = gpu_hist(N, F, faulty, trials, crash_at=sched)
    ref = benor.TrialsPlan(N, F, faulty, seed=SEED, k_max=k_max, mode=T3).run(0, trials)
    assert np.array_equal(got, ref)
    for t in (0, 1, trials - 1):
        a = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=k_max, mode=M5, crash_at=sched)
        b = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=k_max, mode=T3)
        assert a == b, t


def test_empty_schedule_is_mode_4():
    for N, F, kernel in ((10, 4, benor.BO_KERNEL_TALLY3), (11, 4, benor.BO_KERNEL_TALLY)):
        got = gpu_hist(N, F, first(0, N), 2000, kernel=kernel)
        assert np.array_equal(got, benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=16, mode=T3).run(0, 2000))
        got = gpu_hist(N, F, first(0, N), 2000, kernel=kernel, crash_at=at(N, {}))
        assert np.array_equal(got, benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=16, mode=T3).run(0, 2000))


def test_at_the_quorum_from_step_0_the_run_is_lockstep():
    """f + crashes = F, all at step 0: m_s = q throughout, no draw is made."""
    check_exact(10, 4, first(1, 10), 1000, crash_at=at(10, {3: 0, 5: 0, 8: 0}))
    check_exact(140, 48, first(8, 140), 50, crash_at=at(140, {8 + 3 * i: 0 for i in range(40)}))
    # the crashed nodes last: the survivors keep mode 4's compact indices, so its histogram at f = F
    init = [1, 0, 1, 0, 0, 1, Q, 0, 1, 1]
    got = gpu_hist(10, 4, first(1, 10), 1000, init=init, crash_at=at(10, {7: 0, 8: 0, 9: 0}))
    ref = benor.TrialsPlan(10, 4, [i in (0, 7, 8, 9) for i in range(10)], seed=SEED, k_max=16, initial_values=init,
                           mode=T3).run(0, 1000)
    assert np.array_equal(got, ref)


def test_popc_unit():
    N, F, f = 1024, 340, 3
    plan = benor.TrialsPlan(N, F, first(f, N), seed=SEED, k_max=16, mode=M5, crash_count=16, crash_window=4)
    assert plan.kernel == benor.BO_KERNEL_TALLY_CRASH
    assert plan.live_nodes == N - f and plan.popc_words_per_node_round == 4 * -(-(N - f) // 32)
    plan.run(0, 8)
    plan.check()


def test_law_on_device():
    """GPU histogram against the mask-level simulation of tests/test_crash_tally.py,
    (26, 8), 4 random crashes in window 4, 5 * 10^4 trials a side: two-sample
    chi^2 over bins pooled to >= 20, p > 10^-3, fixed seeds."""
    N, F, trials = 26, 8, 50000
    faulty = first(0, N)
    got = gpu_hist(N, F, faulty, trials, crash_count=4, crash_window=4)
    ref = model.mask_sim_hist(N, F, faulty, 16, trials, np.random.default_rng(SEED + 1), crash_count=4, crash_window=4)
    assert int(got[:-1].sum()) == trials == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"(N, F) = ({N}, {F}), 4 crashes in 4 steps: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}, "
          f"agreement violations {int(got[-1])} (device) / {int(ref[-1])} (simulation)")
    assert p > 1e-3, (p, stat, df)


@needs_node
def test_js_run_trials_mode_5(tmp_path):
    N, F, trials = 10, 4, 1000
    script = tmp_path / "crash.js"
    script.write_text(
        "const b = require(%s);\n"
        "b.runTrials({N: %d, F: %d, faultyList: new Array(%d).fill(false), seed: %dn, kMax: 16,\n"
        "             trialCount: %d, mode: b.MODE_CRASH_TALLY, crashCount: 3, crashWindow: 6})\n"
        "  .then((h) => { console.log(JSON.stringify(Array.from(h, Number))); })\n"
        "  .catch((e) => { console.error(e); process.exit(1); });\n"
        % (json.dumps(os.path.join(PKG, "js", "index.js")), N, F, N, SEED, trials))
    p = subprocess.run(["node", str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array(json.loads(p.stdout.strip().splitlines()[-1]), dtype=np.uint64)
    assert np.array_equal(got, gpu_hist(N, F, first(0, N), trials, crash_count=3, crash_window=6))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_cli_trials_mode_crash():
    N, F, trials = 100, 36, 5000
    out = _cli("trials", "--N", str(N), "--F", str(F), "--trials", str(trials), "--mode", "crash", "--crashed", "2",
               "--crash-count", "12", "--crash-window", "5", "--k-max", "16")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["mode"] == "crash" and row["crashed"] == 2 and row["m"] == N - 2 and row["trials"] == trials
    assert row["crash_count"] == 12 and row["crash_window"] == 5 and row["crash_at"] is None
    h = gpu_hist(N, F, first(2, N), trials, crash_count=12, crash_window=5)    # the CLI's default seed is SEED
    assert row["hist"] == [int(v) for v in h]
    out = _cli("trials", "--N", "10", "--F", "4", "--trials", "1000", "--mode", "crash", "--crashed", "1",
               "--crash-at", "3:0,7:1")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["crash_at"] == "3:0,7:1"
    assert row["hist"] == [int(v) for v in gpu_hist(10, 4, first(1, 10), 1000, crash_at=at(10, {3: 0, 7: 1}))]
