"""BO_MODE_CRASH_SUBSET on the device (csrc/benor_tally_subset.hip): bit-exact
against the plain-Python restatement of its definition in
tests/test_crash_subset.py (histograms and per-node states), launch mechanics,
equality with BO_MODE_CRASH_TALLY at reach 0 and with BO_MODE_CRASH_PARTIAL's full
cut at reach UINT32_MAX, the law against that file's mask-level simulation, and
the JS and CLI surfaces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import test_crash_subset as model
from conftest import PKG, ROOT
from test_crash_tally import at, schedule
from test_js_api import needs_node
from test_tally import chi2_two_sample, first

pytestmark = pytest.mark.gpu

M5 = benor.BO_MODE_CRASH_TALLY
M6 = benor.BO_MODE_CRASH_PARTIAL
M7 = getattr(benor, "BO_MODE_CRASH_SUBSET", None)           # absent before the mode: every test fails
SUBSET = getattr(benor, "BO_KERNEL_TALLY_SUBSET", None)
ALL, HALF, QUARTER = model.ALL, model.HALF, model.QUARTER
SEED = model.SEED
Q = "?"


def gpu_hist(N, F, faulty, trials, *, seed=SEED, k_max=16, begin=0, init=None, mode=None, kernel=None, **sched):
    mode = M7 if mode is None else mode
    assert M7 == 7
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=mode, **sched)
    assert plan.kernel == (SUBSET if kernel is None else kernel)
    h = plan.run(begin, trials)
    plan.check()                                              # no overflow or deferral state
    return h


def check_exact(N, F, faulty, trials, *, seed=SEED, k_max=16, begin=0, init=None, **sched):
    got = gpu_hist(N, F, faulty, trials, seed=seed, k_max=k_max, begin=begin, init=init, **sched)
    ref = model.subset_hist(N, F, faulty, seed, begin, trials, k_max, init, **sched)
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init,
                                            mode=M7, **sched)
        _, ref_rounds, ref_st = model.subset_trial(N, F, faulty, seed, t, k_max, init, **sched)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
    return got


@pytest.mark.parametrize("reach", [0, HALF, ALL])
def test_bit_exact_one_crash(reach):
    """(10, 4, f = 0), node 3 at step 0: nobody, about half, everybody hear its x."""
    h = check_exact(10, 4, first(0, 10), 2000, crash_at=at(10, {3: 0}), crash_reach=reach)
    assert int(h[:-1].sum()) == 2000


@pytest.mark.parametrize("steps", [{1: 1, 4: 1}, {0: 0, 5: 5, 9: 9}])
def test_bit_exact_explicit(steps):
    """(10, 4, f = 0): two crashers at one P-step (their proposals vote in some pools); crashes at steps 0, 5, 9."""
    h = check_exact(10, 4, first(0, 10), 2000, crash_at=at(10, steps), crash_reach=HALF)
    assert int(h[:-1].sum()) == 2000


def test_k_max_one():
    h = check_exact(10, 4, first(0, 10), 2000, k_max=1, crash_at=at(10, {2: 0, 7: 1, 8: 2}), crash_reach=HALF)
    assert int(h[:3].sum()) > 0                               # step 2 is never reached


def test_bit_exact_random_schedule_reaches_the_quorum():
    """(10, 4, f = 1) with 3 random crashes: f + crashes = F, so m_s reaches q while a
    receiver that hears j crashers still draws from the table of q + j."""
    check_exact(10, 4, first(1, 10), 2000, crash_count=3, crash_window=6, crash_reach=HALF)


def test_fixed_init_with_question_marks():
    init = [Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1, 0]
    sched = dict(crash_at=at(12, {0: 0, 6: 1}), crash_reach=HALF)     # a "?" reaches some receivers at step 0
    check_exact(12, 4, first(0, 12), 1000, init=init, **sched)
    _, st = benor.run_trial_states(12, 4, first(0, 12), seed=SEED, trial=0, k_max=16, initial_values=init, mode=M7,
                                   **sched)
    assert st[0] == {"killed": True, "x": Q, "decided": False, "k": 1}
    assert st[6] == {"killed": True, "x": 1, "decided": False, "k": 1}


@pytest.mark.parametrize("reach", [HALF, QUARTER])
def test_bit_exact_one_lane_group(reach):
    """(70, 24, f = 5), m0 = 65: group 1 is compact index 64 alone, a group of one lane that
    hears a crasher or not; with four crashers at steps 0..2 group 0's lanes fall into
    several profiles, some drawing from the staged row and some from rows of their own."""
    steps = {7: 0, 20: 1, 33: 1, 50: 2}
    check_exact(70, 24, first(5, 70), 300, crash_at=at(70, steps), crash_reach=reach)


def test_bit_exact_random_schedule_three_groups():
    check_exact(130, 46, first(1, 130), 100, crash_count=10, crash_window=8, crash_reach=HALF)


def test_bit_exact_more_than_64_crashers_at_one_step():
    """(200, 70, f = 0): 70 crashers at step 1, spread over the four groups: the reach pass
    walks a list longer than one 64-entry chunk, and a group's lanes nearly all differ."""
    steps = {(17 * i) % 200: 1 for i in range(70)}
    assert len(steps) == 70
    check_exact(200, 70, first(0, 200), 50, crash_at=at(200, steps), crash_reach=HALF)


def test_bit_exact_large_network():
    check_exact(1024, 340, first(0, 1024), 30, crash_count=16, crash_window=4, crash_reach=HALF)


def test_trial_begin_beyond_32_bits():
    check_exact(10, 4, first(1, 10), 500, begin=(1 << 32) + 12345, crash_count=3, crash_window=6, crash_reach=HALF)
    check_exact(70, 24, first(5, 70), 100, begin=(7 << 32) - 50, crash_count=6, crash_window=4, crash_reach=HALF)


def test_split_invariance():
    N, F, trials, a = 100, 36, 10000, 3333
    assert M7 == 7
    plan = benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=16, mode=M7, crash_count=12, crash_window=5,
                            crash_reach=HALF)
    assert plan.kernel == SUBSET
    whole = plan.run(0, trials)
    parts = plan.run(0, a) + plan.run(a, trials - a)
    assert np.array_equal(whole, parts)
    assert int(whole[:-1].sum()) == trials


@pytest.mark.parametrize("reach", [HALF, QUARTER])
@pytest.mark.parametrize("N,F,f,init,sched", [
    (10, 4, 0, [Q, 1, 0, Q, 1, 1, 0, 0, 1, 0], dict(crash_at=at(10, {0: 0, 3: 1, 7: 2}))),
    (10, 4, 1, None, dict(crash_count=3, crash_window=6)),
    (130, 46, 1, None, dict(crash_count=10, crash_window=8)),
    (130, 46, 0, [Q if i % 9 == 0 else i % 2 for i in range(130)],
     dict(crash_at=at(130, {0: 0, 9: 1, 64: 1, 100: 2, 129: 3}))),
])
def test_per_node_states(N, F, f, init, sched, reach):
    """bo_run_trial_states over 40 trials; nodes 0 (and 3 / 9) hold "?" when they crash in round 1."""
    assert M7 == 7
    faulty = first(f, N)
    for t in range(40):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, initial_values=init, mode=M7,
                                            crash_reach=reach, **sched)
        _, ref_rounds, ref_st = model.subset_trial(N, F, faulty, SEED, t, 16, init, crash_reach=reach, **sched)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
        if init is not None:
            assert st[0] == {"killed": True, "x": Q, "decided": False, "k": 1}


def test_a_random_schedule_given_explicitly_is_the_same_trial():
    """The device draws a random schedule in Floyd's order and reads an explicit one sorted by
    step: the reach pattern does not depend on the order of the list."""
    assert M7 == 7
    N, F, f = 130, 46, 1
    faulty = first(f, N)
    live = [i for i in range(N) if not faulty[i]]
    for t in range(10):
        sched = schedule(SEED, t, live, None, 10, 4)
        explicit = at(N, {live[c]: s for c, s in enumerate(sched) if s is not None})
        a = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, mode=M7, crash_count=10, crash_window=4,
                                   crash_reach=HALF)
        b = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, mode=M7, crash_at=explicit,
                                   crash_reach=HALF)
        assert a == b, t


@pytest.mark.parametrize("N,F,trials", [(10, 4, 2000), (100, 36, 2000), (1024, 340, 100)])
def test_reach_0_equals_mode_5_on_the_subset_kernel(N, F, trials):
    faulty, k_max = first(0, N), 16
    sched = dict(crash_count=min(F, 12), crash_window=5)
    got = gpu_hist(N, F, faulty, trials, crash_reach=0, **sched)
    ref = gpu_hist(N, F, faulty, trials, mode=M5, kernel=benor.BO_KERNEL_TALLY_CRASH, **sched)
    assert np.array_equal(got, ref)
    for t in (0, 1, trials - 1):
        a = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=k_max, mode=M7, crash_reach=0, **sched)
        b = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=k_max, mode=M5, **sched)
        assert a == b, t


@pytest.mark.parametrize("N,F,trials", [(10, 4, 2000), (100, 36, 2000), (1024, 340, 100)])
def test_reach_all_equals_mode_6_with_a_full_cut(N, F, trials):
    faulty, k_max = first(0, N), 16
    n = min(F, 12)
    explicit = dict(crash_at=at(N, {(7 * i) % N: i % 5 for i in range(n)}))
    for sched in (explicit, dict(crash_count=n, crash_window=5)):
        got = gpu_hist(N, F, faulty, trials, crash_reach=ALL, **sched)
        ref = gpu_hist(N, F, faulty, trials, mode=M6, kernel=benor.BO_KERNEL_TALLY_PARTIAL, crash_cut=N, **sched)
        assert np.array_equal(got, ref)
        for t in (0, 1, trials - 1):
            a = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=k_max, mode=M7, crash_reach=ALL, **sched)
            b = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=k_max, mode=M6, crash_cut=N, **sched)
            assert a == b, t


def test_empty_schedule_is_mode_4():
    T3 = benor.BO_MODE_RANDOM_TALLY3
    for N, F, kernel in ((10, 4, benor.BO_KERNEL_TALLY3), (11, 4, benor.BO_KERNEL_TALLY)):
        ref = benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=16, mode=T3).run(0, 2000)
        assert np.array_equal(gpu_hist(N, F, first(0, N), 2000, kernel=kernel, crash_reach=HALF), ref)
        assert np.array_equal(gpu_hist(N, F, first(0, N), 2000, kernel=kernel, crash_at=at(N, {}), crash_reach=ALL), ref)


def test_law_on_device():
    """GPU histogram against the mask-level simulation of tests/test_crash_subset.py,
    (26, 8), 4 random crashes in window 4, reach 1/2, 5 * 10^4 trials a side:
    two-sample chi^2 over bins pooled to >= 20, p > 10^-3, fixed seeds."""
    N, F, trials = 26, 8, 50000
    faulty = first(0, N)
    sched = dict(crash_count=4, crash_window=4, crash_reach=HALF)
    got = gpu_hist(N, F, faulty, trials, **sched)
    ref = model.mask_sim_hist(N, F, faulty, 16, trials, np.random.default_rng(SEED + 1), **sched)
    assert int(got[:-1].sum()) == trials == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"(N, F) = ({N}, {F}), 4 crashes in 4 steps, reach 1/2: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}, "
          f"agreement violations {int(got[-1])} (device) / {int(ref[-1])} (simulation)")
    assert p > 1e-3, (p, stat, df)


@needs_node
def test_js_run_trials_mode_7(tmp_path):
    N, F, trials = 10, 4, 1000
    script = tmp_path / "subset.js"
    script.write_text(
        "const b = require(%s);\n"
        "if (b.MODE_CRASH_SUBSET !== 7 || b.REACH_ALL !== 0xFFFFFFFF) process.exit(2);\n"
        "b.runTrials({N: %d, F: %d, faultyList: new Array(%d).fill(false), seed: %dn, kMax: 16,\n"
        "             trialCount: %d, mode: b.MODE_CRASH_SUBSET, crashCount: 3, crashWindow: 6, crashReach: 0x80000000})\n"
        "  .then((h) => { console.log(JSON.stringify(Array.from(h, Number))); })\n"
        "  .catch((e) => { console.error(e); process.exit(1); });\n"
        % (json.dumps(os.path.join(PKG, "js", "index.js")), N, F, N, SEED, trials))
    p = subprocess.run(["node", str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array(json.loads(p.stdout.strip().splitlines()[-1]), dtype=np.uint64)
    assert np.array_equal(got, gpu_hist(N, F, first(0, N), trials, crash_count=3, crash_window=6, crash_reach=HALF))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_cli_trials_mode_subset():
    N, F, trials = 100, 36, 5000
    out = _cli("trials", "--N", str(N), "--F", str(F), "--trials", str(trials), "--mode", "subset", "--crashed", "2",
               "--crash-count", "12", "--crash-window", "5", "--crash-reach", "0.5", "--k-max", "16")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["mode"] == "subset" and row["crashed"] == 2 and row["m"] == N - 2 and row["trials"] == trials
    assert row["crash_count"] == 12 and row["crash_window"] == 5
    assert row["crash_reach"] == 0.5 and row["crash_reach_word"] == HALF
    h = gpu_hist(N, F, first(2, N), trials, crash_count=12, crash_window=5, crash_reach=HALF)   # the CLI's default seed is SEED
    assert row["hist"] == [int(v) for v in h]
    out = _cli("trials", "--N", "10", "--F", "4", "--trials", "1000", "--mode", "subset", "--crashed", "1",
               "--crash-at", "3:0,7:1", "--crash-reach", "1.0")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["crash_at"] == "3:0,7:1" and row["crash_reach_word"] == ALL
    assert row["hist"] == [int(v) for v in gpu_hist(10, 4, first(1, 10), 1000, crash_at=at(10, {3: 0, 7: 1}),
                                                    crash_reach=ALL)]
