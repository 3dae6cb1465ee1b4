"""BO_MODE_RANDOM_TALLY3 on the device (csrc/benor_tally3.hip): bit-exact against
the plain-Python restatement of its definition in tests/test_tally3.py, launch
mechanics, equality with BO_MODE_RANDOM_TALLY inside that mode's scope and with
BO_MODE_LOCKSTEP at f = F, the law against the CPU oracle's mask-level random
delivery, and the JS and CLI surfaces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: run_sweep runs in this process, on one HIP runtime)

import benor
import oracle
import test_tally3 as model
from conftest import PKG, ROOT
from test_js_api import needs_node
from test_tally import chi2_two_sample, first

pytestmark = pytest.mark.gpu

T3 = benor.BO_MODE_RANDOM_TALLY3
SEED = model.SEED
Q = "?"


def expected_kernel(N, F, faulty, init=None):
    """Mode 3's kernel inside mode 3's scope (odd quorum, no live "?"), else the three-valued one."""
    live_q = init is not None and any(v == Q and not dead for v, dead in zip(init, faulty))
    return benor.BO_KERNEL_TALLY if (N - F) % 2 and not live_q else benor.BO_KERNEL_TALLY3


def gpu_hist(N, F, faulty, trials, *, seed=SEED, k_max=16, begin=0, init=None):
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=T3)
    assert plan.kernel == expected_kernel(N, F, faulty, init)
    return plan.run(begin, trials)


def check_exact(N, F, faulty, trials, *, seed=SEED, k_max=16, begin=0, init=None):
    got = gpu_hist(N, F, faulty, trials, seed=seed, k_max=k_max, begin=begin, init=init)
    ref = model.tally3_hist(N, F, faulty, seed, begin, trials, k_max, init)
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init,
                                            mode=T3)
        _, ref_rounds, ref_st = model.tally3_trial(N, F, faulty, seed, t, k_max, init)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, t
    return got


@pytest.mark.parametrize("N,F,f,trials", [
    (10, 4, 0, 2000),
    (10, 4, 2, 2000),
    (10, 5, 0, 1000),        # q = F: never decides, fills the undecided bins (q odd: mode 3's kernel)
    (68, 22, 4, 300),        # m = 64: one full receiver group
    (70, 24, 5, 300),        # m = 65: one lane in group 2
    (130, 46, 1, 100),
    (300, 110, 0, 50),
    (1024, 392, 0, 5),       # multi-round, 16 receiver groups
    (4096, 1366, 0, 2),      # largest rows, LDS sizing, 64 receiver groups
])
def test_bit_exact(N, F, f, trials):
    h = check_exact(N, F, first(f, N), trials)
    assert int(h[:-1].sum()) == trials
    if (N, F) == (10, 5):
        assert int(h[:3].sum()) == trials                     # the undecided bins, all of them


def test_fixed_init_with_question_marks():
    check_exact(10, 4, first(1, 10), 1000, init=model.INIT_10)
    # odd quorum: outside mode 3's scope only because of the "?"
    check_exact(11, 4, first(0, 11), 1000, init=[1, 0, Q, 1, 1, 0, Q, 0, 0, 1, 0])
    N, F = 140, 48                                            # a third of the votes "?": the longest walks
    faulty = [i % 16 == 3 for i in range(N)]
    assert sum(faulty) == 9
    check_exact(N, F, faulty, 50, init=[(0, 1, Q)[i % 3] for i in range(N)])


def test_fixed_all_question_marks_everyone_flips():
    """Every round-1 tally is empty: every proposal is "?", every x of round 1 a coin."""
    N, F = 10, 4
    check_exact(N, F, first(0, N), 500, init=[Q] * N)
    _, st = benor.run_trial_states(N, F, first(0, N), seed=SEED, trial=3, k_max=1, initial_values=[Q] * N, mode=T3)
    assert [s["x"] for s in st] == [oracle.coin(SEED, 3, c, 1) for c in range(N)]
    assert not any(s["decided"] for s in st)


def test_fixed_all_ones_is_degenerate():
    N, F = 130, 46
    h = check_exact(N, F, first(1, N), 50, init=[1] * N)
    assert int(h[1 * 3 + 1]) == 50


def test_k_max_one_fills_the_undecided_bins():
    h = check_exact(10, 4, first(0, 10), 2000, k_max=1)
    assert int(h[:3].sum()) > 0


def test_trial_begin_beyond_32_bits():
    check_exact(10, 4, first(2, 10), 500, begin=(1 << 32) + 12345)
    check_exact(70, 24, first(5, 70), 100, begin=(7 << 32) - 50)     # the launch crosses a 2^32 boundary


def test_split_invariance():
    N, F, trials, a = 100, 36, 10000, 3333
    plan = benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=16, mode=T3)
    assert plan.kernel == benor.BO_KERNEL_TALLY3
    whole = plan.run(0, trials)
    parts = plan.run(0, a) + plan.run(a, trials - a)
    assert np.array_equal(whole, parts)
    assert int(whole[:-1].sum()) == trials


@pytest.mark.parametrize("N,F,trials", [(11, 4, 2000), (257, 86, 500), (1024, 341, 200)])
def test_equals_mode_3_in_its_scope(N, F, trials):
    faulty = first(0, N)
    assert expected_kernel(N, F, faulty) == benor.BO_KERNEL_TALLY
    got = gpu_hist(N, F, faulty, trials)
    ref = benor.TrialsPlan(N, F, faulty, seed=SEED, k_max=16, mode=benor.BO_MODE_RANDOM_TALLY).run(0, trials)
    assert np.array_equal(got, ref)
    for t in (0, 1, trials - 1):
        a = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, mode=T3)
        b = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, mode=benor.BO_MODE_RANDOM_TALLY)
        assert a == b, t


@pytest.mark.parametrize("N,F,trials,init", [
    (10, 4, 2000, None),                                       # m = 6
    (10, 5, 500, [0, 0, 0, 0, 0, 1, Q, 0, 1, Q]),
    (256, 86, 500, None),                                      # m = 170
    (1024, 342, 200, None),                                    # m = 682
])
def test_f_equal_F_is_lockstep(N, F, trials, init):
    """m = q: every row is a point and every member of S is in the inbox, so the
    mode equals BO_MODE_LOCKSTEP bit for bit for the same seed, even m and "?" included."""
    faulty = first(F, N)
    assert expected_kernel(N, F, faulty, init) == benor.BO_KERNEL_TALLY3
    got = gpu_hist(N, F, faulty, trials, init=init)
    ref = benor.TrialsPlan(N, F, faulty, seed=SEED, k_max=16, initial_values=init,
                           mode=benor.BO_MODE_LOCKSTEP).run(0, trials)
    assert np.array_equal(got, ref)
    for t in (0, 1, trials - 1):
        a = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, initial_values=init, mode=T3)
        b = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=16, initial_values=init,
                                   mode=benor.BO_MODE_LOCKSTEP)
        assert a == b, t


@pytest.mark.parametrize("N,F,trials", [(26, 8, 100000), (100, 36, 50000)])
def test_law_on_device(N, F, trials):
    """GPU histogram against the CPU oracle's mask-level random delivery (f = 0):
    two-sample chi^2 over bins pooled to >= 20, p > 10^-3, fixed seeds."""
    faulty = first(0, N)
    assert expected_kernel(N, F, faulty) == benor.BO_KERNEL_TALLY3
    got = gpu_hist(N, F, faulty, trials)
    ref = oracle.run_trials(N, F, faulty, seed=SEED + 1, trial_count=trials, k_max=16,
                            mode=oracle.MODE_RANDOM_DELIVERY).hist
    assert int(got[:-1].sum()) == trials
    p, stat, df = chi2_two_sample(got, ref)
    print(f"(N, F) = ({N}, {F}): chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}, "
          f"agreement violations {int(got[-1])} (device) / {int(ref[-1])} (oracle)")
    assert p > 1e-3, (p, stat, df)
    if (N, F) == (26, 8):                                     # q = 18 = 2 (F + 1): two receivers can decide apart
        assert int(got[-1]) > 0 and int(ref[-1]) > 0


def test_popc_unit_and_check():
    N, F, f = 1024, 340, 3
    plan = benor.TrialsPlan(N, F, first(f, N), seed=SEED, k_max=16, mode=T3)
    assert plan.kernel == benor.BO_KERNEL_TALLY3
    assert plan.live_nodes == N - f and plan.popc_words_per_node_round == 4 * -(-(N - f) // 32)
    plan.run(0, 8)
    plan.check()                                              # no overflow or deferral state


@needs_node
def test_js_run_trials_mode_4(tmp_path):
    N, F, trials = 10, 4, 1000
    script = tmp_path / "tally3.js"
    script.write_text(
        "const b = require(%s);\n"
        "b.runTrials({N: %d, F: %d, faultyList: new Array(%d).fill(false), seed: %dn, kMax: 16,\n"
        "             trialCount: %d, mode: b.MODE_RANDOM_TALLY3})\n"
        "  .then((h) => { console.log(JSON.stringify(Array.from(h, Number))); })\n"
        "  .catch((e) => { console.error(e); process.exit(1); });\n"
        % (json.dumps(os.path.join(PKG, "js", "index.js")), N, F, N, SEED, trials))
    p = subprocess.run(["node", str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array(json.loads(p.stdout.strip().splitlines()[-1]), dtype=np.uint64)
    assert np.array_equal(got, gpu_hist(N, F, first(0, N), trials))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_cli_trials_mode_tally3():
    N, F, trials = 100, 36, 5000
    out = _cli("trials", "--N", str(N), "--F", str(F), "--trials", str(trials), "--mode", "tally3", "--crashed", "0",
               "--k-max", "16")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["mode"] == "tally3" and row["crashed"] == 0 and row["m"] == N and row["trials"] == trials
    h = gpu_hist(N, F, first(0, N), trials)                    # the CLI's default seed is SEED
    assert row["hist"] == [int(v) for v in h]


def test_cli_sweep_mode_tally3_and_default():
    from benor import cli

    cells, per_cell, k_max = [(10, 4), (11, 4), (64, 21), (64, 22)], 20000, 32
    spec = ",".join(f"{N}:{F}" for N, F in cells)
    out = _cli("sweep", "--mode", "tally3", "--crashed", "0", "--cells", spec, "--per-cell", str(per_cell))
    rows = []
    for N, F in cells:                                        # the sweep's seed rule, its default seed and k_max
        plan = benor.TrialsPlan(N, F, first(0, N), seed=SEED ^ (N << 20) ^ F, k_max=k_max, mode=T3)
        assert plan.kernel == (benor.BO_KERNEL_TALLY if (N - F) % 2 else benor.BO_KERNEL_TALLY3)
        rows.append(cli.summarize(plan.run(0, per_cell), N, F, k_max, 0))
    assert all(r["m"] == r["N"] and r["trials"] == per_cell for r in rows)
    assert out == cli.rows_csv(rows)
    # the default sweep is what it was: lockstep, F crashed per cell
    out = _cli("sweep", "--cells", spec, "--per-cell", str(per_cell))
    assert out == cli.rows_csv(cli.run_sweep(cells, per_cell, SEED, k_max)[0])
    with pytest.raises(ValueError):
        cli.run_sweep(cells, per_cell, SEED, k_max, mode="tally3", crashed=5)
