"""BO_MODE_SCHED_TALLY and BO_MODE_SCHED_RULE_B on the device (csrc/benor_tally_sched.hip, variants 18 to 21):
bit-exact against the plain-Python restatement in tests/test_byz_sched.py (histograms and per-node states), launch
mechanics, the degenerate case f = F, b = 0 against the random-delivery kernels device against device, the plan
without a table, and the JS and CLI surfaces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import oracle
import test_byz_sched as model
from conftest import PKG, ROOT
from test_js_api import needs_node
from test_tally import first

pytestmark = pytest.mark.gpu

M12, M13 = model.M12, model.M13                              # None before the modes: every test fails
BALANCE, SPLIT = model.BALANCE, model.SPLIT
STRATEGIES = model.STRATEGIES
ALL, HALF = model.ALL, model.HALF
SEED = model.SEED
marks = model.marks
Q = "?"
both_strategies = model.both_strategies
both_modes = model.both_modes
every_coin = pytest.mark.parametrize("coin", [0, HALF, ALL])


def gpu_hist(rule, N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, coin_common=0, **kw):
    model.modes_exist()
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=model.mode_of(rule),
                            byzantine=byz, coin_common=coin_common, **kw)
    assert plan.kernel == model.kernel_of(rule, coin_common)
    h = plan.run(begin, trials)
    plan.check()                                              # no overflow or deferral state
    return h


def check_exact(rule, N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, coin_common=0, states=True, **kw):
    """The launch's histogram, and the per-node states of its first two and last trials, against the restatement
    (each trial restated once)."""
    got = gpu_hist(rule, N, F, faulty, byz, trials, seed=seed, k_max=k_max, begin=begin, init=init,
                   coin_common=coin_common, **kw)
    ref = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    restated = {}
    for t in range(begin, begin + trials):
        restated[t] = model.sched_trial(rule, N, F, faulty, byz, seed, t, k_max, init, coin_common=coin_common, **kw)
        for b in restated[t][0]:
            ref[b] += 1
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}) if states else ():
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init,
                                            mode=model.mode_of(rule), byzantine=byz, coin_common=coin_common, **kw)
        _, ref_rounds, ref_st = restated[t]
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
    return got


@both_modes
@both_strategies
@every_coin
def test_bit_exact_small(coin, name, rule):
    """(10, 4, b = 0), an even quorum, and (11, 2) with one and two liars, an odd one: 400 trials each."""
    s = STRATEGIES[name]
    h = check_exact(rule, 10, 4, first(0, 10), marks(set(), 10), 400, byz_strategy=s, coin_common=coin)
    assert int(h[:-1].sum()) == 400
    for ids in ({3}, {3, 8}):
        h = check_exact(rule, 11, 2, first(0, 11), marks(ids, 11), 400, byz_strategy=s, coin_common=coin)
        assert int(h[:-1].sum()) == 400
        if rule == "b":
            assert model.mode9.forbidden_bins(h) == 0


@both_modes
@both_strategies
def test_k_max_one(name, rule):
    h = check_exact(rule, 11, 2, first(0, 11), marks({2, 7}, 11), 400, k_max=1, byz_strategy=STRATEGIES[name])
    assert int(h[:-1].sum()) == 400
    check_exact(rule, 10, 4, first(1, 10), marks({5}, 10), 400, k_max=1, byz_strategy=STRATEGIES[name], coin_common=ALL)


@both_modes
@both_strategies
@pytest.mark.parametrize("ids", [{4}, {0, 4}])
def test_fixed_init_with_question_marks(name, ids, rule):
    """(12, 2) with "?" starts: three-valued class sizes in round 1's R-phase."""
    init = [Q, 1, 0, 1, Q, 1, 1, 0, 1, Q, 1, 1]               # nodes 0 and 4 may be liars: no initial value of the run
    check_exact(rule, 12, 2, first(0, 12), marks(ids, 12), 200, init=init, byz_strategy=STRATEGIES[name], coin_common=HALF)
    init = [Q, 1, 0, 0, Q, 1, 0, 0, 1, Q, 1, 0]               # balanced: coins are taken
    check_exact(rule, 12, 2, first(0, 12), marks(ids, 12), 200, init=init, byz_strategy=STRATEGIES[name])
    init = [Q] * 9 + [1, 0, Q]                                # Hq >= q: an inbox of "?" alone
    check_exact(rule, 12, 2, first(0, 12), marks(ids, 12), 100, init=init, byz_strategy=STRATEGIES[name])


@both_modes
@both_strategies
def test_bit_exact_64_12(name, rule):
    """(64, 12), b = 12 = F: one full lane group."""
    ids = {(5 * i) % 64 for i in range(12)}
    check_exact(rule, 64, 12, first(0, 64), marks(ids, 64), 60, k_max=32, byz_strategy=STRATEGIES[name])
    check_exact(rule, 64, 12, first(0, 64), marks(ids, 64), 60, k_max=8, byz_strategy=STRATEGIES[name], coin_common=HALF)


@both_modes
@both_strategies
def test_group_edges(name, rule):
    """(65, 12) and (130, 46) with liars {0, 63, 64}: the last group holds one node, a liar, and two nodes."""
    check_exact(rule, 65, 12, first(0, 65), marks({0, 63, 64}, 65), 60, byz_strategy=STRATEGIES[name], coin_common=HALF)
    check_exact(rule, 130, 46, first(0, 130), marks({0, 63, 64}, 130), 40, byz_strategy=STRATEGIES[name])
    check_exact(rule, 130, 46, first(3, 130), marks({63, 64, 66}, 130), 40, byz_strategy=STRATEGIES[name], coin_common=ALL)


@both_modes
@both_strategies
def test_a_group_without_an_honest_lane(name, rule):
    """(200, 70) with liars 64 .. 127: group 1 has no receiver."""
    check_exact(rule, 200, 70, first(0, 200), marks(set(range(64, 128)), 200), 30, byz_strategy=STRATEGIES[name])
    check_exact(rule, 200, 70, first(0, 200), marks(set(range(64, 128)), 200), 30, byz_strategy=STRATEGIES[name],
                coin_common=HALF)


@both_modes
@both_strategies
def test_bit_exact_large_network(name, rule):
    """(1024, 204), b = 16, sixteen groups, random starts, 60 trials."""
    ids = {(41 * i) % 1024 for i in range(16)}
    assert len(ids) == 16
    check_exact(rule, 1024, 204, first(0, 1024), marks(ids, 1024), 60, k_max=8, byz_strategy=STRATEGIES[name],
                coin_common=ALL if rule == "b" else 0)


@both_modes
@both_strategies
def test_bit_exact_largest_network(name, rule):
    """(4096, 819), b = 16, all 64 groups, 8 trials."""
    ids = {(163 * i) % 4096 for i in range(16)}
    assert len(ids) == 16
    check_exact(rule, 4096, 819, first(0, 4096), marks(ids, 4096), 8, k_max=4, byz_strategy=STRATEGIES[name],
                coin_common=HALF)


@both_modes
@both_strategies
def test_trial_begin_beyond_32_bits(name, rule):
    """The init, coin and stream-12 counters carry both halves of the trial id."""
    s = STRATEGIES[name]
    check_exact(rule, 10, 4, first(1, 10), marks({5}, 10), 150, begin=(1 << 32) + 12345, byz_strategy=s, coin_common=HALF)
    check_exact(rule, 70, 13, first(5, 70), marks({8, 45}, 70), 40, begin=(1 << 32) + 12345, byz_strategy=s)


@both_modes
@both_strategies
def test_split_invariance(name, rule):
    """One launch against three: the trial loop across launches."""
    N, F, trials, a, c = 100, 40, 9000, 3333, 5000              # N <= 5F and an even quorum: both rules take coins
    model.modes_exist()
    plan = benor.TrialsPlan(N, F, first(2, N), seed=SEED, k_max=16, mode=model.mode_of(rule),
                            byzantine=marks({2 + (7 * i) % 98 for i in range(12)}, N), byz_strategy=STRATEGIES[name],
                            coin_common=HALF)
    assert plan.kernel == model.kernel_of(rule, HALF)
    assert plan.live_nodes == 98 and plan.popc_words_per_node_round == 4 * 4   # mode 8's answer: random delivery's unit
    whole = plan.run(0, trials)
    parts = plan.run(0, a) + plan.run(a, c - a) + plan.run(c, trials - c)
    assert np.array_equal(whole, parts)
    assert int(whole[:-1].sum()) == trials


@both_modes
@pytest.mark.parametrize("N,F,f,ids,init,name", [
    (10, 4, 1, {1, 5, 9}, None, "BALANCE"),                   # a crashed node
    (10, 4, 0, {0, 9}, [Q, 1, 0, Q, 1, 1, 0, 0, 1, 0], "SPLIT"),   # a "?" start
    (130, 50, 1, {1, 64, 65, 100, 129}, None, "SPLIT"),       # liars at the group edges
    (130, 50, 2, {2, 63, 128}, None, "BALANCE"),
])
def test_per_node_states(N, F, f, ids, init, name, rule):
    """bo_run_trial_states over 20 trials with crashed, Byzantine and honest nodes, at shapes where coins are taken."""
    model.modes_exist()
    faulty, byz = first(f, N), marks(ids, N)
    kw = dict(byz_strategy=STRATEGIES[name], coin_common=HALF)
    for t in range(20):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=8, initial_values=init,
                                            mode=model.mode_of(rule), byzantine=byz, **kw)
        _, ref_rounds, ref_st = model.sched_trial(rule, N, F, faulty, byz, SEED, t, 8, init, **kw)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
        for i in ids:
            assert st[i] == {"killed": False, "x": None, "decided": None, "k": None}
        for i in range(f):
            assert st[i] == {"killed": True, "x": None, "decided": None, "k": None}


@both_strategies
@pytest.mark.parametrize("coin", [0, ALL])
@pytest.mark.parametrize("N,F", [(64, 12), (130, 46)])
def test_no_choice_is_the_random_delivery_kernels(N, F, coin, name):
    """f = F, b = 0, so m == q: mode 12 gives mode 4's histogram and states (mode 10's with a coin) and mode 13 gives
    mode 9's (mode 11's), device against device."""
    model.modes_exist()
    trials, faulty = 3000, first(F, N)
    twins = {M12: benor.BO_MODE_BYZ_COIN if coin else benor.BO_MODE_RANDOM_TALLY3,
             M13: benor.BO_MODE_BYZ_RULE_B_COIN if coin else benor.BO_MODE_BYZ_RULE_B}
    for mode, twin in twins.items():
        kw = dict(seed=SEED, k_max=16)
        coin_kw = dict(coin_common=coin) if coin else {}
        mine = benor.TrialsPlan(N, F, faulty, mode=mode, byz_strategy=STRATEGIES[name], coin_common=coin, **kw)
        other = benor.TrialsPlan(N, F, faulty, mode=twin, **coin_kw, **kw)
        assert mine.kernel == model.kernel_of("b" if mode == M13 else "ref", coin) and other.kernel != mine.kernel
        assert np.array_equal(mine.run(7, trials), other.run(7, trials))
        for t in (0, 7, 2999):
            assert benor.run_trial_states(N, F, faulty, trial=t, mode=mode, byz_strategy=STRATEGIES[name], coin_common=coin,
                                          **kw) == benor.run_trial_states(N, F, faulty, trial=t, mode=twin, **coin_kw, **kw)


def test_the_plan_holds_no_table():
    """(4096, 819): mode 8's plan uploads the table HG(m, ., q), about 30 MB; this mode's plan holds the honest plane,
    the live ids and the init plane, well under a megabyte (device allocations are counted in 2 MiB steps at most)."""
    model.modes_exist()
    N, F = 4096, 819
    byz = marks({(163 * i) % 4096 for i in range(16)}, N)
    kw = dict(seed=SEED, k_max=4, byzantine=byz, byz_strategy=BALANCE)

    def plan_bytes(mode):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        plan = benor.TrialsPlan(N, F, first(0, N), mode=mode, **kw)
        return free0 - torch.cuda.mem_get_info()[0], plan

    # free memory is the device's, not this process's: the smallest of three readings for "no table"
    used, plan = min((plan_bytes(M13) for _ in range(3)), key=lambda v: v[0])
    with_table, other = plan_bytes(benor.BO_MODE_BYZ_RULE_B)
    print(f"plan bytes at (4096, 819): {used} under the scheduler, {with_table} under random delivery")
    assert plan.kernel == model.K19 and plan.live_nodes == N
    assert used < 8 << 20, used
    assert with_table > 16 << 20, with_table                 # the measure sees a table where there is one
    assert int(plan.run(0, 4)[:-1].sum()) == 4 and int(other.run(0, 4)[:-1].sum()) == 4


@needs_node
@both_strategies
def test_js_run_trials_mode_13(name, tmp_path):
    N, F, trials = 10, 4, 1000
    script = tmp_path / "sched.js"
    script.write_text(
        "const b = require(%s);\n"
        "if (b.MODE_SCHED_TALLY !== 12 || b.MODE_SCHED_RULE_B !== 13) process.exit(2);\n"
        "const byz = new Array(%d).fill(false); byz[2] = true; byz[7] = true;\n"
        "b.runTrials({N: %d, F: %d, faultyList: new Array(%d).fill(false), seed: %dn, kMax: 16,\n"
        "             trialCount: %d, mode: b.MODE_SCHED_RULE_B, byzantineList: byz,\n"
        "             byzStrategy: b.BYZ_%s, coinCommon: 0x80000000})\n"
        "  .then((h) => { console.log(JSON.stringify(Array.from(h, Number))); })\n"
        "  .catch((e) => { console.error(e); process.exit(1); });\n"
        % (json.dumps(os.path.join(PKG, "js", "index.js")), N, N, F, N, SEED, trials, name))
    p = subprocess.run(["node", str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array(json.loads(p.stdout.strip().splitlines()[-1]), dtype=np.uint64)
    assert np.array_equal(got, gpu_hist("b", N, F, first(0, N), marks({2, 7}, N), trials, byz_strategy=STRATEGIES[name],
                                        coin_common=HALF))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_cli_sweep_delivery_adversarial():
    """`sweep --mode byz --delivery adversarial`: a delivery column, and each cell's counts are its plan's."""
    cells, per_cell = [(64, 20, 0), (64, 12, 4), (130, 46, 0)], 500
    out = _cli("sweep", "--mode", "byz", "--delivery", "adversarial", "--byz-strategy", "balance", "--k-max", "16",
               "--cells", ",".join(f"{N}:{F}:{b}" for N, F, b in cells), "--per-cell", str(per_cell))
    lines = out.strip().splitlines()
    keys = lines[0].split(",")
    assert keys[-1] == "delivery" and len(lines) == 1 + len(cells)
    for line, (N, F, b) in zip(lines[1:], cells):
        row = dict(zip(keys, line.split(",")))
        assert (int(row["N"]), int(row["F"]), int(row["b"])) == (N, F, b)
        assert row["delivery"] == "adversarial" and row["mode"] == "byz" and row["byz_strategy"] == "balance"
        h = gpu_hist("ref", N, F, first(0, N), marks(set(range(b)), N), per_cell, seed=SEED ^ (N << 20) ^ F ^ (b << 44),
                     byz_strategy=BALANCE)
        assert int(row["trials"]) == per_cell and int(row["undecided"]) == int(h[:3].sum())
        assert int(row["agreement_violations"]) == int(h[-1])


@pytest.mark.parametrize("name,b", [("balance", 12), ("split", 0)])
def test_cli_trials_mode_byzb_delivery_adversarial(name, b):
    N, F, trials = 100, 19, 5000
    out = _cli("trials", "--N", str(N), "--F", str(F), "--trials", str(trials), "--mode", "byzb", "--crashed", "2",
               "--byzantine", str(b), "--byz-strategy", name, "--k-max", "16", "--coin-common", "1", "--delivery", "adversarial")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["mode"] == "byzb" and row["crashed"] == 2 and row["m"] == N - 2 and row["trials"] == trials
    assert row["byzantine"] == b and row["byz_strategy"] == name and row["delivery"] == "adversarial"
    assert row["coin_common"] == 1.0 and row["coin_common_word"] == ALL and row["kernel"] == benor.KERNEL_NAMES[model.K21]
    byz = marks(set(range(2, 2 + b)), N)                      # the live nodes after the crashed ones
    h = gpu_hist("b", N, F, first(2, N), byz, trials, byz_strategy=STRATEGIES[name.upper()], coin_common=ALL)   # the CLI's default seed is SEED
    assert row["hist"] == [int(v) for v in h] and row["agreement_violations"] == 0 and row["undecided"] == 0
