"""BO_MODE_BYZ_COIN and BO_MODE_BYZ_RULE_B_COIN on the device (the CoinShared entries of
csrc/benor_tally_byz.hip, variants 16 and 17): bit-exact against the plain-Python restatement
in tests/test_byz_coin.py (histograms and per-node states), launch mechanics, the plans that
collapse to modes 8 and 9, what the shared coin does to Rule B's waiting time, and the JS and
CLI surfaces.  The mode-8 and mode-9 GPU tests are the check that variants 14 and 15, which
share the trial loops, compute what they did."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import oracle
import test_byz_coin as model
import test_byz_rule_b as mode9
from conftest import PKG, ROOT
from test_js_api import needs_node
from test_tally import first

pytestmark = pytest.mark.gpu

M10, M11, K16, K17 = model.M10, model.M11, model.K16, model.K17   # None before the modes: every test fails
RANDOM, OPPOSE, BALANCE, SPLIT = model.RANDOM, model.OPPOSE, model.BALANCE, model.SPLIT
STRATEGIES = model.STRATEGIES
ALL, HALF = model.ALL, model.HALF
SEED = model.SEED
marks = model.marks
Q = "?"
every_strategy = pytest.mark.parametrize("name", list(STRATEGIES))
both_modes = model.both_modes
every_coin = pytest.mark.parametrize("coin", [1, HALF, ALL])


def kernel_of(rule):
    return K17 if rule == "b" else K16


def gpu_hist(rule, N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, kernel=None, coin_common=ALL, **lie):
    model.modes_exist()
    plan = benor.TrialsPlan(N, F, faulty, seed=seed, k_max=k_max, initial_values=init, mode=model.mode_of(rule),
                            byzantine=byz, coin_common=coin_common, **lie)
    assert plan.kernel == (kernel_of(rule) if kernel is None else kernel)
    h = plan.run(begin, trials)
    plan.check()                                              # no overflow or deferral state
    return h


def check_exact(rule, N, F, faulty, byz, trials, *, seed=SEED, k_max=16, begin=0, init=None, coin_common=ALL, **lie):
    """The launch's histogram, and the per-node states of its first two and last trials, against the restatement
    (each trial restated once)."""
    got = gpu_hist(rule, N, F, faulty, byz, trials, seed=seed, k_max=k_max, begin=begin, init=init,
                   coin_common=coin_common, **lie)
    ref = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    restated = {}
    for t in range(begin, begin + trials):
        restated[t] = model.coin_trial(rule, N, F, faulty, byz, seed, t, k_max, init, coin_common=coin_common, **lie)
        for b in restated[t][0]:
            ref[b] += 1
    assert np.array_equal(got, ref), ({i: int(v) for i, v in enumerate(got) if v},
                                      {i: int(v) for i, v in enumerate(ref) if v})
    for t in sorted({begin, begin + min(1, trials - 1), begin + trials - 1}):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=seed, trial=t, k_max=k_max, initial_values=init,
                                            mode=model.mode_of(rule), byzantine=byz, coin_common=coin_common, **lie)
        _, ref_rounds, ref_st = restated[t]
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
    return got


@both_modes
@every_strategy
@every_coin
@pytest.mark.parametrize("ids", [{3}, {3, 8}])
def test_bit_exact_11_2(ids, coin, name, rule):
    """(11, 2, f = 0), one and two liars, 200 trials."""
    h = check_exact(rule, 11, 2, first(0, 11), marks(ids, 11), 200, byz_one=HALF, byz_strategy=STRATEGIES[name], coin_common=coin)
    assert int(h[:-1].sum()) == 200
    if rule == "b":
        assert mode9.forbidden_bins(h) == 0


@both_modes
@every_strategy
@pytest.mark.parametrize("coin", [HALF, ALL])
def test_bit_exact_even_quorum(coin, name, rule):
    """(10, 4), b = 2: an even quorum, so the reference rule ties and takes coins; Rule B is outside N > 5F and
    takes a coin at every node in every round."""
    h = check_exact(rule, 10, 4, first(1, 10), marks({2, 7}, 10), 200, byz_one=HALF, byz_strategy=STRATEGIES[name], coin_common=coin)
    assert int(h[:-1].sum()) == 200


@both_modes
@every_strategy
def test_k_max_one(name, rule):
    h = check_exact(rule, 11, 2, first(0, 11), marks({2, 7}, 11), 400, k_max=1, byz_one=HALF, byz_strategy=STRATEGIES[name])
    assert int(h[:-1].sum()) == 400


@both_modes
@every_strategy
@pytest.mark.parametrize("ids", [{4}, {0, 4}])
def test_fixed_init_with_question_marks(name, ids, rule):
    """(12, 2) with "?" starts: under BALANCE and SPLIT stage 2 runs in round 1's R-phase."""
    init = [Q, 1, 0, 1, Q, 1, 1, 0, 1, Q, 1, 1]               # nodes 0 and 4 may be liars: no initial value of the run
    check_exact(rule, 12, 2, first(0, 12), marks(ids, 12), 200, init=init, byz_one=HALF, byz_strategy=STRATEGIES[name],
                coin_common=HALF)
    init = [Q, 1, 0, 0, Q, 1, 0, 0, 1, Q, 1, 0]               # balanced: coins are taken
    check_exact(rule, 12, 2, first(0, 12), marks(ids, 12), 200, init=init, byz_one=HALF, byz_strategy=STRATEGIES[name])


@both_modes
@every_coin
def test_no_byzantine_node(coin, rule):
    """b = 0 with a shared coin is valid in both modes and runs the new kernels: (11, 2, f = 2), which is m == q, and
    (26, 5) with and without crashed nodes; one histogram for every strategy and byz_one.  Mode 10 is then the
    reference's crash-tolerant rule under random delivery with a shared coin: not mode 4's histogram."""
    for N, F, f in ((11, 2, 2), (26, 5, 0), (26, 5, 3), (10, 4, 0)):
        ref = check_exact(rule, N, F, first(f, N), marks(set(), N), 200, byz_one=0, byz_strategy=RANDOM, coin_common=coin)
        for strategy in STRATEGIES.values():
            assert np.array_equal(ref, gpu_hist(rule, N, F, first(f, N), marks(set(), N), 200, byz_one=HALF,
                                                byz_strategy=strategy, coin_common=coin))
        assert np.array_equal(ref, gpu_hist(rule, N, F, first(f, N), None, 200, coin_common=coin))   # no byzantine= at all
    if rule == "ref" and coin == ALL:
        mode4 = benor.TrialsPlan(10, 4, first(0, 10), seed=SEED, k_max=16, mode=benor.BO_MODE_RANDOM_TALLY3).run(0, 200)
        assert not np.array_equal(ref, mode4)


@both_modes
@every_strategy
def test_bit_exact_64_12(name, rule):
    """(64, 12), b = 12 = F: one full group."""
    ids = {(5 * i) % 64 for i in range(12)}
    check_exact(rule, 64, 12, first(0, 64), marks(ids, 64), 60, k_max=32, byz_one=HALF, byz_strategy=STRATEGIES[name])
    check_exact(rule, 64, 12, first(0, 64), marks(ids, 64), 20, k_max=8, byz_one=HALF, byz_strategy=STRATEGIES[name],
                coin_common=HALF)


@both_modes
@every_strategy
def test_group_boundaries(name, rule):
    """(70, 13), b = 13 with compact index 64 Byzantine (group 1 has five receivers), and (130, 25) with liars in all
    three groups (group 2 is nodes 128, a liar, and 129)."""
    ids = {64} | {(5 * i) % 60 for i in range(12)}
    assert len(ids) == 13
    check_exact(rule, 70, 13, first(0, 70), marks(ids, 70), 60, byz_one=HALF, byz_strategy=STRATEGIES[name], coin_common=HALF)
    check_exact(rule, 130, 25, first(0, 130), marks({0, 63, 64, 100, 128}, 130), 30, byz_one=HALF,
                byz_strategy=STRATEGIES[name])


@both_modes
@every_strategy
def test_more_liars_than_lanes(name, rule):
    """(400, 70), b = 70 = F."""
    ids = {(17 * i) % 400 for i in range(70)}
    assert len(ids) == 70
    check_exact(rule, 400, 70, first(0, 400), marks(ids, 400), 3, byz_one=HALF, byz_strategy=STRATEGIES[name])


@both_modes
@pytest.mark.parametrize("name", ["RANDOM", "SPLIT"])
def test_bit_exact_large_network(name, rule):
    """(1024, 204), b = 16, sixteen groups, random starts, both entries (RANDOM: the per-lane loop, SPLIT: the one
    that reads the inbox).  With a coin common in every round a trial ends after about two rounds."""
    ids = {(41 * i) % 1024 for i in range(16)}
    assert len(ids) == 16
    check_exact(rule, 1024, 204, first(0, 1024), marks(ids, 1024), 12, k_max=32, byz_one=HALF, byz_strategy=STRATEGIES[name])


@both_modes
@pytest.mark.parametrize("name", ["RANDOM", "OPPOSE"])
def test_bit_exact_thresholds_searched_in_global_memory(name, rule):
    """(2048, 682), b = 300: the 2400 B of thresholds would cost a resident workgroup and are searched in global
    memory.  N <= 3F: Rule B never proposes, every node takes the round's coin; k_max 3, two trials."""
    ids = {(7 * i) % 2048 for i in range(300)}
    assert len(ids) == 300
    check_exact(rule, 2048, 682, first(0, 2048), marks(ids, 2048), 2, k_max=3, byz_one=HALF, byz_strategy=STRATEGIES[name])


@both_modes
@every_strategy
def test_trial_begin_beyond_32_bits(name, rule):
    """The stream-12 counter carries both halves of the trial id."""
    strategy = STRATEGIES[name]
    check_exact(rule, 10, 4, first(1, 10), marks({5}, 10), 150, begin=(1 << 32) + 12345, byz_one=HALF, byz_strategy=strategy,
                coin_common=HALF)
    check_exact(rule, 70, 13, first(5, 70), marks({8, 45}, 70), 40, begin=(7 << 32) - 20, byz_one=HALF, byz_strategy=strategy)


@both_modes
@every_strategy
def test_split_invariance(name, rule):
    """One launch against three: the word is keyed by trial and round, not by the launch split."""
    N, F, trials, a, c = 100, 40, 9000, 3333, 5000              # N <= 5F and an even quorum: both rules take coins
    model.modes_exist()
    plan = benor.TrialsPlan(N, F, first(2, N), seed=SEED, k_max=16, mode=model.mode_of(rule),
                            byzantine=marks({2 + (7 * i) % 98 for i in range(12)}, N), byz_one=HALF,
                            byz_strategy=STRATEGIES[name], coin_common=HALF)
    assert plan.kernel == kernel_of(rule)
    assert plan.live_nodes == 98 and plan.popc_words_per_node_round == 4 * 4   # modes 8 and 9's answer: random delivery's unit
    whole = plan.run(0, trials)
    parts = plan.run(0, a) + plan.run(a, c - a) + plan.run(c, trials - c)
    assert np.array_equal(whole, parts)
    assert int(whole[:-1].sum()) == trials


@both_modes
@pytest.mark.parametrize("N,F,f,ids,init,name", [
    (10, 4, 1, {1, 5, 9}, None, "RANDOM"),
    (10, 4, 0, {0, 9}, [Q, 1, 0, Q, 1, 1, 0, 0, 1, 0], "SPLIT"),
    (130, 50, 1, {1, 64, 65, 100, 129}, None, "OPPOSE"),
    (130, 50, 2, {2, 66, 129}, None, "BALANCE"),
])
def test_per_node_states(N, F, f, ids, init, name, rule):
    """bo_run_trial_states over 20 trials with crashed, Byzantine and honest nodes, at shapes where coins are taken."""
    model.modes_exist()
    faulty, byz = first(f, N), marks(ids, N)
    kw = dict(byz_one=HALF, byz_strategy=STRATEGIES[name], coin_common=HALF)
    for t in range(20):
        rounds, st = benor.run_trial_states(N, F, faulty, seed=SEED, trial=t, k_max=8, initial_values=init,
                                            mode=model.mode_of(rule), byzantine=byz, **kw)
        _, ref_rounds, ref_st = model.coin_trial(rule, N, F, faulty, byz, SEED, t, 8, init, **kw)
        assert rounds == ref_rounds, (t, rounds, ref_rounds)
        assert st == ref_st, (t, [(i, a, b) for i, (a, b) in enumerate(zip(st, ref_st)) if a != b])
        for i in ids:
            assert st[i] == {"killed": False, "x": None, "decided": None, "k": None}
        for i in range(f):
            assert st[i] == {"killed": True, "x": None, "decided": None, "k": None}


@every_strategy
@pytest.mark.parametrize("b", [0, 2])
def test_coin_common_0_is_the_parent_modes_plan(b, name):
    """coin_common = 0 on the device: modes 8 and 9, kernel choice included (mode 4's plan at b = 0 in mode 10)."""
    N, F, trials = 100, 19, 3000
    byz, lie = marks(set(range(3, 3 + b)), N), dict(byz_one=HALF, byz_strategy=STRATEGIES[name])
    for init in (None, [Q if i % 9 == 0 else 1 if i % 2 else 0 for i in range(N)]):
        kw = dict(seed=SEED, k_max=16, initial_values=init, byzantine=byz, **lie)
        p8 = benor.TrialsPlan(N, F, first(1, N), mode=benor.BO_MODE_BYZ_TALLY, **kw)
        p9 = benor.TrialsPlan(N, F, first(1, N), mode=benor.BO_MODE_BYZ_RULE_B, **kw)
        p10 = benor.TrialsPlan(N, F, first(1, N), mode=M10, coin_common=0, **kw)
        p11 = benor.TrialsPlan(N, F, first(1, N), mode=M11, coin_common=0, **kw)
        assert p10.kernel == p8.kernel and p11.kernel == p9.kernel == benor.BO_KERNEL_TALLY_BYZ_B
        assert p8.kernel == (benor.BO_KERNEL_TALLY_BYZ if b else benor.BO_KERNEL_TALLY if init is None else benor.BO_KERNEL_TALLY3)
        assert np.array_equal(p10.run(5, trials), p8.run(5, trials))
        assert np.array_equal(p11.run(5, trials), p9.run(5, trials))
        for t in (0, 7):
            s8 = benor.run_trial_states(N, F, first(1, N), trial=t, mode=benor.BO_MODE_BYZ_TALLY, **kw)
            s9 = benor.run_trial_states(N, F, first(1, N), trial=t, mode=benor.BO_MODE_BYZ_RULE_B, **kw)
            assert benor.run_trial_states(N, F, first(1, N), trial=t, mode=M10, coin_common=0, **kw) == s8
            assert benor.run_trial_states(N, F, first(1, N), trial=t, mode=M11, coin_common=0, **kw) == s9


@every_strategy
def test_the_shared_coin_decides_where_local_coins_do_not(name):
    """(1024, 204), b = 16, random starts, k_max 32, 2000 trials: with a coin common in every round no trial stays
    undecided and none violates agreement; mode 9 on the same trials decides none."""
    N, F, trials = 1024, 204, 2000
    byz = marks({(41 * i) % 1024 for i in range(16)}, N)
    lie = dict(byz_one=HALF, byz_strategy=STRATEGIES[name])
    got = gpu_hist("b", N, F, first(0, N), byz, trials, k_max=32, **lie)
    assert int(got[:-1].sum()) == trials
    assert int(got[:3].sum()) == 0, [int(v) for v in got[:3]]
    assert mode9.forbidden_bins(got, 32) == 0
    local = benor.TrialsPlan(N, F, first(0, N), seed=SEED, k_max=32, mode=benor.BO_MODE_BYZ_RULE_B, byzantine=byz, **lie).run(0, trials)
    assert int(local[:3].sum()) == trials


@needs_node
@pytest.mark.parametrize("name", ["OPPOSE", "SPLIT"])
def test_js_run_trials_mode_11(name, tmp_path):
    N, F, trials = 10, 4, 1000
    script = tmp_path / "coin.js"
    script.write_text(
        "const b = require(%s);\n"
        "if (b.MODE_BYZ_RULE_B_COIN !== 11 || b.MODE_BYZ_COIN !== 10) process.exit(2);\n"
        "const byz = new Array(%d).fill(false); byz[2] = true; byz[7] = true;\n"
        "b.runTrials({N: %d, F: %d, faultyList: new Array(%d).fill(false), seed: %dn, kMax: 16,\n"
        "             trialCount: %d, mode: b.MODE_BYZ_RULE_B_COIN, byzantineList: byz, byzOne: 0x80000000,\n"
        "             byzStrategy: b.BYZ_%s, coinCommon: 0x80000000})\n"
        "  .then((h) => { console.log(JSON.stringify(Array.from(h, Number))); })\n"
        "  .catch((e) => { console.error(e); process.exit(1); });\n"
        % (json.dumps(os.path.join(PKG, "js", "index.js")), N, N, F, N, SEED, trials, name))
    p = subprocess.run(["node", str(script)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.array(json.loads(p.stdout.strip().splitlines()[-1]), dtype=np.uint64)
    assert np.array_equal(got, gpu_hist("b", N, F, first(0, N), marks({2, 7}, N), trials, byz_one=HALF,
                                        byz_strategy=STRATEGIES[name], coin_common=HALF))


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "benor.cli", *args], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


@pytest.mark.parametrize("name", ["random", "balance"])
def test_cli_trials_mode_byzb_coin_common(name):
    N, F, trials = 100, 19, 5000
    out = _cli("trials", "--N", str(N), "--F", str(F), "--trials", str(trials), "--mode", "byzb", "--crashed", "2",
               "--byzantine", "12", "--byz-one", "0.5", "--byz-strategy", name, "--k-max", "16", "--coin-common", "1")
    row = json.loads(out.strip().splitlines()[-1])
    assert row["mode"] == "byzb" and row["crashed"] == 2 and row["m"] == N - 2 and row["trials"] == trials
    assert row["byzantine"] == 12 and row["byz_one_word"] == HALF and row["byz_strategy"] == name
    assert row["coin_common"] == 1.0 and row["coin_common_word"] == ALL and row["kernel"] == benor.KERNEL_NAMES[K17]
    byz = marks(set(range(2, 14)), N)                         # the 12 live nodes after the crashed ones
    h = gpu_hist("b", N, F, first(2, N), byz, trials, byz_one=HALF, byz_strategy=STRATEGIES[name.upper()])   # the CLI's default seed is SEED
    assert row["hist"] == [int(v) for v in h] and row["agreement_violations"] == 0 and row["undecided"] == 0
