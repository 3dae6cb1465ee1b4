"""The count-level kernels against their restatements on generated configurations (tests/test_count_level_fuzz.py:
modes 3 to 13, the threshold rules, the class-level chain), and directed cases for the paths a random case reaches
once in 10^6 trials: a rejected word of streams 6, 7 and 11, draw_schedule's later passes, the schedule's clamp.

A failure prints the family, the index and the configuration: fuzz.case(family, i) replays it alone."""
import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import oracle
import test_count_level_fuzz as fuzz
import test_crash_partial as mode6
import test_crash_subset as mode7
import test_crash_tally as mode5
import test_tally3 as mode4

pytestmark = pytest.mark.gpu

HALF = fuzz.HALF
CRASH_MODES = {5: (mode5.crash_trial, {}), 6: (mode6.partial_trial, {"crash_cut": benor.CUT_RANDOM}),
               7: (mode7.subset_trial, {"crash_reach": HALF})}


def bins(h):
    return {i: int(v) for i, v in enumerate(h) if v}


def pieces(begin, trials):
    """Two or three consecutive, uneven pieces of the range, one of them a single trial; a range of one trial twice."""
    if trials < 3:
        return [(begin + k % trials, 1) for k in range(2)]
    a = max(1, (trials - 1) // 3)
    return [(begin, a), (begin + a, 1), (begin + a + 1, trials - a - 1)]


def launch_on_a_stream(plan, begin, trials, ref, label):
    """bo_plan_launch's contract (include/benor.h): outcomes are added into the caller's histogram, and the launches
    of one plan are ordered on one stream."""
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
    pattern = torch.arange(plan.hist_len, dtype=torch.int64, device="cuda") * 7 + 3
    hist = pattern.clone()
    stream.wait_stream(torch.cuda.current_stream())
    for b, n in pieces(begin, trials):
        plan.launch(b, n, hist.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    plan.check()
    got = (hist - pattern).cpu().numpy().astype(np.uint64)
    want = ref * (2 if trials == 1 else 1)          # the one trial was launched twice: added twice
    assert np.array_equal(got, want), (label, "launches on a stream", bins(got), bins(want))


def compare(label, plan, begin, trials, restate, states_of, state_trials, k_max, launch=True):
    """Histogram, asynchronous launches and per-node states of trials [begin, begin + trials) against the restatement
    (each trial restated once)."""
    restated = {t: restate(t) for t in range(begin, begin + trials)}
    ref = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for out in restated.values():
        for b in out[0]:
            ref[b] += 1
    got = plan.run(begin, trials)
    if launch:
        plan.check()
    assert np.array_equal(got, ref), (label, bins(got), bins(ref))
    if launch:
        launch_on_a_stream(plan, begin, trials, ref, label)
    for t in state_trials:
        rounds, st = states_of(t)
        assert rounds == restated[t][1], (label, "rounds of trial", t, rounds, restated[t][1])
        want = restated[t][2]
        if isinstance(want, list):
            assert st == want, (label, "states of trial", t, [(i, a, b) for i, (a, b) in enumerate(zip(st, want)) if a != b])
        else:
            assert st == want, (label, "state of trial", t, st, want)
    return ref


@pytest.mark.parametrize("family,i", fuzz.all_cases())
def test_fuzz(family, i):
    c = fuzz.case(family, i)
    plan = c.plan()
    if c.level == "node":
        assert plan.kernel == c.kernel, str(c)
    compare(str(c), plan, c.begin, c.trials, c.restated, c.states, c.state_trials(), c.kw["k_max"], launch=c.level == "node")


# ------------------------------------------------------------ directed: rejected words
def node_compare(label, kw, restate, begin, trials, state_trials):
    kw = dict(kw)
    N, F, faulty = kw.pop("N"), kw.pop("F"), kw.pop("faulty")
    plan = benor.TrialsPlan(N, F, faulty, **kw)
    return compare(label, plan, begin, trials, restate, lambda t: benor.run_trial_states(N, F, faulty, trial=t, **kw),
                   state_trials, kw["k_max"])


@pytest.mark.parametrize("kind", ["walk", "lane", "heard"])
def test_a_rejected_walk_word(kind):
    """One trial whose walk rejects a word and whose result the rejection decides (the CPU file shows both): stream 6
    in the wave-uniform form (mode 4) and in the lane's own (mode 8, BYZ_RANDOM), stream 11 under BYZ_BALANCE."""
    kw = {"walk": dict(fuzz.BIG, mode=4), "lane": fuzz.LANE, "heard": fuzz.HEARD}[kind]
    t = fuzz.RARE_TRIAL[kind]
    node_compare(f"{kind} trial {t}", kw, fuzz.DIRECTED[kind], t, 1, [t])


def crash_kw(N, F, faulty, mode, k_max, seed=fuzz.SEED, init=None, **sched):
    fn, extra = CRASH_MODES[mode]
    kw = dict(N=N, F=F, faulty=faulty, seed=seed, k_max=k_max, initial_values=init, mode=mode, **sched, **extra)
    return kw, lambda t: fn(N, F, faulty, seed, t, k_max, init, **sched, **extra)


@pytest.mark.parametrize("mode", [5, 6, 7])
@pytest.mark.parametrize("which", ["node", "step"])
def test_a_rejected_schedule_word(which, mode):
    """draw_schedule's `continue`: the first node word, and the first step word (a shape that never decides, so the
    late step is reached)."""
    d = dict(fuzz.SCHED_NODE if which == "node" else fuzz.SCHED_STEP)
    t, N = d.pop("trial"), d["N"]
    kw, restate = crash_kw(N, d["F"], [False] * N, mode, d["k_max"], crash_count=d["crash_count"], crash_window=d["crash_window"])
    node_compare(f"schedule {which} mode {mode} trial {t}", kw, restate, t, 1, [t])


# ------------------------------------------------------------ directed: draw_schedule's second and third pass
@pytest.mark.parametrize("mode", [5, 6, 7])
@pytest.mark.parametrize("N,F,count,trials", [(300, 140, 135, 4), (560, 270, 260, 2)])
def test_schedules_of_more_than_one_pass(N, F, count, trials, mode):
    """A pass holds 256 stream-7 words: 135 crashes need 270, 260 need 520."""
    kw, restate = crash_kw(N, F, [False] * N, mode, 16, crash_count=count, crash_window=6)
    node_compare(f"({N}, {F}) {count} crashes mode {mode}", kw, restate, 11, trials, [11, 11 + trials - 1])


# ------------------------------------------------------------ directed: the clamp at 2 k_max
def scattered(N, ids):
    return [i in ids for i in range(N)]


@pytest.mark.parametrize("mode", [5, 6, 7])
@pytest.mark.parametrize("k_max", [1, 16])
@pytest.mark.parametrize("N,F", [(70, 24), (40, 20)])          # (40, 20) never decides: every run reaches step 2 k_max - 1
def test_explicit_schedules_at_the_clamp(N, F, k_max, mode):
    faulty = scattered(N, {3, 17, N - 1})
    crashers = [5, 6, 20, 33, N - 2]
    beyond = [None] * N
    for k, i in enumerate(crashers):
        beyond[i] = (2 * k_max, 2 * k_max + 1, 2 * k_max + 7, 1 << 20, 0xFFFFFFFE)[k]     # (0xFFFFFFFF is "never")
    astride = [None] * N
    for k, i in enumerate(crashers):
        astride[i] = 2 * k_max - 1 + k % 2
    trials = 40
    kw, restate = crash_kw(N, F, faulty, mode, k_max, crash_at=beyond)
    assert benor.kernel_for(**kw) == benor.BO_KERNEL_TALLY_CRASH + mode - 5     # not demoted: an empty list
    ref = node_compare(f"beyond the clamp ({N}, {F}) k_max {k_max} mode {mode}", kw, restate, 0, trials, [0, trials - 1])
    plain = benor.TrialsPlan(N, F, faulty, seed=fuzz.SEED, k_max=k_max, mode=4).run(0, trials)
    assert np.array_equal(plain, ref), (bins(plain), bins(ref))
    st4 = benor.run_trial_states(N, F, faulty, seed=fuzz.SEED, trial=1, k_max=k_max, mode=4)
    kw5 = dict(kw)
    assert benor.run_trial_states(kw5.pop("N"), kw5.pop("F"), kw5.pop("faulty"), trial=1, **kw5) == st4
    assert restate(1)[1:] == mode4.tally3_trial(N, F, faulty, fuzz.SEED, 1, k_max)[1:]
    kw, restate = crash_kw(N, F, faulty, mode, k_max, crash_at=astride)
    node_compare(f"astride the clamp ({N}, {F}) k_max {k_max} mode {mode}", kw, restate, 0, trials, [0, 1, trials - 1])
