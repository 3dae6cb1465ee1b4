"""Random delivery on the device, path by path: the masks the kernels draw, and the whole kernels around them.

TrialsPlan.delivery_masks (bo_plan_delivery_masks) reads out what the plan's own kernel function -- random_tally for
a Floyd plan, bern_tally<NW, B> through the trial kernel's <NW, B> switch for a Bernoulli plan -- draws for every
receiver of one (trial, round, phase), launched with the plan's own parameters and LDS layout.  Every row must equal
delivery_mask_model (tests/test_delivery_masks.py), whose census says which path each mask takes; that file's census
tests are what make the list below mean something.

Masks (test_masks_equal_the_model, one case of gen.cases() each; test_masks_on_the_rare_paths for the searched ones):

  bern<NW,B> smallest    each of the 21 reachable instantiations at its smallest shape: remove masks, two fix-up
                         blocks or more, flips taken back past the quota, the most padding at m = 2^(b-1) + 1
  bern<NW,B> balanced    the same instantiations with 16 q just below a m: add masks, c = q (no fix-up)
  bern m=2^b             no padding row, rows == W32: no field is refused by its index
  bern m%32=31, W32=5|6  the last mask word's tail and the padding bits of that word, W32 odd and even
  bern NW=. W32%4=.      partial super-blocks of the three-, one- and two-word comparators
  bern a=3, a=14         the comparator's two ends, the largest |c - q|;  16q|m: p = q / m exactly
  floyd k=63 | bern k=64, floyd 8k=m | bern 8k=m+8     the sampler boundary from both sides: the plan must run the
                         sampler oracle.delivery_bernoulli names, or its masks differ (gen.test_boundary_sides_...)
  floyd m<=32, 64, 65, >2048;  k = 0, k = 1 in both senses;  k mod 4 = 1, 2, 3 (a short last fast block)
  floyd 8k=m (600, 525), (600, 75)     collisions, both deliver_T senses
  floyd rare (...)       searched (trial, phase) pairs: Lemire rejections of a block's first and last word with
                         further draws behind them (the exact path re-enters mid-block and leaves the stream
                         misaligned), and screen hits that reject nothing
  bern N=4096 m=200      node ids up to 4095 in the last counter word, live_ids far from the compact indices
  every case             crashed nodes scattered over the ids, a 63-bit seed, a trial id in {0, 2^32 - 1, 2^32,
                         2^40 + 12345} (thi feeds the hoisted x1 of dlv_uniforms and the Floyd counter), a round in
                         {1, 2, 255, 256, 1024} (bits 16-30 of the word that carries the block index), either phase,
                         and a plan with k_max 16 or 1024 (the histogram's LDS in front of the waves' regions)

Whole kernels against oracle.run_trials, per-node states and histograms (the trial kernels' own launches):

  test_instantiations_and_floyd_shapes    the 21 instantiations and every Floyd shape, crashed nodes scattered
  test_trial_ids_across_2_32              trial_begin = 2^32 - 3 with 8 trials, and 2^40: tlo wraps, thi changes
  test_never_deciding_runs_k_max_1024     q = F: nobody can decide; 1024 rounds, k = 1025, the undecided bins
  test_several_trials_per_wave            BENOR_BLOCKS_PER_CU=1 and more trials than that grid has waves: the
                                          grid-stride loop reuses the LDS bitset and planes for a second trial
  test_question_mark_starts               an odd and an even number of "?" starts: round 1's two-plane tally
  test_degenerate_quorums                 q = m, q = m - 1 and q = 1
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import oracle
import test_delivery_masks as gen

pytestmark = pytest.mark.gpu

RD = benor.BO_MODE_RANDOM_DELIVERY
ORD = oracle.MODE_RANDOM_DELIVERY


def popcounts(rows):
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1).sum(axis=1)


def compare(i):
    c = gen.cases()[i]
    plan = benor.TrialsPlan(c.N, c.F, list(c.faulty), seed=c.seed, k_max=1024 if i % 4 == 0 else 16, mode=RD)
    assert plan.kernel == benor.BO_KERNEL_RANDOM and plan.live_nodes == c.m
    got = plan.delivery_masks(c.trial, c.rnd, c.phase)
    masks, census = gen.case_masks(i)
    want = np.array([gen.mask_words(mk, c.m) for mk in masks], dtype=np.uint64).reshape(c.m, (c.m + 63) // 64)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (f"{c}: {bad.size} of {c.m} receivers differ; first: compact index {int(bad[0])}, node "
                           f"{c.live[int(bad[0])]}, census {census[int(bad[0])]}")
    assert (popcounts(got) == c.q).all(), str(c)


@pytest.mark.parametrize("i", range(gen.N_LISTED))
def test_masks_equal_the_model(i):
    compare(i)


def test_masks_on_the_rare_paths():
    assert len(gen.cases()) > gen.N_LISTED
    for i in range(gen.N_LISTED, len(gen.cases())):
        compare(i)


def test_entry_validates_its_arguments():
    N, F = 140, 70
    fl = [i < 4 for i in range(N)]
    plan = benor.TrialsPlan(N, F, fl, seed=1, k_max=8, mode=RD)
    for trial, rnd, phase in ((0, 0, 0), (0, 0x8000, 0), (0, 1, 2)):
        with pytest.raises(RuntimeError, match="libbenor error 3.*bo_plan_delivery_masks"):
            plan.delivery_masks(trial, rnd, phase)
    assert plan.delivery_masks(0, 0x7FFF, 1).shape == (136, 3)
    for other in (benor.TrialsPlan(10, 4, seed=1, k_max=8), benor.TrialsPlan(140, 70, seed=1, k_max=8)):
        assert other.kernel != benor.BO_KERNEL_RANDOM
        with pytest.raises(RuntimeError, match="libbenor error 3.*not BO_KERNEL_RANDOM"):
            other.delivery_masks(0, 1, 0)


# ------------------------------------------------------------------------------------------------ whole kernels
def against_oracle(N, F, fl, *, seed, begin, T, k_max, init=None, state_trials=None):
    """The histogram of trials [begin, begin + T) and the per-node states of state_trials (default: the first)."""
    fl = list(fl)
    plan = benor.TrialsPlan(N, F, fl, seed=seed, k_max=k_max, initial_values=init, mode=RD)
    assert plan.kernel == benor.BO_KERNEL_RANDOM
    got = plan.run(begin, T)
    ref = oracle.run_trials(N, F, fl, seed=seed, trial_begin=begin, trial_count=T, k_max=k_max, initial_values=init,
                            mode=ORD).hist
    np.testing.assert_array_equal(got, ref, err_msg=f"N={N} F={F} begin={begin}")
    states = []
    for t in (begin,) if state_trials is None else state_trials:
        rounds, st = benor.run_trial_states(N, F, fl, seed=seed, trial=t, k_max=k_max, initial_values=init, mode=RD)
        want = oracle.run_trials(N, F, fl, seed=seed, trial_begin=t, trial_count=1, k_max=k_max, initial_values=init,
                                 mode=ORD, want_states=True)
        assert st == want.states, f"N={N} F={F} trial={t}"
        live = [s for s in st if not s["killed"]]
        assert rounds == (live[0]["k"] - 1 if all(s["decided"] for s in live) else 0)
        states.append(st)
    return got, states


def first_case(tag):
    return next(c for c in gen.cases() if c.tag == tag)


WHOLE = [tag for _, _, tag in gen.SHAPES if "smallest" in tag or tag.startswith("floyd")]


@pytest.mark.parametrize("tag", WHOLE)
def test_instantiations_and_floyd_shapes(tag):
    c = first_case(tag)
    assert sum(c.faulty) > 0
    T = 60 if c.m <= 300 else (12 if c.m <= 1100 else 3)
    against_oracle(c.N, c.F, c.faulty, seed=c.seed, begin=c.trial, T=T, k_max=8)


@pytest.mark.parametrize("tag", ["bern<4,8> smallest", "floyd m=65 k=25"])
def test_trial_ids_across_2_32(tag):
    c = first_case(tag)
    against_oracle(c.N, c.F, c.faulty, seed=c.seed, begin=2**32 - 3, T=8, k_max=8, state_trials=(2**32 - 1, 2**32))
    against_oracle(c.N, c.F, c.faulty, seed=c.seed, begin=2**40, T=8, k_max=8)


@pytest.mark.parametrize("N,F", [(200, 100), (40, 20)])
def test_never_deciding_runs_k_max_1024(N, F):
    """q = N - F = F: no count exceeds F, nobody decides, every trial runs all 1024 rounds."""
    assert (gen.sampler_of(N, N - F) is None) == (N == 40)
    hist, (st,) = against_oracle(N, F, [False] * N, seed=0x1024 + N, begin=2**32 - 2, T=4, k_max=1024)
    assert all(s["k"] == 1025 and not s["decided"] for s in st)
    assert int(hist[:3].sum()) == 4 and int(hist.sum()) == 4


@pytest.mark.parametrize("tag", ["bern<4,8> smallest", "floyd m<=32 k=7"])
def test_several_trials_per_wave(tag, monkeypatch):
    """One workgroup per CU and more trials than that grid has waves (4 per workgroup, at most 256 CUs), so a wave
    runs a second and a third trial on the LDS its first one left; the same histogram as the default grid's."""
    c = first_case(tag)
    T = 2 * 4 * 256 + 77
    dflt, _ = against_oracle(c.N, c.F, c.faulty, seed=c.seed, begin=c.trial, T=T, k_max=8)
    monkeypatch.setenv("BENOR_BLOCKS_PER_CU", "1")
    one, _ = against_oracle(c.N, c.F, c.faulty, seed=c.seed, begin=c.trial, T=T, k_max=8)
    np.testing.assert_array_equal(one, dflt)


@pytest.mark.parametrize("nq", [5, 6])
def test_question_mark_starts(nq):
    """Fixed starts with nq "?" among the live nodes: round 1 tallies both planes (c0 is not q - c1)."""
    c = first_case("bern<4,8> smallest")
    rng = np.random.default_rng(gen.BASE + 700 + nq)
    init = [int(v) for v in rng.integers(0, 2, c.N)]
    for i in rng.choice(c.live, nq, replace=False):
        init[int(i)] = "?"
    against_oracle(c.N, c.F, c.faulty, seed=c.seed, begin=2**32 - 1, T=40, k_max=8, init=init)


@pytest.mark.parametrize("m,q", [(300, 300), (300, 299), (130, 1), (50, 50), (37, 36), (37, 1)])
def test_degenerate_quorums(m, q):
    rng = np.random.default_rng(gen.BASE + 800 + m + q)
    N, F, fl = gen.network(rng, m, q)
    assert gen.sampler_of(m, q) is None
    against_oracle(N, F, fl, seed=int(rng.integers(0, 2**63)), begin=2**40 + 5, T=30, k_max=8)
