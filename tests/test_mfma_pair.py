"""The KIND 0 matrix-core kernel's paired form (csrc/benor_mfma.h, PAIR): two
receiver tiles per f32 accumulator, counts in two bit fields
(csrc/benor_mfma_pair.h).

CPU: tests/pair_fields_check.cpp, a host program over the helper header, runs
the field arithmetic in f32 for every odd vote count and every combination of
the extreme and threshold counts in the two fields -- a lockstep GPU run only
ever carries equal counts in both.
GPU: the default (paired) form's histogram against the oracle, against the
one-tile form (BENOR_MFMA_PAIR=0) and against the popcount kernel
(BENOR_NO_MFMA=1), on 20,011 trials (a partial last group of 32): both tile
parities, one live row in the last tile, W = 2 .. 11, the largest thresholds
(m = 1023), and fixed initial values at and next to the proposal threshold.
"""
import contextlib
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import benor
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ben-or-consensus-algorithm_amd", "csrc")
T = 20_011
K_MAX = 8


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def first_f(N, F):
    return [i < F for i in range(N)]


# ------------------------------------------------------------------ CPU
def test_knob_is_registered():
    assert benor.KNOBS["BENOR_MFMA_PAIR"] == "validation"


def test_field_arithmetic_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "pair_fields_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "pair_fields_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[0].isdigit() and int(r.stdout.split()[0]) > 100_000 and " 0 failures" in r.stdout, r.stdout


# ------------------------------------------------------------------ GPU
SHAPES = [
    (97, 32),      # m = 65: W = 2, MT = 3 (the last tile alone in its accumulator), one live row
    (130, 33),     # m = 97: MT = 4, one live row in the last tile
    (256, 85),     # m = 171: configs[2]
    (300, 43),     # m = 257: W = 5, MT = 9 odd, one live row
    (1000, 333),   # m = 667: W = 11
    (1024, 341),   # m = 683: headline
    (1023, 0),     # m = 1023: P threshold 1023, R threshold 512
    (1024, 1),     # m = 1023, F = 1
]


@functools.lru_cache(maxsize=None)
def oracle_hist(N, F, seed, init):
    kw = {"initial_values": list(init)} if init is not None else {}
    h = oracle.run_trials(N, F, first_f(N, F), seed=seed, trial_begin=7, trial_count=T, k_max=K_MAX, **kw).hist
    h.setflags(write=False)
    return h


def run_form(N, F, seed, init, **knobs):
    kw = {"initial_values": list(init)} if init is not None else {}
    with env(**{"BENOR_MFMA_PAIR": None, "BENOR_NO_MFMA": None, **knobs}):
        p = benor.TrialsPlan(N, F, seed=seed, k_max=K_MAX, **kw)
        want = benor.BO_KERNEL_W if knobs.get("BENOR_NO_MFMA") else benor.BO_KERNEL_MFMA
        assert p.kernel == want, (p.kernel, knobs)
        return p.run(7, T)


def check_three_ways(N, F, seed, init=None):
    ref = oracle_hist(N, F, seed, init)
    paired = run_form(N, F, seed, init)
    print(f"N={N} F={F}: paired {paired[paired > 0]}, oracle {ref[ref > 0]}")
    np.testing.assert_array_equal(paired, ref)
    np.testing.assert_array_equal(paired, run_form(N, F, seed, init, BENOR_MFMA_PAIR="0"))
    np.testing.assert_array_equal(paired, run_form(N, F, seed, init, BENOR_NO_MFMA="1"))
    assert int(paired.sum()) - int(paired[-1]) == T        # every trial halts; the last bin counts disagreements
    return paired


@pytest.mark.gpu
@pytest.mark.parametrize("N,F", SHAPES)
def test_paired_form_random_init(N, F):
    check_three_ways(N, F, seed=0xB0 + N)


def fixed_init(N, F, ones, q=0):
    """Live nodes F .. N-1: `q` of them "?", `ones` of them 1, the rest 0, spread
    over the chunks by a fixed permutation."""
    live = np.random.default_rng(N * 31 + ones + q).permutation(np.arange(F, N))
    vals = [0] * N
    for j in live[:q]:
        vals[j] = "?"
    for j in live[q:q + ones]:
        vals[j] = 1
    return tuple(vals)


def fixed_cases():
    out = []
    for N, F in ((97, 32), (256, 85), (300, 43), (1024, 341), (1023, 0)):
        m = N - F
        t = m // 2 + 1
        for ones in (0, m, t - 1, t):
            out.append(pytest.param(N, F, ones, 0, id=f"{N}-{F}-ones{ones}"))
    # "?" inputs: M1 = m - q binary votes, t = floor(M1 / 2) + 1
    for N, F, q in ((256, 85, 2), (1024, 341, 4), (300, 43, 2), (97, 32, 4)):
        t = (N - F - q) // 2 + 1
        for ones in (t - 1, t):
            out.append(pytest.param(N, F, ones, q, id=f"{N}-{F}-q{q}-ones{ones}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N,F,ones,q", fixed_cases())
def test_paired_form_fixed_init(N, F, ones, q):
    init = fixed_init(N, F, ones, q)
    got = check_three_ways(N, F, seed=5, init=init)
    # every trial is the same trial: all decide the majority value in round 1
    t = (N - F - q) // 2 + 1
    assert got[3 + (1 if ones >= t else 0)] == T
