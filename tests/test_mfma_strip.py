"""The KIND 0 matrix-core kernel's strip form (csrc/benor_mfma.h, STRIP): where
the last 32-row receiver tile has at most 16 live rows (and W >= 5), that tile
runs in the 16-row product shape after a row swap of the operand registers
(csrc/benor_mfma_strip.h).

CPU: tests/strip_layout_check.cpp models the 64 lanes, the two shapes' lane
maps and the swaps for every eligible (W, tile parity, live rows), with labels
for votes: every sender and every proposal is counted exactly once in its own
trial's column, no padded row is, and the folded decisions reach their trial.
GPU: the strip form's histogram against the oracle, against the 32-row form
(BENOR_MFMA_STRIP=0) and against the popcount kernel (BENOR_NO_MFMA=1), each
statically scheduled and with claimed chunks (BENOR_MFMA_DYNAMIC=1).
"""
import contextlib
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import benor
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ben-or-consensus-algorithm_amd", "csrc")
T = 20_011
K_MAX = 8
KNOBS = ("BENOR_MFMA_STRIP", "BENOR_MFMA_DYNAMIC", "BENOR_MFMA_CHUNK", "BENOR_MFMA_PAIR", "BENOR_NO_MFMA",
         "BENOR_BLOCKS_PER_CU", "BENOR_TIMELINE")
DYNAMIC = [pytest.param("0", id="static"), pytest.param("1", id="dynamic")]


@contextlib.contextmanager
def env(**kv):
    kv = {**{k: None for k in KNOBS}, **kv}
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
    assert benor.KNOBS["BENOR_MFMA_STRIP"] == "validation"


def build_layout_check(tmp_path, *flags):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "strip_layout_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(ROOT, "tests", "strip_layout_check.cpp"), "-o", str(exe)], check=True)
    return exe


def test_lanes_swaps_and_columns_on_the_host(tmp_path):
    r = subprocess.run([str(build_layout_check(tmp_path))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    # 192 eligible shapes, each with >= 32 trials x 257 senders checked three times
    assert r.stdout.split()[0].isdigit() and int(r.stdout.split()[0]) > 192 * 3 * 32 * 257 and " 0 failures" in r.stdout, r.stdout


# ------------------------------------------------------------------ GPU
# N, F: m, W, live rows of the last tile
SHAPES = [
    (257, 0),      # m = 257: W = 5 odd, last sender chunk <= 32, MT = 9, one live row
    (300, 31),     # m = 269: MT odd, 13 live rows
    (300, 29),     # m = 271: 15 live rows
    (400, 37),     # m = 363: W = 6 even, MT = 12 even, 11 live rows
    (367, 0),      # m = 367: 15 live rows, MT even
    (273, 0),      # m = 273: 17 live rows, not eligible -- the knob set to 1 changes nothing
    (1003, 0),     # m = 1003: W = 16
    (1024, 341),   # m = 683: the headline shape
]


@functools.lru_cache(maxsize=None)
def oracle_hist(N, F, seed, begin, count, init=None):
    kw = {"initial_values": list(init)} if init is not None else {}
    h = oracle.run_trials(N, F, first_f(N, F), seed=seed, trial_begin=begin, trial_count=count, k_max=K_MAX, **kw).hist
    h.setflags(write=False)
    return h


def run_form(N, F, seed, begin, count, init=None, strip=None, **knobs):
    """One launch; `strip`: the timeline header must name this form."""
    kw = {"initial_values": list(init)} if init is not None else {}
    with env(**knobs):
        p = benor.TrialsPlan(N, F, seed=seed, k_max=K_MAX, **kw)
        want = benor.BO_KERNEL_W if knobs.get("BENOR_NO_MFMA") else benor.BO_KERNEL_MFMA
        assert p.kernel == want, (p.kernel, knobs)
        h = p.run(begin, count)
    if strip is not None:
        head = [line for line in open(knobs["BENOR_TIMELINE"]) if line.startswith("#")][-1]
        assert f"strip={strip}" in head, head
    return h


def eligible(N, F, min_w=5):
    m = N - F
    return (m - 1) % 32 + 1 <= 16 and (m + 63) // 64 >= min_w


def check_forms(N, F, seed, begin, count, dynamic, init=None):
    ref = oracle_hist(N, F, seed, begin, count, init)
    got = run_form(N, F, seed, begin, count, init, BENOR_MFMA_STRIP="1", BENOR_MFMA_DYNAMIC=dynamic)
    print(f"N={N} F={F} count={count} dynamic={dynamic}: strip {got[got > 0]}, oracle {ref[ref > 0]}")
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got, run_form(N, F, seed, begin, count, init, BENOR_MFMA_STRIP="0", BENOR_MFMA_DYNAMIC=dynamic))
    np.testing.assert_array_equal(got, run_form(N, F, seed, begin, count, init, BENOR_NO_MFMA="1"))
    assert int(got.sum()) - int(got[-1]) == count          # every trial halts; the last bin counts disagreements
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("dynamic", DYNAMIC)
@pytest.mark.parametrize("N,F", SHAPES)
def test_strip_form_random_init(N, F, dynamic):
    check_forms(N, F, 0x57 + N, 7, T, dynamic)


@pytest.mark.gpu
@pytest.mark.parametrize("N,F", SHAPES)
def test_the_form_that_ran(tmp_path, N, F):
    """The launch's timeline header names the form: the strip where the shape is
    eligible and the knob is 1, or W >= 7 and the knob is not set (the
    planner's rule); the 32-row form otherwise."""
    path = str(tmp_path / "tl.csv")
    ref = oracle_hist(N, F, 0x57 + N, 7, T)
    for knob, want in (("1", int(eligible(N, F))), (None, int(eligible(N, F, min_w=7))), ("0", 0)):
        got = run_form(N, F, 0x57 + N, 7, T, strip=want, BENOR_MFMA_STRIP=knob, BENOR_TIMELINE=path)
        np.testing.assert_array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("dynamic", DYNAMIC)
@pytest.mark.parametrize("count", [1, 15, 16, 17, 31, 32, 33])
def test_trial_counts_around_a_half(count, dynamic):
    check_forms(300, 31, 0x58, 3, count, dynamic)
    check_forms(400, 37, 0x58, 3, count, dynamic)


@pytest.mark.gpu
@pytest.mark.parametrize("dynamic", DYNAMIC)
def test_trial_ids_beyond_40_bits(dynamic):
    check_forms(1024, 341, 0x59, (1 << 40) + 5, 4_099, dynamic)
    check_forms(257, 0, 0x59, (1 << 40) + 29, 4_099, dynamic)


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
    for N, F, q in ((257, 0, 0), (300, 31, 0), (400, 37, 0), (1024, 341, 0), (300, 31, 2), (400, 37, 4), (1024, 341, 4)):
        t = (N - F - q) // 2 + 1                           # M1 = m - q binary votes
        for ones in (t - 1, t):
            out.append(pytest.param(N, F, ones, q, id=f"{N}-{F}-q{q}-ones{ones}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dynamic", DYNAMIC)
@pytest.mark.parametrize("N,F,ones,q", fixed_cases())
def test_strip_form_fixed_init_at_the_threshold(N, F, ones, q, dynamic):
    count = 1_003
    got = check_forms(N, F, 5, 0, count, dynamic, init=fixed_init(N, F, ones, q))
    # every trial is the same trial: all decide the majority value in round 1
    t = (N - F - q) // 2 + 1
    assert got[3 + (1 if ones >= t else 0)] == count


@pytest.mark.gpu
@pytest.mark.parametrize("dynamic", DYNAMIC)
def test_six_unsynchronised_launches_on_one_plan(dynamic):
    N, F, seed = 300, 31, 0x5A
    counts = (1, 17, 32, 33, T, 100_000)
    st = torch.cuda.current_stream()

    def launches(strip):
        with env(BENOR_MFMA_STRIP=strip, BENOR_MFMA_DYNAMIC=dynamic):
            p = benor.TrialsPlan(N, F, seed=seed, k_max=K_MAX)
            h = torch.zeros(p.hist_len, dtype=torch.int64, device="cuda")
            begin = 3
            for c in counts:                              # no sync in between
                p.launch(begin, c, h.data_ptr(), st.cuda_stream)
                begin += c
            torch.cuda.synchronize()
            p.check()
            return h.cpu().numpy().astype(np.uint64)

    got = launches("1")
    np.testing.assert_array_equal(got, launches("0"))
    np.testing.assert_array_equal(got, oracle_hist(N, F, seed, 3, sum(counts)))
