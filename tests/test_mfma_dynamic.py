"""The KIND 0 matrix-core kernel's dynamic form (csrc/benor_mfma.h, DYN): the
waves claim chunks of 32-trial groups from two plan-owned words instead of
striding over them (csrc/benor_mfma_sched.h).

CPU: tests/mfma_sched_check.cpp, a host program over that header, runs the
claim-and-reset protocol on 64 std::atomic threads and checks the planner's
rule; both knobs are registered.
GPU: BENOR_MFMA_DYNAMIC=1 forces the dynamic form on shapes the rule would run
statically (they are far too short to pay).  Its histogram against the oracle,
the static form (=0) and the popcount kernel; many chunks per wave at chunk
sizes 1, 3 and 16; launches of 1 .. 100,000 trials back to back on one plan and
stream with no sync between them (the words reset themselves) and
plan.check(); trial ids beyond 2^32; and the timeline diagnostic, which shows
that the forced form is the one that ran and that its claims add up.
"""
import contextlib
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ben-or-consensus-algorithm_amd", "csrc")
T = 20_011
K_MAX = 8
KNOBS = ("BENOR_MFMA_DYNAMIC", "BENOR_MFMA_CHUNK", "BENOR_MFMA_PAIR", "BENOR_NO_MFMA", "BENOR_BLOCKS_PER_CU",
         "BENOR_TIMELINE")


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
def test_knobs_are_registered():
    assert benor.KNOBS["BENOR_MFMA_DYNAMIC"] == "validation"
    assert benor.KNOBS["BENOR_MFMA_CHUNK"] == "tuning"


def test_claim_protocol_and_planner_rule_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "mfma_sched_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", CSRC,
                    os.path.join(ROOT, "tests", "mfma_sched_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[0].isdigit() and int(r.stdout.split()[0]) >= 292 and " 0 failures" in r.stdout, r.stdout


# ------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def oracle_hist(N, F, seed, begin, count):
    h = oracle.run_trials(N, F, first_f(N, F), seed=seed, trial_begin=begin, trial_count=count, k_max=K_MAX).hist
    h.setflags(write=False)
    return h


def run_form(N, F, seed, begin, count, **knobs):
    with env(**knobs):
        p = benor.TrialsPlan(N, F, seed=seed, k_max=K_MAX)
        want = benor.BO_KERNEL_W if knobs.get("BENOR_NO_MFMA") else benor.BO_KERNEL_MFMA
        assert p.kernel == want, (p.kernel, knobs)
        return p.run(begin, count)


@pytest.mark.gpu
@pytest.mark.parametrize("N,F", [(97, 32), (1000, 333), (1024, 341)])
def test_dynamic_form_equals_oracle_static_and_popcount(N, F):
    """626 groups, the last one partial, on thousands of waves: most claim nothing."""
    seed = 0xD0 + N
    ref = oracle_hist(N, F, seed, 7, T)
    dyn = run_form(N, F, seed, 7, T, BENOR_MFMA_DYNAMIC="1")
    print(f"N={N} F={F}: dynamic {dyn[dyn > 0]}, oracle {ref[ref > 0]}")
    np.testing.assert_array_equal(dyn, ref)
    np.testing.assert_array_equal(dyn, run_form(N, F, seed, 7, T, BENOR_MFMA_DYNAMIC="0"))
    np.testing.assert_array_equal(dyn, run_form(N, F, seed, 7, T, BENOR_NO_MFMA="1"))
    assert int(dyn.sum()) - int(dyn[-1]) == T


@functools.lru_cache(maxsize=None)
def static_many():
    h = run_form(97, 32, 0xD1, 11, 3_000_001, BENOR_MFMA_DYNAMIC="0")
    h.setflags(write=False)
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ["1", "3", "16"])
def test_many_chunks_per_wave(chunk):
    """93,751 groups: more than 8192 waves x 8, so waves claim again and again."""
    dyn = run_form(97, 32, 0xD1, 11, 3_000_001, BENOR_MFMA_DYNAMIC="1", BENOR_MFMA_CHUNK=chunk)
    np.testing.assert_array_equal(dyn, static_many())
    assert int(dyn.sum()) - int(dyn[-1]) == 3_000_001


@pytest.mark.gpu
def test_reuse_and_reset_on_one_plan_and_stream():
    N, F, seed = 97, 32, 0xD2
    counts = (1, 31, 32, 33, T, 100_000)
    st = torch.cuda.current_stream()

    def launches(dynamic, times):
        with env(BENOR_MFMA_DYNAMIC=dynamic):
            p = benor.TrialsPlan(N, F, seed=seed, k_max=K_MAX)
            out = []
            for _ in range(times):
                h = torch.zeros(p.hist_len, dtype=torch.int64, device="cuda")
                begin = 3
                for c in counts:                      # no sync in between: the words reset themselves
                    p.launch(begin, c, h.data_ptr(), st.cuda_stream)
                    begin += c
                torch.cuda.synchronize()
                p.check()
                out.append(h.cpu().numpy().astype(np.uint64))
            return out

    first, again = launches("1", 2)
    np.testing.assert_array_equal(first, launches("0", 1)[0])
    np.testing.assert_array_equal(first, oracle_hist(N, F, seed, 3, sum(counts)))
    np.testing.assert_array_equal(first, again)


@pytest.mark.gpu
def test_trial_ids_beyond_32_bits():
    N, F, seed, begin, count = 1024, 341, 0xD3, (1 << 40) + 5, 4_099
    dyn = run_form(N, F, seed, begin, count, BENOR_MFMA_DYNAMIC="1")
    np.testing.assert_array_equal(dyn, oracle_hist(N, F, seed, begin, count))


def timeline_rows(path):
    head, rows = None, []
    for line in open(path):
        if line.startswith("#"):
            head, rows = line, []
        elif line.strip():
            rows.append([int(x) for x in line.split(",")])
    return head, rows


@pytest.mark.gpu
@pytest.mark.parametrize("dynamic,chunk", [("1", 3), ("0", 0)])
def test_timeline_shows_the_form_that_ran(tmp_path, dynamic, chunk):
    """The last launch's slots: the header names the chunk (0: static), the
    waves' group counts add up to the launch's groups, and the dynamic form
    made one claim per chunk (the failing claims are not counted)."""
    path = tmp_path / "tl.csv"
    knobs = {"BENOR_MFMA_CHUNK": str(chunk)} if chunk else {}
    got = run_form(97, 32, 0xD4, 0, T, BENOR_MFMA_DYNAMIC=dynamic, BENOR_TIMELINE=str(path), **knobs)
    np.testing.assert_array_equal(got, run_form(97, 32, 0xD4, 0, T, BENOR_MFMA_DYNAMIC="0"))
    head, rows = timeline_rows(path)
    groups = (T + 31) // 32
    assert f"kernel=mfma chunk={chunk}" in head, head
    assert sum(r[3] for r in rows) == groups
    assert sum(r[8] for r in rows) == (-(-groups // chunk) if chunk else 0)
    ran = [r for r in rows if r[3]]
    assert all(r[2] >= r[1] > 0 for r in ran)                       # end stamp behind the entry stamp
    assert all(r[4] < 8 for r in rows)                              # XCC ids of an 8-XCD device
