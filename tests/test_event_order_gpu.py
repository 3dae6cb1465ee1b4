"""The order-sensitive cases of tests/test_event_order.py on the device: per-node states against oracle (iii), bit
for bit, on every form the code can route a case to.

A freeze stops every live node before delivery e, so the final states are the network's states at e: which nodes
have finished the round is decided by the exact delivery order (a wrong pick, swap-remove, conflict cut or undo
shows).  Every form's loop ends on a network with no running node, read off the code: the lane-per-trial kernel
(`dead`, benor_kernels.hip), the wave-per-trial kernel and the workgroup kernel's control wave (`!__any(alive)`),
the one-wave LDS kernel and the register kernel (`killed == all`) each set halted = 3 right after the stops of a
delivery index are applied, before anything else of that index; so the freezes here stop every live node.

Routes of one case (forms_of): the default batch route (one lane per trial up to N = 256, one wave per trial
above); BENOR_EVENT_FORM=wg (the register kernel up to N = 16, the one-wave LDS kernel up to 64, the workgroup
kernel above) and the same with BENOR_LIVE_WAVES = 1, 3, 7, 15 (the workgroup kernel at every N, pool in LDS up to
N = 78); BENOR_EVENT_FORM=wave for N <= 64; and Network.start(stop_after=...), which runs the live-run kernels with
no mailbox traffic, on trial 0 of the seed.  The form that ran: the knobs are set and plan.kernel is the event
family on the batch routes; on the network route the BENOR_EVENT_STATS line tells the three live-run kernels apart
(test_the_network_route_runs_the_form_it_names).

The stats line carries no counter per rare path of the workgroup kernel (a cut by a second forwarding level, a cut
by a third picker, adds undone behind the earliest trigger): `conflict_cut` counts batches cut for either of the
first two reasons and `cross_batches` the batches in which a slot reached its quorum.  None was added to the
kernel; the paths are covered by count: every case runs with 15 event waves too, where a batch of up to 960 picks
from a pool of a few thousand words collides in nearly every batch (test_forced_fifteen_waves_cut_and_undo asserts
the two counters that exist).
"""
import json

import numpy as np
import pytest
import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

import benor
import oracle
import test_event_order as gen

pytestmark = pytest.mark.gpu

EVENT = benor.BO_MODE_EVENT
KNOBS = ("BENOR_EVENT_FORM", "BENOR_LIVE_WAVES", "BENOR_EVENT_STATS")


def route_env(monkeypatch, route, waves, stats=None):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    if route in ("wg", "wave"):
        monkeypatch.setenv("BENOR_EVENT_FORM", route)
    if waves:
        monkeypatch.setenv("BENOR_LIVE_WAVES", str(waves))
    if stats:
        monkeypatch.setenv("BENOR_EVENT_STATS", str(stats))


def network_states(c):
    """Network.start with the case's schedule: trial 0 of the seed, the start given as fixed values."""
    init = gen.drawn_start(c)
    net = benor.Network(c.N, c.F, init, c.faulty)
    net.start(seed=c.seed, k_max=c.k_max, stop_after=c.sched["crash_at"])
    return net.get_states(), gen.expected(c, trial=0, init=init)


def differing(got, want):
    return [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w][:4]


def check_states(monkeypatch, c):
    want = gen.expected(c)
    ran = []
    for route, waves in gen.forms_of(c):
        route_env(monkeypatch, route, waves)
        if route == "net":
            got, ref = network_states(c)
        else:
            assert benor.kernel_for(c.N, c.F, c.faulty, mode=EVENT, **c.kw()) == benor.BO_KERNEL_EVENT
            _, got = benor.run_trial_states(c.N, c.F, c.faulty, trial=c.trial, mode=EVENT, **c.kw())
            ref = want
        assert got == ref, (str(c), route, waves, gen.form(c.N, c.m, route, waves, c.rstops), differing(got, ref))
        ran.append(gen.form(c.N, c.m, route, waves, c.rstops))
    return ran


@pytest.mark.parametrize("i", gen.all_cases())
def test_states_on_every_form(monkeypatch, i):
    c = gen.case(i)
    ran = check_states(monkeypatch, c)
    assert {f[0] for f in ran} >= {"wg", "big" if c.N > gen.LANE_MAX else "lane"}
    assert {f[1] for f in ran if f[0] == "wg"} >= {1, 3, 7, 15}


@pytest.mark.parametrize("j", gen.table_cases())
def test_states_at_every_hash_table_size(monkeypatch, j):
    """The workgroup kernel at W = 15 with 8, 4 and 2 hash slots per event lane; the last at N = 4096 with the
    largest random schedule whose keys fit the device's LDS (one stop more is refused when the plan is made:
    tests/test_event_order.py)."""
    c = gen.table_case(j)
    ran = check_states(monkeypatch, c)
    assert ("wg", 15, False, (8, 4, 2)[j]) in ran and (j == 0 or len(ran) == 1)   # (the two large ones: that route alone)


@pytest.mark.parametrize("j", gen.hist_cases())
def test_histograms_on_a_callers_stream(monkeypatch, j):
    """Kinds d and e, some hundred trials, on the batch kernel and under BENOR_EVENT_FORM=wg: two launches on a
    caller's stream into a histogram that already holds a pattern (bo_plan_launch adds)."""
    c = gen.hist_case(j)
    kw = c.kw()
    ref, _ = oracle.event_trials(c.N, c.F, c.faulty, seed=kw.pop("seed"), trial_begin=c.trial, trial_count=c.trials,
                                 k_max=kw.pop("k_max"), initial_values=kw.pop("initial_values"), **kw)
    for route in ("batch", "wg"):
        route_env(monkeypatch, route, 0)
        plan = benor.TrialsPlan(c.N, c.F, c.faulty, mode=EVENT, **c.kw())
        assert plan.kernel == benor.BO_KERNEL_EVENT
        stream = torch.cuda.Stream()
        pattern = torch.arange(plan.hist_len, dtype=torch.int64, device="cuda") * 7 + 3
        hist = pattern.clone()
        stream.wait_stream(torch.cuda.current_stream())
        first = c.trials // 3
        plan.launch(c.trial, first, hist.data_ptr(), stream.cuda_stream)
        plan.launch(c.trial + first, c.trials - first, hist.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        plan.check()
        got = (hist - pattern).cpu().numpy().astype(np.uint64)
        np.testing.assert_array_equal(got, ref.hist, err_msg=f"{c} {route}")
    assert int(ref.hist.sum()) == c.trials


def stats_line(path):
    lines = [json.loads(line) for line in open(path)]
    assert len(lines) == 1
    return lines[0]


@pytest.mark.parametrize("i", [i for i in gen.all_cases() if "crash_at" in gen.case(i).sched and gen.case(i).e][::2])
def test_the_network_route_runs_the_form_it_names(monkeypatch, tmp_path, i):
    """The BENOR_EVENT_STATS line of a network start (the stats instantiation of the same kernels): the register
    kernel counts one batch per trigger and stamps no loop head, the one-wave LDS kernel stamps its loop head and
    counts no batch slots, the workgroup kernel counts its batches' slots, at most 64 per event wave and batch."""
    c = gen.case(i)
    path = tmp_path / "stats.jsonl"
    route_env(monkeypatch, "net", 0, stats=path)
    got, ref = network_states(c)
    assert got == ref, (str(c), differing(got, ref))
    s = stats_line(path)
    f = gen.form(c.N, c.m, "net")
    assert (s["N"], s["F"]) == (c.N, c.F)
    if f[0] == "reg":
        assert s["batch_slots"] == 0 and s["cyc_top"] == 0 and s["batches"] == s["trigger_batches"], (f, s)
    elif f[0] == "wave":
        assert s["batch_slots"] == 0 and s["cyc_top"] > 0 and s["batches"] > 0, (f, s)
    else:
        assert 0 < s["events"] <= s["batch_slots"] <= 64 * f[1] * s["batches"], (f, s)
    if c.kind == "d":
        assert s["events"] >= c.e                  # the half that was not stopped runs on until the pool is empty
    else:
        assert s["events"] <= c.e                  # a freeze: the run ends before delivery e (trial 0 may end sooner)


@pytest.mark.parametrize("i", [i for i in gen.all_cases() if gen.case(i).kind in "ab" and gen.case(i).N <= gen.WAVE_MAX])
def test_forced_fifteen_waves_cut_and_undo(monkeypatch, tmp_path, i):
    """Small N with 15 event waves: batches of up to 960 picks from a pool of at most 4 N^2 words.  The counters
    that exist show the batches cut at a pick conflict and the batches in which a slot reached its quorum (the
    batch ends after the earliest such event, later adds undone)."""
    c = gen.case(i)
    path = tmp_path / "stats.jsonl"
    route_env(monkeypatch, "net", 15, stats=path)
    got, ref = network_states(c)
    assert got == ref, (str(c), differing(got, ref))
    s = stats_line(path)
    assert s["conflict_cut"] > 0 and s["cross_batches"] > 0 and s["events"] < s["batch_slots"], s
