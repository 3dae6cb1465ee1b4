"""BO_MODE_CRASH_TALLY, count-level random delivery with crashes during the run (CPU suite).

The definition, restated here in plain Python over
benor.tally_cdf, oracle.philox4x32_10, oracle.coin, oracle.random_init and
tests/test_tally3.py's WordStream / classes / draw3 -- nothing from the kernel;
tests/test_crash_tally_gpu.py checks the kernel against it bit for bit:

* N, F, q = N - F; `faulty` marks the f <= F nodes crashed before the start,
  m0 = N - f initially-live nodes, compact index c by ascending node id over them,
  fixed for the run.  Initial values as in BO_MODE_RANDOM_TALLY3 ("?" allowed).
* Step s = 2 (r - 1) is the R-phase of round r, s = 2 (r - 1) + 1 its P-phase.
* Schedule: explicit, crash_at[i] = node i's step (None / UINT32_MAX: never;
  entries of faulty nodes ignored); or random, per trial from the word stream of
  the Philox blocks {trial_lo, trial_hi, b, 7 << 24}, b = 0, 1, .., below(d) the
  multiply-shift with exact rejection: for j = m0 - crash_count .. m0 - 1,
  t = below(j + 1), the node is compact index t unless already chosen, then j,
  and it crashes at step below(crash_window).
* A node that crashes at step s completed step s - 1; at step s and after it
  neither sends nor receives.  A crash scheduled after the trial halts never
  happens.
* Step s, alive set A_s, m_s = |A_s| >= q: class sizes over A_s (R-phase: the x
  values; P-phase: the proposals of the nodes still alive at the P-step); each
  receiver c in A_s draws (c0, c1) as BO_MODE_RANDOM_TALLY3's draw3 with m = m_s.
  The R and P rules, the coin and sticky `decided` are that mode's.
* Halt after the round in which every alive node has decided, or after k_max
  rounds.  v = the common x of the nodes alive at the end (2 if they differ);
  if no node is alive after a step's crashes the trial ends in bin[2], rounds 0.
* States: alive {0, x, decided, R + 1}; crashed at a step of round r
  {killed, x and decided as of the crash (x may be "?"), k = r}.

The law is checked against a mask-level simulation of the same model written
here with numpy (explicit uniform q-subsets of the alive senders), which shares
nothing with the count-level argument.
"""
import numpy as np
import pytest

import benor
import oracle
import test_tally3 as t3
from test_tally import chi2_two_sample, first, philox
from test_tally3 import Q, WordStream, draw3

M5 = benor.BO_MODE_CRASH_TALLY
STREAM_TALLY, STREAM_SCHEDULE = 5, 7
SEED = t3.SEED
MIB = 1 << 20


# ------------------------------------------------------------ restatement
class ScheduleStream(WordStream):
    """Words of the Philox blocks {trial_lo, trial_hi, b, 7 << 24}, b = 0, 1, ..., in order."""

    def __init__(self, seed, trial):
        super().__init__(seed, trial & 0xFFFFFFFF, trial >> 32, 0, STREAM_SCHEDULE << 24)

    def next(self):
        if self.i % 4 == 0:
            c0, c1, _, c3 = self.ctr
            self.buf = philox(self.seed, (c0, c1, self.i // 4, c3))
        w = self.buf[self.i % 4]
        self.i += 1
        return w


def schedule(seed, trial, live, crash_at=None, crash_count=0, crash_window=0):
    """The trial's crash step per compact index (None: never)."""
    m0 = len(live)
    if crash_at is not None:
        return [None if crash_at[i] in (None, benor.NEVER) else crash_at[i] for i in live]
    sched = [None] * m0
    if crash_count:
        ws = ScheduleStream(seed, trial)
        for j in range(m0 - crash_count, m0):              # Floyd's algorithm
            t = ws.below(j + 1)
            node = t if sched[t] is None else j
            sched[node] = ws.below(crash_window)
    return sched


def crash_trial(N, F, faulty, seed, trial, k_max, initial_values=None, crash_at=None, crash_count=0, crash_window=0):
    """One trial: (histogram bins it increments, rounds, per-node states)."""
    live = [i for i in range(N) if not faulty[i]]
    m0, q = len(live), N - F
    states = [{"killed": True, "x": None, "decided": None, "k": None} if faulty[i] else None for i in range(N)]
    if m0 == 0:
        return [2], 0, states
    sched = schedule(seed, trial, live, crash_at, crash_count, crash_window)
    assert (N - m0) + sum(s is not None for s in sched) <= F
    if initial_values is None:
        x = [oracle.random_init(seed, trial, c, m0) for c in range(m0)]
    else:
        x = [2 if initial_values[i] == Q else initial_values[i] for i in live]
    alive = [True] * m0
    dec = [False] * m0
    tlo, thi = trial & 0xFFFFFFFF, trial >> 32

    def crashes(s, r):
        """The crashes of step s (in round r); the nodes alive after them."""
        for c in range(m0):
            if alive[c] and sched[c] == s:
                alive[c] = False
                states[live[c]] = {"killed": True, "x": Q if x[c] == 2 else x[c], "decided": dec[c], "k": r}
        return [c for c in range(m0) if alive[c]]

    R = 0
    for r in range(1, k_max + 1):
        A = crashes(2 * (r - 1), r)
        if not A:
            return [2], 0, states
        assert len(A) >= q
        blocks = {c: philox(seed, (tlo, thi, c, (r - 1) | STREAM_TALLY << 24)) for c in A}
        K = tuple(sum(x[c] == v for c in A) for v in (0, 1, 2))
        prop = {}
        for c in A:
            b = blocks[c]
            c0, c1 = draw3(len(A), q, K, seed, trial, c, r, 0, b[1] << 32 | b[0])
            prop[c] = 0 if c0 > c1 else 1 if c1 > c0 else 2
        A = crashes(2 * (r - 1) + 1, r)                    # a node that proposed and crashes here does not vote
        if not A:
            return [2], 0, states
        K2 = tuple(sum(prop[c] == v for c in A) for v in (0, 1, 2))
        for c in A:
            b = blocks[c]
            c0, c1 = draw3(len(A), q, K2, seed, trial, c, r, 1, b[3] << 32 | b[2])
            if c0 > F:
                x[c], dec[c] = 0, True
            elif c1 > F:
                x[c], dec[c] = 1, True
            elif c0 != c1:
                x[c] = 1 if c1 > c0 else 0
            else:
                x[c] = oracle.coin(seed, trial, c, r)
        R = r
        if all(dec[c] for c in A):
            break
    A = [c for c in range(m0) if alive[c]]
    ones = sum(x[c] for c in A)
    v = 2 if 0 < ones < len(A) else (1 if ones else 0)
    all_dec = all(dec[c] for c in A)
    bins = [R * 3 + v] if all_dec else [v]
    if all_dec and v == 2:
        bins.append((k_max + 1) * 3)
    for c in A:
        states[live[c]] = {"killed": False, "x": x[c], "decided": dec[c], "k": R + 1}
    return bins, (R if all_dec else 0), states


def crash_hist(N, F, faulty, seed, trial_begin, trial_count, k_max, initial_values=None, **sched):
    h = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    for t in range(trial_begin, trial_begin + trial_count):
        for b in crash_trial(N, F, faulty, seed, t, k_max, initial_values, **sched)[0]:
            h[b] += 1
    return h


def at(N, steps):
    """crash_at of a {node: step} schedule."""
    return [steps.get(i) for i in range(N)]


def table_bytes(m, q):
    """Bytes of u64 thresholds in the table of (m, q)."""
    return 8 * sum(min(K, q) - max(0, q - (m - K)) for K in range(m + 1))


# ------------------------------------------- mask-level simulation (numpy)
def mask_sim_hist(N, F, faulty, k_max, trials, rng, initial_values=None, crash_at=None, crash_count=0,
                  crash_window=0, chunk=10000):
    """The same model at the level of inboxes: at every step each alive receiver
    hears a uniform q-subset of the alive senders (the q smallest of iid uniform
    keys), drawn explicitly; schedules, initial values and coins from `rng`."""
    live = [i for i in range(N) if not faulty[i]]
    m0, q = len(live), N - F
    hist = np.zeros(oracle.hist_len(k_max), dtype=np.uint64)
    never = 1 << 30

    def counts(vals, alive):
        n = len(vals)
        if q == 0:
            return np.zeros((n, m0), dtype=np.int64), np.zeros((n, m0), dtype=np.int64)
        keys = rng.random((n, m0, m0))                      # [trial, receiver, sender]
        keys[np.broadcast_to(~alive[:, None, :], keys.shape)] = 2.0
        inbox = np.argpartition(keys, q - 1, axis=2)[:, :, :q]
        heard = np.take_along_axis(np.broadcast_to(vals[:, None, :], keys.shape), inbox, axis=2)
        return (heard == 0).sum(axis=2), (heard == 1).sum(axis=2)

    def finish(x, alive, dec, R):
        """Bins of halted (or timed-out) trials."""
        n_alive = alive.sum(axis=1)
        ones = ((x == 1) & alive).sum(axis=1)
        v = np.where((ones > 0) & (ones < n_alive), 2, np.where(ones > 0, 1, 0))
        all_dec = (dec | ~alive).all(axis=1)
        np.add.at(hist, np.where(all_dec, R * 3 + v, v), 1)
        hist[-1] += int((all_dec & (v == 2)).sum())

    for lo in range(0, trials, chunk):
        n = min(chunk, trials - lo)
        if initial_values is None:
            x = rng.integers(0, 2, size=(n, m0)).astype(np.int8)
        else:
            x = np.tile(np.array([2 if initial_values[i] == Q else initial_values[i] for i in live], dtype=np.int8), (n, 1))
        sched = np.full((n, m0), never, dtype=np.int64)
        if crash_at is not None:
            sched[:] = [never if crash_at[i] in (None, benor.NEVER) else crash_at[i] for i in live]
        elif crash_count:
            who = np.argsort(rng.random((n, m0)), axis=1)[:, :crash_count]
            np.put_along_axis(sched, who, rng.integers(0, crash_window, size=(n, crash_count)), axis=1)
        alive = np.ones((n, m0), dtype=bool)
        dec = np.zeros((n, m0), dtype=bool)
        if m0 == 0:
            hist[2] += n
            continue
        for r in range(1, k_max + 1):
            alive &= sched > 2 * (r - 1)
            gone = ~alive.any(axis=1)
            c0, c1 = counts(x, alive)
            prop = np.where(c0 > c1, 0, np.where(c1 > c0, 1, 2)).astype(np.int8)
            alive &= sched > 2 * (r - 1) + 1
            gone |= ~alive.any(axis=1)
            c0, c1 = counts(prop, alive)
            coin = rng.integers(0, 2, size=(len(x), m0))
            new = np.where(c0 > F, 0, np.where(c1 > F, 1, np.where(c1 > c0, 1, np.where(c0 > c1, 0, coin))))
            x = np.where(alive, new, x).astype(np.int8)
            dec |= alive & ((c0 > F) | (c1 > F))
            hist[2] += int(gone.sum())                      # nobody left: bin[2]
            halted = (dec | ~alive).all(axis=1) & ~gone
            if r == k_max:
                halted = ~gone
            finish(x[halted], alive[halted], dec[halted], r)
            keep = ~halted & ~gone
            x, alive, dec, sched = x[keep], alive[keep], dec[keep], sched[keep]
            if not len(x):
                break
    return hist


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("N,F,f", [(10, 4, 0), (11, 4, 2), (69, 24, 5)])
def test_unreached_schedule_equals_mode_4(N, F, f):
    faulty, k_max = first(f, N), 16
    sched = at(N, {f: 2 * k_max, N - 1: 2 * k_max + 7}) if F - f >= 2 else at(N, {N - 1: 2 * k_max})
    for t in range(200):
        assert crash_trial(N, F, faulty, SEED, t, k_max, crash_at=sched) == t3.tally3_trial(N, F, faulty, SEED, t, k_max), t
    assert crash_trial(N, F, faulty, SEED, 5, k_max) == t3.tally3_trial(N, F, faulty, SEED, 5, k_max)   # empty schedule


def test_random_schedule():
    N, f = 12, 2
    live = [i for i in range(N) if i >= f]
    seen = set()
    for trial in list(range(300)) + [(1 << 32) + 5]:
        s = schedule(SEED, trial, live, crash_count=3, crash_window=6)
        assert len(s) == N - f and sum(v is not None for v in s) == 3
        assert all(v is None or 0 <= v < 6 for v in s)
        assert s == schedule(SEED, trial, live, crash_count=3, crash_window=6)
        seen.add(tuple(s))
    assert len(seen) > 200                                  # a schedule per trial
    assert schedule(SEED + 1, 0, live, crash_count=3, crash_window=6) != schedule(SEED, 0, live, crash_count=3, crash_window=6) \
        or schedule(SEED + 1, 1, live, crash_count=3, crash_window=6) != schedule(SEED, 1, live, crash_count=3, crash_window=6)
    # every node crashes: Floyd's last step always finds its t or takes j
    assert all(v is not None for v in schedule(SEED, 3, live, crash_count=N - f, crash_window=1))
    # every initially-live node is drawn about equally often, every step too
    hits, steps = [0] * (N - f), [0] * 6
    for trial in range(3000):
        for c, v in enumerate(schedule(SEED, trial, live, crash_count=3, crash_window=6)):
            if v is not None:
                hits[c] += 1
                steps[v] += 1
    assert all(abs(h - 900) < 5 * 25.1 for h in hits), hits            # Binomial(3000, 0.3): sd 25.1
    assert all(abs(s - 1500) < 5 * 35.4 for s in steps), steps         # Binomial(9000, 1/6): sd 35.4


def test_states_of_crashed_nodes():
    N, F, k_max = 12, 4, 16
    init = [Q, 1, 0, Q, 1, 1, 0, 0, 1, 0, 1, 0]
    faulty = first(0, N)
    # node 0 ("?") crashes at step 0, node 4 at the P-step of round 1, node 7 at the R-step of round 2
    sched = at(N, {0: 0, 4: 1, 7: 2})
    some_round_2 = False
    for t in range(50):
        bins, rounds, st = crash_trial(N, F, faulty, SEED, t, k_max, init, crash_at=sched)
        assert st[0] == {"killed": True, "x": Q, "decided": False, "k": 1}
        assert st[4] == {"killed": True, "x": 1, "decided": False, "k": 1}      # it proposed, it did not vote
        if st[7]["killed"]:
            some_round_2 = True
            assert st[7]["k"] == 2 and st[7]["x"] in (0, 1)
        else:                                               # the trial halted in round 1: that crash never happened
            assert rounds == 1 and st[7]["k"] == 2
        assert all(not s["killed"] for i, s in enumerate(st) if i not in (0, 4, 7))
    assert some_round_2
    # a node crashed after deciding keeps decided = 1: all ones decides in round 1, k_max rounds go on
    # only while somebody is undecided -- so crash a decided node of a trial that runs on
    N, F = 10, 4
    found = False
    for t in range(400):
        _, _, base = crash_trial(N, F, first(0, N), SEED, t, 1)
        decided = [i for i, s in enumerate(base) if s["decided"]]
        if decided and len(decided) < N:                    # round 1 leaves some decided, some not
            _, _, st = crash_trial(N, F, first(0, N), SEED, t, k_max, crash_at=at(N, {decided[0]: 2}))
            assert st[decided[0]] == {"killed": True, "x": base[decided[0]]["x"], "decided": True, "k": 2}
            found = True
            break
    assert found


def test_validation_and_kernel_choice():
    assert M5 == 5 and benor.BO_KERNEL_TALLY_CRASH == 11 and benor.BO_KERNEL_TALLY_CRASH in benor.KERNEL_NAMES
    N, F = 10, 4
    none = first(0, N)
    with pytest.raises(benor.Error):                        # f + crashes > F: error 2
        benor.kernel_for(N, F, first(2, N), mode=M5, crash_count=3, crash_window=6)
    with pytest.raises(benor.Error):
        benor.kernel_for(N, F, first(1, N), mode=M5, crash_at=at(N, {1: 0, 2: 1, 3: 2, 4: 99}))
    assert benor.kernel_for(N, F, first(2, N), mode=M5, crash_count=2, crash_window=6) == benor.BO_KERNEL_TALLY_CRASH
    # entries of initially-faulty nodes are ignored
    assert benor.kernel_for(N, F, first(1, N), mode=M5, crash_at=at(N, {0: 0, 1: 0, 2: 1, 3: 2})) == benor.BO_KERNEL_TALLY_CRASH
    with pytest.raises(RuntimeError, match="libbenor error 3.*crash_window"):
        benor.kernel_for(N, F, none, mode=M5, crash_count=3, crash_window=0)
    with pytest.raises(benor.Error) as e5:                  # everything else: BO_MODE_RANDOM_DELIVERY's validation
        benor.kernel_for(N, F, first(5, N), mode=M5)
    with pytest.raises(benor.Error) as e1:
        benor.kernel_for(N, F, first(5, N), mode=benor.BO_MODE_RANDOM_DELIVERY)
    assert str(e5.value) == str(e1.value)
    # an empty schedule is mode 4's plan, and mode 4 folds into mode 3 inside that mode's scope
    assert benor.kernel_for(N, F, none, mode=M5) == benor.BO_KERNEL_TALLY3
    assert benor.kernel_for(N, F, none, mode=M5, crash_at=at(N, {})) == benor.BO_KERNEL_TALLY3
    assert benor.kernel_for(N, F, first(1, N), mode=M5, crash_at=at(N, {0: 3})) == benor.BO_KERNEL_TALLY3
    assert benor.kernel_for(11, 4, first(0, 11), mode=M5) == benor.BO_KERNEL_TALLY
    assert benor.kernel_for(11, 4, first(0, 11), mode=M5, crash_window=6) == benor.BO_KERNEL_TALLY
    # a non-empty one runs the crash kernel, reached or not, odd quorum or even
    assert benor.kernel_for(N, F, none, mode=M5, crash_count=3, crash_window=6) == benor.BO_KERNEL_TALLY_CRASH
    assert benor.kernel_for(N, F, none, mode=M5, crash_at=at(N, {3: 10 ** 6})) == benor.BO_KERNEL_TALLY_CRASH
    assert benor.kernel_for(11, 4, first(0, 11), mode=M5, crash_at=at(11, {3: 1})) == benor.BO_KERNEL_TALLY_CRASH
    assert benor.kernel_for(1024, 392, first(0, 1024), mode=M5, crash_count=392, crash_window=6) == benor.BO_KERNEL_TALLY_CRASH
    assert benor.kernel_for(3, 3, first(3, 3), mode=M5) == benor.BO_KERNEL_NONE       # m0 = 0
    # the other modes ignore the schedule fields as before
    assert benor.kernel_for(N, F, none, mode=benor.BO_MODE_RANDOM_TALLY3, crash_count=3, crash_window=6) == benor.BO_KERNEL_TALLY3


def test_table_limit():
    """One table per reachable live count, 512 MiB of thresholds at most."""
    limit = 512 * MIB
    N, F = 4096, 1366
    q = N - F
    t16 = sum(table_bytes(N - j, q) for j in range(17))
    t32 = sum(table_bytes(N - j, q) for j in range(33))
    assert t16 == 8 * q * sum(F - j for j in range(17))     # a table of (m', q) holds q (m' - q) thresholds
    assert 480 * MIB < t16 <= limit < t32, (t16 / MIB, t32 / MIB)
    none = first(0, N)
    assert benor.kernel_for(N, F, none, mode=M5, crash_count=16, crash_window=4) == benor.BO_KERNEL_TALLY_CRASH
    with pytest.raises(RuntimeError, match="libbenor error 7.*512 MiB"):
        benor.kernel_for(N, F, none, mode=M5, crash_count=32, crash_window=4)
    # an explicit schedule needs the counts after each distinct step only: 32 crashes at two steps fit
    two_steps = at(N, {i: i % 2 for i in range(32)})
    assert benor.kernel_for(N, F, none, mode=M5, crash_at=two_steps) == benor.BO_KERNEL_TALLY_CRASH
    # N = 1024, F = 392 fits at any schedule: every live count 1024 .. 632 is 371.4 MiB
    full = sum(table_bytes(1024 - j, 1024 - 392) for j in range(393))
    assert 371 * MIB < full <= 372 * MIB
    assert benor.kernel_for(1024, 392, first(0, 1024), mode=M5, crash_count=392, crash_window=6) == benor.BO_KERNEL_TALLY_CRASH
    # ... but not every F does: at F = 600 a random schedule of all 600 crashes needs 583 MiB
    assert sum(table_bytes(1024 - j, 424) for j in range(601)) > limit
    with pytest.raises(RuntimeError, match="libbenor error 7.*512 MiB"):
        benor.kernel_for(1024, 600, first(0, 1024), mode=M5, crash_count=600, crash_window=6)


LAW_SHAPES = {
    "steps-1-2-3": dict(N=10, F=4, f=0, init=None, sched=dict(crash_at=at(10, {2: 1, 5: 2, 9: 3}))),
    "random-3-of-6": dict(N=10, F=4, f=1, init=None, sched=dict(crash_count=3, crash_window=6)),
    "question-marks": dict(N=12, F=4, f=0, init=[Q, 1, 0, 1, Q, 0, 1, 0, 1, 0, 1, 0],
                           sched=dict(crash_at=at(12, {0: 0, 6: 1}))),
}


@pytest.mark.parametrize("name", sorted(LAW_SHAPES))
def test_law_matches_mask_level_simulation(name):
    """The restatement's histogram against the mask-level simulation, 2 * 10^4
    trials a side, k_max 16: two-sample chi^2 over bins pooled to >= 20,
    p > 10^-3 at fixed seeds."""
    s = LAW_SHAPES[name]
    N, F, T, k_max = s["N"], s["F"], 20000, 16
    faulty = first(s["f"], N)
    ref = mask_sim_hist(N, F, faulty, k_max, T, np.random.default_rng(SEED + 1), s["init"], **s["sched"])
    got = crash_hist(N, F, faulty, SEED, 0, T, k_max, s["init"], **s["sched"])
    assert int(got[:-1].sum()) == T == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"{name}: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}, agreement violations {int(got[-1])} / {int(ref[-1])}")
    assert p > 1e-3, (p, stat, df)


def test_all_crashes_at_step_0_has_the_law_of_mode_4_with_those_nodes_faulty():
    N, F, T, k_max = 10, 4, 20000, 16
    got = crash_hist(N, F, first(1, N), SEED, 0, T, k_max, crash_at=at(N, {3: 0, 8: 0}))
    ref = t3.tally3_hist(N, F, [i in (0, 3, 8) for i in range(N)], SEED + 1, 0, T, k_max)
    assert int(got[:-1].sum()) == T == int(ref[:-1].sum())
    p, stat, df = chi2_two_sample(got, ref)
    print(f"step-0 crashes against mode 4: chi^2 = {stat:.2f}, df = {df}, p = {p:.4f}")
    assert p > 1e-3, (p, stat, df)


def test_once_the_live_count_is_the_quorum_the_run_is_lockstep():
    """f + crashes = F, all at step 0: m_s = q from the first step, every receiver
    hears every alive sender.  With the crashed nodes the last ones the survivors
    keep mode 4's compact indices (and coins), so the trial is mode 4's with
    those nodes faulty -- which at f = F is the lockstep trial."""
    N, F, k_max = 10, 4, 16
    init = [1, 0, 1, 0, 0, 1, Q, 0, 1, 1]
    sched = at(N, {7: 0, 8: 0, 9: 0})
    for t in range(100):
        bins, rounds, st = crash_trial(N, F, first(1, N), SEED, t, k_max, init, crash_at=sched)
        ref = t3.tally3_trial(N, F, [i in (0, 7, 8, 9) for i in range(N)], SEED, t, k_max, init)
        assert (bins, rounds) == ref[:2], t
        assert st[1:7] == ref[2][1:7], t
