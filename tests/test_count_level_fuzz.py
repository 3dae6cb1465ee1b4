"""Seeded differential fuzz of the count-level family: the generator, and what can be checked without a device.

case(family, i) builds one configuration of modes 3 to 13, of the threshold rules or of the class-level chain from
np.random.default_rng(BASE[family] + i) and nothing else: the keyword arguments of benor.TrialsPlan /
benor.run_trial_states (benor.LumpedPlan at the class level), the matching plain-Python restatement from the test
module where it lives, and a trial range.  tests/test_count_level_fuzz_gpu.py runs every case on the device; here:

* every case passes the host's validation (benor.kernel_for, benor.LumpedPlan: no device) and plans the kernel that
  the mode or its documented demotion names; nothing is skipped or caught: the share left out is asserted to be 0;
* every edge class of EDGE_CLASSES occurs in at least three cases of every family it applies to.  A class is read
  off the finished configuration, not off the generator's intent;
* the restatements of generated configurations agree with each other through the model's identities
  (test_identity_*): the independent evidence that the references are right where the fuzz leans on them;
* the directed rare-word constants of the GPU file (tools/find_rare_words.py found them) have the property they
  were kept for: a rejected word of stream 6 or 7, and a result that a draw without the rejection would change.

Trials per case, by the live count m (the band's count, divided by FACTOR for the modes whose draws are the lane's
own, and at most what 6 * 10^6 walk words allow: trials_for).  Restated on one core of the build machine; the seconds are
the slowest of a band's cases over all families:

    m           trials   seconds
    <= 64         60      0.6
    <= 300        12      1.1   (rule case 10: 200 nodes, 3 trials)
    <= 1100        2      0.3
    above          1      14    (byz case 7, N = 4096: one trial is the floor; mode 4: 2.0, mode 7: 11, rule: 9.1)
    class level  200      0.3

All 216 cases restate in 71 s.  k_max comes from {1, 2, 3, 16, 40}, above 300 live nodes without 40 and above 1100
without 16 (round_cap): one such trial that does not decide restates in minutes.
"""
import contextlib
import dataclasses

import numpy as np
import pytest

import benor
import oracle
import test_byz_coin as coin_model
import test_byz_heard as heard_model
import test_byz_rule_b as mode9
import test_byz_sched as sched_model
import test_byz_tally as mode8
import test_crash_partial as mode6
import test_crash_subset as mode7
import test_crash_tally as mode5
import test_lumped as lumped_model
import test_rule as rule_model
import test_tally as mode3
import test_tally3 as mode4

Q = "?"
ALL, HALF, QUARTER = 0xFFFFFFFF, 1 << 31, 1 << 30
RANDOM, OPPOSE, BALANCE, SPLIT = 0, 1, 3, 4
SEED = mode3.SEED
MIB = 1 << 20

FAMILIES = ("mode3", "mode4", "mode5", "mode6", "mode7", "byz", "sched", "rule", "lumped")
CRASH, BYZ = ("mode5", "mode6", "mode7"), ("byz", "sched", "rule")
CASES = 24                                        # per family, on the device
# the first seed of a family: chosen (tools/find_rare_words.py bases) so that its first CASES cases hold
# every edge class three times and no more than three cases of over 1100 live nodes.  The generator forces each class with a fixed probability, which alone does not
# promise three of 24: after a change of CASES or of the generator, run `bases` again and paste what it prints
BASE = {"mode3": 30119, "mode4": 40018, "mode5": 50118, "mode6": 60008, "mode7": 70140, "byz": 80066,
        "sched": 120012, "rule": 130016, "lumped": 140000}
TABLE_CAP = 96 * MIB                              # a crash-family case's threshold tables: a quick plan (the host allows 512 MiB)
FACTOR = {"mode6": 2, "mode7": 3, "byz": 3, "rule": 3}

NODE_CLASSES = ("m=q", "m<=32", "m in 64,65,128,129", "N=4096", "f=0", "k_max=1", "all ?", "tied")
CRASH_CLASSES = ("all on step 0", "margin emptied", "wholly beyond 2 k_max")
BYZ_CLASSES = ("b=0", "b=F-f", "group without honest lane", "group of one lane")
LUMPED_CLASSES = ("m=q", "f=0", "k_max=1", "all ?", "tied", "b=0", "b=F-f", "N=2^24")
EDGE_CLASSES = {fam: NODE_CLASSES for fam in ("mode3", "mode4")}
EDGE_CLASSES["mode3"] = tuple(c for c in NODE_CLASSES if c != "all ?")        # mode 3 takes no "?"
EDGE_CLASSES.update({fam: NODE_CLASSES + CRASH_CLASSES for fam in CRASH})
EDGE_CLASSES.update({fam: NODE_CLASSES + BYZ_CLASSES for fam in BYZ})
EDGE_CLASSES["lumped"] = LUMPED_CLASSES


@dataclasses.dataclass
class Case:
    family: str
    i: int
    level: str                                    # "node": TrialsPlan / run_trial_states; "class": LumpedPlan
    kw: dict                                      # the plan's arguments, N and F (and faulty) among them
    restate: object                               # trial -> the restatement's result
    begin: int
    trials: int
    classes: frozenset
    kernel: int                                   # BO_KERNEL_* the host must plan (node level)

    def __str__(self):
        kw = dict(self.kw)
        for name in ("faulty", "byzantine"):
            if kw.get(name) is not None:
                kw[name] = [i for i, v in enumerate(kw[name]) if v]
        if kw.get("crash_at") is not None:
            kw["crash_at"] = {i: v for i, v in enumerate(kw["crash_at"]) if v is not None}
        if kw.get("initial_values") is not None and len(kw["initial_values"]) > 3:
            kw["initial_values"] = "".join(str(v) for v in kw["initial_values"])
        return (f"case({self.family!r}, {self.i}) trials [{self.begin}, +{self.trials}) kernel {self.kernel} "
                f"classes {sorted(self.classes)} {kw}")

    def plan(self):
        kw = dict(self.kw)
        if self.level == "class":
            return benor.LumpedPlan(kw.pop("N"), kw.pop("F"), **kw)
        return benor.TrialsPlan(kw.pop("N"), kw.pop("F"), kw.pop("faulty"), **kw)

    def states(self, trial):
        """(rounds, states) of one trial on the device, in the restatement's form."""
        if self.level == "class":
            st = self.plan().trial(trial)
            return st["rounds"], (st["a"], st["dec"])
        kw = dict(self.kw)
        return benor.run_trial_states(kw.pop("N"), kw.pop("F"), kw.pop("faulty"), trial=trial, **kw)

    def restated(self, trial):
        """(bins, rounds, states) of one trial by the restatement."""
        out = self.restate(trial)
        return (out[0], out[1], out[2]) if self.level == "node" else (out[0], out[1], (out[2], out[3]))

    def state_trials(self):
        """Up to 16 trials spread evenly over the range, first and last included (fewer where a plan is slow to make)."""
        m = self.kw["N"] - sum(1 for v in self.kw.get("faulty", ()) if v) if self.level == "node" else 0
        n = min(self.trials, 16 if m <= 300 else 6 if m <= 1100 else 2)
        return sorted({self.begin + ((self.trials - 1) * k) // max(1, n - 1) for k in range(n)})


# ------------------------------------------------------------ the generator
def pick(rng, options):
    """One of {value: probability}."""
    values = list(options)
    return values[int(rng.choice(len(values), p=[options[v] for v in values]))]


def word(rng, options=(0, ALL, HALF, "random")):
    w = options[int(rng.integers(len(options)))]
    return int(rng.integers(0, 1 << 32)) if w == "random" else w


def trial_range(rng, trials):
    kind = pick(rng, {"low": 0.4, "carry": 0.3, "high": 0.3})
    if kind == "low":
        return int(rng.integers(0, 1 << 20))
    if kind == "carry":                           # the range crosses 2^32: the counter's low half wraps inside a launch
        return (1 << 32) - 1 - int(rng.integers(0, max(1, trials - 1)))
    return (1 << 32) + int(rng.integers(0, 1 << 40))


def trials_for(family, m, k_max):
    """The band's count, and at most what 6 * 10^6 walk words allow: a trial that never decides walks up to m / 3 words
    for each of m receivers in each of 2 k_max phases (the scheduler's closed forms walk none)."""
    t = 60 if m <= 64 else 12 if m <= 300 else 2 if m <= 1100 else 1
    t = max(1, t // FACTOR.get(family, 1))
    return t if family == "sched" else max(1, min(t, 6 * 10 ** 6 // (m * m * k_max)))


def round_cap(rng, m):
    """k_max from {1, 2, 3, 16, 40}; above 300 live nodes without 40 and above 1100 without 16: one such trial that
    does not decide restates in minutes."""
    return int(rng.choice([1, 2, 3, 16, 40][:5 if m <= 300 else 4 if m <= 1100 else 3]))


def sizes(rng, family, tied):
    """(N, F, f): the live count m = N - f from the size class, F from a ratio, f from its own class.  Mode 3 has no
    "?": its tied start needs an even live count, and f = F an odd one (the quorum is then m)."""
    size = pick(rng, {"small": 0.24, "edge": 0.2, "max": 0.1, "band": 0.46})
    fmode = pick(rng, {"zero": 0.26, "full": 0.22, "any": 0.52})
    group = family in BYZ and rng.random() < 0.22  # room for 64 liars side by side
    if size == "max":
        N, f = 4096, 0
        F = int(N * rng.uniform(0.05, 0.45))
    else:
        if size == "small":
            m = int(rng.integers(2, 33))
        elif size == "edge":
            m = int(rng.choice([64, 65, 128, 129]))
        else:
            lo, hi = pick(rng, {(33, 63): 0.3, (66, 300): 0.4, (301, 1100): 0.25, (1101, 3000): 0.05})
            m = int(rng.integers(lo, hi + 1))
        if family in BYZ and rng.random() < 0.18:
            m = 64 * int(rng.integers(1, 5)) + 1      # the last group holds one lane
        if group and m < 129:
            m = int(rng.choice([129, 130, 193, 200]))
        if family == "mode3" and fmode == "full":
            m += 1 - m % 2
        elif family == "mode3" and tied:
            m += m % 2
        u = rng.uniform(0.05, 0.45 if fmode == "zero" else 0.6)
        F = min(int(round(m * u / (1.0 - u))), 4096 - m)
        if group:
            F = max(F, 64)
            if F + m > 4096 or F >= m:
                F = 64
        low = max(0, F - m + 1)                   # q = m - (F - f) >= 1
        f = {"zero": low, "full": F, "any": int(rng.integers(low, F + 1))}[fmode]
        if group:
            f = min(f, F - 64)
        N = m + f
    if family == "mode3" and (N - F) % 2 == 0:    # an odd quorum
        if F > f:
            F -= 1
        elif F + 1 < N:
            F += 1
        else:                                     # N = F + 1 with f = F and an even q cannot be: q = 1
            raise AssertionError((N, F, f))
    return N, F, f


def scatter(rng, pool, n):
    return sorted(int(i) for i in rng.choice(pool, n, replace=False)) if n else []


def start_kind(rng, family):
    return pick(rng, {"random": 0.35, "fixed": 0.3, "tied": 0.35} if family == "mode3" else
                {"random": 0.3, "fixed": 0.26, "all ?": 0.2, "tied": 0.24})


def starts(rng, family, kind, N, honest):
    """initial_values: None (random), or fixed with about 10 % "?", all "?", or tied over the honest live nodes."""
    plain = family == "mode3"
    if kind == "random":
        return None
    if kind == "all ?":
        return [Q] * N
    p = [0.5, 0.5, 0.0] if plain else [0.45, 0.45, 0.10]
    init = [Q if v == 2 else int(v) for v in rng.choice(3, size=N, p=p)]
    if kind == "tied":
        h = len(honest)
        nq = 0 if plain else min(h, int(h * 0.1))
        nq += (h - nq) % 2                        # (mode 3 with an odd live count stays untied)
        if nq <= h and not (plain and nq):
            vals = [Q] * nq + [0, 1] * ((h - nq) // 2)
            for i, k in zip(honest, rng.permutation(h)):
                init[i] = vals[int(k)]
    return init


def table_bytes(m0, q, n):
    """The thresholds of the tables of every pool size m0 - d, d = 0 .. n: an upper bound of what the host builds."""
    total = 0
    for m in range(m0 - n, m0 + 1):
        K = np.arange(m + 1)
        total += 8 * int((np.minimum(K, q) - np.maximum(0, q - (m - K))).sum())
    return total


def crash_schedule(rng, N, F, f, live, faulty, k_max):
    """The schedule's keyword arguments: explicit (several crashers on one step, both phases, steps at and beyond the
    clamp 2 k_max) or random (up to F - f crashes, windows 1 .. 4 k_max)."""
    m0, q, margin = len(live), N - F, F - f
    cap = min(margin, 270 if m0 <= 300 else 24 if m0 <= 1100 else 3)
    while cap and table_bytes(m0, q, cap) > TABLE_CAP:
        cap -= 1
    if cap == 0:
        return {}
    n = cap if (cap == margin and rng.random() < 0.4) else int(rng.integers(1, cap + 1))
    if rng.random() < 0.5:
        window = 1 if rng.random() < 0.25 else int(rng.integers(1, 4 * k_max + 1))
        return {"crash_count": n, "crash_window": window}
    kind = pick(rng, {"step 0": 0.28, "beyond": 0.28, "mixed": 0.44})
    if kind == "step 0":
        steps = [0]
    elif kind == "beyond":
        steps = [2 * k_max, 2 * k_max + 1, 2 * k_max + int(rng.integers(2, 1000)), ALL - 1]
    else:
        steps = sorted({int(s) for s in rng.integers(0, 2 * k_max + 3, size=int(rng.integers(1, 5)))} | {2 * k_max - 1})
        if rng.random() < 0.5:
            steps.append(2 * k_max)
    crash_at = [None] * N
    for i in scatter(rng, live, n):
        crash_at[i] = steps[int(rng.integers(len(steps)))]
    for i in range(N):                            # a faulty node's entry is not read
        if faulty[i] and rng.random() < 0.5:
            crash_at[i] = int(rng.integers(0, 8))
    return {"crash_at": crash_at}


def liars(rng, F, f, live):
    """The Byzantine nodes: b = 0, b = F - f or in between, scattered over the live nodes; where there is room, 64 of
    them side by side on one 64-lane group of compact indices."""
    room, m = F - f, len(live)
    b = {"zero": 0, "full": room, "any": int(rng.integers(0, room + 1))}[pick(rng, {"zero": 0.22, "full": 0.3, "any": 0.48})]
    ids = set()
    if room >= 64 and m >= 129 and rng.random() < 0.8:
        g = int(rng.integers(0, m // 64))         # a whole group: compact indices 64 g .. 64 g + 63
        ids = {live[c] for c in range(64 * g, 64 * g + 64)}
        b = max(b, 64)
    rest = [i for i in live if i not in ids]
    ids |= set(scatter(rng, rest, b - len(ids)))
    return ids


def rule_words(rng, N, F):
    kind = pick(rng, {"a": 0.3, "b": 0.2, "ref": 0.2, "random": 0.3})
    if kind == "random":
        return kind, (int(rng.integers(0, 2 * N + 1)), int(rng.integers(0, N - F + 1)), int(rng.integers(0, 2 * N + 1)))
    return kind, {"a": rule_model.protocol_a, "b": rule_model.protocol_b, "ref": rule_model.reference}[kind](N, F)


def plain_kernel(q, init, live):
    """Mode 4's plan: mode 3's kernel inside that mode's scope (an odd quorum, no "?" among the live nodes)."""
    has_q = init is not None and any(init[i] == Q for i in live)
    return benor.BO_KERNEL_TALLY if q % 2 and not has_q else benor.BO_KERNEL_TALLY3


def node_case(family, i, rng):
    kind = start_kind(rng, family)
    N, F, f = sizes(rng, family, kind == "tied")
    faulty = [False] * N
    for j in scatter(rng, N, f):
        faulty[j] = True
    live = [j for j in range(N) if not faulty[j]]
    m, q = len(live), N - F
    k_max = round_cap(rng, m)
    byz_ids = liars(rng, F, f, live) if family in BYZ else set()
    honest = [j for j in live if j not in byz_ids]
    init = starts(rng, family, kind, N, honest)
    seed = int(rng.integers(0, 1 << 63))
    trials = trials_for(family, m, k_max)
    begin = trial_range(rng, trials)
    kw = dict(N=N, F=F, faulty=faulty, seed=seed, k_max=k_max, initial_values=init)
    classes = set()
    plain = plain_kernel(q, init, live)
    if family == "mode3":
        kw["mode"], kernel = 3, benor.BO_KERNEL_TALLY
        restate = lambda t: mode3.tally_trial(N, F, faulty, seed, t, k_max, init)                       # noqa: E731
    elif family == "mode4":
        kw["mode"], kernel = 4, plain
        restate = lambda t: mode4.tally3_trial(N, F, faulty, seed, t, k_max, init)                      # noqa: E731
    elif family in CRASH:
        sched = crash_schedule(rng, N, F, f, live, faulty, k_max)
        mode = {"mode5": 5, "mode6": 6, "mode7": 7}[family]
        extra = {}
        if family == "mode6":
            cut = pick(rng, {0: 0.2, m: 0.2, "between": 0.3, benor.CUT_RANDOM: 0.3})
            extra["crash_cut"] = int(rng.integers(1, max(2, m))) if cut == "between" else cut
        if family == "mode7":
            extra["crash_reach"] = word(rng, (0, ALL, HALF, QUARTER, "random"))
        kw.update(mode=mode, **sched, **extra)
        fn = {5: mode5.crash_trial, 6: mode6.partial_trial, 7: mode7.subset_trial}[mode]
        restate = lambda t: fn(N, F, faulty, seed, t, k_max, init, **sched, **extra)                    # noqa: E731
        at = sched.get("crash_at")
        steps = [at[j] for j in live if at[j] is not None] if at else []
        n = len(steps) if at else sched.get("crash_count", 0)
        kernel = plain if n == 0 else benor.BO_KERNEL_TALLY_CRASH + mode - 5       # an empty schedule is mode 4's plan
        if n and (all(s == 0 for s in steps) if at else sched["crash_window"] == 1):
            classes.add("all on step 0")
        if n and f + n == F:
            classes.add("margin emptied")
        if steps and all(s >= 2 * k_max for s in steps):
            classes.add("wholly beyond 2 k_max")
    else:
        byz = [j in byz_ids for j in range(N)]
        b = len(byz_ids)
        kw["byzantine"] = byz
        if family == "sched":
            rule = pick(rng, {"ref": 0.5, "b": 0.5})
            extra = dict(byz_strategy=int(rng.choice([BALANCE, SPLIT])), coin_common=word(rng, (0, HALF, ALL)))
            kw.update(mode=sched_model.mode_of(rule), **extra)
            kernel = sched_model.kernel_of(rule, extra["coin_common"])
            restate = lambda t: sched_model.sched_trial(rule, N, F, faulty, byz, seed, t, k_max, init, **extra)   # noqa: E731
        elif family == "byz":
            mode = int(rng.choice([8, 9, 10, 11]))
            rule = "b" if mode in (9, 11) else "ref"
            extra = dict(byz_strategy=int(rng.choice([RANDOM, OPPOSE, BALANCE, SPLIT])), byz_one=word(rng))
            coin = word(rng) if mode >= 10 else 0
            kw.update(mode=mode, **extra, **({"coin_common": coin} if mode >= 10 else {}))
            # a shared-coin mode without its coin is its parent's plan; mode 8 without a liar is mode 4's
            kernel = benor.BO_KERNEL_TALLY_BYZ + (1 if rule == "b" else 0) + (2 if coin else 0)
            if kernel == benor.BO_KERNEL_TALLY_BYZ and b == 0:
                kernel = plain
            restate = lambda t: coin_model.coin_trial(rule, N, F, faulty, byz, seed, t, k_max, init, coin_common=coin,   # noqa: E731
                                                      **extra)
        else:
            mode = int(rng.choice([9, 11, 13]))
            name, words = rule_words(rng, N, F)
            coin = word(rng) if mode >= 11 else 0
            if mode == 13:
                extra = dict(byz_strategy=int(rng.choice([BALANCE, SPLIT])))
                kernel = sched_model.kernel_of("b", coin)
                restate = lambda t: rule_model.sched_trial(words, N, F, faulty, byz, seed, t, k_max, init, coin_common=coin,   # noqa: E731
                                                           **extra)
            else:
                extra = dict(byz_strategy=int(rng.choice([RANDOM, OPPOSE, BALANCE, SPLIT])), byz_one=word(rng))
                kernel = benor.BO_KERNEL_TALLY_BYZ_B + (2 if coin else 0)
                restate = lambda t: rule_model.coin_trial(words, N, F, faulty, byz, seed, t, k_max, init, coin_common=coin,   # noqa: E731
                                                          **extra)
            kw.update(mode=mode, thresholds=words, **extra, **({"coin_common": coin} if mode >= 11 else {}))
        if b == 0:
            classes.add("b=0")
        if b == F - f:
            classes.add("b=F-f")
        groups = [[live[c] in byz_ids for c in range(g, min(g + 64, m))] for g in range(0, m, 64)]
        if any(all(g) for g in groups):
            classes.add("group without honest lane")
        if m % 64 == 1:
            classes.add("group of one lane")
    # the classes every node-level family shares, read off the configuration
    if m == q:
        classes.add("m=q")
    if m <= 32:
        classes.add("m<=32")
    if m in (64, 65, 128, 129):
        classes.add("m in 64,65,128,129")
    if N == 4096 and f == 0:
        classes.add("N=4096")
    if f == 0:
        classes.add("f=0")
    if k_max == 1:
        classes.add("k_max=1")
    if init is not None:
        vals = [init[j] for j in honest]
        if all(v == Q for v in vals):
            classes.add("all ?")
        if vals.count(0) == vals.count(1) > 0:     # (an all-"?" start is its own class)
            classes.add("tied")
    return Case(family, i, "node", kw, restate, begin, trials, frozenset(classes), kernel)


def lumped_case(i, rng):
    size = pick(rng, {"small": 0.25, "node": 0.25, "large": 0.3, "max": 0.2})
    if size == "max":
        N = 1 << 24
    else:
        lo, hi = {"small": (2, 64), "node": (65, 4096), "large": (4097, (1 << 24) - 1)}[size]
        N = int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))))
    F = min(N - 1, int(N * rng.uniform(0.02, 0.6)))
    f = {"zero": 0, "full": F, "any": int(rng.integers(0, F + 1))}[pick(rng, {"zero": 0.3, "full": 0.22, "any": 0.48})]
    room = F - f
    b = {"zero": 0, "full": room, "any": int(rng.integers(0, room + 1))}[pick(rng, {"zero": 0.25, "full": 0.3, "any": 0.45})]
    m = N - f
    even_n, odd_n = (m + 1) // 2, m // 2
    byz_even = int(rng.integers(max(0, b - odd_n), min(b, even_n) + 1))
    hh = m - b
    k_max = int(rng.choice([1, 2, 3, 16, 40]))
    kind = pick(rng, {"random": 0.3, "fixed": 0.26, "all ?": 0.2, "tied": 0.24})
    if kind == "random":
        init = None
    elif kind == "all ?":
        init = (0, 0, hh)
    elif kind == "tied":
        nq = int(hh * 0.1)
        nq += (hh - nq) % 2
        init = ((hh - nq) // 2, (hh - nq) // 2, nq)
    else:
        nq = int(hh * rng.uniform(0.0, 0.2))
        n0 = int(rng.integers(0, hh - nq + 1))
        init = (n0, hh - nq - n0, nq)
    seed = int(rng.integers(0, 1 << 63))
    common = dict(f=f, b=b, byz_even=byz_even, byz_strategy=int(rng.choice([BALANCE, SPLIT])),
                  coin_common=word(rng), )
    trials = 200
    begin = trial_range(rng, trials)
    kw = dict(N=N, F=F, seed=seed, k_max=k_max, initial_values=init, **common)
    if rng.random() < 0.5:
        rule = int(rng.integers(0, 2))
        kw["rule"] = rule
        restate = lambda t: lumped_model.lumped_trial("b" if rule else "ref", N, F, seed, t, k_max, init=init, **common)   # noqa: E731
    else:
        _, words = rule_words(rng, N, F)
        kw["thresholds"] = words
        restate = lambda t: rule_model.lumped_trial(words, N, F, seed, t, k_max, init=init, **common)   # noqa: E731
    classes = {name for name, hit in (("m=q", f == F), ("f=0", f == 0), ("k_max=1", k_max == 1), ("b=0", b == 0),
                                      ("b=F-f", b == room), ("N=2^24", N == 1 << 24),
                                      ("all ?", init is not None and init[2] == hh),
                                      ("tied", init is not None and init[0] == init[1] > 0)) if hit}
    return Case("lumped", i, "class", kw, restate, begin, trials, frozenset(classes), -1)


def case(family, i):
    rng = np.random.default_rng(BASE[family] + i)
    return lumped_case(i, rng) if family == "lumped" else node_case(family, i, rng)


def all_cases():
    return [(family, i) for family in FAMILIES for i in range(CASES)]


def hist_of(c, restated):
    h = np.zeros(oracle.hist_len(c.kw["k_max"]), dtype=np.uint64)
    for out in restated.values():
        for b in out[0]:
            h[b] += 1
    return h


# ------------------------------------------------------------ instrumented word streams
class Counter:
    """What a patched WordStream.below saw: draws, words and the denominators of the draws that rejected."""

    def __init__(self):
        self.draws, self.words, self.rejected = 0, 0, []


@contextlib.contextmanager
def word_streams(reject=True):
    """Every test_tally3.WordStream (and the schedule's subclass) counts its words while the block runs; with
    reject=False a draw takes its first word whatever the low half says: the biased draw that a kernel without the
    rejection test would make."""
    counter = Counter()
    plain = mode4.WordStream.below

    def below(self, d):
        counter.draws += 1
        first = self.i
        if reject:
            v = plain(self, d)
        else:
            v = (self.next() * d) >> 32
        counter.words += self.i - first
        if self.i - first > 1:
            counter.rejected.append(d)
        return v

    mode4.WordStream.below = below
    try:
        yield counter
    finally:
        mode4.WordStream.below = plain


def rejects_first_word(w, d):
    """Whether the multiply-shift draw below d rejects the word w."""
    return ((w * d) & 0xFFFFFFFF) < (1 << 32) % d


M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox_np(seed, c0, c1, c2, c3):
    """Philox4x32-10 over numpy arrays of counters (any of them may be a scalar): the four output words."""
    mask = np.uint64(0xFFFFFFFF)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(x, shape).copy() for x in c]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return c


# ------------------------------------------------------------ directed rare-path constants (tools/find_rare_words.py)
def thirds(N):
    return [(Q, 0, 1)[i % 3] for i in range(N)]


def sensitive(restate, trial):
    """(the denominators of the trial's rejected draws, whether a draw that never rejects changes the result)."""
    with word_streams() as seen:
        exact = restate(trial)
    if not seen.rejected:
        return [], False
    with word_streams(reject=False):
        biased = restate(trial)
    return seen.rejected, biased != exact


# The directed shapes: (1003, 334), starts "?", 0, 1 by node id mod 3, one round (the states are then the P-phase's
# own outcome, which one vote more or less can change): about 2 * 10^5 walk words a trial.
BIG = dict(N=1003, F=334, faulty=[False] * 1003, seed=SEED, k_max=1, initial_values=thirds(1003))
LANE_BYZ = [i % 25 == 0 for i in range(1003)]                 # 41 liars: every draw is the lane's own (draw3_lane)
HEARD_BYZ = [i % 10 < 3 for i in range(1003)]                 # 301 liars that read the inbox: the stream-11 walk
LANE = dict(BIG, mode=8, byzantine=LANE_BYZ, byz_one=HALF, byz_strategy=RANDOM)
HEARD = dict(BIG, mode=8, byzantine=HEARD_BYZ, byz_one=0, byz_strategy=BALANCE)


def restate_big(kw):
    a = (kw["N"], kw["F"], kw["faulty"])
    if kw.get("mode", 4) == 4:
        return lambda t: mode4.tally3_trial(*a, kw["seed"], t, kw["k_max"], kw["initial_values"])
    return lambda t: coin_model.coin_trial("ref", *a, kw["byzantine"], kw["seed"], t, kw["k_max"], kw["initial_values"],
                                           byz_one=kw["byz_one"], byz_strategy=kw["byz_strategy"])


DIRECTED = {"walk": restate_big(BIG), "lane": restate_big(LANE), "heard": restate_big(HEARD)}
# python tools/find_rare_words.py walk | lane | heard --fast --trials 6000: the first trial that rejects a word (in the
# R-phase, at denominators 380, 416 and 402) and is sensitive to it; 10 s, 12 s and 3 s on seven cores.  With two
# rounds no trial of 30000 was sensitive: 567 rejected a word, and all of them decided the same value in round 2.
RARE_TRIAL = {"walk": 1097, "lane": 1979, "heard": 537}
# (c) a rejected stream-7 word: python tools/find_rare_words.py schedule
#     node draw: d = m0 - crash_count + 1 with the largest 2^32 mod d among d <= 700; step draw: window 997
#     (2^32 mod 997 = 966); 2^26 trial ids scanned with philox_np in 35 s, twelve hits each, the first kept
SCHED_NODE = dict(N=684, F=228, crash_count=1, crash_window=2, k_max=4, trial=2085166)     # steps 0, 1: always reached
SCHED_STEP = dict(N=10, F=5, crash_count=3, crash_window=997, k_max=512, trial=7151745)     # N - F <= F: never decides


def restate_schedule(d):
    N = d["N"]
    return lambda t: mode5.crash_trial(N, d["F"], [False] * N, SEED, t, d["k_max"], None, crash_count=d["crash_count"],
                                       crash_window=d["crash_window"])


# ------------------------------------------------------------ the tests
def test_philox_np_is_the_oracles():
    """Against oracle.philox4x32_10 (through test_tally.philox)."""
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 1 << 32, size=(4, 64), dtype=np.uint64)
    got = philox_np(SEED, *ctr)
    for k in range(64):
        assert tuple(int(w[k]) for w in got) == mode3.philox(SEED, tuple(int(x) for x in ctr[:, k]))


def test_every_case_is_valid_and_plans_its_kernel():
    """No generated configuration is refused, skipped or caught: the share left out is zero."""
    made = 0
    for family, i in all_cases():
        c = case(family, i)
        if c.level == "class":
            c.plan()                              # bo_lumped_check(_rule): raises on a refusal
        else:
            kw = dict(c.kw)
            thresholds = kw.pop("thresholds", None)
            got = benor.kernel_for(kw.pop("N"), kw.pop("F"), kw.pop("faulty"), **kw)
            assert got == c.kernel, str(c)
            assert benor.BO_KERNEL_TALLY <= got <= benor.BO_KERNEL_TALLY_SCHED_B_COIN, str(c)
            if thresholds is not None:
                benor.rule_check(thresholds)
        assert c.trials >= 1 and 0 <= c.begin < 1 << 63
        made += 1
    assert made == len(FAMILIES) * CASES and len(all_cases()) - made == 0


def test_the_generator_reads_its_seed_only():
    for family in FAMILIES:
        a, b = case(family, 5), case(family, 5)
        assert str(a) == str(b) and a.state_trials() == b.state_trials()


@pytest.mark.parametrize("family", FAMILIES)
def test_edge_classes_occur(family):
    seen = {name: [] for name in EDGE_CLASSES[family]}
    for i in range(CASES):
        for name in case(family, i).classes:
            if name in seen:
                seen[name].append(i)
    short = {name: ids for name, ids in seen.items() if len(ids) < 3}
    assert not short, (family, short)


def test_both_halves_of_the_trial_counter_carry():
    for family in FAMILIES:
        begins = [case(family, i) for i in range(CASES)]
        assert any(c.begin < 1 << 32 and c.begin + c.trials > 1 << 32 for c in begins), family
        assert any(c.begin > 1 << 32 for c in begins) and any(c.begin + c.trials < 1 << 32 for c in begins), family


# ---- the references against each other, on generated configurations
def small(family, count=5, m_max=300, want=lambda c: True):
    """The family's first `count` cases with at most m_max live nodes that `want` accepts."""
    out = []
    for i in range(CASES):
        c = case(family, i)
        m = c.kw["N"] - sum(1 for v in c.kw["faulty"] if v)
        if m <= m_max and want(c):
            out.append(c)
    assert len(out) >= min(count, 3), (family, len(out))
    return out[:count]


def base_args(c):
    kw = c.kw
    return kw["N"], kw["F"], kw["faulty"], kw["seed"], kw["k_max"], kw["initial_values"]


def three(c):
    return [c.begin, c.begin + c.trials // 2, c.begin + c.trials - 1]


def sched_of(c):
    return {k: c.kw[k] for k in ("crash_at", "crash_count", "crash_window") if k in c.kw}


def test_identity_reach_0_is_mode_5_and_full_reach_is_a_full_cut():
    for c in small("mode7", want=lambda c: sched_of(c)):
        N, F, faulty, seed, k_max, init = base_args(c)
        m0 = N - sum(faulty)
        for t in three(c):
            assert mode7.subset_trial(N, F, faulty, seed, t, k_max, init, crash_reach=0, **sched_of(c)) == \
                mode5.crash_trial(N, F, faulty, seed, t, k_max, init, **sched_of(c)), str(c)
            assert mode7.subset_trial(N, F, faulty, seed, t, k_max, init, crash_reach=ALL, **sched_of(c)) == \
                mode6.partial_trial(N, F, faulty, seed, t, k_max, init, crash_cut=m0, **sched_of(c)), str(c)


@pytest.mark.parametrize("family", CRASH)
def test_identity_an_empty_or_unreached_schedule_is_mode_4(family):
    fn = {"mode5": mode5.crash_trial, "mode6": mode6.partial_trial, "mode7": mode7.subset_trial}[family]
    for c in small(family):
        N, F, faulty, seed, k_max, init = base_args(c)
        extra = {k: c.kw[k] for k in ("crash_cut", "crash_reach") if k in c.kw}
        live = [i for i in range(N) if not faulty[i]]
        never = [None] * N                            # as many crashers as the margin allows, beyond the last step
        for k, i in enumerate(live[:min(3, F - sum(faulty))]):
            never[i] = 2 * k_max + k
        for t in three(c):
            want = mode4.tally3_trial(N, F, faulty, seed, t, k_max, init)
            assert fn(N, F, faulty, seed, t, k_max, init, **extra) == want, str(c)
            assert fn(N, F, faulty, seed, t, k_max, init, crash_at=never, **extra) == want, str(c)


def test_identity_mode_4_in_mode_3s_scope_is_mode_3():
    for c in small("mode3", count=8):
        for t in three(c):
            assert mode4.tally3_trial(*base_args(c)[:4], t, *base_args(c)[4:]) == \
                mode3.tally_trial(*base_args(c)[:4], t, *base_args(c)[4:]), str(c)


def test_identity_no_liar_and_no_coin_is_mode_4():
    for c in small("byz", count=8):
        N, F, faulty, seed, k_max, init = base_args(c)
        nobody = [False] * N
        for t in three(c):
            got = coin_model.coin_trial("ref", N, F, faulty, nobody, seed, t, k_max, init, byz_one=c.kw["byz_one"],
                                        byz_strategy=c.kw["byz_strategy"], coin_common=0)
            bins, rounds, states = mode4.tally3_trial(N, F, faulty, seed, t, k_max, init)
            assert got[:2] == (bins, rounds), str(c)
            assert [s for s, dead in zip(got[2], faulty) if not dead] == [s for s, dead in zip(states, faulty) if not dead], str(c)


def test_identity_coin_common_0_is_the_parent_mode():
    """Against the parent modes' own restatements (tests/test_byz_tally.py, test_byz_heard.py, test_byz_rule_b.py)."""
    for c in small("byz", count=10):
        N, F, faulty, seed, k_max, init = base_args(c)
        byz, lie = c.kw["byzantine"], dict(byz_one=c.kw["byz_one"], byz_strategy=c.kw["byz_strategy"])
        rule = "b" if c.kw["mode"] in (9, 11) else "ref"
        if rule == "b":
            parent = mode9.rule_b_trial
        else:
            parent = heard_model.heard_trial if lie["byz_strategy"] in (BALANCE, SPLIT) else mode8.byz_trial
        for t in three(c):
            assert coin_model.coin_trial(rule, N, F, faulty, byz, seed, t, k_max, init, coin_common=0, **lie) == \
                parent(N, F, faulty, byz, seed, t, k_max, init, **lie), str(c)


def test_identity_protocol_bs_words_are_modes_9_11_and_13():
    for c in small("rule", count=10):
        N, F, faulty, seed, k_max, init = base_args(c)
        byz, coin, words = c.kw["byzantine"], c.kw.get("coin_common", 0), rule_model.protocol_b(N, F)
        for t in three(c):
            if c.kw["mode"] == 13:
                kw = dict(byz_strategy=c.kw["byz_strategy"], coin_common=coin)
                assert rule_model.sched_trial(words, N, F, faulty, byz, seed, t, k_max, init, **kw) == \
                    sched_model.sched_trial("b", N, F, faulty, byz, seed, t, k_max, init, **kw), str(c)
            else:
                kw = dict(byz_strategy=c.kw["byz_strategy"], byz_one=c.kw["byz_one"], coin_common=coin)
                assert rule_model.coin_trial(words, N, F, faulty, byz, seed, t, k_max, init, **kw) == \
                    coin_model.coin_trial("b", N, F, faulty, byz, seed, t, k_max, init, **kw), str(c)


def test_identity_the_references_words_are_modes_8_10_and_12():
    """Where N <= 3F + 1: a quorum cannot hold F + 1 of both values."""
    for c in small("rule", count=8, want=lambda c: c.kw["N"] <= 3 * c.kw["F"] + 1):
        N, F, faulty, seed, k_max, init = base_args(c)
        byz, coin, words = c.kw["byzantine"], c.kw.get("coin_common", 0), rule_model.reference(N, F)
        for t in three(c):
            if c.kw["mode"] == 13:
                kw = dict(byz_strategy=c.kw["byz_strategy"], coin_common=coin)
                assert rule_model.sched_trial(words, N, F, faulty, byz, seed, t, k_max, init, **kw) == \
                    sched_model.sched_trial("ref", N, F, faulty, byz, seed, t, k_max, init, **kw), str(c)
            else:
                kw = dict(byz_strategy=c.kw["byz_strategy"], byz_one=c.kw["byz_one"], coin_common=coin)
                assert rule_model.coin_trial(words, N, F, faulty, byz, seed, t, k_max, init, **kw) == \
                    coin_model.coin_trial("ref", N, F, faulty, byz, seed, t, k_max, init, **kw), str(c)


# ---- the directed constants keep their property
@pytest.mark.parametrize("kind", list(DIRECTED))
def test_rare_trial_rejects_a_walk_word(kind):
    rejected, differs = sensitive(DIRECTED[kind], RARE_TRIAL[kind])
    assert len(rejected) >= 1 and differs, kind


@pytest.mark.parametrize("d,denominator", [(SCHED_NODE, 684), (SCHED_STEP, 997)])
def test_rare_trial_rejects_a_schedule_word(d, denominator):
    """The vectorised scan's hit, re-derived through the restatement's own stream: the draw below `denominator` is
    the one that rejects, and without the rejection another node crashes, or the same one at another step."""
    t = d["trial"]
    w = philox_np(SEED, t & 0xFFFFFFFF, t >> 32, 0, 7 << 24)
    assert rejects_first_word(int(w[0 if d is SCHED_NODE else 1]), denominator)
    rejected, differs = sensitive(restate_schedule(d), t)
    assert rejected == [denominator] and differs
