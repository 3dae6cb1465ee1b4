"""Interleaved A/B of environment-selected variants in ONE process (GPU).

The runtime reads its A/B knobs (BENOR_BIG_FORM, BENOR_COOP_BW, BENOR_BLOCKS_PER_CU,
... -- the registered ones, benor.KNOBS; any other variable is refused, since a
removed knob would time two identical variants) at every launch, so variants can
alternate launch by launch on one plan, one process, one box: ROUNDS rounds,
each timing every variant once per shape in rotated order (cdna_hip_programming.md
section 5.4 rule 24).  Each timing is REPS back-to-back launches between HIP
events on the launch stream.  Prints one JSON line per (shape, variant) with the
median and minimum ms per launch and the variant's median / first variant's.

    python tools/ab_inproc.py --variants "coop=BENOR_BIG_FORM:coop;wave=BENOR_BIG_FORM:wave" \
        --shapes "4096,1365,400000;4096,0,100000" [--rounds 7] [--reps 3]

A shape may carry a fourth field f < F (the first f nodes crashed, the rest of
F the random-delivery slack: BO_MODE_RANDOM_DELIVERY).  A variant may also name
the delivery mode with the pseudo-variable `mode` (lockstep, random, tally, tally3, crash, partial, subset, byz or byzb),
so the mask-level and the count-level random-delivery modes are timed
alternately on one plan each:

    python tools/ab_inproc.py --variants "mask=mode:random;tally=mode:tally" --shapes "1024,341,100000,0"

`mode:crash` (BO_MODE_CRASH_TALLY) takes its schedule from further pseudo-variables:
`crash_count` and `crash_window` (a random schedule per trial) or `crash_at`
(explicit, node@step+node@step; a step of 64 or more is never reached at this
tool's k_max of 32, which times the mode's kernel on mode 4's results):

    python tools/ab_inproc.py --variants "t3=mode:tally3;idle=mode:crash,crash_at:0@64;c16=mode:crash,crash_count:16,crash_window:4" \
        --shapes "1024,340,100000,0"

`mode:partial` (BO_MODE_CRASH_PARTIAL) takes the same schedule and `crash_cut`, a
count of initially-live receivers or `random`; at `crash_cut:0` it gives mode:crash's
results on its own kernel, so that pair times the kernel's overhead alone:

    python tools/ab_inproc.py --rounds 7 --reps 5 --shapes "1024,340,100000,0" --variants \
        "m5=mode:crash,crash_count:16,crash_window:4;cut0=mode:partial,crash_count:16,crash_window:4,crash_cut:0;rand=mode:partial,crash_count:16,crash_window:4,crash_cut:random"

`mode:subset` (BO_MODE_CRASH_SUBSET) takes the same schedule and `crash_reach`: `all`
(UINT32_MAX), a probability with a decimal point (0.5) or the 32-bit word itself.  At
`crash_reach:0` it gives mode:crash's results and at `crash_reach:all` those of
mode:partial with a full cut, both on its own kernel:

    python tools/ab_inproc.py --rounds 7 --reps 5 --shapes "1024,340,100000,0" --variants \
        "m5=mode:crash,crash_count:16,crash_window:4;r0=mode:subset,crash_count:16,crash_window:4,crash_reach:0;half=mode:subset,crash_count:16,crash_window:4,crash_reach:0.5"

`mode:byz` (BO_MODE_BYZ_TALLY) takes `byzantine` (the b live nodes after the crashed
ones lie), `byz_one` (`all`, a probability with a decimal point or the 32-bit word) and
`byz_strategy` (random, oppose, balance or split; the last two read the receiver's inbox
and not `byz_one`); next to mode:tally3 it times what the liars cost:

    python tools/ab_inproc.py --rounds 7 --reps 5 --shapes "1024,340,100000,0" --variants \
        "t3=mode:tally3;half=mode:byz,byzantine:100,byz_one:0.5;all=mode:byz,byzantine:100,byz_one:all;opp=mode:byz,byzantine:100,byz_one:0.5,byz_strategy:oppose"
    python tools/ab_inproc.py --rounds 7 --reps 5 --shapes "1024,340,100000,0" --variants \
        "t3=mode:tally3;half=mode:byz,byzantine:100,byz_one:0.5;bal=mode:byz,byzantine:100,byz_strategy:balance;split=mode:byz,byzantine:100,byz_strategy:split"

`mode:byzb` (BO_MODE_BYZ_RULE_B, Ben-Or's Byzantine-tolerant rule) takes mode:byz's three variables;
next to mode:byz on the same liars it times the two rules, whose rounds per trial differ by design
(compare node_rounds_per_s, the figure per unit of work):

    python tools/ab_inproc.py --rounds 7 --reps 5 --shapes "1024,204,100000,0" --variants \
        "m8=mode:byz,byzantine:16,byz_strategy:split;m9=mode:byzb,byzantine:16,byz_strategy:split"

`coin_common` (`all`, a probability with a decimal point or the 32-bit word) on mode:byz or mode:byzb
selects the shared-coin modes (BO_MODE_BYZ_COIN, BO_MODE_BYZ_RULE_B_COIN).  At `coin_common:1` (one round
in 2^32 is common) the outcomes are the parent mode's through the shared-coin entry, so that pair times
the coin policy alone; at `coin_common:all` the rounds per trial differ by design:

    python tools/ab_inproc.py --rounds 5 --reps 3 --shapes "1024,204,100000,0" --variants \
        "m9=mode:byzb,byzantine:16,byz_strategy:split;one=mode:byzb,byzantine:16,byz_strategy:split,coin_common:1;all=mode:byzb,byzantine:16,byz_strategy:split,coin_common:all"

`delivery:adversarial` on mode:byz or mode:byzb with `byz_strategy:balance` or `byz_strategy:split` selects the
adversarial scheduler's modes (BO_MODE_SCHED_TALLY, BO_MODE_SCHED_RULE_B; `coin_common` stays a variable of
theirs).  Next to the same line without it, it times the closed-form counts against the inbox-reading entries'
draws; rounds per trial differ by design, so compare node_rounds_per_s:

    python tools/ab_inproc.py --rounds 5 --reps 3 --shapes "1024,204,100000,0" --variants \
        "m11=mode:byzb,byzantine:16,byz_strategy:split,coin_common:all;m13=mode:byzb,byzantine:16,byz_strategy:split,coin_common:all,delivery:adversarial"

`level:class` on such a line runs the scheduler at the level of classes (benor.LumpedPlan, the lumped chain of
DESIGN §4.3.12: same law, another random stream, any N up to 2**24).  Its launches are the blocking bo_lumped_run,
so its time per launch includes that call's allocation and read-back; every line reports ns_per_trial_round, the
figure to compare across levels.  Alone it times sizes the node level cannot hold:

    python tools/ab_inproc.py --rounds 5 --reps 3 --shapes "4096,819,200000,0" --variants \
        "m13=mode:byzb,byzantine:16,byz_strategy:balance,delivery:adversarial;cls=mode:byzb,byzantine:16,byz_strategy:balance,delivery:adversarial,level:class"
    python tools/ab_inproc.py --rounds 5 --reps 3 --shapes "16777216,3355443,1000000,0" --variants \
        "cls=mode:byzb,byzantine:16,byz_strategy:balance,delivery:adversarial,level:class"

`rule:a`, `rule:b` or `rule:P:A:D` on a mode:byzb line replaces Protocol B's rule by a threshold rule of three
runtime words (Protocol A's words (N, 0, 2F), Protocol B's own, or the words given), at either
delivery and level.  With `rule:b` both sides produce the same outcomes, so next to the same line without it the
ratio is the cost of runtime thresholds; `rule:a` changes the rounds by design (compare ns_per_trial_round):

    python tools/ab_inproc.py --rounds 5 --reps 3 --shapes "1024,204,100000,0" --variants \
        "m13=mode:byzb,byzantine:16,byz_strategy:split,delivery:adversarial;thr=mode:byzb,byzantine:16,byz_strategy:split,delivery:adversarial,rule:b;a=mode:byzb,byzantine:16,byz_strategy:split,delivery:adversarial,rule:a"

Every line also reports
the live node-rounds per second its launches represent (bench.py node_rounds)
and the rounds a trial ran on average (k_max for an undecided one),
so variants that change the outcome (a diagnostic cap, a lie strategy) compare per unit of work.
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ben-or-consensus-algorithm_amd"))


def parse_variants(spec):
    out = []
    for item in spec.split(";"):
        name, _, kv = item.partition("=")
        env = {}
        for pair in filter(None, kv.split(",")):
            k, _, v = pair.partition(":")
            env[k] = v
        out.append((name, env))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", required=True, help="'name=VAR:val,VAR:val;name2=...' ('name=' = no variables)")
    ap.add_argument("--shapes", required=True,
                    help="'N,F,trials[,f];...' (the first f nodes crashed, f = F by default)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    variants = parse_variants(a.variants)
    shapes = []
    for sp in a.shapes.split(";"):
        v = [int(x) for x in sp.split(",")]
        shapes.append((v[0], v[1], v[2], v[3] if len(v) > 3 else v[1]))
    modes = {name: env.pop("mode", None) for name, env in variants}   # `mode` is no environment variable
    scheds = {name: {k: env.pop(k) for k in ("crash_count", "crash_window", "crash_at", "crash_cut", "crash_reach",
                                             "byzantine", "byz_one", "byz_strategy", "coin_common", "delivery", "level",
                                             "rule")
                     if k in env}
              for name, env in variants}                              # ... nor is the crash schedule
    knobs = sorted({k for _, env in variants for k in env})

    import benor
    unknown = [k for k in knobs if k not in benor.KNOBS]
    if unknown:
        ap.error(f"not a registered libbenor knob (benor.KNOBS): {unknown}")
    mode_ids = {"lockstep": benor.BO_MODE_LOCKSTEP, "random": benor.BO_MODE_RANDOM_DELIVERY,
                "tally": benor.BO_MODE_RANDOM_TALLY, "tally3": benor.BO_MODE_RANDOM_TALLY3,
                "crash": benor.BO_MODE_CRASH_TALLY, "partial": benor.BO_MODE_CRASH_PARTIAL,
                "subset": benor.BO_MODE_CRASH_SUBSET, "byz": benor.BO_MODE_BYZ_TALLY,
                "byzb": benor.BO_MODE_BYZ_RULE_B}
    bad = sorted({v for v in modes.values() if v is not None and v not in mode_ids})
    if bad:
        ap.error(f"mode must be one of {sorted(mode_ids)}: {bad}")
    byz_keys = ("byzantine", "byz_one", "byz_strategy", "coin_common", "delivery", "level", "rule")
    if any(any(k in sc for k in byz_keys) != (modes[name] in ("byz", "byzb")) for name, sc in scheds.items()):
        ap.error("byzantine / byz_one / byz_strategy go with mode:byz or mode:byzb, and they with them")
    if any(sc.get("delivery", "random") not in ("random", "adversarial") for sc in scheds.values()):
        ap.error("delivery is random or adversarial")
    if any(sc.get("delivery") == "adversarial" and sc.get("byz_strategy") not in ("balance", "split") for sc in scheds.values()):
        ap.error("delivery:adversarial needs byz_strategy:balance or byz_strategy:split")
    if any(sc.get("level", "node") not in ("node", "class") for sc in scheds.values()):
        ap.error("level is node or class")
    if any(sc.get("level") == "class" and sc.get("delivery") != "adversarial" for sc in scheds.values()):
        ap.error("level:class needs delivery:adversarial")
    if any("rule" in sc and modes[name] != "byzb" for name, sc in scheds.items()):
        ap.error("rule needs mode:byzb (it replaces Protocol B's rule)")
    if any("rule" in sc and sc["rule"] not in ("a", "b") and not re.fullmatch(r"\d+:\d+:\d+", sc["rule"]) for sc in scheds.values()):
        ap.error("rule is a, b or three words P:A:D")
    if any(any(k not in byz_keys for k in sc) and modes[name] not in ("crash", "partial", "subset")
           for name, sc in scheds.items()):
        ap.error("crash_count / crash_window / crash_at need mode:crash, mode:partial or mode:subset")
    if any("crash_cut" in sc and modes[name] != "partial" for name, sc in scheds.items()):
        ap.error("crash_cut needs mode:partial")
    if any("crash_reach" in sc and modes[name] != "subset" for name, sc in scheds.items()):
        ap.error("crash_reach needs mode:subset")

    def thresholds(name, N, F):
        """The `rule` pseudo-variable: Protocol A's or Protocol B's words at the shape, or the three words."""
        text = scheds[name].get("rule")
        if text is None:
            return {}
        if text in ("a", "b"):
            return {"thresholds": benor.rule_protocol_a(N, F) if text == "a" else benor.rule_protocol_b(N, F)}
        return {"thresholds": tuple(int(w) for w in text.split(":"))}

    def schedule(name, N, f):
        sc, kw = dict(scheds[name]), {}
        if modes[name] in ("byz", "byzb"):
            b, one = int(sc.get("byzantine", 0)), sc.get("byz_one", "0.5")
            coin = sc.get("coin_common")
            if coin is not None:
                kw["coin_common"] = 0xFFFFFFFF if coin == "all" else benor.reach_word(float(coin)) if "." in coin else int(coin)
            return {**kw, "byzantine": [f <= i < f + b for i in range(N)],
                    "byz_one": 0xFFFFFFFF if one == "all" else benor.reach_word(float(one)) if "." in one else int(one),
                    "byz_strategy": {"random": benor.BYZ_RANDOM, "oppose": benor.BYZ_OPPOSE, "balance": benor.BYZ_BALANCE,
                                     "split": benor.BYZ_SPLIT}[sc.get("byz_strategy", "random")]}
        cut = sc.pop("crash_cut", None)
        reach = sc.pop("crash_reach", None)
        if "crash_at" in sc:
            kw["crash_at"] = [None] * N
            for part in sc["crash_at"].split("+"):
                node, _, step = part.partition("@")
                kw["crash_at"][int(node)] = int(step)
        else:
            kw = {k: int(v) for k, v in sc.items()}
        if cut is not None:
            kw["crash_cut"] = benor.CUT_RANDOM if cut == "random" else int(cut)
        if reach is not None:
            kw["crash_reach"] = (benor.REACH_ALL if reach == "all" else
                                 benor.reach_word(float(reach)) if "." in reach else int(reach))
        return kw

    import numpy as np
    import torch

    class ClassLevel:
        """A LumpedPlan behind TrialsPlan's launch: blocking, its histograms kept on the host until take()."""

        def __init__(self, name, N, F, f):
            kw = schedule(name, N, f)
            self.plan = benor.LumpedPlan(N, F, f=f, b=sum(kw["byzantine"]), byz_even=(sum(kw["byzantine"]) + 1) // 2,
                                         rule=1 if modes[name] == "byzb" else 0, byz_strategy=kw["byz_strategy"],
                                         coin_common=kw.get("coin_common", 0), seed=0x5EED + N, k_max=32,
                                         **thresholds(name, N, F))
            self.hist_len = self.plan.hist_len
            self.host = np.zeros(self.hist_len, dtype=np.uint64)

        def launch(self, begin, count, hist_ptr, stream_ptr):
            self.host += self.plan.run(begin, count)

        def take(self):
            h, self.host = self.host, np.zeros(self.hist_len, dtype=np.uint64)
            return torch.from_numpy(h.astype(np.int64)).cuda()

    sys.path.insert(0, ROOT)
    from bench import node_rounds

    torch.cuda.set_device(0)
    st = torch.cuda.current_stream()

    def set_env(env):
        for k in knobs:
            os.environ.pop(k, None)
        os.environ.update(env)

    times, work, length = {}, {}, {}
    for N, F, T, f in shapes:
        dflt = benor.BO_MODE_RANDOM_DELIVERY if f < F else benor.BO_MODE_LOCKSTEP
        plans = {}                                    # one plan per delivery mode the variants name
        for name, _ in variants:
            mode = mode_ids[modes[name]] if modes[name] else dflt
            if "coin_common" in scheds[name]:
                mode = benor.BO_MODE_BYZ_COIN if modes[name] == "byz" else benor.BO_MODE_BYZ_RULE_B_COIN
            if scheds[name].get("delivery") == "adversarial":
                mode = benor.BO_MODE_SCHED_TALLY if modes[name] == "byz" else benor.BO_MODE_SCHED_RULE_B
            key = (mode, tuple(sorted(scheds[name].items())))
            if key not in plans and scheds[name].get("level") == "class":
                plans[key] = ClassLevel(name, N, F, f)
            if key not in plans:
                plans[key] = benor.TrialsPlan(N, F, [i < f for i in range(N)], seed=0x5EED + N, k_max=32, mode=mode,
                                              **schedule(name, N, f), **thresholds(name, N, F))
            plans[name] = plans[key]
        h = torch.zeros(plans[variants[0][0]].hist_len, dtype=torch.int64, device="cuda")
        for name, env in variants:                    # warm-up per variant (allocations, code load)
            set_env(env)
            plans[name].launch(0, max(1, T // 10), h.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        for plan in plans.values():
            if isinstance(plan, ClassLevel):
                plan.take()
        nxt = T
        for rnd in range(a.rounds):
            order = variants[rnd % len(variants):] + variants[:rnd % len(variants)]
            for name, env in order:
                set_env(env)
                h.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.reps):
                    plans[name].launch(nxt, T, h.data_ptr(), st.cuda_stream)
                    nxt += T
                e1.record(st)
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / a.reps
                if isinstance(plans[name], ClassLevel):
                    h += plans[name].take()
                times.setdefault((N, F, T, f, name), []).append(ms)
                nr, tr = node_rounds(h.cpu().numpy().astype(np.uint64), N - f, 32)
                work.setdefault((N, F, T, f, name), []).append(nr / a.reps / (ms * 1e-3))
                length.setdefault((N, F, T, f, name), []).append(tr / (a.reps * T))
    set_env({})
    for N, F, T, f in shapes:
        base = statistics.median(times[(N, F, T, f, variants[0][0])])
        for name, _ in variants:
            t = times[(N, F, T, f, name)]
            print(json.dumps({"N": N, "F": F, "f": f, "trials": T, "variant": name, "median_ms": statistics.median(t),
                              "min_ms": min(t), "max_ms": max(t), "rounds": len(t),
                              "median_vs_first": statistics.median(t) / base,
                              "trials_per_s": T / (statistics.median(t) * 1e-3),
                              "us_per_trial": statistics.median(t) * 1e3 / T, **scheds[name],
                              "ns_per_trial_round": statistics.median(t) * 1e6 / T / statistics.median(length[(N, F, T, f, name)]),
                              "ns_per_trial_round_min": min(t) * 1e6 / T / statistics.median(length[(N, F, T, f, name)]),
                              "ns_per_trial_round_max": max(t) * 1e6 / T / statistics.median(length[(N, F, T, f, name)]),
                              "node_rounds_per_s": statistics.median(work[(N, F, T, f, name)]),
                              "rounds_per_trial": statistics.median(length[(N, F, T, f, name)]),
                              "kernel_version": benor.kernel_version()}), flush=True)


if __name__ == "__main__":
    main()
