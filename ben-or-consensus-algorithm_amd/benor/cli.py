"""Command-line driver.

    python -m benor.cli start [--N 10 --faulty 0,1,2,3 --init 1,1,...]   # src/start.ts
    python -m benor.cli trials --N 1024 --F 341 --trials 1000000          # one batch, JSON summary
    python -m benor.cli trials --N 1024 --F 341 --mode tally --crashed 0  # f = 0 crashed, count-level random delivery
    python -m benor.cli trials --N 10 --F 4 --mode tally3 --crashed 0     # the same for any quorum (ties, coins)
    python -m benor.cli trials --N 1024 --F 340 --mode crash --crashed 0 --crash-count 16 --crash-window 4
                                                                          # ... with 16 crashes in rounds 1-2
    python -m benor.cli trials --N 10 --F 4 --mode crash --crashed 1 --crash-at 3:0,7:1   # node 3 at step 0, node 7 at step 1
    python -m benor.cli trials --N 1024 --F 340 --mode partial --crashed 0 --crash-count 16 --crash-window 4 --crash-cut random
                                                                          # ... each crash cutting its last broadcast short
    python -m benor.cli trials --N 1024 --F 340 --mode subset --crashed 0 --crash-count 16 --crash-window 4 --crash-reach 0.5
                                                                          # ... or reaching each receiver with probability 1/2
    python -m benor.cli trials --N 1024 --F 340 --mode byz --crashed 0 --byzantine 100 --byz-one 0.5 --byz-strategy random
                                                                          # 100 Byzantine senders, a fair coin per receiver and step
    python -m benor.cli trials --N 1024 --F 204 --mode byzb --crashed 0 --byzantine 16 --byz-strategy split
                                                                          # ... under Ben-Or's Byzantine-tolerant rule (N > 5F)
    python -m benor.cli trials --N 1024 --F 204 --mode byzb --crashed 0 --byzantine 16 --byz-strategy split --coin-common 1
                                                                          # ... with a shared coin in every round
    python -m benor.cli trials --N 64 --F 20 --mode byz --crashed 0 --byzantine 0 --byz-strategy split --delivery adversarial
                                                                          # an adversarial scheduler, no Byzantine node
    python -m benor.cli trials --N 16777216 --F 9000 --mode byz --crashed 0 --byz-strategy balance --delivery adversarial --level class
                                                                          # ... at the level of classes: N up to 2**24
    python -m benor.cli trials --N 64 --F 20 --mode byzb --crashed 0 --byz-strategy split --delivery adversarial --rule a
                                                                          # Ben-Or's Protocol A under the scheduler (--rule b, --rule P:A:D)
    python -m benor.cli sweep --N 64,128,...,4096 --steps 32 --trials 2**30 --out sweep.csv
                                                                          # C5 phase diagram
    python -m benor.cli sweep --cells 4096:0,4096:1984 --per-cell 4793490  # two cells of it
    python -m benor.cli sweep --mode tally3 --crashed 0 --N 64,128 --steps 8  # the diagram under random delivery
    python -m benor.cli sweep --mode byzb --N 64,256 --steps 8 --byz-steps 4 --byz-strategy split --coin-common 1
                                                                          # the (N, F, b) diagram of the Byzantine modes

`start` re-states src/start.ts:6-43: same default scenario (N = 10, nodes
0-3 faulty, every initial value 1), same checks ("Lengths don't match",
"Too many faulty nodes" when F > N/2), then launchNetwork + startConsensus,
and prints every node's state.

`sweep` runs the decision-round phase diagram: every N in the list crossed
with F = floor(phi * N), phi on a `--steps` grid in [0, 0.5); the total trial
budget is split evenly over cells, each cell's trials split across ranks
(torch.distributed, one process per GPU).  All cells are launched back to back
into one [cells, H] histogram buffer, merged with a single all-reduce.  Rows: N, F, m, trials, decided fraction, E[R], P(R = 1..4), P(v = 1),
undecided, agreement violations.  `--mode tally3 --crashed f` draws the same
diagram under count-level random delivery (BO_MODE_RANDOM_TALLY3) with the first
f nodes of every cell crashed (f at most each cell's F; the rows' m is N - f).
`--mode byz` and `--mode byzb` (BO_MODE_BYZ_TALLY, BO_MODE_BYZ_RULE_B, and with
`--coin-common p` their shared-coin modes, with `--delivery adversarial` the
adversarial scheduler's modes, whose rows add a delivery column) cross every (N, F) cell with
b = floor(beta (F - f)) Byzantine nodes, beta = i / S for i = 0..S (`--byz-steps S`),
placed as `trials` places them: the first f nodes crashed, the next b Byzantine.
`--cells` then also takes N:F:b.  Their rows add b, mode, byz_strategy,
byz_one_word and coin_common_word.  `--level class` (with `--delivery adversarial`) runs
`trials` and `sweep` on the lumped chain (benor.LumpedPlan): the same
placement, N up to 2**24, a `level` field or column; `--level node` is the default.
`--rule a|b|P:A:D` (with `--mode byzb`, at either delivery and level) replaces Protocol B's rule
by a threshold rule of three words (a: Protocol A) and adds a `rule` field or column.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np


def _int(text: str) -> int:
    """A decimal integer, or a power written a**b (e.g. 2**30)."""
    base, sep, exp = text.strip().partition("**")
    return int(base) ** int(exp) if sep else int(base)


def _ints(s: str) -> list[int]:
    return [_int(part) for part in s.split(",") if part.strip()]


def summarize(hist: np.ndarray, N: int, F: int, k_max: int, crashed: int | None = None) -> dict:
    m = N - (F if crashed is None else crashed)
    trials = int(hist[:-1].sum())
    dec = np.array([int(hist[r * 3] + hist[r * 3 + 1] + hist[r * 3 + 2]) for r in range(1, k_max + 1)])
    decided = int(dec.sum())
    v1 = int(sum(hist[r * 3 + 1] for r in range(1, k_max + 1)))
    er = float((dec * np.arange(1, k_max + 1)).sum() / decided) if decided else float("nan")
    row = {"N": N, "F": F, "m": m, "trials": trials, "decided_frac": decided / trials if trials else 0.0,
           "E_R": er, "P_v1_given_decided": v1 / decided if decided else float("nan"),
           "undecided": int(hist[0] + hist[1] + hist[2]), "agreement_violations": int(hist[-1])}
    for r in range(1, 5):
        row[f"P_R{r}"] = (int(dec[r - 1]) / trials) if trials and r <= k_max else 0.0
    return row


def cmd_start(a) -> int:
    import benor

    N = a.N
    faulty_idx = set(_ints(a.faulty)) if a.faulty is not None else {0, 1, 2, 3}
    faulty = [i in faulty_idx for i in range(N)]
    init = [("?" if v == "?" else int(v)) for v in a.init.split(",")] if a.init else [1] * N
    if len(init) != len(faulty):                                   # start.ts:22-23
        raise benor.Error("Lengths don't match")
    if sum(faulty) > len(init) / 2:                                 # start.ts:25-29
        raise benor.Error("Too many faulty nodes")
    benor.launchNetwork(len(init), sum(faulty), init, faulty)       # start.ts:31-36
    benor.startConsensus(len(init), seed=a.seed, k_max=a.k_max)     # start.ts:40
    for i, s in enumerate(benor.getNodesState(len(init))):
        print(f"Node {i}: {json.dumps(s)}")
    return 0


_BYZ_STRATEGIES = ("random", "oppose", "balance", "split")


def byz_sched(a, benor) -> dict:
    """The --byz-strategy / --byz-one / --coin-common words of `trials` and `sweep` (mode byz or byzb)."""
    if not 0.0 <= a.byz_one <= 1.0:
        raise SystemExit("--byz-one is a probability in [0, 1]")
    sched = {"byz_one": benor.reach_word(a.byz_one),
             "byz_strategy": {"random": benor.BYZ_RANDOM, "oppose": benor.BYZ_OPPOSE, "balance": benor.BYZ_BALANCE,
                              "split": benor.BYZ_SPLIT}[a.byz_strategy]}
    if a.coin_common is not None:                                 # a shared coin
        if not 0.0 <= a.coin_common <= 1.0:
            raise SystemExit("--coin-common is a probability in [0, 1]")
        sched["coin_common"] = benor.reach_word(a.coin_common)
    return sched


def check_delivery(a) -> bool:
    """--delivery of `trials` and `sweep`: whether an adversarial scheduler delivers.  Its argument
    errors need no device."""
    if a.delivery != "adversarial":
        return False
    if a.mode not in ("byz", "byzb"):
        raise SystemExit("--delivery adversarial needs --mode byz or --mode byzb")
    if a.byz_strategy not in ("balance", "split"):
        raise SystemExit("--delivery adversarial needs --byz-strategy balance or --byz-strategy split")
    return True


def check_level(a, adversarial: bool) -> bool:
    """--level of `trials` and `sweep`: whether the adversarial scheduler runs at the level of classes (the lumped
    chain, DESIGN §4.3.12: N up to 2**24).  Its argument errors need no device."""
    if a.level != "class":
        return False
    if not adversarial:
        raise SystemExit("--level class needs --mode byz or --mode byzb with --delivery adversarial")
    return True


def check_rule(a):
    """--rule of `trials` and `sweep`: None, "a" or "b" (Protocol A's or Protocol B's words at each
    shape's (N, F)), or the three words (P, A, D).  It replaces Protocol B's rule, so it goes with --mode byzb, at
    either --delivery and --level.  Its argument errors need no device."""
    if a.rule is None:
        return None
    if a.mode != "byzb":
        raise SystemExit("--rule needs --mode byzb (it replaces Protocol B's rule)")
    if a.rule in ("a", "b"):
        return a.rule
    parts = a.rule.split(":")
    if len(parts) != 3 or not all(p.isdigit() for p in parts):
        raise SystemExit("--rule is a, b or three words P:A:D (propose_gt2:adopt_gt:decide_gt2)")
    import benor

    return benor.rule_check(tuple(int(p) for p in parts)).words     # the library's check of the words


def rule_of(rule, benor, N: int, F: int):
    """The benor.Rule of a checked --rule at a shape."""
    if rule == "a":
        return benor.rule_protocol_a(N, F)
    return benor.rule_protocol_b(N, F) if rule == "b" else benor.Rule(*rule, 0)


def rule_text(rule) -> str:
    return rule if isinstance(rule, str) else ":".join(str(w) for w in rule)


def lumped_words(a, benor, crashed: int, b: int) -> dict:
    """LumpedPlan's words for the placement `trials` and `sweep` use: the first `crashed` nodes crashed, the next b
    Byzantine -- the compact indices 0 .. b - 1, ceil(b / 2) of them even."""
    words = dict(f=crashed, b=b, byz_even=(b + 1) // 2, rule=1 if a.mode == "byzb" else 0,
                 byz_strategy=benor.BYZ_BALANCE if a.byz_strategy == "balance" else benor.BYZ_SPLIT)
    if a.coin_common is not None:
        words["coin_common"] = benor.reach_word(a.coin_common)
    return words


def byz_mode(a, benor) -> int:
    """BO_MODE_* of --mode byz / byzb: with --delivery adversarial the scheduler's mode, else with --coin-common
    the shared-coin mode."""
    if a.delivery == "adversarial":
        return benor.BO_MODE_SCHED_TALLY if a.mode == "byz" else benor.BO_MODE_SCHED_RULE_B
    if a.coin_common is not None:
        return benor.BO_MODE_BYZ_COIN if a.mode == "byz" else benor.BO_MODE_BYZ_RULE_B_COIN
    return benor.BO_MODE_BYZ_TALLY if a.mode == "byz" else benor.BO_MODE_BYZ_RULE_B


def cmd_trials(a) -> int:
    import benor

    mode = {"lockstep": benor.BO_MODE_LOCKSTEP, "random": benor.BO_MODE_RANDOM_DELIVERY,
            "tally": benor.BO_MODE_RANDOM_TALLY, "tally3": benor.BO_MODE_RANDOM_TALLY3,
            "crash": benor.BO_MODE_CRASH_TALLY, "partial": benor.BO_MODE_CRASH_PARTIAL,
            "subset": benor.BO_MODE_CRASH_SUBSET, "byz": benor.BO_MODE_BYZ_TALLY,
            "byzb": benor.BO_MODE_BYZ_RULE_B}[a.mode]
    crashed = a.F if a.crashed is None else a.crashed            # the first f nodes (start.ts:7-18 placement)
    adversarial = check_delivery(a)
    rule = check_rule(a)
    if check_level(a, adversarial):
        return trials_class(a, benor, crashed, rule)
    sched = {}
    if a.mode in ("crash", "partial", "subset"):                  # crashes during the run, in steps
        if a.crash_at and a.crash_count:
            raise SystemExit("--crash-at and --crash-count are exclusive")
        if a.crash_at:
            crash_at = [None] * a.N
            for part in a.crash_at.split(","):
                node, _, step = part.partition(":")
                if not 0 <= int(node) < a.N:
                    raise SystemExit(f"--crash-at: node {node} is not in [0, {a.N})")
                crash_at[int(node)] = int(step)
            sched = {"crash_at": crash_at}
        else:
            sched = {"crash_count": a.crash_count, "crash_window": a.crash_window}
    elif a.crash_at or a.crash_count:
        raise SystemExit("--crash-at / --crash-count need --mode crash, --mode partial or --mode subset")
    if a.mode == "partial":                                       # ... the last broadcast cut short
        if a.crash_cut is None or (a.crash_cut != "random" and not a.crash_cut.isdigit()):
            raise SystemExit("--mode partial needs --crash-cut: a count of initially-live receivers or 'random'")
        sched["crash_cut"] = benor.CUT_RANDOM if a.crash_cut == "random" else int(a.crash_cut)
    elif a.crash_cut is not None:
        raise SystemExit("--crash-cut needs --mode partial")
    if a.mode == "subset":                                        # ... reaching a random subset
        if a.crash_reach is None or not 0.0 <= a.crash_reach <= 1.0:
            raise SystemExit("--mode subset needs --crash-reach: a probability in [0, 1]")
        sched["crash_reach"] = benor.reach_word(a.crash_reach)
    elif a.crash_reach is not None:
        raise SystemExit("--crash-reach needs --mode subset")
    if a.mode in ("byz", "byzb"):                                 # Byzantine senders (byzb: §4.3.9)
        sched = byz_sched(a, benor)
        mode = byz_mode(a, benor)
        if not 0 <= a.byzantine <= a.N - crashed:
            raise SystemExit("--byzantine counts live nodes: 0 .. N - crashed")
        sched["byzantine"] = [crashed <= i < crashed + a.byzantine for i in range(a.N)]   # the live nodes after the crashed
    elif a.byzantine:
        raise SystemExit("--byzantine needs --mode byz or --mode byzb")
    elif a.coin_common is not None:
        raise SystemExit("--coin-common needs --mode byz or --mode byzb")
    if rule is not None:                                          # a threshold rule on mode byzb's plan
        sched["thresholds"] = rule_of(rule, benor, a.N, a.F)
    plan = benor.TrialsPlan(a.N, a.F, [i < crashed for i in range(a.N)], seed=a.seed, k_max=a.k_max, mode=mode,
                            **sched)
    t0 = time.perf_counter()
    h = plan.run(a.begin, a.trials)
    dt = time.perf_counter() - t0
    row = summarize(h, a.N, a.F, a.k_max)
    if a.mode != "lockstep" or a.crashed is not None:
        row.update(m=a.N - crashed, mode=a.mode, crashed=crashed, hist=[int(v) for v in h])
    if a.mode in ("crash", "partial", "subset"):                  # m is the initially-live count
        row.update(crash_count=a.crash_count, crash_window=a.crash_window, crash_at=a.crash_at,
                   kernel=benor.KERNEL_NAMES[plan.kernel])
    if a.mode == "partial":
        row.update(crash_cut=a.crash_cut)
    if a.mode == "subset":
        row.update(crash_reach=a.crash_reach, crash_reach_word=sched["crash_reach"])
    if a.mode in ("byz", "byzb"):
        row.update(byzantine=a.byzantine, byz_one=a.byz_one, byz_one_word=sched["byz_one"], byz_strategy=a.byz_strategy,
                   kernel=benor.KERNEL_NAMES[plan.kernel])
        if a.coin_common is not None:
            row.update(coin_common=a.coin_common, coin_common_word=sched["coin_common"])
        if adversarial:
            row.update(delivery=a.delivery)
        if rule is not None:
            row.update(rule=rule_text(rule), rule_words=list(sched["thresholds"].words))
    row["seconds"] = dt
    print(json.dumps(row))
    return 0


def trials_class(a, benor, crashed: int, rule=None) -> int:
    """`trials --level class`: the batch on the lumped chain, the row of the node level plus a level field (and with
    --rule its rule fields)."""
    if not 0.0 <= a.byz_one <= 1.0:
        raise SystemExit("--byz-one is a probability in [0, 1]")
    if a.coin_common is not None and not 0.0 <= a.coin_common <= 1.0:
        raise SystemExit("--coin-common is a probability in [0, 1]")
    if not 0 <= a.byzantine <= a.N - crashed:
        raise SystemExit("--byzantine counts live nodes: 0 .. N - crashed")
    words = lumped_words(a, benor, crashed, a.byzantine)
    thresholds = None if rule is None else rule_of(rule, benor, a.N, a.F)
    plan = benor.LumpedPlan(a.N, a.F, seed=a.seed, k_max=a.k_max, thresholds=thresholds, **words)
    t0 = time.perf_counter()
    h = plan.run(a.begin, a.trials)
    dt = time.perf_counter() - t0
    row = summarize(h, a.N, a.F, a.k_max)
    row.update(m=a.N - crashed, mode=a.mode, crashed=crashed, hist=[int(v) for v in h], byzantine=a.byzantine,
               byz_even=words["byz_even"], byz_strategy=a.byz_strategy)
    if a.coin_common is not None:
        row.update(coin_common=a.coin_common, coin_common_word=words["coin_common"])
    row.update(delivery=a.delivery, level=a.level)
    if rule is not None:
        row.update(rule=rule_text(rule), rule_words=list(plan.rule.words))
    row.update(seconds=dt)
    print(json.dumps(row))
    return 0


def byz_grid(cells, steps: int, crashed: int = 0):
    """Every (N, F) cell crossed with b = floor(beta (F - crashed)), beta = i / steps, i = 0..steps."""
    if steps < 1:
        raise SystemExit("--byz-steps is at least 1")
    bad = [f"{N}:{F}" for (N, F) in cells if crashed > F]
    if bad:
        raise SystemExit(f"sweep --crashed {crashed} exceeds F in cells {','.join(bad)}")
    return [(N, F, i * (F - crashed) // steps) for (N, F) in cells for i in range(steps + 1)]


def parse_cells(text: str, byz: bool = False):
    """--cells: N:F,N:F,...; with `byz` also N:F:b."""
    cells = [tuple(_int(x) for x in c.split(":")) for c in text.split(",")]
    if byz and any(len(c) not in (2, 3) for c in cells):
        raise SystemExit("--cells takes N:F or N:F:b")
    if not byz and any(len(c) == 3 for c in cells):
        raise SystemExit("--cells N:F:b needs --mode byz or --mode byzb")
    return cells


def sweep_byz_cells(a):
    """The (N, F, b) cells of `sweep --mode byz|byzb` and their argument checks (no device needed)."""
    crashed = 0 if a.crashed is None else a.crashed
    if crashed < 0:
        raise SystemExit("--crashed counts nodes")
    if a.cells:
        cells = []
        for c in parse_cells(a.cells, byz=True):
            cells += [c] if len(c) == 3 else byz_grid([c], a.byz_steps, crashed)
    else:
        cells = byz_grid(grid_cells(_ints(a.N), a.steps), a.byz_steps, crashed)
    bad = [f"{N}:{F}:{b}" for (N, F, b) in cells if b < 0 or crashed + b > F]
    if bad:
        raise SystemExit(f"sweep: crashed + b exceeds F in cells {','.join(bad)}")
    return cells, crashed


def cmd_sweep(a) -> int:
    byz = a.mode in ("byz", "byzb")
    adversarial = check_delivery(a)
    level_class = check_level(a, adversarial)
    rule = check_rule(a)
    if not byz and (a.coin_common is not None or a.byz_steps is not None or a.byz_strategy is not None or
                    a.byz_one is not None):
        raise SystemExit("--byz-steps / --byz-strategy / --byz-one / --coin-common need --mode byz or --mode byzb")
    if byz:                                                       # argument errors before the device is touched
        import benor

        a.byz_steps = 4 if a.byz_steps is None else a.byz_steps
        a.byz_strategy = "random" if a.byz_strategy is None else a.byz_strategy
        a.byz_one = 0.5 if a.byz_one is None else a.byz_one
        byz_cells, byz_crashed = sweep_byz_cells(a)
        sched = byz_sched(a, benor)

    import torch

    import benor
    from benor.parallel import merge_histogram, strong_range

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist

        backend = os.environ.get("BENOR_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(backend)
    if byz:
        cells = byz_cells
    elif a.cells:
        # selected cells of a full sweep, re-run at that sweep's per-cell budget (--per-cell):
        # a cell's rows depend only on (N, F, seed, per-cell trials, k_max)
        cells = parse_cells(a.cells)
    else:
        cells = grid_cells(_ints(a.N), a.steps)
    per_cell = _int(str(a.per_cell)) if a.per_cell else max(1, _int(str(a.trials)) // len(cells))
    if a.mode == "lockstep" and a.crashed is not None:
        raise SystemExit("sweep --crashed needs --mode tally3 (lockstep crashes exactly F nodes per cell)")
    if byz:
        rows, elapsed = run_sweep(cells, per_cell, a.seed, a.k_max, a.streams, rank, world, a.progress,
                                  mode=a.mode, crashed=byz_crashed, byz=dict(sched, strategy_name=a.byz_strategy),
                                  delivery="adversarial" if adversarial else "random",
                                  level="class" if level_class else "node", rule=rule)
    elif a.mode == "tally3":
        crashed = 0 if a.crashed is None else a.crashed
        bad = [f"{N}:{F}" for (N, F) in cells if crashed > F]
        if bad:
            raise SystemExit(f"sweep --crashed {crashed} exceeds F in cells {','.join(bad)}")
        rows, elapsed = run_sweep(cells, per_cell, a.seed, a.k_max, a.streams, rank, world, a.progress,
                                  mode="tally3", crashed=crashed)
    else:
        rows, elapsed = run_sweep(cells, per_cell, a.seed, a.k_max, a.streams, rank, world, a.progress)
    if rank == 0:
        out = open(a.out, "w") if a.out else sys.stdout
        out.write(rows_csv(rows))
        if a.out:
            out.close()
        total = per_cell * len(cells)
        print(json.dumps({"cells": len(cells), "trials": total, "seconds": elapsed, "gpus": world}), file=sys.stderr)
    return 0


def grid_cells(Ns: list[int], steps: int) -> list[tuple[int, int]]:
    """C5 cells: every N crossed with F = floor(phi N), phi on a `steps` grid in [0, 0.5)."""
    phis = [i * 0.5 / steps for i in range(steps)]
    return [(N, int(phi * N)) for N in Ns for phi in phis]


def rows_csv(rows: list[dict]) -> str:
    keys = list(rows[0].keys())
    return ",".join(keys) + "\n" + "".join(",".join(str(r[k]) for k in keys) + "\n" for r in rows)


def run_sweep(cells, per_cell, seed, k_max, streams_n=4, rank=0, world=1, progress=False, mode="lockstep",
              crashed=None, byz=None, delivery="random", level="node", rule=None):
    """The sweep's GPU work on the current device: (rows, seconds).  Under
    torch.distributed (world > 1) each cell's trials are split over the ranks
    and the histograms merged by one all-reduce.  mode "lockstep": F crashed
    per cell; "tally3": BO_MODE_RANDOM_TALLY3 with the first `crashed` nodes of
    every cell crashed (a count, at most each cell's F; default 0).  "byz" and
    "byzb": cells are (N, F, b), the first `crashed` nodes crashed and the next b
    Byzantine; `byz` holds byz_one and byz_strategy (words), strategy_name for the
    rows, and with coin_common the shared-coin modes' word; `delivery` "adversarial"
    runs them under the adversarial scheduler (byz_strategy balance or split), and
    the rows then add a delivery column; `level` "class" runs those on the lumped chain
    (benor.LumpedPlan: N up to 2**24; blocking launches, cell after cell) and adds a level column.  `rule` (mode
    "byzb"): "a", "b" or three words, a threshold rule in the place of Protocol B's on every cell's plan (the presets
    at the cell's own (N, F)); the rows then add a rule column."""
    import torch

    import benor
    from benor.parallel import merge_histogram, strong_range

    # The device context comes up before the clock starts (~0.08 s on a fresh
    # process): "seconds" times the sweep -- plans, launches, merge, read-back.
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stream = torch.cuda.current_stream()
    # Every cell's plan first, then all launches back to back into one [cells, H]
    # histogram buffer, then ONE all-reduce over ranks and one read-back.  Cells go
    # round-robin over --streams streams: each plan owns its buffers, so cells are
    # independent, and one cell's short passes (deferred-trial rounds, the last
    # groups of a launch) overlap the next cell's launches instead of idling CUs.
    if delivery not in ("random", "adversarial") or (delivery == "adversarial" and mode not in ("byz", "byzb")):
        raise ValueError("delivery is 'random', or 'adversarial' with mode 'byz' or 'byzb'")
    if level not in ("node", "class") or (level == "class" and delivery != "adversarial"):
        raise ValueError("level is 'node', or 'class' with delivery 'adversarial'")
    if rule is not None and mode != "byzb":
        raise ValueError("rule needs mode 'byzb' (it replaces Protocol B's rule)")
    if mode == "lockstep":
        if crashed is not None:
            raise ValueError("crashed needs mode 'tally3' (lockstep crashes exactly F nodes per cell)")
        plans = [benor.TrialsPlan(N, F, seed=seed ^ (N << 20) ^ F, k_max=k_max) for (N, F) in cells]
    elif mode == "tally3":
        crashed = 0 if crashed is None else crashed
        if any(crashed > F for (_, F) in cells):
            raise ValueError(f"crashed = {crashed} exceeds a cell's F")
        plans = [benor.TrialsPlan(N, F, [i < crashed for i in range(N)], seed=seed ^ (N << 20) ^ F, k_max=k_max,
                                  mode=benor.BO_MODE_RANDOM_TALLY3) for (N, F) in cells]
    elif mode in ("byz", "byzb"):
        crashed = 0 if crashed is None else crashed
        byz = dict(byz or {})
        name = byz.pop("strategy_name", None)
        byz.setdefault("byz_one", benor.reach_word(0.5))
        byz.setdefault("byz_strategy", benor.BYZ_RANDOM)
        if name is None:
            name = {benor.BYZ_RANDOM: "random", benor.BYZ_OPPOSE: "oppose", benor.BYZ_BALANCE: "balance",
                    benor.BYZ_SPLIT: "split"}[byz["byz_strategy"]]
        if any(crashed + b > F for (_, F, b) in cells):
            raise ValueError("crashed + b exceeds a cell's F")
        coin = "coin_common" in byz
        bo_mode = {("byz", False): benor.BO_MODE_BYZ_TALLY, ("byzb", False): benor.BO_MODE_BYZ_RULE_B,
                   ("byz", True): benor.BO_MODE_BYZ_COIN, ("byzb", True): benor.BO_MODE_BYZ_RULE_B_COIN}[mode, coin]
        if delivery == "adversarial":
            bo_mode = benor.BO_MODE_SCHED_TALLY if mode == "byz" else benor.BO_MODE_SCHED_RULE_B
        def thresholds(N, F):                    # (no keyword at all without a rule: the plans are what they were)
            return {} if rule is None else {"thresholds": rule_of(rule, benor, N, F)}

        if level == "class":                     # the same placement: compact indices 0 .. b - 1 Byzantine
            plans = [benor.LumpedPlan(N, F, f=crashed, b=b, byz_even=(b + 1) // 2, rule=1 if mode == "byzb" else 0,
                                      byz_strategy=byz["byz_strategy"], coin_common=byz.get("coin_common", 0),
                                      seed=seed ^ (N << 20) ^ F ^ (b << 44), k_max=k_max, **thresholds(N, F))
                     for (N, F, b) in cells]
        else:
            plans = [benor.TrialsPlan(N, F, [i < crashed for i in range(N)], seed=seed ^ (N << 20) ^ F ^ (b << 44),
                                      k_max=k_max, mode=bo_mode,
                                      byzantine=[crashed <= i < crashed + b for i in range(N)], **byz, **thresholds(N, F))
                     for (N, F, b) in cells]
    else:
        raise ValueError(f"mode must be 'lockstep', 'tally3', 'byz' or 'byzb': {mode!r}")
    H = plans[0].hist_len
    hists = torch.zeros((len(cells), H), dtype=torch.int64, device="cuda")
    streams = [stream] + [torch.cuda.Stream() for _ in range(max(1, streams_n) - 1)]
    for s in streams[1:]:
        s.wait_stream(stream)                      # the zeroed histograms
    b, n = strong_range(0, per_cell, rank, world)
    for ci, plan in enumerate(plans):
        if level == "class":
            hists[ci] = torch.from_numpy(plan.run(b, n).astype(np.int64)).to(hists.device)
        else:
            plan.launch(b, n, hists[ci].data_ptr(), streams[ci % len(streams)].cuda_stream)
        if rank == 0 and progress:
            print(f"[{ci + 1}/{len(cells)}] N={cells[ci][0]} F={cells[ci][1]} queued", file=sys.stderr, flush=True)
    for s in streams[1:]:
        stream.wait_stream(s)
    merge_histogram(hists)
    allh = hists.cpu().numpy().astype(np.uint64)
    rows = [summarize(allh[ci], c[0], c[1], k_max, crashed) for ci, c in enumerate(cells)]
    if mode in ("byz", "byzb"):
        for row, (_, _, b) in zip(rows, cells):
            row.update(b=b, mode=mode, byz_strategy=name, byz_one_word=byz["byz_one"],
                       coin_common_word=byz.get("coin_common", 0))
            if delivery == "adversarial":
                row.update(delivery=delivery)
            if level == "class":
                row.update(level=level)
            if rule is not None:
                row.update(rule=rule_text(rule))
    elapsed = time.perf_counter() - t0
    for plan in plans if level == "node" else ():
        plan.check()                               # device-side capacity invariants of every cell
    return rows, elapsed


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="benor")
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("start", help="src/start.ts scenario")
    s.add_argument("--N", type=int, default=10)
    s.add_argument("--faulty", default=None, help="comma-separated faulty node ids (default 0,1,2,3)")
    s.add_argument("--init", default=None, help="comma-separated initial values 0/1/? (default all 1)")
    s.add_argument("--seed", type=int, default=None)
    s.add_argument("--k-max", type=int, default=64)
    t = sub.add_parser("trials", help="one batch of independent trials")
    t.add_argument("--N", type=int, default=1024)
    t.add_argument("--F", type=int, default=341)
    t.add_argument("--trials", type=int, default=1_000_000)
    t.add_argument("--begin", type=int, default=0)
    t.add_argument("--seed", type=int, default=0x243F6A8885A308D3)
    t.add_argument("--k-max", type=int, default=16)
    t.add_argument("--mode", choices=["lockstep", "random", "tally", "tally3", "crash", "partial", "subset", "byz", "byzb"],
                   default="lockstep",
                   help="delivery model: lockstep, random (mask-level), tally (count-level random delivery: odd "
                        "quorum, no '?'), tally3 (count-level, any quorum), crash (tally3 with crashes during the run), "
                        "partial (crash with the crasher's last broadcast reaching a prefix of the receivers) or "
                        "subset (... reaching each receiver independently with probability --crash-reach); byz (tally3 "
                        "with --byzantine senders that lie); byzb (byz under Ben-Or's Byzantine-tolerant rule, F as its t)")
    t.add_argument("--crashed", type=int, default=None,
                   help="crash the first f nodes (default F; random, tally, tally3 and crash take f <= F)")
    t.add_argument("--crash-count", type=int, default=0,
                   help="crash: this many initially-live nodes crash, drawn per trial (f + count <= F)")
    t.add_argument("--crash-window", type=int, default=0,
                   help="crash: ... at uniform steps below this (step 2(r-1): R-phase of round r, +1: its P-phase)")
    t.add_argument("--crash-at", default=None, help="crash: explicit schedule node:step,node:step,...")
    t.add_argument("--crash-cut", default=None,
                   help="partial: every crasher's last message reaches this many initially-live nodes, in ascending "
                        "node id (0: nobody, as crash; N - f: everybody), or 'random': uniform per trial and crasher")
    t.add_argument("--crash-reach", type=float, default=None,
                   help="subset: the probability in [0, 1] that a crasher's last message reaches a receiver (0: nobody, "
                        "as crash; 1: everybody), independently per trial, crasher and receiver")
    t.add_argument("--byzantine", type=int, default=0,
                   help="byz: the b live nodes after the --crashed ones are Byzantine (they send at every step and lie; "
                        "crashed + b <= F)")
    t.add_argument("--byz-one", type=float, default=0.5,
                   help="byz: the probability in [0, 1] that a Byzantine message carries 1, independently per trial, "
                        "sender, receiver and step")
    t.add_argument("--byz-strategy", choices=["random", "oppose", "balance", "split"], default="random",
                   help="byz: random (each message by --byz-one), oppose (every message carries the value fewer honest "
                        "senders hold; --byz-one on a tie), balance (the liars in a receiver's inbox see its honest "
                        "messages and make its two tallies as equal as they can) or split (they say 1 to receivers of odd "
                        "compact index and 0 to the others); the last two do not read --byz-one")
    t.add_argument("--delivery", choices=["random", "adversarial"], default="random",
                   help="byz, byzb: who composes a receiver's inbox: random (a uniform draw of N - F of the live senders) "
                        "or adversarial (a scheduler picks the N - F messages and the lies, BO_MODE_SCHED_TALLY and "
                        "BO_MODE_SCHED_RULE_B; needs --byz-strategy balance or split, allows --byzantine 0)")
    t.add_argument("--level", choices=["node", "class"], default="node",
                   help="byz, byzb with --delivery adversarial: node (one bit per node, N <= 4096) or class (the lumped "
                        "chain over the two receiver parities, N <= 2**24; the same law, another random stream)")
    t.add_argument("--coin-common", type=float, default=None,
                   help="byz, byzb: a shared coin (BO_MODE_BYZ_COIN, BO_MODE_BYZ_RULE_B_COIN): the probability in [0, 1] "
                        "that a round's coin is common to all honest nodes (0: the mode without it)")
    rule_help = ("byzb: a threshold rule in the place of Protocol B's (DESIGN §4.3.13): a (Ben-Or's crash-tolerant "
                 "Protocol A, the words (N, 0, 2F)), b (Protocol B's own words, (N + F, F, N + F)) or three words "
                 "P:A:D -- propose v iff 2 c_v > P, adopt v iff c_v > A, decide iff also 2 c_v > D; at either "
                 "--delivery and --level")
    t.add_argument("--rule", default=None, help=rule_help)
    w = sub.add_parser("sweep", help="C5 decision-round phase diagram")
    w.add_argument("--N", default="64,128,256,512,1024,2048,4096")
    w.add_argument("--steps", type=int, default=32)
    w.add_argument("--trials", default="2**30")
    w.add_argument("--seed", type=int, default=0x243F6A8885A308D3)
    w.add_argument("--k-max", type=int, default=32)
    w.add_argument("--cells", default=None, help="N:F,N:F,... instead of the N x phi grid (byz, byzb: also N:F:b)")
    w.add_argument("--per-cell", default=None, help="trials per cell (default: --trials / cells)")
    w.add_argument("--streams", type=int, default=4, help="HIP streams the cells are spread over")
    w.add_argument("--mode", choices=["lockstep", "tally3", "byz", "byzb"], default="lockstep",
                   help="delivery model of every cell: lockstep (F crashed), tally3 (count-level random delivery), "
                        "byz (tally3 with Byzantine senders) or byzb (byz under Ben-Or's Byzantine-tolerant rule)")
    w.add_argument("--crashed", type=int, default=None,
                   help="tally3, byz, byzb: crash the first f nodes of every cell (default 0; at most each cell's F)")
    w.add_argument("--byz-steps", type=int, default=None,
                   help="byz, byzb: every (N, F) cell is crossed with b = floor(i / S (F - f)), i = 0..S (default 4)")
    w.add_argument("--byz-strategy", choices=list(_BYZ_STRATEGIES), default=None, help="byz, byzb: as in `trials`")
    w.add_argument("--byz-one", type=float, default=None, help="byz, byzb: as in `trials` (default 0.5)")
    w.add_argument("--coin-common", type=float, default=None, help="byz, byzb: as in `trials`")
    w.add_argument("--delivery", choices=["random", "adversarial"], default="random", help="byz, byzb: as in `trials`")
    w.add_argument("--level", choices=["node", "class"], default="node",
                   help="byz, byzb with --delivery adversarial: node (one bit per node, N <= 4096) or class (the lumped "
                        "chain over the two receiver parities, N <= 2**24; the same law, another random stream)")
    w.add_argument("--rule", default=None, help=rule_help + " (a and b: at every cell's own (N, F))")
    w.add_argument("--out", default=None)
    w.add_argument("--progress", action="store_true")
    a = ap.parse_args(argv)
    return {"start": cmd_start, "trials": cmd_trials, "sweep": cmd_sweep}[a.cmd](a)


if __name__ == "__main__":
    sys.exit(main())
