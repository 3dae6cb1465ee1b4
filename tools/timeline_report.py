"""Summarise a BENOR_TIMELINE file -- the last launch in the file: the packed
matrix-core kernel's per-wave phase stamps (benor_mfma_small.h), or, where the
launch line says kernel=mfma, the KIND 0 matrix-core kernel's per-wave entry
and last-group stamps with the wave's group count and its XCC, SE and CU ids
(benor_mfma.h): the kernel span, the spread of the waves' end times, the idle
tail of every CU and XCD (from its last wave's end to the end of the span) and
the groups per wave.

    python tools/timeline_report.py <file> [--run N F TRIALS]

--run first launches N, F, TRIALS (random init, k_max 16) twice through the C
ABI with BENOR_TIMELINE=<file> (GPU; the first launch warms up).  Other knobs
(BENOR_MFMA_DYNAMIC, BENOR_BLOCKS_PER_CU, ...) are taken from the environment.

Stamps are the 100 MHz wall clock (10 ns ticks).  Per wave: [0] start, [1]
fresh round-1 batches exhausted, [2] round lists drained, [3] lane path done,
[4] histogram flushed; counts: fresh, r2 full, r3 full, r2 partial, r3
partial, lane-path passes.
"""
import os
import statistics
import sys


def last_launch(path):
    head, rows = None, []
    for line in open(path):
        if line.startswith("#"):
            head, rows = line.strip(), []
        elif line.strip():
            rows.append([int(x) for x in line.split(",")])
    return head, rows


def q(xs, f):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(f * len(xs)))]


def report_mfma(head, rows):
    """Columns: wave, entry stamp, last-group stamp, groups, XCC, SE, CU, HW_ID, claims."""
    t0, t1 = min(r[1] for r in rows), max(r[2] for r in rows)
    span = (t1 - t0) / 100.0
    pct = lambda ticks: 100.0 * (ticks / 100.0) / span
    print(head, f"({len(rows)} waves, {sum(1 for r in rows if r[3])} ran groups)")
    print(f"kernel span (first entry to last end): {span:.2f} us")
    starts = [r[1] - t0 for r in rows]
    print(f"wave entry after the first (us): median {statistics.median(starts) / 100.0:.2f}, "
          f"p90 {q(starts, 0.9) / 100.0:.2f}, max {max(starts) / 100.0:.2f}")
    ends = [r[2] for r in rows if r[3]]
    lo = min(ends)
    print("| wave end time minus the earliest end | us | % of span |")
    print("|---|---|---|")
    for name, v in (("p50", statistics.median(ends) - lo), ("p90", q(ends, 0.9) - lo), ("max", max(ends) - lo)):
        print(f"| {name} | {v / 100.0:.2f} | {pct(v):.2f} |")
    cu_last, xcd_last = {}, {}
    for r in rows:
        cu, xcd = (r[4], r[5], r[6]), r[4]
        cu_last[cu] = max(cu_last.get(cu, 0), r[2])
        xcd_last[xcd] = max(xcd_last.get(xcd, 0), r[2])
    print("| tail idle (last work to the end of the span) | units | mean % | median % | p90 % | max % |")
    print("|---|---|---|---|---|---|")
    for name, last in (("per CU", cu_last), ("per XCD", xcd_last)):
        xs = [pct(t1 - t) for t in last.values()]
        print(f"| {name} | {len(xs)} | {sum(xs) / len(xs):.2f} | {statistics.median(xs):.2f} | {q(xs, 0.9):.2f} | {max(xs):.2f} |")
    # Wave slots: a CU's waves in flight over time against its peak (the
    # resident waves); below 100 % its slots stood empty for part of the span
    # (a last round of fewer workgroups, or waves that ended early).
    fills, peaks = [], []
    by_cu = {}
    for r in rows:
        by_cu.setdefault((r[4], r[5], r[6]), []).append(r)
    for cu, mine in by_cu.items():
        ev = sorted([(r[1], 1) for r in mine] + [(r[2], -1) for r in mine])
        live = peak = 0
        for _, d in ev:
            live += d
            peak = max(peak, live)
        busy = sum(r[2] - r[1] for r in mine)
        fills.append(100.0 * busy / (peak * (t1 - t0)))
        peaks.append(peak)
    print(f"wave slots filled, per CU against its peak of {min(peaks)}..{max(peaks)} waves in flight: "
          f"mean {sum(fills) / len(fills):.2f} %, min {min(fills):.2f} %")
    for x in sorted(xcd_last):
        print(f"  XCD {x}: last work {(xcd_last[x] - t0) / 100.0:.2f} us, "
              f"{sum(1 for c in cu_last if c[0] == x)} CUs, {sum(r[3] for r in rows if r[4] == x)} groups")
    g = [r[3] for r in rows]
    print(f"groups per wave: min {min(g)}, mean {sum(g) / len(g):.2f}, max {max(g)}; "
          f"claims per wave: min {min(r[8] for r in rows)}, max {max(r[8] for r in rows)}")
    per_group = [(r[2] - r[1]) / 100.0 / r[3] for r in rows if r[3]]
    print(f"us per group and wave: min {min(per_group):.2f}, median {statistics.median(per_group):.2f}, "
          f"max {max(per_group):.2f}")


def report(path):
    head, rows = last_launch(path)
    if "kernel=mfma" in head:
        return report_mfma(head, rows)
    rows = [r for r in rows if r[1]]                  # waves that ran
    t0 = min(r[1] for r in rows)
    us = lambda t: (t - t0) / 100.0
    print(head, f"({len(rows)} waves ran)")
    cols = [("start", 1), ("fresh done", 2), ("lists drained", 3), ("lane path done", 4), ("flushed", 5)]
    print("| phase end (us after the first wave's start) | min | median | p90 | max |")
    print("|---|---|---|---|---|")
    for name, i in cols:
        xs = [us(r[i]) for r in rows]
        print(f"| {name} | {min(xs):.2f} | {statistics.median(xs):.2f} | {q(xs, 0.9):.2f} | {max(xs):.2f} |")
    print("| phase length (us) | min | median | p90 | max |")
    print("|---|---|---|---|---|")
    for (a, i), (b, j) in zip(cols, cols[1:]):
        xs = [(r[j] - r[i]) / 100.0 for r in rows]
        print(f"| {a} -> {b} | {min(xs):.2f} | {statistics.median(xs):.2f} | {q(xs, 0.9):.2f} | {max(xs):.2f} |")
    names = ["fresh", "r2 full", "r3 full", "r2 partial", "r3 partial", "lane passes"]
    print("| batches per wave | min | mean | max |")
    print("|---|---|---|---|")
    for k, nm in enumerate(names):
        xs = [r[6 + k] for r in rows]
        print(f"| {nm} | {min(xs)} | {sum(xs) / len(xs):.2f} | {max(xs)} |")
    last = max(rows, key=lambda r: r[5])
    print("slowest wave:", {n: last[6 + k] for k, n in enumerate(names)},
          "phases (us):", [round(us(last[i]), 2) for _, i in cols])


def run(path, N, F, trials):
    os.environ["BENOR_TIMELINE"] = path
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ben-or-consensus-algorithm_amd"))
    import benor
    faulty = [i < F for i in range(N)]
    for _ in range(2):
        plan = benor.TrialsPlan(N, F, faulty, seed=7, k_max=16)
        plan.run(0, trials)


if __name__ == "__main__":
    path = sys.argv[1]
    if len(sys.argv) > 2 and sys.argv[2] == "--run":
        if os.path.exists(path):
            os.remove(path)
        run(path, int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    report(path)
