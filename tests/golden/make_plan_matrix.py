"""Generate tests/golden/plan_matrix.json: what bo_kernel_for (host only) answers
for a grid of trial configurations -- the kernel family, or the error code and
the full bo_last_error text.  tests/test_plan_matrix.py replays the grid on the
library under test and asserts equality, so a change to the planner's
validation, mode demotions, kernel choice or error texts shows as a diff.

A row is [mode, N, F, f, b, three, init, sched, n_sched, count, window, cut]:
  f nodes crashed from the start (faulty 1), then b nodes with faulty 2, then
  `three` nodes with faulty 3;
  init 0 random, 1 fixed 0/1 alternating, 2 the same with a "?" on the last node;
  sched 0 no crash_at, 1 n_sched of the last nodes at steps 0, 1, 2, ..,
  2 all of them at step 2, 3 all of them beyond step 2 k_max;
  count, window, cut: the configuration words crash_count (byz_strategy),
  crash_window (coin_common) and crash_cut (crash_reach, byz_one), as they are.
The fixture holds no rows, only grid()'s digest and one outcome per row in grid()'s
order: the kernel family (BO_OK), or ERROR_BASE + i for "errors"[i] = [code, text].

Run (no BENOR_* knob set):  python tests/golden/make_plan_matrix.py
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "ben-or-consensus-algorithm_amd"))

import benor  # noqa: E402

K_MAX = 8
ERROR_BASE = 100                              # outcomes below it are BO_KERNEL_* values
NEVER = 0xFFFFFFFF
U32 = 0xFFFFFFFF
SHAPES = [(1, 0), (4, 1), (11, 2), (26, 5), (33, 16), (64, 12), (65, 21), (256, 51), (257, 85), (1024, 340),
          (4096, 819)]
MODES = list(range(15))                       # the 14 modes and the unknown mode 14
CRASH_MODES = (5, 6, 7)
BYZ_MODES = (8, 9, 10, 11, 12, 13)
STRATEGIES = (0, 1, 2, 3, 4, 5)               # RANDOM, OPPOSE, (2: none), BALANCE, SPLIT, (5: none)
COINS = (0, 1, U32)


def tally_table_len(m, q):
    """Thresholds of the table of (m, q) (include/benor.h, BO_CRASH_TABLE_MAX_BYTES)."""
    return sum(min(K, q) - max(0, q - (m - K)) for K in range(m + 1))


def table_limit_rows():
    """N = 4096, F = 2048, nobody faulty: a random schedule of c crashes needs the tables of the live
    counts 4096 - d, d = 0..c; 15 crashes fit BO_CRASH_TABLE_MAX_BYTES and 16 do not."""
    N, F = 4096, 2048
    need = [8 * sum(tally_table_len(N - d, N - F) for d in range(c + 1)) for c in (15, 16)]
    assert need[0] <= benor.CRASH_TABLE_MAX_BYTES < need[1], need
    return [[mode, N, F, 0, 0, 0, 0, 0, 0, c, 1, 0] for mode in CRASH_MODES for c in (15, 16)]


def grid():
    rows = []
    for mode in MODES:
        for N, F in SHAPES:
            for f in (0, F, F + 1):
                for init in (0, 1, 2):
                    rows.append([mode, N, F, f, 0, 0, init, 0, 0, 0, 0, 0])
            rows.append([mode, N, F, 0, 0, 1, 0, 0, 0, 0, 0, 0])           # a faulty entry of 3
            # the schedule words, in every mode (most do not read them)
            rows.append([mode, N, F, 0, 0, 0, 0, 1, 1, 0, 0, 0])
            rows.append([mode, N, F, 0, 0, 0, 0, 0, 0, 1, 1, 0])
            if mode in BYZ_MODES:
                for f in (0, F, F + 1):
                    for b in sorted({0, 1, max(F - f, 0), max(F - f + 1, 0)}):
                        for coin in COINS:
                            rows.append([mode, N, F, f, b, 0, 0, 0, 0, 3, coin, 0])
                        for init in (1, 2):
                            rows.append([mode, N, F, f, b, 0, init, 0, 0, 4, 1, 1 << 31])
                for b in (0, min(1, F)):
                    for strategy in STRATEGIES:
                        rows.append([mode, N, F, 0, b, 0, 0, 0, 0, strategy, 1, 12345])
                rows.append([mode, N, F, 0, min(1, F), 1, 0, 0, 0, 3, 1, 0])   # a Byzantine node and an entry of 3
            if mode in CRASH_MODES:
                for f in (0, F):
                    m = N - min(f, N)
                    scheds = [(1, 1, 0, 0), (2, 2, 0, 0), (3, 1, 0, 0), (0, 0, 1, 0), (0, 0, 1, 1),
                              (1, F - f, 0, 0), (1, F - f + 1, 0, 0), (0, 0, F - f, 1), (0, 0, F - f + 1, 1)]
                    for sched, n, count, window in scheds:
                        for cut in (0, m, m + 1, U32):
                            rows.append([mode, N, F, f, 0, 0, 0, sched, n, count, window, cut])
                rows.append([mode, N, F, 0, 0, 0, 2, 1, 1, 0, 0, 0])       # a schedule and a "?"
    rows += table_limit_rows()
    seen, out = set(), []
    for r in rows:
        if tuple(r) not in seen:
            seen.add(tuple(r))
            out.append(r)
    return out


def config(row):
    """The bo_trials_cfg of a row, and the arrays it points into."""
    mode, N, F, f, b, three, init, sched, n_sched, count, window, cut = row
    faulty = (ctypes.c_uint8 * max(1, N))()
    for i in range(N):
        faulty[i] = 1 if i < f else 2 if i < f + b else 3 if i < f + b + three else 0
    values = (ctypes.c_int8 * max(1, N))()
    if init:
        for i in range(N):
            values[i] = i & 1
        if init == 2:
            values[N - 1] = 2
    crash = None
    if sched:
        crash = (ctypes.c_uint32 * max(1, N))(*([NEVER] * max(1, N)))
        for j in range(min(n_sched, N)):
            crash[N - 1 - j] = {1: j % (2 * K_MAX), 2: 2, 3: 2 * K_MAX + 1}[sched]
    cfg = benor.TrialsCfgC(N, F, K_MAX, benor.BO_INIT_FIXED if init else benor.BO_INIT_RANDOM, mode, cut, 0,
                           ctypes.cast(faulty, ctypes.POINTER(ctypes.c_uint8)),
                           ctypes.cast(values, ctypes.POINTER(ctypes.c_int8)),
                           ctypes.cast(crash, ctypes.POINTER(ctypes.c_uint32)) if crash else None, count, window)
    return cfg, (faulty, values, crash)


def outcome(row):
    """(rc, kernel family) or (rc, error text) of bo_kernel_for on the row's configuration."""
    cfg, _keep = config(row)
    k = ctypes.c_int(-99)
    rc = benor.lib().bo_kernel_for(ctypes.byref(cfg), ctypes.byref(k))
    return (rc, k.value) if rc == benor.BO_OK else (rc, benor.last_error())


def grid_digest(rows):
    """Pins the fixture to the grid it was made for: the rows themselves are not stored."""
    return hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()[:16]


def main():
    assert not [k for k in os.environ if k in benor.KNOBS], "unset every BENOR_* knob first"
    rows = grid()
    errors, codes = [], []
    for row in rows:
        rc, what = outcome(row)
        if rc != benor.BO_OK:
            if [rc, what] not in errors:
                errors.append([rc, what])
            what = ERROR_BASE + errors.index([rc, what])
        codes.append(what)
    with open(os.path.join(HERE, "plan_matrix.json"), "w") as f:
        head = {"generator": "tests/golden/make_plan_matrix.py", "k_max": K_MAX, "rows": len(rows),
                "grid_sha256": grid_digest(rows), "errors": errors}
        f.write(json.dumps(head, indent=1)[:-2] + ',\n "outcomes": [\n')
        lines = [",".join(str(c) for c in codes[i:i + 60]) for i in range(0, len(codes), 60)]
        f.write(",\n".join(lines) + "\n ]\n}\n")
    print(f"{len(rows)} rows, {len(errors)} error texts, {sum(1 for c in codes if c >= ERROR_BASE)} errors")


if __name__ == "__main__":
    main()
