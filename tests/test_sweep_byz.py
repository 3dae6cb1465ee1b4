"""`sweep --mode byz|byzb`: the (N, F, b) phase diagram of the Byzantine modes.

Every (N, F) cell is crossed with b = floor(beta (F - f)), beta = i / S for i = 0..S (--byz-steps S, f =
--crashed); --cells also takes N:F:b.  Placement is `trials`': the first f nodes crashed, the next b
Byzantine.  The seed of a cell is seed ^ (N << 20) ^ F ^ (b << 44).  The grid, the parsing and the argument
errors need no device; the GPU tests compare a sweep with per-cell TrialsPlan runs, across stream counts and
across two ranks."""
import csv
import os
import socket
import subprocess
import sys

import pytest

import benor
from benor import cli
from conftest import PKG

SEED = 0x243F6A8885A308D3
HALF = 2 ** 31


def _sweep(*args, **kw):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "benor.cli", "sweep", *args], capture_output=True, text=True,
                          timeout=180, env=env, cwd=PKG, **kw)


# ------------------------------------------------------------------- CPU
def test_the_b_grid():
    assert cli.byz_grid([(64, 12)], 4) == [(64, 12, 0), (64, 12, 3), (64, 12, 6), (64, 12, 9), (64, 12, 12)]
    assert cli.byz_grid([(64, 12)], 4, crashed=2) == [(64, 12, 0), (64, 12, 2), (64, 12, 5), (64, 12, 7), (64, 12, 10)]
    assert cli.byz_grid([(10, 0), (10, 3)], 2) == [(10, 0, 0), (10, 0, 0), (10, 0, 0), (10, 3, 0), (10, 3, 1), (10, 3, 3)]
    assert cli.byz_grid([(26, 5)], 1) == [(26, 5, 0), (26, 5, 5)]
    for cells, steps, f in (([(64, 12), (128, 25)], 4, 0), ([(100, 33)], 7, 5), ([(4096, 819)], 16, 19)):
        grid = cli.byz_grid(cells, steps, f)
        assert len(grid) == len(cells) * (steps + 1)
        for k, (N, F, b) in enumerate(grid):
            i = k % (steps + 1)
            assert (N, F) == cells[k // (steps + 1)] and b == i * (F - f) // steps and f + b <= F
    with pytest.raises(SystemExit):
        cli.byz_grid([(64, 12)], 0)
    with pytest.raises(SystemExit, match="exceeds F"):
        cli.byz_grid([(64, 12), (64, 2)], 4, crashed=3)


def test_cells_parsing():
    assert cli.parse_cells("64:12,128:25") == [(64, 12), (128, 25)]
    assert cli.parse_cells("64:12:3,2**7:25", byz=True) == [(64, 12, 3), (128, 25)]
    with pytest.raises(SystemExit, match="N:F:b needs --mode byz"):
        cli.parse_cells("64:12:3")
    with pytest.raises(SystemExit, match="N:F or N:F:b"):
        cli.parse_cells("64:12:3:1", byz=True)
    with pytest.raises(SystemExit, match="N:F or N:F:b"):
        cli.parse_cells("64", byz=True)


def test_argument_errors_need_no_device():
    p = _sweep("--mode", "byzb", "--cells", "64:12:13")
    assert p.returncode != 0 and "crashed + b exceeds F in cells 64:12:13" in p.stderr
    p = _sweep("--mode", "byz", "--cells", "64:12:10", "--crashed", "3")
    assert p.returncode != 0 and "crashed + b exceeds F in cells 64:12:10" in p.stderr
    p = _sweep("--mode", "byz", "--cells", "64:2", "--crashed", "3")
    assert p.returncode != 0 and "exceeds F in cells 64:2" in p.stderr
    p = _sweep("--mode", "byzb", "--cells", "64:12", "--byz-steps", "0")
    assert p.returncode != 0 and "--byz-steps is at least 1" in p.stderr
    p = _sweep("--mode", "byzb", "--cells", "64:12", "--coin-common", "2")
    assert p.returncode != 0 and "--coin-common is a probability in [0, 1]" in p.stderr
    p = _sweep("--mode", "byzb", "--cells", "64:12", "--byz-one", "-1")
    assert p.returncode != 0 and "--byz-one is a probability in [0, 1]" in p.stderr
    p = _sweep("--mode", "byzb", "--cells", "64:12", "--byz-strategy", "both")
    assert p.returncode != 0 and "invalid choice" in p.stderr
    p = _sweep("--mode", "byzb", "--cells", "64:12:1:1")
    assert p.returncode != 0 and "N:F or N:F:b" in p.stderr
    for extra in (("--coin-common", "1"), ("--byz-steps", "4"), ("--byz-strategy", "split"), ("--byz-one", "0.5")):
        for mode in ("lockstep", "tally3"):
            p = _sweep("--mode", mode, "--cells", "64:12", *extra)
            assert p.returncode != 0 and "need --mode byz or --mode byzb" in p.stderr


# ------------------------------------------------------------------- GPU
N_CELLS = [(64, 12), (128, 25), (26, 5), (100, 40)]           # 2 x 2 (N, F) cells ...
PER_CELL = 500


def _cell_hist(mode, N, F, b, f, k_max, strategy, byz_one, coin):
    bo = {("byz", False): benor.BO_MODE_BYZ_TALLY, ("byzb", False): benor.BO_MODE_BYZ_RULE_B,
          ("byz", True): benor.BO_MODE_BYZ_COIN, ("byzb", True): benor.BO_MODE_BYZ_RULE_B_COIN}[mode, coin is not None]
    kw = {} if coin is None else {"coin_common": coin}
    plan = benor.TrialsPlan(N, F, [i < f for i in range(N)], seed=SEED ^ (N << 20) ^ F ^ (b << 44), k_max=k_max, mode=bo,
                            byzantine=[f <= i < f + b for i in range(N)], byz_one=byz_one, byz_strategy=strategy, **kw)
    return plan.run(0, PER_CELL)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,strategy,coin,f", [("byzb", "split", "1", 0), ("byzb", "random", None, 1),
                                                  ("byz", "balance", "0.5", 2), ("byz", "oppose", "0", 0)])
def test_sweep_equals_per_cell_plans(mode, strategy, coin, f, tmp_path):
    """... x 3 values of b, N <= 128, 500 trials per cell: every row is `summarize` of the cell's own plan."""
    import torch  # noqa: F401  (before libbenor.so: one HIP runtime in this process)

    out = tmp_path / "sweep.csv"
    args = ["--mode", mode, "--cells", ",".join(f"{N}:{F}" for N, F in N_CELLS), "--byz-steps", "2", "--per-cell", str(PER_CELL),
            "--k-max", "16", "--byz-strategy", strategy, "--crashed", str(f), "--out", str(out)]
    if coin is not None:
        args += ["--coin-common", coin]
    p = _sweep(*args)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = list(csv.DictReader(open(out)))
    assert len(rows) == len(N_CELLS) * 3
    word = None if coin is None else benor.reach_word(float(coin))
    code = {"random": benor.BYZ_RANDOM, "oppose": benor.BYZ_OPPOSE, "balance": benor.BYZ_BALANCE, "split": benor.BYZ_SPLIT}[strategy]
    for k, row in enumerate(rows):
        N, F = N_CELLS[k // 3]
        b = (k % 3) * (F - f) // 2
        assert (int(row["N"]), int(row["F"]), int(row["b"]), int(row["m"])) == (N, F, b, N - f)
        assert row["mode"] == mode and row["byz_strategy"] == strategy and int(row["byz_one_word"]) == HALF
        assert int(row["coin_common_word"]) == (word or 0) and int(row["trials"]) == PER_CELL
        want = cli.summarize(_cell_hist(mode, N, F, b, f, 16, code, HALF, word), N, F, 16, f)
        for key, v in want.items():
            assert row[key] == str(v), (k, key, row[key], v)


STREAM_ARGS = ["--mode", "byzb", "--N", "64,128", "--steps", "6", "--byz-steps", "2", "--per-cell", "501", "--k-max", "16",
               "--byz-strategy", "split", "--coin-common", "0.5"]


@pytest.mark.gpu
def test_sweep_streams(tmp_path):
    """1, 3 and 4 streams write byte-identical CSV: every cell has a plan of its own."""
    outs = []
    for streams in (1, 3, 4):
        out = tmp_path / f"s{streams}.csv"
        p = _sweep(*STREAM_ARGS, "--streams", str(streams), "--out", str(out))
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] == outs[2]
    assert len(outs[0].splitlines()) == 1 + 2 * 6 * 3


@pytest.mark.gpu
def test_sweep_two_ranks_equal_one(tmp_path):
    """Two ranks over gloo on one GPU write the CSV of one rank: the trials of a cell are keyed by the global trial
    id and the shared coin by trial and round."""
    one = tmp_path / "one.csv"
    p = _sweep(*STREAM_ARGS, "--out", str(one))
    assert p.returncode == 0, p.stdout + p.stderr
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    two = tmp_path / "two.csv"
    env = dict(os.environ, PYTHONPATH=PKG, BENOR_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "benor.cli", "sweep", *STREAM_ARGS,
                    "--out", str(two)], check=True, env=env, cwd=PKG, timeout=180)
    assert two.read_bytes() == one.read_bytes()
