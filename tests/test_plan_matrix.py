"""The planner's answers over a grid of configurations (host only): every delivery
mode and the unknown one, shapes on both sides of every kernel threshold, the
fault counts at and past F, the Byzantine words, crash schedules and cuts.
tests/golden/plan_matrix.json records, per configuration, what bo_kernel_for
answered when the fixture was made -- the kernel family, or the error code and
the full bo_last_error text; the library under test must answer the same, byte
for byte (tests/golden/make_plan_matrix.py makes the fixture and expands a row).
"""
import json
import os

import benor
import make_plan_matrix as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_matrix(monkeypatch):
    for knob in benor.KNOBS:                      # every knob forces a planner choice
        monkeypatch.delenv(knob, raising=False)
    with open(os.path.join(ROOT, "tests", "golden", "plan_matrix.json")) as f:
        fx = json.load(f)
    rows = pm.grid()
    assert fx["k_max"] == pm.K_MAX and fx["rows"] == len(rows) == len(fx["outcomes"]) >= 3000
    assert fx["grid_sha256"] == pm.grid_digest(rows), "the fixture is not the generator's grid: run make_plan_matrix.py"
    want = [(benor.BO_OK, c) if c < pm.ERROR_BASE else tuple(fx["errors"][c - pm.ERROR_BASE]) for c in fx["outcomes"]]
    assert {r[0] for r in rows} == set(range(15)) and {(r[1], r[2]) for r in rows} >= set(pm.SHAPES)
    # the kernel families the grid reaches, and the table limit on both sides
    assert {k for rc, k in want if rc == benor.BO_OK} >= {0, 1, 2, 4, 6, 7, 8} | set(range(9, 22))
    limit = sorted((r[9], w[0]) for r, w in zip(rows, want) if r[1:3] == [4096, 2048])
    assert limit == [(15, benor.BO_OK)] * 3 + [(16, benor.BO_ERR_UNSUPPORTED)] * 3
    bad = [(r, w, got) for r, w in zip(rows, want) for got in [pm.outcome(r)] if got != w]
    assert not bad, f"{len(bad)} of {len(rows)} configurations differ, the first: {bad[:5]}"
