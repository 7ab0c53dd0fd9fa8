"""The fused solve's launch plan (csrc/solve_plan.hpp) is pinned, row by row, to the table recorded before
the plan was gathered into one derivation: every byte count, wave count, LDS size and status over a grid
that crosses each branch (LDS / global-vector mode, XL, the scalar slice, wave counts, on-chip history,
hybrid) and each debug override.  Host-only: no device is touched."""
import importlib.util
import json
import os

from conftest import GOLDEN


def _generator():
    spec = importlib.util.spec_from_file_location("make_plan_table", os.path.join(GOLDEN, "make_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_solve_plan_reproduces_the_recorded_table():
    from deep_attention_visual_odometry_amd import _native

    gen = _generator()
    with open(gen.TABLE) as f:
        want = gen.unpack(json.load(f))
    try:
        got = gen.build_table(_native.load_library())
    finally:
        _native.clear_debug_overrides()
    assert got["columns"] == want["columns"]
    n = len(gen.OVERRIDES) * len(gen.SHAPES) * len(gen.OBJECTIVES) * len(gen.MODES)
    assert len(want["groups"]) == n and len(got["groups"]) == n
    wrong = []
    for g, w in zip(got["groups"], want["groups"]):
        key = {k: w[k] for k in ("shape", "distortion", "residual", "mode", "override")}
        assert {k: g[k] for k in key} == key
        assert len(w["rows"]) == len(gen.ITERATIONS)
        wrong += [(key, rg, rw) for rg, rw in zip(g["rows"], w["rows"]) if rg != rw]
    assert not wrong, f"{len(wrong)} rows differ (case, got, recorded); the first: {wrong[:3]}"
