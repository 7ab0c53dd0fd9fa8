"""Records the fused solve's host-side launch plan over a grid that crosses every branch of its derivation.

    python tests/golden/make_plan_table.py [path/to/libdava_ba.so]

writes tests/golden/solve_plan_table.json from the given build of the library (default: the in-tree one).
The committed table was written by the library as it stood BEFORE the plan was gathered into one derivation
(csrc/solve_plan.hpp); tests/test_solve_plan_table.py asserts that the current library reproduces every row.
Host-only: no device is touched.

Per (shape, distortion, residual, Hessian mode, override) one group; per iteration count one row
  [iterations, plan status, global_vectors, workgroup_threads, lds_bytes, lds_history_entries,
   solve workspace bytes, tape bytes, backward workspace bytes, backward LDS entries]
(the four plan fields are -1 where dava_ba_solve_plan refuses the arguments and leaves them unwritten).
The file keeps the no-override groups whole and, for each override, only the values that differ from them
(pack / unpack below: lossless, every row of the grid is recorded).
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "solve_plan_table.json")

# (batch, views, points): C1, C2, C3 and C4-like shapes, C5, P = 1023 and 1026 (the single-pass limit of
# 4 float4 groups per lane, without distortion), many views (the per-view LDS rows dominate), and so many
# that no image fits (DAVA_ERR_UNSUPPORTED)
SHAPES = [(8192, 2, 64), (1024, 2, 128), (8192, 4, 256), (64, 8, 512), (256, 16, 4096), (512, 2, 338), (512, 2, 339),
          (64, 64, 64), (4, 600, 8)]
# (distortion, residual): the ray-angle residual has no distorted form
OBJECTIVES = [(0, 0), (1, 0), (0, 1)]
MODES = [0, 1]  # DAVA_HESSIAN_DENSE, DAVA_HESSIAN_COMPACT
ITERATIONS = [0, 1, 2, 3, 9, 30, 100, 400, 950, 1000, 1025, 1026, 5000]
OVERRIDES = [None, ("FORCE_GV", 1), ("GV_NO_XL", 1), ("SOLVE_WAVES", 1), ("SOLVE_WAVES", 2), ("SOLVE_WAVES", 4),
             ("LDS_HISTORY", 0), ("LDS_HISTORY", 3), ("WG_PER_CU", 1), ("COMPACT_SWITCH", 8), ("GV_SCALAR_SLICE", 0),
             ("GV_SCALAR_SLICE", 1)]
COLUMNS = ["iterations", "plan_status", "global_vectors", "workgroup_threads", "lds_bytes", "lds_history_entries",
           "workspace_bytes", "tape_bytes", "backward_workspace_bytes", "backward_lds_entries"]


def build_table(lib):
    """The whole grid from `lib` (a typed ctypes handle, _native.load_library)."""
    for p in (REPO, os.path.join(REPO, "deep-attention-visual-odometry_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from deep_attention_visual_odometry_amd import _native as N

    groups = []
    for override in OVERRIDES:
        lib.dava_debug_clear_overrides()
        if override is not None:
            assert lib.dava_debug_set_override(override[0].encode(), override[1]) == 0
        for b, m, n in SHAPES:
            for distortion, residual in OBJECTIVES:
                p = 3 + 3 * n + 6 * (m - 1) + (5 if distortion else 0)
                scene = N.DavaScene(b, m, n, distortion, p, None, None, residual)
                for mode in MODES:
                    rows = []
                    for k in ITERATIONS:
                        cfg = N.DavaSolverConfig(1e-4, 0.9, 1e-4, 1e-8, k, 1000, 1, mode, 0.0, 0, 0, 0)
                        plan = N.DavaSolvePlan(-1, -1, -1, -1)
                        sp, cp = ctypes.byref(scene), ctypes.byref(cfg)
                        status = lib.dava_ba_solve_plan(sp, cp, ctypes.byref(plan))
                        rows.append([k, status, plan.global_vectors, plan.workgroup_threads, plan.lds_bytes,
                                     plan.lds_history_entries, lib.dava_ba_solve_workspace_bytes(sp, cp),
                                     lib.dava_ba_solve_tape_bytes(sp, cp),
                                     lib.dava_ba_solve_backward_workspace_bytes(sp, cp),
                                     lib.dava_ba_solve_backward_lds_entries(sp, cp)])
                    groups.append({"shape": [b, m, n], "distortion": distortion, "residual": residual, "mode": mode,
                                   "override": list(override) if override else None, "rows": rows})
    lib.dava_debug_clear_overrides()
    return {"columns": COLUMNS, "groups": groups}


def pack(table):
    """The table as stored: the groups without override in full, then per override the differing values as
    [group, row, column, value, column, value, ...] (group: index among the no-override groups)."""
    n = len(table["groups"]) // len(OVERRIDES)
    base = table["groups"][:n]
    assert all(g["override"] is None for g in base)
    overrides = []
    for o, override in enumerate(OVERRIDES[1:], 1):
        changes = []
        for gi, (g, b) in enumerate(zip(table["groups"][o * n:(o + 1) * n], base)):
            assert g["override"] == list(override) and all(g[k] == b[k] for k in ("shape", "distortion", "residual", "mode"))
            for ri, (r, rb) in enumerate(zip(g["rows"], b["rows"])):
                d = [x for c, (v, vb) in enumerate(zip(r, rb)) if v != vb for x in (c, v)]
                if d:
                    changes.append([gi, ri] + d)
        overrides.append({"override": list(override), "changes": changes})
    return {"columns": table["columns"], "groups": base, "overrides": overrides}


def unpack(packed):
    """The whole grid, as build_table returns it, from the stored form."""
    groups = [dict(g) for g in packed["groups"]]
    for o in packed["overrides"]:
        new = [dict(g, override=o["override"], rows=[list(r) for r in g["rows"]]) for g in packed["groups"]]
        for gi, ri, *d in o["changes"]:
            for c, v in zip(d[::2], d[1::2]):
                new[gi]["rows"][ri][c] = v
        groups += new
    return {"columns": packed["columns"], "groups": groups}


def main():
    for p in (REPO, os.path.join(REPO, "deep-attention-visual-odometry_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from deep_attention_visual_odometry_amd import _native as N

    lib = N.load_library(sys.argv[1]) if len(sys.argv) > 1 else N.load_library()
    table = build_table(lib)
    packed = pack(table)
    assert unpack(packed) == table
    line = lambda v: "  " + json.dumps(v, separators=(",", ":"))  # noqa: E731
    with open(TABLE, "w") as f:
        f.write('{"columns": %s,\n "groups": [\n' % json.dumps(packed["columns"]))
        f.write(",\n".join(line(g) for g in packed["groups"]))
        f.write('\n ],\n "overrides": [\n')
        f.write(",\n".join(line(o) for o in packed["overrides"]))
        f.write("\n ]}\n")
    print(f"{TABLE}: {len(table['groups'])} groups x {len(ITERATIONS)} rows, {os.path.getsize(TABLE)} bytes")


if __name__ == "__main__":
    main()
