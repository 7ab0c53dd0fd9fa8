"""Records what the float32 fused host entry points return, for tests/test_f32_host_codes.py.

Two tables go to f32_host_codes.json:
  queries   the four host-only queries of the adjoint and of the gradient descent (QUERIES) over make_plan_table.py's
            shapes, objectives and iteration counts, both Hessian modes, the shape's batch and batch 0, the view-count
            edges where an LDS image stops fitting, each under no override and under the overrides the solve's plan
            table does not cross (query_rows' order): the exact integers, each distinct row of them kept once;
  launches  the seven float32 fused launch entry points called with arguments the host refuses (fake pointers
            throughout; candidate_rows' order): the status each row returned, one digit per row, and a digest of
            the rows themselves -- scene, config, which pointers are null, the byte counts.  Rows with two defects
            pin the order of the checks.
A launch row is recorded only if it cannot reach a launch: a row that returns DAVA_OK at batch > 0, or
DAVA_ERR_LAUNCH, stops the generator.

The expectations are a record of one build, to hold later ones to it.  Run against the build to record:
    DAVA_DEBUG_OVERRIDES=1 DAVA_LIB=<that libdava_ba.so> python tests/golden/make_f32_host_codes.py
"""
import ctypes
import hashlib
import importlib.util
import json
import os
import sys
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "f32_host_codes.json")
FAKE = 0x1000  # never dereferenced: every recorded call returns on the host
PLENTY = 1 << 40
OK, LAUNCH = 0, 3


def _plan_table():
    spec = importlib.util.spec_from_file_location("make_plan_table", os.path.join(HERE, "make_plan_table.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


_grid = _plan_table()
# (batch, views, points): the view counts between which an image stops fitting 160 KiB, four points each, bisected
# on the recorded build's own answers.  The adjoint's LDS image 169 / 170 (158 / 159 at 1025 iterations: past it the
# workspace gains the vector slices), its last global-vector image 363 / 364 at 12 iterations, 361 / 362 at 100 and
# 336 / 337 at 1025; the gradient descent's adjoint 240 / 241, the second derivatives 252 / 253, the gradient
# descent 404 / 405, the evaluation 459 / 460
EDGES = [(4, m, 4) for m in (158, 159, 169, 170, 240, 241, 252, 253, 336, 337, 361, 362, 363, 364, 404, 405, 459,
                             460)]
SHAPES = list(_grid.SHAPES) + EDGES
OBJECTIVES = list(_grid.OBJECTIVES)
MODES = list(_grid.MODES)
ITERATIONS = list(_grid.ITERATIONS)
OVERRIDES = [None, ("ADJ_FORCE_GV", 1), ("ADJ_GV_WAVES", 4), ("ADJ_LDS_ENTRIES", 0), ("ADJ_LDS_ENTRIES", 3),
             ("ADJ_SC_GLOBAL", 0), ("ADJ_SC_GLOBAL", 1), ("ADJ_GD_HBM", 1), ("FORCE_GV", 1), ("NO_PPT", 1)]
QUERIES = ("dava_ba_solve_backward_workspace_bytes", "dava_ba_solve_backward_lds_entries", "dava_ba_sgd_tape_bytes",
           "dava_ba_sgd_backward_supported")


def num_parameters(m, n, distortion):
    return 3 + 3 * n + 6 * (m - 1) + (5 if distortion else 0)


def set_override(N, override):
    N.clear_debug_overrides()
    if override is not None:
        N.set_debug_override(override[0], override[1])


def scene_struct(N, s):
    if s is None:
        return None
    data = FAKE if s["data"] else None
    return ctypes.byref(N.DavaScene(s["b"], s["m"], s["n"], s["d"], s["p"], data, data, s["res"]))


def solver_config(N, c):
    if c is None:
        return None
    return ctypes.byref(N.DavaSolverConfig(1e-4, 0.9, 1e-4, 1e-8, c["k"], 1000, 1, c["mode"], 0.0, 0, 0, 0))


def sgd_config(N, c):
    if c is None:
        return None
    return ctypes.byref(N.DavaSgdConfig(1e-3, c["k"]))


def query_rows():
    """(key, spec), in a fixed order."""
    for override in OVERRIDES:
        for shape in SHAPES:
            for distortion, residual in OBJECTIVES:
                for mode in MODES:
                    for b in (shape[0], 0):
                        for k in ITERATIONS:
                            yield (f"{shape[1]}x{shape[2]}|d{distortion}|r{residual}|m{mode}|b{b}|k{k}|{override}",
                                   (override, shape[1], shape[2], distortion, residual, mode, b, k))


def run_query(lib, N, spec):
    override, m, n, distortion, residual, mode, b, k = spec
    set_override(N, override)
    sc = scene_struct(N, dict(b=b, m=m, n=n, d=distortion, p=num_parameters(m, n, distortion), data=False,
                              res=residual))
    cfg, sgd = solver_config(N, dict(k=k, mode=mode)), sgd_config(N, dict(k=k))
    return [int(lib.dava_ba_solve_backward_workspace_bytes(sc, cfg)),
            int(lib.dava_ba_solve_backward_lds_entries(sc, cfg)),
            int(lib.dava_ba_sgd_tape_bytes(sc, sgd)), int(lib.dava_ba_sgd_backward_supported(sc, sgd))]


# ------------------------------------------------------------------------------------------------ launch rows

EVAL = "dava_ba_evaluate"
SECONDS = ("dava_ba_second_order", "dava_ba_second_order_obs")
ADJOINT = "dava_ba_solve_backward"
SGD_SOLVES = ("dava_ba_sgd_solve", "dava_ba_sgd_solve_record")
SGD_ADJOINT = "dava_ba_sgd_backward"
LAUNCH_SYMBOLS = (EVAL,) + SECONDS + (ADJOINT,) + SGD_SOLVES + (SGD_ADJOINT,)


def run_launch(lib, N, r):
    """Call r["sym"] as the row says.  Pointers are FAKE unless named in r["null"]."""
    set_override(N, r["override"])
    p = lambda name: None if name in r["null"] else FAKE  # noqa: E731
    sym, f = r["sym"], getattr(lib, r["sym"])
    sc = scene_struct(N, r["scene"])
    if sym == EVAL:
        return f(sc, p("x"), p("direction"), p("alpha"), p("err"), p("grad"), p("slope"), None)
    if sym == "dava_ba_second_order":
        return f(sc, p("x"), p("direction"), None, None, None, p("obs_grad"), None, None)
    if sym == "dava_ba_second_order_obs":
        return f(sc, p("x"), p("direction"), p("obs_direction"), None, None, None, p("obs_grad"), None, None)
    if sym == ADJOINT:
        return f(sc, solver_config(N, r["cfg"]), p("tape"), r["tape_bytes"], p("status"), p("x_out_grad"), p("x0_grad"),
                 p("obs_grad"), p("ws"), r["ws_bytes"], None)
    if sym == "dava_ba_sgd_solve":
        return f(sc, sgd_config(N, r["cfg"]), p("x0"), p("x_out"), None, None)
    if sym == "dava_ba_sgd_solve_record":
        return f(sc, sgd_config(N, r["cfg"]), p("x0"), p("x_out"), None, p("tape"), r["tape_bytes"], None)
    return f(sc, sgd_config(N, r["cfg"]), p("tape"), r["tape_bytes"], p("x_out_grad"), p("x0_grad"), p("obs_grad"),
             None)


def rows_digest(rows):
    """What pins the launch rows: a build whose queries differ would write other rows, and is not run on them."""
    return hashlib.sha256(json.dumps(rows, sort_keys=True).encode()).hexdigest()


def may_return_ok(r):
    """An empty batch is DAVA_OK; every other row is a refusal."""
    return (r["scene"] or {}).get("b", 1) == 0


def adjoint_tape_blocks_bytes(b, p, k):
    """What dava_ba_solve_backward reads of a tape (dava_tape.hpp: the history, x, g and scalar blocks, no vectors)."""
    pv, kcap, t = (p + 3) // 4 * 4, max(k - 1, 1), (3 * k + 1 + 3) // 4 * 4
    return 4 * b * (2 * kcap * pv + 2 * k * pv + t)


LAUNCH_SCENES = {"2x64": (2, 64, 0), "C3": (4, 256, 1), "2x339": (2, 339, 0), "C5": (16, 4096, 0)}
LAUNCH_OVERRIDES = (None, ("ADJ_FORCE_GV", 1), ("FORCE_GV", 1))
# (views, points, the entry points whose images the scene is past at K = 12, under no override)
PAST = ((241, 4, (SGD_ADJOINT,)), (253, 4, SECONDS + (SGD_ADJOINT,)), (364, 4, SECONDS + (SGD_ADJOINT, ADJOINT)),
        (405, 4, SECONDS + (SGD_ADJOINT, ADJOINT) + SGD_SOLVES), (460, 4, LAUNCH_SYMBOLS), (600, 8, LAUNCH_SYMBOLS))
FIRST_POINTER = {EVAL: "x", SECONDS[0]: "x", SECONDS[1]: "x", ADJOINT: "tape", SGD_SOLVES[0]: "x0",
                 SGD_SOLVES[1]: "x0", SGD_ADJOINT: "x_out_grad"}


def candidate_rows(lib, N):
    """Every launch row, each with at least one defect.  The byte counts follow the queries of the build at hand:
    rows_digest tells whether they are the recorded build's."""
    rows = []
    B, K = 4, 12
    bad_scene = dict(b=B, m=2, n=16, d=1, p=num_parameters(2, 16, 1), data=True, res=1)  # ray angle + distortion

    def add(sym, label, override, scene, cfg=None, null=(), tape_bytes=PLENTY, ws_bytes=PLENTY):
        rows.append(dict(id=f"{sym}|{label}|{override}", sym=sym, override=list(override) if override else None,
                         scene=scene, cfg=cfg, null=sorted(null), tape_bytes=tape_bytes, ws_bytes=ws_bytes))

    for override in LAUNCH_OVERRIDES:
        set_override(N, override)
        for name, (m, n, d) in LAUNCH_SCENES.items():
            good = dict(b=B, m=m, n=n, d=d, p=num_parameters(m, n, d), data=True, res=0)
            empty = dict(good, b=0, data=False)
            scene_defects = (("null-scene", None), ("p-mismatch", dict(good, p=good["p"] + 1)),
                             ("bad-residual", dict(good, res=7)), ("one-view", dict(good, m=1)),
                             ("ray-distorted", bad_scene), ("no-data", dict(good, data=False)))
            # ---- the evaluation ----
            a = lambda label, **kw: add(EVAL, f"{name}|{label}", override, **dict(dict(scene=good), **kw))  # noqa: E731
            for label, s in scene_defects:
                a(label, scene=s)
            a("null-x", null=("x",))
            a("null-error", null=("err",))
            a("slope-without-direction", null=("direction", "alpha"))
            a("slope-without-direction+null-x", null=("direction", "alpha", "x"))
            a("batch-0+null-x", scene=empty, null=("x", "err"))
            a("batch-0+ray-distorted", scene=dict(bad_scene, b=0))
            a("no-data+null-x", scene=dict(good, data=False), null=("x",))
            # ---- the second derivatives ----
            for sym in SECONDS:
                base = dict(scene=good)
                a = lambda label, **kw: add(sym, f"{name}|{label}", override, **dict(base, **kw))  # noqa: E731
                for label, s in scene_defects:
                    a(label, scene=s)
                a("null-x", null=("x",))
                a("batch-0+null-x", scene=empty, null=("x", "obs_grad"))
                a("batch-0+ray-distorted", scene=dict(bad_scene, b=0))
                a("no-data+null-x", scene=dict(good, data=False), null=("x",))
            # ---- the adjoint of the solve ----
            cfg = dict(k=K, mode=1)
            sc, cf = scene_struct(N, good), solver_config(N, cfg)
            ws = int(lib.dava_ba_solve_backward_workspace_bytes(sc, cf))
            tape = adjoint_tape_blocks_bytes(B, good["p"], K)
            if ws > 0:  # (C5's rows are past 14 groups per thread under no override: the refusals only)
                base = dict(scene=good, cfg=cfg, tape_bytes=tape, ws_bytes=ws)
                a = lambda label, **kw: add(ADJOINT, f"{name}|{label}", override, **dict(base, **kw))  # noqa: E731
                for label, s in scene_defects[:5]:
                    a(label, scene=s)
                a("null-config", cfg=None)
                a("null-config+null-scene", cfg=None, scene=None)
                a("null-config+ray-distorted", cfg=None, scene=bad_scene)
                a("dense", cfg=dict(k=K, mode=0))
                a("dense+ray-distorted", cfg=dict(k=K, mode=0), scene=bad_scene)
                a("bad-mode", cfg=dict(k=K, mode=2))
                for k in (-1, 0, 1026):
                    a(f"iterations-{k}", cfg=dict(k=k, mode=1))
                    a(f"iterations-{k}+null-tape", cfg=dict(k=k, mode=1), null=("tape",))
                    a(f"iterations-{k}+batch-0", cfg=dict(k=k, mode=1), scene=empty)
                    a(f"iterations-{k}+p-mismatch", cfg=dict(k=k, mode=1), scene=dict(good, p=good["p"] + 1))
                a("no-data", scene=dict(good, data=False))
                for missing in ("tape", "status", "x_out_grad", "x0_grad"):
                    a(f"null-{missing}", null=(missing,))
                a("batch-0+null-tape", scene=empty, null=("tape", "status", "x_out_grad", "x0_grad", "ws"),
                  tape_bytes=0, ws_bytes=0)
                a("batch-0+ray-distorted", scene=dict(bad_scene, b=0))
                # (the launch reads neither tail: one byte short of the tape's blocks, of the rows and vectors)
                a("short-tape", tape_bytes=tape - 1)
                a("null-workspace", null=("ws",))
                a("short-workspace", ws_bytes=ws - 257)
                a("short-tape+short-workspace", tape_bytes=tape - 1, ws_bytes=ws - 257)
                a("null-status+short-tape", null=("status",), tape_bytes=tape - 1)
                a("no-data+short-tape", scene=dict(good, data=False), tape_bytes=tape - 1)
            else:
                add(ADJOINT, f"{name}|rows-too-long", override, good, cfg=cfg)
                add(ADJOINT, f"{name}|rows-too-long+null-tape", override, good, cfg=cfg, null=("tape",))
                add(ADJOINT, f"{name}|rows-too-long+batch-0", override, empty, cfg=cfg)
            # ---- the gradient descent and its adjoint ----
            cfg = dict(k=K)
            tape = int(lib.dava_ba_sgd_tape_bytes(sc, sgd_config(N, cfg)))
            assert tape > 0
            for sym in SGD_SOLVES + (SGD_ADJOINT,):
                first = FIRST_POINTER[sym]
                base = dict(scene=good, cfg=cfg, tape_bytes=tape)
                a = lambda label, **kw: add(sym, f"{name}|{label}", override, **dict(base, **kw))  # noqa: E731
                for label, s in scene_defects:
                    a(label, scene=s)
                a("null-config", cfg=None)
                a("null-config+null-scene", cfg=None, scene=None)
                a("null-config+ray-distorted", cfg=None, scene=bad_scene)
                a("negative-iterations", cfg=dict(k=-1))
                a(f"negative-iterations+null-{first}", cfg=dict(k=-1), null=(first,))
                a("negative-iterations+batch-0", cfg=dict(k=-1), scene=empty)
                a("negative-iterations+no-data", cfg=dict(k=-1), scene=dict(good, data=False))
                for missing in (("x0", "x_out") if sym in SGD_SOLVES else ("x_out_grad", "x0_grad")):
                    a(f"null-{missing}", null=(missing,))
                a(f"batch-0+null-{first}", scene=empty, null=(first, "tape"), tape_bytes=0)
                a("batch-0+ray-distorted", scene=dict(bad_scene, b=0))
                a("batch-0+iterations-0", scene=empty, cfg=dict(k=0))
                if sym != SGD_SOLVES[0]:
                    a("null-tape", null=("tape",))
                    a("short-tape", tape_bytes=tape - 1)
                    a(f"null-{first}+short-tape", null=(first,), tape_bytes=tape - 1)
        # ---- scenes past an image: refused on the host, before or after the argument checks ----
        for m, n, past in PAST if override is None else PAST[-1:]:
            good = dict(b=B, m=m, n=n, d=0, p=num_parameters(m, n, 0), data=True, res=0)
            for sym in LAUNCH_SYMBOLS:
                cfg = dict(k=K, mode=1) if sym == ADJOINT else None if sym == EVAL or sym in SECONDS else dict(k=K)
                first = FIRST_POINTER[sym]
                label = f"{m}x{n}|" + ("past-the-image" if sym in past else "within-the-image")
                add(sym, f"{label}+null-{first}", override, good, cfg=cfg, null=(first,))
                add(sym, f"{label}+batch-0", override, dict(good, b=0), cfg=cfg)
                if sym in past:
                    add(sym, label, override, good, cfg=cfg)
                    add(sym, f"{label}+ray", override, dict(good, res=1), cfg=cfg)
    return rows


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "deep-attention-visual-odometry_amd"))
    from deep_attention_visual_odometry_amd import _native as N

    lib = N.load_library()
    print("recording", N.LIB_PATH)
    try:
        queries = [run_query(lib, N, spec) for _, spec in query_rows()]
        launches = candidate_rows(lib, N)
        expect = []
        for r in launches:
            st = int(run_launch(lib, N, r))
            if st == LAUNCH or (st == OK and not may_return_ok(r)):
                raise SystemExit(f"{r['id']}: status {st} -- the host did not refuse this row; not recorded")
            expect.append(st)
    finally:
        N.clear_debug_overrides()
    ids = [r["id"] for r in launches]
    assert len(set(ids)) == len(ids), "duplicate row id"
    assert {r["sym"] for r in launches} == set(LAUNCH_SYMBOLS)
    values = sorted({tuple(q) for q in queries})  # (most rows of the grid repeat another: each distinct row once)
    index = {v: i for i, v in enumerate(values)}
    record = {"query_symbols": list(QUERIES), "query_values": values,
              "query_rows": [index[tuple(q)] for q in queries],
              "launch_rows_sha256": rows_digest(launches),
              "launch_expect": textwrap.wrap("".join(map(str, expect)), 100)}  # (100 rows a line)
    with open(OUT, "w") as f:
        f.write(textwrap.fill(json.dumps(record), 118, break_long_words=False, break_on_hyphens=False) + "\n")
    print(f"{len(queries)} query rows ({len(values)} distinct), {len(launches)} launch rows -> {OUT}")


if __name__ == "__main__":
    main()
