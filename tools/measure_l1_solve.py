"""The fused legacy solve (BFGSCameraSolver(fused=True): dava_l1_camera_solve, one launch) against the loop it
restates (fused=False: BFGSCameraSolver + LineSearchStrongWolfeConditions driving PinholeCameraModelL1 from the host,
one evaluation launch per trial plus the torch bookkeeping between them), one JSON line per configuration
(default: profiles/l1_solve.jsonl).

Configurations (the reference's bfgs_solver_*_config.yaml settings: 10 iterations, epsilon 1e-6, steps in
[1e-3, 1e3], max_step_size 1e5 = 17 widening trials, 20 zoom trials, c1 1e-4, c2 0.9, constrain, max_gradient 1e3):
  4 x 8 float64 at B E = 64 (the configurations' batch), 4,096 and 65,536;
  6 x 70 at B E = 1,024 in float64 and float32 (form 1: the inverse Hessian in the workspace).
Scenes: a truth per batch item, targets projected from it, the start point the truth + N(0, 0.02^2).

Method (tools/measure_sgd.py's): the two paths interleaved in one process, in both orders, best of `--repeats`
(>= 5) rounds after a warm-up; times are HIP events around the calls, ended by a device synchronise; every
round's times are kept.  Needs a ROCm device: there is no fallback.

usage: python tools/measure_l1_solve.py [--out FILE] [--repeats 5] [--configs 4x8:64:f64,...]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "deep-attention-visual-odometry_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = "4x8:64:f64,4x8:4096:f64,4x8:65536:f64,6x70:1024:f64,6x70:1024:f32"
SETTINGS = dict(max_iterations=10, epsilon=1e-6, max_step_distance=1e3, min_step_distance=1e-3)
LINE_SEARCH = dict(max_step_size=1e5, zoom_iterations=20, sufficient_decrease=1e-4, curvature=0.9)
PARAMS = ("focal_length", "cx", "cy", "translation", "lie", "world")


def timed(fn, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end), out


def scene(m, n, b, dtype, seed=7):
    from deep_attention_visual_odometry_amd.geometry import LieRotation

    rng = np.random.default_rng(seed)
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    truth = dict(focal_length=t(rng.uniform(0.6, 1.8, size=(b, 1))), cx=t(rng.normal(0.0, 0.1, size=(b, 1))),
                 cy=t(rng.normal(0.0, 0.1, size=(b, 1))),
                 translation=t(rng.normal(0.0, 0.5, size=(b, 1, m, 3)) + np.array([0.0, 0.0, 8.0])),
                 lie=t(rng.normal(0.0, 0.2, size=(b, 1, m, 1, 3))), world=t(rng.normal(0.0, 1.0, size=(b, 1, n - 2, 3))))
    out = {k: (v + t(rng.normal(0.0, 0.02, size=tuple(v.shape)))).to(dtype) for k, v in truth.items()}
    pts = torch.cat([torch.zeros(b, 2, 3, dtype=torch.float64), truth["world"][:, 0]], dim=1)
    pts[:, 1, 0] = 1.0
    pts[:, 2, 2] = 0.0
    rel = LieRotation(truth["lie"][:, 0]).rotate_vector(pts[:, None]) + truth["translation"][:, 0, :, None, :]
    f, cx, cy = (truth[k][:, 0].reshape(b, 1, 1) for k in ("focal_length", "cx", "cy"))
    out["true"] = torch.stack([f * rel[..., 0] / rel[..., 2] + cx, f * rel[..., 1] / rel[..., 2] + cy],
                              dim=-1).to(dtype)
    out["vis"] = torch.tensor(rng.random((b, m, n)) > 0.15)
    return out


def measure(m, n, b, dtype, repeats, dev):
    from deep_attention_visual_odometry_amd import native_ops
    from deep_attention_visual_odometry_amd.camera_model import PinholeCameraModelL1
    from deep_attention_visual_odometry_amd.geometry import LieRotation
    from deep_attention_visual_odometry_amd.solvers import BFGSCameraSolver, LineSearchStrongWolfeConditions

    t = {k: v.to(dev) for k, v in scene(m, n, b, dtype).items()}
    solvers = {name: BFGSCameraSolver(line_search=LineSearchStrongWolfeConditions(**LINE_SEARCH), fused=fused,
                                      **SETTINGS) for name, fused in (("fused", True), ("loop", False))}

    def run(name):
        model = PinholeCameraModelL1(focal_length=t["focal_length"], cx=t["cx"], cy=t["cy"],
                                     translation=t["translation"], orientation=LieRotation(t["lie"]),
                                     world_points=t["world"], true_projected_points=t["true"],
                                     visibility_mask=t["vis"], max_gradient=1e3, constrain=True)
        with torch.no_grad():
            out = solvers[name](model)
            return out, out.get_error()

    rounds = {"fused": [], "loop": []}
    outs = {}
    for name in rounds:  # warm-up: code objects, allocator
        outs[name] = timed(lambda: run(name), dev)[1]
    assert solvers["fused"].last_trace_exit is not None and solvers["loop"].last_trace_exit is None
    exits = solvers["fused"].last_trace_exit
    for rep in range(repeats):
        for name in (("fused", "loop") if rep % 2 == 0 else ("loop", "fused")):  # both orders
            rounds[name].append(timed(lambda: run(name), dev)[0])

    def rows(model):
        parts = (model.focal_length, model.cx, model.cy, model._translation, model._orientation.lie_vector,
                 model._world_points)
        return torch.cat([p.double().reshape(b, -1) for p in parts], dim=-1)

    diff = (rows(outs["fused"][0]) - rows(outs["loop"][0])).norm(dim=-1) / rows(outs["loop"][0]).norm(dim=-1)
    diff = diff[torch.isfinite(diff)]
    widen = int(np.ceil(np.log2(LINE_SEARCH["max_step_size"])))
    rec = {"shape": f"{m}x{n}", "dtype": str(dtype).replace("torch.", ""), "B": b, "E": 1,
           "P": 3 + 6 * m + 3 * n - 7, "form": native_ops.l1_solve_form(m, n, dtype), "repeats": repeats,
           "iterations": SETTINGS["max_iterations"], "widen_trials": widen,
           "zoom_trials": LINE_SEARCH["zoom_iterations"]}
    for name, ms in rounds.items():
        rec[name + "_ms"] = round(min(ms), 3)
        rec[name + "_rounds_ms"] = [round(x, 3) for x in ms]
        rec[name + "_solves_per_s"] = round(b / (min(ms) * 1e-3), 1)
    rec["speedup"] = round(min(rounds["loop"]) / min(rounds["fused"]), 2)
    rec["fused_faster_every_round"] = all(f < c for f, c in zip(rounds["fused"], rounds["loop"]))
    rec["max_rel_diff"] = float(diff.max())
    rec["median_rel_diff"] = float(diff.median())
    rec["exit_counts"] = {str(code): int((exits == code).sum()) for code in range(5)}
    rec["mean_error_out"] = {name: float(outs[name][1].double().mean()) for name in outs}  # (the solved error)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "l1_solve.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default=CONFIGS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_l1_solve.py needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []
    for config in args.configs.split(","):
        shape, b, dt = config.split(":")
        m, n = (int(v) for v in shape.split("x"))
        rec = measure(m, n, int(b), torch.float32 if dt == "f32" else torch.float64, max(args.repeats, 5), dev)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
