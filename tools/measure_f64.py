#!/usr/bin/env python
"""GPU.  The float64 fused solve (dava_ba_solve_f64) measured against the fp32 fused solve and against the
generic float64 loop, one JSON line per configuration (default: profiles/f64_solve.jsonl).

  c2, c3         C2 (2 x 128, B = 1024) and C3 (4 x 256, Brown-Conrady, B = 8192) at K = 100 fixed
                 iterations: float64 fused and float32 fused alternated in one process.
  c3_b256_k20    C3 at B = 256, K = 20: float64 fused against the only float64 route there was before it, the
                 drop-in's generic loop around the torch closure (geometry.closure_ops) in float64.

--mode grad (default output profiles/f64_adjoint.jsonl): solve PLUS gradient, d (w . x_K) / d (x0, observations):
  c2, c3         the float64 recording solve + adjoint (dava_ba_solve_record_f64, dava_ba_solve_backward_f64)
                 and the float32 recording solve + adjoint at the same shapes, K = 100, alternated in one process.
  c3_b32_k20     C3 at B = 32, K = 20 (a batch whose dense graph, about 3 K P^2 8 bytes per problem, fits): the
                 float64 fused route against the generic float64 loop with torch's graph (GENERIC_BACKWARD).
  No rate is a requirement in this mode: the numbers are reported as measured.

--mode train (default output profiles/f64_training.jsonl): training mode as the reference trains (drop_path_p = 0.1),
solve PLUS gradient through the drop-in on an objective built with float64_derivatives=True:
  c3_b32_k20, c2_b1024_k100   the fused route (dava_ba_solve_record_train_f64 + the adjoint, counter-based drop
                 schedule) against the generic float64 loop with torch's graph and torch's random stream
                 (GENERIC_TRAINING), alternated run by run in one process.  The two draw different schedules from
                 the same distribution; the mean steps per problem of the fused runs is reported.
  No rate is a requirement in this mode either.

--large (default output profiles/f64_large.jsonl): the float64 solve beyond the LDS image (dava_ba_solve_large_f64),
float64 and float32 fused alternated solve by solve in one process, K = 100 fixed iterations:
  c5             C5 (16 x 4096, B = 256): float64 form 2 (scene in place, vectors in the workspace) against float32.
  c3_forms       C3 (B = 8192): float64 form 0, and forms 1 and 2 forced through the F64_FORM override, against
                 float32 -- what reading the scene in place, and the vectors from the workspace, cost where all run.
  m6_n700        (6 x 700, Brown-Conrady, B = 1024): float64 form 1, the form it takes, against float32.
  Every float64 run is checked: all problems finite, all took K steps.  No rate is a requirement.

--mode grad --large (default output profiles/f64_large_grad.jsonl): solve PLUS gradient beyond the LDS image, the
recording solve and the adjoint through the operators that take any scene size (dava_ba_solve_record_large_f64,
dava_ba_solve_backward_large_f64):
  c5             C5 (16 x 4096, B = 256, K = 20): recording and adjoint both form 2.
  m6_n700        (6 x 700, Brown-Conrady, B = 1024, K = 100): recording form 1, adjoint form 2.
  c3_forms       C3 (B = 8192, K = 100): the adjoint in form 0 and forced to forms 1 and 2 through F64_FORM (the
                 recording rises with it) -- what leaving LDS costs where all three run.
  m6_n700_b8_k20, m8_n600_b8_k20   (B = 8, K = 20) through the drop-in on an objective built with
                 float64_large_gradients=True: the fused route against the generic float64 loop with torch's graph
                 (GENERIC_BACKWARD).  At (6, 700) Brown-Conrady, P = 2138, the backward of the generic loop's dense
                 update keeps its nine vectors in a workspace (past P = 2133); at (8, 600), P = 1845, in LDS.
  The one requirement applies: the fused route beats the generic loop wherever both run.

Timing: device events around each solve, every shape warmed up first, median of --repeats (>= 5) solves.
Reported: problems/s, algorithmic HBM bytes (bench.py's compact model; 8-byte elements for float64, computed
here), the fraction of 8 TB/s they amount to, and the ratio to the fp32 fused rate.  The one requirement
(exit status 1 otherwise): the fused float64 solve is faster than the generic float64 loop at the same shape.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "deep-attention-visual-odometry_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PEAK_BYTES_PER_S = 8e12  # MI355X HBM3E


def compact_algorithmic_bytes(p, mn, iters, element, lds_entries=0):
    """bench.py's compact_algorithmic_bytes with `element`-byte values: iteration k >= 2 reads the k - 1 rows of
    S and W once, iterations 1 .. K-1 append one row of each; observations (2 values) and visibility (1 byte)
    per pair and x0 read once, x written once.  The oldest `lds_entries` entries never leave the CU."""
    pv = (p + 3) // 4 * 4
    reads = 2.0 * element * pv * sum(max(k - 1 - lds_entries, 0) for k in range(2, iters))
    writes = 2.0 * element * pv * max(iters - 1 - lds_entries, 0)
    return reads + writes + (2.0 * element + 1.0) * mn + 2.0 * element * p


def timed(fn, repeats):
    fn()  # warm-up of this shape (module load, allocator)
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end) * 1e-3)
    return times


def scene(b, m, n, distortion, dev):
    from deep_attention_visual_odometry_amd import make_scenes

    s = make_scenes(b, m, n, distortion=distortion, seed=7, drop=0.0 if distortion else 0.1)
    return (torch.tensor(s.initial, device=dev), torch.tensor(s.observations, device=dev),
            torch.tensor(s.visibility, device=dev).to(torch.uint8))


def fused_pair(tag, b, m, n, distortion, k, repeats, dev):
    """float64 fused and float32 fused, alternated solve by solve."""
    from deep_attention_visual_odometry_amd import _native as N
    from deep_attention_visual_odometry_amd import native_ops

    x32, obs32, vis = scene(b, m, n, distortion, dev)
    x64, obs64 = x32.double(), obs32.double()
    p, mn = x32.shape[1], m * n
    ws32 = torch.empty(native_ops.solve_workspace_bytes(b, m, n, distortion, N.DAVA_HESSIAN_COMPACT, k),
                       dtype=torch.uint8, device=dev)
    ws64 = torch.empty(native_ops.solve_workspace_bytes_f64(b, m, n, distortion, k), dtype=torch.uint8, device=dev)
    kw = dict(iterations=k, error_threshold=-1.0, minimum_step=-1.0, hessian_mode=N.DAVA_HESSIAN_COMPACT)
    runs = {"f64": lambda: native_ops.ba_solve(x64, obs64, vis, m, n, distortion, workspace=ws64, **kw),
            "f32": lambda: native_ops.ba_solve(x32, obs32, vis, m, n, distortion, workspace=ws32, **kw)}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    times = {"f64": [], "f32": []}
    for _ in range(repeats):
        for name, fn in runs.items():
            times[name] += timed(fn, 1)
    lds_entries = native_ops.solve_plan(b, m, n, distortion, N.DAVA_HESSIAN_COMPACT, k)["lds_history_entries"]
    out = {"config": tag, "batch": b, "views": m, "points": n, "distortion": distortion, "iterations": k,
           "repeats": repeats, "device": torch.cuda.get_device_name(dev)}
    for name, element, lds in (("f64", 8, 0), ("f32", 4, lds_entries)):
        med = statistics.median(times[name])
        algo = b * compact_algorithmic_bytes(p, mn, k, element, lds)
        out[name] = {"median_s": med, "min_s": min(times[name]), "problems_per_s": b / med,
                     "algorithmic_bytes": algo, "fraction_of_8TBps": algo / med / PEAK_BYTES_PER_S,
                     "lds_history_entries": lds}
    out["f64_over_f32_rate"] = out["f64"]["problems_per_s"] / out["f32"]["problems_per_s"]
    return out


def large_forms(tag, b, m, n, distortion, k, repeats, dev, forms):
    """float64 in each of `forms` (None: the form the fit chooses; 1 | 2: raised through F64_FORM) and float32 fused,
    alternated solve by solve."""
    from deep_attention_visual_odometry_amd import _native as N
    from deep_attention_visual_odometry_amd import native_ops

    x32, obs32, vis = scene(b, m, n, distortion, dev)
    x64, obs64 = x32.double(), obs32.double()
    p, mn = x32.shape[1], m * n
    kw = dict(iterations=k, error_threshold=-1.0, minimum_step=-1.0, hessian_mode=N.DAVA_HESSIAN_COMPACT)
    ws32 = torch.empty(native_ops.solve_workspace_bytes(b, m, n, distortion, N.DAVA_HESSIAN_COMPACT, k),
                       dtype=torch.uint8, device=dev)
    runs, taken, ws64 = {}, {}, {}

    def f64_run(name, forced):
        def run():
            with N.debug_overrides(**({} if forced is None else {"F64_FORM": forced})):
                return native_ops.ba_solve(x64, obs64, vis, m, n, distortion, workspace=ws64[name], want_status=True,
                                           **kw)
        return run

    for forced in forms:
        with N.debug_overrides(**({} if forced is None else {"F64_FORM": forced})):
            form = native_ops.solve_form_f64(b, m, n, distortion, iterations=k)
            need = native_ops.solve_large_workspace_bytes_f64(b, m, n, distortion, iterations=k)
        name = f"f64_form{form}"
        taken[name] = form
        ws64[name] = torch.empty(need, dtype=torch.uint8, device=dev)
        runs[name] = f64_run(name, forced)
    runs["f32"] = lambda: native_ops.ba_solve(x32, obs32, vis, m, n, distortion, workspace=ws32, want_status=True, **kw)
    checks = {}
    for name, fn in runs.items():  # warm-up of every variant, and the check of its result
        x, _, status = fn()
        checks[name] = {"all_finite": bool(torch.isfinite(x).all().item()),
                        "all_took_k_steps": bool((status[:, 0] == k).all().item())}
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(repeats):
        for name, fn in runs.items():
            times[name] += timed(fn, 1)
    lds_entries = native_ops.solve_plan(b, m, n, distortion, N.DAVA_HESSIAN_COMPACT, k)["lds_history_entries"]
    out = {"config": tag, "batch": b, "views": m, "points": n, "distortion": distortion, "iterations": k,
           "repeats": repeats, "device": torch.cuda.get_device_name(dev)}
    for name in runs:
        element, lds = (4, lds_entries) if name == "f32" else (8, 0)
        med = statistics.median(times[name])
        algo = b * compact_algorithmic_bytes(p, mn, k, element, lds)
        out[name] = {"median_s": med, "min_s": min(times[name]), "max_s": max(times[name]), "problems_per_s": b / med,
                     "algorithmic_bytes": algo, "fraction_of_8TBps": algo / med / PEAK_BYTES_PER_S, **checks[name]}
        if name != "f32":
            out[name]["form"] = taken[name]
    for name in taken:
        out[name]["over_f32_rate"] = out[name]["problems_per_s"] / out["f32"]["problems_per_s"]
    return out


def fused_vs_generic(tag, b, m, n, distortion, k, repeats, dev):
    """float64 fused against the generic float64 loop around the torch closure."""
    from deep_attention_visual_odometry_amd import BFGSSolver, ReprojectionError
    from deep_attention_visual_odometry_amd.geometry.closure_ops import reprojection_objective

    x32, obs32, vis = scene(b, m, n, distortion, dev)
    x64, obs64 = x32.double(), obs32.double()
    p, mn = x64.shape[1], m * n
    solver = BFGSSolver(iterations=k, error_threshold=-1.0, minimum_step=-1.0).eval()
    fn64 = ReprojectionError(obs64, vis, m, n, distortion)

    def closure(parameters, mask):
        return reprojection_objective(parameters, obs64[mask], vis[mask], m, n, distortion)

    t_fused = timed(lambda: solver(x64, fn64), repeats)
    assert solver.last_status is not None, "the float64 objective did not take the fused launch"
    x_fused = solver(x64, fn64)
    t_generic = timed(lambda: solver(x64, closure), repeats)
    x_generic = solver(x64, closure)
    rel = ((x_fused - x_generic).norm(dim=-1) / x_generic.norm(dim=-1)).max().item()
    fused, generic = statistics.median(t_fused), statistics.median(t_generic)
    algo = b * compact_algorithmic_bytes(p, mn, k, 8)
    return {"config": tag, "batch": b, "views": m, "points": n, "distortion": distortion, "iterations": k,
            "repeats": repeats, "device": torch.cuda.get_device_name(dev),
            "f64_fused": {"median_s": fused, "problems_per_s": b / fused, "algorithmic_bytes": algo,
                          "fraction_of_8TBps": algo / fused / PEAK_BYTES_PER_S},
            "f64_generic_closure": {"median_s": generic, "problems_per_s": b / generic},
            "fused_over_generic_rate": generic / fused, "max_rel_difference_fused_vs_generic": rel}


def grad_pair(tag, b, m, n, distortion, k, repeats, dev):
    """Solve + backward, float64 and float32 fused (recording solve + adjoint kernel), alternated run by run."""
    from deep_attention_visual_odometry_amd import native_ops

    x32, obs32, vis = scene(b, m, n, distortion, dev)
    w32 = torch.randn(x32.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    kw = dict(iterations=k, error_threshold=-1.0, minimum_step=-1.0)
    marks = {}

    def run(name, solve, x, obs, w):
        xg, og = x.clone().requires_grad_(True), obs.clone().requires_grad_(True)
        start, mid, end = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        start.record()
        out, status = solve(xg, og, vis, m, n, distortion, **kw)
        mid.record()
        gx, go = torch.autograd.grad((out * w).sum(), [xg, og])
        end.record()
        end.synchronize()
        finite = (torch.isfinite(gx).all(dim=-1) & (status[:, 0] == k)).float().mean().item()
        marks[name] = (start.elapsed_time(mid) * 1e-3, mid.elapsed_time(end) * 1e-3, finite)

    runs = {"f64": lambda: run("f64", native_ops.ba_solve_differentiable_f64, x32.double(), obs32.double(),
                               w32.double()),
            "f32": lambda: run("f32", native_ops.ba_solve_differentiable, x32, obs32, w32)}
    for fn in runs.values():  # warm-up of both (module load, allocator)
        fn()
    torch.cuda.synchronize()
    times = {"f64": [], "f32": []}
    for _ in range(repeats):
        for name, fn in runs.items():
            fn()
            times[name].append(marks[name])
    out = {"config": "grad_" + tag, "batch": b, "views": m, "points": n, "distortion": distortion, "iterations": k,
           "repeats": repeats, "device": torch.cuda.get_device_name(dev)}
    for name in ("f64", "f32"):
        fwd = statistics.median(t[0] for t in times[name])
        bwd = statistics.median(t[1] for t in times[name])
        total = statistics.median(t[0] + t[1] for t in times[name])
        out[name] = {"median_s": total, "recording_solve_median_s": fwd, "backward_median_s": bwd,
                     "problems_per_s": b / total,
                     "fraction_of_problems_with_k_steps_and_finite_gradients": times[name][-1][2]}
    out["f64_over_f32_rate"] = out["f64"]["problems_per_s"] / out["f32"]["problems_per_s"]
    return out


def grad_large_forms(tag, b, m, n, distortion, k, repeats, dev, forms):
    """Solve + backward in float64 through the operators that take any scene size, in each of `forms` (None: the forms
    the fit chooses; 1 | 2: raised through F64_FORM), alternated run by run."""
    from deep_attention_visual_odometry_amd import _native as N
    from deep_attention_visual_odometry_amd import native_ops

    x32, obs32, vis = scene(b, m, n, distortion, dev)
    x64, obs64 = x32.double(), obs32.double()
    w = torch.randn(x64.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
    kw = dict(iterations=k, error_threshold=-1.0, minimum_step=-1.0)
    marks, taken = {}, {}

    def run(name, forced):
        with N.debug_overrides(**({} if forced is None else {"F64_FORM": forced})):
            xg, og = x64.clone().requires_grad_(True), obs64.clone().requires_grad_(True)
            start, mid, end = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            start.record()
            out, status = native_ops.ba_solve_differentiable_f64(xg, og, vis, m, n, distortion, large=True, **kw)
            mid.record()
            gx, go = torch.autograd.grad((out * w).sum(), [xg, og])
            end.record()
            end.synchronize()
        finite = (torch.isfinite(gx).all(dim=-1) & (status[:, 0] == k)).float().mean().item()
        marks[name] = (start.elapsed_time(mid) * 1e-3, mid.elapsed_time(end) * 1e-3, finite)

    runs = {}
    for forced in forms:
        with N.debug_overrides(**({} if forced is None else {"F64_FORM": forced})):
            rec = native_ops.solve_form_f64(b, m, n, distortion, iterations=k)
            adj = native_ops.backward_form_f64(b, m, n, distortion, iterations=k)
        name = f"f64_rec{rec}_adj{adj}"
        taken[name] = (rec, adj)
        runs[name] = (lambda name=name, forced=forced: run(name, forced))
    for fn in runs.values():  # warm-up of every variant (module load, allocator)
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(repeats):
        for name, fn in runs.items():
            fn()
            times[name].append(marks[name])
    out = {"config": "large_grad_" + tag, "batch": b, "views": m, "points": n, "distortion": distortion,
           "iterations": k, "repeats": repeats, "device": torch.cuda.get_device_name(dev)}
    for name in runs:
        total = statistics.median(t[0] + t[1] for t in times[name])
        out[name] = {"recording_form": taken[name][0], "adjoint_form": taken[name][1], "median_s": total,
                     "recording_solve_median_s": statistics.median(t[0] for t in times[name]),
                     "backward_median_s": statistics.median(t[1] for t in times[name]),
                     "problems_per_s": b / total,
                     "fraction_of_problems_with_k_steps_and_finite_gradients": times[name][-1][2]}
    first = next(iter(runs))
    for name in runs:
        out[name]["rate_over_" + first] = out[name]["problems_per_s"] / out[first]["problems_per_s"]
    return out


def grad_vs_generic(tag, b, m, n, distortion, k, repeats, dev, large=False):
    """Solve + backward in float64 through the drop-in: the fused route against the generic loop with torch's graph.
    large: on an objective built with float64_large_gradients=True (a generic loop that refuses is recorded)."""
    from deep_attention_visual_odometry_amd import BFGSSolver, ReprojectionError, _native

    x32, obs32, vis = scene(b, m, n, distortion, dev)
    x64, obs64 = x32.double(), obs32.double()
    w = torch.randn(x64.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
    solver = BFGSSolver(iterations=k, error_threshold=-1.0, minimum_step=-1.0).eval()
    grads = {}

    def run(name):
        xg, og = x64.clone().requires_grad_(True), obs64.clone().requires_grad_(True)
        out = solver(xg, ReprojectionError(og, vis, m, n, distortion, float64_derivatives=True,
                                           float64_large_gradients=large))
        grads[name] = torch.autograd.grad((out * w).sum(), [xg, og])
        assert (solver.last_status is not None) == (name == "fused")

    t_fused = timed(lambda: run("fused"), repeats)
    try:
        with _native.debug_overrides(GENERIC_BACKWARD=1):
            t_generic = timed(lambda: run("generic"), repeats)
    except RuntimeError as e:
        if not large:
            raise
        fused = statistics.median(t_fused)
        return {"config": "large_grad_" + tag, "batch": b, "views": m, "points": n, "distortion": distortion,
                "iterations": k, "repeats": repeats, "device": torch.cuda.get_device_name(dev),
                "parameters": x64.shape[1], "f64_fused": {"median_s": fused, "problems_per_s": b / fused},
                "f64_generic_graph": {"error": str(e)}, "fused_over_generic_rate": None}
    rel = [((a - c).reshape(b, -1).norm(dim=-1) / c.reshape(b, -1).norm(dim=-1)).max().item()
           for a, c in zip(grads["fused"], grads["generic"])]
    fused, generic = statistics.median(t_fused), statistics.median(t_generic)
    return {"config": ("large_grad_" if large else "grad_") + tag, "batch": b, "views": m, "points": n,
            "distortion": distortion, "iterations": k,
            "repeats": repeats, "device": torch.cuda.get_device_name(dev),
            "f64_fused": {"median_s": fused, "problems_per_s": b / fused},
            "f64_generic_graph": {"median_s": generic, "problems_per_s": b / generic},
            "fused_over_generic_rate": generic / fused,
            "max_rel_difference_fused_vs_generic": {"x0_grad": rel[0], "observations_grad": rel[1]}}


def train_vs_generic(tag, b, m, n, distortion, k, repeats, dev, drop_p=0.1):
    """Training mode (drop path) solve + backward in float64 through the drop-in: the fused route against the generic
    loop with torch's graph, alternated run by run."""
    from deep_attention_visual_odometry_amd import BFGSSolver, ReprojectionError, _native

    x32, obs32, vis = scene(b, m, n, distortion, dev)
    x64, obs64 = x32.double(), obs32.double()
    w = torch.randn(x64.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
    solver = BFGSSolver(drop_path_p=drop_p, training_iterations=k, training_error_threshold=-1.0, minimum_step=-1.0)
    assert solver.training
    steps = []

    def run(name):
        xg, og = x64.clone().requires_grad_(True), obs64.clone().requires_grad_(True)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        with _native.debug_overrides(GENERIC_TRAINING=1 if name == "generic" else -1):
            out = solver(xg, ReprojectionError(og, vis, m, n, distortion, float64_derivatives=True))
        gx, go = torch.autograd.grad((out * w).sum(), [xg, og])
        end.record()
        end.synchronize()
        assert (solver.last_status is not None) == (name == "fused")
        assert torch.isfinite(gx).all() and torch.isfinite(go).all()
        if name == "fused":
            steps.append(solver.last_status[:, 0].float().mean().item())
        return start.elapsed_time(end) * 1e-3

    torch.manual_seed(0)
    for name in ("fused", "generic"):  # warm-up of both (module load, allocator)
        run(name)
    times = {"fused": [], "generic": []}
    for _ in range(repeats):
        for name in times:
            times[name].append(run(name))
    fused, generic = statistics.median(times["fused"]), statistics.median(times["generic"])
    return {"config": "train_" + tag, "batch": b, "views": m, "points": n, "distortion": distortion, "iterations": k,
            "drop_path_p": drop_p, "repeats": repeats, "device": torch.cuda.get_device_name(dev),
            "f64_fused": {"median_s": fused, "min_s": min(times["fused"]), "problems_per_s": b / fused,
                          "mean_steps_per_problem": statistics.mean(steps[1:])},
            "f64_generic_graph": {"median_s": generic, "min_s": min(times["generic"]), "problems_per_s": b / generic},
            "fused_over_generic_rate": generic / fused}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("solve", "grad", "train"), default="solve",
                    help="solve: the solve alone (the default); grad: solve plus gradient; train: training mode's "
                         "drop path, solve plus gradient")
    ap.add_argument("--large", action="store_true",
                    help="the float64 solve beyond the LDS image (forms 1 and 2) instead of --mode's runs; with "
                         "--mode grad: solve plus gradient beyond the LDS image")
    ap.add_argument("--out", default=None,
                    help="default: profiles/f64_solve.jsonl (solve), profiles/f64_adjoint.jsonl (grad), "
                         "profiles/f64_training.jsonl (train)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default=None, help="default: c2,c3,c3_b256_k20 (solve), c2,c3,c3_b32_k20 (grad), "
                                                     "c3_b32_k20,c2_b1024_k100 (train)")
    args = ap.parse_args(argv)
    grad, train = args.mode == "grad", args.mode == "train"
    large_grad = args.large and grad
    if large_grad:
        args.out = args.out or os.path.join(REPO, "profiles", "f64_large_grad.jsonl")
        args.configs = args.configs or "c5,m6_n700,c3_forms,m6_n700_b8_k20,m8_n600_b8_k20"
    elif args.large:
        grad = train = False
        args.out = args.out or os.path.join(REPO, "profiles", "f64_large.jsonl")
        args.configs = args.configs or "c5,c3_forms,m6_n700"
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", {"solve": "f64_solve.jsonl", "grad": "f64_adjoint.jsonl",
                                                   "train": "f64_training.jsonl"}[args.mode])
    if args.configs is None:
        args.configs = {"solve": "c2,c3,c3_b256_k20", "grad": "c2,c3,c3_b32_k20",
                        "train": "c3_b32_k20,c2_b1024_k100"}[args.mode]
    if args.repeats < 5:
        ap.error("--repeats must be at least 5 (the median of at least 5 timed solves)")
    assert torch.cuda.is_available(), "measure_f64.py needs a ROCm device"
    dev = torch.device("cuda", 0)
    lines, ok = [], True
    for name in args.configs.split(","):
        if large_grad and name == "c5":
            lines.append(grad_large_forms("c5", 256, 16, 4096, False, 20, args.repeats, dev, (None,)))
        elif large_grad and name == "m6_n700":
            lines.append(grad_large_forms("m6_n700", 1024, 6, 700, True, 100, args.repeats, dev, (None,)))
        elif large_grad and name == "c3_forms":
            lines.append(grad_large_forms("c3_forms", 8192, 4, 256, True, 100, args.repeats, dev, (None, 1, 2)))
        elif large_grad and name in ("m6_n700_b8_k20", "m8_n600_b8_k20"):
            m, n, distortion = (6, 700, True) if name.startswith("m6") else (8, 600, False)
            line = grad_vs_generic(name, 8, m, n, distortion, 20, args.repeats, dev, large=True)
            ok = ok and (line["fused_over_generic_rate"] is None or line["fused_over_generic_rate"] > 1.0)
            lines.append(line)
        elif large_grad:
            ap.error(f"unknown configuration {name!r} for --mode grad --large")
        elif args.large and name == "c5":
            lines.append(large_forms("large_c5", 256, 16, 4096, False, 100, args.repeats, dev, (None,)))
        elif args.large and name == "c3_forms":
            lines.append(large_forms("large_c3_forms", 8192, 4, 256, True, 100, args.repeats, dev, (None, 1, 2)))
        elif args.large and name == "m6_n700":
            lines.append(large_forms("large_m6_n700", 1024, 6, 700, True, 100, args.repeats, dev, (None,)))
        elif args.large:
            ap.error(f"unknown configuration {name!r} for --large")
        elif train and name == "c3_b32_k20":
            lines.append(train_vs_generic(name, 32, 4, 256, True, 20, args.repeats, dev))
        elif train and name == "c2_b1024_k100":
            lines.append(train_vs_generic(name, 1024, 2, 128, False, 100, args.repeats, dev))
        elif train:
            ap.error(f"unknown configuration {name!r} for --mode train")
        elif grad and name == "c2":
            lines.append(grad_pair("c2", 1024, 2, 128, False, 100, args.repeats, dev))
        elif grad and name == "c3":
            lines.append(grad_pair("c3", 8192, 4, 256, True, 100, args.repeats, dev))
        elif grad and name == "c3_b32_k20":
            lines.append(grad_vs_generic("c3_b32_k20", 32, 4, 256, True, 20, args.repeats, dev))
        elif grad:
            ap.error(f"unknown configuration {name!r} for --mode grad")
        elif name == "c2":
            lines.append(fused_pair("c2", 1024, 2, 128, False, 100, args.repeats, dev))
        elif name == "c3":
            lines.append(fused_pair("c3", 8192, 4, 256, True, 100, args.repeats, dev))
        elif name == "c3_b256_k20":
            line = fused_vs_generic("c3_b256_k20", 256, 4, 256, True, 20, args.repeats, dev)
            ok = ok and line["fused_over_generic_rate"] > 1.0
            lines.append(line)
        else:
            ap.error(f"unknown configuration {name!r}")
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    if not ok:
        print("FAIL: the fused float64 solve is not faster than the generic float64 loop", file=sys.stderr)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
