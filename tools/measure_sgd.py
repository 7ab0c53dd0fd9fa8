"""The fused gradient descent (SGDSolver on a fused objective) against the same work composed from the operators
the package had before it, one JSON line per configuration (default: profiles/sgd_solve.jsonl).

  fused_forward      dava_ba_sgd_solve: K steps in one launch
  composed_forward   K x dava_ba_evaluate (value + gradient) with the torch update x <- x - lr g between them
  fused_gradient     the recording launch + the adjoint kernel: x_K, then d (w . x_K) / d x0 and / d obs
  composed_gradient  the torch loop over ReprojectionError with create_graph (the objective's double backward is
                     dava_ba_second_order), then the same backward

Configurations: C2 (2 x 128, B = 1024) and C3 (4 x 256 + Brown-Conrady, B = 8192), K = 100, lr = 1e-4.  The two
paths of a pair run interleaved in one process, in both orders, best of `--repeats` (>= 5) rounds after a warm-up;
times are HIP events around the calls, ended by a device synchronise.  For C3 the line also gives the ratio of
the fused forward to K x 108.04 us, the time of one C3 evaluation sweep alone at B = 8192
(profiles/r05_eval_summary.json).  Needs a ROCm device: there is no fallback.

--mode large: descent + gradient (the recording launch, then the adjoint for d (w . x_K) / d x0 and / d obs) where
only forms 1 and 2 of the adjoint run -- C5 (16 x 4096, B = 256: form 2) and a two-view scene with 1,800 points
(B = 1024: form 1), K = 100, lr = 1e-5 -- next to the fused forward alone (nothing else on the GPU computes these
gradients); and at C3 (B = 8192) the adjoint in form 0 and raised to forms 1 and 2 through the F32_DUAL_FORM
override, alternated run by run.  Lines are appended to profiles/sgd_large.jsonl.

--mode f64: the float64 fused descent (dava_ba_sgd_solve_f64) against K x dava_ba_evaluate_f64 with torch updates,
and the float64 descent + gradient (the recording launch and the adjoint kernel, SGDSolver on a float64_descent=True
objective) against the torch loop with create_graph on a float64_derivatives=True objective (its double backward is
one dava_ba_second_order_f64 launch per step) -- the paths a float64 SGDSolver call took before the fused ones.
C2 (B = 1024) and C3 (B = 8192) at lr = 1e-4, C5 (B = 256) at lr = 1e-5, K = 100; the method of the default mode
(interleaved in one process, both orders, best of >= 5 rounds after a warm-up, HIP events), every round's times
kept.  Lines are written to profiles/sgd_f64.jsonl.

usage: python tools/measure_sgd.py [--out FILE] [--repeats 5] [--configs c2:1024,c3:8192] [--iterations 100]
       python tools/measure_sgd.py --mode large [--out FILE] [--repeats 5] [--iterations 100]
       python tools/measure_sgd.py --mode f64 [--out FILE] [--repeats 5] [--configs c2:1024,c3:8192,c5:256]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "deep-attention-visual-odometry_amd")]

import torch  # noqa: E402

SHAPES = {"c1": (2, 64, False), "c2": (2, 128, False), "c3": (4, 256, True), "c5": (16, 4096, False),
          "2x1800": (2, 1800, False)}
C3_SWEEP_US = 108.04  # profiles/r05_eval_summary.json, B = 8192


def timed(fn, dev):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize(dev)
    return start.elapsed_time(end), out


def measure(shape, b, k, lr, repeats, dev):
    from deep_attention_visual_odometry_amd import ReprojectionError, SGDSolver, make_scenes, native_ops

    m, n, dist = SHAPES[shape]
    s = make_scenes(b, m, n, distortion=dist, seed=7, drop=0.0 if dist else 0.1)
    x0 = torch.tensor(s.initial, device=dev)
    obs = torch.tensor(s.observations, device=dev)
    vis = torch.tensor(s.visibility, device=dev).to(torch.uint8)
    w = torch.randn(x0.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    solver = SGDSolver(lr, k)

    def fused_forward():
        return native_ops.ba_sgd_solve(x0, obs, vis, m, n, dist, learning_rate=lr, iterations=k)[0]

    def composed_forward():
        x = x0
        for _ in range(k):
            _, g, _ = torch.ops.dava.ba_evaluate(x, obs, vis, m, n, dist, None, None, True, False, 0)
            x = x - lr * g
        return x

    def gradient(loop):
        xg, og = x0.clone().requires_grad_(True), obs.clone().requires_grad_(True)
        fn = ReprojectionError(og, vis, m, n, dist)
        out = solver._loop(xg, fn) if loop else solver(xg, fn)
        gx, go = torch.autograd.grad((out * w).sum(), [xg, og])
        return out.detach(), gx, go

    paths = {"fused_forward": fused_forward, "composed_forward": composed_forward,
             "fused_gradient": lambda: gradient(False), "composed_gradient": lambda: gradient(True)}
    best = {name: float("inf") for name in paths}
    outs = {}
    for pair in (("fused_forward", "composed_forward"), ("fused_gradient", "composed_gradient")):
        for name in pair:  # warm-up: code objects, allocator
            outs[name] = timed(paths[name], dev)[1]
        for rep in range(repeats):
            for name in (pair if rep % 2 == 0 else pair[::-1]):  # both orders
                ms, _ = timed(paths[name], dev)
                best[name] = min(best[name], ms)

    # rows the descent keeps finite in both paths (at lr = 1e-4 a few of thousands of scenes diverge within K = 100,
    # in the oracle too: no stopping rule, no line search)
    finite = torch.isfinite(outs["fused_forward"]).all(dim=-1) & torch.isfinite(outs["composed_forward"]).all(dim=-1)

    def rel(a, c):  # (a row that is about to diverge is ill-conditioned: the median says what a typical row does)
        r = ((a - c).norm(dim=-1) / c.norm(dim=-1))[finite]
        r = r[torch.isfinite(r)]
        return {"max": float(r.max()), "median": float(r.median())}

    rec = {"shape": shape, "B": b, "K": k, "learning_rate": lr, "P": x0.shape[1], "repeats": repeats,
           "nonfinite_rows_fused": int((~torch.isfinite(outs["fused_forward"]).all(dim=-1)).sum()),
           "nonfinite_rows_composed": int((~torch.isfinite(outs["composed_forward"]).all(dim=-1)).sum()),
           "rows_compared": int(finite.sum())}
    for name, ms in best.items():
        rec[name + "_ms"] = round(ms, 3)
        rec[name + "_problems_per_s"] = round(b / (ms * 1e-3), 1)
    rec["forward_speedup"] = round(best["composed_forward"] / best["fused_forward"], 2)
    rec["gradient_speedup"] = round(best["composed_gradient"] / best["fused_gradient"], 2)
    # the two paths compute the same thing (reordered float32 sums apart)
    rec["forward_max_rel_diff"] = rel(outs["fused_forward"], outs["composed_forward"])
    rec["gradient_x0_max_rel_diff"] = rel(outs["fused_gradient"][1] - w, outs["composed_gradient"][1] - w)
    rec["gradient_obs_max_rel_diff"] = rel(outs["fused_gradient"][2].flatten(1), outs["composed_gradient"][2].flatten(1))
    if shape == "c3" and b == 8192:
        rec["fused_forward_over_K_sweeps"] = round(best["fused_forward"] * 1e3 / (k * C3_SWEEP_US), 3)
    return rec


def measure_large(shape, b, k, lr, repeats, forms, dev):
    """Descent + gradient with the adjoint in each of `forms` (None: the form the fit chooses; 1 | 2: raised through
    F32_DUAL_FORM), alternated run by run, and the fused forward alone."""
    from deep_attention_visual_odometry_amd import _native as N
    from deep_attention_visual_odometry_amd import make_scenes, native_ops

    m, n, dist = SHAPES[shape]
    s = make_scenes(b, m, n, distortion=dist, seed=7, drop=0.0 if dist else 0.1)
    x0 = torch.tensor(s.initial, device=dev)
    obs = torch.tensor(s.observations, device=dev)
    vis = torch.tensor(s.visibility, device=dev).to(torch.uint8)
    w = torch.randn(x0.shape, generator=torch.Generator().manual_seed(3)).to(dev)

    def forward():
        return native_ops.ba_sgd_solve(x0, obs, vis, m, n, dist, learning_rate=lr, iterations=k)[0]

    def gradient(forced):
        with N.debug_overrides(**({} if forced is None else {"F32_DUAL_FORM": forced})):
            xg, og = x0.clone().requires_grad_(True), obs.clone().requires_grad_(True)
            out, _ = native_ops.ba_sgd_solve_differentiable_large(xg, og, vis, m, n, dist, learning_rate=lr,
                                                                  iterations=k)
            gx, go = torch.autograd.grad((out * w).sum(), [xg, og])
        return gx, go

    paths = {"forward": forward}
    paths.update({f"gradient_form_{'fit' if f is None else f}": (lambda f=f: gradient(f)) for f in forms})
    best = {name: float("inf") for name in paths}
    outs = {name: timed(fn, dev)[1] for name, fn in paths.items()}  # warm-up: code objects, allocator
    for rep in range(repeats):
        for name in (list(paths) if rep % 2 == 0 else list(paths)[::-1]):  # both orders
            best[name] = min(best[name], timed(paths[name], dev)[0])
    rec = {"mode": "large", "shape": shape, "B": b, "K": k, "learning_rate": lr, "P": x0.shape[1], "repeats": repeats,
           "adjoint_form_by_fit": native_ops.sgd_backward_form(b, m, n, dist, k)}
    for name, ms in best.items():
        rec[name + "_ms"] = round(ms, 3)
        rec[name + "_problems_per_s"] = round(b / (ms * 1e-3), 1)
        if name != "forward":
            rec[name + "_over_forward"] = round(ms / best["forward"], 2)
            gx, go = outs[name]
            rec[name + "_finite_rows"] = int((torch.isfinite(gx).all(dim=-1) & torch.isfinite(go.flatten(1)).all(dim=-1)).sum())
    first = next(name for name in paths if name != "forward")
    for name in paths:  # the forms compute the same bits
        if name not in ("forward", first):
            rec[name + "_bitwise_" + first] = bool(
                torch.equal(outs[name][0].nan_to_num(), outs[first][0].nan_to_num())
                and torch.equal(outs[name][1].nan_to_num(), outs[first][1].nan_to_num()))
    return rec


def measure_f64(shape, b, k, lr, repeats, dev):
    from deep_attention_visual_odometry_amd import ReprojectionError, SGDSolver, make_scenes, native_ops

    m, n, dist = SHAPES[shape]
    s = make_scenes(b, m, n, distortion=dist, seed=7, drop=0.0 if dist else 0.1)
    x0 = torch.tensor(s.initial, device=dev).double()
    obs = torch.tensor(s.observations, device=dev).double()
    vis = torch.tensor(s.visibility, device=dev).to(torch.uint8)
    w = torch.randn(x0.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dev)
    solver = SGDSolver(lr, k)
    forms = (native_ops.sgd_solve_form_f64(b, m, n, dist, k), native_ops.sgd_backward_form_f64(b, m, n, dist, k))
    large = native_ops.second_order_form_f64(b, m, n, dist) != 0  # the loop's double backward beyond the LDS image

    def fused_forward():
        return native_ops.ba_sgd_solve_f64(x0, obs, vis, m, n, dist, learning_rate=lr, iterations=k)[0]

    def composed_forward():
        x = x0
        for _ in range(k):
            _, g, _ = native_ops.ba_evaluate(x, obs, vis, m, n, dist, want_grad=True)
            x = x - lr * g
        return x

    def gradient(loop):
        xg, og = x0.clone().requires_grad_(True), obs.clone().requires_grad_(True)
        if loop:
            fn = ReprojectionError(og, vis, m, n, dist, float64_derivatives=True, float64_large_gradients=large)
            out = solver._loop(xg, fn)
        else:
            out = solver(xg, ReprojectionError(og, vis, m, n, dist, float64_descent=True))
        gx, go = torch.autograd.grad((out * w).sum(), [xg, og])
        return out.detach(), gx, go

    paths = {"fused_forward": fused_forward, "composed_forward": composed_forward,
             "fused_gradient": lambda: gradient(False), "composed_gradient": lambda: gradient(True)}
    rounds = {name: [] for name in paths}
    outs = {}
    for pair in (("fused_forward", "composed_forward"), ("fused_gradient", "composed_gradient")):
        for name in pair:  # warm-up: code objects, allocator
            outs[name] = timed(paths[name], dev)[1]
        for rep in range(repeats):
            for name in (pair if rep % 2 == 0 else pair[::-1]):  # both orders
                rounds[name].append(timed(paths[name], dev)[0])
    finite = torch.isfinite(outs["fused_forward"]).all(dim=-1) & torch.isfinite(outs["composed_forward"]).all(dim=-1)

    def rel(a, c):
        r = ((a - c).norm(dim=-1) / c.norm(dim=-1))[finite]
        r = r[torch.isfinite(r)]
        return {"max": float(r.max()), "median": float(r.median())}

    rec = {"mode": "f64", "shape": shape, "B": b, "K": k, "learning_rate": lr, "P": x0.shape[1], "repeats": repeats,
           "descent_form": forms[0], "adjoint_form": forms[1], "rows_compared": int(finite.sum())}
    for name, ms in rounds.items():
        rec[name + "_ms"] = round(min(ms), 3)
        rec[name + "_rounds_ms"] = [round(t, 3) for t in ms]
        rec[name + "_problems_per_s"] = round(b / (min(ms) * 1e-3), 1)
    for what in ("forward", "gradient"):
        fused, composed = rounds["fused_" + what], rounds["composed_" + what]
        rec[what + "_speedup"] = round(min(composed) / min(fused), 2)
        rec[what + "_fused_faster_every_round"] = all(f < c for f, c in zip(fused, composed))
    rec["forward_max_rel_diff"] = rel(outs["fused_forward"], outs["composed_forward"])
    rec["gradient_x0_max_rel_diff"] = rel(outs["fused_gradient"][1] - w, outs["composed_gradient"][1] - w)
    rec["gradient_obs_max_rel_diff"] = rel(outs["fused_gradient"][2].flatten(1),
                                           outs["composed_gradient"][2].flatten(1))
    return rec


def main_f64(args, dev):
    out = args.out or os.path.join(REPO, "profiles", "sgd_f64.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    configs = "c2:1024,c3:8192,c5:256" if args.configs == "c2:1024,c3:8192" else args.configs
    lines = []
    for config in configs.split(","):
        shape, b = config.split(":")
        lr = args.learning_rate if args.learning_rate is not None else (1e-5 if shape == "c5" else 1e-4)
        rec = measure_f64(shape, int(b), args.iterations, lr, max(args.repeats, 5), dev)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def main_large(args, dev):
    out = args.out or os.path.join(REPO, "profiles", "sgd_large.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lr = 1e-5 if args.learning_rate is None else args.learning_rate
    for shape, b, forms in (("c3", 8192, (None, 1, 2)), ("2x1800", 1024, (None, 2)), ("c5", 256, (None,))):
        rec = measure_large(shape, b, args.iterations, lr, max(args.repeats, 5), forms, dev)
        print(json.dumps(rec), flush=True)
        with open(out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("solve", "large", "f64"), default="solve")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="c2:1024,c3:8192")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--learning-rate", type=float, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_sgd.py needs a ROCm device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    if args.mode == "large":
        return main_large(args, dev)
    if args.mode == "f64":
        return main_f64(args, dev)
    args.out = args.out or os.path.join(REPO, "profiles", "sgd_solve.jsonl")
    args.learning_rate = 1e-4 if args.learning_rate is None else args.learning_rate
    lines = []
    for config in args.configs.split(","):
        shape, b = config.split(":")
        rec = measure(shape, int(b), args.iterations, args.learning_rate, max(args.repeats, 5), dev)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
