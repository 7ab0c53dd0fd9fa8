"""Per-call time of ``torch.ops.dava`` operators, this tree against another checkout of the package (the parent
commit, built), to see what a change of the operator layer in ``_ops.py`` -- or of a kernel whose code object did not
come out identical -- costs per call.

  ba_sgd_solve, ba_sgd_backward_f64, ba_second_order_large, ba_sgd_backward_large at B = 3, 2 views, 16 points, K = 1
  ba_second_order_large, ba_sgd_backward_large, ba_second_order_large_f64, ba_sgd_backward_f64 at B = 3, 2 views,
  3600 points, K = 1 (names ending in @2x3600): the dual-number kernels in form 2

At the small size a call is bound by the dispatch and the launch, not by the kernel.  Two checkouts register the same
operator names, so they cannot share a process: the trees alternate process by process, in both orders (other, this,
this, other, ...), `--rounds` processes each.  A process warms every operator up, then times `--batches` batches of `--calls`
calls each with a host clock around the batch, ended by a device synchronise, and reports the median batch as
microseconds per call.  The line gives both trees' per-round medians, the spread (min, max) of the other tree's
rounds and whether the median of this tree's rounds lies inside it.  Needs a ROCm device: there is no fallback.

The line is printed; with DAVA_WRITE_PROFILES=1 it is also appended to `--out` (default profiles/op_dispatch.jsonl).

usage: python tools/measure_op_dispatch.py --other PATH_TO_BUILT_CHECKOUT [--rounds 5] [--batches 20] [--calls 500]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("ba_sgd_solve", "ba_sgd_backward_f64", "ba_second_order_large", "ba_sgd_backward_large",
       "ba_second_order_large@2x3600", "ba_sgd_backward_large@2x3600", "ba_second_order_large_f64@2x3600",
       "ba_sgd_backward_f64@2x3600")


def child(tree: str, batches: int, calls: int) -> None:
    sys.path[:0] = [tree, os.path.join(tree, "deep-attention-visual-odometry_amd")]
    import torch

    from deep_attention_visual_odometry_amd import make_scenes, native_ops  # noqa: F401  (registers the operators)

    assert torch.cuda.is_available(), "needs a ROCm device"
    dev = torch.device("cuda", 0)
    k, lr = 1, 1e-4
    ops = torch.ops.dava
    def scene_fns(m, n):
        s = make_scenes(3, m, n, distortion=False, seed=7)
        x = torch.tensor(s.initial, dtype=torch.float32, device=dev)
        obs = torch.tensor(s.observations, dtype=torch.float32, device=dev)
        vis = torch.tensor(s.visibility, dtype=torch.uint8, device=dev)
        x64, obs64 = x.double(), obs.double()
        _, _, tape = ops.ba_sgd_solve_differentiable_large(x, obs, vis, m, n, False, lr, k, 0, False)
        _, _, tape64 = ops.ba_sgd_solve_differentiable_f64(x64, obs64, vis, m, n, False, lr, k, 0, False)
        cot, cot64 = torch.ones_like(x), torch.ones_like(x64)
        return {
            "ba_sgd_solve": lambda: ops.ba_sgd_solve(x, obs, vis, m, n, False, lr, k, 0, False),
            "ba_sgd_backward_f64": lambda: ops.ba_sgd_backward_f64(cot64, tape64, obs64, vis, m, n, False, lr, k, 0, True),
            "ba_second_order_large": lambda: ops.ba_second_order_large(x, obs, vis, m, n, False, None, 0, True, True, None),
            "ba_sgd_backward_large": lambda: ops.ba_sgd_backward_large(cot, tape, obs, vis, m, n, False, lr, k, 0, True),
            "ba_second_order_large_f64": lambda: ops.ba_second_order_large_f64(x64, obs64, vis, m, n, False, None, 0, True,
                                                                               True, None),
        }

    fns = scene_fns(2, 16)
    fns.update({name + "@2x3600": fn for name, fn in scene_fns(2, 3600).items()})
    out = {}
    for name in OPS:
        fn = fns[name]
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(dev)
        per_call = []
        for _ in range(batches):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize(dev)
            per_call.append((time.perf_counter() - t0) / calls * 1e6)
        out[name] = statistics.median(per_call)
    print("CHILD " + json.dumps(out), flush=True)


def run_child(tree: str, args) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "--batches", str(args.batches), "--calls",
           str(args.calls)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:  # (a fault ends the measurement: nothing more is started on the device)
        sys.exit(f"measurement process of {tree} ended with {res.returncode}:\n{res.stdout}\n{res.stderr}")
    return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("CHILD ")][-1][6:])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="a built checkout of the repository to compare with (the parent commit)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "op_dispatch.jsonl"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.batches, args.calls)
    if not args.other:
        ap.error("--other is required")
    other = os.path.abspath(args.other)
    rounds = {"other": [], "this": []}
    for i in range(args.rounds):
        for which in (("other", "this") if i % 2 == 0 else ("this", "other")):
            rounds[which].append(run_child(other if which == "other" else REPO, args))
            print(f"round {i + 1}/{args.rounds} {which}: done", file=sys.stderr, flush=True)
    line = {"tool": "measure_op_dispatch", "scene": "B=3, 2 views x 16 points (@2x3600: x 3600 points), K=1", "unit": "us per call",
            "rounds": args.rounds, "batches": args.batches, "calls": args.calls, "ops": {}}
    for name in OPS:
        o = [r[name] for r in rounds["other"]]
        t = [r[name] for r in rounds["this"]]
        med = statistics.median(t)
        line["ops"][name] = {"other_round_medians": [round(v, 3) for v in o],
                             "this_round_medians": [round(v, 3) for v in t],
                             "other_spread": [round(min(o), 3), round(max(o), 3)],
                             "other_median": round(statistics.median(o), 3), "this_median": round(med, 3),
                             "this_inside_other_spread": min(o) <= med <= max(o),
                             "this_at_most_other_max": med <= max(o)}
    text = json.dumps(line)
    print(text)
    if os.environ.get("DAVA_WRITE_PROFILES") == "1":
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
