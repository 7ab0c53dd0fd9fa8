"""Generates tests/golden/l1_solve.npz: the REAL reference's legacy solver (BFGSCameraSolver +
LineSearchStrongWolfeConditions over PinholeCameraModelL1, imported from /root/reference as make_golden.py
does) after k = 1 .. K iterations, for the fused legacy solve's tests.  Only the reference's inputs and outputs are
committed; float64, one estimate per batch item (the reference's fallback step only broadcasts for E = 1).

Scenes: B = 6; a truth model drawn as make_golden._l1_model draws it; targets projected from the truth; the start
point is truth.add(N(0, sigma^2)); max_gradient = 1e3, constrain = True.

Cases (SETTINGS below), each with K separate, deterministic reference solves (max_iterations = k):
  A  3 x 6, the configurations' settings                       accepted while widening, accepted in zoom
  B  1 x 4, the smallest shape add() allows                    minimum shape
  C  as A with zoom_iterations = 2                             unfinished from zoom
  D  as A with max_step_size = 2, step distances 1e-4 / 1e-6   one widening trial, unfinished from widening
  E  as A with epsilon = 0.03                                  estimates freeze at different iterations
  F  5 x 9, perturbation 0.05                                  more views than waves

Per case X: X_<parameter> (the start point), X_true, X_vis, X_settings (SETTING_FIELDS), X_out_<parameter> and
X_out_error (K, ...): the reference's result after k iterations, X_final_<parameter>: the result of the K-iteration
solve that also recorded, per iteration and problem, X_alpha (K, B): the returned step's alpha = step.d / d.d, and
X_wolfe (K, B): whether the returned point satisfies Armijo and the strong curvature condition.  The recording is a
thin module around the reference's line search that calls it unchanged.

Asserted here, at generation time: A shows accepted alphas that are powers of two and accepted alphas that are not;
C and D show unaccepted returns; E has estimates whose error is <= 0.03 before the last iteration; and no case is
ill-conditioned (a second solve from inputs moved by one ulp differs by < 1e-9).  If a seed misses an exit, change
the seed, not the assertion.

    python tests/golden/make_golden_l1_solve.py
"""
import os
import sys
import typing

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

import typing_extensions  # noqa: E402

if not hasattr(typing, "Self"):
    typing.Self = typing_extensions.Self

from deep_attention_visual_odometry.camera_model import PinholeCameraModelL1  # noqa: E402
from deep_attention_visual_odometry.geometry.lie_rotation import LieRotation  # noqa: E402
from deep_attention_visual_odometry.solvers import BFGSCameraSolver  # noqa: E402
from deep_attention_visual_odometry.solvers.line_search_strong_wolfe_conditions import (  # noqa: E402
    LineSearchStrongWolfeConditions,
)

PARAMS = ("focal_length", "cx", "cy", "translation", "lie", "world")
SETTING_FIELDS = ("views", "points", "iterations", "epsilon", "max_step_distance", "min_step_distance",
                  "max_step_size", "zoom_iterations", "sufficient_decrease", "curvature")
BASE = dict(views=3, points=6, epsilon=1e-6, max_step_distance=1e3, min_step_distance=1e-3, max_step_size=1e5,
            zoom_iterations=20, sufficient_decrease=1e-4, curvature=0.9)
SETTINGS = {
    "A": dict(BASE, iterations=6),
    "B": dict(BASE, views=1, points=4, iterations=4),
    "C": dict(BASE, zoom_iterations=2, iterations=3),
    "D": dict(BASE, max_step_size=2.0, max_step_distance=1e-4, min_step_distance=1e-6, iterations=4),
    "E": dict(BASE, epsilon=0.03, iterations=6),
    "F": dict(BASE, views=5, points=9, iterations=6),
}
SIGMA = {"F": 0.05}
SEEDS = {"A": 9501, "B": 9502, "C": 9503, "D": 9504, "E": 9505, "F": 9506}
BATCH = 6


class RecordingLineSearch(nn.Module):
    """Calls the reference's line search unchanged and records, per call and problem, the returned step's alpha and
    whether the returned point satisfies the strong Wolfe conditions."""

    def __init__(self, line_search):
        super().__init__()
        self.line_search = line_search
        self.alpha, self.wolfe = [], []

    def forward(self, function, search_direction):
        next_function, step = self.line_search(function, search_direction)
        d = search_direction
        ls = self.line_search
        scale = torch.tensor(1.0 / function.num_parameters, dtype=torch.float).sqrt()
        alpha = (step * d).sum(dim=-1) / (d * d).sum(dim=-1)
        f0 = scale * function.get_error()
        slope0 = (scale * function.get_gradient() * d).sum(dim=-1)
        f1 = scale * next_function.get_error()
        slope1 = (scale * next_function.get_gradient() * d).sum(dim=-1)
        armijo = f1 <= f0 + ls.sufficient_decrease * alpha * slope0
        curvature = slope1.abs() <= -ls.curvature * slope0
        self.alpha.append(alpha[:, 0].clone())
        self.wolfe.append((armijo & curvature)[:, 0].clone())
        return next_function, step


def draw_parts(rng, b, m, n):
    """make_golden._l1_model's draw (E = 1); its two special rotations where the views exist."""
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    parts = dict(
        focal_length=t(rng.uniform(0.6, 1.8, size=(b, 1))),
        cx=t(rng.normal(0.0, 0.1, size=(b, 1))),
        cy=t(rng.normal(0.0, 0.1, size=(b, 1))),
        translation=t(rng.normal(0.0, 0.5, size=(b, 1, m, 3)) + np.array([0.0, 0.0, 8.0])),
        lie=t(rng.normal(0.0, 0.2, size=(b, 1, m, 1, 3))),
        world=t(rng.normal(0.0, 1.0, size=(b, 1, n - 2, 3))),
    )
    parts["lie"][0, 0, 0] = 0.0          # identity rotation (Taylor branches)
    if m > 1:
        parts["lie"][0, 0, 1] = 1e-3     # tiny angle
    true = t(rng.normal(0.0, 0.3, size=(b, m, n, 2)))
    vis = torch.tensor(rng.random((b, m, n)) > 0.15)
    return parts, true, vis


def model_of(parts, true, vis):
    return PinholeCameraModelL1(
        focal_length=parts["focal_length"], cx=parts["cx"], cy=parts["cy"], translation=parts["translation"],
        orientation=LieRotation(parts["lie"]), world_points=parts["world"], true_projected_points=true,
        visibility_mask=vis, max_gradient=1e3, constrain=True)


def parts_of(model):
    return dict(focal_length=model.focal_length, cx=model.cx, cy=model.cy, translation=model._translation,
                lie=model._orientation._lie_vector, world=model._world_points)


def solve(parts, true, vis, s, iterations, record=False):
    line_search = LineSearchStrongWolfeConditions(
        max_step_size=s["max_step_size"], zoom_iterations=s["zoom_iterations"],
        sufficient_decrease=s["sufficient_decrease"], curvature=s["curvature"])
    if record:
        line_search = RecordingLineSearch(line_search)
    solver = BFGSCameraSolver(max_iterations=iterations, epsilon=s["epsilon"],
                              max_step_distance=s["max_step_distance"], min_step_distance=s["min_step_distance"],
                              line_search=line_search, search_direction_network=None)
    with torch.no_grad():
        res = solver(model_of({k: v.clone() for k, v in parts.items()}, true, vis))
        out = {k: v.clone() for k, v in parts_of(res).items()}
        out["error"] = res.get_error().clone()
    return out, line_search


def gen_case(name):
    s = SETTINGS[name]
    m, n, k_max = s["views"], s["points"], s["iterations"]
    rng = np.random.default_rng(SEEDS[name])
    truth_parts, _, vis = draw_parts(rng, BATCH, m, n)
    with torch.no_grad():
        truth = model_of(truth_parts, torch.zeros(BATCH, m, n, 2, dtype=torch.float64), vis)
        target = torch.stack([truth._get_u(), truth._get_v()], dim=-1)[:, 0]
        start = truth.add(torch.tensor(rng.normal(0.0, SIGMA.get(name, 0.02), size=(BATCH, 1, truth.num_parameters))))
    parts = {k: v.clone() for k, v in parts_of(start).items()}
    out = {f"{name}_{k}": v.numpy() for k, v in parts.items()}
    out[f"{name}_true"], out[f"{name}_vis"] = target.numpy(), vis.numpy()
    out[f"{name}_settings"] = np.array([float(s[f]) for f in SETTING_FIELDS])
    per_k = [solve(parts, target, vis, s, k)[0] for k in range(1, k_max + 1)]
    for key in PARAMS + ("error",):
        out[f"{name}_out_{key}"] = np.stack([r[key].numpy() for r in per_k])
    final, rec = solve(parts, target, vis, s, k_max, record=True)
    for key in PARAMS:
        out[f"{name}_final_{key}"] = final[key].numpy()
        assert np.array_equal(out[f"{name}_final_{key}"], out[f"{name}_out_{key}"][-1]), (name, key)
    alpha, wolfe = torch.stack(rec.alpha).numpy(), torch.stack(rec.wolfe).numpy()
    out[f"{name}_alpha"], out[f"{name}_wolfe"] = alpha, wolfe
    # conditioning: the same solve from a start point moved by one ulp
    moved = {k: torch.nextafter(v, torch.full_like(v, float("inf"))) for k, v in parts.items()}
    other, _ = solve(moved, target, vis, s, k_max)
    spread = max(((other[k] - final[k]).norm() / final[k].norm().clamp(min=1e-30)).item() for k in PARAMS)
    assert spread < 1e-9, (name, spread)
    errors = out[f"{name}_out_error"][:, :, 0]
    print(f"{name}: {m} x {n}, K = {k_max}, one-ulp spread {spread:.1e}, accepted {int(wolfe.sum())}/{wolfe.size}, "
          f"final error {errors[-1].min():.2e} .. {errors[-1].max():.2e}")
    return out, alpha, wolfe, errors


def main():
    out = {}
    shown = {}
    for name in SETTINGS:
        case, alpha, wolfe, errors = gen_case(name)
        out.update(case)
        shown[name] = (alpha, wolfe, errors)
    alpha, wolfe, _ = shown["A"]
    power_of_two = alpha == np.exp2(np.round(np.log2(np.where(alpha > 0, alpha, 1.0))))
    assert (wolfe & power_of_two).any(), "case A: no step accepted while widening"
    assert (wolfe & ~power_of_two).any(), "case A: no step accepted in zoom"
    assert (~shown["C"][1]).any(), "case C: every return was accepted"
    assert (~shown["D"][1]).any(), "case D: every return was accepted"
    e_errors = shown["E"][2]
    assert (e_errors[:-1] <= 0.03).any(), "case E: no estimate froze before the last iteration"
    assert (e_errors[-1] > 0.03).any() or (e_errors[0] > 0.03).any()
    path = os.path.join(HERE, "l1_solve.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
