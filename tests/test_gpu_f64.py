"""The float64 fused path (dava_ba_evaluate_f64, dava_ba_solve_f64, the drop-in BFGSSolver on a float64
objective) against the CPU oracle run in float64.

Bars.  Evaluation: the project's own fp32 bars of test_gpu_objective.py (E rtol 2e-5, gradient normwise 1e-4,
slope rtol 1e-3) carried over in units of machine epsilon, i.e. times 2^-29: 3.7e-14, 1.9e-13, 1.9e-12.  The
float64 oracle against itself with the points permuted (another summation order) stays below 2.1e-16 /
2.4e-16 / 4.7e-15 on these shapes, so the bars leave about two orders of magnitude and would not hide a
float literal left in a series (1e-8).
Solves: per problem and per block (whole vector, intrinsics, distortion coefficients)
max(1e-5 * 2^-29, F x the oracle's own change under a 1-ulp nudge of x0, up and down), F from
tests/golden/parity_envelope.json -- the rule of test_gpu_solver._envelopes with the floor in float64 units.

Shapes (B = 3): (2, 5) fewer points than a wave, P = 24; (3, 70) Brown-Conrady crosses a wave, P = 230 is no
multiple of 4 (padded rows), two moving views; (2, 130) ray angle, P = 399; (2, 260) more points than
threads (the per-thread point loop runs twice).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import objective, solver

pytestmark = pytest.mark.gpu

EPS_RATIO = 2.0 ** -29  # float64 epsilon / float32 epsilon
E_RTOL, G_TOL, SLOPE_RTOL = 2e-5 * EPS_RATIO, 1e-4 * EPS_RATIO, 1e-3 * EPS_RATIO
TOL = 1e-5 * EPS_RATIO
B = 3
# name -> (M, N, distortion, ray angle, scene seed)
SHAPES = {
    "m2_n5": (2, 5, False, False, 31),
    "m3_n70_bc": (3, 70, True, False, 32),
    "m2_n130_ray": (2, 130, False, True, 33),
    "m2_n260": (2, 260, False, False, 34),
}
# test_reference_stopping_rules: (make_scenes seed, row) of problems whose last step crosses the threshold by 2x
FACTOR2_PROBLEMS = ((13, 2), (71, 1), (191, 1), (200, 1))


def _envelope_factor():
    with open(os.path.join(GOLDEN, "parity_envelope.json")) as fh:
        return float(json.load(fh)["envelope_factor"])


@functools.lru_cache(maxsize=None)
def _scene(b, m, n, distortion, seed):
    """make_scenes as test_gpu_solver._scene builds them, cast to double (shared, never modified)."""
    from deep_attention_visual_odometry_amd import make_scenes

    s = make_scenes(b, m, n, distortion=distortion, seed=seed, drop=0.0 if distortion else 0.1)
    return torch.tensor(s.initial).double(), torch.tensor(s.observations).double(), torch.tensor(s.visibility)


def _objective(x, obs, vis, m, n, distortion, ray):
    if ray:
        return objective.ray_angle_error(x, obs, vis, m, n)
    return objective.reprojection_error(x, obs, vis, m, n, distortion)


def _closure(obs, vis, m, n, distortion, ray):
    return objective.RayAngleClosure(obs, vis, m, n) if ray else objective.ReprojectionClosure(obs, vis, m, n, distortion)


def _fn(device, obs, vis, m, n, distortion, ray):
    from deep_attention_visual_odometry_amd import RayAngleError, ReprojectionError

    if ray:
        return RayAngleError(obs.to(device), vis.to(device), m, n)
    return ReprojectionError(obs.to(device), vis.to(device), m, n, distortion)


def _rel(a, b):
    rel = (a - b).norm(dim=-1) / b.norm(dim=-1)
    bad_a, bad_b = ~torch.isfinite(a).all(dim=-1), ~torch.isfinite(b).all(dim=-1)
    rel[bad_a & bad_b] = 0.0
    rel[bad_a != bad_b] = float("inf")
    return rel


def _check_evaluation(device, x, obs, vis, m, n, distortion, ray, tag, fixed=None):
    """E, dE/dx and the slope along a random direction at x + alpha d against the oracle's float64 autograd.
    `fixed` (a slice of parameter entries): the direction is zero there, so x + alpha d keeps x's values bit
    for bit on those entries; E, dE/dx and the slope are then also checked at x itself."""
    from deep_attention_visual_odometry_amd import native_ops

    rng = np.random.default_rng(5)
    d = torch.tensor(rng.normal(size=tuple(x.shape))) * 1e-3
    if fixed is not None:
        d[:, fixed] = 0.0
    alpha = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[: x.shape[0]]
    point = (x + alpha[:, None] * d).clone().requires_grad_(True)
    e_ref = _objective(point, obs, vis, m, n, distortion, ray)
    (g_ref,) = torch.autograd.grad(e_ref.sum(), point)
    e_ref = e_ref.detach()
    sl_ref = (g_ref * d).sum(-1)
    dv = lambda t: t.to(device)  # noqa: E731
    e, g, sl = native_ops.ba_evaluate(dv(x), dv(obs), dv(vis), m, n, distortion, direction=dv(d), alpha=dv(alpha),
                                      want_grad=True, want_slope=True,
                                      residual=1 if ray else 0)
    assert e.dtype == g.dtype == sl.dtype == torch.float64
    e, g, sl = e.cpu(), g.cpu(), sl.cpu()
    e_err = ((e - e_ref).abs() / e_ref.abs()).max().item()
    g_err = _rel(g, g_ref).max().item()
    sl_err = ((sl - sl_ref).abs() / sl_ref.abs()).max().item()
    print("EVAL64", json.dumps({"case": tag, "E_rel": e_err, "grad_rel": g_err, "slope_rel": sl_err,
                                "bars": [E_RTOL, G_TOL, SLOPE_RTOL]}))
    assert e_err <= E_RTOL and g_err <= G_TOL and sl_err <= SLOPE_RTOL, (e_err, g_err, sl_err)
    # the flavours without a gradient / a slope / a trial point give the same numbers (other instantiations)
    e2, g2, _ = native_ops.ba_evaluate(dv(point.detach()), dv(obs), dv(vis), m, n, distortion, want_grad=True,
                                       residual=1 if ray else 0)
    e3, _, sl3 = native_ops.ba_evaluate(dv(x), dv(obs), dv(vis), m, n, distortion, direction=dv(d), alpha=dv(alpha),
                                        want_grad=False, want_slope=True, residual=1 if ray else 0)
    assert ((e2.cpu() - e_ref).abs() / e_ref.abs()).max().item() <= E_RTOL
    assert _rel(g2.cpu(), g_ref).max().item() <= G_TOL
    assert ((e3.cpu() - e_ref).abs() / e_ref.abs()).max().item() <= E_RTOL
    assert ((sl3.cpu() - sl_ref).abs() / sl_ref.abs()).max().item() <= SLOPE_RTOL
    if fixed is not None:
        assert torch.equal(point.detach()[:, fixed], x[:, fixed])  # the trial point kept those entries exactly
        # ... and at x itself, without a trial point: GRAD + SLOPE, GRAD alone and SLOPE alone
        x_req = x.clone().requires_grad_(True)
        e0_ref = _objective(x_req, obs, vis, m, n, distortion, ray)
        (g0_ref,) = torch.autograd.grad(e0_ref.sum(), x_req)
        e0_ref, sl0_ref = e0_ref.detach(), (g0_ref * d).sum(-1)
        assert torch.isfinite(e0_ref).all() and torch.isfinite(g0_ref).all()
        res = 1 if ray else 0
        runs = [native_ops.ba_evaluate(dv(x), dv(obs), dv(vis), m, n, distortion, direction=dv(d), want_grad=True,
                                       want_slope=True, residual=res),
                native_ops.ba_evaluate(dv(x), dv(obs), dv(vis), m, n, distortion, want_grad=True, residual=res),
                native_ops.ba_evaluate(dv(x), dv(obs), dv(vis), m, n, distortion, direction=dv(d), want_grad=False,
                                       want_slope=True, residual=res)]
        worst = [0.0, 0.0, 0.0]
        for e0, g0, sl0 in runs:
            worst[0] = max(worst[0], ((e0.cpu() - e0_ref).abs() / e0_ref.abs()).max().item())
            if g0 is not None:
                worst[1] = max(worst[1], _rel(g0.cpu(), g0_ref).max().item())
            if sl0 is not None:
                worst[2] = max(worst[2], ((sl0.cpu() - sl0_ref).abs() / sl0_ref.abs()).max().item())
        print("EVAL64", json.dumps({"case": tag + "_at_x", "E_rel": worst[0], "grad_rel": worst[1],
                                    "slope_rel": worst[2], "bars": [E_RTOL, G_TOL, SLOPE_RTOL]}))
        assert worst[0] <= E_RTOL and worst[1] <= G_TOL and worst[2] <= SLOPE_RTOL, worst


# ---- 1. evaluation parity ----

@pytest.mark.parametrize("shape", list(SHAPES))
def test_evaluation_matches_the_float64_oracle(device, shape):
    m, n, distortion, ray, seed = SHAPES[shape]
    x, obs, vis = _scene(B, m, n, distortion, seed)
    _check_evaluation(device, x, obs, vis, m, n, distortion, ray, shape)


# ---- 2. Taylor branches ----

@pytest.mark.parametrize("norm2", [1e-3, 0.03])
def test_taylor_branches(device, norm2):
    """(3, 70) with view 1's rotation exactly zero and view 2's of norm 1e-3 (both series: below 0.01 and
    0.05) or 0.03 (between the thresholds: the closed form of sin x / x, the series of (1 - cos x) / x^2).
    The direction is zero on both views' rotation entries, so every launch -- at x + alpha d (GRAD + SLOPE +
    TRIAL, SLOPE + TRIAL), at the shifted point and at x itself (GRAD + SLOPE, GRAD, SLOPE) -- evaluates with
    view 1's theta == 0 exactly (1 / theta taken as 0, the series at 0) and view 2's norm exactly as set.
    A float literal left in a series or a threshold shows here at the 1e-8 level."""
    m, n, distortion, ray, seed = SHAPES["m3_n70_bc"]
    x, obs, vis = _scene(B, m, n, distortion, seed)
    x = x.clone()
    rot = 3 + 3 * n + 3 * (m - 1)
    x[:, rot:rot + 3] = 0.0
    w = torch.tensor([0.6, -0.48, 0.64], dtype=torch.float64)
    x[:, rot + 3:rot + 6] = w / w.norm() * norm2
    assert (x[:, rot:rot + 3] == 0.0).all()
    _check_evaluation(device, x, obs, vis, m, n, distortion, ray, f"taylor_{norm2}", fixed=slice(rot, rot + 6))


# ---- 3. fixed-K solve parity ----

def _oracle_with_envelopes(x0, obs, vis, m, n, distortion, ray, trajectory=None, **kw):
    """(reference, SolveRecord, per-block bounds) from ONE float64 oracle solve of the stacked batch
    [x0, x0 nudged one ulp up, x0 nudged one ulp down] (the problems of a batch are independent)."""
    b = x0.shape[0]
    stacked = torch.cat([x0, torch.nextafter(x0, torch.full_like(x0, float("inf"))),
                         torch.nextafter(x0, torch.full_like(x0, -float("inf")))])
    fn = _closure(torch.cat([obs] * 3), torch.cat([vis] * 3), m, n, distortion, ray)
    rec = solver.SolveRecord(None, None)
    full = solver.bfgs_solve(stacked, fn, record=rec, trajectory=trajectory, **kw)
    ref = full[:b]
    f = _envelope_factor()
    blocks = {"all": slice(None), "intrinsics": slice(0, 3)}
    if distortion:
        blocks["distortion"] = slice(-5, None)
    env = {}
    for name, cols in blocks.items():
        spread = torch.maximum(_rel(full[b:2 * b, cols], ref[:, cols]), _rel(full[2 * b:, cols], ref[:, cols]))
        env[name] = torch.maximum(torch.full((b,), TOL, dtype=torch.float64), f * spread)
    rec.iterations, rec.reason = rec.iterations[:b], rec.reason[:b]
    return ref, rec, env


@functools.lru_cache(maxsize=None)
def _oracle_solve(shape, k):
    """The fixed-K reference of a shape, computed once and shared."""
    m, n, distortion, ray, seed = SHAPES[shape]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    return _oracle_with_envelopes(x0, obs, vis, m, n, distortion, ray, iterations=k, error_threshold=-1.0,
                                  minimum_step=-1.0)


def _blocks(out, ref, distortion):
    rel = {"all": _rel(out, ref), "intrinsics": _rel(out[:, :3], ref[:, :3])}
    if distortion:
        rel["distortion"] = _rel(out[:, -5:], ref[:, -5:])
    return rel


def _report(tag, rel, env):
    """One PARITY line per case (pytest -s shows them; profiles/f64_parity.jsonl keeps a run's lines)."""
    rec = {"case": tag}
    for block in rel:
        rec[block] = {"max_rel": float(rel[block].max()), "max_bound": float(env[block].max()),
                      "max_ratio": float((rel[block] / env[block]).max())}
    print("PARITY", json.dumps(rec))


def _gpu_solve(device, x0, obs, vis, m, n, distortion, ray, **kw):
    from deep_attention_visual_odometry_amd import BFGSSolver

    s = BFGSSolver(**kw).eval()
    out = s(x0.to(device), _fn(device, obs, vis, m, n, distortion, ray))
    assert out.dtype == torch.float64 and out.device.type == "cuda"
    return out.cpu(), (None if s.last_status is None else s.last_status.cpu())


@pytest.mark.parametrize("k", [3, 20])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fixed_iterations_match_the_float64_oracle(device, shape, k):
    """K = 3: steepest descent, the initial scale and the first history entry; K = 20: the history products.

    Measured on the MI355X (max over problems of error / bound, per block): DESIGN.md 3.8
    (all at or below 0.072)."""
    from deep_attention_visual_odometry_amd._native import STOP_ITERATIONS

    m, n, distortion, ray, seed = SHAPES[shape]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    ref, rec, env = _oracle_solve(shape, k)
    out, status = _gpu_solve(device, x0, obs, vis, m, n, distortion, ray, iterations=k, error_threshold=-1.0,
                             minimum_step=-1.0)
    rel = _blocks(out, ref, distortion)
    _report(f"fixed64_{shape}_K{k}", rel, env)
    assert (status[:, 0] == k).all() and torch.equal(status[:, 0], rec.iterations)
    assert (status[:, 1] == STOP_ITERATIONS).all()
    for block in rel:
        assert (rel[block] <= env[block]).all(), (block, rel[block].tolist(), env[block].tolist())


# ---- 4. the reference's stopping rules ----

@functools.lru_cache(maxsize=None)
def _stopping_scene(case):
    if case == "seed15":
        return _scene(4, 2, 64, False, 15)
    rows = [tuple(t[i] for t in _scene(4, 2, 64, False, seed)) for seed, i in FACTOR2_PROBLEMS]
    return tuple(torch.stack([r[j] for r in rows]) for j in range(3))


@pytest.mark.parametrize("case,margin", [("factor2", 2.0), ("seed15", 1.01)])
def test_reference_stopping_rules(device, case, margin):
    """(2, 64) pinhole, B = 4, the reference's defaults 1e-4 / 1000 / 1e-8: steps and stop reasons equal the
    float64 oracle's SolveRecord and the result is held to the fixed-K bound.

    Agreement must not hang on a last-bit comparison, so every problem's oracle error at its stop iteration and
    at the one before are required (asserted below, on the CPU) to be a factor `margin` away from the threshold.
    factor2: a factor 2.  No make_scenes seed in 0 .. 399 gives four such problems at once (6 of the 1600
    problems qualify: the objective usually falls by less than 4x in its last step), so the batch is assembled
    from four of those, FACTOR2_PROBLEMS = (seed, row); they stop after 3, 4, 4, 4 steps.
    seed15: seed 15 as it is (stops after 9, 24, 11, 5 steps, all by the error rule): longer solves, with the
    margin it has -- the nearest error is 1.7% from the threshold (9.83e-5 / 1.0175e-4), against differences of
    ~1e-13 between the kernel and the oracle."""
    m, n, b = 2, 64, 4
    x0, obs, vis = _stopping_scene(case)
    traj = []
    ref, rec, env = _oracle_with_envelopes(x0, obs, vis, m, n, False, False, trajectory=traj)
    assert (rec.reason == solver.STOP_ERROR).all()
    for i in range(b):
        s = int(rec.iterations[i])
        at_stop = objective.reprojection_error(traj[s - 1][i:i + 1], obs[i:i + 1], vis[i:i + 1], m, n).item()
        before = objective.reprojection_error((traj[s - 2] if s >= 2 else x0)[i:i + 1], obs[i:i + 1], vis[i:i + 1],
                                              m, n).item()
        assert at_stop <= 1e-4 / margin and before >= margin * 1e-4, (i, s, at_stop, before)
    out, status = _gpu_solve(device, x0, obs, vis, m, n, False, False)
    rel = _blocks(out, ref, False)
    _report(f"stopping64_{case}_m2_n64", rel, env)
    assert torch.equal(status[:, 0], rec.iterations), (status[:, 0].tolist(), rec.iterations.tolist())
    assert torch.equal(status[:, 1], rec.reason)
    for block in rel:
        assert (rel[block] <= env[block]).all(), (block, rel[block].tolist(), env[block].tolist())


# ---- 5. determinism ----

def test_launches_are_deterministic_and_problems_independent(device):
    m, n, distortion, ray, seed = SHAPES["m3_n70_bc"]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    kw = dict(iterations=12, error_threshold=-1.0, minimum_step=-1.0)
    a, st_a = _gpu_solve(device, x0, obs, vis, m, n, distortion, ray, **kw)
    b, st_b = _gpu_solve(device, x0, obs, vis, m, n, distortion, ray, **kw)
    assert torch.equal(a, b) and torch.equal(st_a, st_b)
    for i in range(B):
        one, st = _gpu_solve(device, x0[i:i + 1], obs[i:i + 1], vis[i:i + 1], m, n, distortion, ray, **kw)
        assert torch.equal(one[0], a[i]) and torch.equal(st[0], st_a[i])


# ---- 6. the drop-in surface ----

def test_drop_in_fused_and_generic_routes(device):
    from deep_attention_visual_odometry_amd import BFGSSolver

    m, n, distortion, ray, seed = SHAPES["m2_n5"]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    ref, _, env = _oracle_solve("m2_n5", 20)
    kw = dict(iterations=20, error_threshold=-1.0, minimum_step=-1.0)
    out, status = _gpu_solve(device, x0, obs, vis, m, n, distortion, ray, **kw)
    assert status is not None and status.shape == (B, 4)
    # dense mode has no float64 kernel: the generic loop runs with the float64 objective as its closure
    dense, st = _gpu_solve(device, x0, obs, vis, m, n, distortion, ray, hessian_mode="dense", **kw)
    assert st is None
    rel = _blocks(dense, ref, distortion)
    _report("generic64_dense_m2_n5_K20", rel, env)
    for block in rel:
        assert (rel[block] <= env[block]).all(), (block, rel[block].tolist(), env[block].tolist())
    # more iterations than the history holds: the generic loop too (default stopping rules end it early)
    long_run, st = _gpu_solve(device, x0, obs, vis, m, n, distortion, ray, iterations=1030)
    assert st is None and torch.isfinite(long_run).all()
    # float64 parameters that require grad: second derivatives are float32 only
    with pytest.raises(TypeError):
        BFGSSolver(**kw).eval()(x0.to(device).requires_grad_(True), _fn(device, obs, vis, m, n, distortion, ray))


def test_batch_dimensions_and_a_nan_problem(device):
    from deep_attention_visual_odometry_amd import BFGSSolver, ReprojectionError
    from deep_attention_visual_odometry_amd._native import STOP_ERROR

    m, n = 2, 5
    x0, obs, vis = _scene(4, m, n, False, 41)
    kw = dict(iterations=10, error_threshold=-1.0, minimum_step=-1.0)
    flat, st_flat = _gpu_solve(device, x0, obs, vis, m, n, False, False, **kw)
    s = BFGSSolver(**kw).eval()
    boxed = s(x0.reshape(2, 2, -1).to(device),
              ReprojectionError(obs.reshape(2, 2, m, n, 2).to(device), vis.reshape(2, 2, m, n).to(device), m, n))
    assert boxed.shape == (2, 2, x0.shape[-1]) and torch.equal(boxed.cpu().reshape(4, -1), flat)
    bad = x0.clone()
    bad[1, 4] = float("nan")
    out, status = _gpu_solve(device, bad, obs, vis, m, n, False, False, **kw)
    assert status[1, 0] == 0 and status[1, 1] == STOP_ERROR
    assert torch.equal(out[[0, 2, 3]], flat[[0, 2, 3]]) and torch.equal(status[[0, 2, 3]], st_flat[[0, 2, 3]])


# ---- 7. fp32 is untouched ----

def test_float32_solve_is_untouched(device):
    from deep_attention_visual_odometry_amd import BFGSSolver, ReprojectionError, native_ops
    from deep_attention_visual_odometry_amd._native import DAVA_HESSIAN_COMPACT

    m, n, distortion, ray, seed = SHAPES["m3_n70_bc"]
    x64, obs64, vis = _scene(B, m, n, distortion, seed)
    x32, obs32 = x64.float().to(device), obs64.float().to(device)
    kw = dict(iterations=15, error_threshold=-1.0, minimum_step=-1.0)
    before = BFGSSolver(**kw).eval()(x32, ReprojectionError(obs32, vis.to(device), m, n, distortion))
    fn64 = ReprojectionError(obs64.to(device), vis.to(device), m, n, distortion)
    out64 = BFGSSolver(**kw).eval()(x64.to(device), fn64)
    assert out64.dtype == torch.float64
    after = BFGSSolver(**kw).eval()(x32, ReprojectionError(obs32, vis.to(device), m, n, distortion))
    mixed = BFGSSolver(**kw).eval()(x32, fn64)  # float32 parameters on a float64-capable objective: float32
    direct, _, _ = native_ops.ba_solve(x32, obs32, vis.to(device), m, n, distortion, iterations=15,
                                       error_threshold=-1.0, minimum_step=-1.0, hessian_mode=DAVA_HESSIAN_COMPACT)
    assert torch.equal(before, after) and torch.equal(before, mixed) and torch.equal(before, direct)
    assert before.dtype == torch.float32
