"""Differentiating through the float64 fused path: the float64 second derivatives (dava_ba_second_order_f64), the
objectives' float64 autograd behind float64_derivatives=True, the recording float64 solve and its adjoint kernel
(dava_ba_solve_record_f64, dava_ba_solve_backward_f64) and the drop-in BFGSSolver's routes, against the CPU
oracle run in float64 with autograd.

Bars.  Second derivatives: the float32 tests' bars (test_gpu_solve_grad.py: gradients 1e-4, second-order outputs
1e-3, normwise per problem) in units of machine epsilon, i.e. times 2^-29: 1.9e-13 and 1.9e-12.  The float64
oracle against itself with the points permuted differs by at most 2.4e-16 (gradients) and 3.0e-16 (second-order
outputs) on these shapes, so the bars leave about four orders of magnitude and still catch a float literal (1e-8).
Adjoint: per problem and per gradient (d/dx0, d/dobs of w . x_K)
max(2e-3 * 2^-29, F x the oracle gradient's own change when x0 is nudged one ulp up and down), 2e-3 the float32
adjoint test's bar and F the envelope_factor of tests/golden/parity_envelope.json; the nudged copies ride in the
same stacked oracle solve (the problems of a batch are independent).  The one widening is the float32 test's own
rule for the ray angle: 4 x the generic loop's distance from the oracle on the same inputs.
x_out: test_gpu_f64.py's solve bound (1e-5 * 2^-29 or F x the oracle's spread, per block).

Shapes (B = 3), test_gpu_f64.py's: (2, 5) fewer points than a wave; (3, 70) Brown-Conrady, P = 230 is no multiple
of 4 and two views move; (2, 130) ray angle; (2, 260) more points than threads.

Measured on the MI355X: profiles/f64_adjoint_parity.jsonl (the PARITY lines of one run), DESIGN.md 3.8.
"""
import functools
import json
import os

import pytest
import torch

from conftest import GOLDEN
from oracle import objective, solver

pytestmark = pytest.mark.gpu

EPS_RATIO = 2.0 ** -29  # float64 epsilon / float32 epsilon
G_TOL, H_TOL = 1e-4 * EPS_RATIO, 1e-3 * EPS_RATIO  # first-order outputs, second-order outputs
ADJ_TOL = 2e-3 * EPS_RATIO
X_TOL = 1e-5 * EPS_RATIO
B = 3
# name -> (M, N, distortion, ray angle, scene seed)
SHAPES = {
    "m2_n5": (2, 5, False, False, 31),
    "m3_n70_bc": (3, 70, True, False, 32),
    "m2_n130_ray": (2, 130, False, True, 33),
    "m2_n260": (2, 260, False, False, 34),
}
# (make_scenes seed, row) of (2, 64) problems whose last step crosses the threshold by a factor 2 (test_gpu_f64.py)
FACTOR2_PROBLEMS = ((13, 2), (71, 1), (191, 1), (200, 1))


def _envelope_factor():
    with open(os.path.join(GOLDEN, "parity_envelope.json")) as fh:
        return float(json.load(fh)["envelope_factor"])


@functools.lru_cache(maxsize=None)
def _scene(b, m, n, distortion, seed):
    """make_scenes as test_gpu_f64._scene builds them, cast to double (shared, never modified)."""
    from deep_attention_visual_odometry_amd import make_scenes

    s = make_scenes(b, m, n, distortion=distortion, seed=seed, drop=0.0 if distortion else 0.1)
    return torch.tensor(s.initial).double(), torch.tensor(s.observations).double(), torch.tensor(s.visibility)


def _weights(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _objective(x, obs, vis, m, n, distortion, ray):
    if ray:
        return objective.ray_angle_error(x, obs, vis, m, n)
    return objective.reprojection_error(x, obs, vis, m, n, distortion)


def _closure(obs, vis, m, n, distortion, ray):
    return objective.RayAngleClosure(obs, vis, m, n) if ray else objective.ReprojectionClosure(obs, vis, m, n, distortion)


def _fn(device, obs, vis, m, n, distortion, ray, **kw):
    """The fused objective on the device (obs: a CPU tensor, or a device tensor that may require grad)."""
    from deep_attention_visual_odometry_amd import RayAngleError, ReprojectionError

    if ray:
        return RayAngleError(obs.to(device), vis.to(device), m, n, **kw)
    return ReprojectionError(obs.to(device), vis.to(device), m, n, distortion, **kw)


def _rows_rel(a, b):
    a, b = a.reshape(a.shape[0], -1).double(), b.reshape(b.shape[0], -1).double()
    rel = (a - b).norm(dim=-1) / b.norm(dim=-1)
    bad_a, bad_b = ~torch.isfinite(a).all(dim=-1), ~torch.isfinite(b).all(dim=-1)
    rel[bad_a & bad_b] = 0.0
    rel[bad_a != bad_b] = float("inf")
    return rel


# ---- 1. second derivatives ----

def _second_oracle(x, obs, vis, m, n, distortion, ray, v, u):
    """(E, dE/dx, dE/dobs, H v + (d2E/dx dobs) u, (d2E/dobs dx) v + (d2E/dobs2) u) by torch double backward
    through the float64 oracle (test_gpu_solve_grad._second_oracle_obs without the casts)."""
    xr = x.clone().requires_grad_(True)
    orr = obs.clone().requires_grad_(True)
    e = _objective(xr, orr, vis, m, n, distortion, ray)
    g, og = torch.autograd.grad(e.sum(), (xr, orr), create_graph=True)
    hv, ohv = torch.autograd.grad((g * v).sum() + (og * u).sum(), (xr, orr))
    return e.detach(), g.detach(), og.detach(), hv, ohv


def _directions(x, obs, which):
    gen = torch.Generator().manual_seed(4)
    u = torch.randn(obs.shape, generator=gen, dtype=torch.float64) * 1e-2
    v = torch.randn(x.shape, generator=gen, dtype=torch.float64) * x.abs().clamp(min=0.1) * 1e-2
    return (v if which in ("v", "both") else None), (u if which in ("u", "both") else None)


def _check_second_order(device, x, obs, vis, m, n, distortion, ray, which, tag, undefined=None):
    """`undefined` (a slice of parameter entries): where the ORACLE's H v is NaN -- a rotation that is exactly zero,
    whose norm torch differentiates twice into 0 * inf.  Asserted to be exactly those entries; the kernel must be
    finite there (the dual number of sqrt(0) carries a zero tangent, torch's first-order subgradient), and every
    other entry of every output is compared as usual."""
    from deep_attention_visual_odometry_amd import native_ops

    v, u = _directions(x, obs, which)
    e_ref, g_ref, og_ref, hv_ref, ohv_ref = _second_oracle(
        x, obs, vis, m, n, distortion, ray, torch.zeros_like(x) if v is None else v,
        torch.zeros_like(obs) if u is None else u)
    dv = lambda t: None if t is None else t.to(device)  # noqa: E731
    e, g, hv, og, ohv = native_ops.ba_second_order_f64(dv(x), dv(obs), dv(vis), m, n, distortion, direction=dv(v),
                                                       residual=1 if ray else 0, obs_direction=dv(u))
    assert e.dtype == g.dtype == hv.dtype == og.dtype == ohv.dtype == torch.float64
    hv_all = hv
    if undefined is not None:
        nan = ~torch.isfinite(hv_ref)
        expected = torch.zeros_like(nan)
        expected[:, undefined] = True
        assert torch.equal(nan, expected) and torch.isfinite(hv).all()
        hv_ref, hv = hv_ref.clone(), hv.clone()
        hv_ref[:, undefined] = 0.0
        hv[:, undefined] = 0.0
    err = {"E": ((e.cpu() - e_ref).abs() / e_ref.abs()).max().item(), "grad": _rows_rel(g.cpu(), g_ref).max().item(),
           "obs_grad": _rows_rel(og.cpu(), og_ref).max().item(), "hv": _rows_rel(hv.cpu(), hv_ref).max().item(),
           "obs_hv": _rows_rel(ohv.cpu(), ohv_ref).max().item()}
    print("SECOND64", json.dumps({"case": tag, **err, "bars": [G_TOL, H_TOL]}))
    assert err["E"] <= G_TOL and err["grad"] <= G_TOL and err["obs_grad"] <= G_TOL, err
    assert err["hv"] <= H_TOL and err["obs_hv"] <= H_TOL, err
    # every output is nullable: the launch without the observation outputs gives the same H v
    _, _, hv2, og2, ohv2 = native_ops.ba_second_order_f64(dv(x), dv(obs), dv(vis), m, n, distortion, direction=dv(v),
                                                          residual=1 if ray else 0, want_obs=False,
                                                          obs_direction=dv(u))
    assert og2 is None and ohv2 is None and torch.equal(hv2, hv_all)


@pytest.mark.parametrize("which", ["v", "u", "both"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_second_order_matches_the_float64_oracle(device, shape, which):
    m, n, distortion, ray, seed = SHAPES[shape]
    x, obs, vis = _scene(B, m, n, distortion, seed)
    _check_second_order(device, x, obs, vis, m, n, distortion, ray, which, f"{shape}_{which}")


@pytest.mark.parametrize("norm2", [1e-3, 0.03])
def test_second_order_taylor_branches(device, norm2):
    """test_gpu_f64.test_taylor_branches' inputs: view 1's rotation exactly zero, view 2's of norm 1e-3 (both
    series) or 0.03 (between the thresholds).  The series' derivatives are taken by the dual numbers too: a
    float literal left in one shows at the 1e-8 level.  The oracle's own H v is NaN on view 1's three rotation
    entries (checked on the CPU: torch's double backward of |w| at w = 0); they are asserted to be the only
    such entries and left out of the comparison, every other entry and output is held to the bars."""
    m, n, distortion, ray, seed = SHAPES["m3_n70_bc"]
    x, obs, vis = _scene(B, m, n, distortion, seed)
    x = x.clone()
    rot = 3 + 3 * n + 3 * (m - 1)
    x[:, rot:rot + 3] = 0.0
    w = torch.tensor([0.6, -0.48, 0.64], dtype=torch.float64)
    x[:, rot + 3:rot + 6] = w / w.norm() * norm2
    _check_second_order(device, x, obs, vis, m, n, distortion, ray, "both", f"taylor_{norm2}",
                        undefined=slice(rot, rot + 3))


# ---- 2. objective-level autograd with the keyword ----

@pytest.mark.parametrize("shape", ["m3_n70_bc", "m2_n130_ray"])
def test_objective_autograd_in_float64(device, shape):
    """create_graph double backward, dE/dobs, and the double backward of dE/dobs of an objective built with
    float64_derivatives=True, against the oracle's."""
    m, n, distortion, ray, seed = SHAPES[shape]
    x, obs, vis = _scene(B, m, n, distortion, seed)
    v, u = _directions(x, obs, "both")
    mask = torch.ones(B, dtype=torch.bool, device=device)
    _, g_ref, og_ref, hv_ref, ohv_ref = _second_oracle(x, obs, vis, m, n, distortion, ray, v, torch.zeros_like(obs))
    _, _, _, hu_ref, ohu_ref = _second_oracle(x, obs, vis, m, n, distortion, ray, torch.zeros_like(x), u)

    def run():
        xd = x.to(device).requires_grad_(True)
        od = obs.to(device).requires_grad_(True)
        e = _fn(device, od, vis, m, n, distortion, ray, float64_derivatives=True)(xd, mask)
        assert e.dtype == torch.float64
        return xd, od, e

    xd, od, e = run()  # create_graph: d/d(x, obs) of v . dE/dx
    (g,) = torch.autograd.grad(e.sum(), xd, create_graph=True)
    hv, ohv = torch.autograd.grad((g * v.to(device)).sum(), (xd, od))
    assert _rows_rel(g.detach().cpu(), g_ref).max() <= G_TOL
    assert _rows_rel(hv.cpu(), hv_ref).max() <= H_TOL and _rows_rel(ohv.cpu(), ohv_ref).max() <= H_TOL
    xd, od, e = run()  # first order in the observations
    (go,) = torch.autograd.grad(e.sum(), od)
    assert go.dtype == torch.float64 and _rows_rel(go.cpu(), og_ref).max() <= G_TOL
    xd, od, e = run()  # dE/dobs differentiated again
    (go,) = torch.autograd.grad(e.sum(), od, create_graph=True)
    hu, ohu = torch.autograd.grad((go * u.to(device)).sum(), (xd, od))
    assert _rows_rel(hu.cpu(), hu_ref).max() <= H_TOL and _rows_rel(ohu.cpu(), ohu_ref).max() <= H_TOL
    # without the keyword: today's refusals
    xd = x.to(device).requires_grad_(True)
    e = _fn(device, obs, vis, m, n, distortion, ray)(xd, mask)
    with pytest.raises(TypeError):
        torch.autograd.grad(e.sum(), xd, create_graph=True)
    with pytest.raises(TypeError):
        _fn(device, obs.to(device).requires_grad_(True), vis, m, n, distortion, ray)(xd, mask)


# ---- 3. the recording launch ----

@pytest.mark.parametrize("shape", list(SHAPES))
def test_recording_is_bitwise_the_solve_and_deterministic(device, shape):
    """x, error and status of the recording launch equal the plain float64 solve's bit for bit, at a fixed
    K = 12 and under stopping rules that end the problems early (the tape's unreached slots are zeroed); two
    recordings give byte-identical tapes whatever the memory held before."""
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray, seed = SHAPES[shape]
    x0, obs, vis = (t.to(device) for t in _scene(B, m, n, distortion, seed))
    vis = vis.to(torch.uint8)
    res = 1 if ray else 0
    early = 0
    for thr, k, min_step in ((-1.0, 12, -1.0), (1e-4, 30, 1e-8), (1e30, 5, 1e-8), (-1.0, 1, -1.0)):
        x, err, st = native_ops.ba_solve(x0, obs, vis, m, n, distortion, error_threshold=thr, iterations=k,
                                         minimum_step=min_step, hessian_mode=1, want_error=True, want_status=True,
                                         residual=res)
        args = (x0, obs, vis, m, n, distortion, 1e-4, 0.9, thr, k, min_step, 1000, True, res, True)
        xr, st_r, tape, err_r = torch.ops.dava.ba_solve_record_f64(*args)
        assert torch.equal(x, xr) and torch.equal(st, st_r) and torch.equal(err, err_r)
        early += int((st[:, 0] < k).sum())
        first = tape.clone()
        junk = torch.empty_like(tape).fill_(255)  # the next tape's allocation starts as 0xFF bytes
        del tape, junk
        _, _, tape, _ = torch.ops.dava.ba_solve_record_f64(*args)
        assert torch.equal(tape, first)
        # the tape's x_0 row is x0, its last word block is the 256-byte tail
        p, pv = x0.shape[1], (x0.shape[1] + 3) // 4 * 4
        words = first[:first.numel() - 256].view(torch.float64)
        rows = words[B * 2 * max(k - 1, 1) * pv:][:B * k * pv].reshape(B, k, pv)
        started = (st[:, 0] > 0).cpu()
        assert torch.equal(rows[:, 0, :p].cpu()[started], x0.cpu()[started])
        assert (rows[:, 0, :p].cpu()[~started] == 0).all()
    assert early >= B  # (the 1e30 threshold stops every problem before its first step)


# ---- 4. the adjoint against the oracle ----

def _oracle_grads(x0, obs, vis, m, n, distortion, ray, w, trajectory=None, **kw):
    """ONE float64 oracle solve with autograd of the stacked batch [x0, x0 one ulp up, x0 one ulp down]: the
    reference x_K, d (w . x_K) / d x0 and / d obs, the SolveRecord of all three copies, and per problem the
    bounds on both gradients and (per block, as test_gpu_f64._oracle_with_envelopes) on x_K."""
    b = x0.shape[0]
    stacked = torch.cat([x0, torch.nextafter(x0, torch.full_like(x0, float("inf"))),
                         torch.nextafter(x0, torch.full_like(x0, -float("inf")))]).requires_grad_(True)
    obs3 = torch.cat([obs] * 3).requires_grad_(True)
    rec = solver.SolveRecord(None, None)
    out = solver.bfgs_solve(stacked, _closure(obs3, torch.cat([vis] * 3), m, n, distortion, ray), record=rec,
                            trajectory=trajectory, **kw)
    (out * torch.cat([w] * 3)).sum().backward()
    out, gx, go = out.detach(), stacked.grad, obs3.grad
    f = _envelope_factor()

    def bound(t, floor, cols=slice(None)):
        ref = t[:b].reshape(b, -1)[:, cols]
        spread = torch.maximum(_rows_rel(t[b:2 * b].reshape(b, -1)[:, cols], ref),
                               _rows_rel(t[2 * b:].reshape(b, -1)[:, cols], ref))
        return torch.maximum(torch.full((b,), floor, dtype=torch.float64), f * spread), spread

    blocks = {"all": slice(None), "intrinsics": slice(0, 3)}
    if distortion:
        blocks["distortion"] = slice(-5, None)
    bx, sx = bound(gx, ADJ_TOL)
    bo, so = bound(go, ADJ_TOL)
    return {"out": out[:b], "gx": gx[:b], "go": go[:b], "rec": rec, "bound_x": bx, "bound_obs": bo,
            "spread": (sx, so), "env_out": {name: bound(out, X_TOL, cols)[0] for name, cols in blocks.items()},
            "blocks": blocks}


@functools.lru_cache(maxsize=None)
def _oracle_fixed(shape, k):
    m, n, distortion, ray, seed = SHAPES[shape]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    return _oracle_grads(x0, obs, vis, m, n, distortion, ray, _weights(x0.shape, k), iterations=k,
                         error_threshold=-1.0, minimum_step=-1.0)


def _gpu_grads(device, x0, obs, vis, m, n, distortion, ray, w, **kw):
    from deep_attention_visual_odometry_amd import BFGSSolver

    xd = x0.to(device).requires_grad_(True)
    od = obs.to(device).requires_grad_(True)
    s = BFGSSolver(**kw).eval()
    out = s(xd, _fn(device, od, vis, m, n, distortion, ray, float64_derivatives=True))
    assert out.dtype == torch.float64 and out.requires_grad
    (out * w.to(device)).sum().backward()
    assert xd.grad.dtype == od.grad.dtype == torch.float64
    return out.detach().cpu(), xd.grad.cpu(), od.grad.cpu(), (None if s.last_status is None else s.last_status.cpu())


def _report(tag, ex, eo, ref):
    print("PARITY", json.dumps({"case": tag, "x0": {"max_err": float(ex.max()), "max_bound": float(ref["bound_x"].max()),
                                                      "max_ratio": float((ex / ref["bound_x"]).max())},
                                "obs": {"max_err": float(eo.max()), "max_bound": float(ref["bound_obs"].max()),
                                        "max_ratio": float((eo / ref["bound_obs"]).max())}}))


def _check_out(out, ref):
    for name, cols in ref["blocks"].items():
        rel = _rows_rel(out[:, cols], ref["out"][:, cols])
        assert (rel <= ref["env_out"][name]).all(), (name, rel.tolist(), ref["env_out"][name].tolist())


@pytest.mark.parametrize("k", [1, 2, 3, 12])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_adjoint_matches_the_float64_oracle(device, shape, k, overrides):
    """K = 1: only d_0 = -g_0; K = 2: the gamma adjoint; K = 3: the first history pass; K = 12: the passes proper.

    Measured on the MI355X (max over problems of error / bound): profiles/f64_adjoint_parity.jsonl, DESIGN.md 3.8."""
    m, n, distortion, ray, seed = SHAPES[shape]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    ref = _oracle_fixed(shape, k)
    w = _weights(x0.shape, k)
    kw = dict(iterations=k, error_threshold=-1.0, minimum_step=-1.0)
    out, gx, go, st = _gpu_grads(device, x0, obs, vis, m, n, distortion, ray, w, **kw)
    assert st is not None and (st[:, 0] == k).all() and torch.equal(st[:, 0], ref["rec"].iterations[:B])
    _check_out(out, ref)
    ex, eo = _rows_rel(gx, ref["gx"]), _rows_rel(go, ref["go"])
    _report(f"adjoint64_{shape}_K{k}", ex, eo, ref)
    bx, bo = ref["bound_x"], ref["bound_obs"]
    if ray and not ((ex <= bx).all() and (eo <= bo).all()):
        # the float32 adjoint test's rule for the ray angle (its Hessian grows like 1 / |residual|): 4 x the
        # generic loop's own distance from the oracle on the same inputs
        overrides("GENERIC_BACKWARD", 1)
        _, gx_g, go_g, st_g = _gpu_grads(device, x0, obs, vis, m, n, distortion, ray, w, **kw)
        assert st_g is None
        bx = torch.maximum(bx, 4.0 * _rows_rel(gx_g, ref["gx"]))
        bo = torch.maximum(bo, 4.0 * _rows_rel(go_g, ref["go"]))
        print("PARITY", json.dumps({"case": f"adjoint64_{shape}_K{k}_ray_rule", "x0_ratio": float((ex / bx).max()),
                                    "obs_ratio": float((eo / bo).max())}))
    assert (ex <= bx).all(), (ex.tolist(), bx.tolist())
    assert (eo <= bo).all(), (eo.tolist(), bo.tolist())


def _adjoint_image_bytes(m, n, p, obs_in_lds):
    """csrc/bfgs_adjoint_f64.hip carve_adjoint: 14 vectors of Pv doubles, the dual view constants and per-wave
    partials, reduction scratch, a chunk's coefficients, the observations (and their cotangent), visibility."""
    pv = (p + 3) // 4 * 4
    doubles = 14 * pv + 2 * 24 * (m - 1) + 2 * 32 * m + 2 * 4 * 32 + 4 * 32 + (4 if obs_in_lds else 2) * m * n
    return 8 * doubles + (m * n + 15) // 16 * 16


def test_adjoint_with_the_observation_cotangent_in_the_output(device):
    """(8, 256), P = 813: the adjoint's image with the observation cotangent in LDS is past 160 KiB, so the kernel
    accumulates it in the output instead (its other path); K = 3 against the oracle, rule 4's bound."""
    from deep_attention_visual_odometry_amd import native_ops

    m, n, k = 8, 256, 3
    x0, obs, vis = _scene(B, m, n, False, 35)
    assert _adjoint_image_bytes(m, n, x0.shape[1], True) > 160 * 1024 >= _adjoint_image_bytes(m, n, x0.shape[1], False)
    assert _adjoint_image_bytes(4, 256, 794, True) <= 160 * 1024  # (C3 keeps it in LDS)
    assert native_ops.solve_tape_supported_f64(B, m, n, False, k)
    w = _weights(x0.shape, k)
    kw = dict(iterations=k, error_threshold=-1.0, minimum_step=-1.0)
    ref = _oracle_grads(x0, obs, vis, m, n, False, False, w, **kw)
    out, gx, go, st = _gpu_grads(device, x0, obs, vis, m, n, False, False, w, **kw)
    assert st is not None and (st[:, 0] == k).all()
    _check_out(out, ref)
    ex, eo = _rows_rel(gx, ref["gx"]), _rows_rel(go, ref["go"])
    _report(f"adjoint64_m8_n256_obs_in_output_K{k}", ex, eo, ref)
    assert (ex <= ref["bound_x"]).all(), (ex.tolist(), ref["bound_x"].tolist())
    assert (eo <= ref["bound_obs"]).all(), (eo.tolist(), ref["bound_obs"].tolist())
    # without an observation gradient the same launch accumulates none, and d/dx0 is bitwise the same
    xd = x0.to(device).requires_grad_(True)
    xk, _ = native_ops.ba_solve_differentiable_f64(xd, obs.to(device), vis.to(device), m, n, False, **kw)
    (gx_only,) = torch.autograd.grad((xk * w.to(device)).sum(), xd)
    assert torch.equal(gx_only.cpu(), gx)


# ---- 5. the reference's stopping rules ----

@functools.lru_cache(maxsize=None)
def _stopping_scene():
    rows = [tuple(t[i] for t in _scene(4, 2, 64, False, seed)) for seed, i in FACTOR2_PROBLEMS]
    return tuple(torch.stack([r[j] for r in rows]) for j in range(3))


def test_adjoint_under_the_reference_stopping_rules(device):
    """(2, 64) pinhole, B = 4, the reference's defaults 1e-4 / 1000 / 1e-8: the problems stop after 3, 4, 4, 4
    steps by the error rule with a factor 2 of margin (test_gpu_f64.test_reference_stopping_rules), so the
    adjoint replays each problem's own steps; the oracle's nudged copies must stop at the same iterations."""
    m, n, b = 2, 64, 4
    x0, obs, vis = _stopping_scene()
    w = _weights(x0.shape, 5)
    traj = []
    ref = _oracle_grads(x0, obs, vis, m, n, False, False, w, trajectory=traj)
    rec = ref["rec"]
    assert (rec.reason == solver.STOP_ERROR).all() and rec.iterations[:b].tolist() == [3, 4, 4, 4]
    assert torch.equal(rec.iterations[b:2 * b], rec.iterations[:b]) and torch.equal(rec.iterations[2 * b:],
                                                                                    rec.iterations[:b])
    for i in range(b):
        s = int(rec.iterations[i])
        at_stop = objective.reprojection_error(traj[s - 1][i:i + 1], obs[i:i + 1], vis[i:i + 1], m, n).item()
        before = objective.reprojection_error(traj[s - 2][i:i + 1], obs[i:i + 1], vis[i:i + 1], m, n).item()
        assert at_stop <= 1e-4 / 2.0 and before >= 2.0 * 1e-4, (i, s, at_stop, before)
    out, gx, go, st = _gpu_grads(device, x0, obs, vis, m, n, False, False, w)
    assert torch.equal(st[:, 0], rec.iterations[:b]) and torch.equal(st[:, 1], rec.reason[:b])
    _check_out(out, ref)
    ex, eo = _rows_rel(gx, ref["gx"]), _rows_rel(go, ref["go"])
    _report("adjoint64_stopping_factor2_m2_n64", ex, eo, ref)
    assert (ex <= ref["bound_x"]).all(), (ex.tolist(), ref["bound_x"].tolist())
    assert (eo <= ref["bound_obs"]).all(), (eo.tolist(), ref["bound_obs"].tolist())


# ---- 6. routes ----

def test_fused_and_generic_backward_agree(device, overrides):
    m, n, distortion, ray, seed = SHAPES["m2_n5"]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    ref = _oracle_fixed("m2_n5", 12)
    w = _weights(x0.shape, 12)
    kw = dict(iterations=12, error_threshold=-1.0, minimum_step=-1.0)
    out, gx, go, st = _gpu_grads(device, x0, obs, vis, m, n, distortion, ray, w, **kw)
    overrides("GENERIC_BACKWARD", 1)
    out_g, gx_g, go_g, st_g = _gpu_grads(device, x0, obs, vis, m, n, distortion, ray, w, **kw)
    assert st is not None and st_g is None  # the recording solve + adjoint, then the generic loop
    _check_out(out_g, ref)
    for tag, a, b_ in (("fused_vs_generic", (gx, go), (gx_g, go_g)), ("generic_vs_oracle", (gx_g, go_g),
                                                                      (ref["gx"], ref["go"]))):
        ex, eo = _rows_rel(a[0], b_[0]), _rows_rel(a[1], b_[1])
        _report(f"route64_{tag}_m2_n5_K12", ex, eo, ref)
        assert (ex <= ref["bound_x"]).all() and (eo <= ref["bound_obs"]).all(), (tag, ex.tolist(), eo.tolist())


def test_dense_mode_takes_the_generic_loop(device):
    m, n, distortion, ray, seed = SHAPES["m2_n5"]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    ref = _oracle_fixed("m2_n5", 12)
    w = _weights(x0.shape, 12)
    out, gx, go, st = _gpu_grads(device, x0, obs, vis, m, n, distortion, ray, w, iterations=12, error_threshold=-1.0,
                                 minimum_step=-1.0, hessian_mode="dense")
    assert st is None
    _check_out(out, ref)
    ex, eo = _rows_rel(gx, ref["gx"]), _rows_rel(go, ref["go"])
    _report("route64_dense_m2_n5_K12", ex, eo, ref)
    assert (ex <= ref["bound_x"]).all() and (eo <= ref["bound_obs"]).all(), (ex.tolist(), eo.tolist())


def test_float32_gradients_are_untouched(device):
    """The float32 fused adjoint run before and after a float64 backward of the same scene gives bitwise the
    same x and gradients (and the float32 path still refuses nothing it took before)."""
    from deep_attention_visual_odometry_amd import BFGSSolver, ReprojectionError

    m, n, distortion, ray, seed = SHAPES["m3_n70_bc"]
    x64, obs64, vis = _scene(B, m, n, distortion, seed)
    w = _weights(x64.shape, 3)
    kw = dict(iterations=10, error_threshold=-1.0, minimum_step=-1.0)

    def run32(fn_obs=None):
        xd = x64.float().to(device).requires_grad_(True)
        od = obs64.float().to(device).requires_grad_(True)
        fn = ReprojectionError(od, vis.to(device), m, n, distortion) if fn_obs is None else fn_obs
        s = BFGSSolver(**kw).eval()
        out = s(xd, fn)
        (out * w.float().to(device)).sum().backward()
        assert out.dtype == torch.float32 and s.last_status is not None
        return out.detach(), xd.grad, (None if fn_obs is not None else od.grad)

    before = run32()
    _, gx64, go64, _ = _gpu_grads(device, x64, obs64, vis, m, n, distortion, ray, w, **kw)
    assert torch.isfinite(gx64).all() and torch.isfinite(go64).all()
    after = run32()
    for a, b_ in zip(before, after):
        assert torch.equal(a, b_)
    # float32 parameters on an objective built with the keyword: the float32 kernels, bit for bit
    fn64 = ReprojectionError(obs64.to(device), vis.to(device), m, n, distortion, float64_derivatives=True)
    mixed = run32(fn64)
    assert torch.equal(mixed[0], before[0]) and torch.equal(mixed[1], before[1])


# ---- 7. edges ----

def test_adjoint_edge_cases(device):
    m, n = 2, 5
    x0, obs, vis = _scene(4, m, n, False, 41)
    w = _weights(x0.shape, 7)
    kw = dict(iterations=10, error_threshold=-1.0, minimum_step=-1.0)
    # empty batch
    _, gx, go, _ = _gpu_grads(device, x0[:0], obs[:0], vis[:0], m, n, False, False, w[:0], iterations=5)
    assert gx.shape == x0[:0].shape and go.shape == obs[:0].shape
    # a threshold that stops before the first step: x_out = x0, the gradient is the cotangent itself
    out, gx, go, st = _gpu_grads(device, x0, obs, vis, m, n, False, False, w, error_threshold=1e30)
    assert (st[:, 0] == 0).all() and torch.equal(out, x0) and torch.equal(gx, w) and (go == 0).all()
    # two backward launches give bitwise the same gradients
    flat = _gpu_grads(device, x0, obs, vis, m, n, False, False, w, **kw)
    again = _gpu_grads(device, x0, obs, vis, m, n, False, False, w, **kw)
    assert all(torch.equal(a, b_) for a, b_ in zip(flat, again))
    assert torch.isfinite(flat[1]).all() and torch.isfinite(flat[2]).all() and flat[2].abs().max() > 0
    # a NaN row in x0 stops that problem at once and leaves the others' gradients bitwise unchanged
    bad = x0.clone()
    bad[1, 4] = float("nan")
    out, gx, go, st = _gpu_grads(device, bad, obs, vis, m, n, False, False, w, **kw)
    keep = [0, 2, 3]
    assert st[1, 0] == 0 and torch.equal(gx[1], w[1]) and (go[1] == 0).all()
    assert torch.equal(out[keep], flat[0][keep]) and torch.equal(gx[keep], flat[1][keep])
    assert torch.equal(go[keep], flat[2][keep]) and torch.equal(st[keep], flat[3][keep])
    # leading batch dimensions (2, 2)
    boxed = _gpu_grads(device, x0.reshape(2, 2, -1), obs.reshape(2, 2, m, n, 2), vis.reshape(2, 2, m, n), m, n, False,
                       False, w.reshape(2, 2, -1), **kw)
    assert boxed[0].shape == (2, 2, x0.shape[-1]) and boxed[2].shape == (2, 2, m, n, 2)
    assert torch.equal(boxed[0].reshape(4, -1), flat[0]) and torch.equal(boxed[1].reshape(4, -1), flat[1])
    assert torch.equal(boxed[2].reshape(4, m, n, 2), flat[2])
