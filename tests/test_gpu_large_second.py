"""The float32 dual-number kernels beyond the LDS image on the GPU: dava_ba_second_order_large and
dava_ba_sgd_backward_large in forms 1 and 2, and the route behind large_derivatives=True.

Forced on small shapes through the F32_DUAL_FORM override (bitwise form 0 there) and taken naturally by (2, 1800)
-- form 1 -- and by (2, 3600) and C5 (16, 4096) -- form 2 --, which dava_ba_second_order_obs and dava_ba_sgd_backward
refuse.

Bars.  Second derivatives, per row against the float64 double backward through oracle.objective (the construction of
test_gpu_solve_grad.py::_second_oracle_obs): 1e-4 for dE/dx and dE/dobs, 1e-3 for the two second-order outputs; the
float32 CPU oracle itself sits <= 5e-6 and <= 2.7e-5 from the float64 one at these scenes.  The descent's gradients,
against sgd_oracle.gradients in float64, measured as test_gpu_sgd.py does (per-row relative norm of x0.grad - w and
of observations.grad): 2e-3 for the squared objective, 2e-2 for the ray angle.  lr = 1e-5 there: at 1e-4 several of
these scenes diverge (C5's E grows 4,000x in three steps), at 1e-5 the float64 oracle's E decreases on every row,
which the test asserts as its precondition.

Every gradient case prints a PARITY line; a run of the whole gradient test rewrites profiles/sgd_large_parity.jsonl.
"""
import functools
import json
import os

import pytest
import torch

import sgd_oracle
from conftest import REPO
from oracle import objective

pytestmark = pytest.mark.gpu

B = 4
KNOB = "F32_DUAL_FORM"
# name: (M, N, distortion, ray, drop, seed) -- the three SGD shapes as tests/test_gpu_sgd.py declares them
SMALL = {
    "pinhole_2x64": (2, 64, False, False, 0.1, 9701),
    "bc_3x70": (3, 70, True, False, 0.0, 9703),
    "ray_2x130": (2, 130, False, True, 0.1, 9702),
    "past_ppt_2x257": (2, 257, False, False, 0.1, 9706),
}
SGD_SMALL = ("pinhole_2x64", "bc_3x70", "ray_2x130")
# name: (M, N, distortion, ray, drop, seed, form)
LARGE = {
    "pinhole_2x1800": (2, 1800, False, False, 0.1, 9721, 1),
    "ray_2x1800": (2, 1800, False, True, 0.1, 9722, 1),
    "pinhole_2x3600": (2, 3600, False, False, 0.1, 9723, 2),
    "bc_2x3600": (2, 3600, True, False, 0.0, 9725, 2),
}
C5 = {"c5_16x4096": (16, 4096, False, False, 0.0, 9707, 2)}
# The large ray-angle scene is make_scenes(2, 2, 1800, seed=9722, drop=0.1) as it stands, without the generator's
# ray_angle=True (which stores the focal slot in the ray objective's parameterisation): with it the float64 loop does
# not contract at lr = 1e-5 on row 0 (E = 56.0, 81.6, 59.2, 80.1 over four iterates), so the precondition below would
# not hold; as generated here E(x_2)/E(x_0) is 0.931 and 0.955 on its two rows.
PLAIN_GENERATOR = ("ray_2x1800",)
LR_LARGE = 1e-5
K_LARGE = 3


@functools.lru_cache(maxsize=None)
def _scene(name, batch):
    from deep_attention_visual_odometry_amd import make_scenes

    m, n, distortion, ray, drop, seed = {**SMALL, **LARGE, **C5}[name][:6]
    s = make_scenes(batch, m, n, distortion=distortion, seed=seed, drop=drop,
                    ray_angle=ray and name not in PLAIN_GENERATOR)
    return torch.tensor(s.initial), torch.tensor(s.observations), torch.tensor(s.visibility)


def _meta(name):
    m, n, distortion, ray = {**SMALL, **LARGE, **C5}[name][:4]
    return m, n, distortion, ray


@functools.lru_cache(maxsize=None)
def _directions(name, batch):
    """v scaled as test_gpu_solve_grad.py scales it, u = 1e-2 randn."""
    x, obs, _ = _scene(name, batch)
    gen = torch.Generator().manual_seed(4)
    u = torch.randn(obs.shape, generator=gen) * 1e-2
    v = torch.randn(x.shape, generator=gen) * x.abs().clamp(min=0.1) * 1e-2
    return v, u


def _second(device, name, batch, large, v=None, u=None, **kw):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray = _meta(name)
    x, obs, vis = (t.to(device) for t in _scene(name, batch))
    fn = native_ops.ba_second_order_large if large else native_ops.ba_second_order
    out = fn(x, obs, vis, m, n, distortion, direction=None if v is None else v.to(device), residual=1 if ray else 0,
             obs_direction=None if u is None else u.to(device), **kw)
    torch.cuda.synchronize(device)
    return tuple(None if t is None else t.cpu() for t in out)


def _same(a, b):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert (s is None) == (t is None)
        if s is not None:
            assert torch.equal(s, t)


def _rows_rel(a, b):
    return sgd_oracle.rows_rel(a, b)


# ---- 1. forms 1 and 2 are bitwise form 0 where all three run ----

@pytest.mark.parametrize("name", list(SMALL))
def test_second_order_forms_are_bitwise_form_0(device, overrides, name):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray = _meta(name)
    v, u = _directions(name, B)
    assert native_ops.second_order_form(B, m, n, distortion, 1 if ray else 0) == 0
    ref = _second(device, name, B, False, v, u)
    ref_hv = _second(device, name, B, False, v, u, want_obs=False)
    ref_v0 = _second(device, name, B, False, None, u)
    assert all(t is not None and torch.isfinite(t).all() for t in ref)
    for form in (1, 2):
        overrides(KNOB, form)
        assert native_ops.second_order_form(B, m, n, distortion, 1 if ray else 0) == form
        _same(_second(device, name, B, True, v, u), ref)
        _same(_second(device, name, B, True, v, u, want_obs=False), ref_hv)  # no dE/dobs workspace
        _same(_second(device, name, B, True, None, u), ref_v0)
        overrides(KNOB, -1)
    _same(_second(device, name, B, True, v, u), ref)  # without the override: form 0's operator


# ---- 2. genuine large shapes ----

@functools.lru_cache(maxsize=None)
def _second_oracle(name, batch):
    """(dE/dx, dE/dobs, H v + (d2E/dx dobs) u, (d2E/dobs dx) v + (d2E/dobs2) u) by double backward in float64."""
    m, n, distortion, ray = _meta(name)
    x, obs, vis = _scene(name, batch)
    v, u = _directions(name, batch)
    x64 = x.double().clone().requires_grad_(True)
    o64 = obs.double().clone().requires_grad_(True)
    if ray:
        e = objective.ray_angle_error(x64, o64, vis, m, n)
    else:
        e = objective.reprojection_error(x64, o64, vis, m, n, distortion)
    g, og = torch.autograd.grad(e.sum(), (x64, o64), create_graph=True)
    hv, ohv = torch.autograd.grad((g * v.double()).sum() + (og * u.double()).sum(), (x64, o64))
    return g.detach(), og.detach(), hv, ohv


@pytest.mark.parametrize("name", list(LARGE))
def test_second_order_at_large_shapes_matches_double_backward(device, overrides, name):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray = _meta(name)
    form = LARGE[name][6]
    assert native_ops.second_order_form(2, m, n, distortion, 1 if ray else 0) == form
    v, u = _directions(name, 2)
    out = _second(device, name, 2, True, v, u)
    g_ref, og_ref, hv_ref, ohv_ref = _second_oracle(name, 2)
    _, g, hv, og, ohv = out
    rels = {"g": _rows_rel(g, g_ref), "obs_grad": _rows_rel(og, og_ref), "hv": _rows_rel(hv, hv_ref),
            "obs_hv": _rows_rel(ohv, ohv_ref)}
    print("SECOND", name, form, {k: float(r.max()) for k, r in rels.items()})
    assert rels["g"].max() < 1e-4 and rels["obs_grad"].max() < 1e-4, rels
    assert rels["hv"].max() < 1e-3 and rels["obs_hv"].max() < 1e-3, rels
    if form == 1:  # form 2 under the override is bitwise form 1
        overrides(KNOB, 2)
        assert native_ops.second_order_form(2, m, n, distortion, 1 if ray else 0) == 2
        _same(_second(device, name, 2, True, v, u), out)


# ---- 3. the descent's adjoint: forms 1 and 2 are bitwise form 0 ----

def _sgd_gradients(device, name, batch, k, lr, w, large, obs_grad=True):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray = _meta(name)
    x0, obs, vis = _scene(name, batch)
    xg = x0.to(device).requires_grad_(True)
    og = obs.to(device).requires_grad_(obs_grad)
    solve = native_ops.ba_sgd_solve_differentiable_large if large else native_ops.ba_sgd_solve_differentiable
    out, errs = solve(xg, og, vis.to(device), m, n, distortion, learning_rate=lr, iterations=k,
                      residual=1 if ray else 0, want_errors=True)
    (out * w.to(device)).sum().backward()
    torch.cuda.synchronize(device)
    return out.detach().cpu(), errs.cpu(), xg.grad.cpu(), (og.grad.cpu() if obs_grad else None)


@pytest.mark.parametrize("name", SGD_SMALL)
def test_sgd_adjoint_forms_are_bitwise_form_0(device, overrides, name):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray = _meta(name)
    k, lr = 5, 1e-4
    w = torch.randn(_scene(name, B)[0].shape, generator=torch.Generator().manual_seed(k))
    assert native_ops.sgd_backward_form(B, m, n, distortion, k, 1 if ray else 0) == 0
    out, errs, gx, go = _sgd_gradients(device, name, B, k, lr, w, False)
    assert torch.isfinite(gx).all() and torch.isfinite(go).all()
    for form in (1, 2):
        overrides(KNOB, form)
        assert native_ops.sgd_backward_form(B, m, n, distortion, k, 1 if ray else 0) == form
        out_f, errs_f, gx_f, go_f = _sgd_gradients(device, name, B, k, lr, w, True)
        assert torch.equal(out_f, out) and torch.equal(errs_f, errs)
        assert torch.equal(gx_f, gx) and torch.equal(go_f, go), form
        # observations that do not require grad: a NULL observations_grad, no dE/dobs workspace
        _, _, gx_only, none = _sgd_gradients(device, name, B, k, lr, w, True, obs_grad=False)
        assert none is None and torch.equal(gx_only, gx)
        overrides(KNOB, -1)


# ---- 4. the descent's adjoint at genuine large shapes ----

@functools.lru_cache(maxsize=None)
def _sgd_oracle64(name, k, unit_w):
    """(w, dL/dx0, dL/dobs, E(x_k) (B, k)) of the float64 loop for L = (w . x_K).sum(), B = 2."""
    m, n, distortion, ray = _meta(name)
    x0, obs, vis = _scene(name, 2)
    w = torch.ones(x0.shape) if unit_w else torch.randn(x0.shape, generator=torch.Generator().manual_seed(k))
    _, gx, go = sgd_oracle.gradients(x0, obs, vis, m, n, distortion, ray, w, LR_LARGE, k, torch.float64)
    _, trace = sgd_oracle.descend(x0.double(), sgd_oracle.closure(obs.double(), vis, m, n, distortion, ray), LR_LARGE,
                                  k, trace=True)
    return w, gx, go, trace


def _gradient_distances(name, gx, go, k, unit_w=False):
    """Per row, as test_gpu_sgd.py measures: x0.grad - w (the identity part of dx_K/dx0 must not mask the solve's
    part) and observations.grad against the float64 loop; asserts the scene's precondition first."""
    w, gx64, go64, trace = _sgd_oracle64(name, k, unit_w)
    assert (trace[:, -1] < trace[:, 0]).all() and torch.isfinite(trace).all(), trace  # the descent contracts
    w64 = w.double()
    return _rows_rel(gx.double() - w64, gx64 - w64), _rows_rel(go, go64), trace


_PARITY_LINES = []


def _report(rec):
    print("PARITY", json.dumps(rec))
    _PARITY_LINES.append(json.dumps(rec))
    if {json.loads(line)["case"] for line in _PARITY_LINES} != set(LARGE) | set(C5):
        return
    try:
        with open(os.path.join(REPO, "profiles", "sgd_large_parity.jsonl"), "w") as fh:
            fh.write("\n".join(_PARITY_LINES) + "\n")
    except OSError:  # (a read-only checkout: the printed lines remain)
        pass


@pytest.mark.parametrize("name", list(LARGE) + list(C5))
def test_sgd_gradients_at_large_shapes_match_float64_autograd(device, name):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray = _meta(name)
    form = {**LARGE, **C5}[name][6]
    assert native_ops.sgd_backward_form(2, m, n, distortion, K_LARGE, 1 if ray else 0) == form
    assert not native_ops.sgd_backward_supported(2, m, n, distortion, K_LARGE, 1 if ray else 0)
    w = _sgd_oracle64(name, K_LARGE, False)[0]
    out, errs, gx, go = _sgd_gradients(device, name, 2, K_LARGE, LR_LARGE, w, True)
    rx, ro, trace = _gradient_distances(name, gx, go, K_LARGE)
    bar = 2e-2 if ray else 2e-3
    _report({"case": name, "form": form, "K": K_LARGE, "lr": LR_LARGE, "x0_grad": float(rx.max()),
             "obs_grad": float(ro.max()), "bar": bar, "E_ratio": [float(t) for t in trace[:, -1] / trace[:, 0]],
             "trace_to_f64": float(_rows_rel(errs, trace).max())})
    assert torch.isfinite(gx).all() and torch.isfinite(go).all()
    assert (rx <= bar).all() and (ro <= bar).all(), (rx, ro)


# ---- 5. slicing and determinism ----

def test_second_order_slices_and_is_deterministic(device):
    """(2, 3600), form 2: B = 5 in one launch is bitwise launches of 2 + 3 (the per-problem workspace slices), and two
    launches into a workspace pre-filled with NaN give identical, finite results."""
    from deep_attention_visual_odometry_amd import _native as N
    from deep_attention_visual_odometry_amd import _ops, native_ops

    name = "pinhole_2x3600"
    m, n, distortion, _ = _meta(name)
    x, obs, vis = (t.to(device) for t in _scene(name, 5))
    vis = vis.to(torch.uint8)
    v, u = (t.to(device) for t in _directions(name, 5))
    assert native_ops.second_order_form(5, m, n, distortion) == 2
    whole = native_ops.ba_second_order_large(x, obs, vis, m, n, distortion, direction=v, obs_direction=u)
    for lo, hi in ((0, 2), (2, 5)):
        part = native_ops.ba_second_order_large(x[lo:hi], obs[lo:hi], vis[lo:hi], m, n, distortion,
                                                direction=v[lo:hi], obs_direction=u[lo:hi])
        for s, t in zip(part, whole):
            assert torch.equal(s, t[lo:hi])
    lib = N.load_library()
    sc = _ops.scene_struct(obs, vis, m, n, distortion, 5)
    need = lib.dava_ba_second_order_large_workspace_bytes(sc, 1)
    runs = []
    for _ in range(2):
        ws = torch.full((need // 4 + 1,), float("nan"), device=device)
        outs = [torch.full((5,), float("nan"), device=device)] + [torch.full_like(x, float("nan")) for _ in range(2)] \
            + [torch.full_like(obs, float("nan")) for _ in range(2)]
        N.check(lib.dava_ba_second_order_large(sc, N.ptr(x), N.ptr(v), N.ptr(u), *(N.ptr(t) for t in outs), N.ptr(ws),
                                               ws.numel() * 4, N.stream_of(device)), "dava_ba_second_order_large")
        torch.cuda.synchronize(device)
        runs.append(outs)
    for s, t, r in zip(runs[0], runs[1], whole):
        assert torch.isfinite(s).all() and torch.equal(s, t) and torch.equal(s, r)


def test_sgd_adjoint_slices_and_is_deterministic(device):
    from deep_attention_visual_odometry_amd import _native as N
    from deep_attention_visual_odometry_amd import _ops, native_ops

    name, k = "pinhole_2x3600", 3
    m, n, distortion, _ = _meta(name)
    assert native_ops.sgd_backward_form(5, m, n, distortion, k) == 2
    x0, obs, vis = (t.to(device) for t in _scene(name, 5))
    vis = vis.to(torch.uint8)
    gout = torch.randn(x0.shape, generator=torch.Generator().manual_seed(2)).to(device)
    args = (m, n, distortion, LR_LARGE, k, 0)
    _, _, tape = torch.ops.dava.ba_sgd_solve_differentiable_large(x0, obs, vis, *args, False)
    gx, go = torch.ops.dava.ba_sgd_backward_large(gout, tape, obs, vis, *args, True)
    for lo, hi in ((0, 2), (2, 5)):
        _, _, tape_p = torch.ops.dava.ba_sgd_solve_differentiable_large(x0[lo:hi], obs[lo:hi], vis[lo:hi], *args, False)
        assert torch.equal(tape_p, tape[lo:hi])
        gx_p, go_p = torch.ops.dava.ba_sgd_backward_large(gout[lo:hi].contiguous(), tape_p, obs[lo:hi], vis[lo:hi],
                                                          *args, True)
        assert torch.equal(gx_p, gx[lo:hi]) and torch.equal(go_p, go[lo:hi])
    lib = N.load_library()
    sc, cfg = _ops.scene_struct(obs, vis, m, n, distortion, 5), _ops.sgd_config(LR_LARGE, k)
    need = lib.dava_ba_sgd_backward_large_workspace_bytes(sc, cfg, 1)
    runs = []
    for _ in range(2):
        ws = torch.full((need // 4 + 1,), float("nan"), device=device)
        outs = [torch.full_like(x0, float("nan")), torch.full_like(obs, float("nan"))]
        N.check(lib.dava_ba_sgd_backward_large(sc, cfg, N.ptr(tape), tape.numel() * 4, N.ptr(gout), N.ptr(outs[0]),
                                               N.ptr(outs[1]), N.ptr(ws), ws.numel() * 4, N.stream_of(device)),
                "dava_ba_sgd_backward_large")
        torch.cuda.synchronize(device)
        runs.append(outs)
    for s, t, r in zip(runs[0], runs[1], (gx, go)):
        assert torch.isfinite(s).all() and torch.equal(s, t) and torch.equal(s, r)


# ---- 6. dispatch: what raises without the keyword ----

def test_solver_at_c5_with_the_keyword_differentiates_through_the_fused_descent(device):
    from deep_attention_visual_odometry_amd import ReprojectionError, SGDSolver, native_ops

    name, k = "c5_16x4096", 2
    m, n, distortion, _ = _meta(name)
    x0, obs, vis = (t.to(device) for t in _scene(name, 2))
    obs.requires_grad_(True)
    fn = ReprojectionError(obs, vis, m, n, large_derivatives=True)
    solver = SGDSolver(LR_LARGE, k)
    xg = x0.clone().requires_grad_(True)
    out = solver(xg, fn)
    ref, errs = native_ops.ba_sgd_solve(x0, obs.detach(), vis, m, n, distortion, learning_rate=LR_LARGE, iterations=k,
                                        want_errors=True)
    assert out.requires_grad and torch.equal(out.detach(), ref)
    assert solver.last_errors is not None and torch.equal(solver.last_errors, errs)
    out.sum().backward()
    assert torch.isfinite(xg.grad).all() and torch.isfinite(obs.grad).all()
    rx, ro, _ = _gradient_distances(name, xg.grad.cpu(), obs.grad.cpu(), k, unit_w=True)
    print("C5-SOLVER x0", float(rx.max()), "obs", float(ro.max()))
    assert (rx <= 2e-3).all() and (ro <= 2e-3).all(), (rx, ro)
    # without the keyword: the torch loop, whose second derivative refuses the shape
    plain = SGDSolver(LR_LARGE, k)
    with pytest.raises(RuntimeError, match="dava_ba_second_order"):
        plain(x0.clone().requires_grad_(True), ReprojectionError(obs.detach(), vis, m, n))
    assert plain.last_errors is None


def test_objective_double_backward_at_a_large_scene_with_the_keyword(device):
    from deep_attention_visual_odometry_amd import ReprojectionError

    name = "pinhole_2x3600"
    m, n, distortion, _ = _meta(name)
    x, obs, vis = (t.to(device) for t in _scene(name, 2))
    v = _directions(name, 2)[0].to(device)
    xg = x.clone().requires_grad_(True)
    e = ReprojectionError(obs, vis, m, n, large_derivatives=True)(xg)
    (g,) = torch.autograd.grad(e.sum(), xg, create_graph=True)
    (hv,) = torch.autograd.grad((g * v).sum(), xg)
    want = _second(device, name, 2, True, v.cpu(), None, want_obs=False)
    assert torch.equal(g.detach().cpu(), want[1]) and torch.equal(hv.cpu(), want[2])
    assert torch.isfinite(hv).all() and hv.abs().max() > 0
    # without the keyword both stay refused
    xg = x.clone().requires_grad_(True)
    e = ReprojectionError(obs, vis, m, n)(xg)
    with pytest.raises(RuntimeError, match="dava_ba_second_order"):
        torch.autograd.grad(e.sum(), xg, create_graph=True)
    og = obs.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="dava_ba_second_order"):
        ReprojectionError(og, vis, m, n)(x)


def test_large_backward_is_once_differentiable(device, overrides):
    from deep_attention_visual_odometry_amd import native_ops

    name, k = "bc_3x70", 5
    m, n, distortion, _ = _meta(name)
    x0, obs, vis = (t.to(device) for t in _scene(name, B))
    overrides(KNOB, 1)
    xg = x0.clone().requires_grad_(True)
    out, _ = native_ops.ba_sgd_solve_differentiable_large(xg, obs, vis, m, n, distortion, learning_rate=1e-4,
                                                          iterations=k)
    (g,) = torch.autograd.grad(out.sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_new_operators_pass_opcheck(device, overrides):
    name = "pinhole_2x64"
    m, n, distortion, _ = _meta(name)
    x0, obs, vis = (t.to(device) for t in _scene(name, B))
    vis = vis.to(torch.uint8)
    v, u = (t.to(device) for t in _directions(name, B))
    for form in (1, 2):
        overrides(KNOB, form)
        torch.library.opcheck(torch.ops.dava.ba_second_order_large.default,
                              (x0, obs, vis, m, n, distortion, v, 0, True, True, u),
                              test_utils=("test_schema", "test_faketensor"))
        args = (x0, obs, vis, m, n, distortion, 1e-4, 4, 0, True)
        torch.library.opcheck(torch.ops.dava.ba_sgd_solve_differentiable_large.default, args,
                              test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
        _, _, tape = torch.ops.dava.ba_sgd_solve_differentiable_large(*args)
        torch.library.opcheck(torch.ops.dava.ba_sgd_backward_large.default,
                              (torch.randn_like(x0), tape, obs, vis, m, n, distortion, 1e-4, 4, 0, True),
                              test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError, match="tape"):
        torch.ops.dava.ba_sgd_backward_large(torch.randn_like(x0), tape[:, :3].contiguous(), obs, vis, m, n,
                                             distortion, 1e-4, 4, 0, True)
