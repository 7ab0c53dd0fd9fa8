"""The fused gradient descent on the GPU: dava_ba_sgd_solve / _record / _backward behind torch.ops.dava.ba_sgd_* and
SGDSolver, against the in-test oracle (sgd_oracle.py: the reference's loop in torch on the CPU, bitwise the
reference's SGDSolver in float32, tests/golden/sgd.npz).

lr = 1e-4 unless a test says otherwise: on the CPU oracle the descent already diverges at 1e-3 (E 0.43 -> 5e7 at
(2, 64), NaN with distortion); at 1e-4 it contracts on the squared objective and a 1-ulp nudge of x0 stays a 1-ulp
difference through K = 100.

Bars.  x_K and the error trace: per-row relative error <= 1e-5 against the float32 oracle (the project's TOL; the
float32 oracle itself sits <= 9.6e-7 from the float64 oracle at K = 100).  Gradients, against autograd through the
loop in float64, of x0.grad - w (the identity part of dx_K/dx0 must not mask the solve's part) and obs.grad, per
row: squared objective <= 2e-3; ray angle <= max(2e-2, 4 x the float32 oracle's own distance for that row) -- the
rule of test_gpu_solve_grad.py::test_fused_adjoint_matches_oracle.

Every parity case prints a PARITY line (the kernel's and the float32 oracle's distance to the float64 oracle) and
a run of the whole parity test rewrites profiles/sgd_parity.jsonl with its lines; DESIGN.md 3.9 quotes them.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import sgd_oracle
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

LR = 1e-4
TOL = 1e-5
B = 4
# name: (M, N, distortion, ray, drop, seed)
SHAPES = {
    "pinhole_2x64": (2, 64, False, False, 0.1, 9701),
    "ray_2x130": (2, 130, False, True, 0.1, 9702),
    "bc_3x70": (3, 70, True, False, 0.0, 9703),
    "bc_4x256": (4, 256, True, False, 0.0, 9704),
    "one_point_2x1": (2, 1, False, False, 0.0, 9705),  # P = 12: every lane but one idle
    "past_ppt_2x257": (2, 257, False, False, 0.1, 9706),  # just past a point per thread
}
PARITY_KS = {name: (1, 5, 20) + ((100,) if name in ("pinhole_2x64", "bc_4x256") else ()) for name in SHAPES}
SHAPES.update({"c2_2x128": (2, 128, False, False, 0.1, 9709), "ray_2x64": (2, 64, False, True, 0.1, 9710)})  # gradients


@functools.lru_cache(maxsize=None)
def _scene(name, batch=B):
    from deep_attention_visual_odometry_amd import make_scenes

    m, n, distortion, ray, drop, seed = SHAPES[name]
    s = make_scenes(batch, m, n, distortion=distortion, seed=seed, drop=drop, ray_angle=ray)
    return torch.tensor(s.initial), torch.tensor(s.observations), torch.tensor(s.visibility)


@functools.lru_cache(maxsize=None)
def _oracle(name, dtype, lr=LR):
    """{K: (x_K, E(x_k) (B, K))} of the CPU oracle for every K the parity test asks, from one descent."""
    m, n, distortion, ray, _, _ = SHAPES[name]
    x0, obs, vis = _scene(name)
    fn = sgd_oracle.closure(obs.to(dtype), vis, m, n, distortion, ray)
    out, x, errs, k_done = {}, x0.to(dtype), [], 0
    for k in sorted(PARITY_KS[name]):
        x, e = sgd_oracle.descend(x, fn, lr, k - k_done, trace=True)
        errs.append(e)
        k_done = k
        out[k] = (x, torch.cat(errs, dim=-1))
    return out


def _solve(device, x0, obs, vis, name, k, lr=LR, record=False):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray = SHAPES[name][:4]
    solve = native_ops.ba_sgd_solve_differentiable if record else native_ops.ba_sgd_solve
    x, errs = solve(x0.to(device), obs.to(device), vis.to(device), m, n, distortion, learning_rate=lr, iterations=k,
                    residual=1 if ray else 0, want_errors=True)
    torch.cuda.synchronize(device)
    return x.detach().cpu(), errs.cpu()


_PARITY_LINES = []


def _report(rec):
    """One PARITY line per case.  Once every case of the parity test has reported in this process,
    profiles/sgd_parity.jsonl is rewritten with the run's lines; a partial run (-k, one case) leaves it alone."""
    print("PARITY", json.dumps(rec))
    _PARITY_LINES.append(json.dumps(rec))
    if {(json.loads(line)["case"], json.loads(line)["K"]) for line in _PARITY_LINES} != {
            (name, k) for name in PARITY_KS for k in PARITY_KS[name]}:
        return
    try:
        with open(os.path.join(REPO, "profiles", "sgd_parity.jsonl"), "w") as fh:
            fh.write("\n".join(_PARITY_LINES) + "\n")
    except OSError:  # (a read-only checkout: the printed lines remain)
        pass


# ---- 1. parity of x_K and of the error trace ----

@pytest.mark.parametrize("name,k", [(name, k) for name in PARITY_KS for k in PARITY_KS[name]])
def test_parity_with_the_float32_oracle(device, name, k):
    x0, obs, vis = _scene(name)
    x, errs = _solve(device, x0, obs, vis, name, k)
    ref, ref_errs = _oracle(name, torch.float32)[k]
    ref64, _ = _oracle(name, torch.float64)[k]
    rel, rel_e = sgd_oracle.rows_rel(x, ref), sgd_oracle.rows_rel(errs, ref_errs)
    _report({"case": name, "K": k, "max_rel_x": float(rel.max()), "max_rel_trace": float(rel_e.max()),
             "kernel_to_f64": float(sgd_oracle.rows_rel(x, ref64).max()),
             "oracle32_to_f64": float(sgd_oracle.rows_rel(ref, ref64).max())})
    assert errs.shape == (B, k)
    assert rel.max() <= TOL, rel
    assert rel_e.max() <= TOL, rel_e


# ---- 2. the reference's golden ----

@pytest.mark.parametrize("case", ["pinhole", "ray", "bc"])
@pytest.mark.parametrize("k", [1, 5, 20])
def test_reference_golden(device, case, k):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray = {"pinhole": (2, 64, False, False), "ray": (2, 64, False, True),
                             "bc": (3, 70, True, False)}[case]
    g = np.load(os.path.join(GOLDEN, "sgd.npz"))
    x0, obs, vis = (torch.tensor(g[case + s]).to(device) for s in ("_x0", "_obs", "_vis"))
    x, _ = native_ops.ba_sgd_solve(x0, obs, vis, m, n, distortion, learning_rate=LR, iterations=k,
                                   residual=1 if ray else 0)
    rel = sgd_oracle.rows_rel(x.cpu(), torch.tensor(g[f"{case}_k{k}"]))
    print("GOLDEN", case, k, float(rel.max()))
    assert rel.max() <= TOL, rel


# ---- 3. the large form ----

def test_large_form_under_the_override(device, overrides):
    """(3, 70) in the LDS form and, under FORCE_GV, in the large form (scene read in place, packed pair sweep,
    eight waves): both inside the bar, and within 1e-6 of each other."""
    name, k = "bc_3x70", 20
    x0, obs, vis = _scene(name)
    x_lds, e_lds = _solve(device, x0, obs, vis, name, k)
    overrides("FORCE_GV", 1)
    x_gv, e_gv = _solve(device, x0, obs, vis, name, k)
    overrides("FORCE_GV", -1)
    ref, ref_errs = _oracle(name, torch.float32)[k]
    for x, e in ((x_lds, e_lds), (x_gv, e_gv)):
        assert sgd_oracle.rows_rel(x, ref).max() <= TOL and sgd_oracle.rows_rel(e, ref_errs).max() <= TOL
    rel = sgd_oracle.rows_rel(x_gv, x_lds)
    print("LARGE-vs-LDS", float(rel.max()))
    assert rel.max() <= 1e-6, rel


def test_large_form_at_c5(device):
    """One genuine C5 shape (16 views x 4096 points, P = 12381: x and the gradient fill 99 KB of LDS), B = 2, K = 3.

    At this shape lr = 1e-4 does not contract: E grows 50-150x per step on every scene tried (seed 9709: 12.5 ->
    659 -> 1.07e5), and on some the reference's own loop is chaotic within three steps (seeds 9707 / 9708: a 1-ulp
    nudge of x0 moves the float32 oracle's x_3 by 0.25 / 0.05 relative).  A bar of 1e-5 decides nothing there, so
    the scene is chosen -- from the oracle alone -- as one whose x_3 moves <= 1e-6 under a +-1-ulp nudge of x0
    (asserted below; seed 9709: 2.1e-7).  x_3 and the error trace are held to the 1e-5 bar (the oracle's trace itself
    moves 1.2e-5 under that nudge: E(x_2) ~ 1e5 follows x_2's last bits; printed, not part of the bar)."""
    from deep_attention_visual_odometry_amd import make_scenes, native_ops

    m, n, k = 16, 4096, 3
    s = make_scenes(2, m, n, seed=9709)
    x0, obs, vis = torch.tensor(s.initial), torch.tensor(s.observations), torch.tensor(s.visibility)
    x, errs = native_ops.ba_sgd_solve(x0.to(device), obs.to(device), vis.to(device), m, n, False, learning_rate=LR,
                                      iterations=k, want_errors=True)
    fn = sgd_oracle.closure(obs, vis, m, n)
    ref, ref_errs = sgd_oracle.descend(x0, fn, LR, k, trace=True)
    own_x, own_e = torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    for toward in (float("inf"), -float("inf")):
        xn, en = sgd_oracle.descend(torch.nextafter(x0, torch.full_like(x0, toward)), fn, LR, k, trace=True)
        own_x = torch.maximum(own_x, sgd_oracle.rows_rel(xn, ref))
        own_e = torch.maximum(own_e, sgd_oracle.rows_rel(en, ref_errs))
    assert own_x.max() <= 1e-6, own_x  # the scene's precondition: the reference itself is stable here
    rel, rel_e = sgd_oracle.rows_rel(x.cpu(), ref), sgd_oracle.rows_rel(errs.cpu(), ref_errs)
    print("C5 x", float(rel.max()), "trace", float(rel_e.max()), "oracle's own 1-ulp sensitivity", float(own_x.max()),
          float(own_e.max()))
    assert rel.max() <= TOL, rel
    assert rel_e.max() <= TOL, rel_e


# ---- 4. state carried across steps ----

def test_one_launch_is_two_launches(device, overrides):
    """K = 12 in one launch is bitwise K = 5 followed by K = 7 from its output (an accumulator that is not
    re-zeroed, or a stale scratch buffer, would show): the LDS form with and without a point per thread, and,
    under FORCE_GV, the large form on both residuals."""
    for name, large in (("bc_4x256", False), ("past_ppt_2x257", False), ("ray_2x130", False), ("bc_3x70", True),
                        ("past_ppt_2x257", True), ("ray_2x130", True)):
        overrides("FORCE_GV", 1 if large else -1)
        x0, obs, vis = _scene(name)
        x12, e12 = _solve(device, x0, obs, vis, name, 12)
        x5, e5 = _solve(device, x0, obs, vis, name, 5)
        x7, e7 = _solve(device, x5, obs, vis, name, 7)
        assert torch.equal(x12, x7), (name, large)
        assert torch.equal(e12, torch.cat([e5, e7], dim=-1)), (name, large)


def test_recording_launch_is_bitwise_the_plain_launch(device, overrides):
    for name in ("pinhole_2x64", "bc_4x256", "past_ppt_2x257", "ray_2x130", "one_point_2x1"):
        x0, obs, vis = _scene(name)
        x, e = _solve(device, x0, obs, vis, name, 9)
        xr, er = _solve(device, x0, obs, vis, name, 9, record=True)
        assert torch.equal(x, xr) and torch.equal(e, er), name


def test_tape_holds_every_iterate(device):
    """The tape's row k is x_k: row 0 is x0, and row k of a K-step recording is the output of a k-step solve."""
    name, k = "bc_3x70", 6
    m, n, distortion, ray = SHAPES[name][:4]
    x0, obs, vis = (t.to(device) for t in _scene(name))
    _, _, tape = torch.ops.dava.ba_sgd_solve_differentiable(x0, obs, vis.to(torch.uint8), m, n, distortion, LR, k, 0,
                                                             False)
    p = x0.shape[1]
    assert tape.shape == (B, k, (p + 3) // 4 * 4)
    assert torch.equal(tape[:, 0, :p], x0) and (tape[:, :, p:] == 0).all()
    x3, _ = _solve(device, x0, obs, vis, name, 3)
    assert torch.equal(tape[:, 3, :p].cpu(), x3)


def test_zero_iterations_returns_x0(device):
    name = "bc_3x70"
    x0, obs, vis = _scene(name)
    for record in (False, True):
        x, e = _solve(device, x0, obs, vis, name, 0, record=record)
        assert torch.equal(x, x0) and e.shape == (B, 0)


def test_more_problems_than_resident_workgroups(device):
    """One launch of B = 600 (more workgroups than are resident at once) against the same problems in launches of
    200: bitwise the same rows."""
    from deep_attention_visual_odometry_amd import make_scenes, native_ops

    m, n, k = 2, 64, 8
    s = make_scenes(600, m, n, seed=9708, drop=0.1)
    x0, obs, vis = (torch.tensor(t).to(device) for t in (s.initial, s.observations, s.visibility))
    kw = dict(learning_rate=LR, iterations=k, want_errors=True)
    x, e = native_ops.ba_sgd_solve(x0, obs, vis, m, n, False, **kw)
    for lo in range(0, 600, 200):
        xs, es = native_ops.ba_sgd_solve(x0[lo:lo + 200], obs[lo:lo + 200], vis[lo:lo + 200], m, n, False, **kw)
        assert torch.equal(xs, x[lo:lo + 200]) and torch.equal(es, e[lo:lo + 200])


# ---- 5. gradients ----

GRADIENT_CASES = [("pinhole_2x64", 10), ("c2_2x128", 20), ("bc_4x256", 8), ("bc_3x70", 12), ("one_point_2x1", 6),
                  ("ray_2x64", 10)]


def _fused_gradients(device, x0, obs, vis, name, k, w, obs_grad=True):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray = SHAPES[name][:4]
    xg = x0.to(device).requires_grad_(True)
    og = obs.to(device).requires_grad_(obs_grad)
    out, _ = native_ops.ba_sgd_solve_differentiable(xg, og, vis.to(device), m, n, distortion, learning_rate=LR,
                                                    iterations=k, residual=1 if ray else 0)
    (out * w.to(device)).sum().backward()
    return out.detach().cpu(), xg.grad.cpu(), (og.grad.cpu() if obs_grad else None)


@pytest.mark.parametrize("name,k", GRADIENT_CASES)
def test_gradients_match_float64_autograd(device, name, k):
    m, n, distortion, ray = SHAPES[name][:4]
    x0, obs, vis = _scene(name)
    w = torch.randn(x0.shape, generator=torch.Generator().manual_seed(k))
    out, gx, go = _fused_gradients(device, x0, obs, vis, name, k, w)
    ref, gx64, go64 = sgd_oracle.gradients(x0, obs, vis, m, n, distortion, ray, w, LR, k, torch.float64)
    w64 = w.double()
    rx, ro = sgd_oracle.rows_rel(gx.double() - w64, gx64 - w64), sgd_oracle.rows_rel(go, go64)
    part = ((gx64 - w64).norm(dim=-1) / w64.norm(dim=-1))  # the solve's share of dx_K/dx0
    tol_x = tol_o = torch.full_like(rx, 2e-3)
    if ray:  # the rule and the factors of test_fused_adjoint_matches_oracle
        _, gx32, go32 = sgd_oracle.gradients(x0, obs, vis, m, n, distortion, ray, w, LR, k, torch.float32)
        tol_x = torch.maximum(torch.full_like(rx, 2e-2), 4.0 * sgd_oracle.rows_rel(gx32.double() - w64, gx64 - w64))
        tol_o = torch.maximum(torch.full_like(ro, 2e-2), 4.0 * sgd_oracle.rows_rel(go32, go64))
    print("GRADIENT", name, k, "x0", float(rx.max()), "obs", float(ro.max()), "tol", float(tol_x.max()),
          float(tol_o.max()), "solve's part of w", float(part.min()), float(part.max()))
    assert sgd_oracle.rows_rel(out, ref).max() <= TOL
    assert (rx <= tol_x).all(), (rx, tol_x)
    assert (ro <= tol_o).all(), (ro, tol_o)
    # observations that do not require grad: the backward runs with a NULL observations_grad, x0.grad bitwise
    _, gx_only, none = _fused_gradients(device, x0, obs, vis, name, k, w, obs_grad=False)
    assert none is None and torch.equal(gx_only, gx)


def test_backward_is_deterministic_and_once_differentiable(device):
    name, k = "bc_3x70", 5
    x0, obs, vis = _scene(name)
    w = torch.randn(x0.shape, generator=torch.Generator().manual_seed(1))
    _, gx, go = _fused_gradients(device, x0, obs, vis, name, k, w)
    _, gx2, go2 = _fused_gradients(device, x0, obs, vis, name, k, w)
    assert torch.equal(gx, gx2) and torch.equal(go, go2)
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, _ = SHAPES[name][:4]
    xg = x0.to(device).requires_grad_(True)
    out, _ = native_ops.ba_sgd_solve_differentiable(xg, obs.to(device), vis.to(device), m, n, distortion,
                                                    learning_rate=LR, iterations=k)
    (g,) = torch.autograd.grad(out.sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---- 6. dispatch ----

def _objective(device, name, dtype=torch.float32, **kw):
    from deep_attention_visual_odometry_amd import RayAngleError, ReprojectionError

    m, n, distortion, ray = SHAPES[name][:4]
    x0, obs, vis = _scene(name)
    obs, vis = obs.to(device=device, dtype=dtype), vis.to(device)
    fn = RayAngleError(obs, vis, m, n, **kw) if ray else ReprojectionError(obs, vis, m, n, distortion, **kw)
    return x0.to(device=device, dtype=dtype), fn


@pytest.mark.parametrize("name", ["bc_3x70", "ray_2x130"])
def test_solver_takes_the_fused_solve(device, name):
    from deep_attention_visual_odometry_amd import SGDSolver, native_ops

    m, n, distortion, ray = SHAPES[name][:4]
    x0, fn = _objective(device, name)
    solver = SGDSolver(learning_rate=LR, iterations=7)
    out = solver(x0, fn)
    ref, errs = native_ops.ba_sgd_solve(x0, fn.observations, fn.visibility, m, n, distortion, learning_rate=LR,
                                        iterations=7, residual=fn.residual, want_errors=True)
    assert not out.requires_grad and torch.equal(out, ref)
    assert solver.last_errors.shape == (B, 7) and torch.equal(solver.last_errors, errs)
    # with a graph: the recording solve and the adjoint, the same values, gradients to x0 and the observations
    xg = x0.clone().requires_grad_(True)
    fn.observations.requires_grad_(True)
    out = solver(xg, fn)
    assert out.requires_grad and torch.equal(out.detach(), ref) and torch.equal(solver.last_errors, errs)
    out.sum().backward()
    assert xg.grad is not None and fn.observations.grad is not None
    assert torch.isfinite(xg.grad).all() and torch.isfinite(fn.observations.grad).all()


def test_solver_runs_a_plain_closure_in_torch(device):
    from deep_attention_visual_odometry_amd import SGDSolver

    name = "bc_3x70"
    m, n, distortion, ray = SHAPES[name][:4]
    x0, obs, vis = (t.to(device) for t in _scene(name))
    fn = sgd_oracle.closure(obs, vis, m, n, distortion, ray)
    solver = SGDSolver(LR, 5)
    out = solver(x0, fn)
    assert solver.last_errors is None and out.device == x0.device and not x0.requires_grad
    assert torch.equal(out, sgd_oracle.descend(x0, fn, LR, 5))
    assert sgd_oracle.rows_rel(out.cpu(), _oracle(name, torch.float32)[5][0]).max() <= TOL


def test_solver_float64_runs_the_loop_on_the_float64_kernels(device):
    from deep_attention_visual_odometry_amd import SGDSolver

    name = "bc_3x70"
    x0, fn = _objective(device, name, torch.float64)
    solver = SGDSolver(LR, 5)
    out = solver(x0, fn)
    assert out.dtype == torch.float64 and solver.last_errors is None
    rel = sgd_oracle.rows_rel(out.cpu(), _oracle(name, torch.float64)[5][0])
    print("F64-LOOP", float(rel.max()))
    assert rel.max() <= 1e-9, rel


def test_solver_at_c5_with_a_graph_does_not_launch_the_adjoint(device):
    """C5's dual image is past 160 KiB: no fused adjoint, so the call takes the torch loop, where the objective is
    an ordinary closure -- and its own second derivative (dava_ba_second_order) refuses the shape: RuntimeError.
    Without a graph the same objective takes the fused solve."""
    from deep_attention_visual_odometry_amd import ReprojectionError, SGDSolver, make_scenes, native_ops

    m, n = 16, 4096
    assert not native_ops.sgd_backward_supported(2, m, n, False, 2)
    s = make_scenes(2, m, n, seed=9707)
    x0, obs, vis = (torch.tensor(t).to(device) for t in (s.initial, s.observations, s.visibility))
    fn = ReprojectionError(obs, vis, m, n)
    solver = SGDSolver(LR, 2)
    with pytest.raises(RuntimeError, match="dava_ba_second_order"):
        solver(x0.clone().requires_grad_(True), fn)
    assert solver.last_errors is None
    out = solver(x0, fn)
    assert solver.last_errors is not None and out.shape == x0.shape


def test_fused_forward_compiles_fullgraph_as_one_node(device):
    from deep_attention_visual_odometry_amd import SGDSolver

    x0, fn = _objective(device, "pinhole_2x64")
    solver = SGDSolver(LR, 9)
    eager = solver(x0, fn)
    graphs = []

    def backend(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    torch._dynamo.reset()
    out = torch.compile(solver, fullgraph=True, backend=backend)(x0, fn)
    assert torch.equal(out, eager)
    assert len(graphs) == 1
    calls = [nd for nd in graphs[0].graph.nodes if nd.op == "call_function" and "dava" in str(nd.target)]
    # (the one operator of the graph; dynamo names it by its packet or by its overload)
    assert [str(nd.target).removesuffix(".default") for nd in calls] == ["dava.ba_sgd_solve"]
    torch._dynamo.reset()
    assert torch.equal(torch.compile(solver, fullgraph=True)(x0, fn), eager)  # (the default backend)
    assert solver.last_errors is not None and solver.last_errors.shape == (B, 9)


def test_operators_pass_opcheck(device):
    name = "bc_3x70"
    m, n, distortion, _ = SHAPES[name][:4]
    x0, obs, vis = (t.to(device) for t in _scene(name))
    vis = vis.to(torch.uint8)
    args = (x0, obs, vis, m, n, distortion, LR, 4, 0, True)
    torch.library.opcheck(torch.ops.dava.ba_sgd_solve.default, args, test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.dava.ba_sgd_solve_differentiable.default, args,
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
    _, _, tape = torch.ops.dava.ba_sgd_solve_differentiable(*args)
    torch.library.opcheck(torch.ops.dava.ba_sgd_backward.default,
                          (torch.randn_like(x0), tape, obs, vis, m, n, distortion, LR, 4, 0, True),
                          test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError, match="tape"):
        torch.ops.dava.ba_sgd_backward(torch.randn_like(x0), tape[:, :3].contiguous(), obs, vis, m, n, distortion,
                                       LR, 4, 0, True)


# ---- 7. overflow ----

def test_overflow_is_not_special(device):
    """lr = 1e-2 at (2, 64), on make_scenes(4, 2, 64, drop=0.1) with the generator's default seed: the oracle's
    rows overflow (row 1: E = 2.8e15 at K = 5) and three of the four are NaN by K = 20.  Every row that is NaN in
    the oracle is non-finite from the kernel, and the launch returns."""
    from deep_attention_visual_odometry_amd import make_scenes, native_ops

    m, n, k = 2, 64, 20
    s = make_scenes(4, m, n, drop=0.1)
    x0, obs, vis = torch.tensor(s.initial), torch.tensor(s.observations), torch.tensor(s.visibility)
    ref = sgd_oracle.descend(x0, sgd_oracle.closure(obs, vis, m, n), 1e-2, k)
    bad = ~torch.isfinite(ref).all(dim=-1)
    assert bad.sum() >= 2
    x, errs = native_ops.ba_sgd_solve(x0.to(device), obs.to(device), vis.to(device), m, n, False, learning_rate=1e-2,
                                      iterations=k, want_errors=True)
    torch.cuda.synchronize(device)
    finite = torch.isfinite(x.cpu()).all(dim=-1)
    print("OVERFLOW oracle non-finite rows", bad.tolist(), "kernel finite rows", finite.tolist())
    assert (~finite[bad]).all(), (bad, finite)
    # and the device still answers: the next launch is an ordinary one
    name = "pinhole_2x64"
    x_ok, _ = _solve(device, *_scene(name), name, 5)
    assert sgd_oracle.rows_rel(x_ok, _oracle(name, torch.float32)[5][0]).max() <= TOL
