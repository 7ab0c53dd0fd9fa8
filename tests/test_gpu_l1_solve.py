"""The legacy solver fused into one launch (BFGSCameraSolver(fused=True), csrc/camera_l1_solve.hip) on the GPU:
against the REAL reference after every iteration count (tests/golden/l1_solve.npz, cases A-F, and the existing
camera_l1.npz solve), against the unchanged loop (fused=False) on the same tensors, its exits and traces, the two
forms bitwise, float32, and the routing of fused=True.

Every displacement / float32 case prints a PARITY line; with DAVA_WRITE_PROFILES=1 set, once all have reported in
one process, profiles/l1_solve_parity.jsonl is rewritten with the run's lines (a partial run, or a run without the
variable, leaves the committed file alone).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

PARAMS = ("focal_length", "cx", "cy", "translation", "lie", "world")
SETTING_FIELDS = ("views", "points", "iterations", "epsilon", "max_step_distance", "min_step_distance",
                  "max_step_size", "zoom_iterations", "sufficient_decrease", "curvature")
CASES = ("A", "B", "C", "D", "E", "F")


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN, "l1_solve.npz"))


def _settings(case):
    return dict(zip(SETTING_FIELDS, _golden()[f"{case}_settings"].tolist()))


def _tensors(case, dtype=torch.float64):
    g = _golden()
    t = {k: torch.tensor(g[f"{case}_{k}"], dtype=dtype) for k in PARAMS}
    t["true"] = torch.tensor(g[f"{case}_true"], dtype=dtype)
    t["vis"] = torch.tensor(g[f"{case}_vis"])
    return t


def _model(device, t, **kw):
    from deep_attention_visual_odometry_amd.camera_model import PinholeCameraModelL1
    from deep_attention_visual_odometry_amd.geometry import LieRotation

    d = {k: v.to(device) for k, v in t.items()}
    kw = dict(dict(max_gradient=1e3, constrain=True), **kw)
    return PinholeCameraModelL1(focal_length=d["focal_length"], cx=d["cx"], cy=d["cy"], translation=d["translation"],
                                orientation=LieRotation(d["lie"]), world_points=d["world"],
                                true_projected_points=d["true"], visibility_mask=d["vis"], **kw)


def _solver(s, iterations, fused, line_search_type=None, **kw):
    from deep_attention_visual_odometry_amd.solvers import BFGSCameraSolver, LineSearchStrongWolfeConditions

    ls = (line_search_type or LineSearchStrongWolfeConditions)(
        max_step_size=s["max_step_size"], zoom_iterations=int(s["zoom_iterations"]),
        sufficient_decrease=s["sufficient_decrease"], curvature=s["curvature"])
    return BFGSCameraSolver(max_iterations=int(iterations), epsilon=s["epsilon"],
                            max_step_distance=s["max_step_distance"], min_step_distance=s["min_step_distance"],
                            line_search=ls, fused=fused, **kw)


def _parts(model):
    return dict(focal_length=model.focal_length, cx=model.cx, cy=model.cy, translation=model._translation,
                lie=model._orientation.lie_vector, world=model._world_points)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-30)).item()


def _rows(parts):
    """(B E, everything): one row per problem."""
    n = parts["focal_length"].numel()
    return torch.cat([parts[k].double().cpu().reshape(n, -1) for k in PARAMS], dim=-1)


def _run(device, case, iterations, fused, dtype=torch.float64):
    solver = _solver(_settings(case), iterations, fused)
    with torch.no_grad():
        out = solver(_model(device, _tensors(case, dtype)))
    return solver, out


_PARITY_LINES = []
_PARITY_KEYS = {("displacement", c) for c in CASES} | {("float32", "A")}


def _report(rec):
    print("PARITY", json.dumps(rec))
    _PARITY_LINES.append(json.dumps(rec))
    if os.environ.get("DAVA_WRITE_PROFILES") != "1":  # an ordinary suite run leaves the committed file alone
        return
    if {(json.loads(line)["test"], json.loads(line)["case"]) for line in _PARITY_LINES} != _PARITY_KEYS:
        return
    try:
        with open(os.path.join(REPO, "profiles", "l1_solve_parity.jsonl"), "w") as fh:
            fh.write("\n".join(_PARITY_LINES) + "\n")
    except OSError:  # (a read-only checkout: the printed lines remain)
        pass


# ---- 1. the reference after every iteration count ----

@pytest.mark.parametrize("case", CASES)
def test_fixture_cases_match_reference_at_every_iteration_count(device, case):
    g = _golden()
    k_max = int(_settings(case)["iterations"])
    for k in range(1, k_max + 1):
        solver, out = _run(device, case, k, True)
        assert solver.last_trace_exit is not None, "the fused kernel did not run"
        for key, got in _parts(out).items():
            rel = _rel(got, torch.tensor(g[f"{case}_out_{key}"][k - 1]))
            assert rel < 1e-6, (case, k, key, rel)
        assert _rel(out.get_error(), torch.tensor(g[f"{case}_out_error"][k - 1])) < 1e-6, (case, k)


def test_configurations_solve_matches_reference(device):
    """The existing camera_l1.npz solve (K = 10, the configurations' settings) with the assertions of
    test_legacy_bfgs_camera_solver_matches_reference, on the fused path."""
    g = np.load(os.path.join(GOLDEN, "camera_l1.npz"))
    t = {k: torch.tensor(g[f"solve_{k}"]) for k in PARAMS + ("true", "vis")}
    model = _model(device, t)
    solver = _solver(dict(epsilon=1e-6, max_step_distance=1e3, min_step_distance=1e-3, max_step_size=1e5,
                          zoom_iterations=20, sufficient_decrease=1e-4, curvature=0.9), 10, True)
    with torch.no_grad():
        assert _rel(model.get_error(), torch.tensor(g["solve_in_error"])) < 1e-12
        out = solver(model)
        assert solver.last_trace_exit is not None
        assert _rel(out.get_error(), torch.tensor(g["solve_out_error"])) < 1e-6
    assert _rel(out.focal_length, torch.tensor(g["solve_out_focal_length"])) < 1e-6
    assert _rel(out._translation, torch.tensor(g["solve_out_translation"])) < 1e-6
    assert _rel(out._orientation.lie_vector, torch.tensor(g["solve_out_lie"])) < 1e-6
    assert _rel(out._world_points, torch.tensor(g["solve_out_world"])) < 1e-6
    assert (out.get_error().cpu() < torch.tensor(g["solve_in_error"])).all()


# ---- 2. displacement error next to the loop's ----

@pytest.mark.parametrize("case", CASES)
def test_displacement_error_is_the_loops(device, case):
    """|x - x_ref| / |x_ref - x_0| per problem, for the loop (fused=False) and the fused path in the same run: both
    differ from the reference only in reduction order (its own one-ulp spread is ~1e-16), so the fused value may be at
    most 10 x the loop's, floored at 1e-12 (the float64 evaluation bar of test_gpu_camera_l1.py)."""
    g = _golden()
    k = int(_settings(case)["iterations"])
    x0 = _rows(_tensors(case))
    ref = _rows({key: torch.tensor(g[f"{case}_final_{key}"]) for key in PARAMS})
    moved = (ref - x0).norm(dim=-1)
    assert (moved > 0).all()
    _, loop = _run(device, case, k, False)
    solver, fused = _run(device, case, k, True)
    assert solver.last_trace_exit is not None
    e_loop = (_rows(_parts(loop)) - ref).norm(dim=-1) / moved
    e_fused = (_rows(_parts(fused)) - ref).norm(dim=-1) / moved
    _report({"test": "displacement", "case": case, "K": k, "loop": e_loop.tolist(), "fused": e_fused.tolist()})
    bound = torch.clamp(10.0 * e_loop, min=1e-12)
    assert (e_fused <= bound).all(), (case, e_fused.tolist(), e_loop.tolist())


# ---- 3. exits, traces, frozen estimates ----

def _exits(device, case):
    solver, out = _run(device, case, int(_settings(case)["iterations"]), True)
    return solver, out, solver.last_trace_exit[:, 0].cpu(), solver.last_trace_alpha[:, 0].cpu()


@pytest.mark.parametrize("case", CASES)
def test_trace_alpha_matches_reference(device, case):
    g = _golden()
    solver, _, exits, alpha = _exits(device, case)
    want = torch.tensor(g[f"{case}_alpha"]).T  # (B, K)
    assert exits.shape == want.shape and exits.dtype == torch.int32
    live = exits != 0
    assert ((alpha - want).abs()[live] <= 1e-6 * want.abs()[live]).all(), (alpha, want)
    accepted = torch.tensor(g[f"{case}_wolfe"]).T
    assert (accepted | ~((exits == 1) | (exits == 2)))[live].all()  # accepted returns satisfy the strong Wolfe pair
    assert (alpha[~live] == 0).all()
    assert _rel(solver.last_trace_error[:, 0, -1], torch.tensor(g[f"{case}_out_error"][-1, :, 0])) < 1e-6


def test_every_exit_is_taken(device):
    _, _, a, _ = _exits(device, "A")
    assert (a == 1).any() and (a == 2).any()
    _, _, c, _ = _exits(device, "C")
    assert (c == 4).any()
    _, out_d, d, alpha_d = _exits(device, "D")
    assert (d == 3).any()
    _, _, e, _ = _exits(device, "E")
    assert (e == 0).any()
    # D, first iteration, a problem that is still widening after its one trial: the step handed on is 2 d while
    # the returned model is the trial at alpha 1
    _, first = _run(device, "D", 1, True)
    s = _settings("D")
    from deep_attention_visual_odometry_amd.solvers.bfgs_camera_solver import clamp_search_direction

    with torch.no_grad():
        base = _model(device, _tensors("D"))
        direction = clamp_search_direction(-1.0 * base.get_gradient(), s["max_step_distance"], s["min_step_distance"])
        at_one = base.add(direction)
    rows = torch.nonzero(d[:, 0] == 3)[:, 0]
    assert len(rows) > 0 and (alpha_d[rows, 0] == 2.0).all()
    for key, got in _parts(first).items():
        assert _rel(got[rows], _parts(at_one)[key][rows]) < 1e-12, key


def test_frozen_estimates_keep_their_point(device):
    """E (epsilon = 0.03): an estimate whose error is no longer above epsilon after iteration j is frozen -- its
    output at K is bitwise its output at j + 1 iterations, and last_iterations says j + 1."""
    solver, out, exits, _ = _exits(device, "E")
    k = exits.shape[1]
    iterations = solver.last_iterations[:, 0].cpu()
    errors = solver.last_trace_error[:, 0].cpu()
    assert (iterations == (exits != 0).sum(dim=-1)).all()
    frozen_early = torch.nonzero(iterations < k)[:, 0].tolist()
    assert frozen_early and len({int(iterations[b]) for b in range(len(iterations))}) > 1  # at different iterations
    for b in range(len(iterations)):
        j = int(iterations[b])
        assert (errors[b, : j - 1] > 0.03).all()
        if j < k:
            assert errors[b, j - 1] <= 0.03 and (errors[b, j:] == errors[b, j - 1]).all()
    for j in sorted({int(iterations[b]) for b in frozen_early}):
        _, early = _run(device, "E", j, True)
        rows = torch.nonzero(iterations == j)[:, 0]
        for key, got in _parts(out).items():
            assert torch.equal(got[rows], _parts(early)[key][rows]), (j, key)
        assert torch.equal(out.get_error()[rows], early.get_error()[rows])


# ---- 4. the loop on the same tensors: estimates, visibility masks, constrain both ways, form 1 ----

def _random_tensors(m, n, b, e, seed, dtype=torch.float64):
    """A truth per batch item, E perturbed starts each, targets projected from the truth."""
    from deep_attention_visual_odometry_amd.geometry import LieRotation

    rng = np.random.default_rng(seed)
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    truth = dict(focal_length=t(rng.uniform(0.6, 1.8, size=(b, 1))), cx=t(rng.normal(0.0, 0.1, size=(b, 1))),
                 cy=t(rng.normal(0.0, 0.1, size=(b, 1))),
                 translation=t(rng.normal(0.0, 0.5, size=(b, 1, m, 3)) + np.array([0.0, 0.0, 8.0])),
                 lie=t(rng.normal(0.0, 0.2, size=(b, 1, m, 1, 3))), world=t(rng.normal(0.0, 1.0, size=(b, 1, n - 2, 3))))
    out = {k: (v.expand(b, e, *v.shape[2:]) + t(rng.normal(0.0, 0.02, size=(b, e) + tuple(v.shape[2:])))).to(dtype)
           for k, v in truth.items()}
    vis = torch.tensor(rng.random((b, m, n)) > 0.15)
    # the projection of the truth: the reference's expressions (test_gpu_camera_l1.py pins them), on the host
    pts = torch.cat([torch.zeros(b, 2, 3, dtype=torch.float64), truth["world"][:, 0]], dim=1)
    pts[:, 1, 0] = 1.0
    pts[:, 2, 2] = 0.0
    rel = LieRotation(truth["lie"][:, 0]).rotate_vector(pts[:, None]) + truth["translation"][:, 0, :, None, :]
    f, cx, cy = (truth[k][:, 0].reshape(b, 1, 1) for k in ("focal_length", "cx", "cy"))
    out["true"] = torch.stack([f * rel[..., 0] / rel[..., 2] + cx, f * rel[..., 1] / rel[..., 2] + cy],
                              dim=-1).to(dtype)
    out["vis"] = vis
    return out


@pytest.mark.parametrize("m,n,k,constrain", [(4, 8, 4, True), (4, 8, 4, False), (6, 70, 3, True)])
def test_fused_matches_the_loop_on_the_same_tensors(device, m, n, k, constrain):
    """B = 3, E = 2 with per-batch visibility masks; 6 x 70 is form 1 with more than 64 points per lane loop."""
    from deep_attention_visual_odometry_amd import native_ops

    assert native_ops.l1_solve_form(m, n) == (1 if n == 70 else 0)
    t = _random_tensors(m, n, 3, 2, seed=100 * m + n)
    s = dict(epsilon=1e-6, max_step_distance=1e3, min_step_distance=1e-3, max_step_size=1e5, zoom_iterations=20,
             sufficient_decrease=1e-4, curvature=0.9)
    with torch.no_grad():
        loop = _solver(s, k, False)(_model(device, t, constrain=constrain))
        solver = _solver(s, k, True)
        fused = solver(_model(device, t, constrain=constrain))
        assert solver.last_trace_exit is not None and solver.last_trace_exit.shape == (3, 2, k)
        for key, got in _parts(fused).items():
            assert got.shape == _parts(loop)[key].shape
            assert _rel(got, _parts(loop)[key]) < 1e-6, key
        cached = fused.get_error()
        fresh = _model(device, dict({key: v.clone() for key, v in _parts(fused).items()}, true=t["true"],
                                    vis=t["vis"]), constrain=constrain).get_error()
        assert torch.equal(cached, fresh)
        assert _rel(cached, loop.get_error()) < 1e-6


# ---- 5. the two forms ----

def test_forms_are_bitwise_equal(device):
    from deep_attention_visual_odometry_amd import _native, native_ops

    t = _random_tensors(4, 8, 3, 2, seed=408)
    s = dict(epsilon=1e-6, max_step_distance=1e3, min_step_distance=1e-3, max_step_size=1e5, zoom_iterations=20,
             sufficient_decrease=1e-4, curvature=0.9)

    def run():
        solver = _solver(s, 5, True)
        with torch.no_grad():
            out = solver(_model(device, t))
        return (list(_parts(out).values()) + [out.get_error(), solver.last_iterations, solver.last_trace_error,
                                              solver.last_trace_alpha, solver.last_trace_exit])

    assert native_ops.l1_solve_form(4, 8) == 0
    lds = run()
    try:
        _native.set_debug_override("L1_SOLVE_FORM", 1)
        assert native_ops.l1_solve_form(4, 8) == 1
        workspace = run()
    finally:
        _native.set_debug_override("L1_SOLVE_FORM", -1)
    for a, b in zip(lds, workspace):
        assert torch.equal(a, b)
    for a, b in zip(lds, run()):  # and run to run
        assert torch.equal(a, b)


# ---- 6. float32 ----

def test_float32_error_is_the_loops(device):
    """Case A's scene cast down: the fused float32 result against the float64 reference is at most 10 x the float32
    loop's, floored at 2e-6 (the float32 evaluation bar of test_gpu_camera_l1.py); the error falls everywhere."""
    g = _golden()
    k = int(_settings("A")["iterations"])
    ref = _rows({key: torch.tensor(g[f"A_final_{key}"]) for key in PARAMS})
    _, loop = _run(device, "A", k, False, torch.float32)
    solver, fused = _run(device, "A", k, True, torch.float32)
    assert solver.last_trace_exit is not None and fused.focal_length.dtype == torch.float32
    assert solver.last_trace_error.dtype == torch.float32
    e_loop = (_rows(_parts(loop)) - ref).norm(dim=-1) / ref.norm(dim=-1)
    e_fused = (_rows(_parts(fused)) - ref).norm(dim=-1) / ref.norm(dim=-1)
    _report({"test": "float32", "case": "A", "K": k, "loop": e_loop.tolist(), "fused": e_fused.tolist()})
    assert (e_fused <= torch.clamp(10.0 * e_loop, min=2e-6)).all(), (e_fused.tolist(), e_loop.tolist())
    with torch.no_grad():
        initial = _model(device, _tensors("A", torch.float32)).get_error()
        assert (fused.get_error() < initial).all()


# ---- 7. routing ----

def test_fused_keyword_routes_back_to_the_loop(device):
    """fused=True with a search_direction_network, a subclassed line search, or an input that requires grad under
    enable_grad takes the loop: last_trace_exit stays None and the results are the loop's."""
    from deep_attention_visual_odometry_amd.solvers import LineSearchStrongWolfeConditions

    s = _settings("A")
    with torch.no_grad():
        want = _parts(_solver(s, 2, False)(_model(device, _tensors("A"))))

    class Identity(torch.nn.Module):
        def forward(self, direction, parameters, error, iteration):
            return direction

    class Subclassed(LineSearchStrongWolfeConditions):
        pass

    def check(solver, model):
        out = solver(model)
        assert solver.last_trace_exit is None and solver.last_iterations is None
        for key, got in _parts(out).items():
            assert torch.equal(got.detach(), want[key]), key

    with torch.no_grad():
        check(_solver(s, 2, True, search_direction_network=Identity()), _model(device, _tensors("A")))
        check(_solver(s, 2, True, line_search_type=Subclassed), _model(device, _tensors("A")))
    t = _tensors("A")
    t["focal_length"] = t["focal_length"].to(device).requires_grad_(True)
    check(_solver(s, 2, True), _model(device, t))
    with torch.no_grad():  # the same tensors without a graph: the kernel
        solver = _solver(s, 2, True)
        solver(_model(device, t))
        assert solver.last_trace_exit is not None
