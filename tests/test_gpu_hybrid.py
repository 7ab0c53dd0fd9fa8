"""COMPACT past its history capacity: the HYBRID solve (csrc/solve_passes.hpp fold_history).

COMPACT keeps one history entry per BFGS update, at most 1024; a problem still running at iteration
1025 folds the history into the dense inverse Hessian once and continues with the dense sweep (the
reference's own data structure, bfgs_solver.py:263-303).  The COMPACT_SWITCH override lowers the
capacity so that the switch happens at K = 24 with capacity 8, where the oracle runs in seconds and the
parity bar is the fixed-K one (per-problem normwise <= 1e-5); the real capacity is exercised past
1025 iterations through size-independent properties (a problem that stops before the capacity gets the
compact solve's result bit for bit; past it the objective does not rise).
"""
import pytest
import torch

from oracle import objective, solver
from test_gpu_solver import TOL, _gpu_solve, _rel, _scene

pytestmark = pytest.mark.gpu

K, CAP = 24, 8


@pytest.mark.parametrize("shape,knobs", [
    ((2, 64, False, 8), {}),                                  # LDS mode, two waves
    ((4, 256, True, 4), {}),                                  # LDS mode, four waves, on-chip entries
    ((4, 256, True, 4), {"LDS_HISTORY": 3}),                  # the fold reads 3 entries from LDS, 5 from HBM
    ((4, 256, True, 4), {"LDS_HISTORY": 0, "SOLVE_WAVES": 1}),  # one wave per problem
    ((4, 256, True, 4), {"FORCE_GV": 1}),                     # global-vector mode, x and d in LDS
    ((4, 256, True, 4), {"FORCE_GV": 1, "GV_NO_XL": 1}),      # global-vector mode in place
    ((3, 1300, True, 2), {}),                                 # P = 3920: global-vector mode by size
    ((2, 3600, False, 1), {"GV_SCALAR_SLICE": 1}),            # P = 10,809: rho_j, c_j in the workspace slice
])
def test_hybrid_switch_matches_oracle(device, shape, knobs, overrides):
    """Capacity 8 at K = 24: 8 compact updates, the fold at iteration 9, 15 dense sweeps -- against the
    oracle (the reference's dense algorithm) and against the GPU's own pure COMPACT and DENSE solves."""
    m, n, dist, b = shape
    x0, obs, vis = _scene(b, m, n, dist, 4100 + n)
    kw = dict(iterations=K, error_threshold=-1.0, minimum_step=-1.0)
    ref = solver.bfgs_solve(x0, objective.ReprojectionClosure(obs, vis, m, n, dist), **kw)
    for name, value in knobs.items():
        overrides(name, value)
    compact, _ = _gpu_solve(device, x0, obs, vis, m, n, dist, hessian_mode="compact", **kw)
    dense, _ = _gpu_solve(device, x0, obs, vis, m, n, dist, hessian_mode="dense", **kw)
    overrides("COMPACT_SWITCH", CAP)
    hybrid, status = _gpu_solve(device, x0, obs, vis, m, n, dist, hessian_mode="compact", **kw)
    assert torch.isfinite(hybrid).all()
    assert (status[:, 0] == K).all() and (status[:, 1] == 0).all()
    assert _rel(hybrid, ref).max() <= TOL, _rel(hybrid, ref)
    assert _rel(hybrid, compact).max() <= TOL and _rel(hybrid, dense).max() <= TOL
    assert not torch.equal(hybrid, compact)  # the dense phase really ran (different rounding)


def test_past_1025_iterations(device):
    """The real capacity (1024 entries): K = 1100 on two-view problems, run to fp32 stagnation.  The
    hybrid kernel runs the compact solve up to iteration 1025, folds, and drives 75 more dense steps:
    finite, every step taken, the objective no higher than the K = 1025 compact solve's (each accepted
    step passes the sufficient-decrease test; 1% + 1e-8 E0 of slack for steps at stagnation), and the
    same converged fraction as the DENSE mode run to 1100.  The drop-in's 'auto' mode now takes
    COMPACT for such caps."""
    from deep_attention_visual_odometry_amd import BFGSSolver, _native, native_ops

    m, n = 2, 64
    x0, obs, vis = (t.to(device) for t in _scene(8, m, n, False, 4300))
    kw = dict(error_threshold=-1.0, minimum_step=-1.0, want_error=True, want_status=True)
    _, e_c, _ = native_ops.ba_solve(x0, obs, vis, m, n, False, iterations=1025, hessian_mode=1, **kw)
    x_h, e_h, s_h = native_ops.ba_solve(x0, obs, vis, m, n, False, iterations=1100, hessian_mode=1, **kw)
    _, e_d, _ = native_ops.ba_solve(x0, obs, vis, m, n, False, iterations=1100, hessian_mode=0, **kw)
    assert torch.isfinite(x_h).all() and (s_h[:, 0] == 1100).all() and (s_h[:, 1] == 0).all()
    e0, _, _ = native_ops.ba_evaluate(x0, obs, vis, m, n, False, want_grad=False)
    assert (e_h <= 1.01 * e_c + 1e-8 * e0).all(), (e_h, e_c)
    assert (e_h < 1e-3 * e0).float().mean() == (e_d < 1e-3 * e0).float().mean(), (e_h / e0, e_d / e0)
    s = BFGSSolver(iterations=2000)
    assert s._resolve_mode(2000, x0.shape[1], 8, device) == _native.DAVA_HESSIAN_COMPACT


def test_hybrid_with_stopping_rules_is_the_compact_solve(device):
    """With the reference's stopping rules the problems stop long before iteration 1025: an iteration cap
    of 3000 (HYBRID) gives the K = 1025 COMPACT solve's parameters and status words bit for bit on every
    problem that a rule stopped (problems are independent workgroups)."""
    from deep_attention_visual_odometry_amd import native_ops

    x0, obs, vis = (t.to(device) for t in _scene(64, 4, 256, True, 4400))
    kw = dict(error_threshold=1e-4, minimum_step=1e-8, want_status=True, hessian_mode=1)
    x_c, _, s_c = native_ops.ba_solve(x0, obs, vis, 4, 256, True, iterations=1025, **kw)
    x_h, _, s_h = native_ops.ba_solve(x0, obs, vis, 4, 256, True, iterations=3000, **kw)
    stopped = s_c[:, 1] != 0
    assert stopped.float().mean() >= 0.9, s_c
    assert torch.equal(x_c[stopped], x_h[stopped]) and torch.equal(s_c[stopped], s_h[stopped])


@pytest.mark.parametrize("knobs", [{}, {"FORCE_GV": 1}])
def test_hybrid_switch_ray_angle_matches_oracle(device, knobs, overrides):
    """The hybrid kernel with the ray-angle residual (CalibrationNetwork's error, its own template
    instantiations): capacity 8 at K = 10, LDS mode and global-vector mode, against the oracle's
    RayAngleClosure at the fixed-K bar used for that residual at this shape
    (test_ray_angle_fixed_iterations_match_oracle_c3_shape)."""
    from deep_attention_visual_odometry_amd import make_scenes
    from test_gpu_solver import _gpu_solve_ray

    s = make_scenes(2, 4, 256, seed=332, drop=0.1, ray_angle=True)
    x0, obs, vis = torch.tensor(s.initial), torch.tensor(s.observations), torch.tensor(s.visibility)
    kw = dict(iterations=10, error_threshold=-1.0, minimum_step=-1.0)
    ref = solver.bfgs_solve(x0, objective.RayAngleClosure(obs, vis, 4, 256), **kw)
    for name, value in knobs.items():
        overrides(name, value)
    overrides("COMPACT_SWITCH", 4)
    out, status = _gpu_solve_ray(device, x0, obs, vis, 4, 256, hessian_mode="compact", **kw)
    assert (status[:, 0] == 10).all()
    assert _rel(out, ref).max() <= TOL, _rel(out, ref)
