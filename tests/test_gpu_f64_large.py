"""The float64 fused path beyond the LDS image (dava_ba_evaluate_large_f64, dava_ba_solve_large_f64): form 1
(the scene read in place) and form 2 (the six vectors in the workspace too), forced on the small shapes of
test_gpu_f64.py through the F64_FORM override and taken naturally by two scenes the old entry points refuse.

Bars: test_gpu_f64.py's, unchanged -- evaluation E_RTOL / G_TOL / SLOPE_RTOL (2e-5, 1e-4, 1e-3, each x 2^-29);
solves per problem and block max(1e-5 * 2^-29, F x the float64 oracle's own change under a 1-ulp nudge of x0),
F from tests/golden/parity_envelope.json.  On top of them the forms are compared with form 0 bit for bit: they
run one text of the solve with other pointers (csrc/solve_f64.hpp).

Natural shapes (B = 2): (6, 700, Brown-Conrady, seed 51), P = 2138, form 1; (2, 1200, seed 52), P = 3609, form 2.
Measured on the MI355X: profiles/f64_large_parity.jsonl (the EVAL64 / PARITY lines of one run), DESIGN.md 3.8.3.
"""
import functools

import pytest
import torch

from oracle import objective, solver
from test_gpu_f64 import (B, E_RTOL, SHAPES, _blocks, _check_evaluation, _gpu_solve, _oracle_solve,
                          _oracle_with_envelopes, _report, _scene, _stopping_scene)

pytestmark = pytest.mark.gpu

STOP_ITERATIONS, STOP_ERROR, STOP_STEP, STOP_DROP = 0, 1, 2, 3
# name -> (M, N, distortion, ray angle, scene seed, the form it takes, iteration counts solved)
NATURAL = {
    "m6_n700_bc": (6, 700, True, False, 51, 1, (3, 12)),
    "m2_n1200": (2, 1200, False, False, 52, 2, (3, 8)),
}
NATURAL_B = 2


def _forced(form):
    from deep_attention_visual_odometry_amd import _native

    return _native.debug_overrides(F64_FORM=form)


def _solve(device, x0, obs, vis, m, n, distortion=False, ray=False, **kw):
    """native_ops.ba_solve on a float64 batch (compact history) -> (x, error, status) on the CPU."""
    from deep_attention_visual_odometry_amd import native_ops

    x, err, st = native_ops.ba_solve(x0.to(device), obs.to(device), vis.to(device), m, n, distortion, hessian_mode=1,
                                     want_error=True, want_status=True, residual=1 if ray else 0, **kw)
    assert x.dtype == torch.float64 and err.dtype == torch.float64
    return x.cpu(), err.cpu(), st.cpu()


def _form_of(b, m, n, distortion, ray, k):
    from deep_attention_visual_odometry_amd import native_ops

    return native_ops.solve_form_f64(b, m, n, distortion, iterations=k, residual=1 if ray else 0)


def _assert_within(rel, env):
    for block in rel:
        assert (rel[block] <= env[block]).all(), (block, rel[block].tolist(), env[block].tolist())


# ---- 1. forced forms on the small shapes ----

@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forced_form_evaluation_matches_the_float64_oracle(device, shape, form):
    """Every instantiation _check_evaluation reaches (GRAD + SLOPE + TRIAL, GRAD, SLOPE + TRIAL and, with the
    direction zero on the intrinsics, GRAD + SLOPE, GRAD and SLOPE at x itself) in forms 1 and 2."""
    m, n, distortion, ray, seed = SHAPES[shape]
    x, obs, vis = _scene(B, m, n, distortion, seed)
    with _forced(form):
        _check_evaluation(device, x, obs, vis, m, n, distortion, ray, f"form{form}_{shape}", fixed=slice(0, 3))


@pytest.mark.parametrize("k", [3, 20])
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forced_form_solve_matches_the_oracle_and_form_0(device, shape, form, k):
    m, n, distortion, ray, seed = SHAPES[shape]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    ref, rec, env = _oracle_solve(shape, k)
    kw = dict(iterations=k, error_threshold=-1.0, minimum_step=-1.0)
    assert _form_of(B, m, n, distortion, ray, k) == 0
    base, base_err, base_st = _solve(device, x0, obs, vis, m, n, distortion, ray, **kw)
    with _forced(form):
        assert _form_of(B, m, n, distortion, ray, k) == form
        out, err, status = _solve(device, x0, obs, vis, m, n, distortion, ray, **kw)
    rel = _blocks(out, ref, distortion)
    _report(f"form{form}_{shape}_K{k}", rel, env)
    assert (status[:, 0] == k).all() and torch.equal(status[:, 0], rec.iterations)
    assert (status[:, 1] == STOP_ITERATIONS).all()
    _assert_within(rel, env)
    # the same text with other pointers: the same bits
    assert torch.equal(status, base_st)
    assert torch.equal(out, base), (out - base).abs().max().item()
    assert torch.equal(err, base_err)


# ---- 2. natural forms, no override ----

@functools.lru_cache(maxsize=None)
def _natural_oracle(shape, k):
    m, n, distortion, ray, seed, _, _ = NATURAL[shape]
    x0, obs, vis = _scene(NATURAL_B, m, n, distortion, seed)
    return _oracle_with_envelopes(x0, obs, vis, m, n, distortion, ray, iterations=k, error_threshold=-1.0,
                                  minimum_step=-1.0)


@pytest.mark.parametrize("shape", list(NATURAL))
def test_natural_form_evaluation(device, shape):
    m, n, distortion, ray, seed, form, ks = NATURAL[shape]
    assert _form_of(NATURAL_B, m, n, distortion, ray, ks[-1]) == form
    x, obs, vis = _scene(NATURAL_B, m, n, distortion, seed)
    _check_evaluation(device, x, obs, vis, m, n, distortion, ray, f"natural_{shape}", fixed=slice(0, 3))


@pytest.mark.parametrize("shape,k", [(s, k) for s in NATURAL for k in NATURAL[s][6]])
def test_natural_form_solve_matches_the_float64_oracle(device, shape, k):
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray, seed, form, _ = NATURAL[shape]
    assert _form_of(NATURAL_B, m, n, distortion, ray, k) == form
    assert native_ops.solve_workspace_bytes_f64(NATURAL_B, m, n, distortion, iterations=k) == 0  # refused before
    x0, obs, vis = _scene(NATURAL_B, m, n, distortion, seed)
    ref, rec, env = _natural_oracle(shape, k)
    assert torch.isfinite(ref).all() and (rec.iterations == k).all()
    out, err, status = _solve(device, x0, obs, vis, m, n, distortion, ray, iterations=k, error_threshold=-1.0,
                              minimum_step=-1.0)
    rel = _blocks(out, ref, distortion)
    _report(f"natural_form{form}_{shape}_K{k}", rel, env)
    assert torch.isfinite(out).all() and torch.isfinite(err).all()
    assert (status[:, 0] == k).all() and (status[:, 1] == STOP_ITERATIONS).all()
    _assert_within(rel, env)
    e_ref = objective.reprojection_error(out, obs, vis, m, n, distortion)
    assert ((err - e_ref).abs() / e_ref.abs()).max().item() <= E_RTOL  # error_out is E(x_out)


# ---- 3. the workspace's previous contents ----

def test_poisoned_workspace_changes_nothing(device):
    """Form 2's vector slices (and the history rows) arrive uninitialised: a workspace of NaN bytes gives the
    bits of a zero-filled one.  (The poisoned block is zeroed again before it goes back to the caching
    allocator: later tests' launches draw their workspaces from it.)"""
    from deep_attention_visual_odometry_amd import native_ops

    m, n, distortion, ray, seed = SHAPES["m3_n70_bc"]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    kw = dict(iterations=12, error_threshold=-1.0, minimum_step=-1.0)
    with _forced(2):
        need = native_ops.solve_large_workspace_bytes_f64(B, m, n, distortion, iterations=12)
        pv = (x0.shape[1] + 3) // 4 * 4
        assert need == B * (2 * 11 + 6) * pv * 8 + 256
        zeros = torch.zeros(need, dtype=torch.uint8, device=device)
        clean = _solve(device, x0, obs, vis, m, n, distortion, ray, workspace=zeros, **kw)
        poison = torch.full((need,), 0xFF, dtype=torch.uint8, device=device)
        try:
            assert torch.isnan(poison.view(torch.float64)).all()
            dirty = _solve(device, x0, obs, vis, m, n, distortion, ray, workspace=poison, **kw)
        finally:
            poison.zero_()
    assert torch.isfinite(clean[0]).all()
    for a, b in zip(clean, dirty):
        assert torch.equal(a, b)


# ---- 4. determinism and independence ----

def test_form_2_is_deterministic_and_problems_are_independent(device):
    m, n, distortion, ray, seed = SHAPES["m3_n70_bc"]
    x0, obs, vis = _scene(B, m, n, distortion, seed)
    kw = dict(iterations=12, error_threshold=-1.0, minimum_step=-1.0)
    with _forced(2):
        a = _solve(device, x0, obs, vis, m, n, distortion, ray, **kw)
        b = _solve(device, x0, obs, vis, m, n, distortion, ray, **kw)
        assert all(torch.equal(s, t) for s, t in zip(a, b))
        for i in range(B):
            one = _solve(device, x0[i:i + 1], obs[i:i + 1], vis[i:i + 1], m, n, distortion, ray, **kw)
            assert all(torch.equal(s[0], t[i]) for s, t in zip(one, a))
        bad = x0.clone()
        bad[1, 4] = float("nan")
        out, _, status = _solve(device, bad, obs, vis, m, n, distortion, ray, **kw)
    assert status[1, 0] == 0 and status[1, 1] == STOP_ERROR
    assert torch.equal(out[[0, 2]], a[0][[0, 2]]) and torch.equal(status[[0, 2]], a[2][[0, 2]])


# ---- 5. the reference's stopping rules ----

@functools.lru_cache(maxsize=None)
def _stopping_oracle(case):
    x0, obs, vis = _stopping_scene(case)
    traj = []
    ref, rec, env = _oracle_with_envelopes(x0, obs, vis, 2, 64, False, False, trajectory=traj)
    return ref, rec, env, traj


@pytest.mark.parametrize("case,margin", [("factor2", 2.0), ("seed15", 1.01)])
def test_reference_stopping_rules_in_form_2(device, case, margin):
    """test_gpu_f64.test_reference_stopping_rules' two batches (the reference's defaults 1e-4 / 1000 / 1e-8) with the
    vectors in the workspace: stop iteration and reason equal the oracle's, with that test's margins."""
    m, n, b = 2, 64, 4
    x0, obs, vis = _stopping_scene(case)
    ref, rec, env, traj = _stopping_oracle(case)
    assert (rec.reason == solver.STOP_ERROR).all()
    for i in range(b):
        s = int(rec.iterations[i])
        at_stop = objective.reprojection_error(traj[s - 1][i:i + 1], obs[i:i + 1], vis[i:i + 1], m, n).item()
        before = objective.reprojection_error((traj[s - 2] if s >= 2 else x0)[i:i + 1], obs[i:i + 1], vis[i:i + 1],
                                              m, n).item()
        assert at_stop <= 1e-4 / margin and before >= margin * 1e-4, (i, s, at_stop, before)
    with _forced(2):
        out, status = _gpu_solve(device, x0, obs, vis, m, n, False, False)
    rel = _blocks(out, ref, False)
    _report(f"form2_stopping64_{case}_m2_n64", rel, env)
    assert torch.equal(status[:, 0], rec.iterations), (status[:, 0].tolist(), rec.iterations.tolist())
    assert torch.equal(status[:, 1], rec.reason)
    _assert_within(rel, env)


# ---- 6. training mode ----

def test_training_mode_in_form_2(device):
    """The drop path (one schedule per seed: form 0's) and return_second_last, through the kernel's TRAIN flag
    with the vectors in the workspace; the drop-in solver in training mode on an objective built with
    float64_derivatives=True takes the same launch."""
    from deep_attention_visual_odometry_amd import BFGSSolver, ReprojectionError

    m, n, b, k, p, seed = 2, 5, 16, 12, 0.5, 20240611
    x0, obs, vis = _scene(b, m, n, False, 61)
    kw = dict(iterations=k, error_threshold=-1.0, minimum_step=-1.0)
    base = _solve(device, x0, obs, vis, m, n, drop_path_p=p, drop_seed=seed, **kw)
    with _forced(2):
        got = _solve(device, x0, obs, vis, m, n, drop_path_p=p, drop_seed=seed, **kw)
        steps, reason = got[2][:, 0], got[2][:, 1]
        assert torch.equal(got[2], base[2]) and torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
        assert torch.equal(steps < k, reason == STOP_DROP) and steps.unique().numel() >= 3, steps.tolist()
        for s in steps.unique().tolist():  # a dropped problem is the eval solve of its step count
            idx = (steps == s).nonzero().flatten()
            if s == 0:
                assert torch.equal(got[0][idx], x0[idx])
                continue
            ref = _solve(device, x0[idx], obs[idx], vis[idx], m, n, iterations=int(s), error_threshold=-1.0,
                         minimum_step=-1.0)
            assert torch.equal(got[0][idx], ref[0]), s
            assert torch.equal(got[2][idx][:, [0, 2, 3]], ref[2][:, [0, 2, 3]])
    # return_second_last on the factor2 batch, minimum-step stops included (2e-3 stops its problems early)
    fx, fobs, fvis = _stopping_scene("factor2")
    sl_kw = dict(iterations=30, error_threshold=-1.0, minimum_step=2e-3, return_second_last=True)
    sl_base = _solve(device, fx, fobs, fvis, 2, 64, **sl_kw)
    with _forced(2):
        sl = _solve(device, fx, fobs, fvis, 2, 64, **sl_kw)
    assert all(torch.equal(s, t) for s, t in zip(sl, sl_base))
    # ... and on test_gpu_f64_training's seed-581 batch, which the minimum-step rule does stop (cap 3, as there)
    sx, sobs, svis = _scene(12, 2, 64, False, 581)
    sl_kw["iterations"] = 3
    sl_base = _solve(device, sx, sobs, svis, 2, 64, **sl_kw)
    plain = _solve(device, sx, sobs, svis, 2, 64, **dict(sl_kw, return_second_last=False))
    with _forced(2):
        sl = _solve(device, sx, sobs, svis, 2, 64, **sl_kw)
    by_rule = sl[2][:, 1] == STOP_STEP
    assert by_rule.sum() >= 4 and not torch.equal(sl[0][by_rule], plain[0][by_rule])
    assert all(torch.equal(s, t) for s, t in zip(sl, sl_base))
    # the drop-in solver, training mode without a graph: fused (status words), one schedule per torch seed
    fn = ReprojectionError(obs.to(device), vis.to(device), m, n, False, float64_derivatives=True)
    s = BFGSSolver(drop_path_p=p, training_iterations=k, training_error_threshold=-1.0, minimum_step=-1.0)
    assert s.training
    torch.manual_seed(7)
    drop_base = s(x0.to(device), fn).cpu()
    st_base = s.last_status.cpu()
    with _forced(2):
        torch.manual_seed(7)
        drop = s(x0.to(device), fn).cpu()
        assert s.last_status is not None and torch.equal(s.last_status.cpu(), st_base)
    assert torch.equal(drop, drop_base) and (st_base[:, 1] == STOP_DROP).any()


# ---- 7. the drop-in surface ----

def test_drop_in_surface_on_a_scene_beyond_the_lds_image(device):
    from deep_attention_visual_odometry_amd import BFGSSolver, ReprojectionError

    m, n, distortion, ray, seed, form, _ = NATURAL["m2_n1200"]
    assert form == 2
    x0, obs, vis = _scene(NATURAL_B, m, n, distortion, seed)
    ref, _, env = _natural_oracle("m2_n1200", 3)
    kw = dict(iterations=3, error_threshold=-1.0, minimum_step=-1.0)
    x32, obs32 = x0.float().to(device), obs.float().to(device)
    before = BFGSSolver(**kw).eval()(x32, ReprojectionError(obs32, vis.to(device), m, n, distortion))
    out, status = _gpu_solve(device, x0, obs, vis, m, n, distortion, ray, **kw)  # float64 on the device: asserted there
    assert status is not None and status.shape == (NATURAL_B, 4)
    rel = _blocks(out, ref, distortion)
    _report("dropin_form2_m2_n1200_K3", rel, env)
    _assert_within(rel, env)
    # dense mode has no float64 kernel: the generic loop, whose closure is the evaluation
    dense, st = _gpu_solve(device, x0, obs, vis, m, n, distortion, ray, hessian_mode="dense", **kw)
    assert st is None
    rel = _blocks(dense, ref, distortion)
    _report("generic64_dense_m2_n1200_K3", rel, env)
    _assert_within(rel, env)
    # no recording solve, adjoint or second derivatives beyond the LDS image: refused before any launch
    fn = ReprojectionError(obs.to(device), vis.to(device), m, n, distortion, float64_derivatives=True)
    with pytest.raises(ValueError, match="160 KiB"):
        BFGSSolver(**kw).eval()(x0.to(device).requires_grad_(True), fn)
    # float32 is untouched
    after = BFGSSolver(**kw).eval()(x32, ReprojectionError(obs32, vis.to(device), m, n, distortion))
    assert before.dtype == torch.float32 and torch.equal(before, after)
