"""Training mode of the float64 fused solve: the drop path and return_second_last in dava_ba_solve_train_f64 /
dava_ba_solve_record_train_f64, their gradients through the float64 adjoint, and the drop-in BFGSSolver's
training-mode routes on an objective built with float64_derivatives=True.

What pins the semantics is bitwise: a dropped problem IS the eval solve of its step count, a return_second_last
problem stopped by the minimum-step rule IS the eval solve of one step fewer, the schedule of a seed IS the
float32 kernel's, and eval mode through the new entry points IS the old launch.
Bars against the CPU oracle run in float64 are the existing float64 tests' and no wider:
x_out: test_gpu_f64's solve bound, per problem and per block max(1e-5 * 2^-29, F x the oracle's own change under a
1-ulp nudge of x0, up and down); gradients: test_gpu_f64_grad's adjoint bound, per problem and per gradient
max(2e-3 * 2^-29, F x the oracle gradient's change under the same nudge); F = 12.5, the envelope_factor of
tests/golden/parity_envelope.json.  Training-mode oracle solves are nudged in solves of their own (the reference's
return_second_last scatter couples the problems of a batch, so the copies must not share one).

All scenes are make_scenes(..., drop=0.1) cast to double, as test_gpu_f64._scene builds them.
Measured on the MI355X: profiles/f64_training_parity.jsonl (the PARITY lines of one run), DESIGN.md 3.8.2.
"""
import ctypes
import json

import pytest
import torch

from oracle import objective, solver
from test_gpu_f64 import TOL, _envelope_factor, _rel, _scene
from test_gpu_f64_grad import ADJ_TOL, _oracle_grads, _rows_rel, _weights

pytestmark = pytest.mark.gpu

STOP_ITERATIONS, STOP_ERROR, STOP_STEP, STOP_DROP = 0, 1, 2, 3
# the seed-581 scene of the float32 return_second_last tests: the float64 oracle stops its 12 problems after these
# steps, all by the minimum-step rule (2e-3); asserted where the oracle runs
SL_SEED, SL_MIN_STEP, SL_B = 581, 2e-3, 12
SL_ORACLE_STEPS = [3, 2, 3, 6, 3, 5, 6, 3, 3, 5, 3, 3]


def _dev(device, *ts):
    return tuple(t.to(device) for t in ts)


def _solve(device, x0, obs, vis, m, n, ray=False, **kw):
    """native_ops.ba_solve in the dtype of x0 (compact history) -> (x, status) on the CPU."""
    from deep_attention_visual_odometry_amd import native_ops

    x, _, st = native_ops.ba_solve(*_dev(device, x0, obs, vis), m, n, False, hessian_mode=1, want_status=True,
                                   residual=1 if ray else 0, **kw)
    return x.cpu(), st.cpu()


def _fn(device, obs, vis, m, n, **kw):
    from deep_attention_visual_odometry_amd import ReprojectionError

    return ReprojectionError(obs.to(device), vis.to(device), m, n, False, **kw)


# ---- 1. the schedule of a seed is the float32 kernel's ----

def test_drop_schedule_equals_float32(device):
    m, n, b, k, p, seed = 2, 5, 64, 12, 0.25, 20240607
    x0, obs, vis = _scene(b, m, n, False, 51)
    kw = dict(iterations=k, error_threshold=-1.0, minimum_step=-1.0, drop_path_p=p, drop_seed=seed)
    x64, st64 = _solve(device, x0, obs, vis, m, n, **kw)
    x32, st32 = _solve(device, x0.float(), obs.float(), vis, m, n, **kw)
    assert x64.dtype == torch.float64 and x32.dtype == torch.float32
    assert torch.equal(st64[:, 0], st32[:, 0]), (st64[:, 0].tolist(), st32[:, 0].tolist())
    steps, reason = st64[:, 0], st64[:, 1]
    assert ((reason == STOP_ITERATIONS) | (reason == STOP_DROP)).all()
    assert torch.equal(steps < k, reason == STOP_DROP) and torch.equal(st64[:, 1], st32[:, 1])
    assert steps.unique().numel() >= 4 and int((steps == 0).sum()) >= 1, steps.tolist()
    assert torch.equal(x64[steps == 0], x0[steps == 0])
    # another seed, another schedule; the same seed, the same bits
    _, other = _solve(device, x0, obs, vis, m, n, **dict(kw, drop_seed=seed + 1))
    again, st_again = _solve(device, x0, obs, vis, m, n, **kw)
    assert not torch.equal(other[:, 0], steps) and torch.equal(again, x64) and torch.equal(st_again, st64)


# ---- 2. a dropped problem is the eval solve stopped early ----

@pytest.mark.parametrize("m,n,b,ray,scene_seed", [(2, 64, 48, False, 52), (2, 130, 8, True, 53)])
def test_dropped_problem_is_the_eval_solve_stopped_early(device, m, n, b, ray, scene_seed):
    k, p = 12, 0.2
    x0, obs, vis = _scene(b, m, n, False, scene_seed)
    x, st = _solve(device, x0, obs, vis, m, n, ray, iterations=k, error_threshold=-1.0, minimum_step=-1.0,
                   drop_path_p=p, drop_seed=72)
    steps = st[:, 0]
    assert torch.equal(steps < k, st[:, 1] == STOP_DROP)
    assert steps.unique().numel() >= 3 and int((steps == 0).sum()) >= 1, steps.tolist()
    for s in steps.unique().tolist():
        idx = (steps == s).nonzero().flatten()
        if s == 0:
            assert torch.equal(x[idx], x0[idx])
            continue
        ref, st_ref = _solve(device, x0[idx], obs[idx], vis[idx], m, n, ray, iterations=int(s), error_threshold=-1.0,
                             minimum_step=-1.0)
        assert torch.equal(x[idx], ref), s
        assert torch.equal(st[idx][:, [0, 2, 3]], st_ref[:, [0, 2, 3]])  # steps, evaluations, trials


# ---- 3. return_second_last is the solve before its last step ----

def _sl_scene():
    return _scene(SL_B, 2, 64, False, SL_SEED)


def test_second_last_is_the_solve_before_its_last_step(device):
    x0, obs, vis = _sl_scene()
    kw = dict(iterations=60, error_threshold=-1.0, minimum_step=SL_MIN_STEP)
    _, st0 = _solve(device, x0, obs, vis, 2, 64, **kw)
    # the cap at the median stopping step (3), as the float32 test sets it: problems stopped by the rule and by the cap
    kw["iterations"] = max(2, int(st0[:, 0].float().median().item()))
    assert kw["iterations"] == 3
    plain, st = _solve(device, x0, obs, vis, 2, 64, **kw)
    sl, st_sl = _solve(device, x0, obs, vis, 2, 64, return_second_last=True, **kw)
    assert torch.equal(st, st_sl)
    by_rule = st[:, 1] == STOP_STEP
    assert by_rule.sum() >= 4 and (~by_rule).sum() >= 1, st.tolist()
    assert torch.equal(sl[~by_rule], plain[~by_rule])
    for steps in st[by_rule, 0].unique().tolist():
        idx = (by_rule & (st[:, 0] == steps)).nonzero().flatten()
        assert steps >= 2  # (no problem of this scene fails the rule at its first step: iterations = steps - 1 >= 1)
        ref, _ = _solve(device, x0[idx], obs[idx], vis[idx], 2, 64, iterations=int(steps) - 1, error_threshold=-1.0,
                        minimum_step=-1.0)
        assert torch.equal(sl[idx], ref), steps
        assert not torch.equal(sl[idx], plain[idx])


# ---- the training-mode oracle with its own bounds ----

def _oracle_training(x0, obs, vis, w=None, **kw):
    """The float64 oracle's training-mode return_second_last solve of a (2, 64) batch, with autograd of w . x when w is
    given, and the nudged copies (x0 one ulp up, one ulp down) as solves of their own.  Returns the reference, its
    SolveRecord, the per-block bounds on x and (with w) the gradients and their bounds."""
    def run(x):
        xr = x.clone().requires_grad_(w is not None)
        orr = obs.clone().requires_grad_(w is not None)
        rec = solver.SolveRecord(None, None)
        out = solver.bfgs_solve(xr, objective.ReprojectionClosure(orr, vis, 2, 64), training=True,
                                return_second_last=True, drop_path_p=0.0, record=rec, **kw)
        if w is None:
            return out, None, None, rec
        (out * w).sum().backward()
        return out.detach(), xr.grad, orr.grad, rec

    ref = run(x0)
    up = run(torch.nextafter(x0, torch.full_like(x0, float("inf"))))
    down = run(torch.nextafter(x0, torch.full_like(x0, -float("inf"))))
    for other in (up, down):  # the copies took the reference's path
        assert torch.equal(other[3].iterations, ref[3].iterations) and torch.equal(other[3].reason, ref[3].reason)
    f, b = _envelope_factor(), x0.shape[0]

    def bound(i, floor, cols=slice(None)):
        r = ref[i].reshape(b, -1)[:, cols]
        spread = torch.maximum(_rows_rel(up[i].reshape(b, -1)[:, cols], r),
                               _rows_rel(down[i].reshape(b, -1)[:, cols], r))
        return torch.maximum(torch.full((b,), floor, dtype=torch.float64), f * spread)

    res = {"out": ref[0], "rec": ref[3], "env": {"all": bound(0, TOL), "intrinsics": bound(0, TOL, slice(0, 3))}}
    if w is not None:
        res.update(gx=ref[1], go=ref[2], bound_x=bound(1, ADJ_TOL), bound_obs=bound(2, ADJ_TOL))
    return res


def _check_x(tag, out, ref):
    rec = {"case": tag}
    for name, cols in (("all", slice(None)), ("intrinsics", slice(0, 3))):
        rel, env = _rel(out[:, cols], ref["out"][:, cols]), ref["env"][name]
        rec[name] = {"max_rel": float(rel.max()), "max_bound": float(env.max()), "max_ratio": float((rel / env).max())}
    print("PARITY", json.dumps(rec))
    for name in ("all", "intrinsics"):
        assert rec[name]["max_ratio"] <= 1.0, rec


def _check_grads(tag, gx, go, ref):
    ex, eo = _rows_rel(gx, ref["gx"]), _rows_rel(go, ref["go"])
    print("PARITY", json.dumps({"case": tag,
                                "x0": {"max_err": float(ex.max()), "max_bound": float(ref["bound_x"].max()),
                                       "max_ratio": float((ex / ref["bound_x"]).max())},
                                "obs": {"max_err": float(eo.max()), "max_bound": float(ref["bound_obs"].max()),
                                        "max_ratio": float((eo / ref["bound_obs"]).max())}}))
    assert (ex <= ref["bound_x"]).all(), (ex.tolist(), ref["bound_x"].tolist())
    assert (eo <= ref["bound_obs"]).all(), (eo.tolist(), ref["bound_obs"].tolist())


SL_KW = dict(iterations=60, error_threshold=-1.0, minimum_step=SL_MIN_STEP)


def _sl_solver(**extra):
    from deep_attention_visual_odometry_amd import BFGSSolver

    s = BFGSSolver(drop_path_p=0.0, return_second_last=True, training_iterations=SL_KW["iterations"],
                   training_error_threshold=SL_KW["error_threshold"], minimum_step=SL_KW["minimum_step"], **extra)
    assert s.training
    return s


# ---- 4. return_second_last against the oracle ----

def test_second_last_matches_the_float64_oracle(device):
    x0, obs, vis = _sl_scene()
    for i in range(4):
        one = (x0[i:i + 1], obs[i:i + 1], vis[i:i + 1])
        ref = _oracle_training(*one, **SL_KW)
        assert ref["rec"].iterations.tolist() == [SL_ORACLE_STEPS[i]] and ref["rec"].reason.tolist() == [STOP_STEP]
        s = _sl_solver()
        out = s(one[0].to(device), _fn(device, one[1], one[2], 2, 64, float64_derivatives=True))
        assert s.last_status is not None and out.dtype == torch.float64  # the fused route ran
        st = s.last_status.cpu()
        assert torch.equal(st[:, 0], ref["rec"].iterations) and torch.equal(st[:, 1], ref["rec"].reason)
        _check_x(f"second_last64_m2_n64_problem{i}", out.cpu(), ref)


# ---- 5. a batch whose scatter moves rows falls back; reordered, it runs fused ----

def _descending(st):
    """The batch order that moves no rows: latest stop first (stable)."""
    return torch.tensor(sorted(range(st.shape[0]), key=lambda i: -int(st[i, 0])))


def test_row_moving_batch_falls_back_and_the_reordered_batch_runs_fused(device):
    from deep_attention_visual_odometry_amd import native_ops

    x0, obs, vis = _sl_scene()
    _, st = _solve(device, x0, obs, vis, 2, 64, return_second_last=True, **SL_KW)
    assert st[:, 0].tolist() == SL_ORACLE_STEPS and (st[:, 1] == STOP_STEP).all()
    assert native_ops.second_last_moves_rows(st)  # problem 1 stops at step 2 while later ones continue
    fn = _fn(device, obs, vis, 2, 64, float64_derivatives=True)
    s = _sl_solver()
    out = s(x0.to(device), fn)
    assert s.last_status is None  # the generic loop ran
    ref = _sl_solver()._generic(x0.to(device), fn, SL_KW["error_threshold"], SL_KW["iterations"])
    assert torch.equal(out, ref)
    order = _descending(st)
    s = _sl_solver()
    out = s(x0[order].to(device), _fn(device, obs[order], vis[order], 2, 64, float64_derivatives=True))
    assert s.last_status is not None and not native_ops.second_last_moves_rows(s.last_status)
    assert torch.equal(s.last_status.cpu(), st[order])


# ---- 6. gradients under the drop path ----

def _drop_run(device, x0, obs, vis, w, k, p, seed):
    from deep_attention_visual_odometry_amd import BFGSSolver

    xd = x0.to(device).requires_grad_(True)
    od = obs.to(device).requires_grad_(True)
    s = BFGSSolver(drop_path_p=p, training_iterations=k, training_error_threshold=-1.0, minimum_step=-1.0)
    assert s.training
    torch.manual_seed(seed)
    out = s(xd, _fn(device, od, vis, 2, 5, float64_derivatives=True))
    assert s.last_status is not None and out.requires_grad  # the recording solve + adjoint
    (out * w.to(device)).sum().backward()
    return out.detach().cpu(), xd.grad.cpu(), od.grad.cpu(), s.last_status.cpu()


def test_gradients_under_the_drop_path(device):
    m, n, b, k, p = 2, 5, 16, 6, 0.3
    x0, obs, vis = _scene(b, m, n, False, 54)
    w = _weights(x0.shape, 6)
    out, gx, go, st = _drop_run(device, x0, obs, vis, w, k, p, seed=3)
    steps = st[:, 0]
    assert torch.equal(steps < k, st[:, 1] == STOP_DROP)
    zero = steps == 0
    assert int(zero.sum()) >= 1 and steps[~zero].unique().numel() >= 2, steps.tolist()
    assert torch.equal(out[zero], x0[zero]) and torch.equal(gx[zero], w[zero]) and (go[zero] == 0).all()
    for s in steps[~zero].unique().tolist():
        idx = (steps == s).nonzero().flatten()
        ref = _oracle_grads(x0[idx], obs[idx], vis[idx], m, n, False, False, w[idx], iterations=int(s),
                            error_threshold=-1.0, minimum_step=-1.0)
        assert (ref["rec"].iterations == s).all()
        rel = _rel(out[idx], ref["out"])
        assert (rel <= ref["env_out"]["all"]).all(), (s, rel.tolist())
        _check_grads(f"drop64_m2_n5_steps{s}", gx[idx], go[idx], ref)
    again = _drop_run(device, x0, obs, vis, w, k, p, seed=3)
    assert all(torch.equal(a, c) for a, c in zip((out, gx, go, st), again))
    other = _drop_run(device, x0, obs, vis, w, k, p, seed=4)
    assert not torch.equal(other[3][:, 0], steps)


# ---- 7. gradients under return_second_last ----

def test_second_last_gradients_match_the_float64_oracle(device):
    from deep_attention_visual_odometry_amd import native_ops

    x0, obs, vis = _sl_scene()
    w = _weights(x0.shape, 12)

    def run(idx, tag):
        xs, os_, vs, ws = x0[idx], obs[idx], vis[idx], w[idx]
        xd = xs.to(device).requires_grad_(True)
        od = os_.to(device).requires_grad_(True)
        s = _sl_solver()
        out = s(xd, _fn(device, od, vs, 2, 64, float64_derivatives=True))
        assert s.last_status is not None and not native_ops.second_last_moves_rows(s.last_status)
        (out * ws.to(device)).sum().backward()
        ref = _oracle_training(xs, os_, vs, ws, **SL_KW)
        st = s.last_status.cpu()
        assert torch.equal(st[:, 0], ref["rec"].iterations) and torch.equal(st[:, 1], ref["rec"].reason)
        _check_x(f"second_last64_{tag}", out.detach().cpu(), ref)
        _check_grads(f"second_last64_grad_{tag}", xd.grad.cpu(), od.grad.cpu(), ref)
        return int((st[:, 1] == STOP_STEP).sum())

    checked = sum(run(torch.tensor([i]), f"problem{i}") for i in range(3))
    assert checked >= 2  # single problems stopped by the rule: each adjoint replays one step fewer
    # the whole batch, latest stop first: the reference's scatter moves no rows, so it runs fused
    order = _descending(torch.tensor(SL_ORACLE_STEPS).reshape(-1, 1))
    assert run(order, "descending_batch") == SL_B


# ---- 8. routes ----

def test_training_mode_routes(device, overrides):
    from deep_attention_visual_odometry_amd import BFGSSolver

    m, n, b = 2, 5, 16
    x0, obs, vis = _scene(b, m, n, False, 55)
    kw = dict(drop_path_p=0.1, training_iterations=20, training_error_threshold=-1.0, minimum_step=-1.0)

    def run(keyword, **extra):
        s = BFGSSolver(**kw, **extra)
        torch.manual_seed(11)
        out = s(x0.to(device), _fn(device, obs, vis, m, n, float64_derivatives=keyword))
        assert out.dtype == torch.float64 and torch.isfinite(out).all()
        return s.last_status

    st = run(True)
    assert st is not None and int((st[:, 1] == STOP_DROP).sum()) >= 1
    assert run(False) is None  # without the keyword: the generic loop with torch's random stream, as before
    assert run(True, hessian_mode="dense") is None
    overrides("GENERIC_TRAINING", 1)
    assert run(True) is None
    # ... and with gradients: the recording solve + adjoint, or the generic loop under GENERIC_BACKWARD
    overrides("GENERIC_TRAINING", -1)
    for generic in (False, True):
        overrides("GENERIC_BACKWARD", 1 if generic else -1)
        xd = x0.to(device).requires_grad_(True)
        s = BFGSSolver(**kw)
        s(xd, _fn(device, obs, vis, m, n, float64_derivatives=True)).sum().backward()
        assert (s.last_status is None) == generic and torch.isfinite(xd.grad).all()


# ---- 9. eval mode through the new entry points is the old launch ----

def test_eval_mode_through_the_training_entry_points_is_unchanged(device):
    from deep_attention_visual_odometry_amd import _native as N
    from deep_attention_visual_odometry_amd import _ops

    m, n, b, k = 3, 70, 3, 12
    x0, obs, vis = _dev(device, *_scene(b, m, n, True, 32))
    vis = vis.to(torch.uint8).contiguous()
    lib = N.load_library()
    sc = _ops.scene_struct_f64(obs, vis, m, n, True, b)
    cfg = _ops.solver_config_f64(1e-4, 0.9, -1.0, k, -1.0, 1000, True)
    sizes = {False: int(lib.dava_ba_solve_workspace_bytes_f64(sc, cfg)),
             True: int(lib.dava_ba_solve_tape_bytes_f64(sc, cfg))}
    stream = N.stream_of(device)

    def launch(record, training):
        x = torch.empty_like(x0)
        err = torch.empty(b, dtype=torch.float64, device=device)
        st = torch.empty((b, 4), dtype=torch.int32, device=device)
        ws = torch.full((sizes[record],), 255, dtype=torch.uint8, device=device)
        head = (sc, cfg) if training == "old" else (sc, cfg, training)
        name = "dava_ba_solve" + ("_record" if record else "") + ("" if training == "old" else "_train") + "_f64"
        with torch.cuda.device(device):
            N.check(getattr(lib, name)(*head, N.ptr(x0), N.ptr(x), N.ptr(err), N.ptr(st), N.ptr(ws), ws.numel(),
                                       stream), name)
        torch.cuda.synchronize(device)
        return x, err, st, ws

    for record in (False, True):
        old = launch(record, "old")
        assert (old[2][:, 0] == k).all()
        for training in (None, ctypes.byref(N.DavaTrainingF64(0.0, 0, 0, 0)),
                         ctypes.byref(N.DavaTrainingF64(0.0, 9, 9, 0))):
            new = launch(record, training)
            assert all(torch.equal(a, c) for a, c in zip(old[:3], new[:3]))
            if record:
                assert torch.equal(old[3], new[3])  # the tape, byte for byte
    # a training launch on the same inputs differs (the flag reaches the kernel)
    drop = launch(False, ctypes.byref(N.DavaTrainingF64(0.5, 5, 0, 0)))
    assert (drop[2][:, 0] < k).any()
