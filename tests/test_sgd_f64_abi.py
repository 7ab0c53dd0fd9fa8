"""The float64 fused gradient descent and its adjoint (dava_ba_sgd_*_f64, torch.ops.dava.ba_sgd_*_f64, the
``float64_descent`` keyword) without a GPU: declarations and exports, the size / form / workspace queries over a
grid, the launch entry points' refusals (codes and precedence, all before a device is touched), the fake kernels
and the keyword's checks."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

SYMBOLS = ("dava_ba_sgd_solve_f64", "dava_ba_sgd_solve_record_f64", "dava_ba_sgd_tape_bytes_f64",
           "dava_ba_sgd_solve_form_f64", "dava_ba_sgd_solve_workspace_bytes_f64", "dava_ba_sgd_backward_f64",
           "dava_ba_sgd_backward_form_f64", "dava_ba_sgd_backward_workspace_bytes_f64")
# (M, N, distortion) of the benchmark configurations, then M = 2 scenes past each form's boundary
C1, C2, C3, C5 = (2, 64, False), (2, 128, False), (4, 256, True), (16, 4096, False)
GRID = (C1, C2, C3, C5, (2, 1200, False), (2, 2400, False), (2, 3600, False))
LR = 1e-4
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 2, 4
TAIL = 256


@pytest.fixture(scope="module")
def native():
    from deep_attention_visual_odometry_amd import _native

    yield _native.load_library(), _native
    _native.clear_debug_overrides()


def _p(m, n, distortion):
    return 3 + 3 * n + 6 * (m - 1) + (5 if distortion else 0)


def _pv(m, n, distortion):
    return (_p(m, n, distortion) + 3) // 4 * 4


def _scene(N, b, m, n, distortion, residual=0, data=None):
    return N.DavaSceneF64(b, m, n, 1 if distortion else 0, _p(m, n, distortion), data, data, residual)


def _queries(lib, N, b, m, n, distortion, k, residual):
    sc, cfg = ctypes.byref(_scene(N, b, m, n, distortion, residual)), ctypes.byref(N.DavaSgdConfigF64(LR, k))
    return {"tape": lib.dava_ba_sgd_tape_bytes_f64(sc, cfg), "form": lib.dava_ba_sgd_solve_form_f64(sc, cfg),
            "ws": lib.dava_ba_sgd_solve_workspace_bytes_f64(sc, cfg),
            "bform": lib.dava_ba_sgd_backward_form_f64(sc, cfg),
            "bws": lib.dava_ba_sgd_backward_workspace_bytes_f64(sc, cfg, 0),
            "bws_obs": lib.dava_ba_sgd_backward_workspace_bytes_f64(sc, cfg, 1)}


def test_header_library_and_binding_agree(native):
    lib, N = native
    text = open(os.path.join(REPO, "include", "dava_ba.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dava_[a-z0-9_]+)\s*\(", text))
    assert len(SYMBOLS) == 8
    for name in SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in N.SIGNATURES, name
    assert re.search(r"typedef struct DavaSgdConfigF64 \{\s*double learning_rate;\s*int32_t iterations;\s*\} "
                     r"DavaSgdConfigF64;", text)
    assert N.DavaSgdConfigF64._fields_ == [("learning_rate", ctypes.c_double), ("iterations", ctypes.c_int32)]
    assert ctypes.sizeof(N.DavaSgdConfigF64) == 16
    assert int(re.search(r"#define DAVA_ABI_VERSION (\d+)", text).group(1)) == 4 == lib.dava_abi_version()  # additive
    assert N.DavaSgdConfigF64(1e-4, 1).learning_rate == 1e-4  # the learning rate crosses as a double, unrounded


@pytest.mark.parametrize("shape", GRID)
def test_queries_over_the_grid(native, shape):
    """Tape bytes B K round_up(P, 4) 8 (0 for K = 0); workspace bytes by the documented layouts; C1-C3 in form 0
    and C5 in form 2 for both operations; the F64_FORM override raises a form and never lowers it."""
    lib, N = native
    m, n, distortion = shape
    pv = _pv(m, n, distortion)
    for residual in (0, 1):
        if residual == 1 and distortion:
            continue  # (the ray-angle residual has no distortion: DAVA_ERR_UNSUPPORTED, below)
        for k in (0, 1, 20):
            for b in (1, 7):
                N.clear_debug_overrides()
                base = _queries(lib, N, b, m, n, distortion, k, residual)
                assert base["tape"] == b * k * pv * 8
                assert base["form"] in (0, 1, 2) and base["bform"] in (0, 1, 2)
                if shape in (C1, C2, C3):
                    assert base["form"] == 0 and base["bform"] == 0
                if shape == C5:
                    assert base["form"] == 2 and base["bform"] == 2
                for forced in (None, 1, 2):
                    if forced is not None:
                        N.set_debug_override("F64_FORM", forced)
                    q = _queries(lib, N, b, m, n, distortion, k, residual)
                    assert q["form"] == max(base["form"], forced or 0)
                    assert q["bform"] == max(base["bform"], forced or 0)
                    assert q["tape"] == base["tape"]  # one tape layout in every form
                    assert q["ws"] == (b * 2 * pv * 8 + TAIL if q["form"] == 2 else 0)
                    obsd = b * 4 * m * n * 8 if q["bform"] != 0 else 0
                    vecs = b * 4 * pv * 8 if q["bform"] == 2 else 0
                    assert q["bws"] == (vecs + TAIL if vecs else 0)
                    assert q["bws_obs"] == (obsd + vecs + TAIL if obsd + vecs else 0)
                N.clear_debug_overrides()


def test_forms_do_not_decrease_with_the_points(native):
    """M = 2: each operation's form is non-decreasing in N; the listed scenes take the expected pairs."""
    lib, N = native
    N.clear_debug_overrides()
    last = (0, 0)
    seen = set()
    for n in sorted(set(range(1, 4200, 37)) | {1200, 2400, 3600}):
        q = _queries(lib, N, 2, 2, n, False, 3, 0)
        assert q["form"] >= last[0] and q["bform"] >= last[1], n
        assert q["bform"] >= q["form"]  # (the dual image is the larger one)
        last = (q["form"], q["bform"])
        seen.add(last)
    assert seen == {(0, 0), (0, 1), (0, 2), (1, 2), (2, 2)}
    pairs = {n: _queries(lib, N, 2, 2, n, False, 3, 0) for n in (1200, 2400, 3600)}
    assert [(pairs[n]["form"], pairs[n]["bform"]) for n in (1200, 2400, 3600)] == [(0, 1), (1, 2), (2, 2)]


def test_queries_refuse_invalid_scenes_and_configs(native):
    lib, N = native
    N.clear_debug_overrides()
    cfg = ctypes.byref(N.DavaSgdConfigF64(LR, 5))
    ok = ctypes.byref(_scene(N, 4, 2, 16, False))
    one_view = N.DavaSceneF64(4, 1, 16, 0, 51, None, None, 0)
    wrong_p = N.DavaSceneF64(4, 2, 16, 0, 50, None, None, 0)
    for bad_scene in (None, ctypes.byref(one_view), ctypes.byref(wrong_p)):
        assert lib.dava_ba_sgd_tape_bytes_f64(bad_scene, cfg) == 0
        assert lib.dava_ba_sgd_solve_workspace_bytes_f64(bad_scene, cfg) == 0
        assert lib.dava_ba_sgd_backward_workspace_bytes_f64(bad_scene, cfg, 1) == 0
        assert lib.dava_ba_sgd_solve_form_f64(bad_scene, cfg) == -INVALID
        assert lib.dava_ba_sgd_backward_form_f64(bad_scene, cfg) == -INVALID
    for bad_cfg in (None, ctypes.byref(N.DavaSgdConfigF64(LR, -1))):
        assert lib.dava_ba_sgd_tape_bytes_f64(ok, bad_cfg) == 0
        assert lib.dava_ba_sgd_solve_form_f64(ok, bad_cfg) == -INVALID
        assert lib.dava_ba_sgd_backward_form_f64(ok, bad_cfg) == -INVALID
    # not even form 2's image fits: the view constants and partials of this many views
    many = ctypes.byref(_scene(N, 1, 2000, 4, False))
    assert lib.dava_ba_sgd_solve_form_f64(many, cfg) == -UNSUPPORTED
    assert lib.dava_ba_sgd_backward_form_f64(many, cfg) == -UNSUPPORTED
    assert lib.dava_ba_sgd_tape_bytes_f64(many, cfg) == 0
    ray_bc = ctypes.byref(_scene(N, 1, 2, 16, True, residual=1))
    assert lib.dava_ba_sgd_solve_form_f64(ray_bc, cfg) == -UNSUPPORTED


@pytest.mark.skipif(torch.cuda.is_available(),
                    reason="host logic: a refusal that regressed into an acceptance would launch on null pointers")
def test_launches_refuse_bad_arguments_before_a_device_is_touched(native):
    """The codes and their precedence: scene, config, empty batch, NULL vectors, unsupported, short tape or
    workspace."""
    lib, N = native
    N.clear_debug_overrides()
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # a dummy pointer, never dereferenced
    cfg = ctypes.byref(N.DavaSgdConfigF64(LR, 10))
    neg = ctypes.byref(N.DavaSgdConfigF64(LR, -1))

    def solve(sc, c=cfg, x0=p, xo=p, ws=None, wsb=0):
        return lib.dava_ba_sgd_solve_f64(sc, c, x0, xo, None, ws, wsb, None)

    def record(sc, c=cfg, x0=p, xo=p, tape=None, tb=0, ws=None, wsb=0):
        return lib.dava_ba_sgd_solve_record_f64(sc, c, x0, xo, None, tape, tb, ws, wsb, None)

    def backward(sc, c=cfg, tape=None, tb=0, go=p, gx=p, gobs=None, ws=None, wsb=0):
        return lib.dava_ba_sgd_backward_f64(sc, c, tape, tb, go, gx, gobs, ws, wsb, None)

    small = _scene(N, 4, 2, 16, False, data=p)
    sc = ctypes.byref(small)
    for call in (solve, record, backward):
        assert call(None) == INVALID  # 1. the scene
        assert call(ctypes.byref(N.DavaSceneF64(4, 2, 16, 0, 50, p, p, 0))) == INVALID
        assert call(ctypes.byref(_scene(N, 4, 2, 16, False))) == INVALID  # (no data pointers)
        assert call(sc, None) == INVALID and call(sc, neg) == INVALID  # 2. the config
        assert call(ctypes.byref(_scene(N, 0, 2, 16, False)), None) == INVALID  # ... before the empty batch
        assert call(ctypes.byref(_scene(N, 0, 2, 16, False))) == OK  # 3. an empty batch
    # ... which is OK before the NULL vectors and the unsupported image are looked at
    assert solve(ctypes.byref(_scene(N, 0, 2000, 4, False)), x0=None) == OK
    # 4. NULL vectors, before the unsupported image and the tape
    assert solve(sc, x0=None) == INVALID and solve(sc, xo=None) == INVALID
    assert record(sc, x0=None) == INVALID and record(sc, xo=None) == INVALID
    assert backward(sc, go=None) == INVALID and backward(sc, gx=None) == INVALID
    many = ctypes.byref(_scene(N, 1, 2000, 4, False, data=p))
    assert solve(many, x0=None) == INVALID and backward(many, gx=None) == INVALID
    # 5. unsupported, before the tape
    assert solve(many) == UNSUPPORTED and record(many) == UNSUPPORTED and backward(many) == UNSUPPORTED
    # 6. a missing or short tape
    tape_bytes = lib.dava_ba_sgd_tape_bytes_f64(sc, cfg)
    assert tape_bytes == 4 * 10 * _pv(2, 16, False) * 8
    assert record(sc) == WORKSPACE and record(sc, tape=p, tb=tape_bytes - 1) == WORKSPACE
    assert backward(sc) == WORKSPACE and backward(sc, tape=p, tb=tape_bytes - 1) == WORKSPACE
    # ... and a missing or short workspace at a form-2 shape
    m, n, distortion = C5
    big = ctypes.byref(_scene(N, 2, m, n, distortion, data=p))
    need = lib.dava_ba_sgd_solve_workspace_bytes_f64(big, cfg)
    assert need == 2 * 2 * _pv(m, n, distortion) * 8 + TAIL
    assert solve(big) == WORKSPACE and solve(big, ws=p, wsb=need - 1) == WORKSPACE
    big_tape = lib.dava_ba_sgd_tape_bytes_f64(big, cfg)
    assert record(big, tape=p, tb=big_tape) == WORKSPACE
    assert record(big, tape=p, tb=big_tape, ws=p, wsb=need - 1) == WORKSPACE
    assert record(big, ws=p, wsb=need) == WORKSPACE  # (the tape)
    for want_obs in (0, 1):
        bneed = lib.dava_ba_sgd_backward_workspace_bytes_f64(big, cfg, want_obs)
        gobs = p if want_obs else None
        assert backward(big, tape=p, tb=big_tape, gobs=gobs) == WORKSPACE
        assert backward(big, tape=p, tb=big_tape, gobs=gobs, ws=p, wsb=bneed - 1) == WORKSPACE
    # the override raises the small scene to form 2: it needs its workspace then
    N.set_debug_override("F64_FORM", 2)
    try:
        assert solve(sc) == WORKSPACE and backward(sc, tape=p, tb=tape_bytes) == WORKSPACE
    finally:
        N.clear_debug_overrides()


def test_operators_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from deep_attention_visual_odometry_amd import _ops

    names = ("ba_sgd_solve_f64", "ba_sgd_solve_differentiable_f64", "ba_sgd_backward_f64")
    for name in names:
        assert name in _ops.OPS
        assert getattr(torch.ops.dava, name).default._schema.name == f"dava::{name}"
    with FakeTensorMode():
        dev, f64 = "cuda", torch.float64
        p = _p(2, 18, False)
        rows = (p + 3) // 4 * 4
        assert rows != p  # (padded tape rows)
        x = torch.empty(5, p, device=dev, dtype=f64)
        obs = torch.empty(5, 2, 18, 2, device=dev, dtype=f64)
        vis = torch.empty(5, 2, 18, dtype=torch.uint8, device=dev)
        xo, errs = torch.ops.dava.ba_sgd_solve_f64(x, obs, vis, 2, 18, False, LR, 7, 0, True)
        assert xo.shape == x.shape and xo.dtype == f64 and errs.shape == (5, 7) and errs.dtype == f64
        xo, errs = torch.ops.dava.ba_sgd_solve_f64(x, obs, vis, 2, 18, False, LR, 7, 0, False)
        assert xo.shape == x.shape and errs.shape == (0,)
        xo, errs, tape = torch.ops.dava.ba_sgd_solve_differentiable_f64(x, obs, vis, 2, 18, False, LR, 7, 0, True)
        assert xo.shape == x.shape and xo.dtype == f64 and errs.shape == (5, 7) and errs.dtype == f64
        assert tape.shape == (5, 7, rows) and tape.dtype == f64
        _, errs, _ = torch.ops.dava.ba_sgd_solve_differentiable_f64(x, obs, vis, 2, 18, False, LR, 7, 0, False)
        assert errs.shape == (0,)
        gx, gobs = torch.ops.dava.ba_sgd_backward_f64(x, tape, obs, vis, 2, 18, False, LR, 7, 0, True)
        assert gx.shape == x.shape and gx.dtype == f64 and gobs.shape == obs.shape and gobs.dtype == f64
        gx, gobs = torch.ops.dava.ba_sgd_backward_f64(x, tape, obs, vis, 2, 18, False, LR, 7, 0, False)
        assert gobs.shape == (0,)
        # the differentiable operator is an autograd node w.r.t. x0 and the observations
        xg, og = x.clone().requires_grad_(True), obs.clone().requires_grad_(True)
        xo, _, _ = torch.ops.dava.ba_sgd_solve_differentiable_f64(xg, obs, vis, 2, 18, False, LR, 7, 0, False)
        assert xo.requires_grad
        xo, _, _ = torch.ops.dava.ba_sgd_solve_differentiable_f64(x, og, vis, 2, 18, False, LR, 7, 0, False)
        assert xo.requires_grad
        xo, _, _ = torch.ops.dava.ba_sgd_solve_differentiable_f64(x, obs, vis, 2, 18, False, LR, 7, 0, False)
        assert not xo.requires_grad


def test_operators_refuse_cpu_tensors():
    x = torch.zeros(2, _p(2, 16, False), dtype=torch.float64)
    obs = torch.zeros(2, 2, 16, 2, dtype=torch.float64)
    vis = torch.ones(2, 2, 16, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        torch.ops.dava.ba_sgd_solve_f64(x, obs, vis, 2, 16, False, LR, 3, 0, False)


def test_keyword_needs_float64_device_observations():
    from deep_attention_visual_odometry_amd import RayAngleError, ReprojectionError

    vis = torch.ones(2, 2, 16, dtype=torch.uint8)
    for cls in (ReprojectionError, RayAngleError):
        for obs in (torch.zeros(2, 2, 16, 2, dtype=torch.float64), torch.zeros(2, 2, 16, 2)):
            with pytest.raises(ValueError, match="float64_descent=True needs float64 observations on a ROCm device"):
                cls(obs, vis, 2, 16, float64_descent=True)
            assert cls(obs, vis, 2, 16).float64_descent is False
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():  # float32 observations on the device
        with pytest.raises(ValueError, match="float64_descent=True needs float64 observations"):
            ReprojectionError(torch.empty(2, 2, 16, 2, device="cuda"),
                              torch.empty(2, 2, 16, dtype=torch.uint8, device="cuda"), 2, 16, float64_descent=True)
        fn = ReprojectionError(torch.empty(2, 2, 16, 2, device="cuda", dtype=torch.float64),
                               torch.empty(2, 2, 16, dtype=torch.uint8, device="cuda"), 2, 16, float64_descent=True)
        assert fn.float64_descent and not fn.float64_derivatives and not fn.large_derivatives  # independent


def test_solver_on_cpu_float64_tensors_still_runs_the_loop():
    from deep_attention_visual_odometry_amd import ReprojectionError, SGDSolver, make_scenes

    s = make_scenes(2, 2, 9, seed=3)
    x0, obs = torch.tensor(s.initial).double(), torch.tensor(s.observations).double()
    solver = SGDSolver(LR, 3)
    out = solver(x0, ReprojectionError(obs, torch.tensor(s.visibility), 2, 9))
    assert solver.last_errors is None and out.dtype == torch.float64 and not torch.equal(out, x0)
