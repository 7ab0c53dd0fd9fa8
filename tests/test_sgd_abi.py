"""The fused gradient descent (dava_ba_sgd_*, torch.ops.dava.ba_sgd_*, SGDSolver) without a GPU: declarations and
exports, the size queries, argument checks that return before a device is touched, the fake kernels, and
SGDSolver on CPU tensors against the reference's golden and the in-test loop (sgd_oracle.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sgd_oracle
from conftest import GOLDEN, REPO

SGD_SYMBOLS = ("dava_ba_sgd_solve", "dava_ba_sgd_tape_bytes", "dava_ba_sgd_solve_record",
               "dava_ba_sgd_backward_supported", "dava_ba_sgd_backward")
# (M, N, distortion) of the benchmark configurations
C1, C2, C3, C5 = (2, 64, False), (2, 128, False), (4, 256, True), (16, 4096, False)
LR = 1e-4
GOLDEN_CASES = {"pinhole": (2, 64, False, False), "ray": (2, 64, False, True), "bc": (3, 70, True, False)}


@pytest.fixture(scope="module")
def lib():
    from deep_attention_visual_odometry_amd import _native

    return _native.load_library()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sgd.npz"))


def _p(m, n, distortion):
    return 3 + 3 * n + 6 * (m - 1) + (5 if distortion else 0)


def _scene(b, m, n, distortion, residual=0, p=None):
    from deep_attention_visual_odometry_amd import _native as N

    return N.DavaScene(b, m, n, 1 if distortion else 0, _p(m, n, distortion) if p is None else p, None, None, residual)


def _config(iterations=10, lr=LR):
    from deep_attention_visual_odometry_amd import _native as N

    return N.DavaSgdConfig(lr, iterations)


def _golden_case(golden, name):
    m, n, distortion, ray = GOLDEN_CASES[name]
    x0, obs, vis = (torch.tensor(golden[name + s]) for s in ("_x0", "_obs", "_vis"))
    return x0, obs, vis, m, n, distortion, ray


def test_header_library_and_binding_agree(lib):
    from deep_attention_visual_odometry_amd import _native as N

    text = open(os.path.join(REPO, "include", "dava_ba.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dava_[a-z0-9_]+)\s*\(", text))
    for name in SGD_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in N.SIGNATURES
    assert re.search(r"typedef struct DavaSgdConfig \{\s*float learning_rate;\s*int32_t iterations;\s*\} DavaSgdConfig;",
                     text)
    assert N.DavaSgdConfig._fields_ == [("learning_rate", ctypes.c_float), ("iterations", ctypes.c_int32)]
    assert ctypes.sizeof(N.DavaSgdConfig) == 8
    assert int(re.search(r"#define DAVA_ABI_VERSION (\d+)", text).group(1)) == 4  # additive
    # the learning rate crosses the ABI rounded to float32, as the kernel uses it
    assert N.DavaSgdConfig(1e-4, 1).learning_rate == float(np.float32(1e-4))


def test_operators_are_registered_with_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from deep_attention_visual_odometry_amd import SGDSolver, ReprojectionError, _ops

    for name in ("ba_sgd_solve", "ba_sgd_solve_differentiable", "ba_sgd_backward"):
        assert name in _ops.OPS
        assert getattr(torch.ops.dava, name).default._schema.name == f"dava::{name}"
    with FakeTensorMode():
        dev = "cuda"
        p = _p(2, 17, False)
        x = torch.empty(5, p, device=dev)
        obs = torch.empty(5, 2, 17, 2, device=dev)
        vis = torch.empty(5, 2, 17, dtype=torch.uint8, device=dev)
        xo, errs = torch.ops.dava.ba_sgd_solve(x, obs, vis, 2, 17, False, LR, 7, 0, True)
        assert xo.shape == x.shape and errs.shape == (5, 7) and errs.dtype == torch.float32
        xo, errs = torch.ops.dava.ba_sgd_solve(x, obs, vis, 2, 17, False, LR, 7, 0, False)
        assert xo.shape == x.shape and errs.shape == (0,)
        xo, errs, tape = torch.ops.dava.ba_sgd_solve_differentiable(x, obs, vis, 2, 17, False, LR, 7, 0, True)
        assert xo.shape == x.shape and errs.shape == (5, 7)
        assert tape.shape == (5, 7, (p + 3) // 4 * 4) and tape.dtype == torch.float32
        gx, gobs = torch.ops.dava.ba_sgd_backward(x, tape, obs, vis, 2, 17, False, LR, 7, 0, True)
        assert gx.shape == x.shape and gobs.shape == obs.shape
        gx, gobs = torch.ops.dava.ba_sgd_backward(x, tape, obs, vis, 2, 17, False, LR, 7, 0, False)
        assert gobs.shape == (0,)
        # the differentiable operator is an autograd node w.r.t. x0 and the observations
        xg, og = x.clone().requires_grad_(True), obs.clone().requires_grad_(True)
        xo, _, _ = torch.ops.dava.ba_sgd_solve_differentiable(xg, og, vis, 2, 17, False, LR, 7, 0, False)
        assert xo.requires_grad  # (its backward needs a device: test_gpu_sgd.py)
        xo, _, _ = torch.ops.dava.ba_sgd_solve_differentiable(x, og, vis, 2, 17, False, LR, 7, 0, False)
        assert xo.requires_grad
        # the module's fused forward on fake device tensors (tracing asks the library nothing)
        solver = SGDSolver(LR, 7)
        out = torch.compile(solver, backend="eager", fullgraph=True)(x, ReprojectionError(obs, vis, 2, 17))
        assert out.shape == x.shape


@pytest.mark.parametrize("shape", [C1, C2, C3, C5, (2, 1, False), (2, 257, False)])
@pytest.mark.parametrize("k", [1, 100])
def test_tape_bytes_is_the_documented_formula(lib, shape, k):
    m, n, distortion = shape
    pv = (_p(m, n, distortion) + 3) // 4 * 4
    for b in (1, 7):
        assert lib.dava_ba_sgd_tape_bytes(ctypes.byref(_scene(b, m, n, distortion)), ctypes.byref(_config(k))) \
            == b * k * pv * 4  # no header


def test_size_queries_refuse_what_does_not_fit(lib):
    from deep_attention_visual_odometry_amd import native_ops

    cfg = ctypes.byref(_config(10))
    # x and the gradient alone (2 Pv floats = 480 KB) are beyond both forms
    huge = _scene(2, 2, 20000, False)
    assert lib.dava_ba_sgd_tape_bytes(ctypes.byref(huge), cfg) == 0
    assert lib.dava_ba_sgd_backward_supported(ctypes.byref(huge), cfg) == 0
    assert lib.dava_ba_sgd_solve(ctypes.byref(huge), cfg, None, None, None, None) == 1  # (no data pointers)
    assert not native_ops.sgd_solve_supported(2, 2, 20000, False)
    # the adjoint's image is carve_second's plus the float accumulator: C1-C3 fit 160 KiB, C5 does not
    for m, n, distortion in (C1, C2, C3):
        assert lib.dava_ba_sgd_backward_supported(ctypes.byref(_scene(4, m, n, distortion)), cfg) == 1
        assert native_ops.sgd_backward_supported(4, m, n, distortion, 10)
    m, n, distortion = C5
    assert lib.dava_ba_sgd_tape_bytes(ctypes.byref(_scene(2, m, n, distortion)), cfg) > 0  # the forward runs C5
    assert lib.dava_ba_sgd_backward_supported(ctypes.byref(_scene(2, m, n, distortion)), cfg) == 0
    assert native_ops.sgd_solve_supported(2, m, n, distortion)
    assert not native_ops.sgd_backward_supported(2, m, n, distortion, 10)
    assert lib.dava_ba_sgd_backward(ctypes.byref(_scene(0, m, n, distortion)), cfg, None, 0, None, None, None,
                                    None) == 4
    # invalid scenes and configs answer 0
    for bad in (None, ctypes.byref(_scene(4, 1, 16, False, p=51)), ctypes.byref(_scene(4, 2, 16, False, p=50))):
        assert lib.dava_ba_sgd_tape_bytes(bad, cfg) == 0
        assert lib.dava_ba_sgd_backward_supported(bad, cfg) == 0
    ok = ctypes.byref(_scene(4, 2, 16, False))
    assert lib.dava_ba_sgd_tape_bytes(ok, None) == 0
    assert lib.dava_ba_sgd_tape_bytes(ok, ctypes.byref(_config(-1))) == 0
    assert lib.dava_ba_sgd_backward_supported(ok, ctypes.byref(_config(-1))) == 0


def test_invalid_arguments_are_rejected_without_a_device(lib):
    from deep_attention_visual_odometry_amd import _native as N

    cfg = ctypes.byref(_config())
    solve = lambda sc, c=cfg: lib.dava_ba_sgd_solve(sc, c, None, None, None, None)  # noqa: E731
    record = lambda sc, c=cfg: lib.dava_ba_sgd_solve_record(sc, c, None, None, None, None, 0, None)  # noqa: E731
    backward = lambda sc, c=cfg: lib.dava_ba_sgd_backward(sc, c, None, 0, None, None, None, None)  # noqa: E731
    for call in (solve, record, backward):
        assert call(None) == 1  # null scene
        assert call(ctypes.byref(_scene(4, 1, 16, False, p=51))) == 1  # one view
        assert call(ctypes.byref(_scene(4, 2, 16, False, p=50))) == 1  # wrong P
        assert call(ctypes.byref(_scene(0, 2, 16, False, residual=7))) == 1
        assert call(ctypes.byref(_scene(0, 2, 16, True, residual=N.DAVA_RESIDUAL_RAY_ANGLE))) == 4
        assert call(ctypes.byref(_scene(0, 2, 16, False))) == 0  # batch == 0
        assert call(ctypes.byref(_scene(0, 2, 16, False)), None) == 1  # null config
        assert call(ctypes.byref(_scene(0, 2, 16, False)), ctypes.byref(_config(-1))) == 1
        assert call(ctypes.byref(_scene(4, 2, 16, False))) == 1  # data pointers are required, checked on the host
    # with a scene that has (dummy, never dereferenced) data pointers: null x0 / x_out / cotangents
    buf = (ctypes.c_float * 4)()
    sc = _scene(4, 2, 16, False)
    sc.observations = ctypes.cast(buf, ctypes.c_void_p)
    sc.visibility = ctypes.cast(buf, ctypes.c_void_p)
    assert solve(ctypes.byref(sc)) == 1 and record(ctypes.byref(sc)) == 1 and backward(ctypes.byref(sc)) == 1
    # a recording needs its tape, a backward the recording's: missing or short is a workspace error
    x = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.dava_ba_sgd_solve_record(ctypes.byref(sc), cfg, x, x, None, None, 0, None) == 2
    assert lib.dava_ba_sgd_solve_record(ctypes.byref(sc), cfg, x, x, None, x, 16, None) == 2
    assert lib.dava_ba_sgd_backward(ctypes.byref(sc), cfg, None, 0, x, x, None, None) == 2
    assert lib.dava_ba_sgd_backward(ctypes.byref(sc), cfg, x, 16, x, x, None, None) == 2


def test_operators_refuse_cpu_tensors():
    x = torch.zeros(2, _p(2, 16, False))
    obs = torch.zeros(2, 2, 16, 2)
    vis = torch.ones(2, 2, 16, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        torch.ops.dava.ba_sgd_solve(x, obs, vis, 2, 16, False, LR, 3, 0, False)


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
@pytest.mark.parametrize("k", [1, 5, 20])
def test_cpu_solver_is_bitwise_the_reference(golden, name, k):
    """SGDSolver on CPU tensors with a plain torch closure runs the reference's loop: bitwise the reference's own
    SGDSolver (sgd.npz), and so is the in-test oracle loop every GPU test compares against."""
    from deep_attention_visual_odometry_amd import SGDSolver

    x0, obs, vis, m, n, distortion, ray = _golden_case(golden, name)
    fn = sgd_oracle.closure(obs, vis, m, n, distortion, ray)
    solver = SGDSolver(learning_rate=LR, iterations=k)
    out = solver(x0.clone(), fn)
    assert out.dtype == torch.float32 and not out.requires_grad and solver.last_errors is None
    assert torch.equal(out, torch.tensor(golden[f"{name}_k{k}"]))
    assert torch.equal(sgd_oracle.descend(x0, fn, LR, k), torch.tensor(golden[f"{name}_k{k}"]))


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_cpu_solver_float64(golden, name):
    """float64 on the CPU: the oracle closure and the package's own objective (ReprojectionError / RayAngleError on
    CPU tensors, an ordinary closure there) within 1e-9 of the in-test loop, per row."""
    from deep_attention_visual_odometry_amd import RayAngleError, ReprojectionError, SGDSolver

    x0, obs, vis, m, n, distortion, ray = _golden_case(golden, name)
    x0, obs = x0.double(), obs.double()
    ref = sgd_oracle.descend(x0, sgd_oracle.closure(obs, vis, m, n, distortion, ray), LR, 20)
    solver = SGDSolver(LR, 20)
    out = solver(x0.clone(), sgd_oracle.closure(obs, vis, m, n, distortion, ray))
    assert out.dtype == torch.float64 and sgd_oracle.rows_rel(out, ref).max() <= 1e-9
    fn = RayAngleError(obs, vis, m, n) if ray else ReprojectionError(obs, vis, m, n, distortion)
    out = solver(x0.clone(), fn)
    assert solver.last_errors is None  # the torch loop, not a fused call
    assert out.dtype == torch.float64 and sgd_oracle.rows_rel(out, ref).max() <= 1e-9


def test_cpu_solver_leaves_the_callers_tensor_alone_and_follows_requires_grad(golden):
    from deep_attention_visual_odometry_amd import SGDSolver

    x0, obs, vis, m, n, distortion, ray = _golden_case(golden, "pinhole")
    fn = sgd_oracle.closure(obs.double(), vis, m, n)
    x = x0.double()
    out = SGDSolver(LR, 3)(x, fn)
    assert not out.requires_grad and not x.requires_grad
    xg = x0.double().requires_grad_(True)
    out = SGDSolver(LR, 3)(xg, fn)
    assert out.requires_grad
    assert torch.equal(SGDSolver(LR, 0)(x, fn), x)
    assert SGDSolver(LR, 0)(xg, fn).requires_grad


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_cpu_gradient_through_the_solve(golden, name):
    """With a graph on the CPU the gradient (to x0 and to observations the closure captures) equals autograd's
    through the in-test loop."""
    from deep_attention_visual_odometry_amd import SGDSolver

    x0, obs, vis, m, n, distortion, ray = _golden_case(golden, name)
    k = 6
    w = torch.randn(x0.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    ref, gx_ref, go_ref = sgd_oracle.gradients(x0, obs, vis, m, n, distortion, ray, w, LR, k, torch.float64)
    xg = x0.double().requires_grad_(True)
    og = obs.double().requires_grad_(True)
    out = SGDSolver(LR, k)(xg, sgd_oracle.closure(og, vis, m, n, distortion, ray))
    gx, go = torch.autograd.grad((out * w).sum(), [xg, og])
    assert sgd_oracle.rows_rel(out.detach(), ref).max() <= 1e-12
    assert sgd_oracle.rows_rel(gx, gx_ref).max() <= 1e-12 and sgd_oracle.rows_rel(go, go_ref).max() <= 1e-12
    assert (gx - w).abs().max() > 0  # (the solve's part of dx_K/dx0, not just the identity)


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_objective_without_a_mask_is_the_all_true_mask(golden, name):
    """ReprojectionError(...)(x) -- SGDSolver's one-argument contract -- equals the call with an all-true mask."""
    from deep_attention_visual_odometry_amd import RayAngleError, ReprojectionError

    x0, obs, vis, m, n, distortion, ray = _golden_case(golden, name)
    fn = RayAngleError(obs, vis, m, n) if ray else ReprojectionError(obs, vis, m, n, distortion)
    mask = torch.ones(x0.shape[0], dtype=torch.bool)
    assert torch.equal(fn(x0), fn(x0, mask)) and torch.equal(fn(x0, None), fn(x0, mask))
    oracle = sgd_oracle.closure(obs, vis, m, n, distortion, ray)(x0)
    assert sgd_oracle.rows_rel(fn(x0)[:, None], oracle[:, None]).max() <= 1e-5
