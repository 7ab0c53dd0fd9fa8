"""The float64 entry points (dava_ba_solve_f64, dava_ba_evaluate_f64, the workspace query) without a GPU:
declarations and exports, argument checks that return before a device is touched, the workspace formula,
the fake kernels and the Python layer's refusals."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

F64_SYMBOLS = ("dava_ba_solve_workspace_bytes_f64", "dava_ba_solve_f64", "dava_ba_evaluate_f64")
# (M, N, distortion) of the benchmark configurations
C1, C2, C3, C5 = (2, 64, False), (2, 128, False), (4, 256, True), (16, 4096, False)


@pytest.fixture(scope="module")
def lib():
    from deep_attention_visual_odometry_amd import _native

    return _native.load_library()


def _p(m, n, distortion):
    return 3 + 3 * n + 6 * (m - 1) + (5 if distortion else 0)


def _scene(b, m, n, distortion, residual=0, p=None):
    from deep_attention_visual_odometry_amd import _native as N

    return N.DavaSceneF64(b, m, n, 1 if distortion else 0, _p(m, n, distortion) if p is None else p, None, None,
                          residual)


def _config(iterations=10):
    from deep_attention_visual_odometry_amd import _native as N

    return N.DavaSolverConfigF64(1e-4, 0.9, 1e-4, 1e-8, iterations, 1000, 1)


def test_header_declares_and_library_exports_the_f64_entry_points(lib):
    text = open(os.path.join(REPO, "include", "dava_ba.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dava_[a-z0-9_]+)\s*\(", text))
    for name in F64_SYMBOLS:
        assert name in declared
        assert hasattr(lib, name)
    assert "typedef struct DavaSceneF64" in text and "typedef struct DavaSolverConfigF64" in text
    assert int(re.search(r"#define DAVA_ABI_VERSION (\d+)", text).group(1)) == 4  # additive


def test_f64_structs_mirror_the_header():
    from deep_attention_visual_odometry_amd import _native as N

    assert [f[0] for f in N.DavaSceneF64._fields_] == [f[0] for f in N.DavaScene._fields_]
    assert ctypes.sizeof(N.DavaSceneF64) == ctypes.sizeof(N.DavaScene)
    assert [f for f in N.DavaSolverConfigF64._fields_] == [
        ("sufficient_decrease", ctypes.c_double), ("curvature", ctypes.c_double),
        ("error_threshold", ctypes.c_double), ("minimum_step", ctypes.c_double), ("iterations", ctypes.c_int32),
        ("max_line_search_trials", ctypes.c_int32), ("strong_wolfe", ctypes.c_int32)]
    # thresholds cross the ABI as doubles: 1e-4 stays the reference's 1e-4
    assert N.DavaSolverConfigF64(1e-4, 0.9, 1e-4, 1e-8, 1, 1, 1).sufficient_decrease == 1e-4


def test_invalid_arguments_are_rejected_without_a_device(lib):
    from deep_attention_visual_odometry_amd import _native as N

    cfg = _config()
    solve = lambda sc: lib.dava_ba_solve_f64(sc, ctypes.byref(cfg), None, None, None, None, None, 0, None)  # noqa: E731
    evaluate = lambda sc: lib.dava_ba_evaluate_f64(sc, None, None, None, None, None, None, None)  # noqa: E731
    assert solve(None) == 1 and evaluate(None) == 1  # null scene
    one_view = ctypes.byref(_scene(4, 1, 16, False, p=3 + 48))
    assert solve(one_view) == 1 and evaluate(one_view) == 1
    wrong_p = ctypes.byref(_scene(4, 2, 16, False, p=50))
    assert solve(wrong_p) == 1 and evaluate(wrong_p) == 1
    ray_distorted = ctypes.byref(_scene(0, 2, 16, True, residual=N.DAVA_RESIDUAL_RAY_ANGLE))
    assert solve(ray_distorted) == 4 and evaluate(ray_distorted) == 4
    empty = ctypes.byref(_scene(0, 2, 16, False))
    assert solve(empty) == 0 and evaluate(empty) == 0  # batch == 0
    assert lib.dava_ba_solve_f64(empty, None, None, None, None, None, None, 0, None) == 1  # null config
    # data pointers are required for a non-empty batch, and checked on the host
    assert solve(ctypes.byref(_scene(4, 2, 16, False))) == 1
    for query_scene in (None, one_view, wrong_p, ray_distorted):
        assert lib.dava_ba_solve_workspace_bytes_f64(query_scene, ctypes.byref(cfg)) == 0


@pytest.mark.parametrize("shape", [C1, C2, C3])
@pytest.mark.parametrize("k", [100, 1025])
def test_workspace_query_is_the_documented_formula(lib, shape, k):
    m, n, distortion = shape
    b = 37
    pv = (_p(m, n, distortion) + 3) // 4 * 4
    got = lib.dava_ba_solve_workspace_bytes_f64(ctypes.byref(_scene(b, m, n, distortion)), ctypes.byref(_config(k)))
    assert got == b * 2 * (k - 1) * pv * 8 + 256


def test_workspace_query_is_zero_where_the_solve_does_not_run(lib):
    from deep_attention_visual_odometry_amd import native_ops

    q = lambda shape, k: lib.dava_ba_solve_workspace_bytes_f64(  # noqa: E731
        ctypes.byref(_scene(8, *shape)), ctypes.byref(_config(k)))
    assert q(C5, 100) == 0  # the double LDS image of 16 x 4096 observations does not fit
    assert q(C3, 1026) == 0 and q(C3, 0) == 0
    pv = (_p(*C1) + 3) // 4 * 4
    assert q(C1, 1) == q(C1, 2) == 8 * 2 * pv * 8 + 256  # max(iterations - 1, 1) entries, as in fp32
    assert native_ops.solve_workspace_bytes_f64(8, *C3, iterations=100) == q(C3, 100)


def test_solve_requires_the_workspace_size_the_query_reports(lib):
    """A workspace smaller than the query's figure (the 256-byte tail included) is refused on the host, before
    any launch (the pointers are never dereferenced: the call returns DAVA_ERR_WORKSPACE first)."""
    from deep_attention_visual_odometry_amd import _native as N

    m, n, distortion = C1
    fake = ctypes.c_void_p(0x1000)
    sc = N.DavaSceneF64(4, m, n, 0, _p(m, n, distortion), fake, fake, 0)
    cfg = _config(10)
    need = lib.dava_ba_solve_workspace_bytes_f64(ctypes.byref(sc), ctypes.byref(cfg))
    assert need == 4 * 2 * 9 * ((_p(m, n, distortion) + 3) // 4 * 4) * 8 + 256
    for short in (0, need - 256, need - 1):
        assert lib.dava_ba_solve_f64(ctypes.byref(sc), ctypes.byref(cfg), fake, fake, None, None, fake, short,
                                     None) == 2
    assert lib.dava_ba_solve_f64(ctypes.byref(sc), ctypes.byref(cfg), fake, fake, None, None, None, need, None) == 2


def test_fake_kernels_carry_float64():
    """Under FakeTensorMode the two operators return float64 outputs of the kernels' shapes for float64
    inputs, and the whole drop-in forward on a float64 objective traces, with no GPU and no launch."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    from deep_attention_visual_odometry_amd import BFGSSolver, RayAngleError, ReprojectionError, native_ops

    with FakeTensorMode():
        dev = "cuda"
        x = torch.empty(5, 3 + 3 * 16 + 6, device=dev, dtype=torch.float64)
        obs = torch.empty(5, 2, 16, 2, device=dev, dtype=torch.float64)
        vis = torch.empty(5, 2, 16, dtype=torch.uint8, device=dev)
        ws = torch.empty(0, dtype=torch.uint8, device=dev)
        xo, err, st = torch.ops.dava.ba_solve(x, obs, vis, 2, 16, False, 1e-4, 0.9, -1.0, 7, -1.0, 1000, True, 1, 0,
                                              True, ws)
        assert xo.shape == x.shape and xo.dtype == torch.float64
        assert err.shape == (5,) and err.dtype == torch.float64
        assert st.shape == (5, 4) and st.dtype == torch.int32
        e, g, sl = torch.ops.dava.ba_evaluate(x, obs, vis, 2, 16, False, x, None, True, True, 0)
        assert e.shape == (5,) and g.shape == x.shape and sl.shape == (5,)
        assert e.dtype == g.dtype == sl.dtype == torch.float64
        e, g, sl = torch.ops.dava.ba_evaluate(x, obs, vis, 2, 16, False, None, None, False, False, 1)
        assert e.dtype == torch.float64 and g.shape == (0,) and sl.shape == (0,)
        for cls in (ReprojectionError, RayAngleError):
            fn = cls(obs, vis, 2, 16)
            assert fn.observations.dtype == torch.float32 and fn.observations64.dtype == torch.float64
            solver = BFGSSolver(iterations=7, error_threshold=-1.0, minimum_step=-1.0).eval()
            out = solver(x, fn)
            assert out.shape == x.shape and out.dtype == torch.float64 and out.device.type == "cuda"
            assert solver.last_status.shape == (5, 4)
        # second derivatives stay float32 only
        with pytest.raises(TypeError):
            native_ops.ba_second_order(x, obs, vis, 2, 16)
        with pytest.raises(TypeError):
            BFGSSolver(iterations=7).eval()(x.clone().requires_grad_(True), ReprojectionError(obs, vis, 2, 16))
        # an objective built from float32 observations has no float64 flavour
        with pytest.raises(TypeError):
            BFGSSolver(iterations=7).eval()(x, ReprojectionError(obs.float(), vis, 2, 16))
        with pytest.raises(TypeError):
            ReprojectionError(obs.float(), vis, 2, 16)(x, torch.ones(5, dtype=torch.bool, device=dev))
        assert ReprojectionError(obs.float(), vis, 2, 16).observations64 is None


def test_mixed_dtypes_are_refused_on_the_host():
    from deep_attention_visual_odometry_amd import _ops

    p = 3 + 3 * 16 + 6
    vis = torch.zeros(2, 2, 16, dtype=torch.uint8)
    with pytest.raises(TypeError):  # float32 parameters, float64 observations: as before
        _ops._check_scene_tensors(torch.zeros(2, p), torch.zeros(2, 2, 16, 2, dtype=torch.float64), vis, 2, 16, False)
    with pytest.raises(TypeError):  # and the other way round
        _ops._check_scene_tensors(torch.zeros(2, p, dtype=torch.float64), torch.zeros(2, 2, 16, 2), vis, 2, 16, False)
    with pytest.raises(TypeError):
        _ops._check_scene_tensors(torch.zeros(2, p, dtype=torch.float16),
                                  torch.zeros(2, 2, 16, 2, dtype=torch.float16), vis, 2, 16, False)
    _ops._check_scene_tensors(torch.zeros(2, p, dtype=torch.float64), torch.zeros(2, 2, 16, 2, dtype=torch.float64),
                              vis, 2, 16, False)
    _ops._check_scene_tensors(torch.zeros(2, p), torch.zeros(2, 2, 16, 2), vis, 2, 16, False)


@pytest.mark.parametrize("ray", [False, True])
def test_a_float64_objective_on_cpu_tensors_takes_the_torch_form(ray):
    """CPU tensors never reach a kernel: the float64 objective is the torch form there, like the float32 one."""
    from deep_attention_visual_odometry_amd import RayAngleError, ReprojectionError, make_scenes
    from oracle import objective

    s = make_scenes(3, 2, 16, distortion=False, seed=11)
    x = torch.tensor(s.initial).double()
    obs = torch.tensor(s.observations).double()
    vis = torch.tensor(s.visibility)
    fn = (RayAngleError if ray else ReprojectionError)(obs, vis, 2, 16)
    assert fn.observations64 is None and fn.observations.dtype == torch.float64  # (CPU tensors keep their dtype)
    got = fn(x, torch.ones(3, dtype=torch.bool))
    ref = (objective.ray_angle_error(x, obs, vis, 2, 16) if ray
           else objective.reprojection_error(x, obs, vis, 2, 16))
    assert got.dtype == torch.float64
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=0.0)
