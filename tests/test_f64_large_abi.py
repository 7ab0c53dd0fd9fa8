"""The float64 entry points for scenes beyond the LDS image (dava_ba_solve_form_f64,
dava_ba_solve_large_workspace_bytes_f64, dava_ba_solve_large_f64, dava_ba_evaluate_large_f64) without a GPU:
declarations and exports, the form a scene takes, the workspace formula of each form, the F64_FORM override,
host refusals that return before a device is touched, and the drop-in forward under FakeTensorMode."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO
from test_f64_abi import C1, C2, C3, C5, _config, _p, _scene

LARGE_SYMBOLS = ("dava_ba_solve_form_f64", "dava_ba_solve_large_workspace_bytes_f64", "dava_ba_solve_large_f64",
                 "dava_ba_evaluate_large_f64")
FORM1 = (6, 700, True)    # P = 2138: the six vectors fit LDS, not with the scene beside them
FORM2 = (2, 1200, False)  # P = 3609: the six vectors alone are 169 KiB


@pytest.fixture(scope="module")
def lib():
    from deep_attention_visual_odometry_amd import _native

    return _native.load_library()


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "dava_ba.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dava_[a-z0-9_]+)\s*\(", text)))


def _form(lib, shape, k, b=8, residual=0, p=None):
    m, n, distortion = shape
    return lib.dava_ba_solve_form_f64(ctypes.byref(_scene(b, m, n, distortion, residual, p)), ctypes.byref(_config(k)))


def _large_bytes(lib, shape, k, b):
    return lib.dava_ba_solve_large_workspace_bytes_f64(ctypes.byref(_scene(b, *shape)), ctypes.byref(_config(k)))


def _pv(shape):
    return (_p(*shape) + 3) // 4 * 4


def test_symbols_are_declared_exported_and_typed(lib):
    from deep_attention_visual_odometry_amd import _native

    declared = _declared_symbols()
    for name in LARGE_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name)
    assert sorted(_native.SIGNATURES) == declared
    assert _native.SIGNATURES["dava_ba_solve_form_f64"][0] is ctypes.c_int
    assert _native.SIGNATURES["dava_ba_solve_large_workspace_bytes_f64"][0] is ctypes.c_size_t
    assert _native.SIGNATURES["dava_ba_solve_large_f64"] == (
        ctypes.c_int, _native.SIGNATURES["dava_ba_solve_train_f64"][1])
    assert _native.SIGNATURES["dava_ba_evaluate_large_f64"] == _native.SIGNATURES["dava_ba_evaluate_f64"]
    assert "F64_FORM" in _native.LIBRARY_KNOBS
    assert lib.dava_abi_version() == 4  # additive


def test_form_is_chosen_by_fit(lib):
    from deep_attention_visual_odometry_amd import _native, native_ops

    for shape in (C1, C2, C3):
        assert _form(lib, shape, 100) == 0
    assert _form(lib, C5, 100) == 2
    assert _form(lib, FORM1, 12) == 1
    assert _form(lib, FORM2, 12) == 2
    assert native_ops.solve_form_f64(8, *FORM1, iterations=12) == 1
    # where no form runs: the iteration count, an invalid scene, ray angle with distortion
    assert _form(lib, C3, 0) < 0 and _form(lib, C3, 1026) < 0
    assert _form(lib, (1, 16, False), 10, p=3 + 48) < 0
    assert _form(lib, (2, 16, False), 10, p=50) < 0
    assert _form(lib, (2, 16, True), 10, residual=_native.DAVA_RESIDUAL_RAY_ANGLE) < 0
    assert lib.dava_ba_solve_form_f64(None, ctypes.byref(_config(10))) < 0
    assert lib.dava_ba_solve_form_f64(ctypes.byref(_scene(8, *C1)), None) < 0
    # form 2 keeps the view constants and 6 x 1024 history scalars in LDS: 251 views fit at 1025 iterations
    assert _form(lib, (251, 4, False), 1025) == 2 and _form(lib, (252, 4, False), 1025) < 0


def test_the_override_raises_the_form_and_never_lowers_it(lib):
    from deep_attention_visual_odometry_amd import _native

    try:
        for forced in (1, 2):
            with _native.debug_overrides(F64_FORM=forced):
                assert _native.library_knob("F64_FORM") == forced
                assert _form(lib, C1, 100) == forced
                assert _form(lib, C5, 100) == 2
                assert _form(lib, FORM1, 12) == max(forced, 1)
                # the queries reflect it
                vectors = 37 * 6 * _pv(C1) * 8 if forced == 2 else 0
                assert _large_bytes(lib, C1, 100, 37) == 37 * 2 * 99 * _pv(C1) * 8 + vectors + 256
            assert _form(lib, C1, 100) == 0 and _native.library_knob("F64_FORM") == -1
        with _native.debug_overrides(F64_FORM=0):  # not a form to raise to: the fit decides
            assert _form(lib, C1, 100) == 0 and _form(lib, C5, 100) == 2
    finally:
        _native.clear_debug_overrides()
    assert _form(lib, C1, 100) == 0


@pytest.mark.parametrize("shape,k,form", [(C1, 100, 0), (C3, 1025, 0), (FORM1, 12, 1), (FORM2, 12, 2), (C5, 100, 2),
                                          (C5, 1025, 2)])
def test_workspace_query_is_the_documented_formula(lib, shape, k, form):
    from deep_attention_visual_odometry_amd import native_ops

    b, pv = 37, _pv(shape)
    assert _form(lib, shape, k, b) == form
    want = b * 2 * max(k - 1, 1) * pv * 8 + (b * 6 * pv * 8 if form == 2 else 0) + 256
    assert _large_bytes(lib, shape, k, b) == want
    assert native_ops.solve_large_workspace_bytes_f64(b, *shape, iterations=k) == want
    old = lib.dava_ba_solve_workspace_bytes_f64(ctypes.byref(_scene(b, *shape)), ctypes.byref(_config(k)))
    assert old == (want if form == 0 else 0)  # form 0: the old query's figure; beyond it the old symbols refuse


def test_workspace_query_edges(lib):
    assert _large_bytes(lib, C1, 1, 37) == _large_bytes(lib, C1, 2, 37) == 37 * 2 * _pv(C1) * 8 + 256
    assert _large_bytes(lib, FORM2, 1, 37) == _large_bytes(lib, FORM2, 2, 37) == 37 * 8 * _pv(FORM2) * 8 + 256
    assert _large_bytes(lib, C3, 0, 37) == 0 and _large_bytes(lib, C5, 1026, 37) == 0
    assert lib.dava_ba_solve_large_workspace_bytes_f64(None, ctypes.byref(_config(10))) == 0
    assert lib.dava_ba_solve_large_workspace_bytes_f64(ctypes.byref(_scene(8, *C5)), None) == 0
    # the old symbols still refuse C5 (test_f64_abi.py pins the rest)
    assert lib.dava_ba_solve_workspace_bytes_f64(ctypes.byref(_scene(8, *C5)), ctypes.byref(_config(100))) == 0


@pytest.mark.parametrize("shape,k", [(C1, 10), (FORM1, 10), (FORM2, 10), (FORM2, 1)])
def test_host_refusals_never_touch_the_pointers(lib, shape, k):
    """Fake pointers throughout: every call returns on the host, before any launch."""
    from deep_attention_visual_odometry_amd import _native as N

    m, n, distortion = shape
    fake = ctypes.c_void_p(0x1000)
    sc = N.DavaSceneF64(4, m, n, 1 if distortion else 0, _p(*shape), fake, fake, 0)
    cfg = _config(k)
    solve = lambda s, c, x0, ws, size, tr=None: lib.dava_ba_solve_large_f64(  # noqa: E731
        s, c, tr, x0, fake, None, None, ws, size, None)
    assert solve(None, ctypes.byref(cfg), fake, fake, 1 << 40) == 1  # null scene
    assert solve(ctypes.byref(sc), None, fake, fake, 1 << 40) == 1  # null config
    empty = N.DavaSceneF64(0, m, n, 1 if distortion else 0, _p(*shape), None, None, 0)
    assert solve(ctypes.byref(empty), ctypes.byref(cfg), None, None, 0) == 0  # batch == 0, before the pointer checks
    assert solve(ctypes.byref(empty), None, None, None, 0) == 1  # ... but after the config's
    assert solve(ctypes.byref(sc), ctypes.byref(cfg), None, fake, 1 << 40) == 1  # missing x0
    no_data = N.DavaSceneF64(4, m, n, 1 if distortion else 0, _p(*shape), None, None, 0)
    assert solve(ctypes.byref(no_data), ctypes.byref(cfg), fake, fake, 1 << 40) == 1
    bad_p = N.DavaTrainingF64(1.5, 0, 0, 0)
    assert solve(None, None, None, None, 0, ctypes.byref(bad_p)) == 1  # checked before anything else
    need = lib.dava_ba_solve_large_workspace_bytes_f64(ctypes.byref(sc), ctypes.byref(cfg))
    assert need > 256
    form = lib.dava_ba_solve_form_f64(ctypes.byref(sc), ctypes.byref(cfg))
    if k > 1 or form == 2:  # a workspace is needed: short by 1 byte, by the tail, or missing
        for short in (need - 1, need - 256, 0):
            assert solve(ctypes.byref(sc), ctypes.byref(cfg), fake, fake, short) == 2
        assert solve(ctypes.byref(sc), ctypes.byref(cfg), fake, None, need) == 2
    too_long = _config(1026)
    assert solve(ctypes.byref(sc), ctypes.byref(too_long), fake, fake, 1 << 40) == 4
    assert solve(ctypes.byref(sc), ctypes.byref(too_long), None, fake, 1 << 40) == 1  # invalid before unsupported
    # the evaluation: the same refusals as dava_ba_evaluate_f64
    evaluate = lambda s, x, d=None, e=fake, sl=None: lib.dava_ba_evaluate_large_f64(  # noqa: E731
        s, x, d, None, e, None, sl, None)
    assert evaluate(None, fake) == 1 and evaluate(ctypes.byref(no_data), fake) == 1
    assert evaluate(ctypes.byref(empty), None) == 0
    assert evaluate(ctypes.byref(sc), None) == 1 and evaluate(ctypes.byref(sc), fake, e=None) == 1
    assert evaluate(ctypes.byref(sc), fake, sl=fake) == 1  # a slope needs a direction
    ray_distorted = N.DavaSceneF64(0, 2, 16, 1, _p(2, 16, True), None, None, N.DAVA_RESIDUAL_RAY_ANGLE)
    assert evaluate(ctypes.byref(ray_distorted), None) == 4
    assert solve(ctypes.byref(ray_distorted), ctypes.byref(cfg), None, None, 0) == 4


def test_drop_in_forward_traces_on_a_scene_beyond_the_lds_image():
    """Under FakeTensorMode the drop-in forward on a (2, 1200) float64 objective -- form 2; refused before this
    entry existed -- traces and returns float64 of the right shape; parameters that require grad are refused with
    the limit named, before any launch."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    from deep_attention_visual_odometry_amd import BFGSSolver, RayAngleError, ReprojectionError, native_ops

    m, n, _ = FORM2
    assert native_ops.solve_workspace_bytes_f64(5, m, n, False, iterations=7) == 0
    assert native_ops.solve_form_f64(5, m, n, False, iterations=7) == 2
    with FakeTensorMode():
        dev = "cuda"
        x = torch.empty(5, _p(*FORM2), device=dev, dtype=torch.float64)
        obs = torch.empty(5, m, n, 2, device=dev, dtype=torch.float64)
        vis = torch.empty(5, m, n, dtype=torch.uint8, device=dev)
        for cls in (ReprojectionError, RayAngleError):
            solver = BFGSSolver(iterations=7, error_threshold=-1.0, minimum_step=-1.0).eval()
            out = solver(x, cls(obs, vis, m, n))
            assert out.shape == x.shape and out.dtype == torch.float64 and out.device.type == "cuda"
            assert solver.last_status.shape == (5, 4) and solver.last_status.dtype == torch.int32
        fn = ReprojectionError(obs, vis, m, n, float64_derivatives=True)
        with pytest.raises(ValueError, match="160 KiB"):
            BFGSSolver(iterations=7).eval()(x.clone().requires_grad_(True), fn)
        with pytest.raises(TypeError):  # (without the float64 derivatives: as on every scene)
            BFGSSolver(iterations=7).eval()(x.clone().requires_grad_(True), ReprojectionError(obs, vis, m, n))
