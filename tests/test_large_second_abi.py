"""The float32 dual-number kernels beyond the LDS image -- the second derivatives and the adjoint of the fused
gradient descent in forms 1 and 2 (dava_ba_second_order_form, dava_ba_second_order_large_workspace_bytes,
dava_ba_second_order_large, dava_ba_sgd_backward_form, dava_ba_sgd_backward_large_workspace_bytes,
dava_ba_sgd_backward_large) -- without a GPU: declarations and exports, the form each scene takes, the workspace
formula, the F32_DUAL_FORM override, host refusals that return before a device is touched, the fake kernels and the
opt-in keyword of the objectives."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

NEW_SYMBOLS = ("dava_ba_second_order_form", "dava_ba_second_order_large_workspace_bytes",
               "dava_ba_second_order_large", "dava_ba_sgd_backward_form",
               "dava_ba_sgd_backward_large_workspace_bytes", "dava_ba_sgd_backward_large")
NEW_OPS = ("ba_second_order_large", "ba_sgd_solve_differentiable_large", "ba_sgd_backward_large")
# (M, N, distortion) of the benchmark configurations, and the scenes of the GPU tests
C1, C2, C3, C5 = (2, 64, False), (2, 128, False), (4, 256, True), (16, 4096, False)
FORM1, FORM2, FORM2_BC = (2, 1800, False), (2, 3600, False), (2, 3600, True)
LDS = 160 * 1024
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 2, 4


@pytest.fixture(scope="module")
def lib():
    from deep_attention_visual_odometry_amd import _native

    return _native.load_library()


def _p(m, n, distortion):
    return 3 + 3 * n + 6 * (m - 1) + (5 if distortion else 0)


def _pv(shape):
    return (_p(*shape) + 3) // 4 * 4


def _scene(b, m, n, distortion, residual=0, p=None, data=None):
    from deep_attention_visual_odometry_amd import _native as N

    return N.DavaScene(b, m, n, 1 if distortion else 0, _p(m, n, distortion) if p is None else p, data, data, residual)


def _config(iterations=3, lr=1e-5):
    from deep_attention_visual_odometry_amd import _native as N

    return N.DavaSgdConfig(lr, iterations)


def _second_form(lib, shape, residual=0, b=8):
    return lib.dava_ba_second_order_form(ctypes.byref(_scene(b, *shape, residual=residual)))


def _sgd_form(lib, shape, residual=0, b=8, k=3):
    return lib.dava_ba_sgd_backward_form(ctypes.byref(_scene(b, *shape, residual=residual)), ctypes.byref(_config(k)))


def _workspace(shape, b, form, obs):
    """[dual dE/dobs: B x 4MN floats, only with an observation output | form 2: B x 4 Pv floats | 256-byte tail]"""
    m, n, _ = shape
    return (b * 4 * m * n * 4 if (obs and form != 0) else 0) + (b * 4 * _pv(shape) * 4 if form == 2 else 0) + 256


def test_symbols_are_declared_exported_and_typed(lib):
    from deep_attention_visual_odometry_amd import _native, _ops

    text = open(os.path.join(REPO, "include", "dava_ba.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(dava_[a-z0-9_]+)\s*\(", text)))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert sorted(_native.SIGNATURES) == declared
    sig = _native.SIGNATURES
    scene, cfg = ctypes.POINTER(_native.DavaScene), ctypes.POINTER(_native.DavaSgdConfig)
    assert sig["dava_ba_second_order_form"] == (ctypes.c_int, [scene])
    assert sig["dava_ba_second_order_large_workspace_bytes"] == (ctypes.c_size_t, [scene, ctypes.c_int])
    # the old symbols' arguments with (workspace, workspace_bytes) before the stream
    second = sig["dava_ba_second_order_obs"][1]
    assert sig["dava_ba_second_order_large"] == (ctypes.c_int,
                                                 second[:-1] + [ctypes.c_void_p, ctypes.c_size_t] + second[-1:])
    assert sig["dava_ba_sgd_backward_form"] == (ctypes.c_int, [scene, cfg])
    assert sig["dava_ba_sgd_backward_large_workspace_bytes"] == (ctypes.c_size_t, [scene, cfg, ctypes.c_int])
    back = sig["dava_ba_sgd_backward"][1]
    assert sig["dava_ba_sgd_backward_large"] == (ctypes.c_int,
                                                 back[:-1] + [ctypes.c_void_p, ctypes.c_size_t] + back[-1:])
    for op in NEW_OPS:
        assert op in _ops.OPS and getattr(torch.ops.dava, op).default._schema.name == f"dava::{op}"
    assert lib.dava_abi_version() == 4  # additive
    assert int(re.search(r"#define DAVA_ABI_VERSION (\d+)", text).group(1)) == 4
    assert _native.LIBRARY_KNOBS[-1] == "F32_DUAL_FORM"  # appended


def test_forms_are_chosen_by_fit(lib):
    from deep_attention_visual_odometry_amd import native_ops

    want = {C1: 0, C2: 0, C3: 0, FORM1: 1, FORM2: 2, FORM2_BC: 2, C5: 2}
    for shape, form in want.items():
        assert _second_form(lib, shape) == form, shape
        assert native_ops.second_order_form(8, *shape) == form
        for k in (0, 1, 3, 100):  # the adjoint's image does not depend on the iteration count
            assert _sgd_form(lib, shape, k=k) == form, (shape, k)
        assert native_ops.sgd_backward_form(8, *shape, 3) == form
    # the ray angle shares the images
    assert _second_form(lib, FORM1, residual=1) == 1 and _sgd_form(lib, FORM2, residual=1) == 2
    # C5: 16 Pv bytes of dual x and gradient do not fit (198 KB), so form 2
    assert 16 * _pv(C5) > LDS and 16 * _pv(FORM1) < LDS < 16 * _pv(FORM2)
    # invalid scene or config: minus the status
    assert lib.dava_ba_second_order_form(None) == -INVALID
    assert lib.dava_ba_second_order_form(ctypes.byref(_scene(8, 2, 64, False, p=7))) == -INVALID
    assert _second_form(lib, (2, 16, True), residual=1) == -UNSUPPORTED  # no distorted ray angle
    assert lib.dava_ba_sgd_backward_form(None, ctypes.byref(_config())) == -INVALID
    assert lib.dava_ba_sgd_backward_form(ctypes.byref(_scene(8, *C1)), None) == -INVALID
    assert _sgd_form(lib, C1, k=-1) == -INVALID
    assert lib.dava_ba_sgd_backward_form(ctypes.byref(_scene(8, 2, 64, False, p=7)), ctypes.byref(_config())) == -INVALID
    # where not even form 2's image (the dual view constants and partials) fits
    assert _second_form(lib, (4000, 4, False)) == -UNSUPPORTED and _sgd_form(lib, (4000, 4, False)) == -UNSUPPORTED


@pytest.mark.parametrize("which", ["second", "sgd"])
def test_form_thresholds_at_two_views(lib, which):
    """From the query itself: the largest N at M = 2 that takes form 0 and the largest that takes form 1; N + 1
    takes the next form, and the forms never go back down as N grows."""
    form = (lambda n: _second_form(lib, (2, n, False))) if which == "second" else (
        lambda n: _sgd_form(lib, (2, n, False)))

    def last(f, lo, hi):  # the largest n in [lo, hi) with form(n) <= f (the form is monotone in n)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if form(mid) <= f else (lo, mid)
        return lo

    n0 = last(0, 1, 1 << 14)
    n1 = last(1, n0, 1 << 14)
    assert form(n0) == 0 and form(n0 + 1) == 1
    assert form(n1) == 1 and form(n1 + 1) == 2
    assert 1000 < n0 < 1800 < n1 < 3600
    assert all(form(n) == 0 for n in range(1, n0, 97)) and all(form(n) == 1 for n in range(n0 + 1, n1, 97))
    assert all(form(n) == 2 for n in range(n1 + 1, n1 + 2000, 97))
    # form 1 holds 16 Pv bytes of dual x and gradient (plus the dual view constants, partials and scratch) in LDS
    assert 16 * _pv((2, n1, False)) < LDS < 16 * _pv((2, n1 + 1, False)) + 4096


def test_workspace_sizes_are_the_documented_formula(lib):
    for shape, form in ((FORM1, 1), (FORM2, 2), (FORM2_BC, 2), (C5, 2), (C3, 0)):
        for b in (1, 7):
            sc = ctypes.byref(_scene(b, *shape))
            for obs in (0, 1):
                assert lib.dava_ba_second_order_large_workspace_bytes(sc, obs) == _workspace(shape, b, form, obs), (
                    shape, b, obs)
                assert lib.dava_ba_sgd_backward_large_workspace_bytes(sc, ctypes.byref(_config()), obs) \
                    == _workspace(shape, b, form, obs), (shape, b, obs)
    # unsupported or invalid: 0
    bad = ctypes.byref(_scene(4, 4000, 4, False))
    assert lib.dava_ba_second_order_large_workspace_bytes(bad, 1) == 0
    assert lib.dava_ba_sgd_backward_large_workspace_bytes(bad, ctypes.byref(_config()), 1) == 0
    assert lib.dava_ba_second_order_large_workspace_bytes(None, 1) == 0
    assert lib.dava_ba_sgd_backward_large_workspace_bytes(ctypes.byref(_scene(4, *C1)), None, 1) == 0
    assert lib.dava_ba_sgd_backward_large_workspace_bytes(ctypes.byref(_scene(4, *C1)), ctypes.byref(_config(-1)), 1) == 0


def test_override_raises_the_form_and_never_lowers_it(lib):
    from deep_attention_visual_odometry_amd import _native

    try:
        for forced in (1, 2):
            with _native.debug_overrides(F32_DUAL_FORM=forced):
                assert _native.library_knob("F32_DUAL_FORM") == forced
                for shape in (C1, C3, (2, 257, False)):
                    assert _second_form(lib, shape) == forced and _sgd_form(lib, shape) == forced
                    sc = ctypes.byref(_scene(4, *shape))
                    assert lib.dava_ba_second_order_large_workspace_bytes(sc, 1) == _workspace(shape, 4, forced, 1)
                assert _second_form(lib, FORM2) == 2 and _sgd_form(lib, C5) == 2  # never lowered
                assert _second_form(lib, FORM1) == forced
            assert _second_form(lib, C1) == 0 and _native.library_knob("F32_DUAL_FORM") == -1
        with _native.debug_overrides(F32_DUAL_FORM=0):  # not a form to raise to: the fit decides
            assert _second_form(lib, C1) == 0 and _sgd_form(lib, FORM1) == 1
        with _native.debug_overrides(F64_FORM=2):  # the float64 override is another one
            assert _second_form(lib, C1) == 0 and _sgd_form(lib, C1) == 0
    finally:
        _native.clear_debug_overrides()


def test_large_entry_points_refuse_on_the_host(lib):
    """Every refusal returns before a device is touched (the data pointers are never dereferenced)."""
    ref, fake = ctypes.byref, ctypes.c_void_p(0x1000)
    for shape, form in ((FORM1, 1), (FORM2, 2)):
        sc, empty, no_data = _scene(3, *shape, data=fake), _scene(0, *shape), _scene(3, *shape)
        second = lambda s, x=fake, og=fake, w=fake, wb=1 << 40: lib.dava_ba_second_order_large(  # noqa: E731
            s, x, None, None, None, None, None, og, None, w, wb, None)
        assert second(None) == INVALID and second(ref(no_data)) == INVALID
        assert second(ref(empty), None, None, None, 0) == OK
        assert second(ref(sc), x=None) == INVALID
        need = lib.dava_ba_second_order_large_workspace_bytes(ref(sc), 1)
        assert need == _workspace(shape, 3, form, 1)
        assert second(ref(sc), w=None) == WORKSPACE and second(ref(sc), wb=0) == WORKSPACE
        assert second(ref(sc), wb=need - 1) == WORKSPACE
        if form == 2:  # without an observation output the vectors still need their slices
            assert second(ref(sc), og=None, w=None) == WORKSPACE
            assert second(ref(sc), og=None, wb=lib.dava_ba_second_order_large_workspace_bytes(ref(sc), 0) - 1) == WORKSPACE
        assert second(ref(_scene(3, 4000, 4, False, data=fake))) == UNSUPPORTED
        # ---- the descent's adjoint ----
        cfg, tape = _config(3), 3 * 3 * _pv(shape) * 4
        back = lambda s, c, t=fake, tb=tape, g=fake, gx=fake, go=fake, w=fake, wb=1 << 40: (  # noqa: E731
            lib.dava_ba_sgd_backward_large(s, c, t, tb, g, gx, go, w, wb, None))
        assert back(None, ref(cfg)) == INVALID and back(ref(sc), None) == INVALID
        assert back(ref(sc), ref(_config(-1))) == INVALID and back(ref(no_data), ref(cfg)) == INVALID
        assert back(ref(empty), ref(cfg), None, 0, None, None, None, None, 0) == OK
        assert back(ref(sc), ref(cfg), g=None) == INVALID and back(ref(sc), ref(cfg), gx=None) == INVALID
        assert back(ref(sc), ref(cfg), t=None) == WORKSPACE and back(ref(sc), ref(cfg), tb=tape - 1) == WORKSPACE
        need = lib.dava_ba_sgd_backward_large_workspace_bytes(ref(sc), ref(cfg), 1)
        assert need == _workspace(shape, 3, form, 1)
        assert back(ref(sc), ref(cfg), w=None) == WORKSPACE and back(ref(sc), ref(cfg), wb=0) == WORKSPACE
        assert back(ref(sc), ref(cfg), wb=need - 1) == WORKSPACE
        assert back(ref(_scene(3, 4000, 4, False, data=fake)), ref(cfg)) == UNSUPPORTED


def test_old_entry_points_are_unchanged(lib):
    from deep_attention_visual_odometry_amd import _native, native_ops

    ref, fake = ctypes.byref, ctypes.c_void_p(0x1000)
    cfg = ref(_config(10))
    assert lib.dava_ba_sgd_backward_supported(ref(_scene(2, *C5)), cfg) == 0
    assert lib.dava_ba_sgd_backward_supported(ref(_scene(2, *FORM1)), cfg) == 0
    assert lib.dava_ba_sgd_backward_supported(ref(_scene(2, *C3)), cfg) == 1
    assert not native_ops.sgd_backward_supported(2, *C5, 10)
    assert lib.dava_ba_sgd_backward(ref(_scene(2, *C5, data=fake)), cfg, fake, 1 << 40, fake, fake, None,
                                    None) == UNSUPPORTED
    # no data pointers: the scene check answers first, as it does today
    args = (None,) * 9
    assert lib.dava_ba_second_order_obs(ref(_scene(2, *FORM2)), *args) == INVALID
    assert lib.dava_ba_second_order_obs(ref(_scene(2, *FORM2, data=fake)), fake, *args[1:]) == UNSUPPORTED
    assert lib.dava_ba_second_order(ref(_scene(2, *FORM2, data=fake)), fake, *args[2:]) == UNSUPPORTED
    try:  # and they ignore the override: form 0 by fit alone
        with _native.debug_overrides(F32_DUAL_FORM=2):
            assert lib.dava_ba_sgd_backward_supported(ref(_scene(2, *C3)), cfg) == 1
            assert lib.dava_ba_second_order_obs(ref(_scene(0, *C3)), *args) == OK
    finally:
        _native.clear_debug_overrides()


def test_fake_kernels_give_the_kernels_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode

    m, n, _ = FORM2
    with FakeTensorMode():
        dev = "cuda"
        p = _p(*FORM2)
        x = torch.empty(5, p, device=dev)
        obs = torch.empty(5, m, n, 2, device=dev)
        vis = torch.empty(5, m, n, dtype=torch.uint8, device=dev)
        e, g, hv, og, ohv = torch.ops.dava.ba_second_order_large(x, obs, vis, m, n, False, x, 0, True, True, obs)
        assert e.shape == (5,) and g.shape == hv.shape == x.shape and og.shape == ohv.shape == obs.shape
        assert e.dtype == g.dtype == hv.dtype == og.dtype == ohv.dtype == torch.float32
        e, g, hv, og, ohv = torch.ops.dava.ba_second_order_large(x, obs, vis, m, n, False, None, 1, False, True)
        assert hv.shape == (0,) and og.shape == obs.shape and ohv.shape == (0,)
        e, g, hv, og, ohv = torch.ops.dava.ba_second_order_large(x, obs, vis, m, n, False, x, 0, True, False)
        assert hv.shape == x.shape and og.shape == (0,) and ohv.shape == (0,)
        xo, errs, tape = torch.ops.dava.ba_sgd_solve_differentiable_large(x, obs, vis, m, n, False, 1e-5, 7, 0, True)
        assert xo.shape == x.shape and errs.shape == (5, 7) and errs.dtype == torch.float32
        assert tape.shape == (5, 7, (p + 3) // 4 * 4) and tape.dtype == torch.float32
        xo, errs, _ = torch.ops.dava.ba_sgd_solve_differentiable_large(x, obs, vis, m, n, False, 1e-5, 7, 0, False)
        assert errs.shape == (0,)
        gx, gobs = torch.ops.dava.ba_sgd_backward_large(x, tape, obs, vis, m, n, False, 1e-5, 7, 0, True)
        assert gx.shape == x.shape and gobs.shape == obs.shape and gx.dtype == gobs.dtype == torch.float32
        gx, gobs = torch.ops.dava.ba_sgd_backward_large(x, tape, obs, vis, m, n, False, 1e-5, 7, 0, False)
        assert gobs.shape == (0,)
        # the differentiable operator is an autograd node w.r.t. x0 and the observations
        xg, og = x.clone().requires_grad_(True), obs.clone().requires_grad_(True)
        xo, _, _ = torch.ops.dava.ba_sgd_solve_differentiable_large(xg, og, vis, m, n, False, 1e-5, 7, 0, False)
        assert xo.requires_grad
        xo, _, _ = torch.ops.dava.ba_sgd_solve_differentiable_large(x, og, vis, m, n, False, 1e-5, 7, 0, False)
        assert xo.requires_grad


def test_keyword_constructs_and_changes_nothing_on_cpu_tensors():
    from deep_attention_visual_odometry_amd import RayAngleError, ReprojectionError, SGDSolver, make_scenes

    s = make_scenes(2, 2, 12, seed=5, drop=0.1)
    x, obs, vis = torch.tensor(s.initial), torch.tensor(s.observations), torch.tensor(s.visibility)
    for cls in (ReprojectionError, RayAngleError):
        plain, large = cls(obs, vis, 2, 12), cls(obs, vis, 2, 12, large_derivatives=True)
        assert large.large_derivatives and not plain.large_derivatives
        assert not large.float64_derivatives and not large.float64_large_gradients  # independent keywords
        assert torch.equal(large(x), plain(x))
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        out_a, out_b = SGDSolver(1e-5, 3)(xa, large), SGDSolver(1e-5, 3)(xb, plain)
        assert out_a.requires_grad and torch.equal(out_a, out_b)
        out_a.sum().backward()
        out_b.sum().backward()
        assert torch.equal(xa.grad, xb.grad)
    assert ReprojectionError(obs, vis, 2, 12, distortion=False, large_derivatives=1).large_derivatives is True
