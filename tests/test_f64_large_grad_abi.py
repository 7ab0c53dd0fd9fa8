"""The float64 gradient entry points for scenes beyond the LDS image -- the recording solve, the adjoint and the
second derivatives in forms 1 and 2 (dava_ba_solve_tape_bytes_large_f64,
dava_ba_solve_record_large_workspace_bytes_f64, dava_ba_solve_record_large_f64, dava_ba_solve_backward_form_f64,
dava_ba_solve_backward_large_workspace_bytes_f64, dava_ba_solve_backward_large_f64, dava_ba_second_order_form_f64,
dava_ba_second_order_large_workspace_bytes_f64, dava_ba_second_order_large_f64) -- without a GPU: declarations and
exports, the form each scene takes, the workspace and tape formulas, the F64_FORM override, host refusals that
return before a device is touched, the fake kernels and the opt-in keyword of the objectives."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO
from test_f64_abi import C1, C2, C3, C5, _config, _p, _scene

NEW_SYMBOLS = ("dava_ba_solve_tape_bytes_large_f64", "dava_ba_solve_record_large_workspace_bytes_f64",
               "dava_ba_solve_record_large_f64", "dava_ba_solve_backward_form_f64",
               "dava_ba_solve_backward_large_workspace_bytes_f64", "dava_ba_solve_backward_large_f64",
               "dava_ba_second_order_form_f64", "dava_ba_second_order_large_workspace_bytes_f64",
               "dava_ba_second_order_large_f64",
               "dava_bfgs_update_inverse_hessian_backward_large_workspace_bytes_f64",
               "dava_bfgs_update_inverse_hessian_backward_large_f64")
LDS = 160 * 1024
OBS_IN_OUTPUT = (8, 256, False)  # form 0 with the observation cotangent in the output
ADJ_FORM1 = (12, 400, False)     # P = 1269: the image without the scene is 155,904 B
ADJ_FORM2 = (2, 500, False)      # P = 1509: the 14 vectors alone are 169,344 B; the solve itself is form 0
SOLVE_FORM1 = (6, 700, True)     # the recording takes form 1, the adjoint form 2
SOLVE_FORM2 = (2, 1200, False)   # recording and adjoint both form 2


@pytest.fixture(scope="module")
def lib():
    from deep_attention_visual_odometry_amd import _native

    return _native.load_library()


def _pv(shape):
    return (_p(*shape) + 3) // 4 * 4


def _adjoint_image_bytes(m, n, p, obs_in_lds):
    """carve_adjoint (csrc/adjoint_f64.hpp), as tests/test_gpu_f64_grad.py states it: 14 vectors of Pv doubles, the
    dual view constants and per-wave partials, reduction scratch, a chunk's coefficients, the observations (and
    their cotangent), visibility."""
    pv = (p + 3) // 4 * 4
    doubles = 14 * pv + 2 * 24 * (m - 1) + 2 * 32 * m + 2 * 4 * 32 + 4 * 32 + (4 if obs_in_lds else 2) * m * n
    return 8 * doubles + (m * n + 15) // 16 * 16


def _adjoint_large_image_bytes(m, p, form):
    """carve_adjoint_large: the same image without the scene and, in form 2, without the 14 vectors."""
    pv = (p + 3) // 4 * 4
    return 8 * ((14 * pv if form == 1 else 0) + 2 * 24 * (m - 1) + 2 * 32 * m + 2 * 4 * 32 + 4 * 32)


def _expected_adjoint_form(shape):
    m, n, distortion = shape
    p = _p(*shape)
    if _adjoint_image_bytes(m, n, p, False) <= LDS:
        return 0
    return 1 if _adjoint_large_image_bytes(m, p, 1) <= LDS else 2


def _q(lib, name, shape, k, b=8, residual=0):
    return getattr(lib, name)(ctypes.byref(_scene(b, *shape, residual=residual)), ctypes.byref(_config(k)))


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "dava_ba.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dava_[a-z0-9_]+)\s*\(", text)))


def test_symbols_are_declared_exported_and_typed(lib):
    from deep_attention_visual_odometry_amd import _native, _ops

    declared = _declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert sorted(_native.SIGNATURES) == declared
    sig = _native.SIGNATURES
    assert sig["dava_ba_solve_backward_form_f64"][0] is ctypes.c_int
    assert sig["dava_ba_solve_backward_large_f64"] == sig["dava_ba_solve_backward_f64"]
    assert sig["dava_ba_solve_tape_bytes_large_f64"] == sig["dava_ba_solve_tape_bytes_f64"]
    assert sig["dava_ba_solve_backward_large_workspace_bytes_f64"] == sig["dava_ba_solve_backward_workspace_bytes_f64"]
    # the recording: dava_ba_solve_record_train_f64's arguments with (workspace, workspace_bytes) before the stream
    train = sig["dava_ba_solve_record_train_f64"][1]
    assert sig["dava_ba_solve_record_large_f64"][1] == train[:-1] + [ctypes.c_void_p, ctypes.c_size_t] + train[-1:]
    second = sig["dava_ba_second_order_f64"][1]
    assert sig["dava_ba_second_order_large_f64"][1] == second[:-1] + [ctypes.c_void_p, ctypes.c_size_t] + second[-1:]
    for op in ("ba_second_order_large_f64", "ba_solve_record_large_f64", "ba_solve_backward_large_f64"):
        assert op in _ops.OPS and getattr(torch.ops.dava, op).default._schema.name == f"dava::{op}"
    assert lib.dava_abi_version() == 4  # additive


def test_adjoint_form_is_chosen_by_fit(lib):
    from deep_attention_visual_odometry_amd import native_ops

    # the stated sizes
    assert _adjoint_image_bytes(4, 256, _p(*C3), True) <= LDS
    assert _adjoint_image_bytes(8, 256, _p(*OBS_IN_OUTPUT), True) > LDS >= _adjoint_image_bytes(
        8, 256, _p(*OBS_IN_OUTPUT), False)
    assert _p(*ADJ_FORM1) == 1269 and _adjoint_large_image_bytes(12, 1269, 1) == 155904
    assert _adjoint_image_bytes(12, 400, 1269, False) > LDS
    assert _p(*ADJ_FORM2) == 1509 and 14 * _pv(ADJ_FORM2) * 8 == 169344
    want = {C1: 0, C2: 0, C3: 0, OBS_IN_OUTPUT: 0, ADJ_FORM1: 1, ADJ_FORM2: 2, SOLVE_FORM1: 2, SOLVE_FORM2: 2, C5: 2}
    for shape, form in want.items():
        assert _expected_adjoint_form(shape) == form, shape
        for k in (1, 3, 100, 1025):  # the adjoint's image does not depend on the iteration count
            assert _q(lib, "dava_ba_solve_backward_form_f64", shape, k) == form, (shape, k)
        assert native_ops.backward_form_f64(8, *shape, iterations=3) == form
    # independent of the form the recording takes
    assert _q(lib, "dava_ba_solve_form_f64", ADJ_FORM2, 6) == 0
    assert _q(lib, "dava_ba_solve_form_f64", ADJ_FORM1, 3) == 0
    assert _q(lib, "dava_ba_solve_form_f64", SOLVE_FORM1, 12) == 1
    assert _q(lib, "dava_ba_solve_form_f64", SOLVE_FORM2, 2) == 2
    # the ray angle shares the image
    assert _q(lib, "dava_ba_solve_backward_form_f64", ADJ_FORM2, 3, residual=1) == 2
    # where none runs: minus the status
    assert _q(lib, "dava_ba_solve_backward_form_f64", C3, 0) == -4
    assert _q(lib, "dava_ba_solve_backward_form_f64", C3, 1026) == -4
    assert _q(lib, "dava_ba_solve_backward_form_f64", (2, 16, True), 10, residual=1) == -4
    assert lib.dava_ba_solve_backward_form_f64(None, ctypes.byref(_config(10))) == -1
    assert lib.dava_ba_solve_backward_form_f64(ctypes.byref(_scene(8, *C1)), None) == -1
    # form 2 keeps the dual view constants and partials in LDS: 8 * (112 m + 336) bytes
    assert _adjoint_large_image_bytes(179, 0, 2) <= LDS < _adjoint_large_image_bytes(180, 0, 2)
    assert _q(lib, "dava_ba_solve_backward_form_f64", (179, 4, False), 3) == 2
    assert _q(lib, "dava_ba_solve_backward_form_f64", (180, 4, False), 3) == -4
    assert _q(lib, "dava_ba_solve_backward_large_workspace_bytes_f64", (180, 4, False), 3) == 0


@pytest.mark.parametrize("shape", [C1, C3, OBS_IN_OUTPUT, ADJ_FORM1, ADJ_FORM2, SOLVE_FORM1, SOLVE_FORM2, C5])
@pytest.mark.parametrize("k", [1, 2, 20, 1025])
def test_workspace_and_tape_queries_are_the_documented_formulas(lib, shape, k):
    from deep_attention_visual_odometry_amd import _ops, native_ops

    b, pv = 37, _pv(shape)
    solve_form = _q(lib, "dava_ba_solve_form_f64", shape, k, b)
    adj_form = _q(lib, "dava_ba_solve_backward_form_f64", shape, k, b)
    # the tape: dava_tape.hpp's layout in doubles in every form
    tape = 8 * b * (2 * max(k - 1, 1) * pv + 2 * k * pv + (3 * k + 1 + 3) // 4 * 4) + 256
    assert _q(lib, "dava_ba_solve_tape_bytes_large_f64", shape, k, b) == tape == _ops.tape_bytes_f64(b, _p(*shape), k)
    old_tape = _q(lib, "dava_ba_solve_tape_bytes_f64", shape, k, b)
    assert old_tape == (tape if solve_form == 0 else 0)
    # form 2's six vectors: a workspace of their own
    want = b * 6 * pv * 8 + 256 if solve_form == 2 else 0
    assert _q(lib, "dava_ba_solve_record_large_workspace_bytes_f64", shape, k, b) == want
    # the adjoint: rows a_j, form 2's 14 vectors, the tail
    want = b * k * pv * 8 + (b * 14 * pv * 8 if adj_form == 2 else 0) + 256
    assert _q(lib, "dava_ba_solve_backward_large_workspace_bytes_f64", shape, k, b) == want
    old = _q(lib, "dava_ba_solve_backward_workspace_bytes_f64", shape, k, b)
    assert old == (want if adj_form == 0 else 0)
    assert native_ops.solve_tape_supported_large_f64(b, *shape, k)
    assert native_ops.solve_tape_supported_f64(b, *shape, k) == (solve_form == 0 and adj_form == 0)


def test_tape_query_is_positive_exactly_where_the_large_solve_runs(lib):
    for shape in (C1, C3, C5, SOLVE_FORM1, SOLVE_FORM2, (251, 4, False), (252, 4, False)):
        for k in (0, 1, 2, 100, 1025, 1026):
            tape = _q(lib, "dava_ba_solve_tape_bytes_large_f64", shape, k)
            assert (tape > 0) == (_q(lib, "dava_ba_solve_large_workspace_bytes_f64", shape, k) > 0), (shape, k)
    assert lib.dava_ba_solve_tape_bytes_large_f64(None, ctypes.byref(_config())) == 0
    assert lib.dava_ba_solve_tape_bytes_large_f64(ctypes.byref(_scene(8, *C1)), None) == 0
    assert lib.dava_ba_solve_record_large_workspace_bytes_f64(None, ctypes.byref(_config())) == 0


def test_the_override_raises_the_adjoint_form_and_never_lowers_it(lib):
    from deep_attention_visual_odometry_amd import _native

    natural = {C1: 0, OBS_IN_OUTPUT: 0, ADJ_FORM1: 1, ADJ_FORM2: 2, C5: 2}
    try:
        for forced in (1, 2):
            with _native.debug_overrides(F64_FORM=forced):
                for shape, form in natural.items():
                    assert _q(lib, "dava_ba_solve_backward_form_f64", shape, 12) == max(form, forced), shape
                    assert lib.dava_ba_second_order_form_f64(ctypes.byref(_scene(8, *shape))) >= forced
                b, pv = 37, _pv(C1)
                vectors = b * 14 * pv * 8 if forced == 2 else 0
                assert _q(lib, "dava_ba_solve_backward_large_workspace_bytes_f64", C1, 12, b) == (
                    b * 12 * pv * 8 + vectors + 256)
                assert _q(lib, "dava_ba_solve_record_large_workspace_bytes_f64", C1, 12, b) == (
                    b * 6 * pv * 8 + 256 if forced == 2 else 0)
                # the old symbols keep ignoring it
                assert _q(lib, "dava_ba_solve_backward_workspace_bytes_f64", C1, 12, b) == b * 12 * pv * 8 + 256
            assert _q(lib, "dava_ba_solve_backward_form_f64", C1, 12) == 0
        with _native.debug_overrides(F64_FORM=0):  # not a form to raise to: the fit decides
            for shape, form in natural.items():
                assert _q(lib, "dava_ba_solve_backward_form_f64", shape, 12) == form
    finally:
        _native.clear_debug_overrides()
    assert _q(lib, "dava_ba_solve_backward_form_f64", C1, 12) == 0


def test_second_order_form_and_workspace(lib):
    from deep_attention_visual_odometry_amd import native_ops

    form = lambda shape, residual=0: lib.dava_ba_second_order_form_f64(  # noqa: E731
        ctypes.byref(_scene(8, *shape, residual=residual)))
    size = lambda shape, obs, b=37: lib.dava_ba_second_order_large_workspace_bytes_f64(  # noqa: E731
        ctypes.byref(_scene(b, *shape)), obs)
    for shape in (C1, C2, C3):
        assert form(shape) == 0 and size(shape, 1) == size(shape, 0) == 256
    # the dual x and gradient (4 Pv doubles) fit LDS without the scene ...
    for shape in (SOLVE_FORM1, SOLVE_FORM2, ADJ_FORM1):
        m, n, _ = shape
        assert form(shape) == 1 and native_ops.second_order_form_f64(8, *shape) == 1
        assert size(shape, 1) == 37 * 4 * m * n * 8 + 256 and size(shape, 0) == 256
    # ... and not at C5 (P = 12381: 396 KB)
    assert form(C5) == 2
    assert size(C5, 1) == 37 * (4 * 16 * 4096 + 4 * _pv(C5)) * 8 + 256
    assert size(C5, 0) == 37 * 4 * _pv(C5) * 8 + 256
    assert form((2, 16, True), residual=1) == -4 and lib.dava_ba_second_order_form_f64(None) == -1
    assert lib.dava_ba_second_order_large_workspace_bytes_f64(None, 1) == 0
    # form 2 keeps the dual view constants and partials in LDS, 8 * (112 m + 208) bytes: 181 views fit
    assert form((181, 4, False)) == 2 and form((182, 4, False)) == -4
    assert size((182, 4, False), 1) == 0


def test_the_old_symbols_still_refuse_scenes_beyond_the_lds_image(lib):
    from deep_attention_visual_odometry_amd import _native as N

    fake = ctypes.c_void_p(0x1000)
    for shape in (SOLVE_FORM2, C5):
        assert _q(lib, "dava_ba_solve_tape_bytes_f64", shape, 12) == 0
        assert _q(lib, "dava_ba_solve_backward_workspace_bytes_f64", shape, 12) == 0
        m, n, distortion = shape
        sc = N.DavaSceneF64(4, m, n, 0, _p(*shape), fake, fake, 0)
        cfg = _config(12)
        assert lib.dava_ba_solve_record_f64(ctypes.byref(sc), ctypes.byref(cfg), fake, fake, None, fake, fake, 1 << 40,
                                            None) == 4
        assert lib.dava_ba_solve_backward_f64(ctypes.byref(sc), ctypes.byref(cfg), fake, 1 << 40, fake, fake, fake, None,
                                              fake, 1 << 40, None) == 4
        assert lib.dava_ba_second_order_f64(ctypes.byref(sc), fake, None, None, None, None, None, None, None,
                                            None) == 4
    # (2, 500): the solve records in form 0, the old adjoint refuses
    assert _q(lib, "dava_ba_solve_tape_bytes_f64", ADJ_FORM2, 6) > 0
    assert _q(lib, "dava_ba_solve_backward_workspace_bytes_f64", ADJ_FORM2, 6) == 0


@pytest.mark.parametrize("shape,k", [(ADJ_FORM1, 10), (ADJ_FORM2, 10), (SOLVE_FORM2, 10), (SOLVE_FORM2, 1)])
def test_host_refusals_never_touch_the_pointers(lib, shape, k):
    """Fake pointers throughout: every call returns on the host, before any launch."""
    from deep_attention_visual_odometry_amd import _native as N

    m, n, distortion = shape
    fake = ctypes.c_void_p(0x1000)
    sc = N.DavaSceneF64(4, m, n, 1 if distortion else 0, _p(*shape), fake, fake, 0)
    empty = N.DavaSceneF64(0, m, n, 1 if distortion else 0, _p(*shape), None, None, 0)
    no_data = N.DavaSceneF64(4, m, n, 1 if distortion else 0, _p(*shape), None, None, 0)
    cfg, bad_k, zero_k = _config(k), _config(1026), _config(0)
    ref = ctypes.byref
    # ---- the recording ----
    tape = lib.dava_ba_solve_tape_bytes_large_f64(ref(sc), ref(cfg))
    ws = lib.dava_ba_solve_record_large_workspace_bytes_f64(ref(sc), ref(cfg))
    form = lib.dava_ba_solve_form_f64(ref(sc), ref(cfg))
    record = lambda s, c, x0=fake, st=fake, t=fake, tb=tape, w=fake, wb=ws: lib.dava_ba_solve_record_large_f64(  # noqa: E731
        s, c, None, x0, fake, None, st, t, tb, w, wb, None)
    assert record(None, ref(cfg)) == 1 and record(ref(sc), None) == 1
    assert record(ref(empty), ref(cfg), None, None, None, 0, None, 0) == 0  # batch 0: nothing is looked at
    assert record(ref(sc), ref(cfg), x0=None) == 1 and record(ref(no_data), ref(cfg)) == 1
    assert record(ref(sc), ref(cfg), st=None) == 1  # a recording needs the status words
    assert record(ref(sc), ref(bad_k)) == 4 and record(ref(sc), ref(zero_k)) == 4
    if form != 0:
        assert record(ref(sc), ref(cfg), t=None) == 2 and record(ref(sc), ref(cfg), tb=tape - 1) == 2
    if form == 2:
        assert ws > 256
        for short in (ws - 1, ws - 256, 0):
            assert record(ref(sc), ref(cfg), wb=short) == 2
        assert record(ref(sc), ref(cfg), w=None) == 2
    # ---- the adjoint ----
    need = lib.dava_ba_solve_backward_large_workspace_bytes_f64(ref(sc), ref(cfg))
    adj_form = lib.dava_ba_solve_backward_form_f64(ref(sc), ref(cfg))
    assert adj_form in (1, 2) and need > 256
    backward = lambda s, c, t=fake, tb=tape, st=fake, g=fake, gx=fake, w=fake, wb=need: (  # noqa: E731
        lib.dava_ba_solve_backward_large_f64(s, c, t, tb, st, g, gx, None, w, wb, None))
    assert backward(None, ref(cfg)) == 1 and backward(ref(sc), None) == 1
    assert backward(ref(empty), ref(cfg), None, 0, None, None, None, None, 0) == 0
    assert backward(ref(sc), ref(bad_k)) == 4 and backward(ref(sc), ref(zero_k)) == 4
    assert backward(ref(no_data), ref(cfg)) == 1
    for missing in ("t", "st", "g", "gx"):
        assert backward(ref(sc), ref(cfg), **{missing: None}) == 1
    assert backward(ref(sc), ref(cfg), tb=tape - 257) == 2  # short tape (its tail is not read)
    assert backward(ref(sc), ref(cfg), w=None) == 2 and backward(ref(sc), ref(cfg), wb=0) == 2
    assert backward(ref(sc), ref(cfg), wb=need - 257) == 2  # short by one byte of the rows / vectors
    # ---- the second derivatives ----
    second = lambda s, x=fake, og=fake, w=fake, wb=1 << 40: lib.dava_ba_second_order_large_f64(  # noqa: E731
        s, x, None, None, None, None, None, og, None, w, wb, None)
    assert second(None) == 1 and second(ref(no_data)) == 1 and second(ref(empty), None, None, None, 0) == 0
    assert second(ref(sc), x=None) == 1
    sneed = lib.dava_ba_second_order_large_workspace_bytes_f64(ref(sc), 1)
    if lib.dava_ba_second_order_form_f64(ref(sc)) == 1:  # ((2, 500) keeps its dual image in LDS: form 0, no workspace)
        assert sneed == 4 * 4 * m * n * 8 + 256
        assert second(ref(sc), w=None) == 2 and second(ref(sc), wb=sneed - 1) == 2 and second(ref(sc), wb=0) == 2
    else:
        assert shape == ADJ_FORM2 and sneed == 256


def test_fake_kernels_and_the_keyword():
    """Under FakeTensorMode the three operators return the kernels' shapes in float64 on a (2, 1200) scene; the
    keyword needs float64_derivatives=True, and without it the drop-in solver refuses parameters that require grad
    as it does today (with it the recording launch runs: tests/test_gpu_f64_large_grad.py)."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    from deep_attention_visual_odometry_amd import BFGSSolver, RayAngleError, ReprojectionError, _ops

    m, n, _ = SOLVE_FORM2
    with FakeTensorMode():
        dev = "cuda"
        x = torch.empty(5, _p(*SOLVE_FORM2), device=dev, dtype=torch.float64)
        obs = torch.empty(5, m, n, 2, device=dev, dtype=torch.float64)
        vis = torch.empty(5, m, n, dtype=torch.uint8, device=dev)
        e, g, hv, og, ohv = torch.ops.dava.ba_second_order_large_f64(x, obs, vis, m, n, False, x, 0, True, True, obs)
        assert e.shape == (5,) and g.shape == hv.shape == x.shape and og.shape == ohv.shape == obs.shape
        assert e.dtype == g.dtype == hv.dtype == og.dtype == ohv.dtype == torch.float64
        e, g, hv, og, ohv = torch.ops.dava.ba_second_order_large_f64(x, obs, vis, m, n, False, None, 1, False, True)
        assert hv.shape == (0,) and og.shape == obs.shape and ohv.shape == (0,)
        xo, st, tape, err = torch.ops.dava.ba_solve_record_large_f64(x, obs, vis, m, n, False, 1e-4, 0.9, -1.0, 7,
                                                                     -1.0, 1000, True, 0, True)
        assert xo.shape == x.shape and xo.dtype == torch.float64 and err.shape == (5,)
        assert st.shape == (5, 4) and st.dtype == torch.int32
        assert tape.dtype == torch.uint8 and tape.shape == (_ops.tape_bytes_f64(5, x.shape[1], 7),)
        gx, go = torch.ops.dava.ba_solve_backward_large_f64(x, tape, st, obs, vis, m, n, False, 7, 0, True)
        assert gx.shape == x.shape and go.shape == obs.shape and gx.dtype == go.dtype == torch.float64
        gx, go = torch.ops.dava.ba_solve_backward_large_f64(x, tape, st, obs, vis, m, n, False, 7, 0, False)
        assert go.shape == (0,)
        for cls in (ReprojectionError, RayAngleError):
            fn = cls(obs, vis, m, n, float64_derivatives=True, float64_large_gradients=True)
            assert fn.float64_large_gradients and fn.float64_derivatives
            solver = BFGSSolver(iterations=7, error_threshold=-1.0, minimum_step=-1.0).eval()
            out = solver(x, fn)  # without a graph the solve is no node: the plain float64 launch, as before
            assert out.shape == x.shape and out.dtype == torch.float64 and not out.requires_grad
            assert solver.last_status is not None and solver.last_status.shape == (5, 4)
            # without the keyword: the refusal it has today
            with pytest.raises(ValueError, match="160 KiB"):
                solver(x.clone().requires_grad_(True), cls(obs, vis, m, n, float64_derivatives=True))
            with pytest.raises(ValueError, match="float64_derivatives"):
                cls(obs, vis, m, n, float64_large_gradients=True)
            assert not cls(obs, vis, m, n).float64_large_gradients


def test_update_backward_large_query_and_host_refusals(lib):
    """The dense update's float64 backward beyond its LDS image (9 vectors of n doubles, 150 KiB: n <= 2133): the
    workspace query is 0 where the LDS launch is taken, and every refusal returns on the host."""
    from deep_attention_visual_odometry_amd import _native

    q = lib.dava_bfgs_update_inverse_hessian_backward_large_workspace_bytes_f64
    assert 9 * 2133 * 8 <= 150 * 1024 < 9 * 2134 * 8
    assert q(5, 2133) == 0 and q(5, 24) == 0
    assert q(5, 2134) == 5 * 9 * 2134 * 8 + 256 and q(2, 3609) == 2 * 9 * 3609 * 8 + 256
    assert q(0, 3609) == 0 and q(5, 0) == 0 and q(-1, 3609) == 0
    try:
        for forced in (1, 2):
            with _native.debug_overrides(F64_FORM=forced):
                assert q(5, 24) == 5 * 9 * 24 * 8 + 256
        with _native.debug_overrides(F64_FORM=0):
            assert q(5, 24) == 0
    finally:
        _native.clear_debug_overrides()
    fake = ctypes.c_void_p(0x1000)
    call = lambda b, n, h=fake, s=fake, y=fake, g=fake, ws=fake, size=1 << 40: (  # noqa: E731
        lib.dava_bfgs_update_inverse_hessian_backward_large_f64(b, n, h, s, y, g, None, None, None, ws, size, None))
    assert call(-1, 3609) == 1 and call(2, -1) == 1
    assert call(0, 3609, None, None, None, None, None, 0) == 0 and call(2, 0, None, None, None, None, None, 0) == 0
    for missing in ("h", "s", "y", "g"):
        assert call(2, 3609, **{missing: None}) == 1
    need = q(2, 3609)
    assert call(2, 3609, ws=None) == 2 and call(2, 3609, size=need - 1) == 2 and call(2, 3609, size=0) == 2
    # the old symbol keeps its limit
    assert lib.dava_bfgs_update_inverse_hessian_backward_f64(2, 3609, fake, fake, fake, fake, None, None, None,
                                                             None) == 4
