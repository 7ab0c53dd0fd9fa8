"""Training mode of the float64 fused solve (DavaTrainingF64, dava_ba_solve_train_f64,
dava_ba_solve_record_train_f64) without a GPU: declarations, exports and ctypes mirrors, the host-side argument
checks, the fake kernels of the extended operators and the unchanged refusals, in the manner of test_f64_grad_abi.py."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

NEW_SYMBOLS = ("dava_ba_solve_train_f64", "dava_ba_solve_record_train_f64")
C1, C5 = (2, 64, False), (16, 4096, False)  # (M, N, distortion) of two benchmark configurations


@pytest.fixture(scope="module")
def lib():
    from deep_attention_visual_odometry_amd import _native

    return _native.load_library()


def _p(m, n, distortion):
    return 3 + 3 * n + 6 * (m - 1) + (5 if distortion else 0)


def _header():
    text = open(os.path.join(REPO, "include", "dava_ba.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_struct_and_entry_points_are_declared_exported_and_mirrored(lib):
    from deep_attention_visual_odometry_amd import _native as N

    text = _header()
    declared = set(re.findall(r"\b(dava_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in N.SIGNATURES
        res, args = N.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == 10  # the eval entry point's nine and the training struct
        assert args[2]._type_ is N.DavaTrainingF64 and args[:2] == N.SIGNATURES[name.replace("_train", "")][1][:2]
        assert args[3:] == N.SIGNATURES[name.replace("_train", "")][1][2:]
    assert int(re.search(r"#define DAVA_ABI_VERSION (\d+)", text).group(1)) == 4  # additive
    assert N.ABI_VERSION == 4 and lib.dava_abi_version() == 4
    # the struct, field by field
    body = re.search(r"typedef struct DavaTrainingF64 \{(.*?)\} DavaTrainingF64;", text, re.S).group(1)
    ctype = {"float": ctypes.c_float, "uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32}
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        fields += [(name, ctype[words[0]]) for name in words[1:]]
    assert fields == [("drop_path_p", ctypes.c_float), ("drop_seed_lo", ctypes.c_uint32),
                      ("drop_seed_hi", ctypes.c_uint32), ("return_second_last", ctypes.c_int32)]
    assert N.DavaTrainingF64._fields_ == fields and ctypes.sizeof(N.DavaTrainingF64) == 16
    # DavaSolverConfigF64 is not touched: the training fields live in the new struct only
    assert [f for f, _ in N.DavaSolverConfigF64._fields_] == [
        "sufficient_decrease", "curvature", "error_threshold", "minimum_step", "iterations",
        "max_line_search_trials", "strong_wolfe"]


def test_training_struct_helper_splits_the_seed():
    from deep_attention_visual_odometry_amd import _ops

    t = _ops.training_f64(0.25, (7 << 32) | 5, True)
    assert (t.drop_path_p, t.drop_seed_lo, t.drop_seed_hi, t.return_second_last) == (0.25, 5, 7, 1)
    t = _ops.training_f64()
    assert (t.drop_path_p, t.drop_seed_lo, t.drop_seed_hi, t.return_second_last) == (0.0, 0, 0, 0)


def test_arguments_are_checked_on_the_host(lib):
    from deep_attention_visual_odometry_amd import _native as N

    cfg = N.DavaSolverConfigF64(1e-4, 0.9, 1e-4, 1e-8, 10, 1000, 1)
    fake = ctypes.c_void_p(0x1000)
    nowhere = N.DavaSceneF64(4, 2, 64, 0, _p(*C1), None, None, 0)
    pointed = N.DavaSceneF64(4, 2, 64, 0, _p(*C1), fake, fake, 0)
    big = N.DavaSceneF64(1, 16, 4096, 0, _p(*C5), fake, fake, 0)
    empty = N.DavaSceneF64(0, 2, 64, 0, _p(*C1), None, None, 0)
    sc_cfg = (ctypes.byref(pointed), ctypes.byref(cfg))
    need = {"dava_ba_solve_train_f64": lib.dava_ba_solve_workspace_bytes_f64(*sc_cfg),
            "dava_ba_solve_record_train_f64": lib.dava_ba_solve_tape_bytes_f64(*sc_cfg)}
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        for p in (-0.1, 1.5, float("nan")):  # refused before anything else: null device pointers, even batch == 0
            tr = ctypes.byref(N.DavaTrainingF64(p, 0, 0, 0))
            for sc in (nowhere, pointed, empty):
                got = fn(ctypes.byref(sc), ctypes.byref(cfg), tr, None, None, None, None, None, 0, None)
                assert got == 1, (name, p)
        ok = ctypes.byref(N.DavaTrainingF64(0.1, 3, 0, 1))
        for tr in (None, ok, ctypes.byref(N.DavaTrainingF64(1.0, 0, 0, 0))):
            assert fn(None, ctypes.byref(cfg), tr, None, None, None, None, None, 0, None) == 1
            assert fn(ctypes.byref(empty), ctypes.byref(cfg), tr, None, None, None, None, None, 0, None) == 0
            assert fn(ctypes.byref(nowhere), ctypes.byref(cfg), tr, fake, fake, None, fake, None, 0, None) == 1
            # C5's image does not fit the LDS: unsupported, before any launch
            assert fn(ctypes.byref(big), ctypes.byref(cfg), tr, fake, fake, None, fake, fake, 1 << 40, None) == 4
            # a workspace / tape of the (unchanged) query's size is required
            assert fn(ctypes.byref(pointed), ctypes.byref(cfg), tr, fake, fake, None, fake, fake, need[name] - 1,
                      None) == 2
    # the size queries take no training argument
    from deep_attention_visual_odometry_amd._native import SIGNATURES

    assert len(SIGNATURES["dava_ba_solve_workspace_bytes_f64"][1]) == 2
    assert len(SIGNATURES["dava_ba_solve_tape_bytes_f64"][1]) == 2


def test_fake_kernels_trace_with_the_training_arguments():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from deep_attention_visual_odometry_amd import _ops

    with FakeTensorMode():
        x = torch.empty(5, 3 + 3 * 16 + 6, device="cuda", dtype=torch.float64)
        obs = torch.empty(5, 2, 16, 2, device="cuda", dtype=torch.float64)
        vis = torch.empty(5, 2, 16, dtype=torch.uint8, device="cuda")
        ws = torch.empty(0, dtype=torch.uint8, device="cuda")
        xo, err, st = torch.ops.dava.ba_solve(x, obs, vis, 2, 16, False, 1e-4, 0.9, -1.0, 7, -1.0, 1000, True, 1, 0,
                                              True, ws, 0.1, 12345, True)
        assert xo.shape == x.shape and xo.dtype == torch.float64 and err.shape == (5,) and st.shape == (5, 4)
        head = (x, obs, vis, 2, 16, False, 1e-4, 0.9, -1.0, 7, -1.0, 1000, True, 0)
        for tail in ((), (True,), (True, 0.1, 2 ** 61 + 5, True)):  # positional callers of before, and the new ones
            xo, st, tape, err = torch.ops.dava.ba_solve_record_f64(*head, *tail)
            assert xo.shape == x.shape and xo.dtype == torch.float64 and st.shape == (5, 4) and st.dtype == torch.int32
            assert tape.dtype == torch.uint8 and tape.numel() == _ops.tape_bytes_f64(5, x.shape[1], 7)
            assert err.shape == ((5,) if tail else (0,))
        xo, st, tape, err = torch.ops.dava.ba_solve_record_f64(*head, drop_path_p=0.2, drop_seed=3,
                                                               return_second_last=False)
        assert tape.numel() == _ops.tape_bytes_f64(5, x.shape[1], 7)
    schema = str(torch.ops.dava.ba_solve_record_f64.default._schema)
    assert schema.index("want_error") < schema.index("drop_path_p") < schema.index("drop_seed") \
        < schema.index("return_second_last")
    assert "drop_path_p=0." in schema and "drop_seed=0" in schema and "return_second_last=False" in schema  # defaulted


def test_refusals_are_unchanged():
    """Training mode without float64_derivatives=True keeps today's refusals and routes: float64 parameters that
    require grad raise TypeError in training mode as in eval mode, and the non-compact float64 solve is refused."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    from deep_attention_visual_odometry_amd import BFGSSolver, RayAngleError, ReprojectionError

    with FakeTensorMode():
        x = torch.empty(5, 3 + 3 * 16 + 6, device="cuda", dtype=torch.float64)
        obs = torch.empty(5, 2, 16, 2, device="cuda", dtype=torch.float64)
        vis = torch.empty(5, 2, 16, dtype=torch.uint8, device="cuda")
        for cls in (ReprojectionError, RayAngleError):
            for s in (BFGSSolver(iterations=7), BFGSSolver(iterations=7, drop_path_p=0.0, return_second_last=True),
                      BFGSSolver(iterations=7).eval()):
                with pytest.raises(TypeError, match="second derivatives"):
                    s(x.clone().requires_grad_(True), cls(obs, vis, 2, 16))


def test_non_compact_float64_solve_is_still_refused():
    """The hessian_mode refusal of the float64 branch of dava::ba_solve comes before anything touches the device."""
    from deep_attention_visual_odometry_amd import _native as N
    from deep_attention_visual_odometry_amd import _ops

    x = torch.zeros(2, 3 + 3 * 16 + 6, dtype=torch.float64)
    obs = torch.zeros(2, 2, 16, 2, dtype=torch.float64)
    vis = torch.zeros(2, 2, 16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="compact"):
        _ops.ba_solve._init_fn(x, obs, vis, 2, 16, False, 1e-4, 0.9, 1e-4, 7, 1e-8, 1000, True, N.DAVA_HESSIAN_DENSE, 0,
                               False, torch.empty(0, dtype=torch.uint8), 0.1, 3, True)
