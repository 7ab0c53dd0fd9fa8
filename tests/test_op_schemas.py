"""The operator boundary as data (CPU only, no library call): every ``torch.ops.dava`` schema and the order of
``_ops.OPS`` against ``tests/golden/op_schemas.json``, the fake kernels of the twelve operators that the factories
of ``_ops.py`` write (second derivatives, gradient descent, its recording and its adjoint, in float32, float64 and
their ``*_large`` forms) against a table, and the operand check those operators share."""
import itertools
import json
import os

import pytest
import torch

from conftest import REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "op_schemas.json")


def test_schemas_and_operator_order_are_the_recorded_ones():
    from deep_attention_visual_odometry_amd import _ops

    golden = json.load(open(GOLDEN))
    assert list(_ops.OPS) == golden["order"]
    assert sorted(golden["schemas"]) == sorted(_ops.OPS)
    for name in _ops.OPS:
        assert str(getattr(torch.ops.dava, name).default._schema) == golden["schemas"][name], name


# B = 3 problems of M = 2 views and N = 16 points: P = 3 + 3 N + 6 (M - 1) = 57, tape rows round_up(P, 4) = 60; K = 3
B, M, N, P, ROWS, K = 3, 2, 16, 57, 60, 3
F32, F64 = torch.float32, torch.float64
X, OBS, NONE = (B, P), (B, M, N, 2), (0,)

# operator -> (dtype, schema row); the rows' output shapes by their want_* flags are below
TABLE = {
    "ba_second_order": (F32, "second"), "ba_second_order_large": (F32, "second"),
    "ba_second_order_f64": (F64, "second"), "ba_second_order_large_f64": (F64, "second"),
    "ba_sgd_solve": (F32, "descent"), "ba_sgd_solve_f64": (F64, "descent"),
    "ba_sgd_solve_differentiable": (F32, "record"), "ba_sgd_solve_differentiable_large": (F32, "record"),
    "ba_sgd_solve_differentiable_f64": (F64, "record"),
    "ba_sgd_backward": (F32, "adjoint"), "ba_sgd_backward_large": (F32, "adjoint"),
    "ba_sgd_backward_f64": (F64, "adjoint"),
}


def _cases(row, x, obs, vis, tape):
    """(arguments, expected output shapes) for both values of each want_* flag of the row."""
    if row == "second":
        for want_hv, want_obs in itertools.product((False, True), repeat=2):
            yield ((x, obs, vis, M, N, False, x, 0, want_hv, want_obs, obs),
                   ((B,), X, X if want_hv else NONE, OBS if want_obs else NONE,
                    OBS if (want_obs and want_hv) else NONE))
    elif row == "descent":
        for want_errors in (False, True):
            yield (x, obs, vis, M, N, False, 1e-3, K, 0, want_errors), (X, (B, K) if want_errors else NONE)
    elif row == "record":
        for want_errors in (False, True):
            yield ((x, obs, vis, M, N, False, 1e-3, K, 0, want_errors),
                   (X, (B, K) if want_errors else NONE, (B, K, ROWS)))
    else:
        for want_observations in (False, True):
            yield ((x, tape, obs, vis, M, N, False, 1e-3, K, 0, want_observations),
                   (X, OBS if want_observations else NONE))


@pytest.mark.parametrize("name", sorted(TABLE))
def test_fake_kernels_match_the_table(name):
    from torch._subclasses.fake_tensor import FakeTensorMode

    from deep_attention_visual_odometry_amd import _ops  # noqa: F401  (registers torch.ops.dava.*)

    dtype, row = TABLE[name]
    assert P == _ops.num_parameters(M, N, False) and ROWS == _ops.sgd_tape_rows(P)
    with FakeTensorMode():
        x = torch.empty(X, dtype=dtype, device="meta")
        obs = torch.empty(OBS, dtype=dtype, device="meta")
        vis = torch.empty((B, M, N), dtype=torch.uint8, device="meta")
        tape = torch.empty((B, K, ROWS), dtype=dtype, device="meta")
        cases = list(_cases(row, x, obs, vis, tape))
        assert len(cases) == (4 if row == "second" else 2)
        for args, shapes in cases:
            outs = getattr(torch.ops.dava, name)(*args)
            assert tuple(tuple(o.shape) for o in outs) == shapes, (name, args[-4:])
            assert all(o.dtype == dtype for o in outs), (name, [o.dtype for o in outs])


def test_the_twelve_operators_are_all_in_ops():
    from deep_attention_visual_odometry_amd import _ops

    assert set(TABLE) <= set(_ops.OPS) and len(TABLE) == 12


def test_same_refuses_another_device_dtype_shape_or_layout():
    """``_ops._same``, the check of ``direction`` / ``obs_direction`` in all four second-derivative operators: an
    operand on another device than the tensor whose extents the kernel reads it with is refused on the host (no
    launch), as are another dtype, another shape and a strided view; None and a matching tensor pass."""
    from deep_attention_visual_odometry_amd import _ops

    like = torch.empty((B, P), dtype=F32, device="meta")
    with pytest.raises(ValueError, match=r"direction must be a contiguous float32 tensor of shape \(3, 57\) on meta"):
        _ops._same(torch.zeros(B, P), like, F32, "direction")  # cpu against meta
    host = torch.zeros(B, P)
    with pytest.raises(ValueError, match="contiguous float32 tensor"):
        _ops._same(torch.zeros(B, P, dtype=F64), host, F32, "direction")
    with pytest.raises(ValueError, match="contiguous float64 tensor"):
        _ops._same(host, host, F64, "direction")
    with pytest.raises(ValueError, match="of shape"):
        _ops._same(torch.zeros(B, P + 1), host, F32, "direction")
    with pytest.raises(ValueError, match="contiguous"):
        _ops._same(torch.zeros(P, B).t(), host, F32, "obs_direction")
    assert not torch.zeros(P, B).t().is_contiguous()
    _ops._same(None, host, F32, "direction")
    _ops._same(torch.ones(B, P), host, F32, "direction")
    _ops._same(torch.empty((B, P), dtype=F64, device="meta"), like.double(), F64, "direction")
