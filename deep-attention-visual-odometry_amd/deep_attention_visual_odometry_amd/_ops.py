"""The C ABI (include/dava_ba.h) registered as PyTorch operators: ``torch.ops.dava.*``.

Every HIP entry point of ``libdava_ba.so`` is a ``torch.library`` custom op with a
fake (meta) implementation, so ``torch.compile`` and FakeTensor tracing see opaque
operators with known output shapes and dtypes (no graph break at a ctypes call),
and eager calls dispatch straight to the HIP launch on the tensor's current stream.

The ops are registered for the ``cuda`` (= ROCm/HIP) dispatch key only: a CPU tensor
reaching one of them raises ``NotImplementedError`` from the dispatcher -- there is no
CPU kernel and no fallback.  Outputs a caller did not ask for come back as empty
(numel 0) tensors so every op has a fixed schema; ``native_ops`` maps them to None.
Ops never alias or mutate their inputs, except the Wolfe state machine's
``state``/``flags`` (declared in ``mutates_args``) and a caller-supplied workspace.
"""
from typing import Callable, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import _native as N

_CUDA = "cuda"
_POISON = N._DEBUG_ENV and bool(__import__("os").environ.get("DAVA_POISON_SCRATCH"))  # NaN-filled tapes (diagnostics)


def _dt(t: Tensor) -> str:
    if t.dtype == torch.float32:
        return "f32"
    if t.dtype == torch.float64:
        return "f64"
    raise TypeError(f"unsupported dtype {t.dtype}: the HIP kernels implement float32 and float64")


def _empty0(like: Tensor, dtype=None) -> Tensor:
    return like.new_empty((0,), dtype=dtype or like.dtype)


def num_parameters(num_views: int, num_points: int, distortion: bool) -> int:
    return 3 + 3 * num_points + 6 * (num_views - 1) + (5 if distortion else 0)


def scene_struct(observations: Optional[Tensor], visibility: Optional[Tensor], num_views: int, num_points: int,
                 distortion: bool, batch: int, residual: int = N.DAVA_RESIDUAL_SQUARED_REPROJECTION) -> N.DavaScene:
    return N.DavaScene(batch, num_views, num_points, 1 if distortion else 0,
                       num_parameters(num_views, num_points, distortion),
                       N.ptr(observations), N.ptr(visibility), residual)


def scene_struct_f64(observations: Optional[Tensor], visibility: Optional[Tensor], num_views: int, num_points: int,
                     distortion: bool, batch: int,
                     residual: int = N.DAVA_RESIDUAL_SQUARED_REPROJECTION) -> N.DavaSceneF64:
    return N.DavaSceneF64(batch, num_views, num_points, 1 if distortion else 0,
                          num_parameters(num_views, num_points, distortion),
                          N.ptr(observations), N.ptr(visibility), residual)


def solver_config_f64(sufficient_decrease, curvature, error_threshold, iterations, minimum_step,
                      max_line_search_trials, strong) -> N.DavaSolverConfigF64:
    return N.DavaSolverConfigF64(float(sufficient_decrease), float(curvature), float(error_threshold),
                                 float(minimum_step), int(iterations), int(max_line_search_trials),
                                 1 if strong else 0)


def training_f64(drop_path_p: float = 0.0, drop_seed: int = 0, return_second_last: bool = False) -> N.DavaTrainingF64:
    """Training mode of the float64 fused solve (all zero: eval mode, the eval launch)."""
    seed = int(drop_seed) & 0xFFFFFFFFFFFFFFFF
    return N.DavaTrainingF64(float(drop_path_p), seed & 0xFFFFFFFF, seed >> 32, 1 if return_second_last else 0)


def solver_config(sufficient_decrease, curvature, error_threshold, iterations, minimum_step, max_line_search_trials,
                  strong, hessian_mode, drop_path_p: float = 0.0, drop_seed: int = 0,
                  return_second_last: bool = False) -> N.DavaSolverConfig:
    seed = int(drop_seed) & 0xFFFFFFFFFFFFFFFF
    return N.DavaSolverConfig(float(sufficient_decrease), float(curvature), float(error_threshold),
                              float(minimum_step), int(iterations), int(max_line_search_trials),
                              1 if strong else 0, int(hessian_mode), float(drop_path_p), seed & 0xFFFFFFFF, seed >> 32,
                              1 if return_second_last else 0)


def _check_scene_tensors(x: Tensor, observations: Tensor, visibility: Tensor, num_views: int, num_points: int,
                         distortion: bool) -> None:
    """Host-side shape checks BEFORE a launch: the kernels index with exactly these extents."""
    b = x.shape[0]
    p = num_parameters(num_views, num_points, distortion)
    if x.dim() != 2 or x.shape[1] != p:
        raise ValueError(f"parameters must be (B, {p}), got {tuple(x.shape)}")
    if tuple(observations.shape) != (b, num_views, num_points, 2):
        raise ValueError(f"observations must be ({b}, {num_views}, {num_points}, 2), got {tuple(observations.shape)}")
    if tuple(visibility.shape) != (b, num_views, num_points):
        raise ValueError(f"visibility must be ({b}, {num_views}, {num_points}), got {tuple(visibility.shape)}")
    if x.dtype not in (torch.float32, torch.float64) or observations.dtype != x.dtype \
            or visibility.dtype != torch.uint8:
        raise TypeError("parameters and observations must both be float32 or both float64 (observations "
                        f"{observations.dtype}, parameters {x.dtype}) and visibility uint8")
    for t in (x, observations, visibility):
        if not t.is_contiguous() or t.device != x.device:
            raise ValueError("scene tensors must be contiguous and on one device")


def _require_float32(x: Tensor, what: str) -> None:
    if x.dtype != torch.float32:
        raise TypeError(f"{what} are float32 only (got {x.dtype}); the float64 flavour covers ba_solve and "
                        "ba_evaluate")


def _require_float64(x: Tensor, what: str) -> None:
    if x.dtype != torch.float64:
        raise TypeError(f"{what} take float64 tensors (got {x.dtype})")


def _same(t: Optional[Tensor], like: Tensor, dtype: torch.dtype, what: str) -> None:
    """An optional operand a kernel reads with ``like``'s extents: its shape, its device, ``dtype``, contiguous."""
    if t is not None and (t.shape != like.shape or t.dtype != dtype or t.device != like.device
                          or not t.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous {_name(dtype)} tensor of shape {tuple(like.shape)} on "
                         f"{like.device}")


def _name(dtype: torch.dtype) -> str:
    return str(dtype).split(".")[-1]  # "float32"


def _scratch(need: int, dev) -> Tensor:
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    if _POISON:  # debugging aid: every byte the kernels do not write reads back as NaN
        ws.fill_(0xFF)
    return ws


def sgd_config(learning_rate: float, iterations: int) -> N.DavaSgdConfig:
    return N.DavaSgdConfig(float(learning_rate), int(iterations))


def sgd_config_f64(learning_rate: float, iterations: int) -> N.DavaSgdConfigF64:
    return N.DavaSgdConfigF64(float(learning_rate), int(iterations))


class _Flavour(NamedTuple):
    """What the float32 and the float64 operator of one schema differ in, besides their C symbols and refusals: the
    factories below (second derivatives, gradient descent, its recording and its adjoint) write each body once."""
    dtype: torch.dtype
    scene: Callable      # scene_struct / scene_struct_f64
    sgd_config: Callable
    require: Callable    # (tensor, what): the TypeError of another dtype


_F32 = _Flavour(torch.float32, scene_struct, sgd_config, _require_float32)
_F64 = _Flavour(torch.float64, scene_struct_f64, sgd_config_f64, _require_float64)


def f64_old_symbol_runs(probe) -> bool:
    """The routing rule of every float64 operation that has a ``*_large_*`` symbol, written once: the symbol of the
    LDS image takes the call where no F64_FORM override is set (it ignores the override, so a run that asks for
    another form must not reach it) and ``probe()`` -- its size query, its form query or the host refusal of the
    launch itself -- says it runs the scene; every other call goes to the ``*_large_*`` symbol."""
    return N.library_knob("F64_FORM") <= 0 and bool(probe())


# ---------------------------------------------------------------- fused BA ops

@torch.library.custom_op("dava::ba_solve", mutates_args=("workspace",), device_types=_CUDA)
def ba_solve(x0: Tensor, observations: Tensor, visibility: Tensor, num_views: int, num_points: int,
             distortion: bool, sufficient_decrease: float, curvature: float, error_threshold: float,
             iterations: int, minimum_step: float, max_line_search_trials: int, strong: bool, hessian_mode: int,
             residual: int, want_error: bool, workspace: Tensor, drop_path_p: float = 0.0,
             drop_seed: int = 0, return_second_last: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """``dava_ba_solve``: the whole eval-mode BFGS solve of a (B, P) fp32 batch in one launch.
    ``workspace``: a uint8 scratch buffer of at least ``dava_ba_solve_workspace_bytes`` (its contents
    are overwritten), or an empty tensor to allocate one per call.
    Returns (x, error (B,) or empty, status (B, 4) int32).
    A float64 batch (parameters and observations) runs ``dava_ba_solve_train_f64``: compact history, the
    training-mode arguments with the float32 semantics (all off: the launch of ``dava_ba_solve_f64``) -- or, for a
    scene beyond that kernel's LDS image, ``dava_ba_solve_large_f64`` with the same contract."""
    lib = N.load_library()
    _check_scene_tensors(x0, observations, visibility, num_views, num_points, distortion)
    b = x0.shape[0]
    dev = x0.device
    if x0.dtype == torch.float64:
        if hessian_mode != N.DAVA_HESSIAN_COMPACT:
            raise ValueError("the float64 fused solve runs the compact history only "
                             "(hessian_mode == DAVA_HESSIAN_COMPACT)")
        train64 = training_f64(drop_path_p, drop_seed, return_second_last)
        sc64 = scene_struct_f64(observations, visibility, num_views, num_points, distortion, b, residual)
        cfg64 = solver_config_f64(sufficient_decrease, curvature, error_threshold, iterations, minimum_step,
                                  max_line_search_trials, strong)
        # the symbols of the LDS image where they take the call, else the ones that take any scene size (forms 1
        # and 2: the scene, then the vectors too, out of LDS)
        large = not f64_old_symbol_runs(lambda: lib.dava_ba_solve_workspace_bytes_f64(sc64, cfg64) > 0)
        query = "dava_ba_solve_large_workspace_bytes_f64" if large else "dava_ba_solve_workspace_bytes_f64"
        need = int(getattr(lib, query)(sc64, cfg64))
        if need == 0:
            raise ValueError("this scene / configuration has no float64 fused solve (1 <= iterations <= 1025, "
                             "at most 251 views at 1025 iterations)")
        if workspace.numel() < need or workspace.device != dev or workspace.dtype != torch.uint8:
            if workspace.numel() > 0:
                raise ValueError(f"workspace holds {workspace.numel()} bytes, the solve needs {need} "
                                 "(uint8, same device)")
            workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        x_out = torch.empty_like(x0)
        err = torch.empty(b, device=dev, dtype=torch.float64) if want_error else _empty0(x0)
        status = torch.empty((b, N.STATUS_WORDS), device=dev, dtype=torch.int32)
        name = "dava_ba_solve_large_f64" if large else "dava_ba_solve_train_f64"
        with torch.cuda.device(dev):
            N.check(getattr(lib, name)(sc64, cfg64, train64, N.ptr(x0), N.ptr(x_out),
                                       N.ptr(err) if want_error else None, N.ptr(status), N.ptr(workspace),
                                       workspace.numel(), N.stream_of(dev)), name)
        return x_out, err, status
    sc = scene_struct(observations, visibility, num_views, num_points, distortion, b, residual)
    cfg = solver_config(sufficient_decrease, curvature, error_threshold, iterations, minimum_step,
                        max_line_search_trials, strong, hessian_mode, drop_path_p, drop_seed, return_second_last)
    need = int(lib.dava_ba_solve_workspace_bytes(sc, cfg))
    if workspace.numel() < need or workspace.device != dev or workspace.dtype != torch.uint8:
        if workspace.numel() > 0:
            raise ValueError(f"workspace holds {workspace.numel()} bytes, the solve needs {need} (uint8, same device)")
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    x_out = torch.empty_like(x0)
    err = torch.empty(b, device=dev, dtype=torch.float32) if want_error else _empty0(x0)
    status = torch.empty((b, N.STATUS_WORDS), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        N.check(lib.dava_ba_solve(sc, cfg, N.ptr(x0), N.ptr(x_out), N.ptr(err) if want_error else None,
                                  N.ptr(status), N.ptr(workspace), workspace.numel(), N.stream_of(dev)),
                "dava_ba_solve")
    return x_out, err, status


@ba_solve.register_fake
def _(x0, observations, visibility, num_views, num_points, distortion, sufficient_decrease, curvature,
      error_threshold, iterations, minimum_step, max_line_search_trials, strong, hessian_mode, residual, want_error,
      workspace, drop_path_p=0.0, drop_seed=0, return_second_last=False):
    b = x0.shape[0]
    return (torch.empty_like(x0), x0.new_empty((b,) if want_error else (0,)),
            x0.new_empty((b, N.STATUS_WORDS), dtype=torch.int32))


@torch.library.custom_op("dava::bfgs_solve", mutates_args=(), device_types=_CUDA)
def bfgs_solve(parameters: Tensor, observations: Tensor, visibility: Tensor, num_views: int, num_points: int,
               distortion: bool = False, iterations: int = 1000, error_threshold: float = 1e-4,
               minimum_step: float = 1e-8, sufficient_decrease: float = 1e-4, curvature: float = 0.9,
               residual: int = 0) -> Tuple[Tensor, Tensor]:
    """The functional entry SURVEY.md 8(b) names: ``BFGSSolver().eval()`` on the fused objective with
    the reference's defaults (``bfgs_solver.py:49-60``, strong Wolfe, ``wolfe_conditions.py:116``'s
    1000 trials), compact inverse-Hessian history, workspace allocated per call.
    Returns (x (B, P), status (B, 4) int32: steps, stop reason, evaluations, line-search trials)."""
    x, _, status = ba_solve(parameters, observations, visibility, num_views, num_points, distortion,
                            sufficient_decrease, curvature, error_threshold, iterations, minimum_step, 1000, True,
                            N.DAVA_HESSIAN_COMPACT, residual, False, _empty0(parameters, torch.uint8))
    return x, status


@bfgs_solve.register_fake
def _(parameters, observations, visibility, num_views, num_points, distortion=False, iterations=1000,
      error_threshold=1e-4, minimum_step=1e-8, sufficient_decrease=1e-4, curvature=0.9, residual=0):
    return torch.empty_like(parameters), parameters.new_empty((parameters.shape[0], N.STATUS_WORDS), dtype=torch.int32)


@torch.library.custom_op("dava::ba_evaluate", mutates_args=(), device_types=_CUDA)
def ba_evaluate(x: Tensor, observations: Tensor, visibility: Tensor, num_views: int, num_points: int,
                distortion: bool, direction: Optional[Tensor], alpha: Optional[Tensor], want_grad: bool,
                want_slope: bool, residual: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``dava_ba_evaluate``: E, dE/dx and d . dE/dx at x + alpha d.  Unrequested outputs are empty."""
    lib = N.load_library()
    _check_scene_tensors(x, observations, visibility, num_views, num_points, distortion)
    b = x.shape[0]
    for t in (direction, alpha):
        if t is not None and (t.device != x.device or t.dtype != x.dtype or not t.is_contiguous()):
            raise ValueError("direction / alpha must be contiguous, of the parameters' dtype and on their device")
    if direction is not None and direction.shape != x.shape:
        raise ValueError("direction must have the parameters' shape")
    if alpha is not None and alpha.numel() != b:
        raise ValueError("alpha must hold one value per problem")
    if want_slope and direction is None:
        raise ValueError("the slope needs a direction")
    err = torch.empty(b, device=x.device, dtype=x.dtype)
    grad = torch.empty_like(x) if want_grad else _empty0(x)
    slope = torch.empty(b, device=x.device, dtype=x.dtype) if want_slope else _empty0(x)
    if x.dtype == torch.float64:
        sc64 = scene_struct_f64(observations, visibility, num_views, num_points, distortion, b, residual)
        args = (sc64, N.ptr(x), N.ptr(direction), N.ptr(alpha), N.ptr(err), N.ptr(grad) if want_grad else None,
                N.ptr(slope) if want_slope else None, N.stream_of(x.device))
        status = N.DAVA_OK

        def old_symbol_takes_it() -> bool:  # (its refusal comes from the host, before any launch)
            nonlocal status
            status = lib.dava_ba_evaluate_f64(*args)
            return status != N.DAVA_ERR_UNSUPPORTED

        with torch.cuda.device(x.device):
            if f64_old_symbol_runs(old_symbol_takes_it):
                N.check(status, "dava_ba_evaluate_f64")
            else:
                N.check(lib.dava_ba_evaluate_large_f64(*args), "dava_ba_evaluate_large_f64")
        return err, grad, slope
    sc = scene_struct(observations, visibility, num_views, num_points, distortion, b, residual)
    with torch.cuda.device(x.device):
        N.check(lib.dava_ba_evaluate(sc, N.ptr(x), N.ptr(direction), N.ptr(alpha), N.ptr(err),
                                     N.ptr(grad) if want_grad else None, N.ptr(slope) if want_slope else None,
                                     N.stream_of(x.device)), "dava_ba_evaluate")
    return err, grad, slope


@ba_evaluate.register_fake
def _(x, observations, visibility, num_views, num_points, distortion, direction, alpha, want_grad, want_slope,
      residual):
    b = x.shape[0]
    return (x.new_empty((b,)), torch.empty_like(x) if want_grad else x.new_empty((0,)),
            x.new_empty((b,) if want_slope else (0,)))


# ---------------------------------------- second derivatives: float32, float64 and their `*_large` forms
# One body and one fake kernel for the four operators.  ba_second_order and ba_second_order_f64 keep one problem's
# whole dual image in LDS (160 KiB), keep their limits and ignore the form overrides; the `*_large` operators take
# any admitted scene size (forms 1 and 2 beyond the LDS image; a scene whose image fits runs the launch of the first)
# and differ in the C symbol, one scratch buffer from torch's allocator and the refusal text.

def _second_order_op(name: str, doc: str, flavour: _Flavour, what: str, symbol: str = "",
                     workspace_query: Optional[str] = None, refusal: str = ""):
    symbol = symbol or f"dava_{name}"

    @torch.library.custom_op(f"dava::{name}", mutates_args=(), device_types=_CUDA)
    def op(x: Tensor, observations: Tensor, visibility: Tensor, num_views: int, num_points: int, distortion: bool,
           direction: Optional[Tensor], residual: int, want_hv: bool, want_obs: bool,
           obs_direction: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
        lib = N.load_library()
        flavour.require(x, what)
        _check_scene_tensors(x, observations, visibility, num_views, num_points, distortion)
        _same(direction, x, flavour.dtype, "direction")
        _same(obs_direction, observations, flavour.dtype, "obs_direction")
        b = x.shape[0]
        err = torch.empty(b, device=x.device, dtype=flavour.dtype)
        grad = torch.empty_like(x)
        hv = torch.empty_like(x) if want_hv else _empty0(x)
        obs_grad = torch.empty_like(observations) if want_obs else _empty0(x)
        obs_hv = torch.empty_like(observations) if (want_obs and want_hv) else _empty0(x)
        sc = flavour.scene(observations, visibility, num_views, num_points, distortion, b, residual)
        scratch = ()
        if workspace_query:
            need = int(getattr(lib, workspace_query)(sc, 1 if want_obs else 0))
            if need == 0:
                raise ValueError(refusal)
            ws = _scratch(need, x.device)
            scratch = (N.ptr(ws), ws.numel())
        with torch.cuda.device(x.device):
            N.check(getattr(lib, symbol)(sc, N.ptr(x), N.ptr(direction), N.ptr(obs_direction), N.ptr(err), N.ptr(grad),
                                         N.ptr(hv) if want_hv else None, N.ptr(obs_grad) if want_obs else None,
                                         N.ptr(obs_hv) if (want_obs and want_hv) else None, *scratch,
                                         N.stream_of(x.device)), symbol)
        return err, grad, hv, obs_grad, obs_hv

    op.__doc__ = doc
    op.register_fake(_second_order_fake)
    return op


def _second_order_fake(x, observations, visibility, num_views, num_points, distortion, direction, residual,
                       want_hv, want_obs, obs_direction=None):
    b = x.shape[0]
    return (x.new_empty((b,)), torch.empty_like(x), torch.empty_like(x) if want_hv else x.new_empty((0,)),
            torch.empty_like(observations) if want_obs else x.new_empty((0,)),
            torch.empty_like(observations) if (want_obs and want_hv) else x.new_empty((0,)))


ba_second_order = _second_order_op(
    "ba_second_order",
    """``dava_ba_second_order_obs``: (E, dE/dx, H v + (d2E/dx dobs) u, dE/dobs, (d2E/dobs dx) v + (d2E/dobs2) u),
    forward-over-reverse.  direction / obs_direction None mean v = 0 / u = 0.  Unrequested outputs are empty.""",
    _F32, "second derivatives of the fused objectives", "dava_ba_second_order_obs")
ba_second_order_large = _second_order_op(
    "ba_second_order_large", "``dava_ba_second_order_large``: ``ba_second_order`` for a scene of any size.",
    _F32, "second derivatives of the fused objectives", "", "dava_ba_second_order_large_workspace_bytes",
    "this scene has no float32 second derivatives (more views than the dual view constants can hold in LDS)")
ba_second_order_f64 = _second_order_op(
    "ba_second_order_f64",
    "``dava_ba_second_order_f64``: ``ba_second_order`` on a float64 batch (dual numbers over double).",
    _F64, "the float64 second derivatives")
ba_second_order_large_f64 = _second_order_op(
    "ba_second_order_large_f64",
    "``dava_ba_second_order_large_f64``: ``ba_second_order_f64`` for a scene of any size.",
    _F64, "the float64 second derivatives", "", "dava_ba_second_order_large_workspace_bytes_f64",
    "this scene has no float64 second derivatives (more views than the dual view constants can hold in LDS)")


@torch.library.custom_op("dava::ba_solve_record", mutates_args=(), device_types=_CUDA)
def ba_solve_record(x0: Tensor, observations: Tensor, visibility: Tensor, num_views: int, num_points: int,
                    distortion: bool, sufficient_decrease: float, curvature: float, error_threshold: float,
                    iterations: int, minimum_step: float, max_line_search_trials: int, strong: bool,
                    residual: int, drop_path_p: float = 0.0, drop_seed: int = 0,
                    return_second_last: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """``dava_ba_solve_record``: the fused COMPACT solve (bitwise ``ba_solve``'s x and status) plus the
    tape the adjoint replays.  Returns (x, status (B, 4) int32, tape uint8)."""
    lib = N.load_library()
    _require_float32(x0, "the recording solve")
    _check_scene_tensors(x0, observations, visibility, num_views, num_points, distortion)
    b, dev = x0.shape[0], x0.device
    sc = scene_struct(observations, visibility, num_views, num_points, distortion, b, residual)
    cfg = solver_config(sufficient_decrease, curvature, error_threshold, iterations, minimum_step,
                        max_line_search_trials, strong, N.DAVA_HESSIAN_COMPACT, drop_path_p, drop_seed,
                        return_second_last)
    need = int(lib.dava_ba_solve_tape_bytes(sc, cfg))
    if need == 0:
        raise ValueError("this scene / configuration has no fused adjoint (compact mode, P <= 14336, "
                         "iterations >= 1)")
    tape = torch.empty(need, dtype=torch.uint8, device=dev)
    if _POISON:  # debugging aid: every byte the kernels do not write reads back as NaN
        tape.fill_(0xFF)
    x_out = torch.empty_like(x0)
    status = torch.empty((b, N.STATUS_WORDS), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        N.check(lib.dava_ba_solve_record(sc, cfg, N.ptr(x0), N.ptr(x_out), None, N.ptr(status), N.ptr(tape),
                                         tape.numel(), N.stream_of(dev)), "dava_ba_solve_record")
    return x_out, status, tape


@ba_solve_record.register_fake
def _(x0, observations, visibility, num_views, num_points, distortion, sufficient_decrease, curvature,
      error_threshold, iterations, minimum_step, max_line_search_trials, strong, residual, drop_path_p=0.0,
      drop_seed=0, return_second_last=False):
    b = x0.shape[0]
    ctx = torch.library.get_ctx()
    return (torch.empty_like(x0), x0.new_empty((b, N.STATUS_WORDS), dtype=torch.int32),
            x0.new_empty((ctx.new_dynamic_size(),), dtype=torch.uint8))


@torch.library.custom_op("dava::ba_solve_backward", mutates_args=(), device_types=_CUDA)
def ba_solve_backward(x_out_grad: Tensor, tape: Tensor, status: Tensor, observations: Tensor, visibility: Tensor,
                      num_views: int, num_points: int, distortion: bool, iterations: int, residual: int,
                      want_observations: bool) -> Tuple[Tensor, Tensor]:
    """``dava_ba_solve_backward``: (dL/dx0, dL/dobs or empty) of a recorded solve for dL/dx_out."""
    lib = N.load_library()
    _require_float32(x_out_grad, "the fused solve's adjoint")
    _check_scene_tensors(x_out_grad, observations, visibility, num_views, num_points, distortion)
    b, dev = x_out_grad.shape[0], x_out_grad.device
    if tuple(status.shape) != (b, N.STATUS_WORDS) or status.dtype != torch.int32 or not status.is_contiguous():
        raise ValueError("status must be the recording call's contiguous (B, 4) int32 tensor")
    # the kernel dereferences tape and status as device memory of this launch: refuse anything else
    # loudly rather than fault the GPU (a CPU or other-device tensor, a short or strided tape)
    for what, t in (("tape", tape), ("status", status)):
        if t.device != dev:
            raise ValueError(f"{what} must be on {dev} (the cotangent's device), got {t.device}")
    if tape.dtype != torch.uint8 or tape.dim() != 1 or not tape.is_contiguous():
        raise ValueError("tape must be the recording call's contiguous 1-D uint8 tensor")
    sc = scene_struct(observations, visibility, num_views, num_points, distortion, b, residual)
    cfg = solver_config(1e-4, 0.9, 1e-4, iterations, 1e-8, 1000, True, N.DAVA_HESSIAN_COMPACT)
    tape_need = int(lib.dava_ba_solve_tape_bytes(sc, cfg))
    if tape.numel() < tape_need:
        raise ValueError(f"tape holds {tape.numel()} bytes; a recording of this scene and iteration count "
                         f"writes {tape_need}")
    need = int(lib.dava_ba_solve_backward_workspace_bytes(sc, cfg))
    if need == 0:
        raise ValueError("this scene / configuration has no fused adjoint")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    if _POISON:
        ws.fill_(0xFF)
    gx = torch.empty_like(x_out_grad)
    gobs = torch.empty_like(observations) if want_observations else _empty0(x_out_grad)
    with torch.cuda.device(dev):
        N.check(lib.dava_ba_solve_backward(sc, cfg, N.ptr(tape), tape.numel(), N.ptr(status), N.ptr(x_out_grad),
                                           N.ptr(gx), N.ptr(gobs) if want_observations else None, N.ptr(ws),
                                           ws.numel(), N.stream_of(dev)), "dava_ba_solve_backward")
    return gx, gobs


@ba_solve_backward.register_fake
def _(x_out_grad, tape, status, observations, visibility, num_views, num_points, distortion, iterations, residual,
      want_observations):
    return (torch.empty_like(x_out_grad),
            torch.empty_like(observations) if want_observations else x_out_grad.new_empty((0,)))


# ---------------------------------------- fused gradient descent (SGDSolver) and its adjoint
# Three schemas -- the descent, the recording descent (an autograd node) and its adjoint -- each with one body, one
# fake kernel and, for the node, one backward.  The float32 operators keep one problem's image in LDS and keep their
# refusals; ba_sgd_solve_differentiable_large and ba_sgd_backward_large take any admitted scene size (forms 1 and 2
# of csrc/ba_second_carve.hpp).  In float64 there is one operator per operation: the C symbols take forms 0, 1 and 2
# themselves (csrc/sgd_solve_f64.hip, sgd_adjoint_f64.hip).  Workspaces come from torch's allocator, sized by the
# library's host queries.

def sgd_tape_rows(p: int) -> int:
    """Floats per tape row: round_up(P, 4) (csrc/sgd_plan.hpp)."""
    return (p + 3) // 4 * 4


def _sgd_scene(flavour: _Flavour, x0: Tensor, observations: Tensor, visibility: Tensor, num_views: int,
               num_points: int, distortion: bool, learning_rate: float, iterations: int, residual: int, what: str):
    flavour.require(x0, what)
    _check_scene_tensors(x0, observations, visibility, num_views, num_points, distortion)
    if iterations < 0:
        raise ValueError(f"iterations must be >= 0, got {iterations}")
    sc = flavour.scene(observations, visibility, num_views, num_points, distortion, x0.shape[0], residual)
    return sc, flavour.sgd_config(learning_rate, iterations)


_SGD_REFUSAL = ("this scene has no fused gradient descent: its image (x and the gradient, 2 round_up(P, 4) floats, "
                "and the objective's view constants) does not fit one workgroup's 160 KiB of LDS")
_SGD_REFUSAL_F64 = ("this scene has no float64 fused gradient descent: more views than the view constants can hold "
                    "in one workgroup's 160 KiB of LDS")
_SGD_ADJOINT_REFUSAL_F64 = ("this scene has no float64 fused adjoint of the gradient descent: more views than the "
                            "dual view constants can hold in one workgroup's 160 KiB of LDS")
_SGD_ADJOINT_REFUSAL_LARGE = ("this scene has no fused adjoint of the gradient descent: more views than the dual view "
                              "constants can hold in LDS")


def _sgd_solve_workspace_f64(lib, sc, cfg, dev):
    """(tensor, pointer, bytes) of the descent's workspace: form 2's vectors, or (None, None, 0)."""
    if lib.dava_ba_sgd_solve_form_f64(sc, cfg) < 0:
        raise ValueError(_SGD_REFUSAL_F64)
    need = int(lib.dava_ba_sgd_solve_workspace_bytes_f64(sc, cfg))
    if need == 0:
        return None, None, 0
    ws = _scratch(need, dev)
    return ws, N.ptr(ws), ws.numel()


def _sgd_solve_op(name: str, doc: str, flavour: _Flavour, what: str, workspace: bool):
    """``workspace`` (float64): the form is asked before the launch and refuses there, and the symbol takes a
    workspace; without it (float32) the launch's own ``DAVA_ERR_UNSUPPORTED`` is the refusal."""
    symbol = f"dava_{name}"

    @torch.library.custom_op(f"dava::{name}", mutates_args=(), device_types=_CUDA)
    def op(x0: Tensor, observations: Tensor, visibility: Tensor, num_views: int, num_points: int, distortion: bool,
           learning_rate: float, iterations: int, residual: int, want_errors: bool) -> Tuple[Tensor, Tensor]:
        lib = N.load_library()
        sc, cfg = _sgd_scene(flavour, x0, observations, visibility, num_views, num_points, distortion, learning_rate,
                             iterations, residual, what)
        b, dev = x0.shape[0], x0.device
        scratch = ()
        if workspace:
            _ws, *scratch = _sgd_solve_workspace_f64(lib, sc, cfg, dev)
        x_out = torch.empty_like(x0)
        errs = torch.empty((b, iterations), device=dev, dtype=flavour.dtype) if want_errors else _empty0(x0)
        with torch.cuda.device(dev):
            status = getattr(lib, symbol)(sc, cfg, N.ptr(x0), N.ptr(x_out), N.ptr(errs) if want_errors else None,
                                          *scratch, N.stream_of(dev))
        if not workspace and status == N.DAVA_ERR_UNSUPPORTED:
            raise ValueError(_SGD_REFUSAL)
        N.check(status, symbol)
        return x_out, errs

    op.__doc__ = doc
    op.register_fake(_sgd_solve_fake)
    return op


def _sgd_solve_fake(x0, observations, visibility, num_views, num_points, distortion, learning_rate, iterations,
                    residual, want_errors):
    return torch.empty_like(x0), x0.new_empty((x0.shape[0], iterations) if want_errors else (0,))


ba_sgd_solve = _sgd_solve_op(
    "ba_sgd_solve",
    """``dava_ba_sgd_solve``: ``iterations`` steps x <- x - learning_rate dE/dx of a (B, P) fp32 batch in one
    launch.  Returns (x, E(x_k) (B, iterations) or empty).""",
    _F32, "the fused gradient descent", workspace=False)
ba_sgd_solve_f64 = _sgd_solve_op(
    "ba_sgd_solve_f64",
    """``dava_ba_sgd_solve_f64``: ``iterations`` steps x <- x - learning_rate dE/dx of a (B, P) float64 batch in
    one launch, at any form.  Returns (x, E(x_k) (B, iterations) or empty).""",
    _F64, "the float64 fused gradient descent", workspace=True)


def _check_sgd_tape(tape: Tensor, x_out_grad: Tensor, iterations: int, dtype: torch.dtype) -> None:
    """The kernel dereferences the tape as device memory of this launch: refuse anything else loudly."""
    b, dev = x_out_grad.shape[0], x_out_grad.device
    if (tape.device != dev or tape.dtype != dtype or not tape.is_contiguous()
            or tuple(tape.shape) != (b, iterations, sgd_tape_rows(x_out_grad.shape[1]))):
        raise ValueError(f"tape must be the recording call's contiguous {_name(dtype)} ({b}, {iterations}, "
                         f"{sgd_tape_rows(x_out_grad.shape[1])}) tensor on {dev}, got {tuple(tape.shape)} "
                         f"{tape.dtype} on {tape.device}")


def _sgd_backward_op(name: str, doc: str, flavour: _Flavour, what: str, workspace_query: Optional[str] = None,
                     form_query: Optional[str] = None, refusal: str = ""):
    """``refusal`` is raised where ``form_query`` answers < 0; without a form query, where ``workspace_query`` answers
    0 bytes (with one, 0 bytes mean a ``NULL`` workspace)."""
    symbol = f"dava_{name}"

    @torch.library.custom_op(f"dava::{name}", mutates_args=(), device_types=_CUDA)
    def op(x_out_grad: Tensor, tape: Tensor, observations: Tensor, visibility: Tensor, num_views: int,
           num_points: int, distortion: bool, learning_rate: float, iterations: int, residual: int,
           want_observations: bool) -> Tuple[Tensor, Tensor]:
        lib = N.load_library()
        sc, cfg = _sgd_scene(flavour, x_out_grad, observations, visibility, num_views, num_points, distortion,
                             learning_rate, iterations, residual, what)
        dev = x_out_grad.device
        _check_sgd_tape(tape, x_out_grad, iterations, flavour.dtype)
        if form_query and getattr(lib, form_query)(sc, cfg) < 0:
            raise ValueError(refusal)
        scratch = ()
        if workspace_query:
            need = int(getattr(lib, workspace_query)(sc, cfg, 1 if want_observations else 0))
            if need == 0 and not form_query:
                raise ValueError(refusal)
            ws = _scratch(need, dev) if need else None
            scratch = (N.ptr(ws), need)
        gx = torch.empty_like(x_out_grad)
        gobs = torch.empty_like(observations) if want_observations else _empty0(x_out_grad)
        with torch.cuda.device(dev):
            N.check(getattr(lib, symbol)(sc, cfg, N.ptr(tape) if tape.numel() else None, tape.nbytes,
                                         N.ptr(x_out_grad), N.ptr(gx), N.ptr(gobs) if want_observations else None,
                                         *scratch, N.stream_of(dev)), symbol)
        return gx, gobs

    op.__doc__ = doc
    op.register_fake(_sgd_backward_fake)
    return op


def _sgd_backward_fake(x_out_grad, tape, observations, visibility, num_views, num_points, distortion, learning_rate,
                       iterations, residual, want_observations):
    return (torch.empty_like(x_out_grad),
            torch.empty_like(observations) if want_observations else x_out_grad.new_empty((0,)))


ba_sgd_backward = _sgd_backward_op(
    "ba_sgd_backward",
    "``dava_ba_sgd_backward``: (dL/dx0, dL/dobs or empty) of a recorded descent for dL/dx_out.",
    _F32, "the gradient descent's adjoint")
ba_sgd_backward_large = _sgd_backward_op(
    "ba_sgd_backward_large", "``dava_ba_sgd_backward_large``: ``ba_sgd_backward`` for a scene of any size.",
    _F32, "the gradient descent's adjoint", "dava_ba_sgd_backward_large_workspace_bytes",
    refusal=_SGD_ADJOINT_REFUSAL_LARGE)
ba_sgd_backward_f64 = _sgd_backward_op(
    "ba_sgd_backward_f64",
    "``dava_ba_sgd_backward_f64``: (dL/dx0, dL/dobs or empty) of a recorded float64 descent for dL/dx_out.",
    _F64, "the float64 gradient descent's adjoint", "dava_ba_sgd_backward_workspace_bytes_f64",
    "dava_ba_sgd_backward_form_f64", _SGD_ADJOINT_REFUSAL_F64)


def _sgd_record_op(name: str, doc: str, flavour: _Flavour, what: str, symbol: str, adjoint, has_adjoint,
                   refusal: str, unsupported_is_refusal: bool = False, workspace: bool = False):
    """``has_adjoint(lib, scene, config)`` is asked before anything is allocated and ``refusal`` raised where it is
    false; ``adjoint`` is the operator the backward calls.  ``unsupported_is_refusal``: the launch's
    ``DAVA_ERR_UNSUPPORTED`` becomes ``_SGD_REFUSAL``.  ``workspace``: the forward's, as in :func:`_sgd_solve_op`."""

    @torch.library.custom_op(f"dava::{name}", mutates_args=(), device_types=_CUDA)
    def op(x0: Tensor, observations: Tensor, visibility: Tensor, num_views: int, num_points: int, distortion: bool,
           learning_rate: float, iterations: int, residual: int, want_errors: bool) -> Tuple[Tensor, Tensor, Tensor]:
        lib = N.load_library()
        sc, cfg = _sgd_scene(flavour, x0, observations, visibility, num_views, num_points, distortion, learning_rate,
                             iterations, residual, what)
        if not has_adjoint(lib, sc, cfg):
            raise ValueError(refusal)
        b, dev = x0.shape[0], x0.device
        scratch = ()
        if workspace:
            _ws, *scratch = _sgd_solve_workspace_f64(lib, sc, cfg, dev)
        tape = torch.empty((b, iterations, sgd_tape_rows(x0.shape[1])), device=dev, dtype=flavour.dtype)
        if _POISON:
            tape.fill_(float("nan"))
        x_out = torch.empty_like(x0)
        errs = torch.empty((b, iterations), device=dev, dtype=flavour.dtype) if want_errors else _empty0(x0)
        with torch.cuda.device(dev):
            status = getattr(lib, symbol)(sc, cfg, N.ptr(x0), N.ptr(x_out), N.ptr(errs) if want_errors else None,
                                          N.ptr(tape) if tape.numel() else None, tape.nbytes, *scratch,
                                          N.stream_of(dev))
        if unsupported_is_refusal and status == N.DAVA_ERR_UNSUPPORTED:
            raise ValueError(_SGD_REFUSAL)
        N.check(status, symbol)
        return x_out, errs, tape

    @torch.autograd.function.once_differentiable
    def backward(ctx, x_grad, _errors_grad, _tape_grad):
        tape, observations, visibility = ctx.saved_tensors
        need_x, need_obs = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        x_grad = x_grad.to(flavour.dtype)
        gx, gobs = adjoint(x_grad if x_grad.is_contiguous() else x_grad.contiguous(), tape, observations.detach(),
                           visibility, *ctx.meta, bool(need_obs))
        return (gx if need_x else None, gobs if need_obs else None) + (None,) * 8

    op.__doc__ = doc
    op.register_fake(_sgd_record_fake)
    op.register_autograd(backward, setup_context=_sgd_setup_context)
    return op


def _sgd_record_fake(x0, observations, visibility, num_views, num_points, distortion, learning_rate, iterations,
                     residual, want_errors):
    b = x0.shape[0]
    return (torch.empty_like(x0), x0.new_empty((b, iterations) if want_errors else (0,)),
            x0.new_empty((b, iterations, sgd_tape_rows(x0.shape[1]))))


def _sgd_setup_context(ctx, inputs, output):
    x0, observations, visibility, num_views, num_points, distortion, learning_rate, iterations, residual, _ = inputs
    ctx.save_for_backward(output[2], observations, visibility)
    ctx.meta = (num_views, num_points, distortion, learning_rate, iterations, residual)


ba_sgd_solve_differentiable = _sgd_record_op(
    "ba_sgd_solve_differentiable",
    """``dava_ba_sgd_solve_record``: ``ba_sgd_solve`` (bitwise its x and errors) that also writes the tape
    (B, iterations, round_up(P, 4)) of x_k.  An autograd node w.r.t. x0 and the observations: its backward is
    ``ba_sgd_backward`` (not differentiable twice).  Returns (x, errors or empty, tape).""",
    _F32, "the recording gradient descent", "dava_ba_sgd_solve_record", ba_sgd_backward,
    lambda lib, sc, cfg: lib.dava_ba_sgd_backward_supported(sc, cfg),
    "this scene has no fused adjoint of the gradient descent: its dual-number image must fit one workgroup's 160 KiB "
    "of LDS")
ba_sgd_solve_differentiable_large = _sgd_record_op(
    "ba_sgd_solve_differentiable_large",
    """``ba_sgd_solve_differentiable`` for a scene of any size the recording descent runs: the same recording
    launch and tape; its backward is ``ba_sgd_backward_large`` (not differentiable twice).""",
    _F32, "the recording gradient descent", "dava_ba_sgd_solve_record", ba_sgd_backward_large,
    lambda lib, sc, cfg: lib.dava_ba_sgd_backward_form(sc, cfg) >= 0, _SGD_ADJOINT_REFUSAL_LARGE,
    unsupported_is_refusal=True)
ba_sgd_solve_differentiable_f64 = _sgd_record_op(
    "ba_sgd_solve_differentiable_f64",
    """``dava_ba_sgd_solve_record_f64``: ``ba_sgd_solve_f64`` (bitwise its x and errors) that also writes the tape
    (B, iterations, round_up(P, 4)) of x_k in float64.  An autograd node w.r.t. x0 and the observations: its backward
    is ``ba_sgd_backward_f64`` (not differentiable twice).  Returns (x, errors or empty, tape).""",
    _F64, "the float64 recording gradient descent", "dava_ba_sgd_solve_record_f64", ba_sgd_backward_f64,
    lambda lib, sc, cfg: lib.dava_ba_sgd_backward_form_f64(sc, cfg) >= 0, _SGD_ADJOINT_REFUSAL_F64, workspace=True)


# ---------------------------------------- routing between an operator and its `*_large` form

def f32_old_symbol_runs(probe) -> bool:
    """:func:`f64_old_symbol_runs` for the float32 dual-number kernels and their F32_DUAL_FORM override."""
    return N.library_knob("F32_DUAL_FORM") <= 0 and bool(probe())


# ---------------------------------------- float64 recording solve and adjoint
# Operators of their own: ba_solve_record and ba_solve_backward stay float32 only.  Each comes as a pair with one
# body and one fake kernel: `*_f64` keeps one problem's whole image in LDS (160 KiB), keeps its limits and error
# texts and ignores the F64_FORM override; `*_large_f64` takes any scene size (forms 1 and 2 beyond the LDS image; a
# scene whose image fits runs the launch of the first) and differs in the C symbols, one scratch buffer and the
# refusal text.

def tape_bytes_f64(batch: int, p: int, iterations: int) -> int:
    """csrc/dava_tape.hpp's layout with 8-byte elements (what ``dava_ba_solve_tape_bytes_f64`` returns where the
    solve runs): a function of the shapes alone, so the fake kernel needs no data-dependent size."""
    k = max(int(iterations), 1)
    pv = (p + 3) // 4 * 4
    return 8 * batch * (2 * max(k - 1, 1) * pv + 2 * k * pv + (3 * k + 1 + 3) // 4 * 4) + 256


def _solve_record_f64_op(name: str, doc: str, symbol: str, tape_query: str, refusal: str,
                         workspace_query: Optional[str] = None):
    @torch.library.custom_op(f"dava::{name}", mutates_args=(), device_types=_CUDA)
    def op(x0: Tensor, observations: Tensor, visibility: Tensor, num_views: int, num_points: int, distortion: bool,
           sufficient_decrease: float, curvature: float, error_threshold: float, iterations: int,
           minimum_step: float, max_line_search_trials: int, strong: bool, residual: int, want_error: bool = False,
           drop_path_p: float = 0.0, drop_seed: int = 0,
           return_second_last: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        lib = N.load_library()
        _require_float64(x0, "the float64 recording solve")
        _check_scene_tensors(x0, observations, visibility, num_views, num_points, distortion)
        b, dev = x0.shape[0], x0.device
        sc = scene_struct_f64(observations, visibility, num_views, num_points, distortion, b, residual)
        cfg = solver_config_f64(sufficient_decrease, curvature, error_threshold, iterations, minimum_step,
                                max_line_search_trials, strong)
        train = training_f64(drop_path_p, drop_seed, return_second_last)
        need = int(getattr(lib, tape_query)(sc, cfg))
        if need == 0:
            raise ValueError(refusal)
        tape = torch.empty(need, dtype=torch.uint8, device=dev)
        if _POISON:
            tape.fill_(0xFF)
        scratch = ()
        if workspace_query:  # form 2's vectors
            ws = _scratch(int(getattr(lib, workspace_query)(sc, cfg)), dev)
            scratch = (N.ptr(ws), ws.numel())
        x_out = torch.empty_like(x0)
        err = torch.empty(b, device=dev, dtype=torch.float64) if want_error else _empty0(x0)
        status = torch.empty((b, N.STATUS_WORDS), device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            N.check(getattr(lib, symbol)(sc, cfg, train, N.ptr(x0), N.ptr(x_out), N.ptr(err) if want_error else None,
                                         N.ptr(status), N.ptr(tape), tape.numel(), *scratch, N.stream_of(dev)),
                    symbol)
        return x_out, status, tape, err

    op.__doc__ = doc
    op.register_fake(_solve_record_f64_fake)
    return op


def _solve_record_f64_fake(x0, observations, visibility, num_views, num_points, distortion, sufficient_decrease,
                           curvature, error_threshold, iterations, minimum_step, max_line_search_trials, strong,
                           residual, want_error=False, drop_path_p=0.0, drop_seed=0, return_second_last=False):
    b = x0.shape[0]
    return (torch.empty_like(x0), x0.new_empty((b, N.STATUS_WORDS), dtype=torch.int32),
            x0.new_empty((tape_bytes_f64(b, x0.shape[1], iterations),), dtype=torch.uint8),
            x0.new_empty((b,) if want_error else (0,)))


ba_solve_record_f64 = _solve_record_f64_op(
    "ba_solve_record_f64",
    """``dava_ba_solve_record_train_f64``: the float64 fused solve (bitwise ``ba_solve``'s x, error and status on a
    float64 batch, training-mode arguments included) plus the float64 tape.
    Returns (x, status (B, 4) int32, tape uint8, error (B,) or empty).""",
    "dava_ba_solve_record_train_f64", "dava_ba_solve_tape_bytes_f64",
    "this scene / configuration has no float64 fused solve (the LDS image must fit 160 KiB, 1 <= iterations <= 1025)")
ba_solve_record_large_f64 = _solve_record_f64_op(
    "ba_solve_record_large_f64",
    """``dava_ba_solve_record_large_f64``: ``ba_solve_record_f64`` for a scene of any size (the same tape).
    Returns (x, status (B, 4) int32, tape uint8, error (B,) or empty).""",
    "dava_ba_solve_record_large_f64", "dava_ba_solve_tape_bytes_large_f64",
    "this scene / configuration has no float64 fused solve (1 <= iterations <= 1025, at most 251 views at 1025 "
    "iterations)", "dava_ba_solve_record_large_workspace_bytes_f64")


def _solve_backward_f64_op(name: str, doc: str, tape_query: str, workspace_query: str, refusal: str):
    symbol = f"dava_{name}"

    @torch.library.custom_op(f"dava::{name}", mutates_args=(), device_types=_CUDA)
    def op(x_out_grad: Tensor, tape: Tensor, status: Tensor, observations: Tensor, visibility: Tensor,
           num_views: int, num_points: int, distortion: bool, iterations: int, residual: int,
           want_observations: bool) -> Tuple[Tensor, Tensor]:
        lib = N.load_library()
        _require_float64(x_out_grad, "the float64 fused solve's adjoint")
        _check_scene_tensors(x_out_grad, observations, visibility, num_views, num_points, distortion)
        b, dev = x_out_grad.shape[0], x_out_grad.device
        if tuple(status.shape) != (b, N.STATUS_WORDS) or status.dtype != torch.int32 or not status.is_contiguous():
            raise ValueError("status must be the recording call's contiguous (B, 4) int32 tensor")
        # the kernel dereferences tape and status as device memory of this launch: refuse anything else loudly
        for what, t in (("tape", tape), ("status", status)):
            if t.device != dev:
                raise ValueError(f"{what} must be on {dev} (the cotangent's device), got {t.device}")
        if tape.dtype != torch.uint8 or tape.dim() != 1 or not tape.is_contiguous():
            raise ValueError("tape must be the recording call's contiguous 1-D uint8 tensor")
        sc = scene_struct_f64(observations, visibility, num_views, num_points, distortion, b, residual)
        cfg = solver_config_f64(1e-4, 0.9, 1e-4, iterations, 1e-8, 1000, True)
        tape_need = int(getattr(lib, tape_query)(sc, cfg))
        need = int(getattr(lib, workspace_query)(sc, cfg))
        if need == 0 or tape_need == 0:
            raise ValueError(refusal)
        if tape.numel() < tape_need:
            raise ValueError(f"tape holds {tape.numel()} bytes; a recording of this scene and iteration count "
                             f"writes {tape_need}")
        ws = _scratch(need, dev)
        gx = torch.empty_like(x_out_grad)
        gobs = torch.empty_like(observations) if want_observations else _empty0(x_out_grad)
        with torch.cuda.device(dev):
            N.check(getattr(lib, symbol)(sc, cfg, N.ptr(tape), tape.numel(), N.ptr(status), N.ptr(x_out_grad),
                                         N.ptr(gx), N.ptr(gobs) if want_observations else None, N.ptr(ws), ws.numel(),
                                         N.stream_of(dev)), symbol)
        return gx, gobs

    op.__doc__ = doc
    op.register_fake(_solve_backward_f64_fake)
    return op


def _solve_backward_f64_fake(x_out_grad, tape, status, observations, visibility, num_views, num_points, distortion,
                             iterations, residual, want_observations):
    return (torch.empty_like(x_out_grad),
            torch.empty_like(observations) if want_observations else x_out_grad.new_empty((0,)))


ba_solve_backward_f64 = _solve_backward_f64_op(
    "ba_solve_backward_f64",
    "``dava_ba_solve_backward_f64``: (dL/dx0, dL/dobs or empty) of a recorded float64 solve for dL/dx_out.",
    "dava_ba_solve_tape_bytes_f64", "dava_ba_solve_backward_workspace_bytes_f64",
    "this scene / configuration has no float64 fused adjoint")
ba_solve_backward_large_f64 = _solve_backward_f64_op(
    "ba_solve_backward_large_f64",
    "``dava_ba_solve_backward_large_f64``: ``ba_solve_backward_f64`` for a scene of any size.",
    "dava_ba_solve_tape_bytes_large_f64", "dava_ba_solve_backward_large_workspace_bytes_f64",
    "this scene / configuration has no float64 fused adjoint (1 <= iterations <= 1025, the dual view constants must "
    "fit LDS)")


# ------------------------------------------------- generic BFGS building blocks

def _square_batch(h: Tensor) -> Tuple[int, int]:
    # the kernels (GPU and host) read raw row-major pointers: a transposed or sliced view would be
    # computed on the wrong layout, and empty_like would copy its strides into the outputs
    if h.dim() != 3 or h.shape[1] != h.shape[2] or not h.is_contiguous():
        raise ValueError(f"expected a contiguous (B, n, n) batch of matrices, got {tuple(h.shape)} "
                         f"(contiguous={h.is_contiguous()})")
    return h.shape[0], h.shape[1]


def _row_batch(t: Tensor, what: str) -> Tuple[int, int]:
    """The primary (B, n) operand of an op: contiguous, for the same reason as _square_batch."""
    if t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous (B, n) batch, got {tuple(t.shape)} "
                         f"(contiguous={t.is_contiguous()})")
    return t.shape[0], t.shape[1]


def _expect(t: Tensor, like: Tensor, shape, what: str) -> None:
    if tuple(t.shape) != tuple(shape) or t.dtype != like.dtype or t.device != like.device or not t.is_contiguous():
        raise ValueError(f"{what}: expected contiguous {like.dtype} {tuple(shape)} on {like.device}, "
                         f"got {t.dtype} {tuple(t.shape)} on {t.device}")


@torch.library.custom_op("dava::bfgs_update_inverse_hessian", mutates_args=(), device_types=_CUDA)
def bfgs_update_inverse_hessian(h: Tensor, s: Tensor, y: Tensor) -> Tensor:
    """(B, n, n), (B, n), (B, n) -> H+ (``bfgs_solver.py:235-303``)."""
    b, n = _square_batch(h)
    _expect(s, h, (b, n), "step")
    _expect(y, h, (b, n), "delta_gradient")
    out = torch.empty_like(h)
    with torch.cuda.device(h.device):
        N.check(getattr(N.load_library(), f"dava_bfgs_update_inverse_hessian_{_dt(h)}")(
            b, n, N.ptr(h), N.ptr(s), N.ptr(y), N.ptr(out), N.stream_of(h.device)), "dava_bfgs_update_inverse_hessian")
    return out


@bfgs_update_inverse_hessian.register_fake
def _(h, s, y):
    return torch.empty_like(h)


_UPDATE_BACKWARD_VECTORS, _UPDATE_BACKWARD_LDS_BYTES = 9, 150 * 1024  # update_backward (csrc/bfgs_grad.hip)


@torch.library.custom_op("dava::bfgs_update_inverse_hessian_backward", mutates_args=(), device_types=_CUDA)
def bfgs_update_inverse_hessian_backward(h: Tensor, s: Tensor, y: Tensor, grad: Tensor, need_h: bool, need_s: bool,
                                         need_y: bool) -> Tuple[Tensor, Tensor, Tensor]:
    b, n = _square_batch(h)
    _expect(grad, h, (b, n, n), "grad")
    gh = torch.empty_like(h) if need_h else _empty0(h)
    gs = torch.empty_like(s) if need_s else _empty0(h)
    gy = torch.empty_like(y) if need_y else _empty0(h)
    lib = N.load_library()
    outs = (N.ptr(gh) if need_h else None, N.ptr(gs) if need_s else None, N.ptr(gy) if need_y else None)
    with torch.cuda.device(h.device):
        if h.dtype == torch.float64 and _UPDATE_BACKWARD_VECTORS * n * 8 > _UPDATE_BACKWARD_LDS_BYTES:
            # beyond the LDS image of the float64 kernel (n > 2133): its nine vectors in a workspace
            ws = torch.empty(b * _UPDATE_BACKWARD_VECTORS * n * 8 + 256, dtype=torch.uint8, device=h.device)
            if _POISON:
                ws.fill_(0xFF)
            N.check(lib.dava_bfgs_update_inverse_hessian_backward_large_f64(
                b, n, N.ptr(h), N.ptr(s), N.ptr(y), N.ptr(grad), *outs, N.ptr(ws), ws.numel(),
                N.stream_of(h.device)), "dava_bfgs_update_inverse_hessian_backward_large_f64")
        else:
            N.check(getattr(lib, f"dava_bfgs_update_inverse_hessian_backward_{_dt(h)}")(
                b, n, N.ptr(h), N.ptr(s), N.ptr(y), N.ptr(grad), *outs, N.stream_of(h.device)),
                "dava_bfgs_update_inverse_hessian_backward")
    return gh, gs, gy


@bfgs_update_inverse_hessian_backward.register_fake
def _(h, s, y, grad, need_h, need_s, need_y):
    return (torch.empty_like(h) if need_h else h.new_empty((0,)), torch.empty_like(s) if need_s else h.new_empty((0,)),
            torch.empty_like(y) if need_y else h.new_empty((0,)))


@torch.library.custom_op("dava::bfgs_initial_scale", mutates_args=(), device_types=_CUDA)
def bfgs_initial_scale(s: Tensor, y: Tensor) -> Tensor:
    """(B, n), (B, n) -> gamma (B,) (``bfgs_solver.py:217-233``)."""
    b, n = _row_batch(s, "step")
    _expect(y, s, (b, n), "delta_gradient")
    out = s.new_empty((b,))
    with torch.cuda.device(s.device):
        N.check(getattr(N.load_library(), f"dava_bfgs_initial_scale_{_dt(s)}")(
            b, n, N.ptr(s), N.ptr(y), N.ptr(out), N.stream_of(s.device)), "dava_bfgs_initial_scale")
    return out


@bfgs_initial_scale.register_fake
def _(s, y):
    return s.new_empty((s.shape[0],))


@torch.library.custom_op("dava::bfgs_initial_scale_backward", mutates_args=(), device_types=_CUDA)
def bfgs_initial_scale_backward(s: Tensor, y: Tensor, grad: Tensor, need_s: bool,
                                need_y: bool) -> Tuple[Tensor, Tensor]:
    b, n = _row_batch(s, "step")
    _expect(grad, s, (b,), "grad")
    gs = torch.empty_like(s) if need_s else _empty0(s)
    gy = torch.empty_like(y) if need_y else _empty0(s)
    with torch.cuda.device(s.device):
        N.check(getattr(N.load_library(), f"dava_bfgs_initial_scale_backward_{_dt(s)}")(
            b, n, N.ptr(s), N.ptr(y), N.ptr(grad), N.ptr(gs) if need_s else None, N.ptr(gy) if need_y else None,
            N.stream_of(s.device)), "dava_bfgs_initial_scale_backward")
    return gs, gy


@bfgs_initial_scale_backward.register_fake
def _(s, y, grad, need_s, need_y):
    return (torch.empty_like(s) if need_s else s.new_empty((0,)), torch.empty_like(y) if need_y else s.new_empty((0,)))


@torch.library.custom_op("dava::bfgs_scale_matrix", mutates_args=(), device_types=_CUDA)
def bfgs_scale_matrix(scale: Tensor, h: Tensor) -> Tensor:
    """scale (B,) * H (B, n, n): the k == 1 rescale of H0 (``bfgs_solver.py:159-167``)."""
    b, n = _square_batch(h)
    _expect(scale, h, (b,), "scale")
    out = torch.empty_like(h)
    with torch.cuda.device(h.device):
        N.check(getattr(N.load_library(), f"dava_bfgs_scale_matrix_{_dt(h)}")(
            b, n, N.ptr(scale), N.ptr(h), N.ptr(out), N.stream_of(h.device)), "dava_bfgs_scale_matrix")
    return out


@bfgs_scale_matrix.register_fake
def _(scale, h):
    return torch.empty_like(h)


@torch.library.custom_op("dava::bfgs_scale_matrix_backward", mutates_args=(), device_types=_CUDA)
def bfgs_scale_matrix_backward(scale: Tensor, h: Tensor, grad: Tensor, need_scale: bool,
                               need_h: bool) -> Tuple[Tensor, Tensor]:
    b, n = _square_batch(h)
    _expect(grad, h, (b, n, n), "grad")
    gsc = torch.empty_like(scale) if need_scale else _empty0(h)
    gh = torch.empty_like(h) if need_h else _empty0(h)
    with torch.cuda.device(h.device):
        N.check(getattr(N.load_library(), f"dava_bfgs_scale_matrix_backward_{_dt(h)}")(
            b, n, N.ptr(scale), N.ptr(h), N.ptr(grad), N.ptr(gsc) if need_scale else None,
            N.ptr(gh) if need_h else None, N.stream_of(h.device)), "dava_bfgs_scale_matrix_backward")
    return gsc, gh


@bfgs_scale_matrix_backward.register_fake
def _(scale, h, grad, need_scale, need_h):
    return (torch.empty_like(scale) if need_scale else h.new_empty((0,)),
            torch.empty_like(h) if need_h else h.new_empty((0,)))


@torch.library.custom_op("dava::bfgs_search_direction", mutates_args=(), device_types=_CUDA)
def bfgs_search_direction(h: Tensor, g: Tensor) -> Tensor:
    """d = -H g (``bfgs_solver.py:173-176``)."""
    b, n = _square_batch(h)
    _expect(g, h, (b, n), "gradient")
    out = torch.empty_like(g)
    with torch.cuda.device(h.device):
        N.check(getattr(N.load_library(), f"dava_bfgs_search_direction_{_dt(h)}")(
            b, n, N.ptr(h), N.ptr(g), N.ptr(out), N.stream_of(h.device)), "dava_bfgs_search_direction")
    return out


@bfgs_search_direction.register_fake
def _(h, g):
    return torch.empty_like(g)


@torch.library.custom_op("dava::bfgs_compact_direction",
                         mutates_args=("history_s", "history_w", "history_rho", "history_c", "gamma"),
                         device_types=_CUDA)
def bfgs_compact_direction(g: Tensor, y: Tensor, s: Tensor, problem_index: Tensor, count: int, history_s: Tensor,
                           history_w: Tensor, history_rho: Tensor, history_c: Tensor, gamma: Tensor) -> Tensor:
    """The generic loop's update + search direction on compact history rows (no dense matrix): appends
    entry ``count`` to the history of the problems ``problem_index`` and returns d = -H g (n_active, P)."""
    n_act, p = _row_batch(g, "gradient")
    _expect(y, g, (n_act, p), "delta_gradient")
    _expect(s, g, (n_act, p), "step")
    if problem_index.dtype != torch.int64 or tuple(problem_index.shape) != (n_act,) \
            or problem_index.device != g.device or not problem_index.is_contiguous():
        raise ValueError("problem_index must be a contiguous int64 (n_active,) tensor on the gradient's device")
    if history_s.dim() != 3 or history_w.shape != history_s.shape or history_s.dtype != g.dtype \
            or history_w.dtype != g.dtype or history_s.shape[2] < p:
        raise ValueError("history rows must be (B, capacity, >= P) in the gradient's dtype")
    b_all, cap, stride = history_s.shape
    for t, shape, what in ((history_rho, (b_all, cap), "history_rho"), (history_c, (b_all, cap), "history_c"),
                           (gamma, (b_all,), "gamma")):
        if tuple(t.shape) != shape or t.dtype != g.dtype:
            raise ValueError(f"{what} must be {shape} in the gradient's dtype")
    for t in (history_s, history_w, history_rho, history_c, gamma):
        if not t.is_contiguous() or t.device != g.device:
            raise ValueError("history tensors must be contiguous and on the gradient's device")
    if not 0 <= count < cap:
        raise ValueError(f"count {count} outside the history capacity {cap}")
    out = torch.empty_like(g)
    with torch.cuda.device(g.device):
        N.check(getattr(N.load_library(), f"dava_bfgs_compact_direction_{_dt(g)}")(
            n_act, p, stride, cap, count, N.ptr(problem_index), N.ptr(g), N.ptr(y), N.ptr(s), N.ptr(history_s),
            N.ptr(history_w), N.ptr(history_rho), N.ptr(history_c), N.ptr(gamma), N.ptr(out),
            N.stream_of(g.device)), "dava_bfgs_compact_direction")
    return out


@bfgs_compact_direction.register_fake
def _(g, y, s, problem_index, count, history_s, history_w, history_rho, history_c, gamma):
    return torch.empty_like(g)


@torch.library.custom_op("dava::bfgs_search_direction_backward", mutates_args=(), device_types=_CUDA)
def bfgs_search_direction_backward(h: Tensor, g: Tensor, grad: Tensor, need_h: bool,
                                   need_g: bool) -> Tuple[Tensor, Tensor]:
    b, n = _square_batch(h)
    _expect(grad, h, (b, n), "grad")
    gh = torch.empty_like(h) if need_h else _empty0(h)
    gg = torch.empty_like(g) if need_g else _empty0(h)
    with torch.cuda.device(h.device):
        N.check(getattr(N.load_library(), f"dava_bfgs_search_direction_backward_{_dt(h)}")(
            b, n, N.ptr(h), N.ptr(g), N.ptr(grad), N.ptr(gh) if need_h else None, N.ptr(gg) if need_g else None,
            N.stream_of(h.device)), "dava_bfgs_search_direction_backward")
    return gh, gg


@bfgs_search_direction_backward.register_fake
def _(h, g, grad, need_h, need_g):
    return (torch.empty_like(h) if need_h else h.new_empty((0,)), torch.empty_like(g) if need_g else h.new_empty((0,)))


# ------------------------------------------------------- batched Wolfe state machine

WOLFE_STATE_COLUMNS = 9
WOLFE_FLAG_COLUMNS = 2


@torch.library.custom_op("dava::wolfe_init", mutates_args=(), device_types=_CUDA)
def wolfe_init(direction: Tensor, f0: Tensor, g0: Tensor) -> Tuple[Tensor, Tensor]:
    """(state (B, 9), flags (B, 2) uint8) for a line search along ``direction`` from (f0, g0)."""
    b, n = _row_batch(direction, "search_direction")
    _expect(g0, direction, (b, n), "base_gradient")
    _expect(f0, direction, (b,), "base_error")
    state = direction.new_empty((b, WOLFE_STATE_COLUMNS))
    flags = direction.new_empty((b, WOLFE_FLAG_COLUMNS), dtype=torch.uint8)
    with torch.cuda.device(direction.device):
        N.check(getattr(N.load_library(), f"dava_wolfe_init_{_dt(direction)}")(
            b, n, N.ptr(direction), N.ptr(f0), N.ptr(g0), N.ptr(state), N.ptr(flags), N.stream_of(direction.device)),
            "dava_wolfe_init")
    return state, flags


@wolfe_init.register_fake
def _(direction, f0, g0):
    b = direction.shape[0]
    return direction.new_empty((b, WOLFE_STATE_COLUMNS)), direction.new_empty((b, WOLFE_FLAG_COLUMNS),
                                                                               dtype=torch.uint8)


def _check_wolfe(state: Tensor, flags: Tensor) -> int:
    b = state.shape[0]
    if tuple(state.shape) != (b, WOLFE_STATE_COLUMNS) or tuple(flags.shape) != (b, WOLFE_FLAG_COLUMNS) \
            or flags.dtype != torch.uint8 or not state.is_contiguous() or not flags.is_contiguous():
        raise ValueError("Wolfe state must be (B, 9) and flags (B, 2) uint8, contiguous")
    return b


@torch.library.custom_op("dava::wolfe_propose", mutates_args=("state",), device_types=_CUDA)
def wolfe_propose(state: Tensor, flags: Tensor) -> None:
    """Next trial alpha of every active line search (widen x2 or bisect), in place."""
    b = _check_wolfe(state, flags)
    with torch.cuda.device(state.device):
        N.check(getattr(N.load_library(), f"dava_wolfe_propose_{_dt(state)}")(
            b, N.ptr(state), N.ptr(flags), N.stream_of(state.device)), "dava_wolfe_propose")


@wolfe_propose.register_fake
def _(state, flags):
    return None


@torch.library.custom_op("dava::wolfe_update", mutates_args=("state", "flags"), device_types=_CUDA)
def wolfe_update(state: Tensor, flags: Tensor, trial: int, c1: float, c2: float, strong: bool) -> None:
    """Consume (f(alpha), phi'(alpha)) already written into ``state`` and advance the brackets."""
    b = _check_wolfe(state, flags)
    with torch.cuda.device(state.device):
        N.check(getattr(N.load_library(), f"dava_wolfe_update_{_dt(state)}")(
            b, int(trial), float(c1), float(c2), 1 if strong else 0, N.ptr(state), N.ptr(flags),
            N.stream_of(state.device)), "dava_wolfe_update")


@wolfe_update.register_fake
def _(state, flags, trial, c1, c2, strong):
    return None


# ------------------------------------------------ the same building blocks on CPU tensors
# The reference's solver runs wherever `parameters` live (bfgs_solver.py:94-117; BASELINE C1 is "BFGS on
# PyTorch CPU").  These CPU kernels call the host C++ flavours of the same library (csrc/bfgs_host.hip,
# dava_cpu_*): explicit dispatch on the tensor's device, never a fallback for device tensors (a ROCm
# tensor still goes to the HIP kernels and raises without them).  The fused BA objectives stay GPU-only.

def _cpu(name: str, t: Tensor, *args) -> None:
    N.check(getattr(N.load_library(), f"dava_cpu_{name}_{_dt(t)}")(*args), f"dava_cpu_{name}")


def _cpu_ptr(t: Optional[Tensor]):
    return None if t is None else N.ptr(t)


@bfgs_update_inverse_hessian.register_kernel("cpu")
def _(h, s, y):
    b, n = _square_batch(h)
    _expect(s, h, (b, n), "step")
    _expect(y, h, (b, n), "delta_gradient")
    out = torch.empty_like(h)
    _cpu("bfgs_update_inverse_hessian", h, b, n, N.ptr(h), N.ptr(s), N.ptr(y), N.ptr(out))
    return out


@bfgs_update_inverse_hessian_backward.register_kernel("cpu")
def _(h, s, y, grad, need_h, need_s, need_y):
    b, n = _square_batch(h)
    _expect(grad, h, (b, n, n), "grad")
    gh = torch.empty_like(h) if need_h else _empty0(h)
    gs = torch.empty_like(s) if need_s else _empty0(h)
    gy = torch.empty_like(y) if need_y else _empty0(h)
    _cpu("bfgs_update_inverse_hessian_backward", h, b, n, N.ptr(h), N.ptr(s), N.ptr(y), N.ptr(grad),
         _cpu_ptr(gh if need_h else None), _cpu_ptr(gs if need_s else None), _cpu_ptr(gy if need_y else None))
    return gh, gs, gy


@bfgs_initial_scale.register_kernel("cpu")
def _(s, y):
    b, n = _row_batch(s, "step")
    _expect(y, s, (b, n), "delta_gradient")
    out = s.new_empty((b,))
    _cpu("bfgs_initial_scale", s, b, n, N.ptr(s), N.ptr(y), N.ptr(out))
    return out


@bfgs_initial_scale_backward.register_kernel("cpu")
def _(s, y, grad, need_s, need_y):
    b, n = _row_batch(s, "step")
    _expect(grad, s, (b,), "grad")
    gs = torch.empty_like(s) if need_s else _empty0(s)
    gy = torch.empty_like(y) if need_y else _empty0(s)
    _cpu("bfgs_initial_scale_backward", s, b, n, N.ptr(s), N.ptr(y), N.ptr(grad), _cpu_ptr(gs if need_s else None),
         _cpu_ptr(gy if need_y else None))
    return gs, gy


@bfgs_scale_matrix.register_kernel("cpu")
def _(scale, h):
    b, n = _square_batch(h)
    _expect(scale, h, (b,), "scale")
    out = torch.empty_like(h)
    _cpu("bfgs_scale_matrix", h, b, n, N.ptr(scale), N.ptr(h), N.ptr(out))
    return out


@bfgs_scale_matrix_backward.register_kernel("cpu")
def _(scale, h, grad, need_scale, need_h):
    b, n = _square_batch(h)
    _expect(grad, h, (b, n, n), "grad")
    gsc = torch.empty_like(scale) if need_scale else _empty0(h)
    gh = torch.empty_like(h) if need_h else _empty0(h)
    _cpu("bfgs_scale_matrix_backward", h, b, n, N.ptr(scale), N.ptr(h), N.ptr(grad),
         _cpu_ptr(gsc if need_scale else None), _cpu_ptr(gh if need_h else None))
    return gsc, gh


@bfgs_search_direction.register_kernel("cpu")
def _(h, g):
    b, n = _square_batch(h)
    _expect(g, h, (b, n), "gradient")
    out = torch.empty_like(g)
    _cpu("bfgs_search_direction", h, b, n, N.ptr(h), N.ptr(g), N.ptr(out))
    return out


@bfgs_search_direction_backward.register_kernel("cpu")
def _(h, g, grad, need_h, need_g):
    b, n = _square_batch(h)
    _expect(grad, h, (b, n), "grad")
    gh = torch.empty_like(h) if need_h else _empty0(h)
    gg = torch.empty_like(g) if need_g else _empty0(h)
    _cpu("bfgs_search_direction_backward", h, b, n, N.ptr(h), N.ptr(g), N.ptr(grad), _cpu_ptr(gh if need_h else None),
         _cpu_ptr(gg if need_g else None))
    return gh, gg


@wolfe_init.register_kernel("cpu")
def _(direction, f0, g0):
    b, n = _row_batch(direction, "search_direction")
    _expect(g0, direction, (b, n), "base_gradient")
    _expect(f0, direction, (b,), "base_error")
    state = direction.new_empty((b, WOLFE_STATE_COLUMNS))
    flags = direction.new_empty((b, WOLFE_FLAG_COLUMNS), dtype=torch.uint8)
    _cpu("wolfe_init", direction, b, n, N.ptr(direction), N.ptr(f0), N.ptr(g0), N.ptr(state), N.ptr(flags))
    return state, flags


@wolfe_propose.register_kernel("cpu")
def _(state, flags):
    b = _check_wolfe(state, flags)
    _cpu("wolfe_propose", state, b, N.ptr(state), N.ptr(flags))


@wolfe_update.register_kernel("cpu")
def _(state, flags, trial, c1, c2, strong):
    b = _check_wolfe(state, flags)
    _cpu("wolfe_update", state, b, int(trial), float(c1), float(c2), 1 if strong else 0, N.ptr(state), N.ptr(flags))


# ------------------------------------------------ legacy L1 camera model evaluation

@torch.library.custom_op("dava::l1_camera_evaluate", mutates_args=(), device_types=_CUDA)
def l1_camera_evaluate(focal: Tensor, cx: Tensor, cy: Tensor, translation: Tensor, lie: Tensor, world: Tensor,
                       target: Tensor, visibility: Tensor, minimum_z_distance: float, maximum_pixel_ratio: float,
                       max_gradient: float, error_scale: float, want_error: bool,
                       want_gradient: bool) -> Tuple[Tensor, Tensor]:
    """``dava_l1_camera_evaluate``: PinholeCameraModelL1 error (B, E) and its hand-written gradient
    (B, E, P) (``camera_model/pinhole_camera_model_l1.py:132-285``).  Shapes: focal/cx/cy (B, E),
    translation/lie (B, E, M, 3), world (B, E, N-2, 3), target (B, M, N, 2), visibility (B, M, N) uint8."""
    b, e = focal.shape
    m, n = target.shape[1], target.shape[2]
    p = 3 + 6 * m + 3 * n - 7
    for t, shape, what in ((cx, (b, e), "cx"), (cy, (b, e), "cy"), (translation, (b, e, m, 3), "translation"),
                           (lie, (b, e, m, 3), "orientation"), (world, (b, e, n - 2, 3), "world_points"),
                           (target, (b, m, n, 2), "true_projected_points")):
        _expect(t, focal, shape, what)
    if tuple(visibility.shape) != (b, m, n) or visibility.dtype != torch.uint8 or not visibility.is_contiguous():
        raise ValueError("visibility must be a contiguous (B, M, N) uint8 tensor")
    err = focal.new_empty((b, e)) if want_error else _empty0(focal)
    grad = focal.new_empty((b, e, p)) if want_gradient else _empty0(focal)
    with torch.cuda.device(focal.device):
        N.check(getattr(N.load_library(), f"dava_l1_camera_evaluate_{_dt(focal)}")(
            b, e, m, n, N.ptr(focal), N.ptr(cx), N.ptr(cy), N.ptr(translation), N.ptr(lie), N.ptr(world),
            N.ptr(target), N.ptr(visibility), minimum_z_distance, maximum_pixel_ratio, max_gradient, error_scale,
            N.ptr(err) if want_error else None, N.ptr(grad) if want_gradient else None, N.stream_of(focal.device)),
            "dava_l1_camera_evaluate")
    return err, grad


@l1_camera_evaluate.register_fake
def _(focal, cx, cy, translation, lie, world, target, visibility, minimum_z_distance, maximum_pixel_ratio,
      max_gradient, error_scale, want_error, want_gradient):
    b, e = focal.shape
    m, n = target.shape[1], target.shape[2]
    return (focal.new_empty((b, e) if want_error else (0,)),
            focal.new_empty((b, e, 3 + 6 * m + 3 * n - 7) if want_gradient else (0,)))


@torch.library.custom_op("dava::l1_camera_vjp", mutates_args=(), device_types=_CUDA)
def l1_camera_vjp(focal: Tensor, cx: Tensor, cy: Tensor, translation: Tensor, lie: Tensor, world: Tensor,
                  target: Tensor, visibility: Tensor, minimum_z_distance: float, maximum_pixel_ratio: float,
                  max_gradient: float, error_scale: float, error_cotangent: Optional[Tensor],
                  gradient_cotangent: Optional[Tensor], detach_points: bool) -> Tensor:
    """``dava_l1_camera_vjp``: the model's inputs' cotangent (B, E, D), D = 3 + 6M + 3(N-2) in the
    order focal, cx, cy, translation (M, 3), lie (M, 3), world (N-2, 3), from the error's (B, E)
    and / or the gradient's (B, E, P) cotangents.  Same input shapes as ``l1_camera_evaluate``."""
    b, e = focal.shape
    m, n = target.shape[1], target.shape[2]
    p = 3 + 6 * m + 3 * n - 7
    for t, shape, what in ((cx, (b, e), "cx"), (cy, (b, e), "cy"), (translation, (b, e, m, 3), "translation"),
                           (lie, (b, e, m, 3), "orientation"), (world, (b, e, n - 2, 3), "world_points"),
                           (target, (b, m, n, 2), "true_projected_points")):
        _expect(t, focal, shape, what)
    if error_cotangent is not None:
        _expect(error_cotangent, focal, (b, e), "error cotangent")
    if gradient_cotangent is not None:
        _expect(gradient_cotangent, focal, (b, e, p), "gradient cotangent")
    if tuple(visibility.shape) != (b, m, n) or visibility.dtype != torch.uint8 or not visibility.is_contiguous():
        raise ValueError("visibility must be a contiguous (B, M, N) uint8 tensor")
    out = focal.new_zeros((b, e, 3 + 6 * m + 3 * (n - 2)))
    if error_cotangent is None and gradient_cotangent is None:
        return out
    with torch.cuda.device(focal.device):
        N.check(getattr(N.load_library(), f"dava_l1_camera_vjp_{_dt(focal)}")(
            b, e, m, n, N.ptr(focal), N.ptr(cx), N.ptr(cy), N.ptr(translation), N.ptr(lie), N.ptr(world),
            N.ptr(target), N.ptr(visibility), minimum_z_distance, maximum_pixel_ratio, max_gradient, error_scale,
            N.ptr(error_cotangent) if error_cotangent is not None else None,
            N.ptr(gradient_cotangent) if gradient_cotangent is not None else None, int(detach_points), N.ptr(out),
            N.stream_of(focal.device)), "dava_l1_camera_vjp")
    return out


@l1_camera_vjp.register_fake
def _(focal, cx, cy, translation, lie, world, target, visibility, minimum_z_distance, maximum_pixel_ratio,
      max_gradient, error_scale, error_cotangent, gradient_cotangent, detach_points):
    b, e = focal.shape
    m, n = target.shape[1], target.shape[2]
    return focal.new_empty((b, e, 3 + 6 * m + 3 * (n - 2)))


# ------------------------------------------------ the legacy solver fused (BFGSCameraSolver + its line search)

def l1_solve_config(max_iterations: int, widen_iterations: int, zoom_iterations: int, constrain: bool,
                    epsilon: float, max_step_distance: float, min_step_distance: float, max_step_size: float,
                    sufficient_decrease: float, curvature: float, slope_scale: float,
                    derived_pixel_ratio: float) -> N.DavaL1SolveConfig:
    return N.DavaL1SolveConfig(int(max_iterations), int(widen_iterations), int(zoom_iterations), int(bool(constrain)),
                               float(max_step_distance), float(min_step_distance), float(derived_pixel_ratio),
                               float(epsilon), float(max_step_size), float(sufficient_decrease), float(curvature),
                               float(slope_scale))


@torch.library.custom_op("dava::l1_camera_solve", mutates_args=(), device_types=_CUDA)
def l1_camera_solve(focal: Tensor, cx: Tensor, cy: Tensor, translation: Tensor, lie: Tensor, world: Tensor,
                    target: Tensor, visibility: Tensor, minimum_z_distance: float, maximum_pixel_ratio: float,
                    max_gradient: float, error_scale: float, max_iterations: int, widen_iterations: int,
                    zoom_iterations: int, constrain: bool, epsilon: float, max_step_distance: float,
                    min_step_distance: float, max_step_size: float, sufficient_decrease: float, curvature: float,
                    slope_scale: float, derived_pixel_ratio: float, want_traces: bool
                    ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """``dava_l1_camera_solve``: ``BFGSCameraSolver.forward`` with ``LineSearchStrongWolfeConditions`` inside it, over
    a ``PinholeCameraModelL1``, in one launch (csrc/camera_l1_solve.hip).  Input shapes as ``l1_camera_evaluate``.
    Returns (focal, cx, cy, translation, lie, world) at the solved point, its error (B, E), the iterations each
    estimate was updated in (B, E) int32, and -- or empty -- the traces (B, E, max_iterations): error, alpha, exit
    (int32).  The inverse Hessian's workspace, where the form needs one, comes from torch's allocator.  Not
    differentiable."""
    b, e = focal.shape
    m, n = target.shape[1], target.shape[2]
    for t, shape, what in ((cx, (b, e), "cx"), (cy, (b, e), "cy"), (translation, (b, e, m, 3), "translation"),
                           (lie, (b, e, m, 3), "orientation"), (world, (b, e, n - 2, 3), "world_points"),
                           (target, (b, m, n, 2), "true_projected_points")):
        _expect(t, focal, shape, what)
    if tuple(visibility.shape) != (b, m, n) or visibility.dtype != torch.uint8 or not visibility.is_contiguous():
        raise ValueError("visibility must be a contiguous (B, M, N) uint8 tensor")
    if max_iterations < 1 or widen_iterations < 0 or zoom_iterations < 0:
        raise ValueError("the fused legacy solve needs max_iterations >= 1 and non-negative trial counts")
    if n < 4:
        raise ValueError("the fused legacy solve needs at least 4 points (add() has no z block at 3)")
    lib = N.load_library()
    dt = _dt(focal)
    if getattr(lib, f"dava_l1_camera_solve_form_{dt}")(m, n) < 0:
        raise ValueError("this scene has no fused legacy solve: its evaluation scratch and solver state do not fit "
                         "one workgroup's LDS")
    cfg = l1_solve_config(max_iterations, widen_iterations, zoom_iterations, constrain, epsilon, max_step_distance,
                          min_step_distance, max_step_size, sufficient_decrease, curvature, slope_scale,
                          derived_pixel_ratio)
    need = int(getattr(lib, f"dava_l1_camera_solve_workspace_bytes_{dt}")(b, e, m, n))
    ws = _scratch(need, focal.device) if need else None
    outs = [torch.empty_like(t) for t in (focal, cx, cy, translation, lie, world)]
    err = focal.new_empty((b, e))
    iters = focal.new_empty((b, e), dtype=torch.int32)
    k = max_iterations
    tr_err = focal.new_empty((b, e, k)) if want_traces else _empty0(focal)
    tr_alpha = focal.new_empty((b, e, k)) if want_traces else _empty0(focal)
    tr_exit = focal.new_empty((b, e, k), dtype=torch.int32) if want_traces else _empty0(focal, torch.int32)
    with torch.cuda.device(focal.device):
        N.check(getattr(lib, f"dava_l1_camera_solve_{dt}")(
            b, e, m, n, N.ptr(focal), N.ptr(cx), N.ptr(cy), N.ptr(translation), N.ptr(lie), N.ptr(world),
            N.ptr(target), N.ptr(visibility), minimum_z_distance, maximum_pixel_ratio, max_gradient, error_scale,
            cfg, *[N.ptr(t) for t in outs], N.ptr(err), N.ptr(iters),
            *[N.ptr(t) if want_traces else None for t in (tr_err, tr_alpha, tr_exit)],
            N.ptr(ws) if need else None, ws.numel() if need else 0, N.stream_of(focal.device)),
            "dava_l1_camera_solve")
    return (*outs, err, iters, tr_err, tr_alpha, tr_exit)


@l1_camera_solve.register_fake
def _(focal, cx, cy, translation, lie, world, target, visibility, minimum_z_distance, maximum_pixel_ratio,
      max_gradient, error_scale, max_iterations, widen_iterations, zoom_iterations, constrain, epsilon,
      max_step_distance, min_step_distance, max_step_size, sufficient_decrease, curvature, slope_scale,
      derived_pixel_ratio, want_traces):
    b, e = focal.shape
    tr = (b, e, max_iterations) if want_traces else (0,)
    return (*[torch.empty_like(t) for t in (focal, cx, cy, translation, lie, world)], focal.new_empty((b, e)),
            focal.new_empty((b, e), dtype=torch.int32), focal.new_empty(tr), focal.new_empty(tr),
            focal.new_empty(tr, dtype=torch.int32))


OPS = ("bfgs_solve", "ba_solve", "ba_solve_record", "ba_solve_backward", "ba_evaluate", "ba_second_order",
       "ba_second_order_f64", "ba_solve_record_f64", "ba_solve_backward_f64", "ba_second_order_large_f64",
       "ba_solve_record_large_f64", "ba_solve_backward_large_f64", "bfgs_update_inverse_hessian",
       "bfgs_update_inverse_hessian_backward", "bfgs_initial_scale", "bfgs_initial_scale_backward",
       "bfgs_scale_matrix", "bfgs_scale_matrix_backward", "bfgs_search_direction", "bfgs_search_direction_backward",
       "wolfe_init", "wolfe_propose", "wolfe_update", "l1_camera_evaluate", "l1_camera_vjp",
       "ba_sgd_solve", "ba_sgd_solve_differentiable", "ba_sgd_backward", "ba_second_order_large",
       "ba_sgd_solve_differentiable_large", "ba_sgd_backward_large", "ba_sgd_solve_f64",
       "ba_sgd_solve_differentiable_f64", "ba_sgd_backward_f64", "l1_camera_solve")
