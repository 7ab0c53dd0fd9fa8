"""``BFGSCameraSolver`` (reference: ``solvers/bfgs_camera_solver.py:13-95``).

BFGS over an :class:`IOptimisableFunction` holding B x E estimates: per iteration the search
direction -H g (HIP ``search_direction``), the reference's max/min step clamp, the line search
(a module, normally :class:`LineSearchStrongWolfeConditions`), then H0 = (s.y / max(y.y, 1e-5)) I
on the first iteration (N&W 6.20, no lower clamp in this legacy variant) and the rank-2 update
(HIP ``update_inverse_hessian``, the same formula as ``BFGSSolver``).  Estimates keep updating
while their error exceeds ``epsilon`` (an fp32 constant, as in the reference).
"""
from typing import Optional

import torch
import torch.nn as nn

from .. import native_ops
from .i_optimisable_function import IOptimisableFunction


def clamp_search_direction(search_direction: torch.Tensor, max_step_length: float,
                           min_step_length: float) -> torch.Tensor:
    """Rescale each direction so its largest component lies in [min, max] (``:98-112``)."""
    largest = search_direction.abs().max(dim=-1).values.clamp(min=1e-8)
    scale = torch.ones_like(largest)
    too_large = largest > max_step_length
    too_small = largest < min_step_length
    scale[too_large] = max_step_length / largest[too_large]
    scale[too_small] = min_step_length / largest[too_small]
    return scale.clamp(min=1e-16)[:, :, None] * search_direction


def estimate_initial_inverse_hessian(ndim: int, step: torch.Tensor, delta_gradient: torch.Tensor) -> torch.Tensor:
    """H0 = (s.y / clamp(y.y, 1e-5)) I per estimate (``:115-131``)."""
    denominator = delta_gradient.square().sum(dim=-1).clamp(min=1e-5)
    gamma = (step * delta_gradient).sum(dim=-1) / denominator
    return gamma[:, :, None, None] * torch.eye(ndim, device=step.device, dtype=step.dtype).reshape(1, 1, ndim, ndim)


class BFGSCameraSolver(nn.Module):
    """``fused=True`` (opt-in; the default keeps the loop below) runs the whole forward -- this loop with
    ``LineSearchStrongWolfeConditions`` inside it -- in ONE HIP launch (``dava_l1_camera_solve``,
    csrc/camera_l1_solve.hip: one workgroup per (batch item, estimate), the loop restated statement for statement)
    when ``type(function) is PinholeCameraModelL1``, ``type(line_search) is LineSearchStrongWolfeConditions``,
    there is no ``search_direction_network``, no input tensor (the targets included) needs a graph under the
    current grad mode, the tensors are on the device in one of float32 / float64, and the library runs the shape
    (``native_ops.l1_solve_form`` >= 0).  Otherwise the forward runs the loop exactly as without the keyword;
    nothing falls back from GPU to CPU.  The fused call returns a new model at the solved parameters with its
    error cached, and sets ``last_iterations`` (B, E) and ``last_trace_error`` / ``last_trace_alpha`` /
    ``last_trace_exit`` (B, E, max_iterations; exit: 0 already frozen, 1 accepted while widening, 2 accepted in
    zoom, 3 unfinished from widening, 4 unfinished from zoom); they are ``None`` after a loop call.  The fused
    kernel has no adjoint: training through the legacy path (gradients through the solve) stays on the loop."""

    def __init__(self, max_iterations: int, epsilon: float, max_step_distance: float, min_step_distance: float,
                 line_search: nn.Module, search_direction_network: Optional[nn.Module] = None, fused: bool = False):
        super().__init__()
        self.line_search = line_search
        self.search_direction_network = search_direction_network
        self.max_iterations = int(max_iterations)
        self.epsilon = torch.tensor(float(epsilon))
        self.max_step_distance = float(max_step_distance)
        self.min_step_distance = float(min_step_distance)
        self.fused = bool(fused)
        self.last_iterations = self.last_trace_error = self.last_trace_alpha = self.last_trace_exit = None

    def _fused_inputs(self, function):
        """The fused kernel's tensors when this call may take it (see the class docstring), else None."""
        from ..camera_model.pinhole_camera_model_l1 import PinholeCameraModelL1
        from .line_search_strong_wolfe_conditions import LineSearchStrongWolfeConditions

        if not self.fused or self.max_iterations < 1 or self.search_direction_network is not None:
            return None
        if type(function) is not PinholeCameraModelL1 or type(self.line_search) is not LineSearchStrongWolfeConditions:
            return None
        tensors = (function._focal_length, function._cx, function._cy, function._translation,
                   function._orientation.lie_vector, function._world_points, function._true_projected_points)
        if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
            return None
        dt = tensors[0].dtype
        if dt not in (torch.float32, torch.float64) or any(t.dtype != dt or t.device.type != "cuda" for t in tensors):
            return None
        if function._visibility_mask.device.type != "cuda" or function._num_points < 4:
            return None
        if native_ops.l1_solve_form(function._num_views, function._num_points, dt) < 0:
            return None
        return tensors

    def _forward_fused(self, function, tensors):
        b, e, m, n = function.batch_size, function.num_estimates, function._num_views, function._num_points
        ls = self.line_search
        shapes = ((b, e), (b, e), (b, e), (b, e, m, 3), (b, e, m, 3), (b, e, n - 2, 3), (b, m, n, 2))
        flat = [t.detach().reshape(s) for t, s in zip(tensors, shapes)]
        # add() / masked_update() build their models without maximum_pixel_ratio: the constructor's default
        default_ratio = type(function).DEFAULT_MAXIMUM_PIXEL_RATIO
        slope_scale = torch.tensor(1.0 / function.num_parameters, dtype=torch.float).sqrt()
        res = native_ops.l1_camera_solve(
            *flat, function._visibility_mask.reshape(b, m, n),
            minimum_z_distance=function.minimum_z_distance, inverse_pixel_ratio=function.maximum_pixel_ratio,
            max_gradient=function._max_gradient, error_scale=float(function._error_scale.item()),
            max_iterations=self.max_iterations, widen_iterations=max(ls.widen_iterations, 0),
            zoom_iterations=max(ls.zoom_iterations, 0), constrain=function._constrain,
            epsilon=float(self.epsilon.item()), max_step_distance=self.max_step_distance,
            min_step_distance=self.min_step_distance, max_step_size=float(ls.max_step_size.item()),
            sufficient_decrease=float(ls.sufficient_decrease.item()), curvature=float(ls.curvature.item()),
            slope_scale=float(slope_scale.item()), derived_pixel_ratio=1.0 / abs(float(default_ratio)))
        self.last_iterations = res["iterations"]
        self.last_trace_error, self.last_trace_alpha = res["trace_error"], res["trace_alpha"]
        self.last_trace_exit = res["trace_exit"]
        like = lambda key, t: res[key].reshape(t.shape)  # noqa: E731
        return type(function)(
            focal_length=like("focal", tensors[0]), cx=like("cx", tensors[1]), cy=like("cy", tensors[2]),
            translation=like("translation", tensors[3]),
            orientation=type(function._orientation)(like("lie", tensors[4])),
            world_points=like("world", tensors[5]), true_projected_points=function._true_projected_points,
            visibility_mask=function._visibility_mask, minimum_z_distance=function.minimum_z_distance,
            constrain=function._constrain, max_gradient=function._max_gradient,
            enable_error_gradients=function._enable_error_gradients,
            enable_grad_gradients=function._enable_grad_gradients, _error=res["error"])

    def forward(self, function: IOptimisableFunction) -> IOptimisableFunction:
        self.last_iterations = self.last_trace_error = self.last_trace_alpha = self.last_trace_exit = None
        tensors = self._fused_inputs(function)
        if tensors is not None:
            return self._forward_fused(function, tensors)
        h = None
        updating = torch.ones(function.batch_size, function.num_estimates, device=function.device, dtype=torch.bool)
        for it in range(self.max_iterations):
            g = function.get_gradient()
            d = -1.0 * g if it == 0 else native_ops.search_direction(h, g)
            d = clamp_search_direction(d, self.max_step_distance, self.min_step_distance)
            if self.search_direction_network is not None:
                d = self.search_direction_network(d, function.as_parameters_vector(), function.get_error(), it)
            next_fn, step = self.line_search(function, d)
            dg = next_fn.get_gradient() - g
            if it == 0:
                h = estimate_initial_inverse_hessian(g.size(2), step, dg)
            h = native_ops.update_inverse_hessian(h, step, dg)
            function = function.masked_update(next_fn, updating)
            updating = updating & torch.greater(function.get_error(), self.epsilon)
        return function
