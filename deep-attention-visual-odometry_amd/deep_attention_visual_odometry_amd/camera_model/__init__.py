"""Calibration parameter layout and the native reprojection objective.

``unpack_calibration_parameters`` mirrors
``camera_model/calibration_pinhole_camera_model.py:33-75`` (same names,
same shapes, same ValueError on a wrong P).  ``ReprojectionError`` is the
error-function object the drop-in ``BFGSSolver`` recognises and runs fully
fused on the GPU; it is also an ordinary ``error_function(parameters,
batch_mask)`` closure (``networks/calibration_network.py:58-67`` contract)
whose value and derivatives (first order, and second order for
create_graph callers: H v and the observation cross term) come from HIP
kernels, differentiable w.r.t. the parameters and the observations.
"""
from typing import NamedTuple, Optional

import torch

from .. import native_ops
from ..geometry.closure_ops import get_camera_relative_points  # noqa: F401  (reference: camera_model/__init__.py)


def num_parameters(num_views: int, num_points: int, distortion: bool = False) -> int:
    return 3 + 3 * num_points + 6 * (num_views - 1) + (5 if distortion else 0)


class CalibrationParameters(NamedTuple):
    intrinsics: torch.Tensor
    world_points: torch.Tensor
    camera_translations: torch.Tensor
    camera_rotations: torch.Tensor


def unpack_calibration_parameters(parameters: torch.Tensor, num_views: int, num_points: int) -> CalibrationParameters:
    """Views of a (B..., 3 + 3N + 6(M-1)) parameter tensor (pinhole layout)."""
    expected = 3 + 3 * num_points + 6 * (num_views - 1)
    if parameters.size(-1) != expected:
        raise ValueError(
            f"The final dimension of the input tensor must be 3 + 3 * num_points + 6 * (num_views - 1) = "
            f"{expected}, got {parameters.size(-1)}")
    lead = parameters.shape[:-1]
    p_end = 3 + 3 * num_points
    t_end = p_end + 3 * (num_views - 1)
    return CalibrationParameters(
        intrinsics=parameters[..., 0:3].reshape(lead + (1, 1, 3)),
        world_points=parameters[..., 3:p_end].reshape(lead + (1, num_points, 3)),
        camera_translations=parameters[..., p_end:t_end].reshape(lead + (num_views - 1, 1, 3)),
        camera_rotations=parameters[..., t_end:].reshape(lead + (num_views - 1, 1, 3)),
    )


_F64_FIRST_ORDER_ONLY = ("the float64 fused objectives give E and dE/dx only: second derivatives and the "
                         "observation gradient are float32 only")


_F64_LARGE = 2  # f64_derivatives of an objective built with float64_large_gradients=True (True / 1: without)
_F32_LARGE = 3  # the same slot for float32 parameters of an objective built with large_derivatives=True


def _second_order(x, f64_derivatives=False):
    """The forward-over-reverse launch of x's dtype (float64 only on objectives built with float64_derivatives;
    with float64_large_gradients too: the launch that takes any scene size where the LDS image does not fit;
    float32 on an objective built with large_derivatives likewise)."""
    if x.dtype != torch.float64:
        return native_ops.ba_second_order_large if f64_derivatives == _F32_LARGE else native_ops.ba_second_order
    if f64_derivatives == _F64_LARGE:
        return native_ops.ba_second_order_large_f64
    return native_ops.ba_second_order_f64


class _NativeObjective(torch.autograd.Function):
    """E(x, obs) per row from the HIP objective kernel.  Its backward is itself
    differentiable (``_NativeGradient``), so ``torch.autograd.grad(..., create_graph=True)``
    -- the reference's differentiate-through-the-solve mode -- gets exact second
    derivatives from the forward-over-reverse kernel (``dava_ba_second_order``)."""

    @staticmethod
    def forward(ctx, x, observations, visibility, num_views, num_points, distortion, residual, f64_derivatives=False):
        need_x, need_obs = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if need_obs and x.dtype == torch.float64 and not f64_derivatives:
            raise TypeError(_F64_FIRST_ORDER_ONLY + " (the observations require grad)")
        if need_obs:  # dE/dobs comes from the second-order kernel (v = 0)
            err, grad, _, obs_grad, _ = _second_order(x, f64_derivatives)(
                x, observations, visibility, num_views, num_points, distortion, residual=residual, want_hv=False)
        else:
            err, grad, _ = native_ops.ba_evaluate(x, observations, visibility, num_views, num_points, distortion,
                                                  want_grad=need_x, residual=residual)
            obs_grad = None
        ctx.save_for_backward(x, observations, visibility)
        ctx.meta = (num_views, num_points, distortion, residual, f64_derivatives)
        ctx.first = (grad, obs_grad)
        return err

    @staticmethod
    def backward(ctx, grad_out):
        x, obs, vis = ctx.saved_tensors
        need_x, need_obs = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if torch.is_grad_enabled() and x.dtype == torch.float64 and not ctx.meta[4]:
            raise TypeError(_F64_FIRST_ORDER_ONLY + " (create_graph)")
        if torch.is_grad_enabled():  # create_graph: keep the gradient differentiable
            grad, obs_grad = _NativeGradient.apply(x, obs, vis, *ctx.meta)
        else:
            grad, obs_grad = ctx.first
        gx = grad_out.unsqueeze(-1) * grad if need_x else None
        gobs = grad_out[:, None, None, None] * obs_grad if (need_obs and obs_grad is not None) else None
        return gx, gobs, None, None, None, None, None, None


class _NativeGradient(torch.autograd.Function):
    """(dE/dx, dE/dobs) as a differentiable function of (x, obs): its VJP along the x-cotangent
    u is (H u, (d2E/dobs dx) u), from one forward-over-reverse launch."""

    @staticmethod
    def forward(ctx, x, observations, visibility, num_views, num_points, distortion, residual, f64_derivatives=False):
        if x.dtype == torch.float64 and not f64_derivatives:
            raise TypeError(_F64_FIRST_ORDER_ONLY)
        _, grad, _, obs_grad, _ = _second_order(x, f64_derivatives)(
            x, observations, visibility, num_views, num_points, distortion, residual=residual, want_hv=False)
        ctx.save_for_backward(x, observations, visibility)
        ctx.meta = (num_views, num_points, distortion, residual, f64_derivatives)
        ctx.set_materialize_grads(False)
        return grad, obs_grad

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, u, u_obs):
        # u_obs: a cotangent on dE/dobs (differentiating it again): the observations carry it as a tangent in
        # the same forward-over-reverse launch (dava_ba_second_order_obs)
        if u is None and u_obs is None:
            return None, None, None, None, None, None, None, None
        x, obs, vis = ctx.saved_tensors
        _, _, hv, _, obs_hv = _second_order(x, ctx.meta[4])(x, obs, vis, *ctx.meta[:3], direction=u,
                                                            residual=ctx.meta[3], want_obs=ctx.needs_input_grad[1],
                                                            obs_direction=u_obs)
        return (hv if ctx.needs_input_grad[0] else None, obs_hv if ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None)


class ReprojectionError:
    """Squared multi-view reprojection error of SURVEY.md 8(a).

    E(x) = sum_{m,n} vis[m,n] || pi_m(X_n) - obs[m,n] ||^2

    observations: (B..., M, N, 2) float32, visibility: (B..., M, N) bool/0-1,
    on the same ROCm device as the parameters.  float64 device observations also enable the float64
    kernels: float64 parameters then evaluate and solve in float64 (value and first derivative only;
    ``float64_derivatives=True`` -- float64 device observations required, else ``ValueError`` -- adds the float64
    second derivatives: create_graph, observations that require grad, double backward of dE/dobs, and the
    drop-in solver differentiates through a float64 solve; ``float64_large_gradients=True`` -- which requires
    ``float64_derivatives=True``, else ``ValueError`` -- extends both to scenes beyond the kernels' LDS image:
    the second derivatives, the recording solve and the adjoint in their forms 1 and 2).
    ``large_derivatives=True`` (independent of the float64 keywords) does the same for float32 parameters: the
    float32 second derivatives -- create_graph, observations that require grad, the double backward of dE/dobs --
    run at any admitted scene size (``dava_ba_second_order_large``), and ``SGDSolver`` differentiates through its
    fused descent there; without it such scenes keep raising ``RuntimeError``.
    ``float64_descent=True`` (independent of the other keywords; float64 device observations required, else
    ``ValueError``) makes ``SGDSolver`` run float64 parameters as the fused float64 descent
    (``dava_ba_sgd_solve_f64``) and, with ``requires_grad``, its recording launch and adjoint kernel, at every
    scene size their forms take; without it a float64 ``SGDSolver`` call keeps the torch loop.
    With ``distortion=True`` the five Brown-Conrady coefficients (k1 k2 k3 p1 p2) are appended to the
    parameter vector (``camera_model/distorted_camera_model.py:59-86``).
    """

    def __init__(self, observations: torch.Tensor, visibility: torch.Tensor, num_views: int, num_points: int,
                 distortion: bool = False, float64_derivatives: bool = False,
                 float64_large_gradients: bool = False, large_derivatives: bool = False,
                 float64_descent: bool = False):
        if observations.shape[-3:] != (num_views, num_points, 2):
            raise ValueError(f"observations must end in ({num_views}, {num_points}, 2), got {tuple(observations.shape)}")
        if visibility.shape != observations.shape[:-1]:
            raise ValueError("visibility must have shape observations.shape[:-1]")
        if num_views < 2:
            raise ValueError("num_views must be >= 2")
        # (device tensors: the kernels read float32; CPU tensors keep their dtype for the torch objective)
        self.observations = observations if observations.device.type == "cpu" else observations.to(torch.float32)
        # float64 device observations are the opt-in to the float64 kernels: kept beside the float32 copy, and
        # float64 parameters then evaluate (and solve) in float64.  Built from float32 observations the
        # objective stays float32 only, as before.
        self.observations64 = (observations if observations.device.type != "cpu"
                               and observations.dtype == torch.float64 else None)
        # opt-in: the float64 second derivatives (dava_ba_second_order_f64) and, through them, the float64 adjoint
        self.float64_derivatives = bool(float64_derivatives)
        if self.float64_derivatives and self.observations64 is None:
            raise ValueError("float64_derivatives=True needs float64 observations on a ROCm device "
                             f"(got {observations.dtype} on {observations.device})")
        # opt-in on top of it: second derivatives and gradients through the solve for scenes beyond the LDS image
        self.float64_large_gradients = bool(float64_large_gradients)
        if self.float64_large_gradients and not self.float64_derivatives:
            raise ValueError("float64_large_gradients=True needs float64_derivatives=True")
        # opt-in: float32 second derivatives (and SGDSolver's adjoint) for scenes beyond the LDS image
        self.large_derivatives = bool(large_derivatives)
        # opt-in: SGDSolver runs float64 parameters as the fused float64 descent (and its adjoint)
        self.float64_descent = bool(float64_descent)
        if self.float64_descent and self.observations64 is None:
            raise ValueError("float64_descent=True needs float64 observations on a ROCm device "
                             f"(got {observations.dtype} on {observations.device})")
        self.visibility = visibility.to(torch.uint8)
        self.num_views = int(num_views)
        self.num_points = int(num_points)
        self.distortion = bool(distortion)

    residual = native_ops.N.DAVA_RESIDUAL_SQUARED_REPROJECTION

    @property
    def num_parameters(self) -> int:
        return num_parameters(self.num_views, self.num_points, self.distortion)

    @property
    def batch_shape(self) -> torch.Size:
        return self.observations.shape[:-3]

    def __call__(self, parameters: torch.Tensor, batch_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``batch_mask`` None means every problem: the one-argument contract of ``SGDSolver``'s error function
        (``autograd_solvers/sgd_solver.py:29``)."""
        if parameters.size(-1) != self.num_parameters:
            raise ValueError(f"expected {self.num_parameters} parameters, got {parameters.size(-1)}")
        on_device = parameters.device.type != "cpu"
        if on_device and parameters.dtype == torch.float64 and self.observations64 is None:
            raise TypeError("ReprojectionError evaluates in float32 (construct it from float64 observations to "
                            "evaluate float64 parameters)")
        use64 = on_device and parameters.dtype == torch.float64
        obs = self.observations64 if use64 else self.observations
        vis = self.visibility
        if batch_mask is not None:
            obs, vis = obs[batch_mask], vis[batch_mask]
        lead = parameters.shape[:-1]
        x = parameters.reshape(-1, parameters.size(-1))
        obs = obs.reshape(-1, self.num_views, self.num_points, 2)
        vis = vis.reshape(-1, self.num_views, self.num_points)
        if x.device.type == "cpu":
            # CPU tensors: the same objective as torch ops (geometry.closure_ops), so the drop-in solves where
            # the parameters live, as the reference does (bfgs_solver.py:94-117); autograd gives its derivatives
            # to any order.  Device tensors take the HIP kernels below, never this.
            return self._torch_objective(x, obs.to(x.dtype), vis).reshape(lead)
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError("ReprojectionError evaluates in float32 (or float64, built from float64 observations)")
        if use64:
            flavour = (_F64_LARGE if self.float64_large_gradients else True) if self.float64_derivatives else False
        else:
            flavour = _F32_LARGE if self.large_derivatives else False
        err = _NativeObjective.apply(x, obs, vis, self.num_views, self.num_points, self.distortion, self.residual,
                                     flavour)
        return err.reshape(lead)


    def _torch_objective(self, x, obs, vis):
        from ..geometry.closure_ops import reprojection_objective

        return reprojection_objective(x, obs, vis, self.num_views, self.num_points, self.distortion)


class RayAngleError(ReprojectionError):
    """The error ``CalibrationNetwork`` minimises (``networks/calibration_network.py:58-67``):

    E(x) = sum_{m,n} vis[m,n] * angle(ray(obs[m,n]), p_m(X_n))

    with ray(u, v) = (u - cx, v - cy, elu(f) + 1)
    (``geometry/homogeneous_projection.py:21-44``), p_m(X_n) the scale-normalised
    camera-relative point (``camera_model/calibration_pinhole_camera_model.py:78-117``)
    and the angle in Kahan's form 2 atan2(|a^ - b^|, |a^ + b^|)
    (``geometry/projective_plane_angle_distance.py:20-64``).  Pinhole parameter
    layout only; the fused solver and the evaluation kernel both run it on the GPU (on CPU tensors, torch ops).
    """

    residual = native_ops.N.DAVA_RESIDUAL_RAY_ANGLE

    def __init__(self, observations: torch.Tensor, visibility: torch.Tensor, num_views: int, num_points: int,
                 float64_derivatives: bool = False, float64_large_gradients: bool = False,
                 large_derivatives: bool = False, float64_descent: bool = False):
        super().__init__(observations, visibility, num_views, num_points, distortion=False,
                         float64_derivatives=float64_derivatives, float64_large_gradients=float64_large_gradients,
                         large_derivatives=large_derivatives, float64_descent=float64_descent)

    def _torch_objective(self, x, obs, vis):
        from ..geometry.closure_ops import ray_angle_objective

        return ray_angle_objective(x, obs, vis, self.num_views, self.num_points)


from .pinhole_camera_model_l1 import PinholeCameraModelL1  # noqa: E402  (legacy IOptimisableFunction model)
