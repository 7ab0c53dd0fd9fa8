"""Drop-in ``SGDSolver`` (reference: ``autograd_solvers/sgd_solver.py:23-44``): plain gradient descent,

    for k in 0 .. iterations-1:  x <- x - learning_rate * d/dx sum_b error_function(x)

with the reference's two constructor keywords and its ``forward(parameters, error_function)`` contract:
``error_function`` takes ONE argument, there is no stopping rule, no mask and no training-mode behaviour, and the
output requires grad iff the input does.  Four execution paths:

1. **Fused** -- ``error_function`` is a :class:`ReprojectionError` or :class:`RayAngleError` and the parameters
   are float32 on the device: the whole descent is ONE launch of ``dava_ba_sgd_solve`` (include/dava_ba.h), one
   workgroup per problem.
2. **Fused, differentiable** -- the same with ``parameters.requires_grad``: the recording launch
   (``dava_ba_sgd_solve_record``) and, as its backward, the adjoint kernel (``dava_ba_sgd_backward``), which
   carries gradients to the parameters and to the objective's observations; taken where
   ``dava_ba_sgd_backward_supported``.  An objective built with ``large_derivatives=True`` takes it at every scene
   the recording descent and some form of the adjoint run (``dava_ba_sgd_backward_large``: forms 1 and 2 beyond the
   LDS image, C5 among them).
3. **Fused, float64** -- the objective was built with ``float64_descent=True`` (from float64 device observations)
   and the parameters are float64 on the device: ONE launch of ``dava_ba_sgd_solve_f64`` wherever
   ``dava_ba_sgd_solve_form_f64`` >= 0; with ``parameters.requires_grad`` the recording launch
   (``dava_ba_sgd_solve_record_f64``) and the adjoint kernel (``dava_ba_sgd_backward_f64``) wherever both form
   queries are >= 0.  Each operation takes form 0, 1 or 2 by its own fit, so C5 runs fused in both directions.
4. **The reference's loop** in torch, with ``error_function(parameters)`` and ``torch.autograd.grad(...,
   create_graph=...)`` -- any closure, CPU tensors, float64 without ``float64_descent``, and a fused objective
   whose image the fused kernels do not take (there the objective is an ordinary closure on its own kernels).

Nothing falls back from the GPU to the CPU.  ``last_errors`` holds E(x_k), k = 0 .. iterations-1, shaped
(B..., iterations), after a fused call (float64 after a float64 one) and ``None`` otherwise.
"""
from typing import Callable, Optional

import torch
from torch.nn import Module

from .. import native_ops
from ..camera_model import ReprojectionError


class SGDSolver(Module):
    def __init__(self, learning_rate: float, iterations: int):
        super().__init__()
        self.learning_rate = float(learning_rate)
        self.iterations = int(iterations)
        self.last_errors: Optional[torch.Tensor] = None

    def forward(self, parameters: torch.Tensor, error_function: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
        self.last_errors = None
        if (isinstance(error_function, ReprojectionError) and parameters.device.type == "cuda"
                and parameters.dtype == torch.float32 and self.iterations >= 0):
            batch = max(parameters.numel() // max(parameters.size(-1), 1), 1)
            shape = (batch, error_function.num_views, error_function.num_points, error_function.distortion)
            # (tracing under torch.compile asks the library nothing, on either route: there an unsupported scene is
            # the operator's ValueError when the compiled graph runs)
            if not parameters.requires_grad:
                if torch.compiler.is_compiling() or native_ops.sgd_solve_supported(*shape, error_function.residual):
                    return self._fused(parameters, error_function, native_ops.ba_sgd_solve)
            elif error_function.large_derivatives:
                if torch.compiler.is_compiling() or (
                        native_ops.sgd_backward_form(*shape, self.iterations, error_function.residual) >= 0
                        and native_ops.sgd_solve_supported(*shape, error_function.residual)):
                    return self._fused(parameters, error_function, native_ops.ba_sgd_solve_differentiable_large)
            elif torch.compiler.is_compiling() or native_ops.sgd_backward_supported(*shape, self.iterations,
                                                                                    error_function.residual):
                return self._fused(parameters, error_function, native_ops.ba_sgd_solve_differentiable)
        elif (isinstance(error_function, ReprojectionError) and error_function.float64_descent
                and parameters.device.type == "cuda" and parameters.dtype == torch.float64 and self.iterations >= 0):
            batch = max(parameters.numel() // max(parameters.size(-1), 1), 1)
            query = (batch, error_function.num_views, error_function.num_points, error_function.distortion,
                     self.iterations, error_function.residual)
            if not parameters.requires_grad:
                if torch.compiler.is_compiling() or native_ops.sgd_solve_form_f64(*query) >= 0:
                    return self._fused(parameters, error_function, native_ops.ba_sgd_solve_f64, float64=True)
            elif torch.compiler.is_compiling() or (native_ops.sgd_solve_form_f64(*query) >= 0
                                                   and native_ops.sgd_backward_form_f64(*query) >= 0):
                return self._fused(parameters, error_function, native_ops.ba_sgd_solve_differentiable_f64,
                                   float64=True)
        return self._loop(parameters, error_function)

    def _fused(self, parameters, fn: ReprojectionError, solve, float64: bool = False):
        lead = parameters.shape[:-1]
        if fn.batch_shape != lead:
            raise ValueError(f"ReprojectionError batch shape {tuple(fn.batch_shape)} != parameters {tuple(lead)}")
        observations = fn.observations64 if float64 else fn.observations
        x, errors = solve(parameters.reshape(-1, parameters.size(-1)),
                          observations.reshape(-1, fn.num_views, fn.num_points, 2),
                          fn.visibility.reshape(-1, fn.num_views, fn.num_points), fn.num_views, fn.num_points,
                          fn.distortion, learning_rate=self.learning_rate, iterations=self.iterations,
                          residual=fn.residual, want_errors=True)
        self.last_errors = errors.reshape(lead + (self.iterations,))
        return x.reshape(parameters.shape)

    def _loop(self, parameters, error_function):
        """The reference's loop (``sgd_solver.py:34-44``); the caller's tensor is left as it was."""
        create_graph = parameters.requires_grad
        for _ in range(self.iterations):
            if not parameters.requires_grad:
                parameters = parameters.detach().requires_grad_(True)
            with torch.enable_grad():
                error = error_function(parameters).sum()
            (gradient,) = torch.autograd.grad(error, parameters, create_graph=create_graph)
            parameters = parameters - self.learning_rate * gradient
        return parameters if create_graph else parameters.detach()
