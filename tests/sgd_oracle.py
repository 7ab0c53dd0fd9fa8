"""The oracle of the SGDSolver tests (test_sgd_abi.py, test_gpu_sgd.py): the reference's loop
(``autograd_solvers/sgd_solver.py:29-44``) in torch on the CPU around ``oracle.objective``.

    for k in 0 .. K-1:  g = d/dx sum_b E(x_k);  x_{k+1} = x_k - learning_rate * g

In float32 it is bitwise the reference's ``SGDSolver`` on the same closure (tests/golden/sgd.npz pins that);
in float64 it is the yardstick the float32 results' own rounding is measured against.
"""
import torch

from oracle import objective


def closure(obs, vis, m, n, distortion=False, ray=False):
    """The one-argument error function over ``oracle.objective`` (obs / vis are captured: gradients reach obs)."""
    if ray:
        return lambda x: objective.ray_angle_error(x, obs, vis, m, n)
    return lambda x: objective.reprojection_error(x, obs, vis, m, n, distortion)


def descend(x0, fn, learning_rate, iterations, create_graph=False, trace=False):
    """x_K (and, with ``trace``, E(x_k) for k = 0 .. K-1 as (B, K))."""
    x = x0
    errors = []
    for _ in range(iterations):
        if not x.requires_grad:
            x = x.detach().requires_grad_(True)
        with torch.enable_grad():
            e = fn(x)
        errors.append(e.detach())
        (g,) = torch.autograd.grad(e.sum(), x, create_graph=create_graph)
        x = x - learning_rate * g
    x = x if create_graph else x.detach()
    if trace:
        return x, (torch.stack(errors, dim=-1) if errors else x0.new_zeros(x0.shape[:-1] + (0,)))
    return x


def rows_rel(a, b):
    """Per-row relative error |a - b| / |b| over everything but the batch dimension."""
    a, b = a.reshape(a.shape[0], -1).double(), b.reshape(b.shape[0], -1).double()
    return (a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-300)


def gradients(x0, obs, vis, m, n, distortion, ray, w, learning_rate, iterations, dtype):
    """(x_K, dL/dx0, dL/dobs) for L = (w . x_K).sum(), by autograd through the loop in ``dtype``."""
    x = x0.to(dtype).clone().requires_grad_(True)
    o = obs.to(dtype).clone().requires_grad_(True)
    out = descend(x, closure(o, vis, m, n, distortion, ray), learning_rate, iterations, create_graph=True)
    gx, go = torch.autograd.grad((out * w.to(dtype)).sum(), [x, o])
    return out.detach(), gx, go
