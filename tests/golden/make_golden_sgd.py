"""Generate ``sgd.npz`` from the REAL reference's ``SGDSolver`` (build container only).

Run:   python tests/golden/make_golden_sgd.py          (needs the reference checkout make_golden.py reads)

``SGDSolver(learning_rate=1e-4, iterations=K)`` (``autograd_solvers/sgd_solver.py:23-44``), K in {1, 5, 20},
float32, on the reference-composed closures ``make_golden.py`` builds, with the one-argument contract of
``SGDSolver``'s error function:

* ``pinhole``  ``make_scenes(4, 2, 64)``: the squared reprojection objective (``ref_objective``);
* ``ray``      ``make_scenes(4, 2, 64, ray_angle=True)``: CalibrationNetwork's ray-angle error (``ref_ray_angle``);
* ``bc``       ``make_scenes(3, 3, 70, distortion=True)``: the objective with the reference's own distorted
               camera model in eager mode (``ref_objective_bc``).

10 % of the (view, point) pairs are masked.  Stored per case: x0, obs, vis and x_K as ``<case>_k<K>``.  Data
only; about 30 KB.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up the import paths and the reference's imports)

from deep_attention_visual_odometry.autograd_solvers import SGDSolver  # noqa: E402

LEARNING_RATE = 1e-4
ITERATIONS = (1, 5, 20)


def cases():
    eager = G.reference_distorted_model(False)
    yield "pinhole", G.make_scenes(4, 2, 64, seed=9601, drop=0.1), G.ref_objective
    yield "ray", G.make_scenes(4, 2, 64, seed=9602, drop=0.1, ray_angle=True), G.ref_ray_angle
    yield ("bc", G.make_scenes(3, 3, 70, distortion=True, seed=9603, drop=0.1),
           lambda x, obs, vis, m, n: G.ref_objective_bc(x, obs, vis, m, n, eager))


def main():
    torch.set_num_threads(8)
    out = {}
    for name, s, objective in cases():
        x0, obs, vis = torch.tensor(s.initial), torch.tensor(s.observations), torch.tensor(s.visibility)
        out[name + "_x0"], out[name + "_obs"], out[name + "_vis"] = x0.numpy(), obs.numpy(), vis.numpy()

        def fn(x, obs=obs, vis=vis, m=s.num_views, n=s.num_points, objective=objective):
            return objective(x, obs, vis, m, n)

        for k in ITERATIONS:
            out[f"{name}_k{k}"] = SGDSolver(learning_rate=LEARNING_RATE, iterations=k)(x0.clone(), fn).numpy()
    np.savez_compressed(os.path.join(HERE, "sgd.npz"), **out)
    print("sgd.npz written to", HERE)


if __name__ == "__main__":
    main()
