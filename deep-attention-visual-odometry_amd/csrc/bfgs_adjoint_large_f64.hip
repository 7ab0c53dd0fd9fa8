// The float64 adjoint for scenes whose adjoint image does not fit 160 KiB: dava_ba_solve_backward_large_f64, with
// the host-only queries dava_ba_solve_backward_form_f64 and dava_ba_solve_backward_large_workspace_bytes_f64.
//
// The kernel is bfgs_ba_adjoint_f64_kernel (adjoint_f64.hpp) in its forms 1 and 2: the body of the form-0 adjoint
// with the scene read in place and the observation cotangent accumulated in the output (form 1) and, beyond that,
// the 14 Pv vectors in a per-problem slice of the workspace (form 2).  The entry points here plan with
// any_form = true (adjoint_f64.hpp: the checks of dava_ba_solve_backward_f64, the form chosen by fit,
// f64::choose_adjoint_form, independently of the form the recording took); a scene whose whole image fits takes
// form 0, i.e. the launch bfgs_adjoint_f64.hip instantiates (f64::adjoint_form0).
// Workspace: [rows a_j B x K x Pv | form 2: vectors B x 14 x Pv | 256-byte tail], doubles.  The vector slices
// arrive uninitialised: the kernel writes all 14 x Pv doubles of its slice, pads included, before it reads any
// (the staging loop covers the ten plain vectors; every step writes the four dual slots -- as s, w, y, g_k for
// k > 0, as the dual x and gradient for every k -- over all Pv elements before reading them).
// Not here: LDS copies of x for a form-2 problem, single-pass row products, on-chip tape rows.
#include "adjoint_f64.hpp"

using namespace dava;

extern "C" int dava_ba_solve_backward_form_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config) {
  const f64::AdjointPlan p = f64::adjoint_shape(scene, config, true);
  return p.status == DAVA_OK ? p.form : -p.status;
}

extern "C" size_t dava_ba_solve_backward_large_workspace_bytes_f64(const DavaSceneF64* scene,
                                                                   const DavaSolverConfigF64* config) {
  const f64::AdjointPlan p = f64::adjoint_shape(scene, config, true);
  return p.status == DAVA_OK ? p.workspace_bytes() : 0;
}

extern "C" int dava_ba_solve_backward_large_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                                const void* tape, size_t tape_bytes, const int32_t* status,
                                                const double* x_out_grad, double* x0_grad,
                                                double* observations_grad, void* workspace, size_t workspace_bytes,
                                                void* stream) {
  const f64::AdjointPlan p = f64::plan_adjoint(scene, config, tape, tape_bytes, status, x_out_grad, x0_grad,
                                               observations_grad, workspace, workspace_bytes, true);
  if (!p.launch || p.form == 0) return f64::adjoint_form0(p, stream);
  return p.form == 1 ? f64::launch_adjoint<1>(p, stream) : f64::launch_adjoint<2>(p, stream);
}
