// Reverse mode of the float64 fused solve with the whole image in LDS (dava_ba_solve_backward_f64): the form-0
// instantiation of bfgs_ba_adjoint_f64_kernel.  The kernel, the plan and the launcher are in adjoint_f64.hpp; the
// entry points here plan with any_form = false, so a scene that needs forms 1 or 2
// (bfgs_adjoint_large_f64.hip: dava_ba_solve_backward_large_f64) is DAVA_ERR_UNSUPPORTED.
#include "adjoint_f64.hpp"

using namespace dava;

int dava::f64::adjoint_form0(const AdjointPlan& p, void* stream) {
  return p.launch ? launch_adjoint<0>(p, stream) : p.status;
}

extern "C" size_t dava_ba_solve_backward_workspace_bytes_f64(const DavaSceneF64* scene,
                                                             const DavaSolverConfigF64* config) {
  const f64::AdjointPlan p = f64::adjoint_shape(scene, config, false);
  return p.status == DAVA_OK ? p.workspace_bytes() : 0;
}

extern "C" int dava_ba_solve_backward_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                          const void* tape, size_t tape_bytes, const int32_t* status,
                                          const double* x_out_grad, double* x0_grad, double* observations_grad,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return f64::adjoint_form0(f64::plan_adjoint(scene, config, tape, tape_bytes, status, x_out_grad, x0_grad,
                                              observations_grad, workspace, workspace_bytes, false), stream);
}
