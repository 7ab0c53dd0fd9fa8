// Adjoint of the float64 fused gradient descent (sgd_solve_f64.hip): the entry points over sgd_adjoint.hpp, on
// dual numbers over double.  One symbol takes forms 0, 1 and 2.
#include "sgd_adjoint.hpp"

using namespace dava;

extern "C" int dava_ba_sgd_backward_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config, const void* tape,
                                        size_t tape_bytes, const double* x_out_grad, double* x0_grad,
                                        double* observations_grad, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  return run_sgd_adjoint(plan_sgd_adjoint(scene, config, tape, tape_bytes, x_out_grad, x0_grad, observations_grad,
                                          workspace, workspace_bytes, true), stream);
}

// host-only: 0, 1, 2, or minus the status
extern "C" int dava_ba_sgd_backward_form_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config) {
  const SgdAdjointPlan<double> p = sgd_adjoint_query<double>(scene, config, false, true);
  return p.status == DAVA_OK ? p.form : -p.status;
}

// host-only; observations_grad != 0: the observation gradient will be asked for.  0: form 0, or unsupported.
extern "C" size_t dava_ba_sgd_backward_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config,
                                                           int observations_grad) {
  const SgdAdjointPlan<double> p = sgd_adjoint_query<double>(scene, config, observations_grad != 0, true);
  return p.status == DAVA_OK ? sgd_adjoint_query_bytes(p) : 0;
}
