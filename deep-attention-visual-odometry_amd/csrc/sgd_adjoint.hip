// Adjoint of the float32 fused gradient descent (sgd_solve.hip): the entry points over sgd_adjoint.hpp.
// dava_ba_sgd_backward and dava_ba_sgd_backward_supported are the symbols of the LDS image (any_form = false),
// dava_ba_sgd_backward_large takes forms 0, 1 and 2.
#include "sgd_adjoint.hpp"

using namespace dava;

extern "C" int dava_ba_sgd_backward_supported(const DavaScene* scene, const DavaSgdConfig* config) {
  return sgd_adjoint_query<float>(scene, config, false, false).status == DAVA_OK ? 1 : 0;
}

extern "C" int dava_ba_sgd_backward(const DavaScene* scene, const DavaSgdConfig* config, const void* tape,
                                    size_t tape_bytes, const float* x_out_grad, float* x0_grad,
                                    float* observations_grad, void* stream) {
  return run_sgd_adjoint(plan_sgd_adjoint(scene, config, tape, tape_bytes, x_out_grad, x0_grad, observations_grad,
                                          nullptr, 0, false), stream);
}

// host-only: 0, 1, 2, or minus the status
extern "C" int dava_ba_sgd_backward_form(const DavaScene* scene, const DavaSgdConfig* config) {
  const SgdAdjointPlan<float> p = sgd_adjoint_query<float>(scene, config, false, true);
  return p.status == DAVA_OK ? p.form : -p.status;
}

// host-only; obs_grad: observations_grad will be asked for.  0: unsupported.
extern "C" size_t dava_ba_sgd_backward_large_workspace_bytes(const DavaScene* scene, const DavaSgdConfig* config,
                                                             int obs_grad) {
  const SgdAdjointPlan<float> p = sgd_adjoint_query<float>(scene, config, obs_grad != 0, true);
  return p.status == DAVA_OK ? sgd_adjoint_query_bytes(p) : 0;
}

extern "C" int dava_ba_sgd_backward_large(const DavaScene* scene, const DavaSgdConfig* config, const void* tape,
                                          size_t tape_bytes, const float* x_out_grad, float* x0_grad,
                                          float* observations_grad, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  return run_sgd_adjoint(plan_sgd_adjoint(scene, config, tape, tape_bytes, x_out_grad, x0_grad, observations_grad,
                                          workspace, workspace_bytes, true), stream);
}
