// Second derivatives of the fused BA objectives in float32: the entry points over ba_second_order.hpp.
// dava_ba_second_order and dava_ba_second_order_obs are the symbols of the LDS image (any_form = false),
// dava_ba_second_order_large takes forms 0, 1 and 2.
#include "ba_second_order.hpp"

using namespace dava;

extern "C" int dava_ba_second_order(const DavaScene* scene, const float* x, const float* direction,
                                    float* error_out, float* grad_out, float* hv_out, float* obs_grad_out,
                                    float* obs_hv_out, void* stream) {
  return dava_ba_second_order_obs(scene, x, direction, nullptr, error_out, grad_out, hv_out, obs_grad_out, obs_hv_out,
                                  stream);
}

extern "C" int dava_ba_second_order_obs(const DavaScene* scene, const float* x, const float* direction,
                                        const float* obs_direction, float* error_out, float* grad_out, float* hv_out,
                                        float* obs_grad_out, float* obs_hv_out, void* stream) {
  return run_second(plan_second(scene, x, direction, obs_direction, error_out, grad_out, hv_out, obs_grad_out,
                                obs_hv_out, nullptr, 0, false), stream);
}

// host-only: 0, 1, 2, or minus the status
extern "C" int dava_ba_second_order_form(const DavaScene* scene) {
  const SecondPlan<float> p = second_query<float>(scene, false);
  return p.status == DAVA_OK ? p.form : -p.status;
}

// host-only; obs_outputs: an observation output (obs_grad_out or obs_hv_out) will be asked for.  0: unsupported.
extern "C" size_t dava_ba_second_order_large_workspace_bytes(const DavaScene* scene, int obs_outputs) {
  const SecondPlan<float> p = second_query<float>(scene, obs_outputs != 0);
  return p.status == DAVA_OK ? p.workspace_bytes() : 0;
}

extern "C" int dava_ba_second_order_large(const DavaScene* scene, const float* x, const float* direction,
                                          const float* obs_direction, float* error_out, float* grad_out,
                                          float* hv_out, float* obs_grad_out, float* obs_hv_out, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  return run_second(plan_second(scene, x, direction, obs_direction, error_out, grad_out, hv_out, obs_grad_out,
                                obs_hv_out, workspace, workspace_bytes, true), stream);
}
