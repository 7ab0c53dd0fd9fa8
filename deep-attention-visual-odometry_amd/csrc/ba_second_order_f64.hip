// Second derivatives of the fused BA objectives in float64: the entry points over ba_second_order.hpp, on dual
// numbers over double.  This is what the float64 objective's create_graph double backward and the generic loop's
// graph through a float64 solve need (bfgs_solver.py:133-135).  dava_ba_second_order_f64 is the symbol of the LDS
// image (any_form = false), dava_ba_second_order_large_f64 takes forms 0, 1 and 2.
#include "ba_second_order.hpp"

using namespace dava;

extern "C" int dava_ba_second_order_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                        const double* obs_direction, double* error_out, double* grad_out,
                                        double* hv_out, double* obs_grad_out, double* obs_hv_out, void* stream) {
  return run_second(plan_second(scene, x, direction, obs_direction, error_out, grad_out, hv_out, obs_grad_out,
                                obs_hv_out, nullptr, 0, false), stream);
}

// host-only: 0, 1, 2, or minus the status
extern "C" int dava_ba_second_order_form_f64(const DavaSceneF64* scene) {
  const SecondPlan<double> p = second_query<double>(scene, false);
  return p.status == DAVA_OK ? p.form : -p.status;
}

// host-only; obs_outputs: an observation output (obs_grad_out or obs_hv_out) will be asked for.  0: unsupported.
extern "C" size_t dava_ba_second_order_large_workspace_bytes_f64(const DavaSceneF64* scene, int obs_outputs) {
  const SecondPlan<double> p = second_query<double>(scene, obs_outputs != 0);
  return p.status == DAVA_OK ? p.workspace_bytes() : 0;
}

extern "C" int dava_ba_second_order_large_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                              const double* obs_direction, double* error_out, double* grad_out,
                                              double* hv_out, double* obs_grad_out, double* obs_hv_out,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  return run_second(plan_second(scene, x, direction, obs_direction, error_out, grad_out, hv_out, obs_grad_out,
                                obs_hv_out, workspace, workspace_bytes, true), stream);
}
