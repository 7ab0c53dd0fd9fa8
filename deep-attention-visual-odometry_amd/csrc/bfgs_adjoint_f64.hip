// Reverse mode of the float64 fused solve with the whole image in LDS (dava_ba_solve_backward_f64): the launch of
// bfgs_ba_adjoint_f64_kernel (adjoint_f64.hpp) in its form 0.  Scenes whose image does not fit take forms 1 and 2
// (bfgs_adjoint_large_f64.hip: dava_ba_solve_backward_large_f64).
#include "adjoint_f64.hpp"

using namespace dava;

extern "C" size_t dava_ba_solve_backward_workspace_bytes_f64(const DavaSceneF64* scene,
                                                             const DavaSolverConfigF64* config) {
  DavaScene sc;
  bool obs_lds;
  if (f64::adjoint_check(scene, config, sc, obs_lds) != DAVA_OK) return 0;
  const TapeLayout tl = tape_layout_f64(sc.batch, sc.num_parameters, config->iterations);
  return (size_t)sc.batch * tl.K * tl.Pv * sizeof(double) + f64::kTailBytes;
}

extern "C" int dava_ba_solve_backward_f64(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                                          const void* tape, size_t tape_bytes, const int32_t* status,
                                          const double* x_out_grad, double* x0_grad, double* observations_grad,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  DavaScene sc;
  bool obs_lds = false;
  const int st = f64::adjoint_check(scene, config, sc, obs_lds);
  if (st != DAVA_OK) return st;
  if (sc.batch == 0) return DAVA_OK;
  if (!scene->observations || !scene->visibility || !tape || !status || !x_out_grad || !x0_grad)
    return DAVA_ERR_INVALID_ARGUMENT;
  const TapeLayout tl = tape_layout_f64(sc.batch, sc.num_parameters, config->iterations);
  if (tape_bytes < tl.queue_byte) return DAVA_ERR_WORKSPACE;
  if (!workspace || workspace_bytes < (size_t)sc.batch * tl.K * tl.Pv * sizeof(double)) return DAVA_ERR_WORKSPACE;
  f64::AdjointArgs a;
  a.L = make_layout(&sc);
  a.Pv = tl.Pv;
  a.K = tl.K;
  a.tl = tl;
  a.tape = static_cast<const double*>(tape);
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.status = status;
  a.xbar = x_out_grad;
  a.x0_grad = x0_grad;
  a.obs_grad = observations_grad;
  a.arows = static_cast<double*>(workspace);
  a.obs_lds = obs_lds ? 1 : 0;
  const int lds = (int)f64::carve_adjoint(sc.num_views, sc.num_points, tl.Pv, obs_lds).total_bytes;
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto go = [&](auto kernel) {
    set_dynamic_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, dim3(sc.batch), dim3(kBlock), lds, s, a);
  };
  if (sc.residual == DAVA_RESIDUAL_RAY_ANGLE) go(f64::bfgs_ba_adjoint_f64_kernel<DAVA_RESIDUAL_RAY_ANGLE>);
  else go(f64::bfgs_ba_adjoint_f64_kernel<DAVA_RESIDUAL_SQUARED_REPROJECTION>);
  return hipGetLastError() == hipSuccess ? DAVA_OK : DAVA_ERR_LAUNCH;
}
