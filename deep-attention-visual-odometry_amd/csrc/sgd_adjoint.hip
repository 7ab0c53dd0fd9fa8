// Adjoint of the fused gradient descent (sgd_solve.hip): the reference's create_graph gradient through
// SGDSolver.forward (autograd_solvers/sgd_solver.py:29-44), one workgroup per problem.
//
// x_{k+1} = x_k - lr dE/dx(x_k, obs), so with lambda = dL/dx_{k+1}
//   dL/dx_k   = lambda - lr H(x_k) lambda                       (H symmetric)
//   dL/dobs  -= lr (d2E/dobs dx)(x_k) lambda
// Both products come out of ONE pass of the objective on dual numbers (forward-over-reverse, dava_dual.hpp,
// the body of ba_second_order.hip): x carries x_k as its value -- read from the recording's tape -- and
// lambda as its tangent; the gradient's tangents are H lambda and dE/dobs's tangents the mixed term.
// lambda stays in x's tangent slots from step to step.  Deterministic: no atomics, every element has one
// owner thread.
#include <hip/hip_runtime.h>

#include "sgd_plan.hpp"

namespace dava {

struct SgdAdjointArgs {
  Layout L;
  int Pv, K;
  float lr;
  const float* obs;
  const uint8_t* vis;
  const float* tape;   // (B, K, Pv) x_k
  const float* gout;   // (B, P) dL/dx_K
  float* gx0;          // (B, P) dL/dx_0
  float* gobs;         // (B, M, N, 2) dL/dobs, or nullptr (then not formed)
};

template <int RES>
__global__ __launch_bounds__(kBlock) void sgd_ba_adjoint_kernel(SgdAdjointArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, MN = M * N, Pv = a.Pv, K = a.K;
  const int b = blockIdx.x, tid = threadIdx.x;
  const SecondCarve cv = carve_second(M, N, Pv);
  Dual* x = reinterpret_cast<Dual*>(lds + cv.x);
  Dual* g = reinterpret_cast<Dual*>(lds + cv.g);
  Dual* views = reinterpret_cast<Dual*>(lds + cv.views);
  Dual* vpart = reinterpret_cast<Dual*>(lds + cv.vpart);
  Dual* obsd = reinterpret_cast<Dual*>(lds + cv.obsd);
  float* scratch = lds + cv.scratch;
  float* obs = lds + cv.obs;
  uint8_t* vis = reinterpret_cast<uint8_t*>(lds) + cv.vis_bytes_off;
  float* acc = lds + sgd_adjoint_acc_bytes_off(cv) / 4;
  const bool want_obs = a.gobs != nullptr;  // uniform
  for (int i = tid; i < Pv; i += kBlock) {
    x[i] = Dual(0.0f, i < P ? a.gout[(size_t)b * P + i] : 0.0f);
    g[i] = Dual(0.0f);
  }
  for (int i = tid; i < 2 * MN; i += kBlock) {
    obs[i] = a.obs[(size_t)b * 2 * MN + i];
    acc[i] = 0.0f;
  }
  for (int i = tid; i < MN; i += kBlock) vis[i] = a.vis[(size_t)b * MN + i] ? 1 : 0;
  const float lr = a.lr;
  int buf = 0;
  for (int k = K - 1; k >= 0; --k) {
    const float* t = a.tape + ((size_t)b * K + k) * Pv;
    for (int i = tid; i < Pv; i += kBlock) x[i].v = t[i];  // (element i is this thread's in every loop here)
    __syncthreads();
    Dual E(0.0f), unused(0.0f);
    ba_eval<true, false, false, false, false, RES, Dual>(L, x, nullptr, 0.0f, obs, vis, g, views, vpart, scratch, buf,
                                                         E, unused, want_obs ? obsd : nullptr, nullptr, nullptr);
    // (the evaluation ends on a barrier: g and obsd are complete)
    for (int i = tid; i < P; i += kBlock) x[i].t = x[i].t - lr * g[i].t;
    if (want_obs)
      for (int i = tid; i < 2 * MN; i += kBlock) acc[i] = acc[i] - lr * obsd[i].t;
  }
  for (int i = tid; i < P; i += kBlock) a.gx0[(size_t)b * P + i] = x[i].t;
  if (want_obs)
    for (int i = tid; i < 2 * MN; i += kBlock) a.gobs[(size_t)b * 2 * MN + i] = acc[i];
}

// DAVA_OK where the adjoint runs this scene / config: the config's validity and the fit of the adjoint's own
// image, whatever form (or override) the forward takes.  check_scene(scene, ...) must have passed.
static int sgd_adjoint_status(const DavaScene* scene, const DavaSgdConfig* config, int* lds_out) {
  if (!config || config->iterations < 0) return DAVA_ERR_INVALID_ARGUMENT;
  if (!sgd_sizes_sane(scene)) return DAVA_ERR_UNSUPPORTED;
  const int lds = plan_second(scene).lds_bytes + sgd_adjoint_acc_bytes(scene->num_views, scene->num_points);
  if (lds > kMaxLds) return DAVA_ERR_UNSUPPORTED;
  if (lds_out) *lds_out = lds;
  return DAVA_OK;
}

}  // namespace dava

using namespace dava;

extern "C" int dava_ba_sgd_backward_supported(const DavaScene* scene, const DavaSgdConfig* config) {
  if (check_scene(scene, false) != DAVA_OK) return 0;
  return sgd_adjoint_status(scene, config, nullptr) == DAVA_OK ? 1 : 0;
}

extern "C" int dava_ba_sgd_backward(const DavaScene* scene, const DavaSgdConfig* config, const void* tape,
                                    size_t tape_bytes, const float* x_out_grad, float* x0_grad,
                                    float* observations_grad, void* stream) {
  const int st = check_scene(scene, true);
  if (st != DAVA_OK) return st;
  int lds = 0;
  const int as = sgd_adjoint_status(scene, config, &lds);
  if (as != DAVA_OK) return as;
  if (scene->batch == 0) return DAVA_OK;
  if (!x_out_grad || !x0_grad) return DAVA_ERR_INVALID_ARGUMENT;
  const int K = config->iterations, Pv = round_up(scene->num_parameters, 4);
  if (K > 0 && (!tape || tape_bytes < sgd_tape_bytes(scene->batch, K, Pv))) return DAVA_ERR_WORKSPACE;
  SgdAdjointArgs a;
  a.L = make_layout(scene);
  a.Pv = Pv;
  a.K = K;
  a.lr = config->learning_rate;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.tape = static_cast<const float*>(tape);
  a.gout = x_out_grad;
  a.gx0 = x0_grad;
  a.gobs = observations_grad;
  with_flag(scene->residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
    constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
    launch_lds(sgd_ba_adjoint_kernel<kRes>, scene->batch, kBlock, lds, static_cast<hipStream_t>(stream), a);
  });
  return launched();
}
