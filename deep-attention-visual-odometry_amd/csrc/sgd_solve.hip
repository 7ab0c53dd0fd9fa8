// Fused gradient descent on the BA objectives: the reference's SGDSolver (autograd_solvers/sgd_solver.py:29-44)
//   for k in 0 .. K-1:  g = d/dx sum_b E(x_k);  x_{k+1} = x_k - learning_rate * g
// as ONE launch, one workgroup per problem for the whole descent.  No stopping rule, no mask: every problem
// does the same work, so the grid is B workgroups and there is no work queue.
//
// Two forms, the ones dava_ba_evaluate takes (plan_eval, solve_plan.hpp; the layouts measured there):
//   LDS form (C1-C3)  observations, visibility, x and the gradient staged in LDS once; four waves; a point
//                     per thread in registers across the views when N <= 256 (PPT = 1);
//   large form (C5)   x and the gradient in LDS (2 Pv floats), the scene read in place with the packed pair
//                     sweep, eight waves -- the evaluate kernel's GV + XL form without the direction slot.
// A step is ba_eval<GRAD> (which ends on a barrier and overwrites every gradient entry: nothing to re-zero),
// the update, and one barrier.  The update rounds as torch does: the product first, then the difference.
// RECORD also writes x_k, k = 0 .. K-1, to the tape (B, K, Pv) the adjoint replays (sgd_adjoint.hpp); it
// changes no arithmetic, so a recording launch returns bitwise the plain launch's x_out and error trace.
#include <hip/hip_runtime.h>

#include "sgd_plan.hpp"

namespace dava {

struct SgdArgs {
  Layout L;
  int Pv, K;
  float lr;
  const float* obs;
  const uint8_t* vis;
  const float* x0;
  float* x_out;
  float* trace;  // (B, K) E(x_k), or nullptr
  float* tape;   // (B, K, Pv) x_k (RECORD)
};

template <bool GV, int RES, int PPT, int NW, bool RECORD>
__global__ __launch_bounds__(kWave * NW) void sgd_ba_solve_kernel(SgdArgs a) {
  constexpr int BLOCK = kWave * NW;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, Pv = a.Pv, K = a.K, MN = M * N;
  const int b = blockIdx.x, tid = threadIdx.x;
  const SgdCarve cv = carve_sgd(M, N, Pv, GV, NW);
  float* x = lds + cv.x;
  float* g = lds + cv.g;
  float* views = lds + cv.views;
  float* vpart = lds + cv.vpart;
  float* scratch = lds + cv.scratch;
  const float* obs;
  const uint8_t* vis;
  for (int i = tid; i < Pv; i += BLOCK) {
    x[i] = i < P ? a.x0[(size_t)b * P + i] : 0.f;
    g[i] = 0.f;
  }
  if constexpr (GV) {  // the scene stays in HBM, read in place
    obs = a.obs + (size_t)b * 2 * MN;
    vis = a.vis + (size_t)b * MN;
  } else {
    float* ol = lds + cv.obs;
    uint8_t* vl = reinterpret_cast<uint8_t*>(lds) + cv.vis_bytes_off;
    for (int i = tid; i < 2 * MN; i += BLOCK) ol[i] = a.obs[(size_t)b * 2 * MN + i];
    for (int i = tid; i < MN; i += BLOCK) vl[i] = a.vis[(size_t)b * MN + i] ? 1 : 0;
    obs = ol; vis = vl;
  }
  __syncthreads();
  const float lr = a.lr;
  int buf = 0;
  float unused = 0.f;
  for (int k = 0; k < K; ++k) {
    if constexpr (RECORD) {
      float* t = a.tape + ((size_t)b * K + k) * Pv;
      for (int i = tid; i < Pv; i += BLOCK) t[i] = x[i];
    }
    float E = 0.f;
    ba_eval<true, false, false, false, false, RES, float, NW, PPT, GV>(L, x, nullptr, 0.f, obs, vis, g, views, vpart,
                                                                       scratch, buf, E, unused);
    if (tid == 0 && a.trace) a.trace[(size_t)b * K + k] = E;
    for (int i = tid; i < P; i += BLOCK) x[i] = __fsub_rn(x[i], __fmul_rn(lr, g[i]));
    __syncthreads();
  }
  for (int i = tid; i < P; i += BLOCK) a.x_out[(size_t)b * P + i] = x[i];
}

template <int RES, bool RECORD>
static void launch_sgd(const SgdArgs& a, int B, const SgdPlan& p, hipStream_t s) {
  auto go = [&](auto kernel, int nw) { launch_lds(kernel, B, kWave * nw, p.lds_bytes, s, a); };
  if (p.gv) go(sgd_ba_solve_kernel<true, RES, 0, solve_waves(true), RECORD>, solve_waves(true));
  else if (p.ppt) go(sgd_ba_solve_kernel<false, RES, 1, kWaves, RECORD>, kWaves);
  else go(sgd_ba_solve_kernel<false, RES, 0, kWaves, RECORD>, kWaves);
}

static int sgd_solve_impl(const DavaScene* scene, const DavaSgdConfig* config, const float* x0, float* x_out,
                          float* error_trace_out, void* tape, size_t tape_bytes, bool record, void* stream) {
  const int st = check_scene(scene, true);
  if (st != DAVA_OK) return st;
  const SgdPlan p = plan_sgd(scene, config);
  if (p.status != DAVA_OK) return p.status;
  if (scene->batch == 0) return DAVA_OK;
  if (!x0 || !x_out) return DAVA_ERR_INVALID_ARGUMENT;
  const int K = config->iterations;
  if (record && K > 0 && (!tape || tape_bytes < sgd_tape_bytes(scene->batch, K, p.Pv))) return DAVA_ERR_WORKSPACE;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (K == 0) {  // no step: x_out = x0
    if (x_out != x0 && hipMemcpyAsync(x_out, x0, (size_t)scene->batch * scene->num_parameters * sizeof(float),
                                      hipMemcpyDeviceToDevice, s) != hipSuccess)
      return DAVA_ERR_LAUNCH;
    return DAVA_OK;
  }
  SgdArgs a;
  a.L = make_layout(scene);
  a.Pv = p.Pv;
  a.K = K;
  a.lr = config->learning_rate;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.x0 = x0;
  a.x_out = x_out;
  a.trace = error_trace_out;
  a.tape = record ? static_cast<float*>(tape) : nullptr;
  with_flag(record, [&](auto rec) {
    with_flag(scene->residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
      constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
      launch_sgd<kRes, decltype(rec)::value>(a, scene->batch, p, s);
    });
  });
  return launched();
}

}  // namespace dava

using namespace dava;

extern "C" int dava_ba_sgd_solve(const DavaScene* scene, const DavaSgdConfig* config, const float* x0, float* x_out,
                                 float* error_trace_out, void* stream) {
  return sgd_solve_impl(scene, config, x0, x_out, error_trace_out, nullptr, 0, false, stream);
}

extern "C" size_t dava_ba_sgd_tape_bytes(const DavaScene* scene, const DavaSgdConfig* config) {
  if (check_scene(scene, false) != DAVA_OK) return 0;
  const SgdPlan p = plan_sgd(scene, config);
  return p.status == DAVA_OK ? sgd_tape_bytes(scene->batch, config->iterations, p.Pv) : 0;
}

extern "C" int dava_ba_sgd_solve_record(const DavaScene* scene, const DavaSgdConfig* config, const float* x0,
                                        float* x_out, float* error_trace_out, void* tape, size_t tape_bytes,
                                        void* stream) {
  return sgd_solve_impl(scene, config, x0, x_out, error_trace_out, tape, tape_bytes, true, stream);
}
