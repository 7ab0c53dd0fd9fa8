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
// owner thread.  Beyond the LDS image (dava_ba_sgd_backward_large) the kernel takes forms 1 and 2 below.
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

// What the form 1 and 2 instantiations take (the form-0 one keeps its kernel argument as it was)
struct LargeSgdAdjointArgs : SgdAdjointArgs {
  float* obsd;  // B x 4MN (Dual dE/dobs of one step), or null: gobs is null, not formed
  float* vecs;  // form 2: B x 4 Pv (Dual x, g), uninitialised
};

template <int FORM>
using sgd_adjoint_args_t = std::conditional_t<FORM != 0, LargeSgdAdjointArgs, SgdAdjointArgs>;

// FORM as in ba_second_order.hip: 0 everything in LDS; 1 the dual x and gradient in LDS, the scene read in place,
// the step's dual dE/dobs in the workspace and the accumulator of dL/dobs the output itself (zeroed and updated
// by the thread that owns the element, the arithmetic and order of form 0); 2 the dual x and gradient in the
// problem's workspace slice as well.
template <int RES, int FORM = 0>
__global__ __launch_bounds__(kBlock) void sgd_ba_adjoint_kernel(sgd_adjoint_args_t<FORM> a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, MN = M * N, Pv = a.Pv, K = a.K;
  const int b = blockIdx.x, tid = threadIdx.x;
  const SecondCarve cv = FORM == 0 ? carve_second(M, N, Pv) : carve_second_large(M, Pv, FORM);
  float* vec = lds;  // the dual x and gradient: LDS, or (form 2) this problem's workspace slice
  if constexpr (FORM == 2) vec = a.vecs + (size_t)b * 4 * Pv;
  Dual* x = reinterpret_cast<Dual*>(vec + cv.x);
  Dual* g = reinterpret_cast<Dual*>(vec + cv.g);
  Dual* views = reinterpret_cast<Dual*>(lds + cv.views);
  Dual* vpart = reinterpret_cast<Dual*>(lds + cv.vpart);
  Dual* obsd = reinterpret_cast<Dual*>(lds + cv.obsd);
  float* scratch = lds + cv.scratch;
  float* acc = lds + sgd_adjoint_acc_bytes_off(cv) / 4;
  const float* obs;
  const uint8_t* vis;
  const bool want_obs = a.gobs != nullptr;  // uniform
  for (int i = tid; i < Pv; i += kBlock) {
    x[i] = Dual(0.0f, i < P ? a.gout[(size_t)b * P + i] : 0.0f);
    g[i] = Dual(0.0f);
  }
  if constexpr (FORM == 0) {
    float* obl = lds + cv.obs;
    uint8_t* vil = reinterpret_cast<uint8_t*>(lds) + cv.vis_bytes_off;
    for (int i = tid; i < 2 * MN; i += kBlock) {
      obl[i] = a.obs[(size_t)b * 2 * MN + i];
      acc[i] = 0.0f;
    }
    for (int i = tid; i < MN; i += kBlock) vil[i] = a.vis[(size_t)b * MN + i] ? 1 : 0;
    obs = obl;
    vis = vil;
  } else {  // the scene where the caller put it; the accumulator is the output
    obs = a.obs + (size_t)b * 2 * MN;
    vis = a.vis + (size_t)b * MN;
    obsd = want_obs ? reinterpret_cast<Dual*>(a.obsd + (size_t)b * 4 * MN) : nullptr;
    acc = want_obs ? a.gobs + (size_t)b * 2 * MN : nullptr;
    if (want_obs)
      for (int i = tid; i < 2 * MN; i += kBlock) acc[i] = 0.0f;
  }
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
  if constexpr (FORM == 0) {
    if (want_obs)
      for (int i = tid; i < 2 * MN; i += kBlock) a.gobs[(size_t)b * 2 * MN + i] = acc[i];
  }
}

// ---- host side: one plan and one launcher for the entry points (as ba_second_order.hip) ----
struct SgdAdjointLaunch {
  int status;
  bool launch;  // false: return `status` (a refusal, or DAVA_OK for an empty batch)
  int form, lds;
  size_t tape_bytes;
  size_t obsd_bytes;    // workspace, forms 1 and 2 with an observation gradient: a step's dual dE/dobs, B x 4MN floats
  size_t vector_bytes;  // workspace after it, form 2: the dual x and g, B x 4 Pv floats
  LargeSgdAdjointArgs args;  // the form-0 kernel takes its base
  size_t workspace_bytes() const { return obsd_bytes + vector_bytes + kSecondTailBytes; }
};

// What a scene / config needs, from its shape alone, whatever form (or override) the forward takes: the queries and
// the launch's checks read the same numbers.  any_form false: the symbols of the LDS image, form 0 by fit alone.
// check_scene(sc, ...) must have passed.
static SgdAdjointLaunch sgd_adjoint_shape(const DavaScene* sc, const DavaSgdConfig* config, bool obs_grad,
                                          bool any_form) {
  SgdAdjointLaunch p{};
  p.form = -1;
  p.status = DAVA_ERR_INVALID_ARGUMENT;
  if (!config || config->iterations < 0) return p;
  p.status = DAVA_ERR_UNSUPPORTED;
  const int M = sc->num_views, N = sc->num_points, Pv = round_up(sc->num_parameters, 4);
  const int acc = sgd_adjoint_acc_bytes(M, N);
  if (any_form) p.form = choose_second_form(sc, acc);
  else if (sgd_sizes_sane(sc) && plan_second(sc).lds_bytes + acc <= kMaxLds) p.form = 0;
  if (p.form < 0) return p;
  p.status = DAVA_OK;
  p.lds = p.form == 0 ? plan_second(sc).lds_bytes + acc : carve_second_large(M, Pv, p.form).total_bytes;
  p.tape_bytes = sgd_tape_bytes(sc->batch, config->iterations, Pv);
  p.obsd_bytes = p.form != 0 && obs_grad ? (size_t)sc->batch * 4 * M * N * sizeof(float) : 0;
  p.vector_bytes = p.form == 2 ? (size_t)sc->batch * 4 * Pv * sizeof(float) : 0;
  return p;
}

// the checks of the entry points, in their order
static SgdAdjointLaunch plan_sgd_adjoint(const DavaScene* scene, const DavaSgdConfig* config, const void* tape,
                                         size_t tape_bytes, const float* x_out_grad, float* x0_grad,
                                         float* observations_grad, void* workspace, size_t workspace_bytes,
                                         bool any_form) {
  SgdAdjointLaunch p{};
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  const int st = check_scene(scene, true);
  if (st != DAVA_OK) return refuse(st);
  p = sgd_adjoint_shape(scene, config, observations_grad != nullptr, any_form);
  // (the symbol of the LDS image answers for its fit before the empty batch, the other one after the pointers)
  if (p.status == DAVA_ERR_INVALID_ARGUMENT || (!any_form && p.status != DAVA_OK)) return p;
  if (scene->batch == 0) return refuse(DAVA_OK);
  if (!x_out_grad || !x0_grad) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  if (p.status != DAVA_OK) return p;
  if (config->iterations > 0 && (!tape || tape_bytes < p.tape_bytes)) return refuse(DAVA_ERR_WORKSPACE);
  if (p.obsd_bytes + p.vector_bytes > 0 && (!workspace || workspace_bytes < p.workspace_bytes()))
    return refuse(DAVA_ERR_WORKSPACE);
  LargeSgdAdjointArgs& a = p.args;
  a.L = make_layout(scene);
  a.Pv = round_up(scene->num_parameters, 4);
  a.K = config->iterations;
  a.lr = config->learning_rate;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.tape = static_cast<const float*>(tape);
  a.gout = x_out_grad;
  a.gx0 = x0_grad;
  a.gobs = observations_grad;
  a.obsd = p.obsd_bytes ? static_cast<float*>(workspace) : nullptr;
  a.vecs = p.form == 2 ? reinterpret_cast<float*>(static_cast<char*>(workspace) + p.obsd_bytes) : nullptr;
  p.launch = true;
  return p;
}

template <int FORM>
static int launch_sgd_adjoint(const SgdAdjointLaunch& p, const DavaScene* scene, void* stream) {
  const sgd_adjoint_args_t<FORM>& a = p.args;
  with_flag(scene->residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
    constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
    launch_lds(sgd_ba_adjoint_kernel<kRes, FORM>, scene->batch, kBlock, p.lds, static_cast<hipStream_t>(stream), a);
  });
  return launched();
}

static int run_sgd_adjoint(const SgdAdjointLaunch& p, const DavaScene* scene, void* stream) {
  if (!p.launch) return p.status;
  if (p.form == 0) return launch_sgd_adjoint<0>(p, scene, stream);
  return p.form == 1 ? launch_sgd_adjoint<1>(p, scene, stream) : launch_sgd_adjoint<2>(p, scene, stream);
}

// the shape behind a host-only query (which looks at no data pointer)
static SgdAdjointLaunch sgd_adjoint_query(const DavaScene* scene, const DavaSgdConfig* config, bool obs_grad,
                                          bool any_form) {
  SgdAdjointLaunch p{};
  p.status = check_scene(scene, false);
  return p.status == DAVA_OK ? sgd_adjoint_shape(scene, config, obs_grad, any_form) : p;
}

}  // namespace dava

using namespace dava;

extern "C" int dava_ba_sgd_backward_supported(const DavaScene* scene, const DavaSgdConfig* config) {
  return sgd_adjoint_query(scene, config, false, false).status == DAVA_OK ? 1 : 0;
}

extern "C" int dava_ba_sgd_backward(const DavaScene* scene, const DavaSgdConfig* config, const void* tape,
                                    size_t tape_bytes, const float* x_out_grad, float* x0_grad,
                                    float* observations_grad, void* stream) {
  return run_sgd_adjoint(plan_sgd_adjoint(scene, config, tape, tape_bytes, x_out_grad, x0_grad, observations_grad,
                                          nullptr, 0, false), scene, stream);
}

// host-only: 0, 1, 2, or minus the status
extern "C" int dava_ba_sgd_backward_form(const DavaScene* scene, const DavaSgdConfig* config) {
  const SgdAdjointLaunch p = sgd_adjoint_query(scene, config, false, true);
  return p.status == DAVA_OK ? p.form : -p.status;
}

// host-only; obs_grad: observations_grad will be asked for.  0: unsupported.
extern "C" size_t dava_ba_sgd_backward_large_workspace_bytes(const DavaScene* scene, const DavaSgdConfig* config,
                                                             int obs_grad) {
  const SgdAdjointLaunch p = sgd_adjoint_query(scene, config, obs_grad != 0, true);
  return p.status == DAVA_OK ? p.workspace_bytes() : 0;
}

extern "C" int dava_ba_sgd_backward_large(const DavaScene* scene, const DavaSgdConfig* config, const void* tape,
                                          size_t tape_bytes, const float* x_out_grad, float* x0_grad,
                                          float* observations_grad, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  return run_sgd_adjoint(plan_sgd_adjoint(scene, config, tape, tape_bytes, x_out_grad, x0_grad, observations_grad,
                                          workspace, workspace_bytes, true), scene, stream);
}
