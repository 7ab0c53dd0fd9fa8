// Adjoint of the fused gradient descent (sgd_solve.hip, sgd_solve_f64.hip), for float and double: the reference's
// create_graph gradient through SGDSolver.forward (autograd_solvers/sgd_solver.py:29-44), one workgroup per
// problem.  sgd_adjoint.hip and sgd_adjoint_f64.hip hold the entry points.
//
// x_{k+1} = x_k - lr dE/dx(x_k, obs), so with lambda = dL/dx_{k+1}
//   dL/dx_k   = lambda - lr H(x_k) lambda                       (H symmetric)
//   dL/dobs  -= lr (d2E/dobs dx)(x_k) lambda
// Both products come out of ONE pass of the objective on dual numbers (forward-over-reverse, dava_dual.hpp, the
// body of ba_second_order.hpp): x carries x_k as its value -- read from the recording's tape -- and lambda as its
// tangent; the gradient's tangents are H lambda and dE/dobs's tangents the mixed term.  lambda stays in x's tangent
// slots from step to step.  Forms (dual_image.hpp), chosen by the adjoint's own fit whatever the forward took:
//   form 0  everything in LDS: carve_dual's image and, after it, the accumulator of dL/dobs (2 M N elements)
//   form 1  the dual x and gradient in LDS, the scene read in place, the step's dual dE/dobs in a workspace of
//           B x 4MN elements, and the accumulator is the observations_grad output itself, zeroed and updated by the
//           thread that owns the element, in form 0's arithmetic and order
//   form 2  as form 1, the dual x and gradient in a per-problem workspace slice of 4 Pv elements
// Workspace: [dual dE/dobs B x 4MN, forms 1 and 2 with an observation gradient | form 2: B x 4 Pv | 256-byte tail].
// With a NULL observations_grad the dual dE/dobs is not formed.  Deterministic: no atomics, every element has one
// owner thread.
#pragma once

#include "sgd_plan.hpp"

namespace dava {

template <class T>
struct SgdAdjointArgs {
  Layout L;
  int Pv, K;
  T lr;
  const T* obs;
  const uint8_t* vis;
  const T* tape;  // (B, K, Pv) x_k
  const T* gout;  // (B, P) dL/dx_K
  T* gx0;         // (B, P) dL/dx_0
  T* gobs;        // (B, M, N, 2) dL/dobs, or nullptr (then not formed)
  T* obsd;        // forms 1, 2: B x 4MN (dual dE/dobs of one step), or null: gobs is null
  T* vecs;        // form 2: B x 4 Pv (dual x, g), uninitialised
};

template <class T, int RES, int FORM>
__global__ __launch_bounds__(kBlock, DualTraits<T>::kMinBlocks) void sgd_ba_adjoint_kernel(SgdAdjointArgs<T> a) {
  using D = DualT<T>;
  T* lds = dual_lds<T>();
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, MN = M * N, Pv = a.Pv, K = a.K;
  const int tid = threadIdx.x;
  const typename DualTraits<T>::block_index b = blockIdx.x;
  const DualCarve cv = carve_dual<T, FORM>(M, N, Pv);
  T* vec = lds;  // the dual x and gradient: LDS, or (form 2) this problem's workspace slice
  if constexpr (FORM == 2) vec = a.vecs + (size_t)b * 4 * Pv;
  D* x = reinterpret_cast<D*>(vec + cv.x);
  D* g = reinterpret_cast<D*>(vec + cv.g);
  D* views = reinterpret_cast<D*>(lds + cv.views);
  D* vpart = reinterpret_cast<D*>(lds + cv.vpart);
  D* obsd = reinterpret_cast<D*>(lds + cv.obsd);
  T* scratch = lds + cv.scratch;
  T* acc = lds + cv.total_bytes / (long long)sizeof(T);  // form 0: after the image (a multiple of 16 bytes)
  const T* obs;
  const uint8_t* vis;
  const bool want_obs = a.gobs != nullptr;  // uniform
  for (int i = tid; i < Pv; i += kBlock) {
    x[i] = D(T(0), i < P ? a.gout[(size_t)b * P + i] : T(0));
    g[i] = D(T(0));
  }
  if constexpr (FORM == 0) {
    T* obl = lds + cv.obs;
    uint8_t* vil = reinterpret_cast<uint8_t*>(lds) + cv.vis_bytes_off;
    for (int i = tid; i < 2 * MN; i += kBlock) {
      obl[i] = a.obs[(size_t)b * 2 * MN + i];
      acc[i] = T(0);
    }
    for (int i = tid; i < MN; i += kBlock) vil[i] = a.vis[(size_t)b * MN + i] ? 1 : 0;
    obs = obl;
    vis = vil;
  } else {  // the scene where the caller put it; the accumulator is the output
    obs = a.obs + (size_t)b * 2 * MN;
    vis = a.vis + (size_t)b * MN;
    obsd = want_obs ? reinterpret_cast<D*>(a.obsd + (size_t)b * 4 * MN) : nullptr;
    acc = want_obs ? a.gobs + (size_t)b * 2 * MN : nullptr;
    if (want_obs)
      for (int i = tid; i < 2 * MN; i += kBlock) acc[i] = T(0);
  }
  const T lr = a.lr;
  int buf = 0;
  for (int k = K - 1; k >= 0; --k) {
    const T* t = a.tape + ((size_t)b * K + k) * Pv;
    for (int i = tid; i < Pv; i += kBlock) x[i].v = t[i];  // (element i is this thread's in every loop here)
    __syncthreads();
    D E(T(0)), unused(T(0));
    ba_eval<true, false, false, false, false, RES, D>(L, x, nullptr, T(0), obs, vis, g, views, vpart, scratch, buf, E,
                                                      unused, want_obs ? obsd : nullptr, nullptr, nullptr);
    // (the evaluation ends on a barrier: g and obsd are complete)
    for (int i = tid; i < P; i += kBlock) x[i].t = descend(x[i].t, lr, g[i].t);
    if (want_obs)
      for (int i = tid; i < 2 * MN; i += kBlock) acc[i] = descend(acc[i], lr, obsd[i].t);
  }
  for (int i = tid; i < P; i += kBlock) a.gx0[(size_t)b * P + i] = x[i].t;
  if constexpr (FORM == 0) {
    if (want_obs)
      for (int i = tid; i < 2 * MN; i += kBlock) a.gobs[(size_t)b * 2 * MN + i] = acc[i];
  }
}

// ---- host side: one plan and one launcher for the entry points (as ba_second_order.hpp) ----

template <class T>
size_t sgd_adjoint_tape_bytes(int B, int K, int Pv) {  // the forward's tape, in its type
  if constexpr (std::is_same_v<T, float>) return sgd_tape_bytes(B, K, Pv);
  else return f64::sgd_tape_bytes(B, K, Pv);
}

template <class T>
struct SgdAdjointPlan {
  int status;
  bool launch;  // false: return `status` (a refusal, or DAVA_OK for an empty batch)
  int form, lds, batch, residual;
  size_t tape_bytes;
  size_t obsd_bytes;    // workspace, forms 1 and 2 with an observation gradient: a step's dual dE/dobs, B x 4MN elements
  size_t vector_bytes;  // workspace after it, form 2: the dual x and g, B x 4 Pv elements
  SgdAdjointArgs<T> args;
  size_t block_bytes() const { return obsd_bytes + vector_bytes; }
};

// What a scene / config needs, from its shape alone, whatever form (or override) the forward takes: the queries and
// the launch's checks read the same numbers.  any_form false: the symbols of the LDS image, form 0 by fit alone.
// check_scene(sc, ...) must have passed.
template <class T, class Config>
SgdAdjointPlan<T> sgd_adjoint_shape(const DavaScene& sc, const Config* config, bool obs_grad, bool any_form) {
  SgdAdjointPlan<T> p{};
  p.form = -1;
  p.status = DAVA_ERR_INVALID_ARGUMENT;
  if (!config || config->iterations < 0) return p;
  p.status = DAVA_ERR_UNSUPPORTED;
  if (!sizes_sane(sc)) return p;
  const int M = sc.num_views, N = sc.num_points, Pv = round_up(sc.num_parameters, 4);
  const long long acc = dual_acc_bytes<T>(M, N);
  p.form = any_form ? choose_dual_form<T>(sc, acc) : dual_fits_form0<T>(sc, acc) ? 0 : -1;
  if (p.form < 0) return p;
  p.status = DAVA_OK;
  p.lds = (int)(carve_dual<T>(M, N, Pv, p.form).total_bytes + (p.form == 0 ? acc : 0));
  p.batch = sc.batch;
  p.residual = sc.residual;
  p.tape_bytes = sgd_adjoint_tape_bytes<T>(sc.batch, config->iterations, Pv);
  p.obsd_bytes = p.form != 0 && obs_grad ? (size_t)sc.batch * 4 * M * N * sizeof(T) : 0;
  p.vector_bytes = p.form == 2 ? (size_t)sc.batch * 4 * Pv * sizeof(T) : 0;
  return p;
}

// the shape behind a host-only query (which looks at no data pointer)
template <class T, class Scene, class Config>
SgdAdjointPlan<T> sgd_adjoint_query(const Scene* scene, const Config* config, bool obs_grad, bool any_form) {
  DavaScene sc;
  SgdAdjointPlan<T> p{};
  p.form = -1;
  p.status = check_dual_scene(scene, false, sc);
  return p.status == DAVA_OK ? sgd_adjoint_shape<T>(sc, config, obs_grad, any_form) : p;
}

// What the workspace query answers.  The two types differ, and their recorded answers hold them to it: the
// float32 query (dava_ba_sgd_backward_large_workspace_bytes) always counts the tail, the float64 one
// (dava_ba_sgd_backward_workspace_bytes_f64, which serves form 0 as well) says 0 where no block is needed.
inline size_t sgd_adjoint_query_bytes(const SgdAdjointPlan<float>& p) { return p.block_bytes() + kTailBytes; }
inline size_t sgd_adjoint_query_bytes(const SgdAdjointPlan<double>& p) {
  return p.block_bytes() ? p.block_bytes() + kTailBytes : 0;
}

// The checks of the entry points, in their order.  any_form is false only for float32's symbols of the LDS image
// (dava_ba_sgd_backward), which answer for their fit before the empty batch; every other symbol, float64's one
// among them, answers for the form after the pointers.
template <class T, class Scene, class Config>
SgdAdjointPlan<T> plan_sgd_adjoint(const Scene* scene, const Config* config, const void* tape, size_t tape_bytes,
                                   const T* x_out_grad, T* x0_grad, T* observations_grad, void* workspace,
                                   size_t workspace_bytes, bool any_form) {
  SgdAdjointPlan<T> p{};
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  DavaScene sc;
  const int st = check_dual_scene(scene, true, sc);
  if (st != DAVA_OK) return refuse(st);
  p = sgd_adjoint_shape<T>(sc, config, observations_grad != nullptr, any_form);
  if (p.status == DAVA_ERR_INVALID_ARGUMENT || (!any_form && p.status != DAVA_OK)) return p;
  if (sc.batch == 0) return refuse(DAVA_OK);
  if (!x_out_grad || !x0_grad) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  if (p.status != DAVA_OK) return p;
  if (config->iterations > 0 && (!tape || tape_bytes < p.tape_bytes)) return refuse(DAVA_ERR_WORKSPACE);
  if (p.block_bytes() > 0 && (!workspace || workspace_bytes < p.block_bytes() + kTailBytes))
    return refuse(DAVA_ERR_WORKSPACE);
  SgdAdjointArgs<T>& a = p.args;
  a.L = make_layout(&sc);
  a.Pv = round_up(sc.num_parameters, 4);
  a.K = config->iterations;
  a.lr = config->learning_rate;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.tape = static_cast<const T*>(tape);
  a.gout = x_out_grad;
  a.gx0 = x0_grad;
  a.gobs = observations_grad;
  a.obsd = p.obsd_bytes ? static_cast<T*>(workspace) : nullptr;
  a.vecs = p.form == 2 ? reinterpret_cast<T*>(static_cast<char*>(workspace) + p.obsd_bytes) : nullptr;
  p.launch = true;
  return p;
}

template <class T, int FORM>
int launch_sgd_adjoint(const SgdAdjointPlan<T>& p, void* stream) {
  with_flag(p.residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
    constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
    launch_lds(sgd_ba_adjoint_kernel<T, kRes, FORM>, p.batch, kBlock, p.lds, static_cast<hipStream_t>(stream),
               p.args);
  });
  return launched();
}

template <class T>
int run_sgd_adjoint(const SgdAdjointPlan<T>& p, void* stream) {
  if (!p.launch) return p.status;
  if (p.form == 0) return launch_sgd_adjoint<T, 0>(p, stream);
  return p.form == 1 ? launch_sgd_adjoint<T, 1>(p, stream) : launch_sgd_adjoint<T, 2>(p, stream);
}

}  // namespace dava
