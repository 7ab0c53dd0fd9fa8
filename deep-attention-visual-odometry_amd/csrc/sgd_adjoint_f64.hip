// Adjoint of the float64 fused gradient descent (sgd_solve_f64.hip): sgd_adjoint.hip's body on DualT<double>, one
// kBlock workgroup per problem.
//
// x_{k+1} = x_k - lr dE/dx(x_k, obs), so with lambda = dL/dx_{k+1}
//   dL/dx_k   = lambda - lr H(x_k) lambda                       (H symmetric)
//   dL/dobs  -= lr (d2E/dobs dx)(x_k) lambda
// Both products come out of ONE pass of the objective on dual numbers (forward-over-reverse, the body of
// ba_second_order_f64.hip): x carries x_k as its value -- read from the recording's tape -- and lambda as its
// tangent; the gradient's tangents are H lambda and dE/dobs's tangents the mixed term.  lambda stays in x's tangent
// slots from step to step.  Forms (ba_second_carve_f64.hpp), chosen by the adjoint's own fit whatever the forward took:
//   form 0  everything in LDS: carve_second's image and, after it, the accumulator of dL/dobs (2 M N doubles)
//   form 1  the dual x and gradient in LDS, the scene read in place, the step's dual dE/dobs in a workspace of
//           B x 4MN doubles, and the accumulator is the observations_grad output itself, zeroed and updated by the
//           thread that owns the element, in form 0's arithmetic and order
//   form 2  as form 1, the dual x and gradient in a per-problem workspace slice of 4 Pv doubles
// Workspace: [dual dE/dobs B x 4MN, forms 1 and 2 with an observation gradient | form 2: B x 4 Pv | 256-byte tail].
// With a NULL observations_grad the dual dE/dobs is not formed.  Deterministic: no atomics, every element has one
// owner thread.
#include "ba_second_carve_f64.hpp"
#include "sgd_f64.hpp"

namespace dava {
namespace f64 {

struct SgdAdjointArgs {
  Layout L;
  int Pv, K;
  double lr;
  const double* obs;
  const uint8_t* vis;
  const double* tape;  // (B, K, Pv) x_k
  const double* gout;  // (B, P) dL/dx_K
  double* gx0;         // (B, P) dL/dx_0
  double* gobs;        // (B, M, N, 2) dL/dobs, or nullptr (then not formed)
  double* obsd;        // forms 1, 2: B x 4MN (Dual64 dE/dobs of one step), or null: gobs is null
  double* vecs;        // form 2: B x 4 Pv (Dual64 x, g), uninitialised
};

inline long long sgd_adjoint_acc_bytes(int M, int N) { return 2LL * M * N * (long long)sizeof(double); }

template <int RES, int FORM>
__global__ __launch_bounds__(kBlock, 1) void sgd_ba_adjoint_f64_kernel(SgdAdjointArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, MN = M * N, Pv = a.Pv, K = a.K;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const SecondCarve cv = FORM == 0 ? carve_second(M, N, Pv) : carve_second_large(M, Pv, FORM);
  double* vec = lds64;  // the dual x and gradient: LDS, or (form 2) this problem's workspace slice
  if constexpr (FORM == 2) vec = a.vecs + b * 4 * Pv;
  Dual64* x = reinterpret_cast<Dual64*>(vec + cv.x);
  Dual64* g = reinterpret_cast<Dual64*>(vec + cv.g);
  Dual64* views = reinterpret_cast<Dual64*>(lds64 + cv.views);
  Dual64* vpart = reinterpret_cast<Dual64*>(lds64 + cv.vpart);
  Dual64* obsd = reinterpret_cast<Dual64*>(lds64 + cv.obsd);
  double* scratch = lds64 + cv.scratch;
  double* acc = lds64 + cv.total_bytes / 8;  // form 0: after the image (a multiple of 16 bytes)
  const double* obs;
  const uint8_t* vis;
  const bool want_obs = a.gobs != nullptr;  // uniform
  for (int i = tid; i < Pv; i += kBlock) {
    x[i] = Dual64(0.0, i < P ? a.gout[b * P + i] : 0.0);
    g[i] = Dual64(0.0);
  }
  if constexpr (FORM == 0) {
    double* obl = lds64 + cv.obs;
    uint8_t* vil = reinterpret_cast<uint8_t*>(lds64) + cv.vis_bytes_off;
    for (int i = tid; i < 2 * MN; i += kBlock) {
      obl[i] = a.obs[b * 2 * MN + i];
      acc[i] = 0.0;
    }
    for (int i = tid; i < MN; i += kBlock) vil[i] = a.vis[b * MN + i] ? 1 : 0;
    obs = obl;
    vis = vil;
  } else {  // the scene where the caller put it; the accumulator is the output
    obs = a.obs + b * 2 * MN;
    vis = a.vis + b * MN;
    obsd = want_obs ? reinterpret_cast<Dual64*>(a.obsd + b * 4 * MN) : nullptr;
    acc = want_obs ? a.gobs + b * 2 * MN : nullptr;
    if (want_obs)
      for (int i = tid; i < 2 * MN; i += kBlock) acc[i] = 0.0;
  }
  const double lr = a.lr;
  int buf = 0;
  for (int k = K - 1; k >= 0; --k) {
    const double* t = a.tape + (b * K + k) * Pv;
    for (int i = tid; i < Pv; i += kBlock) x[i].v = t[i];  // (element i is this thread's in every loop here)
    __syncthreads();
    Dual64 E(0.0), unused(0.0);
    ba_eval<true, false, false, false, false, RES, Dual64>(L, x, nullptr, 0.0, obs, vis, g, views, vpart, scratch, buf,
                                                           E, unused, want_obs ? obsd : nullptr, nullptr, nullptr);
    // (the evaluation ends on a barrier: g and obsd are complete)
    for (int i = tid; i < P; i += kBlock) x[i].t = descend(x[i].t, lr, g[i].t);
    if (want_obs)
      for (int i = tid; i < 2 * MN; i += kBlock) acc[i] = descend(acc[i], lr, obsd[i].t);
  }
  for (int i = tid; i < P; i += kBlock) a.gx0[b * P + i] = x[i].t;
  if constexpr (FORM == 0) {
    if (want_obs)
      for (int i = tid; i < 2 * MN; i += kBlock) a.gobs[b * 2 * MN + i] = acc[i];
  }
}

// ---- host side ----

// What a scene and a config need, from the shapes alone (obs_grad: observations_grad is asked for)
struct SgdAdjointShape {
  int status;  // DAVA_OK: `form` runs this scene / config
  int form, Pv, lds;
  size_t tape_bytes;
  size_t obsd_bytes;    // forms 1 and 2 with an observation gradient: B x 4MN doubles, else 0
  size_t vector_bytes;  // form 2: B x 4 Pv doubles, else 0
  size_t workspace_bytes() const { return obsd_bytes + vector_bytes ? obsd_bytes + vector_bytes + kTailBytes : 0; }
};

inline SgdAdjointShape sgd_adjoint_shape(const DavaScene& sc, const DavaSgdConfigF64* c, bool obs_grad) {
  SgdAdjointShape s{};
  s.form = -1;
  s.status = sgd_config_status(c);
  if (s.status != DAVA_OK) return s;
  s.status = DAVA_ERR_UNSUPPORTED;
  if (!sgd_sizes_sane(sc)) return s;
  const int M = sc.num_views, N = sc.num_points;
  s.Pv = round_up(sc.num_parameters, 4);
  s.form = choose_second_form(M, N, s.Pv, sgd_adjoint_acc_bytes(M, N));
  if (s.form < 0) return s;
  s.status = DAVA_OK;
  s.lds = (int)(s.form == 0 ? carve_second(M, N, s.Pv).total_bytes + sgd_adjoint_acc_bytes(M, N)
                            : carve_second_large(M, s.Pv, s.form).total_bytes);
  s.tape_bytes = sgd_tape_bytes(sc.batch, c->iterations, s.Pv);
  s.obsd_bytes = s.form != 0 && obs_grad ? (size_t)sc.batch * 4 * M * N * sizeof(double) : 0;
  s.vector_bytes = s.form == 2 ? (size_t)sc.batch * 4 * s.Pv * sizeof(double) : 0;
  return s;
}

// the shape behind a host-only query (which looks at no data pointer)
inline SgdAdjointShape sgd_adjoint_query(const DavaSceneF64* scene, const DavaSgdConfigF64* c, bool obs_grad) {
  DavaScene sc;
  SgdAdjointShape s{};
  s.form = -1;
  s.status = check_scene_f64(scene, false, sc);
  return s.status == DAVA_OK ? sgd_adjoint_shape(sc, c, obs_grad) : s;
}

struct SgdAdjointPlan {
  int status;
  bool launch;  // false: return `status` (a refusal, or DAVA_OK for an empty batch)
  bool ray;
  int batch;
  SgdAdjointShape shape;
  SgdAdjointArgs args;
};

// the checks of the entry point, in their order
inline SgdAdjointPlan plan_sgd_adjoint(const DavaSceneF64* scene, const DavaSgdConfigF64* config, const void* tape,
                                       size_t tape_bytes, const double* x_out_grad, double* x0_grad,
                                       double* observations_grad, void* workspace, size_t workspace_bytes) {
  SgdAdjointPlan p{};
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  DavaScene sc;
  const int st = check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return refuse(st);
  const SgdAdjointShape& s = p.shape = sgd_adjoint_shape(sc, config, observations_grad != nullptr);
  if (s.status == DAVA_ERR_INVALID_ARGUMENT) return refuse(s.status);
  if (sc.batch == 0) return refuse(DAVA_OK);
  const int K = config->iterations;
  if (!x_out_grad || !x0_grad) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  if (s.status != DAVA_OK) return refuse(s.status);
  if (K > 0 && (!tape || tape_bytes < s.tape_bytes)) return refuse(DAVA_ERR_WORKSPACE);
  if (s.workspace_bytes() > 0 && (!workspace || workspace_bytes < s.workspace_bytes()))
    return refuse(DAVA_ERR_WORKSPACE);
  p.ray = sc.residual == DAVA_RESIDUAL_RAY_ANGLE;
  p.batch = sc.batch;
  SgdAdjointArgs& a = p.args;
  a.L = make_layout(&sc);
  a.Pv = s.Pv;
  a.K = K;
  a.lr = config->learning_rate;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.tape = static_cast<const double*>(tape);
  a.gout = x_out_grad;
  a.gx0 = x0_grad;
  a.gobs = observations_grad;
  a.obsd = s.obsd_bytes ? static_cast<double*>(workspace) : nullptr;
  a.vecs = s.form == 2 ? reinterpret_cast<double*>(static_cast<char*>(workspace) + s.obsd_bytes) : nullptr;
  p.launch = true;
  return p;
}

template <int FORM>
int launch_sgd_adjoint(const SgdAdjointPlan& p, void* stream) {
  with_flag(p.ray, [&](auto ray) {
    constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
    launch_lds(sgd_ba_adjoint_f64_kernel<kRes, FORM>, p.batch, kBlock, p.shape.lds, static_cast<hipStream_t>(stream),
               p.args);
  });
  return launched();
}

inline int run_sgd_adjoint(const SgdAdjointPlan& p, void* stream) {
  if (!p.launch) return p.status;
  if (p.shape.form == 0) return launch_sgd_adjoint<0>(p, stream);
  return p.shape.form == 1 ? launch_sgd_adjoint<1>(p, stream) : launch_sgd_adjoint<2>(p, stream);
}

}  // namespace f64
}  // namespace dava

using namespace dava;

extern "C" int dava_ba_sgd_backward_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config, const void* tape,
                                        size_t tape_bytes, const double* x_out_grad, double* x0_grad,
                                        double* observations_grad, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  return f64::run_sgd_adjoint(f64::plan_sgd_adjoint(scene, config, tape, tape_bytes, x_out_grad, x0_grad,
                                                    observations_grad, workspace, workspace_bytes), stream);
}

// host-only: 0, 1, 2, or minus the status
extern "C" int dava_ba_sgd_backward_form_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config) {
  const f64::SgdAdjointShape s = f64::sgd_adjoint_query(scene, config, false);
  return s.status == DAVA_OK ? s.form : -s.status;
}

// host-only; observations_grad != 0: the observation gradient will be asked for.  0: form 0, or unsupported.
extern "C" size_t dava_ba_sgd_backward_workspace_bytes_f64(const DavaSceneF64* scene, const DavaSgdConfigF64* config,
                                                           int observations_grad) {
  const f64::SgdAdjointShape s = f64::sgd_adjoint_query(scene, config, observations_grad != 0);
  return s.status == DAVA_OK ? s.workspace_bytes() : 0;
}
