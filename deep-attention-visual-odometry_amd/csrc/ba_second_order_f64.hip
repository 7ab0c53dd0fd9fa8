// Second derivatives of the fused BA objectives in float64 (dava_ba_second_order_f64): the float64 counterpart
// of ba_second_order.hip.  The SAME objective code (ba_objective.hpp) instantiated with dual numbers over
// double (DualT<double>, dava_dual.hpp), x seeded with the tangent v and the observations with the tangent u:
// E, dE/dx, H v + (d2E/dx dobs) u, dE/dobs and (d2E/dobs dx) v + (d2E/dobs2) u, one launch, one 256-thread
// workgroup per problem with the dual image in LDS.  This is what the float64 objective's create_graph double
// backward and the generic loop's graph through a float64 solve need (bfgs_solver.py:133-135).
// Beyond the LDS image (dava_ba_second_order_large_f64) the same kernel body takes other pointers, FORM as in
// solve_f64.hpp:
//   form 0  the dual x and gradient, the dual dE/dobs, the observations and visibility in LDS
//   form 1  the dual x and gradient in LDS; the scene read in place; the dual dE/dobs (written per pair by its
//           owner thread) in a workspace of B x 4MN doubles, split into the two outputs after the evaluation's
//           final barrier -- not formed when neither output is asked for
//   form 2  as form 1, the dual x and gradient in a per-problem workspace slice of 4 Pv doubles
// Workspace: [dual dE/dobs B x 4MN, if an observation output is asked for | form 2: B x 4 Pv | 256-byte tail].
// The host side is one plan and one launcher for the two entry points (the conventions of dava_f64.hpp):
// dava_ba_second_order_f64 plans with any_form = false, dava_ba_second_order_large_f64 and the queries with true.
#include "ba_second_carve_f64.hpp"

#include <type_traits>

namespace dava {
namespace f64 {

struct SecondArgs {
  Layout L;
  int Pv;
  const double *obs, *x, *v, *obs_v;
  const uint8_t* vis;
  double *err, *grad, *hv, *obs_grad, *obs_hv;
};

// What the form 1 and 2 instantiations take (the form-0 one keeps its kernel argument as it was)
struct LargeSecondArgs : SecondArgs {
  double* obsd;  // B x 4MN (Dual64 dE/dobs), or null: not formed
  double* vecs;  // form 2: B x 4 Pv (Dual64 x, g), uninitialised
};

template <int FORM>
using second_args_t = std::conditional_t<FORM != 0, LargeSecondArgs, SecondArgs>;

template <int RES, int FORM = 0>
__global__ __launch_bounds__(kBlock, 1) void ba_second_order_f64_kernel(second_args_t<FORM> a) {
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, MN = M * N;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const SecondCarve cv = FORM == 0 ? carve_second(M, N, a.Pv) : carve_second_large(M, a.Pv, FORM);
  double* vec = lds64;  // the dual x and gradient: LDS, or (form 2) this problem's workspace slice
  if constexpr (FORM == 2) vec = a.vecs + b * 4 * a.Pv;
  Dual64* x = reinterpret_cast<Dual64*>(vec + cv.x);
  Dual64* g = reinterpret_cast<Dual64*>(vec + cv.g);
  Dual64* views = reinterpret_cast<Dual64*>(lds64 + cv.views);
  Dual64* vpart = reinterpret_cast<Dual64*>(lds64 + cv.vpart);
  Dual64* obsd = reinterpret_cast<Dual64*>(lds64 + cv.obsd);
  if constexpr (FORM != 0) obsd = a.obsd ? reinterpret_cast<Dual64*>(a.obsd + b * 4 * MN) : nullptr;
  double* scratch = lds64 + cv.scratch;
  double* obl = lds64 + cv.obs;  // form 0: the scene's LDS copy
  uint8_t* vil = reinterpret_cast<uint8_t*>(lds64) + cv.vis_bytes_off;
  const double* obs = obl;
  const uint8_t* vis = vil;
  for (int i = tid; i < a.Pv; i += kBlock) {
    x[i] = i < P ? Dual64(a.x[b * P + i], a.v ? a.v[b * P + i] : 0.0) : Dual64(0.0);
    g[i] = Dual64(0.0);
  }
  if constexpr (FORM == 0) {
    for (int i = tid; i < 2 * MN; i += kBlock) obl[i] = a.obs[b * 2 * MN + i];
    for (int i = tid; i < MN; i += kBlock) vil[i] = a.vis[b * MN + i] ? 1 : 0;
  } else {  // the scene where the caller put it
    obs = a.obs + b * 2 * MN;
    vis = a.vis + b * MN;
  }
  __syncthreads();
  int buf = 0;
  Dual64 E(0.0), unused(0.0);
  ba_eval<true, false, false, false, false, RES, Dual64>(L, x, nullptr, 0.0, obs, vis, g, views, vpart, scratch, buf, E,
                                                         unused, obsd, nullptr,
                                                         a.obs_v ? a.obs_v + b * 2 * MN : nullptr);
  if (tid == 0 && a.err) a.err[b] = E.v;
  for (int i = tid; i < P; i += kBlock) {
    if (a.grad) a.grad[b * P + i] = g[i].v;
    if (a.hv) a.hv[b * P + i] = g[i].t;
  }
  // dE/dobs was written per (view, point) pair by its owner thread; the eval's final barrier makes it visible
  if (FORM == 0 || obsd) {
    for (int i = tid; i < 2 * MN; i += kBlock) {
      if (a.obs_grad) a.obs_grad[b * 2 * MN + i] = obsd[i].v;
      if (a.obs_hv) a.obs_hv[b * 2 * MN + i] = obsd[i].t;
    }
  }
}

struct SecondPlan {
  int status;
  bool launch;  // false: return `status` (a refusal, or DAVA_OK for an empty batch)
  int form, lds, batch, residual;
  size_t obsd_bytes;    // forms 1 and 2 with an observation output: B x 4MN doubles, else 0
  size_t vector_bytes;  // form 2: B x 4 Pv doubles, else 0
  LargeSecondArgs args;  // the form-0 kernel takes its base
  size_t workspace_bytes() const { return obsd_bytes + vector_bytes + kTailBytes; }
};

// What a scene needs, from its shape alone (obs_out: an observation output is asked for): the queries and the
// launch's checks read the same numbers.
inline SecondPlan second_shape(const DavaScene& sc, bool obs_out, bool any_form) {
  SecondPlan p{};
  const int M = sc.num_views, N = sc.num_points, Pv = round_up(sc.num_parameters, 4);
  p.status = DAVA_ERR_UNSUPPORTED;
  p.form = any_form ? choose_second_form(M, N, Pv) : carve_second(M, N, Pv).total_bytes <= kMaxLdsBytes ? 0 : -1;
  if (p.form < 0) return p;
  p.status = DAVA_OK;
  p.lds = (int)(p.form == 0 ? carve_second(M, N, Pv) : carve_second_large(M, Pv, p.form)).total_bytes;
  p.batch = sc.batch;
  p.residual = sc.residual;
  p.obsd_bytes = p.form != 0 && obs_out ? (size_t)sc.batch * 4 * M * N * sizeof(double) : 0;
  p.vector_bytes = p.form == 2 ? (size_t)sc.batch * 4 * Pv * sizeof(double) : 0;
  return p;
}

// the shape behind a host-only query (which looks at no data pointer)
inline SecondPlan second_query(const DavaSceneF64* scene, bool obs_out) {
  DavaScene sc;
  SecondPlan p{};
  p.form = -1;
  p.status = check_scene_f64(scene, false, sc);
  return p.status == DAVA_OK ? second_shape(sc, obs_out, true) : p;
}

// the checks of both entry points, in their order
inline SecondPlan plan_second(const DavaSceneF64* scene, const double* x, const double* direction,
                              const double* obs_direction, double* error_out, double* grad_out, double* hv_out,
                              double* obs_grad_out, double* obs_hv_out, void* workspace, size_t workspace_bytes,
                              bool any_form) {
  SecondPlan p{};
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  DavaScene sc;
  const int st = check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return refuse(st);
  if (sc.batch == 0) return refuse(DAVA_OK);
  if (!x) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  p = second_shape(sc, obs_grad_out || obs_hv_out, any_form);
  if (p.status != DAVA_OK) return p;
  if (p.obsd_bytes + p.vector_bytes > 0 && (!workspace || workspace_bytes < p.workspace_bytes()))
    return refuse(DAVA_ERR_WORKSPACE);
  LargeSecondArgs& a = p.args;
  a.L = make_layout(&sc);
  a.Pv = round_up(sc.num_parameters, 4);
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.x = x;
  a.v = direction;
  a.obs_v = obs_direction;
  a.err = error_out;
  a.grad = grad_out;
  a.hv = hv_out;
  a.obs_grad = obs_grad_out;
  a.obs_hv = obs_hv_out;
  a.obsd = p.obsd_bytes ? static_cast<double*>(workspace) : nullptr;
  a.vecs = p.form == 2 ? reinterpret_cast<double*>(static_cast<char*>(workspace) + p.obsd_bytes) : nullptr;
  p.launch = true;
  return p;
}

template <int FORM>
int launch_second(const SecondPlan& p, void* stream) {
  const second_args_t<FORM>& a = p.args;
  with_flag(p.residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
    constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
    const auto kernel = ba_second_order_f64_kernel<kRes, FORM>;
    set_dynamic_lds(kernel, p.lds);
    hipLaunchKernelGGL(kernel, dim3(p.batch), dim3(kBlock), p.lds, static_cast<hipStream_t>(stream), a);
  });
  return launched();
}

inline int run_second(const SecondPlan& p, void* stream) {
  if (!p.launch) return p.status;
  if (p.form == 0) return launch_second<0>(p, stream);
  return p.form == 1 ? launch_second<1>(p, stream) : launch_second<2>(p, stream);
}

}  // namespace f64
}  // namespace dava

using namespace dava;

extern "C" int dava_ba_second_order_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                        const double* obs_direction, double* error_out, double* grad_out,
                                        double* hv_out, double* obs_grad_out, double* obs_hv_out, void* stream) {
  return f64::run_second(f64::plan_second(scene, x, direction, obs_direction, error_out, grad_out, hv_out,
                                          obs_grad_out, obs_hv_out, nullptr, 0, false), stream);
}

// host-only: 0, 1, 2, or minus the status
extern "C" int dava_ba_second_order_form_f64(const DavaSceneF64* scene) {
  const f64::SecondPlan p = f64::second_query(scene, false);
  return p.status == DAVA_OK ? p.form : -p.status;
}

// host-only; obs_outputs: an observation output (obs_grad_out or obs_hv_out) will be asked for.  0: unsupported.
extern "C" size_t dava_ba_second_order_large_workspace_bytes_f64(const DavaSceneF64* scene, int obs_outputs) {
  const f64::SecondPlan p = f64::second_query(scene, obs_outputs != 0);
  return p.status == DAVA_OK ? p.workspace_bytes() : 0;
}

extern "C" int dava_ba_second_order_large_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                              const double* obs_direction, double* error_out, double* grad_out,
                                              double* hv_out, double* obs_grad_out, double* obs_hv_out,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  return f64::run_second(f64::plan_second(scene, x, direction, obs_direction, error_out, grad_out, hv_out,
                                          obs_grad_out, obs_hv_out, workspace, workspace_bytes, true), stream);
}
