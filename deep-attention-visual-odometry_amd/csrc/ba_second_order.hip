// Second derivatives of the fused BA objectives (forward-over-reverse, dava_dual.hpp).
//
// For each problem: E, g = dE/dx, H v (v a direction per problem), dE/dobs and
// d(dE/dobs)/dx . v -- one launch, one workgroup per problem, the SAME objective
// code as the solver (ba_objective.hpp) instantiated with Dual scalars and x
// seeded with tangent v.  With an observation direction u as well (r06), the
// observations carry tangent u: the outputs become H v + (d2E/dx dobs) u and
// (d2E/dobs dx) v + (d2E/dobs2) u -- differentiating dE/dobs again.  This is the node that lets the caller differentiate
// THROUGH a solve whose error function is a fused objective: autograd's double
// backward of the reference's closure (bfgs_solver.py:133-135, create_graph)
// becomes g's VJP = H v (+ the mixed observation term).
//
// Beyond the LDS image (dava_ba_second_order_large) the same kernel body takes other pointers, FORM as in
// ba_second_order_f64.hip:
//   form 0  the dual x and gradient, the dual dE/dobs, the observations and visibility in LDS
//   form 1  the dual x and gradient in LDS; the scene read in place; the dual dE/dobs (written per pair by its
//           owner thread) in a workspace of B x 4MN floats, split into the two outputs after the evaluation's
//           final barrier -- not formed when neither output is asked for
//   form 2  as form 1, the dual x and gradient in a per-problem workspace slice of 4 Pv floats
// Workspace: [dual dE/dobs B x 4MN, if an observation output is asked for | form 2: B x 4 Pv | 256-byte tail].
// Outside ba_eval element i of every vector is touched only by the thread that owns it in the strided loops.
#include "ba_second_carve.hpp"

namespace dava {

struct SecondArgs {
  Layout L;
  int Pv;
  const float *obs, *x, *v, *obs_v;
  const uint8_t* vis;
  float *err, *grad, *hv, *obs_grad, *obs_hv;
};

// What the form 1 and 2 instantiations take (the form-0 one keeps its kernel argument as it was)
struct LargeSecondArgs : SecondArgs {
  float* obsd;  // B x 4MN (Dual dE/dobs), or null: not formed
  float* vecs;  // form 2: B x 4 Pv (Dual x, g), uninitialised
};

template <int FORM>
using second_args_t = std::conditional_t<FORM != 0, LargeSecondArgs, SecondArgs>;

template <int RES, int FORM = 0>
__global__ __launch_bounds__(kBlock) void ba_second_order_kernel(second_args_t<FORM> a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, MN = M * N;
  const int b = blockIdx.x, tid = threadIdx.x;
  const SecondCarve cv = FORM == 0 ? carve_second(M, N, a.Pv) : carve_second_large(M, a.Pv, FORM);
  float* vec = lds;  // the dual x and gradient: LDS, or (form 2) this problem's workspace slice
  if constexpr (FORM == 2) vec = a.vecs + (size_t)b * 4 * a.Pv;
  Dual* x = reinterpret_cast<Dual*>(vec + cv.x);
  Dual* g = reinterpret_cast<Dual*>(vec + cv.g);
  Dual* views = reinterpret_cast<Dual*>(lds + cv.views);
  Dual* vpart = reinterpret_cast<Dual*>(lds + cv.vpart);
  Dual* obsd = reinterpret_cast<Dual*>(lds + cv.obsd);
  if constexpr (FORM != 0) obsd = a.obsd ? reinterpret_cast<Dual*>(a.obsd + (size_t)b * 4 * MN) : nullptr;
  float* scratch = lds + cv.scratch;
  const float* obs;
  const uint8_t* vis;
  for (int i = tid; i < a.Pv; i += kBlock) {
    x[i] = i < P ? Dual(a.x[(size_t)b * P + i], a.v ? a.v[(size_t)b * P + i] : 0.0f) : Dual(0.0f);
    g[i] = Dual(0.0f);
  }
  if constexpr (FORM == 0) {
    float* obl = lds + cv.obs;
    uint8_t* vil = reinterpret_cast<uint8_t*>(lds) + cv.vis_bytes_off;
    for (int i = tid; i < 2 * MN; i += kBlock) obl[i] = a.obs[(size_t)b * 2 * MN + i];
    for (int i = tid; i < MN; i += kBlock) vil[i] = a.vis[(size_t)b * MN + i] ? 1 : 0;
    obs = obl;
    vis = vil;
  } else {  // the scene where the caller put it
    obs = a.obs + (size_t)b * 2 * MN;
    vis = a.vis + (size_t)b * MN;
  }
  __syncthreads();
  int buf = 0;
  Dual E(0.0f), unused(0.0f);
  ba_eval<true, false, false, false, false, RES, Dual>(L, x, nullptr, 0.0f, obs, vis, g, views, vpart, scratch, buf,
                                                       E, unused, obsd, nullptr,
                                                       a.obs_v ? a.obs_v + (size_t)b * 2 * MN : nullptr);
  if (tid == 0 && a.err) a.err[b] = E.v;
  for (int i = tid; i < P; i += kBlock) {
    if (a.grad) a.grad[(size_t)b * P + i] = g[i].v;
    if (a.hv) a.hv[(size_t)b * P + i] = g[i].t;
  }
  // dE/dobs was written per (view, point) pair by its owner thread; the eval's final
  // barrier makes it visible
  if (FORM == 0 || obsd) {
    for (int i = tid; i < 2 * MN; i += kBlock) {
      if (a.obs_grad) a.obs_grad[(size_t)b * 2 * MN + i] = obsd[i].v;
      if (a.obs_hv) a.obs_hv[(size_t)b * 2 * MN + i] = obsd[i].t;
    }
  }
}

// ---- host side: one plan and one launcher for the entry points ----
struct SecondLaunch {
  int status;
  bool launch;  // false: return `status` (a refusal, or DAVA_OK for an empty batch)
  int form, lds, batch, residual;
  size_t obsd_bytes;    // forms 1 and 2 with an observation output: B x 4MN floats, else 0
  size_t vector_bytes;  // form 2: B x 4 Pv floats, else 0
  LargeSecondArgs args;  // the form-0 kernel takes its base
  size_t workspace_bytes() const { return obsd_bytes + vector_bytes + kSecondTailBytes; }
};

// What a scene needs, from its shape alone (obs_out: an observation output is asked for): the queries and the
// launch's checks read the same numbers.  any_form false: the symbols of the LDS image, form 0 by fit alone.
static SecondLaunch second_shape(const DavaScene* sc, bool obs_out, bool any_form) {
  SecondLaunch p{};
  p.status = DAVA_ERR_UNSUPPORTED;
  const SecondPlan p0 = plan_second(sc);
  p.form = any_form ? choose_second_form(sc) : p0.status == DAVA_OK ? 0 : -1;
  if (p.form < 0) return p;
  p.status = DAVA_OK;
  p.lds = p.form == 0 ? p0.lds_bytes : carve_second_large(sc->num_views, p0.Pv, p.form).total_bytes;
  p.batch = sc->batch;
  p.residual = sc->residual;
  p.obsd_bytes = p.form != 0 && obs_out ? (size_t)sc->batch * 4 * sc->num_views * sc->num_points * sizeof(float) : 0;
  p.vector_bytes = p.form == 2 ? (size_t)sc->batch * 4 * p0.Pv * sizeof(float) : 0;
  return p;
}

// the checks of the entry points, in their order
static SecondLaunch plan_second_launch(const DavaScene* scene, const float* x, const float* direction,
                                       const float* obs_direction, float* error_out, float* grad_out, float* hv_out,
                                       float* obs_grad_out, float* obs_hv_out, void* workspace, size_t workspace_bytes,
                                       bool any_form) {
  SecondLaunch p{};
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  const int st = check_scene(scene, true);
  if (st != DAVA_OK) return refuse(st);
  if (scene->batch == 0) return refuse(DAVA_OK);
  if (!x) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  p = second_shape(scene, obs_grad_out || obs_hv_out, any_form);
  if (p.status != DAVA_OK) return p;
  if (p.obsd_bytes + p.vector_bytes > 0 && (!workspace || workspace_bytes < p.workspace_bytes()))
    return refuse(DAVA_ERR_WORKSPACE);
  LargeSecondArgs& a = p.args;
  a.L = make_layout(scene);
  a.Pv = round_up(scene->num_parameters, 4);
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
  a.obsd = p.obsd_bytes ? static_cast<float*>(workspace) : nullptr;
  a.vecs = p.form == 2 ? reinterpret_cast<float*>(static_cast<char*>(workspace) + p.obsd_bytes) : nullptr;
  p.launch = true;
  return p;
}

template <int FORM>
static int launch_second(const SecondLaunch& p, void* stream) {
  const second_args_t<FORM>& a = p.args;
  with_flag(p.residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
    constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
    launch_lds(ba_second_order_kernel<kRes, FORM>, p.batch, kBlock, p.lds, static_cast<hipStream_t>(stream), a);
  });
  return launched();
}

static int run_second(const SecondLaunch& p, void* stream) {
  if (!p.launch) return p.status;
  if (p.form == 0) return launch_second<0>(p, stream);
  return p.form == 1 ? launch_second<1>(p, stream) : launch_second<2>(p, stream);
}

// the shape behind a host-only query (which looks at no data pointer)
static SecondLaunch second_query(const DavaScene* scene, bool obs_out) {
  SecondLaunch p{};
  p.form = -1;
  p.status = check_scene(scene, false);
  return p.status == DAVA_OK ? second_shape(scene, obs_out, true) : p;
}

}  // namespace dava

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
  return run_second(plan_second_launch(scene, x, direction, obs_direction, error_out, grad_out, hv_out, obs_grad_out,
                                       obs_hv_out, nullptr, 0, false), stream);
}

// host-only: 0, 1, 2, or minus the status
extern "C" int dava_ba_second_order_form(const DavaScene* scene) {
  const SecondLaunch p = second_query(scene, false);
  return p.status == DAVA_OK ? p.form : -p.status;
}

// host-only; obs_outputs: an observation output (obs_grad_out or obs_hv_out) will be asked for.  0: unsupported.
extern "C" size_t dava_ba_second_order_large_workspace_bytes(const DavaScene* scene, int obs_outputs) {
  const SecondLaunch p = second_query(scene, obs_outputs != 0);
  return p.status == DAVA_OK ? p.workspace_bytes() : 0;
}

extern "C" int dava_ba_second_order_large(const DavaScene* scene, const float* x, const float* direction,
                                          const float* obs_direction, float* error_out, float* grad_out,
                                          float* hv_out, float* obs_grad_out, float* obs_hv_out, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  return run_second(plan_second_launch(scene, x, direction, obs_direction, error_out, grad_out, hv_out, obs_grad_out,
                                       obs_hv_out, workspace, workspace_bytes, true), stream);
}
