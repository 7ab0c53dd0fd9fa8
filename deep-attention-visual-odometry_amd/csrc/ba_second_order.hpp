// Second derivatives of the fused BA objectives (forward-over-reverse, dava_dual.hpp), for float and double: the
// kernel, its plan and its launcher.  ba_second_order.hip and ba_second_order_f64.hip hold the entry points.
//
// For each problem: E, g = dE/dx, H v (v a direction per problem), dE/dobs and d(dE/dobs)/dx . v -- one launch,
// one workgroup per problem, the SAME objective code as the solver (ba_objective.hpp) instantiated with dual
// scalars and x seeded with tangent v.  With an observation direction u as well, the observations carry tangent
// u: the outputs become H v + (d2E/dx dobs) u and (d2E/dobs dx) v + (d2E/dobs2) u -- differentiating dE/dobs
// again.  This is the node that lets the caller differentiate THROUGH a solve whose error function is a fused
// objective: autograd's double backward of the reference's closure (bfgs_solver.py:133-135, create_graph) becomes
// g's VJP = H v (+ the mixed observation term).
//
// Beyond the LDS image (the *_large symbols) the same kernel body takes other pointers, FORM as in dual_image.hpp:
//   form 0  the dual x and gradient, the dual dE/dobs, the observations and visibility in LDS
//   form 1  the dual x and gradient in LDS; the scene read in place; the dual dE/dobs (written per pair by its
//           owner thread) in a workspace of B x 4MN elements, split into the two outputs after the evaluation's
//           final barrier -- not formed when neither output is asked for
//   form 2  as form 1, the dual x and gradient in a per-problem workspace slice of 4 Pv elements
// Workspace: [dual dE/dobs B x 4MN, if an observation output is asked for | form 2: B x 4 Pv | 256-byte tail].
// Outside ba_eval element i of every vector is touched only by the thread that owns it in the strided loops.
// The host side is one plan and one launcher (the conventions of dava_f64.hpp): the symbols of the LDS image plan
// with any_form = false, the *_large symbols and the queries with true.
#pragma once

#include "dual_image.hpp"

namespace dava {

template <class T>
struct SecondArgs {
  Layout L;
  int Pv;
  const T *obs, *x, *v, *obs_v;
  const uint8_t* vis;
  T *err, *grad, *hv, *obs_grad, *obs_hv;
};

// What the form 1 and 2 instantiations take (the form-0 one takes the shorter argument)
template <class T>
struct LargeSecondArgs : SecondArgs<T> {
  T* obsd;  // B x 4MN (dual dE/dobs), or null: not formed
  T* vecs;  // form 2: B x 4 Pv (dual x, g), uninitialised
};

template <class T, int FORM>
using second_args_t = std::conditional_t<FORM != 0, LargeSecondArgs<T>, SecondArgs<T>>;

template <class T, int RES, int FORM>
__global__ __launch_bounds__(kBlock, DualTraits<T>::kMinBlocks) void ba_second_order_kernel(second_args_t<T, FORM> a) {
  using D = DualT<T>;
  T* lds = dual_lds<T>();
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, MN = M * N;
  const int tid = threadIdx.x;
  const typename DualTraits<T>::block_index b = blockIdx.x;
  const DualCarve cv = carve_dual<T, FORM>(M, N, a.Pv);
  T* vec = lds;  // the dual x and gradient: LDS, or (form 2) this problem's workspace slice
  if constexpr (FORM == 2) vec = a.vecs + (size_t)b * 4 * a.Pv;
  D* x = reinterpret_cast<D*>(vec + cv.x);
  D* g = reinterpret_cast<D*>(vec + cv.g);
  D* views = reinterpret_cast<D*>(lds + cv.views);
  D* vpart = reinterpret_cast<D*>(lds + cv.vpart);
  D* obsd = reinterpret_cast<D*>(lds + cv.obsd);
  if constexpr (FORM != 0) obsd = a.obsd ? reinterpret_cast<D*>(a.obsd + (size_t)b * 4 * MN) : nullptr;
  T* scratch = lds + cv.scratch;
  T* obl = lds + cv.obs;  // form 0: the scene's LDS copy
  uint8_t* vil = reinterpret_cast<uint8_t*>(lds) + cv.vis_bytes_off;
  const T* obs = obl;
  const uint8_t* vis = vil;
  for (int i = tid; i < a.Pv; i += kBlock) {
    x[i] = i < P ? D(a.x[(size_t)b * P + i], a.v ? a.v[(size_t)b * P + i] : T(0)) : D(T(0));
    g[i] = D(T(0));
  }
  if constexpr (FORM == 0) {
    for (int i = tid; i < 2 * MN; i += kBlock) obl[i] = a.obs[(size_t)b * 2 * MN + i];
    for (int i = tid; i < MN; i += kBlock) vil[i] = a.vis[(size_t)b * MN + i] ? 1 : 0;
  } else {  // the scene where the caller put it
    obs = a.obs + (size_t)b * 2 * MN;
    vis = a.vis + (size_t)b * MN;
  }
  __syncthreads();
  int buf = 0;
  D E(T(0)), unused(T(0));
  ba_eval<true, false, false, false, false, RES, D>(L, x, nullptr, T(0), obs, vis, g, views, vpart, scratch, buf, E,
                                                    unused, obsd, nullptr,
                                                    a.obs_v ? a.obs_v + (size_t)b * 2 * MN : nullptr);
  if (tid == 0 && a.err) a.err[b] = E.v;
  for (int i = tid; i < P; i += kBlock) {
    if (a.grad) a.grad[(size_t)b * P + i] = g[i].v;
    if (a.hv) a.hv[(size_t)b * P + i] = g[i].t;
  }
  // dE/dobs was written per (view, point) pair by its owner thread; the eval's final barrier makes it visible
  if (FORM == 0 || obsd) {
    for (int i = tid; i < 2 * MN; i += kBlock) {
      if (a.obs_grad) a.obs_grad[(size_t)b * 2 * MN + i] = obsd[i].v;
      if (a.obs_hv) a.obs_hv[(size_t)b * 2 * MN + i] = obsd[i].t;
    }
  }
}

// ---- host side ----
template <class T>
struct SecondPlan {
  int status;
  bool launch;  // false: return `status` (a refusal, or DAVA_OK for an empty batch)
  int form, lds, batch, residual;
  size_t obsd_bytes;        // forms 1 and 2 with an observation output: B x 4MN elements, else 0
  size_t vector_bytes;      // form 2: B x 4 Pv elements, else 0
  LargeSecondArgs<T> args;  // the form-0 kernel takes its base
  size_t workspace_bytes() const { return obsd_bytes + vector_bytes + kTailBytes; }
};

// What a scene needs, from its shape alone (obs_out: an observation output is asked for): the queries and the
// launch's checks read the same numbers.  check_scene(sc, ...) must have passed.
template <class T>
SecondPlan<T> second_shape(const DavaScene& sc, bool obs_out, bool any_form) {
  SecondPlan<T> p{};
  const int M = sc.num_views, N = sc.num_points, Pv = round_up(sc.num_parameters, 4);
  p.status = DAVA_ERR_UNSUPPORTED;
  p.form = any_form ? choose_dual_form<T>(sc) : dual_fits_form0<T>(sc) ? 0 : -1;
  if (p.form < 0) return p;
  p.status = DAVA_OK;
  p.lds = (int)carve_dual<T>(M, N, Pv, p.form).total_bytes;
  p.batch = sc.batch;
  p.residual = sc.residual;
  p.obsd_bytes = p.form != 0 && obs_out ? (size_t)sc.batch * 4 * M * N * sizeof(T) : 0;
  p.vector_bytes = p.form == 2 ? (size_t)sc.batch * 4 * Pv * sizeof(T) : 0;
  return p;
}

// the shape behind a host-only query (which looks at no data pointer)
template <class T, class Scene>
SecondPlan<T> second_query(const Scene* scene, bool obs_out) {
  DavaScene sc;
  SecondPlan<T> p{};
  p.form = -1;
  p.status = check_dual_scene(scene, false, sc);
  return p.status == DAVA_OK ? second_shape<T>(sc, obs_out, true) : p;
}

// the checks of the entry points, in their order
template <class T, class Scene>
SecondPlan<T> plan_second(const Scene* scene, const T* x, const T* direction, const T* obs_direction, T* error_out,
                          T* grad_out, T* hv_out, T* obs_grad_out, T* obs_hv_out, void* workspace,
                          size_t workspace_bytes, bool any_form) {
  SecondPlan<T> p{};
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  DavaScene sc;
  const int st = check_dual_scene(scene, true, sc);
  if (st != DAVA_OK) return refuse(st);
  if (sc.batch == 0) return refuse(DAVA_OK);
  if (!x) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  p = second_shape<T>(sc, obs_grad_out || obs_hv_out, any_form);
  if (p.status != DAVA_OK) return p;
  if (p.obsd_bytes + p.vector_bytes > 0 && (!workspace || workspace_bytes < p.workspace_bytes()))
    return refuse(DAVA_ERR_WORKSPACE);
  LargeSecondArgs<T>& a = p.args;
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
  a.obsd = p.obsd_bytes ? static_cast<T*>(workspace) : nullptr;
  a.vecs = p.form == 2 ? reinterpret_cast<T*>(static_cast<char*>(workspace) + p.obsd_bytes) : nullptr;
  p.launch = true;
  return p;
}

template <class T, int FORM>
int launch_second(const SecondPlan<T>& p, void* stream) {
  const second_args_t<T, FORM>& a = p.args;
  with_flag(p.residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
    constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
    launch_lds(ba_second_order_kernel<T, kRes, FORM>, p.batch, kBlock, p.lds, static_cast<hipStream_t>(stream), a);
  });
  return launched();
}

template <class T>
int run_second(const SecondPlan<T>& p, void* stream) {
  if (!p.launch) return p.status;
  if (p.form == 0) return launch_second<T, 0>(p, stream);
  return p.form == 1 ? launch_second<T, 1>(p, stream) : launch_second<T, 2>(p, stream);
}

}  // namespace dava
