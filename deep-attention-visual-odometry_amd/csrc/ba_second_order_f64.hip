// Second derivatives of the fused BA objectives in float64 (dava_ba_second_order_f64): the float64 counterpart
// of ba_second_order.hip.  The SAME objective code (ba_objective.hpp) instantiated with dual numbers over
// double (DualT<double>, dava_dual.hpp), x seeded with the tangent v and the observations with the tangent u:
// E, dE/dx, H v + (d2E/dx dobs) u, dE/dobs and (d2E/dobs dx) v + (d2E/dobs2) u, one launch, one 256-thread
// workgroup per problem with the dual image in LDS.  This is what the float64 objective's create_graph double
// backward and the generic loop's graph through a float64 solve need (bfgs_solver.py:133-135).
#include "ba_objective.hpp"
#include "dava_f64.hpp"

namespace dava {
namespace f64 {

using Dual64 = DualT<double>;

struct SecondArgs {
  Layout L;
  int Pv;
  const double *obs, *x, *v, *obs_v;
  const uint8_t* vis;
  double *err, *grad, *hv, *obs_grad, *obs_hv;
};

struct SecondCarve {
  int x, g, views, vpart, obsd, scratch, obs, vis_bytes_off;  // offsets in doubles
  long long total_bytes;
};

__host__ __device__ inline SecondCarve carve_second(int M, int N, int Pv) {
  SecondCarve c{};
  const long long MN = (long long)M * N;
  const long long doubles = 4LL * Pv + 2LL * views_floats(M) + 2LL * vpart_floats(M) + 4 * MN + 2 * kWaves * 32 + 2 * MN;
  c.total_bytes = doubles * 8 + round_up((int)(MN < (1 << 30) ? MN : (1 << 30)), 16);
  if (c.total_bytes > kMaxLdsBytes) return c;  // (offsets are meaningful only for an image that fits)
  int off = 0;
  c.x = off; off += 2 * Pv;                  // Dual64
  c.g = off; off += 2 * Pv;                  // Dual64
  c.views = off; off += 2 * views_floats(M);  // Dual64
  c.vpart = off; off += 2 * vpart_floats(M);  // Dual64
  c.obsd = off; off += 4 * (int)MN;          // Dual64 dE/dobs
  c.scratch = off; off += 2 * kWaves * 32;
  c.obs = off; off += 2 * (int)MN;
  c.vis_bytes_off = off * 8;
  return c;
}

template <int RES>
__global__ __launch_bounds__(kBlock, 1) void ba_second_order_f64_kernel(SecondArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, MN = M * N;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const SecondCarve cv = carve_second(M, N, a.Pv);
  Dual64* x = reinterpret_cast<Dual64*>(lds64 + cv.x);
  Dual64* g = reinterpret_cast<Dual64*>(lds64 + cv.g);
  Dual64* views = reinterpret_cast<Dual64*>(lds64 + cv.views);
  Dual64* vpart = reinterpret_cast<Dual64*>(lds64 + cv.vpart);
  Dual64* obsd = reinterpret_cast<Dual64*>(lds64 + cv.obsd);
  double* scratch = lds64 + cv.scratch;
  double* obs = lds64 + cv.obs;
  uint8_t* vis = reinterpret_cast<uint8_t*>(lds64) + cv.vis_bytes_off;
  for (int i = tid; i < a.Pv; i += kBlock) {
    x[i] = i < P ? Dual64(a.x[b * P + i], a.v ? a.v[b * P + i] : 0.0) : Dual64(0.0);
    g[i] = Dual64(0.0);
  }
  for (int i = tid; i < 2 * MN; i += kBlock) obs[i] = a.obs[b * 2 * MN + i];
  for (int i = tid; i < MN; i += kBlock) vis[i] = a.vis[b * MN + i] ? 1 : 0;
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
  for (int i = tid; i < 2 * MN; i += kBlock) {
    if (a.obs_grad) a.obs_grad[b * 2 * MN + i] = obsd[i].v;
    if (a.obs_hv) a.obs_hv[b * 2 * MN + i] = obsd[i].t;
  }
}

template <int RES>
static void launch_second(const SecondArgs& a, int B, int lds, hipStream_t s) {
  set_dynamic_lds(ba_second_order_f64_kernel<RES>, lds);
  hipLaunchKernelGGL(ba_second_order_f64_kernel<RES>, dim3(B), dim3(kBlock), lds, s, a);
}

}  // namespace f64
}  // namespace dava

using namespace dava;

extern "C" int dava_ba_second_order_f64(const DavaSceneF64* scene, const double* x, const double* direction,
                                        const double* obs_direction, double* error_out, double* grad_out,
                                        double* hv_out, double* obs_grad_out, double* obs_hv_out, void* stream) {
  DavaScene sc;
  const int st = f64::check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return st;
  if (sc.batch == 0) return DAVA_OK;
  if (!x) return DAVA_ERR_INVALID_ARGUMENT;
  const int Pv = round_up(sc.num_parameters, 4);
  const f64::SecondCarve cv = f64::carve_second(sc.num_views, sc.num_points, Pv);
  if (cv.total_bytes > f64::kMaxLdsBytes) return DAVA_ERR_UNSUPPORTED;
  f64::SecondArgs a;
  a.L = make_layout(&sc);
  a.Pv = Pv;
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
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int lds = (int)cv.total_bytes;
  if (sc.residual == DAVA_RESIDUAL_RAY_ANGLE) f64::launch_second<DAVA_RESIDUAL_RAY_ANGLE>(a, sc.batch, lds, s);
  else f64::launch_second<DAVA_RESIDUAL_SQUARED_REPROJECTION>(a, sc.batch, lds, s);
  return hipGetLastError() == hipSuccess ? DAVA_OK : DAVA_ERR_LAUNCH;
}
