// The legacy camera model's entry points: dava_l1_camera_evaluate_* and dava_l1_camera_vjp_* (the model itself,
// l1_body, is in camera_l1.hpp, shared with the fused legacy solve in camera_l1_solve.hip).
#include "camera_l1.hpp"

namespace dava {

template <typename T>
__global__ __launch_bounds__(kBlock) void l1_camera_kernel(L1Args<T> a) {
  const int64_t be = blockIdx.x;  // (b, e) flattened
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* g = a.grad ? a.grad + be * a.P : nullptr;
  l1_body<T, T>(a, l1_point(a, be), reinterpret_cast<T*>(smem), -1, g != nullptr, false,
                [&](T e) { if (a.err) a.err[be] = e; }, [&](int i, T v) { g[i] = v; });
}

// Reverse mode for autograd through the model, one forward-mode pass per input direction:
// workgroup (be, d) evaluates estimate be with tangent 1 on its input element d and contracts the
// output tangents with the cotangents, vjp[be, d] = e_bar[be] de/dd + sum_q g_bar[be, q] dg_q/dd
// (error_cot / grad_cot may be null).  The sum is per thread in a fixed order, then wave
// butterflies and the 4 wave partials in wave order: deterministic.
template <typename T>
__global__ __launch_bounds__(kBlock) void l1_camera_vjp_kernel(L1Args<T> a, int D, const T* error_cot,
                                                                const T* grad_cot, int detach_points, T* vjp) {
  const int64_t be = blockIdx.x / D;
  const int d = blockIdx.x % D;
  const T* gb = grad_cot ? grad_cot + be * a.P : nullptr;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T acc = T(0);
  l1_body<T, LDual<T>>(a, l1_point(a, be), reinterpret_cast<LDual<T>*>(smem), d, gb != nullptr, detach_points != 0,
                       [&](LDual<T> e) { if (error_cot) acc += error_cot[be] * e.t; },
                       [&](int i, LDual<T> v) { acc += gb[i] * v.t; });
  __shared__ T red[kWaves];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  acc = wave_sum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) vjp[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

template <typename T>
int l1_camera_vjp(int64_t batch, int32_t estimates, int32_t views, int32_t points, const T* focal, const T* cx,
                  const T* cy, const T* trans, const T* lie, const T* world, const T* target, const uint8_t* vis,
                  T min_z, T pixel_ratio, T max_grad, T scale, const T* error_cot, const T* grad_cot,
                  int32_t detach_points, T* vjp, void* stream) {
  if (batch < 0 || estimates < 0 || views < 1 || points < 3) return DAVA_ERR_INVALID_ARGUMENT;
  if (batch == 0 || estimates == 0) return DAVA_OK;
  if (!focal || !cx || !cy || !trans || !lie || !world || !target || !vis || !vjp) return DAVA_ERR_INVALID_ARGUMENT;
  const int64_t D = 3 + 6 * (int64_t)views + 3 * ((int64_t)points - 2);
  if (batch * estimates * D > 0x7fffffff) return DAVA_ERR_UNSUPPORTED;
  const size_t lds = grad_cot ? (size_t)views * points * 4 * sizeof(LDual<T>) : 0;
  if (lds > 150 * 1024) return DAVA_ERR_UNSUPPORTED;
  set_dynamic_lds(l1_camera_vjp_kernel<T>, (int)lds);
  const L1Args<T> a = l1_args(estimates, views, points, focal, cx, cy, trans, lie, world, target, vis, min_z,
                              pixel_ratio, max_grad, scale);
  hipLaunchKernelGGL(l1_camera_vjp_kernel<T>, dim3((unsigned)(batch * estimates * D)), dim3(kBlock), lds,
                     static_cast<hipStream_t>(stream), a, (int)D, error_cot, grad_cot, (int)detach_points, vjp);
  return launched();
}

template <typename T>
int l1_camera_evaluate(int64_t batch, int32_t estimates, int32_t views, int32_t points, const T* focal, const T* cx,
                       const T* cy, const T* trans, const T* lie, const T* world, const T* target,
                       const uint8_t* vis, T min_z, T pixel_ratio, T max_grad, T scale, T* err, T* grad,
                       void* stream) {
  if (batch < 0 || estimates < 0 || views < 1 || points < 3) return DAVA_ERR_INVALID_ARGUMENT;
  if (batch == 0 || estimates == 0) return DAVA_OK;
  if (!focal || !cx || !cy || !trans || !lie || !world || !target || !vis) return DAVA_ERR_INVALID_ARGUMENT;
  if (!err && !grad) return DAVA_OK;
  const size_t lds = grad ? (size_t)views * points * 4 * sizeof(T) : 0;
  if (lds > 150 * 1024) return DAVA_ERR_UNSUPPORTED;
  set_dynamic_lds(l1_camera_kernel<T>, (int)lds);
  L1Args<T> a = l1_args(estimates, views, points, focal, cx, cy, trans, lie, world, target, vis, min_z, pixel_ratio,
                        max_grad, scale);
  a.err = err; a.grad = grad;
  hipLaunchKernelGGL(l1_camera_kernel<T>, dim3((unsigned)(batch * estimates)), dim3(kBlock), lds,
                     static_cast<hipStream_t>(stream), a);
  return launched();
}

}  // namespace dava

using namespace dava;

#define DAVA_L1_ENTRY(SUFFIX, T)                                                                                 \
  extern "C" int dava_l1_camera_evaluate_##SUFFIX(                                                              \
      int64_t batch, int32_t estimates, int32_t views, int32_t points, const T* focal, const T* cx, const T* cy,  \
      const T* translation, const T* lie_vector, const T* world_points, const T* true_points,                    \
      const uint8_t* visibility, T minimum_z_distance, T inverse_pixel_ratio, T max_gradient, T error_scale,     \
      T* error_out, T* gradient_out, void* stream) {                                                             \
    return l1_camera_evaluate<T>(batch, estimates, views, points, focal, cx, cy, translation, lie_vector,        \
                                 world_points, true_points, visibility, minimum_z_distance, inverse_pixel_ratio, \
                                 max_gradient, error_scale, error_out, gradient_out, stream);                    \
  }

DAVA_L1_ENTRY(f32, float)
DAVA_L1_ENTRY(f64, double)

#define DAVA_L1_VJP_ENTRY(SUFFIX, T)                                                                             \
  extern "C" int dava_l1_camera_vjp_##SUFFIX(                                                                   \
      int64_t batch, int32_t estimates, int32_t views, int32_t points, const T* focal, const T* cx, const T* cy,  \
      const T* translation, const T* lie_vector, const T* world_points, const T* true_points,                    \
      const uint8_t* visibility, T minimum_z_distance, T inverse_pixel_ratio, T max_gradient, T error_scale,     \
      const T* error_cotangent, const T* gradient_cotangent, int32_t detach_points, T* input_cotangent_out,      \
      void* stream) {                                                                                            \
    return l1_camera_vjp<T>(batch, estimates, views, points, focal, cx, cy, translation, lie_vector,            \
                            world_points, true_points, visibility, minimum_z_distance, inverse_pixel_ratio,      \
                            max_gradient, error_scale, error_cotangent, gradient_cotangent, detach_points,       \
                            input_cotangent_out, stream);                                                        \
  }

DAVA_L1_VJP_ENTRY(f32, float)
DAVA_L1_VJP_ENTRY(f64, double)
