// The reductions and matrix-vector products of the dense update's backward kernels: update_backward_kernel<T> and
// its siblings (bfgs_grad.hip, float32 and float64) and update_backward_large_f64_kernel (bfgs_grad_large_f64.hip).
// The helpers are shared; the two update-backward kernel bodies are not (bfgs_grad_large_f64.hip says why).
#pragma once

#include "dava_common.hpp"

namespace dava {

template <typename T>
__device__ __forceinline__ T block_total(T v, T* red) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// A v: one wave per row (coalesced along the row), result to out[i]
template <typename T, typename F>
__device__ __forceinline__ void rows_dot(int64_t n, const T* A, F&& v, T* out) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int64_t i = wave; i < n; i += kWaves) {
    T acc = 0;
    for (int64_t j = lane; j < n; j += kWave) acc += A[i * n + j] * v(j);
    acc = wave_sum(acc);
    if (lane == 0) out[i] = acc;
  }
}

// A^T u: one thread per column (consecutive threads -> consecutive columns)
template <typename T, typename F>
__device__ __forceinline__ void cols_dot(int64_t n, const T* A, F&& u, T* out) {
  for (int64_t j = threadIdx.x; j < n; j += kBlock) {
    T acc = 0;
    for (int64_t i = 0; i < n; ++i) acc += u(i) * A[i * n + j];
    out[j] = acc;
  }
}

}  // namespace dava
