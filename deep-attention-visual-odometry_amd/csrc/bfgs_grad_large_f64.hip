// The float64 backward of the dense inverse-Hessian update beyond its LDS image
// (dava_bfgs_update_inverse_hessian_backward_large_f64, with the host-only query
// dava_bfgs_update_inverse_hessian_backward_large_workspace_bytes_f64).
//
// update_backward_kernel<double> (bfgs_grad.hip) keeps its nine O(n) vectors in LDS and refuses 9 n 8 > 150 KiB,
// n > 2133 -- where the generic loop's graph through a float64 solve of a large scene (dense mode, the
// GENERIC_BACKWARD override) needs it: (2, 1200) has n = 3609.  This is that kernel's text with the nine vectors in
// a per-problem slice of a workspace, B x 9 x n doubles: the same formulas (its header comment), the same passes,
// the same reduction trees (the three helpers of bfgs_grad_helpers.hpp, shared with that kernel), so the same bits
// where both run.  The two kernel bodies stay two texts: one force-inlined body taking the vectors' and the
// reduction buffer's pointers, called from both kernels (tried with and without __restrict__ on its parameters),
// made the compiler reschedule update_backward_kernel<float> and <double> -- 7,180 -> 7,192 bytes of code, about
// 700 listing lines -- and that kernel is float32's too.  One 256-thread workgroup per problem, which
// touches only its own slice and writes every vector before it reads it; __syncthreads() is the only
// synchronisation (it orders a workgroup's global accesses as it does its LDS ones); no queue, no spin-wait.
// Where the LDS kernel takes the shape the launch is dava_bfgs_update_inverse_hessian_backward_f64's, unless the
// F64_FORM override (1 | 2) asks for the workspace, as it raises the forms of solve_f64.hpp.
#include "bfgs_grad_helpers.hpp"
#include "dava_debug.hpp"

namespace dava {
namespace {

constexpr int kVectors = 9;                  // yH Hy Gs GyH GTsr GTHy yHbar t1 t2
constexpr size_t kLdsLimit = 150 * 1024;     // update_backward (bfgs_grad.hip)
constexpr size_t kTail = 256;

__global__ __launch_bounds__(kBlock) void update_backward_large_f64_kernel(int64_t n, const double* __restrict__ h,
                                                                           const double* __restrict__ s,
                                                                           const double* __restrict__ y,
                                                                           const double* __restrict__ g,
                                                                           double* __restrict__ gh, double* __restrict__ gs,
                                                                           double* __restrict__ gy, double* vecs) {
  __shared__ double red[kWaves];
  const int64_t b = blockIdx.x;
  double* yH = vecs + b * kVectors * n;
  double* Hy = yH + n;
  double* Gs = Hy + n;
  double* GyH = Gs + n;
  double* GTsr = GyH + n;
  double* GTHy = GTsr + n;
  double* yHbar = GTHy + n;
  double* t1 = yHbar + n;
  double* t2 = t1 + n;
  const double* H = h + b * n * n;
  const double* G = g + b * n * n;
  const double* sv = s + b * n;
  const double* yv = y + b * n;
  const int tid = threadIdx.x;

  cols_dot(n, H, [&](int64_t i) { return yv[i]; }, yH);
  rows_dot(n, H, [&](int64_t j) { return yv[j]; }, Hy);
  double sy = 0;
  for (int64_t i = tid; i < n; i += kBlock) sy += sv[i] * yv[i];
  sy = block_total(sy, red);  // (barriers publish yH / Hy)
  const double r = sy <= 0.0 ? 0.0 : 1.0 / sy;
  double gip = 0, yyh = 0;
  for (int64_t j = tid; j < n; j += kBlock) {
    gip += yH[j] * (yv[j] * r);
    yyh += yv[j] * yH[j];
  }
  gip = block_total(gip, red);
  yyh = block_total(yyh, red);
  const double q = 1.0 + gip;

  rows_dot(n, G, [&](int64_t j) { return sv[j]; }, Gs);
  rows_dot(n, G, [&](int64_t j) { return yH[j]; }, GyH);
  cols_dot(n, G, [&](int64_t i) { return sv[i] * r; }, GTsr);
  cols_dot(n, G, [&](int64_t i) { return Hy[i]; }, GTHy);
  __syncthreads();
  double gipbar = 0;
  for (int64_t i = tid; i < n; i += kBlock) gipbar += (sv[i] * r) * Gs[i];
  gipbar = block_total(gipbar, red);
  for (int64_t j = tid; j < n; j += kBlock) yHbar[j] = gipbar * (yv[j] * r) - GTsr[j];
  __syncthreads();
  // Hybar_i = -r Gs_i
  rows_dot(n, H, [&](int64_t j) { return yHbar[j]; }, t1);
  cols_dot(n, H, [&](int64_t i) { return -1.0 * r * Gs[i]; }, t2);
  double rbar = 0;
  for (int64_t i = tid; i < n; i += kBlock) rbar += sv[i] * (q * Gs[i] - GyH[i] - GTHy[i]);
  rbar = block_total(rbar, red) + gipbar * yyh;  // (barriers publish t1 / t2)
  const double go = -1.0 * r * r * rbar;
  for (int64_t i = tid; i < n; i += kBlock) {
    const double sbar_r = q * Gs[i] - GyH[i] - GTHy[i];
    if (gs) gs[b * n + i] = q * GTsr[i] + r * sbar_r + go * yv[i];
    if (gy) gy[b * n + i] = t1[i] + t2[i] + r * gipbar * yH[i] + go * sv[i];
  }
  if (gh) {
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    for (int64_t i = wave; i < n; i += kWaves) {
      const double yi = yv[i], hyb = -1.0 * r * Gs[i];
      for (int64_t j = lane; j < n; j += kWave) gh[b * n * n + i * n + j] = G[i * n + j] + yi * yHbar[j] + hyb * yv[j];
    }
  }
}

// does this shape take the workspace kernel?
bool in_workspace(int64_t n) {
  const long long forced = debug_knob(kDbgF64Form);
  return kVectors * (size_t)n * sizeof(double) > kLdsLimit || forced == 1 || forced == 2;
}

}  // namespace
}  // namespace dava

using namespace dava;

extern "C" size_t dava_bfgs_update_inverse_hessian_backward_large_workspace_bytes_f64(int64_t batch, int64_t n) {
  if (batch <= 0 || n <= 0 || !in_workspace(n)) return 0;
  return (size_t)batch * kVectors * (size_t)n * sizeof(double) + kTail;
}

extern "C" int dava_bfgs_update_inverse_hessian_backward_large_f64(int64_t batch, int64_t n, const double* h,
                                                                   const double* s, const double* y,
                                                                   const double* grad_out, double* grad_h,
                                                                   double* grad_s, double* grad_y, void* workspace,
                                                                   size_t workspace_bytes, void* stream) {
  if (batch < 0 || n < 0) return DAVA_ERR_INVALID_ARGUMENT;
  if (batch == 0 || n == 0) return DAVA_OK;
  if (!h || !s || !y || !grad_out) return DAVA_ERR_INVALID_ARGUMENT;
  if (!in_workspace(n))  // the nine vectors fit LDS: the launch of dava_bfgs_update_inverse_hessian_backward_f64
    return dava_bfgs_update_inverse_hessian_backward_f64(batch, n, h, s, y, grad_out, grad_h, grad_s, grad_y, stream);
  if (!workspace || workspace_bytes < (size_t)batch * kVectors * (size_t)n * sizeof(double) + kTail)
    return DAVA_ERR_WORKSPACE;
  hipLaunchKernelGGL(update_backward_large_f64_kernel, dim3((unsigned)batch), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), n, h, s, y, grad_out, grad_h, grad_s, grad_y,
                     static_cast<double*>(workspace));
  return launched();
}
