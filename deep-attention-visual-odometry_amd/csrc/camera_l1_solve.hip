// The legacy solver fused: BFGSCameraSolver.forward with LineSearchStrongWolfeConditions inside it, over a
// PinholeCameraModelL1, in ONE launch -- one workgroup per (batch item, estimate), float32 and float64.
//
// Restated from solvers/bfgs_camera_solver.py and solvers/line_search_strong_wolfe_conditions.py of this package
// (themselves pinned to the reference), statement for statement; every evaluation is l1_body (camera_l1.hpp).
//
// State of one estimate (LDS, elements of T):
//   pp      [M][N][4]   l1_body's scratch
//   slots   4 x SLOT    a model each: parameters [D] (focal, cx, cy, translation [M][3], lie [M][3], world [N-2][3]),
//                       its gradient [P], its error, its slope along the iteration's direction.  The Python keeps
//                       function / fn_lo / fn_hi / out_fn / trial as objects that alias one another; here they are
//                       slot indices, so masked_update is an index assignment and a model's cached error and
//                       gradient travel with it exactly as merge_cached_values carries them.  A trial takes a
//                       slot that function, fn_lo and fn_hi do not name; four slots always leave one.
//   d, y, yH, Hy  [P]   search direction, gradient difference, and the rank-2 update's two products
//   H       [P][P]      form 0: here; form 1: this estimate's slice of the caller's workspace
// Per estimate the line search's masks are plain booleans: the widening loop ends when `widen` clears, the zoom
// loop when `zoom` clears, and the solve when `updating` clears (only masked_update(next, updating) writes the
// returned parameters, so nothing the loop does afterwards can be seen).
//
// Arithmetic outside l1_body is compiled without contraction: torch rounds every elementwise operation, and
// alpha * d is a rounded step both when it moves the model and when it enters the BFGS update.
// Reductions: per-thread strided partials, wave butterflies, wave partials in wave order -- deterministic.
#include "camera_l1.hpp"
#include "dava_debug.hpp"

// (l1_body is defined above this pragma and keeps the build's default contraction, as in camera_l1.hip.  That a
// trial's error here is bitwise dava_l1_camera_evaluate's -- the cached error a fused call returns equals a fresh
// get_error() -- relies on the compiler contracting the same inlined body the same way in both kernels; it is
// checked with torch.equal by tests/test_gpu_l1_solve.py::test_fused_matches_the_loop_on_the_same_tensors.)
#pragma clang fp contract(off)

namespace dava {

constexpr size_t kL1SolveLds = 150 * 1024;  // dynamic LDS limit, the evaluation entry's

__host__ __device__ inline int l1_slot_elems(int P) { return round_up(2 * P + 3, 2); }  // D + P + error + slope

template <typename T>
struct L1SolveArgs {
  L1Args<T> m;      // the scene and the INPUT model's constants
  T derived_ratio;  // the inverse pixel ratio of every model add() / masked_update() makes
  int K, W, Z, constrain;
  T eps, max_dist, min_dist, max_step, c1, c2, sscale;
  T *focal_o, *cx_o, *cy_o, *trans_o, *lie_o, *world_o, *err_o;
  int32_t* iters_o;
  T *tr_err, *tr_alpha;
  int32_t* tr_exit;
  T* hws;  // form 1: (B E, P, P)
};

template <typename T>
__device__ __forceinline__ T l1s_block_sum(T v, T* red) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// torch.max / torch.minimum / torch.maximum: NaN wins
template <typename T>
__device__ __forceinline__ T nan_max(T a, T b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
template <typename T>
__device__ __forceinline__ T nan_min(T a, T b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

template <typename T>
__device__ __forceinline__ T l1s_block_max(T v, T* red) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = nan_max(v, __shfl_xor(v, off, kWave));
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return nan_max(nan_max(nan_max(red[0], red[1]), red[2]), red[3]);
}

// utils.secant_alpha's forward: the root of the line through (a1, v1), (a2, v2); the midpoint where the line is
// flat or the root is not 1e-3 inside the bracket; a NaN root is kept (its comparisons are false)
template <typename T>
__device__ __forceinline__ T secant_alpha(T a1, T a2, T v1, T v2) {
  const T low = nan_min(a1, a2), high = nan_max(a1, a2);
  const T rise = v2 - v1;
  const T run_over_rise = (a2 - a1) / rise;
  const T root = a1 - v1 * run_over_rise;
  const bool midpoint = rise == T(0) || root < low + T(1e-3) || root > high - T(1e-3);
  return midpoint ? (a1 + a2) / T(2) : root;
}

__device__ __forceinline__ int l1s_free_slot(int a, int b, int c) {
  int s = 0;
  while (s == a || s == b || s == c) ++s;
  return s;  // < 4: three names leave one of four slots
}

template <typename T, int FORM>
__global__ __launch_bounds__(kBlock) void l1_solve_kernel(L1SolveArgs<T> a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ T red[kWaves];
  const int M = a.m.M, N = a.m.N, P = a.m.P, D = P + 1;
  const int SLOT = l1_slot_elems(P);
  const int ERR = D + P, SLOPE = D + P + 1;  // within a slot
  const int64_t be = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  T* pp = reinterpret_cast<T*>(smem);
  T* slots = pp + (size_t)M * N * 4;
  T* d = slots + 4 * SLOT;
  T* y = d + P;
  T* yH = y + P;
  T* Hy = yH + P;
  T* H;
  if constexpr (FORM == 0) H = Hy + P;
  else H = a.hws + (size_t)be * P * P;
  const L1Point<T> in = l1_point(a.m, be);
  // add()'s parameter offsets (pinhole_camera_model_l1.py add): cx, cy, f, a, b, c, tx, ty, tz, x, y, z
  const int ia = 3, itx = 3 + 3 * M, ix = 3 + 6 * M, iy = ix + (N - 2), iz = iy + (N - 2);
  // a slot's parameter offsets
  const int st = 3, sl = 3 + 3 * M, sw = 3 + 6 * M;

  auto slot = [&](int s) { return slots + s * SLOT; };
  // error and gradient of slot s, as a model with inverse pixel ratio `ratio`
  auto evaluate = [&](int s, T ratio) {
    T* X = slot(s);
    L1Args<T> m = a.m;
    m.pixel_ratio = ratio;
    const L1Point<T> pt{X, X + 1, X + 2, X + st, X + sl, X + sw, in.target, in.vis};
    T* g = X + D;
    __syncthreads();  // the slot's parameters are written
    l1_body<T, T>(m, pt, pp, -1, true, false, [&](T e) { X[ERR] = e; }, [&](int i, T v) { g[i] = v; });
    __syncthreads();
  };
  // slope(fn): sum(scale * gradient * d)
  auto set_slope = [&](int s) {
    T* X = slot(s);
    const T* g = X + D;
    T acc = T(0);
    for (int i = tid; i < P; i += kBlock) acc += (a.sscale * g[i]) * d[i];
    acc = l1s_block_sum(acc, red);
    if (tid == 0) X[SLOPE] = acc;
    __syncthreads();
  };
  // slot t = slot fn .add(alpha * d), by a model whose inverse pixel ratio is `ratio`
  auto make_trial = [&](int t, int fn, T alpha, T ratio) {
    const T* X = slot(fn);
    T* Y = slot(t);
    for (int i = tid; i < D; i += kBlock) {
      if (i == 0) {
        const T v = X[0] + alpha * d[2];
        Y[0] = a.constrain ? clip(v, ratio, T(1e3)) : v;
      } else if (i < 3) {
        const T v = X[i] + alpha * d[i - 1];
        Y[i] = a.constrain ? clip(v, T(-1), T(1)) : v;
      } else if (i < sl) {
        const int k = i - st, m = k / 3, c = k - 3 * m;
        Y[i] = X[i] + alpha * d[itx + c * M + m];
      } else if (i >= sw) {
        const int k = i - sw, p = k / 3, c = k - 3 * p;
        const T step = c == 0 ? alpha * d[ix + p] : c == 1 ? alpha * d[iy + p] : p == 0 ? T(0) : alpha * d[iz + p - 1];
        Y[i] = X[i] + step;
      }
    }
    for (int m = tid; m < M; m += kBlock) {  // LieRotation.add_lie_parameters
      const T* w = X + sl + 3 * m;
      T n0 = w[0] + alpha * d[ia + m], n1 = w[1] + alpha * d[ia + M + m], n2 = w[2] + alpha * d[ia + 2 * M + m];
      if (a.constrain) {  // keep the angle in [-pi, pi)
        const T pi = T(3.141592653589793238462643383279502884);
        T angle = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
        const T den = clamp_min(angle, T(1e-8));
        const T a0 = n0 / den, a1 = n1 / den, a2 = n2 / den;
        angle = fmod(angle + pi, T(2) * pi) - pi;
        n0 = angle * a0; n1 = angle * a1; n2 = angle * a2;
      }
      T* o = Y + sl + 3 * m;
      o[0] = n0; o[1] = n1; o[2] = n2;
    }
  };

  {
    T* X = slot(0);
    for (int i = tid; i < D; i += kBlock)
      X[i] = i == 0 ? *in.focal : i == 1 ? *in.cx : i == 2 ? *in.cy
           : i < sl ? in.trans[i - st] : i < sw ? in.lie[i - sl] : in.world[i - sw];
  }
  int fn = 0;
  evaluate(fn, a.m.pixel_ratio);
  int iterations = 0;
  for (int it = 0; it < a.K; ++it) {
    const T* g = slot(fn) + D;
    // ---- search direction: -g, then -H g; clamp_search_direction ----
    if (it == 0) {
      for (int i = tid; i < P; i += kBlock) d[i] = T(-1) * g[i];
    } else {
      for (int i = wave; i < P; i += kWaves) {
        T acc = T(0);
        for (int j = lane; j < P; j += kWave) acc += H[(size_t)i * P + j] * g[j];
        acc = wave_sum(acc);
        if (lane == 0) d[i] = T(-1) * acc;
      }
    }
    __syncthreads();
    {
      T big = T(0);
      for (int i = tid; i < P; i += kBlock) big = nan_max(big, fabs(d[i]));
      const T largest = clamp_min(l1s_block_max(big, red), T(1e-8));
      T sc = T(1);
      if (largest > a.max_dist) sc = a.max_dist / largest;
      if (largest < a.min_dist) sc = a.min_dist / largest;
      sc = clamp_min(sc, T(1e-16));
      for (int i = tid; i < P; i += kBlock) d[i] = sc * d[i];  // (each thread its own elements)
      __syncthreads();
    }
    // ---- LineSearchStrongWolfeConditions.forward ----
    set_slope(fn);
    const T f0 = a.sscale * slot(fn)[ERR], slope0 = slot(fn)[SLOPE];
    const T curvature_bound = (T(-1) * a.c2) * slope0;
    const T add_ratio = it == 0 ? a.m.pixel_ratio : a.derived_ratio;  // function is the input model only once
    int lo = fn, hi = fn, out = fn, exit_code = 0;
    T a_lo = T(0), a_hi = T(1), f_prev = f0, alpha_out = T(0);
    bool widen = true, zoom = false, done = false;
    for (int w = 0; w < a.W && widen; ++w) {  // widening (N&W 3.5)
      const int t = l1s_free_slot(fn, lo, hi);
      make_trial(t, fn, a_hi, add_ratio);
      evaluate(t, a.derived_ratio);
      set_slope(t);
      hi = t;
      const T f = a.sscale * slot(hi)[ERR];
      bool rising = f > f0 + (a.c1 * a_hi) * slope0;
      if (w > 0) rising = rising || f >= f_prev;
      if (rising) { zoom = true; widen = false; break; }
      const T s = slot(hi)[SLOPE];
      if (fabs(s) <= curvature_bound) { out = hi; alpha_out = a_hi; done = true; exit_code = 1; widen = false; break; }
      if (s >= T(0)) {  // swap: the trial becomes the lower end
        const T ta = a_lo; a_lo = a_hi; a_hi = ta;
        const int ts = lo; lo = hi; hi = ts;
        zoom = true; widen = false;
        break;
      }
      a_lo = a_hi;
      a_hi = T(2) * a_hi < a.max_step ? T(2) * a_hi : a.max_step;
      lo = hi;
      f_prev = f;
    }
    for (int z = 0; z < a.Z && zoom; ++z) {  // zoom (N&W 3.6), secant on the slopes
      const T alpha = secant_alpha(a_lo, a_hi, slot(lo)[SLOPE], slot(hi)[SLOPE]);
      const int t = l1s_free_slot(fn, lo, hi);
      make_trial(t, fn, alpha, add_ratio);
      evaluate(t, a.derived_ratio);
      set_slope(t);
      const T f_lo = a.sscale * slot(lo)[ERR], f = a.sscale * slot(t)[ERR];
      bool rising = f > f0 + (a.c1 * alpha) * slope0;
      rising = f >= f_lo || rising;
      if (rising) { a_hi = alpha; hi = t; continue; }
      const T s = slot(t)[SLOPE];
      if (fabs(s) <= curvature_bound) { out = t; alpha_out = alpha; done = true; exit_code = 2; zoom = false; break; }
      if (s * (a_hi - a_lo) >= T(0)) { a_hi = a_lo; hi = lo; }
      a_lo = alpha;
      lo = t;
    }
    if (!done) {  // unfinished: the upper bracket rather than no step
      out = hi;
      alpha_out = a_hi;
      exit_code = zoom ? 4 : 3;
    }
    // ---- back in BFGSCameraSolver.forward: function = masked_update(next, updating); updating &= error > eps ----
    const T* gn = slot(out) + D;
    for (int i = tid; i < P; i += kBlock) y[i] = gn[i] - g[i];
    const T err = slot(out)[ERR];
    if (tid == 0) {
      const int64_t k = be * a.K + it;
      if (a.tr_err) a.tr_err[k] = err;
      if (a.tr_alpha) a.tr_alpha[k] = alpha_out;
      if (a.tr_exit) a.tr_exit[k] = exit_code;
    }
    iterations = it + 1;
    const bool last = !(err > a.eps) || it == a.K - 1;
    if (last) { fn = out; break; }  // (H is not read again)
    __syncthreads();  // y
    if (it == 0) {  // estimate_initial_inverse_hessian: (s.y / clamp(y.y, 1e-5)) I
      T yy = T(0), sy = T(0);
      for (int i = tid; i < P; i += kBlock) { yy += y[i] * y[i]; sy += (alpha_out * d[i]) * y[i]; }
      yy = l1s_block_sum(yy, red);
      sy = l1s_block_sum(sy, red);
      const T gamma = sy / clamp_min(yy, T(1e-5));
      for (int i = wave; i < P; i += kWaves)
        for (int j = lane; j < P; j += kWave) H[(size_t)i * P + j] = gamma * (i == j ? T(1) : T(0));
      __syncthreads();
    }
    // update_inverse_hessian (bfgs_ops.hip's formula), in place: every element depends on itself, yH and Hy only
    for (int j = tid; j < P; j += kBlock) {
      T acc = T(0);
      for (int i = 0; i < P; ++i) acc += y[i] * H[(size_t)i * P + j];
      yH[j] = acc;
    }
    for (int i = wave; i < P; i += kWaves) {
      T acc = T(0);
      for (int j = lane; j < P; j += kWave) acc += H[(size_t)i * P + j] * y[j];
      acc = wave_sum(acc);
      if (lane == 0) Hy[i] = acc;
    }
    T sy = T(0);
    for (int i = tid; i < P; i += kBlock) sy += (alpha_out * d[i]) * y[i];
    sy = l1s_block_sum(sy, red);
    const T rho = sy <= T(0) ? T(0) : T(1) / sy;
    T yhy = T(0);
    for (int j = tid; j < P; j += kBlock) yhy += yH[j] * (y[j] * rho);
    yhy = l1s_block_sum(yhy, red);  // (its barriers also publish yH / Hy)
    const T c = T(1) + yhy;
    for (int i = wave; i < P; i += kWaves) {
      const T sri = (alpha_out * d[i]) * rho, hyi = Hy[i];
      for (int j = lane; j < P; j += kWave) {
        const T sj = alpha_out * d[j], srj = sj * rho;
        T t = H[(size_t)i * P + j] + (sri * sj) * c;
        t = t - sri * yH[j];
        H[(size_t)i * P + j] = t - hyi * srj;
      }
    }
    fn = out;
    __syncthreads();
  }
  // ---- outputs: the (frozen) point, its cached error, the iterations it was updated in ----
  const T* X = slot(fn);
  const T err = X[ERR];
  for (int i = tid; i < D; i += kBlock) {
    if (i == 0) a.focal_o[be] = X[0];
    else if (i == 1) a.cx_o[be] = X[1];
    else if (i == 2) a.cy_o[be] = X[2];
    else if (i < sl) a.trans_o[be * 3 * M + (i - st)] = X[i];
    else if (i < sw) a.lie_o[be * 3 * M + (i - sl)] = X[i];
    else a.world_o[be * 3 * (int64_t)(N - 2) + (i - sw)] = X[i];
  }
  if (tid == 0) {
    a.err_o[be] = err;
    a.iters_o[be] = iterations;
  }
  for (int k = iterations + tid; k < a.K; k += kBlock) {  // frozen iterations
    if (a.tr_err) a.tr_err[be * a.K + k] = err;
    if (a.tr_alpha) a.tr_alpha[be * a.K + k] = T(0);
    if (a.tr_exit) a.tr_exit[be * a.K + k] = 0;
  }
}

// ---- host ----
template <typename T>
size_t l1_solve_lds_bytes(int M, int N, int form) {
  const size_t P = 3 + 6 * (size_t)M + 3 * (size_t)N - 7;
  const size_t elems = (size_t)M * N * 4 + 4 * (size_t)l1_slot_elems((int)P) + 4 * P + (form == 0 ? P * P : 0);
  return elems * sizeof(T);
}

// 0: H in LDS; 1: H in the workspace; -1: not even form 1's image fits.  L1_SOLVE_FORM raises, never lowers.
template <typename T>
int l1_solve_form(int32_t views, int32_t points) {
  if (views < 1 || points < 4) return -1;
  if ((size_t)views * points * 4 * sizeof(T) > kL1SolveLds) return -1;  // the evaluation's own limit
  if (l1_solve_lds_bytes<T>(views, points, 1) > kL1SolveLds) return -1;
  int form = l1_solve_lds_bytes<T>(views, points, 0) <= kL1SolveLds ? 0 : 1;
  if (debug_knob(kDbgL1SolveForm) == 1 && form < 1) form = 1;
  return form;
}

template <typename T>
size_t l1_solve_workspace_bytes(int64_t batch, int32_t estimates, int32_t views, int32_t points) {
  if (batch <= 0 || estimates <= 0 || l1_solve_form<T>(views, points) != 1) return 0;
  const size_t P = 3 + 6 * (size_t)views + 3 * (size_t)points - 7;
  return (size_t)batch * estimates * P * P * sizeof(T);
}

template <typename T>
int l1_camera_solve(int64_t batch, int32_t estimates, int32_t views, int32_t points, const T* focal, const T* cx,
                    const T* cy, const T* trans, const T* lie, const T* world, const T* target, const uint8_t* vis,
                    T min_z, T pixel_ratio, T max_grad, T scale, const DavaL1SolveConfig* cfg, T* focal_o, T* cx_o,
                    T* cy_o, T* trans_o, T* lie_o, T* world_o, T* err_o, int32_t* iters_o, T* tr_err, T* tr_alpha,
                    int32_t* tr_exit, void* workspace, size_t workspace_bytes, void* stream) {
  if (batch < 0 || estimates < 0 || views < 1 || points < 4 || !cfg) return DAVA_ERR_INVALID_ARGUMENT;
  if (cfg->max_iterations < 0 || cfg->widen_iterations < 0 || cfg->zoom_iterations < 0)
    return DAVA_ERR_INVALID_ARGUMENT;
  if (batch == 0 || estimates == 0 || cfg->max_iterations == 0) return DAVA_OK;
  if (!focal || !cx || !cy || !trans || !lie || !world || !target || !vis || !focal_o || !cx_o || !cy_o || !trans_o ||
      !lie_o || !world_o || !err_o || !iters_o)
    return DAVA_ERR_INVALID_ARGUMENT;
  const int form = l1_solve_form<T>(views, points);
  if (form < 0 || batch * estimates > 0x7fffffff) return DAVA_ERR_UNSUPPORTED;
  const size_t need = l1_solve_workspace_bytes<T>(batch, estimates, views, points);
  if (need && (!workspace || workspace_bytes < need)) return DAVA_ERR_WORKSPACE;
  L1SolveArgs<T> a;
  a.m = l1_args(estimates, views, points, focal, cx, cy, trans, lie, world, target, vis, min_z, pixel_ratio, max_grad,
                scale);
  a.derived_ratio = (T)cfg->derived_inverse_pixel_ratio;
  a.K = cfg->max_iterations; a.W = cfg->widen_iterations; a.Z = cfg->zoom_iterations; a.constrain = cfg->constrain;
  a.eps = (T)cfg->epsilon; a.max_dist = (T)cfg->max_step_distance; a.min_dist = (T)cfg->min_step_distance;
  a.max_step = (T)cfg->max_step_size; a.c1 = (T)cfg->sufficient_decrease; a.c2 = (T)cfg->curvature;
  a.sscale = (T)cfg->slope_scale;
  a.focal_o = focal_o; a.cx_o = cx_o; a.cy_o = cy_o; a.trans_o = trans_o; a.lie_o = lie_o; a.world_o = world_o;
  a.err_o = err_o; a.iters_o = iters_o; a.tr_err = tr_err; a.tr_alpha = tr_alpha; a.tr_exit = tr_exit;
  a.hws = static_cast<T*>(workspace);
  const int lds = (int)l1_solve_lds_bytes<T>(views, points, form);
  const auto kernel = form == 0 ? l1_solve_kernel<T, 0> : l1_solve_kernel<T, 1>;
  launch_lds(kernel, (int)(batch * estimates), kBlock, lds, static_cast<hipStream_t>(stream), a);
  return launched();
}

}  // namespace dava

using namespace dava;

#define DAVA_L1_SOLVE_ENTRY(SUFFIX, T)                                                                              \
  extern "C" int dava_l1_camera_solve_##SUFFIX(                                                                    \
      int64_t batch, int32_t estimates, int32_t views, int32_t points, const T* focal, const T* cx, const T* cy,     \
      const T* translation, const T* lie_vector, const T* world_points, const T* true_points,                       \
      const uint8_t* visibility, T minimum_z_distance, T inverse_pixel_ratio, T max_gradient, T error_scale,        \
      const DavaL1SolveConfig* config, T* focal_out, T* cx_out, T* cy_out, T* translation_out, T* lie_vector_out,   \
      T* world_points_out, T* error_out, int32_t* iterations_out, T* trace_error, T* trace_alpha,                   \
      int32_t* trace_exit, void* workspace, size_t workspace_bytes, void* stream) {                                 \
    return l1_camera_solve<T>(batch, estimates, views, points, focal, cx, cy, translation, lie_vector, world_points, \
                              true_points, visibility, minimum_z_distance, inverse_pixel_ratio, max_gradient,       \
                              error_scale, config, focal_out, cx_out, cy_out, translation_out, lie_vector_out,      \
                              world_points_out, error_out, iterations_out, trace_error, trace_alpha, trace_exit,    \
                              workspace, workspace_bytes, stream);                                                  \
  }                                                                                                                 \
  extern "C" int dava_l1_camera_solve_form_##SUFFIX(int32_t views, int32_t points) {                               \
    return l1_solve_form<T>(views, points);                                                                         \
  }                                                                                                                 \
  extern "C" size_t dava_l1_camera_solve_workspace_bytes_##SUFFIX(int64_t batch, int32_t estimates, int32_t views,  \
                                                                  int32_t points) {                                 \
    return l1_solve_workspace_bytes<T>(batch, estimates, views, points);                                            \
  }

DAVA_L1_SOLVE_ENTRY(f32, float)
DAVA_L1_SOLVE_ENTRY(f64, double)
