// The float64 kernels (objective evaluation, the one-launch BFGS + strong-Wolfe solve) and their host side -- one
// plan and one launcher per operation, at the end of this file -- shared by bfgs_solve_f64.hip (which instantiates
// form 0: the whole image in LDS) and bfgs_solve_large_f64.hip (forms 1 and 2).
// The body is written once; FORM, a compile-time parameter, only says where its pointers come from:
//   form 0  x d g g_prev/y s H'y, the observations (as doubles) and visibility staged in LDS
//   form 1  the six vectors in LDS, observations and visibility read in place from HBM
//   form 2  observations and visibility in place, the six vectors in a per-problem workspace slice of 6 x Pv
//           doubles (the evaluation kernel: x and the direction in place, the gradient in grad_out's rows)
// In every form the view constants, the per-wave view partials, the two reduction buffers, rho_j, c_j and the
// per-entry product coefficients are in LDS.  One workgroup owns one problem (and its slice); __syncthreads()
// is the only synchronisation.
#pragma once

#include "ba_objective.hpp"
#include "dava_debug.hpp"
#include "dava_f64.hpp"
#include "dava_tape.hpp"

#include <type_traits>

namespace dava {
namespace f64 {

constexpr int kSolveVectors = 6;      // x d g g_prev/y s H'y
constexpr int kEvalVectors = 3;       // x d g

// The LDS image, offsets in doubles (vis: in bytes).  kcap = history capacity (0: evaluation image).
struct Carve {
  int x, d, g, gp, s, hy, views, vpart, scratch, coef, rho, c, obs, vis_bytes_off;
  long long total_bytes;
};

__host__ __device__ inline Carve carve(int M, int N, int Pv, int kcap) {
  Carve cv{};
  const bool solve = kcap > 0;
  const long long MN = (long long)M * N;
  const long long doubles = (long long)(solve ? kSolveVectors : kEvalVectors) * Pv + views_floats(M) +
                            (long long)vpart_floats(M) + 2 * kWaves * 32 + 6LL * kcap + 2 * MN;
  cv.total_bytes = doubles * 8 + round_up((int)(MN < (1 << 30) ? MN : (1 << 30)), 8);
  if (cv.total_bytes > kMaxLdsBytes) return cv;  // (offsets are meaningful only for an image that fits)
  int o = 0;
  cv.x = o; o += Pv;
  cv.d = o; o += Pv;
  cv.g = o; o += Pv;
  if (solve) {
    cv.gp = o; o += Pv;
    cv.s = o; o += Pv;
    cv.hy = o; o += Pv;
  }
  cv.views = o; o += views_floats(M);
  cv.vpart = o; o += vpart_floats(M);
  cv.scratch = o; o += 2 * kWaves * 32;
  cv.coef = o; o += 4 * kcap;
  cv.rho = o; o += kcap;
  cv.c = o; o += kcap;
  cv.obs = o; o += 2 * (int)MN;
  cv.vis_bytes_off = o * 8;
  return cv;
}

// The LDS image of forms 1 and 2: no scene, and in form 2 no vectors either (their offsets stay 0, unused).
__host__ __device__ inline Carve carve_large(int M, int Pv, int kcap, int form) {
  Carve cv{};
  const bool solve = kcap > 0;
  const long long vectors = form == 1 ? (long long)(solve ? kSolveVectors : kEvalVectors) * Pv : 0;
  const long long doubles = vectors + views_floats(M) + (long long)vpart_floats(M) + 2 * kWaves * 32 + 6LL * kcap;
  cv.total_bytes = doubles * 8;
  if (cv.total_bytes > kMaxLdsBytes) return cv;
  int o = 0;
  if (form == 1) {
    cv.x = o; o += Pv;
    cv.d = o; o += Pv;
    cv.g = o; o += Pv;
    if (solve) {
      cv.gp = o; o += Pv;
      cv.s = o; o += Pv;
      cv.hy = o; o += Pv;
    }
  }
  cv.views = o; o += views_floats(M);
  cv.vpart = o; o += vpart_floats(M);
  cv.scratch = o; o += 2 * kWaves * 32;
  cv.coef = o; o += 4 * kcap;
  cv.rho = o; o += kcap;
  cv.c = o; o += kcap;
  return cv;
}

// The form a scene takes: the lowest whose image fits 160 KiB, raised (never lowered) by the F64_FORM override;
// -1 where not even form 2's image fits (its view constants and history scalars: M > 251 at 1025 iterations).
// kcap = history capacity (0: the evaluation).
inline int choose_form(int M, int N, int Pv, int kcap) {
  int form = 2;
  if (carve(M, N, Pv, kcap).total_bytes <= kMaxLdsBytes) form = 0;
  else if (carve_large(M, Pv, kcap, 1).total_bytes <= kMaxLdsBytes) form = 1;
  const long long forced = debug_knob(kDbgF64Form);
  if ((forced == 1 || forced == 2) && forced > form) form = (int)forced;  // (an image that fits form 0 fits form 1)
  if (form == 2 && carve_large(M, Pv, kcap, 2).total_bytes > kMaxLdsBytes) return -1;
  return form;
}

struct SolveArgs {
  Layout L;
  int B, Pv, kcap;
  const double* obs;
  const uint8_t* vis;
  const double* x0;
  double* x_out;
  double* err_out;
  int32_t* status;
  double* hist;  // B x (S[kcap][Pv], W[kcap][Pv]), or null (iterations == 1)
  double c1, c2, thr, min_step;
  int iters, max_trials, strong;
  // RECORD: the tape's x, g and scalar blocks (B x K x Pv, B x K x Pv, B x T doubles); hist is its history block
  double* tape_x;
  double* tape_g;
  double* tape_sc;
  double* tape_tail;  // the tape's 256-byte tail (32 doubles)
  int T;
};

// What the TRAIN instantiations take (the eval-mode ones keep SolveArgs, their kernel argument as it was)
struct TrainArgs : SolveArgs {
  float drop_p;  // training-mode drop path probability (0: none)
  unsigned long long drop_seed;
  int second_last;  // training mode's return_second_last: a minimum-step stop keeps x_k
};

// What the form 1 and 2 instantiations take (the form-0 ones keep their kernel argument as it was)
struct LargeArgs : TrainArgs {
  double* vecs;  // form 2: B x (x, d, g, g_prev/y, s, H'y)[Pv], uninitialised
};

template <bool TRAIN, int FORM>
using solve_args_t = std::conditional_t<FORM != 0, LargeArgs, std::conditional_t<TRAIN, TrainArgs, SolveArgs>>;

template <bool GRAD, bool SLOPE, bool TRIAL, int RES>
__device__ __forceinline__ void eval(const Layout& L, const double* x, const double* d, double alpha,
                                     const double* obs, const uint8_t* vis, double* grad, double* views,
                                     double* vpart, double* scratch, int& buf, double& E, double& slope) {
  ba_eval<GRAD, SLOPE, TRIAL, false, false, RES, double, kWaves, 0, false>(L, x, d, alpha, obs, vis, grad, views, vpart,
                                                                         scratch, buf, E, slope);
}

// TRAIN: training mode's drop path and return_second_last, as bfgs_solve.hip runs them in float32.  Everything
// they add stands behind `if constexpr (TRAIN)` or folds away with `hold`: the eval-mode instantiations are the
// code they were without the flag.
// FORM (the header's list): where x, d, g, g_prev / y, s, H'y and the scene live.  It changes only the pointers the
// body below is given, so the compiler knows each one's address space; the arithmetic, the reduction trees and the
// pass order are one text for the three forms.  RECORD adds stores only and no LDS, so it exists in every form.
template <int RES, bool RECORD, bool TRAIN, int FORM = 0>
__global__ __launch_bounds__(kBlock, 1) void bfgs_ba_solve_f64_kernel(solve_args_t<TRAIN, FORM> a) {
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, Pv = a.Pv;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const size_t b = blockIdx.x;
  const Carve cv = FORM == 0 ? carve(M, N, Pv, a.kcap) : carve_large(M, Pv, a.kcap, FORM);
  double* vec = lds64;  // the six vectors: LDS, or (form 2) this problem's workspace slice, laid out alike
  if constexpr (FORM == 2) vec = a.vecs + b * kSolveVectors * Pv;
  double* x = vec + (FORM == 2 ? 0 : cv.x);
  double* d = vec + (FORM == 2 ? Pv : cv.d);
  double* g = vec + (FORM == 2 ? 2 * Pv : cv.g);
  double* gp = vec + (FORM == 2 ? 3 * Pv : cv.gp);  // previous gradient, then y = g - g_prev, then the trial gradients
  double* s = vec + (FORM == 2 ? 4 * Pv : cv.s);
  double* hy = vec + (FORM == 2 ? 5 * Pv : cv.hy);
  double* views = lds64 + cv.views;
  double* vpart = lds64 + cv.vpart;
  double* scratch = lds64 + cv.scratch;
  double* coef = lds64 + cv.coef;
  double* hrho = lds64 + cv.rho;
  double* hc = lds64 + cv.c;
  double* obl = lds64 + cv.obs;  // form 0: the scene's LDS copy
  uint8_t* vil = reinterpret_cast<uint8_t*>(lds64) + cv.vis_bytes_off;
  const int MN = M * N;

  // ---- stage the problem (form 0: into LDS; form 2's slice arrives uninitialised) and zero the vector pads ----
  const double* x0 = a.x0 + b * P;
  for (int i = tid; i < Pv; i += kBlock) {
    x[i] = i < P ? x0[i] : 0.0;
    d[i] = g[i] = gp[i] = s[i] = hy[i] = 0.0;
  }
  const double* obs = obl;
  const uint8_t* vis = vil;
  if constexpr (FORM == 0) {
    const double* ob = a.obs + b * 2 * MN;
    for (int i = tid; i < 2 * MN; i += kBlock) obl[i] = ob[i];
    const uint8_t* vb = a.vis + b * MN;
    for (int i = tid; i < MN; i += kBlock) vil[i] = vb[i] ? 1 : 0;
  } else {  // the scene where the caller put it
    obs = a.obs + b * 2 * MN;
    vis = a.vis + b * MN;
  }
  __syncthreads();

  double* SH = a.hist ? a.hist + b * 2 * a.kcap * Pv : nullptr;  // history rows S[kcap][Pv], W[kcap][Pv]
  double* WH = SH ? SH + (size_t)a.kcap * Pv : nullptr;
  int buf = 0;
  int steps = 0, reason = DAVA_STOP_ITERATIONS, evals = 0, trials = 0;
  double E = 0.0, unused = 0.0, gamma0 = 1.0;
  // When the line search accepts the step it evaluated last, that trial IS the evaluation at
  // x_{k+1} = x_k + alpha d (the same point, bit for bit): its objective and gradient are kept.
  bool have_next = false;
  double E_next = 0.0;

  // Training mode: the drop path stops this problem at the top of iteration kend (a.iters: never), drawn once
  // here with float32's generator and float comparison (drop_uniform, dava_common.hpp) and used as the loop's
  // bound, so the loop itself carries nothing extra; return_second_last holds x back until the step has passed
  // the minimum-step test.
  int kend = a.iters;
  bool hold = false;
  if constexpr (TRAIN) {
    if (a.drop_p > 0.f) {
      kend = 0;
      while (kend < a.iters && drop_uniform(a.drop_seed, (int)b, kend) > a.drop_p) ++kend;
    }
    hold = a.second_last != 0;
  }
  int k = 0;
  for (; k < kend; ++k) {
    { double* t = g; g = gp; gp = t; }  // gp <- previous gradient; g <- the (trial) gradient buffer
    if (have_next) {
      E = E_next;
    } else {
      eval<true, false, false, RES>(L, x, nullptr, 0.0, obs, vis, g, views, vpart, scratch, buf, E, unused);
      ++evals;
    }
    if (!(E > a.thr)) { reason = DAVA_STOP_ERROR; break; }
    if constexpr (RECORD) {  // x_k and g_k = dE/dx(x_k) (the pads of both vectors are zero)
      double* xr = a.tape_x + (b * a.iters + k) * Pv;
      double* gr = a.tape_g + (b * a.iters + k) * Pv;
      for (int i = tid; i < Pv; i += kBlock) { xr[i] = x[i]; gr[i] = g[i]; }
    }

    // phi'(0) = d . g is accumulated where d is formed; its block reduction also publishes d
    double dg = 0.0;
    if (k == 0) {
      // first step: no inverse Hessian yet, d = -g (bfgs_solver.py:152-155)
      for (int i = tid; i < P; i += kBlock) {
        const double di = -1.0 * g[i];
        d[i] = di;
        dg += di * g[i];
      }
    } else {
      // compact_direction_kernel<double>'s update + direction (bfgs_ops.hip), entry `count` appended
      const int count = k - 1;
      for (int i = tid; i < P; i += kBlock) gp[i] = g[i] - gp[i];  // y
      __syncthreads();
      // pass 1: per entry the four dots (s_j.y, s_j.g, w_j.y, w_j.g) -> coefficients, entries dealt to waves
      for (int j = wave; j < count; j += kWaves) {
        const double* sj = SH + (size_t)j * Pv;
        const double* wj = WH + (size_t)j * Pv;
        double sy = 0, sg = 0, wy = 0, wg = 0;
        for (int i = lane; i < P; i += kWave) {
          const double aj = sj[i], w = wj[i], yi = gp[i], gi = g[i];
          sy += aj * yi; sg += aj * gi; wy += w * yi; wg += w * gi;
        }
        sy = wave_sum(sy); sg = wave_sum(sg); wy = wave_sum(wy); wg = wave_sum(wg);
        if (lane == 0) {
          const double rj = hrho[j], cj = hc[j];
          coef[4 * j + 0] = cj * rj * sy - rj * wy;
          coef[4 * j + 1] = -rj * sy;
          coef[4 * j + 2] = cj * rj * sg - rj * wg;
          coef[4 * j + 3] = -rj * sg;
        }
      }
      double gm;
      if (count == 0) {  // H_0 = gamma I, N&W eq. 6.20 (bfgs_solver.py:159-167, 217-233)
        double r[2] = {0.0, 0.0};
        for (int i = tid; i < P; i += kBlock) { r[0] += s[i] * gp[i]; r[1] += gp[i] * gp[i]; }
        block_sum<2>(r, scratch, buf); buf ^= 1;
        gm = clamp_min(r[0] / clamp_min(r[1], 1e-5), 1e-4);
        gamma0 = gm;
      } else {
        __syncthreads();  // coefficients complete
        gm = gamma0;
      }
      // pass 2: H'y and H'g column by column; H'y is the new entry's w row, H'g is parked in d
      double* wn = WH + (size_t)count * Pv;
      double* sn = SH + (size_t)count * Pv;
      double r[4] = {0.0, 0.0, 0.0, 0.0};
      for (int i = tid; i < P; i += kBlock) {
        const double yi = gp[i], gi = g[i], si = s[i];
        double hyi = gm * yi, hgi = gm * gi;
        int j = 0;
        for (; j + 4 <= count; j += 4) {  // four entries' loads in flight
          double aj[4], w[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) { aj[u] = SH[(size_t)(j + u) * Pv + i]; w[u] = WH[(size_t)(j + u) * Pv + i]; }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const double* cf = coef + 4 * (j + u);
            hyi += cf[0] * aj[u] + cf[1] * w[u];
            hgi += cf[2] * aj[u] + cf[3] * w[u];
          }
        }
        for (; j < count; ++j) {
          const double aj = SH[(size_t)j * Pv + i], w = WH[(size_t)j * Pv + i];
          const double* cf = coef + 4 * j;
          hyi += cf[0] * aj + cf[1] * w;
          hgi += cf[2] * aj + cf[3] * w;
        }
        wn[i] = hyi;
        sn[i] = si;
        hy[i] = hyi;
        d[i] = hgi;
        r[0] += si * yi; r[1] += hyi * yi; r[2] += si * gi; r[3] += hyi * gi;
      }
      for (int i = P + tid; i < Pv; i += kBlock) { wn[i] = 0.0; sn[i] = 0.0; }
      block_sum<4>(r, scratch, buf); buf ^= 1;
      const double rh = r[0] <= 0.0 ? 0.0 : 1.0 / r[0];  // inverse_curvature (func_inverse_curvature.py:24-28)
      const double c = 1.0 + rh * r[1];
      const double sg = r[2], hyg = r[3], rsg = rh * sg;
      // d = -H_k g,  H_k = H' + c (rho s) s^T - (rho s) (H'y)^T - (H'y) (rho s)^T
      for (int i = tid; i < P; i += kBlock) {  // (each thread reads back what it wrote)
        const double sri = s[i] * rh;
        const double di = -1.0 * (d[i] + sri * (c * sg) - sri * hyg - hy[i] * rsg);
        d[i] = di;
        dg += di * g[i];
      }
      if (tid == 0) {
        hrho[count] = rh;
        hc[count] = c;
      }
    }

    // ---- strong-Wolfe line search (wolfe_conditions.py:23-239) ----
    double dphi0;
    {
      double r[1] = {dg};
      block_sum<1>(r, scratch, buf); buf ^= 1;
      dphi0 = r[0];
    }
    double a_lo = 0.0, a_hi = 0.0, al = 1.0, f_lo = E, f_hi = E, fa = E, dfa = dphi0;
    double last_al = 0.0, last_fa = 0.0;
    bool widen = true, zoom = false, evaluated = false;
    const double lim = (-1.0 * a.c2) * dphi0;
    for (int t = 0; t < a.max_trials; ++t) {
      if (!(widen || zoom)) break;
      if (t > 0) {
        if (widen) { a_hi = al; f_hi = fa; al = 2.0 * al; }
        if (zoom) al = 0.5 * (a_lo + a_hi);
      }
      // E, phi'(alpha) (forward mode) and the gradient (reverse mode, into g_prev's buffer: y is dead once d
      // is formed) at x + alpha d
      eval<true, true, true, RES>(L, x, d, al, obs, vis, gp, views, vpart, scratch, buf, fa, dfa);
      ++evals;
      // Overflowed trial: the reference's phi'(alpha) is autograd w.r.t. alpha, (grad E(x + alpha d) * d).sum()
      // -- NaN as soon as the gradient holds a NaN or infinities of both signs, where the forward-mode tangent
      // may come out as +-Inf, and the NaN-blind Wolfe comparisons branch on that class (bfgs_solve.hip).
      // Uniform branch (fa, dfa are block-reduced); eval<GRAD> ends with a barrier.
      if (!(isfinite(fa) && isfinite(dfa))) {
        double r[1] = {0.0};
        for (int i = tid; i < P; i += kBlock) r[0] += gp[i] * d[i];
        block_sum<1>(r, scratch, buf); buf ^= 1;
        dfa = r[0];
      }
      ++trials;
      evaluated = true;
      last_al = al;
      last_fa = fa;
      bool fail = fa > E + (a.c1 * al) * dphi0;
      if (zoom) fail = fail || (fa >= f_lo);
      if (t > 0 && widen) fail = fail || (fa >= f_hi);
      const bool curv = a.strong ? (fabs(dfa) <= lim) : (-1.0 * dfa <= lim);
      const bool up = widen ? (dfa >= 0.0) : (dfa * (a_hi - a_lo) >= 0.0);
      if (zoom) {
        const bool done = !fail && curv;
        const bool flip = !fail && !curv && up;
        const bool setlo = !fail && !curv;
        if (fail || done) { a_hi = al; f_hi = fa; }
        if (flip) { a_hi = a_lo; f_hi = f_lo; }
        if (setlo || done) { a_lo = al; f_lo = fa; }
        if (done) zoom = false;
      } else if (widen) {
        const bool bracket = fail;
        const bool done = !fail && curv;
        const bool flip = !fail && !curv && up;
        if (bracket) { a_lo = a_hi; f_lo = f_hi; }
        if (bracket || done) { a_hi = al; f_hi = fa; }
        if (done || flip) { a_lo = al; f_lo = fa; }
        if (bracket || flip) zoom = true;
        if (bracket || done || flip) widen = false;
      }
      if (a_lo == a_hi) zoom = false;
    }
    const double alpha = a_hi;
    if constexpr (RECORD) {
      if (tid == 0) a.tape_sc[b * a.T + k] = alpha;
    }
    have_next = evaluated && last_al == alpha;
    E_next = last_fa;

    // ---- take the step (bfgs_solver.py:191-199) and test its length (:203-207) ----
    {
      double r[1] = {0.0};
      if (hold) {  // x moves only once the step has passed the test (uniform branch; never in eval mode)
        for (int i = tid; i < P; i += kBlock) {
          const double si = fmul_rn(alpha, d[i]);
          s[i] = si;
          r[0] += si * si;
        }
      } else {
        for (int i = tid; i < P; i += kBlock) {
          const double si = fmul_rn(alpha, d[i]);
          s[i] = si;
          x[i] = fadd_rn(x[i], si);
          r[0] += si * si;
        }
      }
      block_sum<1>(r, scratch, buf); buf ^= 1;
      ++steps;  // (the failed step counts: the status words equal the eval solve's)
      if (!(sqrt(r[0]) > a.min_step)) { reason = DAVA_STOP_STEP; break; }
      if (hold) {  // the same additions, after the test (bfgs_solver.py:208-212)
        for (int i = tid; i < P; i += kBlock) x[i] = fadd_rn(x[i], s[i]);
        __syncthreads();
      }
    }
  }
  if constexpr (TRAIN) {
    if (k == kend && kend < a.iters) reason = DAVA_STOP_DROP;  // uniform
  }

  // ---- outputs ----
  __syncthreads();
  double* xo = a.x_out + b * P;
  for (int i = tid; i < P; i += kBlock) xo[i] = x[i];
  if (a.err_out) {
    double e2 = 0.0;
    eval<false, false, false, RES>(L, x, nullptr, 0.0, obs, vis, nullptr, views, vpart, scratch, buf, e2, unused);
    if (tid == 0) a.err_out[b] = e2;
  }
  if (a.status && tid == 0) {
    int32_t* st = a.status + b * DAVA_STATUS_WORDS;
    st[0] = steps; st[1] = reason; st[2] = evals; st[3] = trials;
  }
  if constexpr (RECORD) {
    // The scalar row [alpha_0.. | rho_0.. | c_0.. | gamma]: alpha_k, k < steps, is in place (thread 0, above);
    // rho_j, c_j of the steps - 1 entries made come from LDS.  Every slot the solve did not reach -- of the
    // scalar row, the x / g rows and the history rows -- is zeroed: a tape is a function of its solve alone.
    const int K = a.iters, made = steps > 1 ? steps - 1 : 0;
    double* sc = a.tape_sc + b * a.T;
    for (int i = steps + tid; i < a.T; i += kBlock) {
      double v = 0.0;
      if (i >= K && i < 2 * K) v = i - K < made ? hrho[i - K] : 0.0;
      else if (i >= 2 * K && i < 3 * K) v = i - 2 * K < made ? hc[i - 2 * K] : 0.0;
      else if (i == 3 * K) v = gamma0;
      sc[i] = v;  // (i < K here: an alpha slot past the last step)
    }
    for (int k = steps; k < K; ++k) {
      double* xr = a.tape_x + (b * K + k) * Pv;
      double* gr = a.tape_g + (b * K + k) * Pv;
      for (int i = tid; i < Pv; i += kBlock) { xr[i] = 0.0; gr[i] = 0.0; }
    }
    for (int j = made; j < a.kcap; ++j)
      for (int i = tid; i < Pv; i += kBlock) { SH[(size_t)j * Pv + i] = 0.0; WH[(size_t)j * Pv + i] = 0.0; }
    if (b == 0 && tid < (int)(kTailBytes / sizeof(double))) a.tape_tail[tid] = 0.0;
  }
}

// ---- single evaluation kernel (dava_ba_evaluate_f64) ----
struct EvalArgs {
  Layout L;
  int Pv;
  const double* obs;
  const uint8_t* vis;
  const double* x;
  const double* dir;
  const double* alpha;
  double* err;
  double* grad;
  double* slope;
};

// One workgroup per problem; x, d, the gradient, the observations and the view constants in LDS, as the
// LDS-mode ba_evaluate_kernel (bfgs_solve.hip) and as the solve above evaluates its trials.
// FORM 1 reads the scene in place; FORM 2 also reads x and the direction in place (rows of P doubles: the
// objective indexes no pad) and forms the gradient in grad_out's rows, so it needs no workspace.
template <bool GRAD, bool SLOPE, bool TRIAL, int RES, int FORM = 0>
__global__ __launch_bounds__(kBlock, 1) void ba_evaluate_f64_kernel(EvalArgs a) {
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, Pv = a.Pv;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const Carve cv = FORM == 0 ? carve(M, N, Pv, 0) : carve_large(M, Pv, 0, FORM);
  const int MN = M * N;
  double* xl = lds64 + cv.x;
  double* dl = lds64 + cv.d;
  double* gl = lds64 + cv.g;
  double* obl = lds64 + cv.obs;
  uint8_t* vil = reinterpret_cast<uint8_t*>(lds64) + cv.vis_bytes_off;
  const double* x = xl;
  const double* d = dl;
  double* g = gl;
  const double* obs = obl;
  const uint8_t* vis = vil;
  if constexpr (FORM != 2) {
    for (int i = tid; i < Pv; i += kBlock) {
      xl[i] = i < P ? a.x[b * P + i] : 0.0;
      dl[i] = (a.dir && i < P) ? a.dir[b * P + i] : 0.0;
      gl[i] = 0.0;
    }
  } else {
    x = a.x + b * P;
    d = a.dir ? a.dir + b * P : nullptr;
    g = GRAD ? a.grad + b * P : nullptr;
    if constexpr (GRAD)  // (the objective writes every entry before it reads it; the rows arrive uninitialised)
      for (int i = tid; i < P; i += kBlock) g[i] = 0.0;
  }
  if constexpr (FORM == 0) {
    for (int i = tid; i < 2 * MN; i += kBlock) obl[i] = a.obs[b * 2 * MN + i];
    for (int i = tid; i < MN; i += kBlock) vil[i] = a.vis[b * MN + i] ? 1 : 0;
  } else {
    obs = a.obs + b * 2 * MN;
    vis = a.vis + b * MN;
  }
  __syncthreads();
  const double al = (TRIAL && a.alpha) ? a.alpha[b] : 0.0;
  int buf = 0;
  double E = 0.0, sl = 0.0;
  eval<GRAD, SLOPE, TRIAL, RES>(L, x, d, al, obs, vis, g, lds64 + cv.views, lds64 + cv.vpart, lds64 + cv.scratch, buf,
                                E, sl);
  if (tid == 0) {
    a.err[b] = E;
    if (SLOPE && a.slope) a.slope[b] = sl;
  }
  if (FORM != 2 && GRAD && a.grad)
    for (int i = tid; i < P; i += kBlock) a.grad[b * P + i] = g[i];
}

// ---- host side: the solve (plain, recording, training) ----

// What a scene and a config need, from the shapes alone: the size and form queries and the launch's checks read
// the same numbers.
struct SolveShape {
  int status;  // DAVA_OK: `form` runs this scene / config
  int form, Pv, kcap, lds;
  size_t history_bytes;  // B x (S[kcap][Pv], W[kcap][Pv])
  size_t vector_bytes;   // form 2: B x 6 x Pv doubles, else 0
  TapeLayout tape;       // dava_tape.hpp in doubles: the layout of every form
  // the plain solve: [history | form 2: vectors | tail]
  size_t workspace_bytes() const { return history_bytes + vector_bytes + kTailBytes; }
  // the recording solve, whose history is the tape's first block: [form 2: vectors | tail], else nothing
  size_t record_workspace_bytes() const { return form == 2 ? vector_bytes + kTailBytes : 0; }
};

inline SolveShape solve_shape(const DavaScene& sc, const DavaSolverConfigF64* c, bool any_form) {
  SolveShape s{};
  s.form = -1;
  s.status = DAVA_ERR_INVALID_ARGUMENT;
  if (!c || c->iterations < 0 || c->max_line_search_trials < 0) return s;
  s.status = DAVA_ERR_UNSUPPORTED;
  if (c->iterations < 1 || c->iterations > kMaxIterations) return s;
  const int M = sc.num_views, N = sc.num_points;
  s.Pv = round_up(sc.num_parameters, 4);
  s.kcap = history_capacity(c->iterations);
  // (form 2's own image -- view constants, view partials, history scalars -- grows with the views: more than
  //  251 of them at 1025 iterations do not fit)
  s.form = any_form ? choose_form(M, N, s.Pv, s.kcap) : carve(M, N, s.Pv, s.kcap).total_bytes <= kMaxLdsBytes ? 0 : -1;
  if (s.form < 0) return s;
  s.status = DAVA_OK;
  s.lds = (int)(s.form == 0 ? carve(M, N, s.Pv, s.kcap) : carve_large(M, s.Pv, s.kcap, s.form)).total_bytes;
  s.history_bytes = (size_t)sc.batch * 2 * s.kcap * s.Pv * sizeof(double);
  s.vector_bytes = s.form == 2 ? (size_t)sc.batch * kSolveVectors * s.Pv * sizeof(double) : 0;
  s.tape = tape_layout_f64(sc.batch, sc.num_parameters, c->iterations);
  return s;
}

// the shape behind a host-only query (which looks at no data pointer)
inline SolveShape solve_query(const DavaSceneF64* scene, const DavaSolverConfigF64* c, bool any_form) {
  DavaScene sc;
  SolveShape s{};
  s.form = -1;
  s.status = check_scene_f64(scene, false, sc);
  return s.status == DAVA_OK ? solve_shape(sc, c, any_form) : s;
}

struct SolvePlan {
  int status;
  bool launch;  // false: return `status` (a refusal, or DAVA_OK for an empty batch)
  bool ray, train, record;
  SolveShape shape;
  LargeArgs args;  // the form-0 kernels take its base, TrainArgs or SolveArgs
};

// The checks of every solve entry point, in their order.  `tape` (record): the tape, whose first block is the
// history rows; `workspace`: the history rows and form 2's vectors, or (record) form 2's vectors alone.
// training: null or all zero = eval mode, the instantiations without TRAIN.
inline SolvePlan plan_solve(const DavaSceneF64* scene, const DavaSolverConfigF64* config,
                            const DavaTrainingF64* training, const double* x0, double* x_out, double* error_out,
                            int32_t* status_out, void* tape, size_t tape_bytes, void* workspace,
                            size_t workspace_bytes, bool record, bool any_form) {
  SolvePlan p{};
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  if (training && !(training->drop_path_p >= 0.f && training->drop_path_p <= 1.f))
    return refuse(DAVA_ERR_INVALID_ARGUMENT);
  p.train = training && (training->drop_path_p > 0.f || training->return_second_last);
  p.record = record;
  DavaScene sc;
  const int st = check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return refuse(st);
  const SolveShape& s = p.shape = solve_shape(sc, config, any_form);
  if (s.status == DAVA_ERR_INVALID_ARGUMENT) return refuse(s.status);
  if (sc.batch == 0) return refuse(DAVA_OK);
  if (!x0 || !x_out) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  if (s.status != DAVA_OK) return refuse(s.status);
  const int iters = config->iterations;
  if (record) {
    if (!status_out) return refuse(DAVA_ERR_INVALID_ARGUMENT);
    if (!tape || tape_bytes < s.tape.total_bytes) return refuse(DAVA_ERR_WORKSPACE);
    if (s.form == 2 && (!workspace || workspace_bytes < s.record_workspace_bytes())) return refuse(DAVA_ERR_WORKSPACE);
  } else if ((s.form == 2 || iters > 1) && (!workspace || workspace_bytes < s.workspace_bytes())) {
    // (the size the query reports, tail included: a queue counter put there later finds its bytes)
    return refuse(DAVA_ERR_WORKSPACE);
  }
  p.ray = sc.residual == DAVA_RESIDUAL_RAY_ANGLE;
  double* tp = static_cast<double*>(tape);
  LargeArgs& a = p.args;
  a.L = make_layout(&sc);
  a.B = sc.batch;
  a.Pv = s.Pv;
  a.kcap = s.kcap;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.x0 = x0;
  a.x_out = x_out;
  a.err_out = error_out;
  a.status = status_out;
  a.hist = record ? tp : iters > 1 ? static_cast<double*>(workspace) : nullptr;
  a.c1 = config->sufficient_decrease;
  a.c2 = config->curvature;
  a.thr = config->error_threshold;
  a.min_step = config->minimum_step;
  a.iters = iters;
  a.max_trials = config->max_line_search_trials;
  a.strong = config->strong_wolfe;
  a.tape_x = record ? tp + s.tape.x : nullptr;
  a.tape_g = record ? tp + s.tape.g : nullptr;
  a.tape_sc = record ? tp + s.tape.scal : nullptr;
  a.tape_tail = record ? tp + s.tape.vecs : nullptr;
  a.T = s.tape.T;
  a.drop_p = p.train ? training->drop_path_p : 0.f;
  a.drop_seed = p.train ? ((unsigned long long)training->drop_seed_hi << 32) | training->drop_seed_lo : 0ull;
  a.second_last = p.train && training->return_second_last ? 1 : 0;
  a.vecs = s.form != 2 ? nullptr
           : record    ? static_cast<double*>(workspace)
                       : reinterpret_cast<double*>(static_cast<char*>(workspace) + s.history_bytes);
  p.launch = true;
  return p;
}

// RES x RECORD x TRAIN of one form
template <int FORM>
int launch_solve(const SolvePlan& p, void* stream) {
  with_flag(p.ray, [&](auto ray) {
    with_flag(p.record, [&](auto record) {
      with_flag(p.train, [&](auto train) {
        constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
        constexpr bool kRecord = decltype(record)::value, kTrain = decltype(train)::value;
        const auto kernel = bfgs_ba_solve_f64_kernel<kRes, kRecord, kTrain, FORM>;
        const solve_args_t<kTrain, FORM>& a = p.args;  // (form 0: the base the kernel takes)
        set_dynamic_lds(kernel, p.shape.lds);
        hipLaunchKernelGGL(kernel, dim3(p.args.B), dim3(kBlock), p.shape.lds, static_cast<hipStream_t>(stream), a);
      });
    });
  });
  return launched();
}

// A plan's outcome where it asks for no launch, else the form-0 launch: instantiated in bfgs_solve_f64.hip, and
// reached from bfgs_solve_large_f64.hip for a scene whose whole image fits LDS.
int solve_form0(const SolvePlan& p, void* stream);

// ---- host side: the evaluation ----
struct EvalPlan {
  int status;
  bool launch;
  int form, lds, batch, residual;
  EvalArgs args;
};

inline EvalPlan plan_eval(const DavaSceneF64* scene, const double* x, const double* direction, const double* alpha,
                          double* error_out, double* grad_out, double* slope_out, bool any_form) {
  EvalPlan p{};
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  DavaScene sc;
  const int st = check_scene_f64(scene, true, sc);
  if (st != DAVA_OK) return refuse(st);
  if (sc.batch == 0) return refuse(DAVA_OK);
  if (!x || !error_out) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  if (slope_out && !direction) return refuse(DAVA_ERR_INVALID_ARGUMENT);
  const int M = sc.num_views, N = sc.num_points, Pv = round_up(sc.num_parameters, 4);
  // (any form: more than 361 views do not fit -- form 2's view constants and partials alone)
  p.form = any_form ? choose_form(M, N, Pv, 0) : carve(M, N, Pv, 0).total_bytes <= kMaxLdsBytes ? 0 : -1;
  if (p.form < 0) return refuse(DAVA_ERR_UNSUPPORTED);
  p.lds = (int)(p.form == 0 ? carve(M, N, Pv, 0) : carve_large(M, Pv, 0, p.form)).total_bytes;
  p.batch = sc.batch;
  p.residual = sc.residual;
  EvalArgs& a = p.args;
  a.L = make_layout(&sc);
  a.Pv = Pv;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.x = x;
  a.dir = direction;
  a.alpha = alpha;
  a.err = error_out;
  a.grad = grad_out;
  a.slope = slope_out;
  p.launch = true;
  return p;
}

// the instantiation for the residual and the outputs asked for (gradient, slope, trial point x + alpha d)
template <int FORM>
int launch_eval(const EvalPlan& p, void* stream) {
  const EvalArgs& a = p.args;
  with_flag(p.residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
    with_flag(a.grad != nullptr, [&](auto grad) {
      with_flag(a.slope != nullptr, [&](auto slope) {
        with_flag(a.dir != nullptr && a.alpha != nullptr, [&](auto trial) {
          constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
          const auto kernel = ba_evaluate_f64_kernel<decltype(grad)::value, decltype(slope)::value,
                                                     decltype(trial)::value, kRes, FORM>;
          set_dynamic_lds(kernel, p.lds);
          hipLaunchKernelGGL(kernel, dim3(p.batch), dim3(kBlock), p.lds, static_cast<hipStream_t>(stream), a);
        });
      });
    });
  });
  return launched();
}

// as solve_form0
int eval_form0(const EvalPlan& p, void* stream);

}  // namespace f64
}  // namespace dava
