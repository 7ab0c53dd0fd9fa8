// Reverse mode of the float64 fused solve: d x_out / d (x0, observations) applied to a cotangent, replaying the
// float64 tape (dava_ba_solve_record_f64, dava_tape.hpp in doubles) backwards.  The kernel, its plan (every host
// check, once for all forms) and its launcher, shared by bfgs_adjoint_f64.hip (which instantiates form 0:
// dava_ba_solve_backward_f64) and bfgs_adjoint_large_f64.hip (forms 1 and 2: dava_ba_solve_backward_large_f64).
// As in solve_f64.hpp the body is written once and FORM, a compile-time
// parameter, only says where its pointers come from:
//   form 0  the 14 Pv vectors, the observations and visibility, and (obs_lds) the observation cotangent in LDS
//   form 1  the 14 Pv vectors in LDS; the scene read in place; the observation cotangent accumulated in
//           observations_grad (zeroed here; not formed when null)
//   form 2  as form 1, the 14 Pv vectors in a per-problem workspace slice laid out as the LDS image lays them out
// In every form the dual view constants, the dual per-wave view partials, the reduction scratch and the chunk
// coefficients are in LDS.
//
// The mathematics is bfgs_adjoint.hip's (its header comment: the adjoint of the inverse Hessian kept as rows
// a_j, the gamma adjoint through both clamps at k = 1, the rho > 0 guard of the inverse-curvature backward,
// k = 0), in the deliberately small first form bfgs_solve_f64.hip set:
//  * one 256-thread workgroup per problem, every O(P) vector in LDS as doubles; thread t owns elements
//    t, t + 256, ... of every vector in every elementwise loop;
//  * the two passes of a step -- over the tape rows (a_j, g_j), j = k .. n-1, and over the history rows
//    (s_j, w_j), j = 0 .. k-2 -- are plain loops: per chunk of kChunk rows the four dots of every row (rows
//    dealt to the waves, xor-butterfly wave sums) go to LDS, then every thread adds the chunk's rows to its own
//    elements in row order.  No on-chip history entries, no global-vector mode, no staged copies;
//  * the tape's scalar row (alpha_k, rho_j, c_j, gamma) is read in place;
//  * the Hessian-vector step is ba_eval<..., DualT<double>> with obs_tangent_acc; the vectors that live only
//    between the top of a step and that evaluation (s, w, y, g_k) sit in the dual vectors' space;
//  * the observation cotangent accumulates in LDS, or -- where that does not fit -- in the output;
//  * every loop bounded by the problem's recorded step count; no queue, no spin-wait; every sum in a fixed
//    order (block_sum(double), wave_sum), so two launches give bitwise the same gradients.
#pragma once

#include "ba_objective.hpp"
#include "dava_debug.hpp"
#include "dava_f64.hpp"
#include "dava_tape.hpp"

#include <type_traits>

namespace dava {
namespace f64 {

constexpr int kChunk = 32;      // rows per round of a pass (8 per wave)
constexpr int kAdjVectors = 10;  // xb sbp gbp an db gk p1 p2 wb ak; s w y g_k share the dual vectors' 4 Pv

struct AdjointArgs {
  Layout L;
  int Pv, K;
  TapeLayout tl;
  const double* tape;
  const double* obs;
  const uint8_t* vis;
  const int32_t* status;
  const double* xbar;  // (B, P) cotangent of x_out
  double* x0_grad;     // (B, P)
  double* obs_grad;    // (B, M, N, 2) or null
  double* arows;       // (B, K, Pv) workspace
  int obs_lds;         // the observation cotangent accumulates in LDS (else in obs_grad)
};

// What the form 1 and 2 instantiations take (the form-0 one keeps its kernel argument as it was)
struct LargeAdjointArgs : AdjointArgs {
  double* vecs;  // form 2: B x 14 x Pv doubles, uninitialised
};

template <int FORM>
using adjoint_args_t = std::conditional_t<FORM != 0, LargeAdjointArgs, AdjointArgs>;

struct AdjointCarve {
  int xb, sbp, gbp, an, db, gk, p1, p2, wb, ak, xd, gd, views, vpart, scratch, coef, obs, obsacc, vis_bytes_off;
  long long total_bytes;  // offsets in doubles
};

__host__ __device__ inline AdjointCarve carve_adjoint(int M, int N, int Pv, bool obs_lds) {
  AdjointCarve c{};
  const long long MN = (long long)M * N;
  const long long doubles = (long long)(kAdjVectors + 4) * Pv + 2LL * views_floats(M) + 2LL * vpart_floats(M) +
                            2 * kWaves * 32 + 4 * kChunk + 2 * MN + (obs_lds ? 2 * MN : 0);
  c.total_bytes = doubles * 8 + round_up((int)(MN < (1 << 30) ? MN : (1 << 30)), 16);
  if (c.total_bytes > kMaxLdsBytes) return c;  // (offsets are meaningful only for an image that fits)
  int o = 0;
  int* vec[] = {&c.xb, &c.sbp, &c.gbp, &c.an, &c.db, &c.gk, &c.p1, &c.p2, &c.wb, &c.ak};
  for (int* v : vec) { *v = o; o += Pv; }
  c.xd = o; o += 2 * Pv;  // Dual64
  c.gd = o; o += 2 * Pv;  // Dual64
  c.views = o; o += 2 * views_floats(M);
  c.vpart = o; o += 2 * vpart_floats(M);
  c.scratch = o; o += 2 * kWaves * 32;
  c.coef = o; o += 4 * kChunk;
  c.obs = o; o += 2 * (int)MN;
  c.obsacc = o; o += obs_lds ? 2 * (int)MN : 0;
  c.vis_bytes_off = o * 8;
  return c;
}

// The LDS image of forms 1 and 2: no scene, no observation cotangent and in form 2 no vectors either.  The vector
// offsets are relative to the vectors' base (LDS, or the problem's slice), the others to the LDS base.
__host__ __device__ inline AdjointCarve carve_adjoint_large(int M, int Pv, int form) {
  AdjointCarve c{};
  const long long vectors = (long long)(kAdjVectors + 4) * Pv;
  const long long doubles = (form == 1 ? vectors : 0) + 2LL * views_floats(M) + 2LL * vpart_floats(M) +
                            2 * kWaves * 32 + 4 * kChunk;
  c.total_bytes = doubles * 8;
  if (c.total_bytes > kMaxLdsBytes) return c;
  int o = 0;
  int* vec[] = {&c.xb, &c.sbp, &c.gbp, &c.an, &c.db, &c.gk, &c.p1, &c.p2, &c.wb, &c.ak};
  for (int* v : vec) { *v = o; o += Pv; }
  c.xd = o; o += 2 * Pv;
  c.gd = o; o += 2 * Pv;
  if (form != 1) o = 0;  // (form 2: the LDS image starts at the view constants)
  c.views = o; o += 2 * views_floats(M);
  c.vpart = o; o += 2 * vpart_floats(M);
  c.scratch = o; o += 2 * kWaves * 32;
  c.coef = o; o += 4 * kChunk;
  return c;
}

// out1 = base v1 + sum_j (k1 R1_j + k2 R2_j), out2 = base v2 + sum_j (k3 R1_j + k4 R2_j) over rows j0 .. j1-1
// (R1_j = R1 + j Pv, R2_j = R2 + j Pv in HBM), (k1..k4) = coef(j, R1_j.v1, R2_j.v1, R1_j.v2, R2_j.v2).
// v1, v2, out1, out2: the kernel's vectors (LDS, or form 2's slice), out not aliasing v.  Rows are added in row order; ends with a barrier.
template <class Coef>
__device__ __forceinline__ void pair_pass(int P, int Pv, int j0, int j1, const double* R1,
                                          const double* R2, const double* v1, const double* v2,
                                          double base, Coef coef, double* out1, double* out2, double* cf) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  for (int i = tid; i < Pv; i += kBlock) { out1[i] = 0.0; out2[i] = 0.0; }
  for (int jc = j0; jc < j1; jc += kChunk) {
    const int je = min(jc + kChunk, j1);
    for (int j = jc + wave; j < je; j += kWaves) {
      const double* r1 = R1 + (size_t)j * Pv;
      const double* r2 = R2 + (size_t)j * Pv;
      double d11 = 0.0, d21 = 0.0, d12 = 0.0, d22 = 0.0;
      for (int i = lane; i < P; i += kWave) {
        const double a = r1[i], g = r2[i], s = v1[i], w = v2[i];
        d11 += a * s; d21 += g * s; d12 += a * w; d22 += g * w;
      }
      d11 = wave_sum(d11); d21 = wave_sum(d21); d12 = wave_sum(d12); d22 = wave_sum(d22);
      if (lane == 0) {
        double k1, k2, k3, k4;
        coef(j, d11, d21, d12, d22, k1, k2, k3, k4);
        double* c = cf + 4 * (j - jc);
        c[0] = k1; c[1] = k2; c[2] = k3; c[3] = k4;
      }
    }
    __syncthreads();  // the chunk's coefficients complete
    for (int i = tid; i < P; i += kBlock) {
      double s1 = out1[i], s2 = out2[i];
      for (int j = jc; j < je; ++j) {
        const double a = R1[(size_t)j * Pv + i], g = R2[(size_t)j * Pv + i];
        const double* c = cf + 4 * (j - jc);
        s1 += c[0] * a + c[1] * g;
        s2 += c[2] * a + c[3] * g;
      }
      out1[i] = s1;
      out2[i] = s2;
    }
    __syncthreads();  // coefficients consumed before the next chunk overwrites them
  }
  for (int i = tid; i < P; i += kBlock) {
    out1[i] += base * v1[i];
    out2[i] += base * v2[i];
  }
  __syncthreads();
}

// FORM (the header's list) changes only the pointers the body below is given, so the compiler knows each one's
// address space; the arithmetic, the reduction trees and the pass order are one text for the three forms.
template <int RES, int FORM = 0>
__global__ __launch_bounds__(kBlock, 1) void bfgs_ba_adjoint_f64_kernel(adjoint_args_t<FORM> a) {
  extern __shared__ __attribute__((aligned(16))) double lds64[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, MN = M * N, Pv = a.Pv, K = a.K;
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const TapeLayout& tl = a.tl;
  const AdjointCarve cv = FORM == 0 ? carve_adjoint(M, N, Pv, a.obs_lds != 0) : carve_adjoint_large(M, Pv, FORM);
  double* vec = lds64;  // the 14 Pv vectors: LDS, or (form 2) this problem's workspace slice, laid out alike
  if constexpr (FORM == 2) vec = a.vecs + b * (kAdjVectors + 4) * Pv;
  double* xb = vec + cv.xb;    // xbar: adjoint of x_{k+1} entering step k, of x_k leaving it
  double* sbp = vec + cv.sbp;  // adjoint of s_k from the update that used it (step k + 1)
  double* gbp = vec + cv.gbp;  // adjoint of g_k from y_{k+1} = g_{k+1} - g_k
  double* anl = vec + cv.an;   // -wbar_{k+1}: the start of a_k
  double* db = vec + cv.db;
  double* gk = vec + cv.gk;
  double* p1 = vec + cv.p1;
  double* p2 = vec + cv.p2;
  double* wb = vec + cv.wb;
  double* akl = vec + cv.ak;
  // H_{k-1} dbar, H_{k-1} wbar: p1 is dead once wbar / sbar are formed, gk until the final loop (which reads
  // hw[i] before it writes gk[i], in the same thread)
  double* hd = p1;
  double* hw = gk;
  Dual64* xd = reinterpret_cast<Dual64*>(vec + cv.xd);
  Dual64* gd = reinterpret_cast<Dual64*>(vec + cv.gd);
  // s_{k-1}, w_{k-1}, y_k, g_k of a step: dead before the step's dual evaluation is set up
  double* sv = vec + cv.xd;
  double* wv = sv + Pv;
  double* yv = vec + cv.gd;
  double* gv = yv + Pv;
  Dual64* views = reinterpret_cast<Dual64*>(lds64 + cv.views);
  Dual64* vpart = reinterpret_cast<Dual64*>(lds64 + cv.vpart);
  double* scratch = lds64 + cv.scratch;
  double* cf = lds64 + cv.coef;
  double* obl = lds64 + cv.obs;  // form 0: the scene's LDS copy
  // the observation cotangent: in LDS (form 0 only), else accumulated in place in the output (or not at all)
  double* obsacc;
  if constexpr (FORM == 0) obsacc = a.obs_lds ? lds64 + cv.obsacc : (a.obs_grad ? a.obs_grad + b * 2 * MN : nullptr);
  else obsacc = a.obs_grad ? a.obs_grad + b * 2 * MN : nullptr;
  uint8_t* vil = reinterpret_cast<uint8_t*>(lds64) + cv.vis_bytes_off;
  const double* obs = obl;
  const uint8_t* vis = vil;

  const double* sc = a.tape + tl.scal + b * tl.T;                  // the scalar row, read in place
  const double* S = a.tape + tl.hist + b * 2 * tl.kcap * Pv;       // history rows s_j
  const double* W = S + (size_t)tl.kcap * Pv;                      // w_j
  const double* X = a.tape + tl.x + b * K * Pv;
  const double* Gr = a.tape + tl.g + b * K * Pv;
  double* Ar = a.arows + b * K * Pv;

  for (int i = tid; i < Pv; i += kBlock) {
    xb[i] = i < P ? a.xbar[b * P + i] : 0.0;
    sbp[i] = gbp[i] = anl[i] = 0.0;
    db[i] = gk[i] = p1[i] = p2[i] = wb[i] = akl[i] = 0.0;
  }
  if constexpr (FORM == 0) {
    for (int i = tid; i < 2 * MN; i += kBlock) {
      obl[i] = a.obs[b * 2 * MN + i];
      if (obsacc) obsacc[i] = 0.0;
    }
    for (int i = tid; i < MN; i += kBlock) vil[i] = a.vis[b * MN + i] ? 1 : 0;
  } else {  // the scene where the caller put it; the cotangent's rows arrive uninitialised
    obs = a.obs + b * 2 * MN;
    vis = a.vis + b * MN;
    if (obsacc)
      for (int i = tid; i < 2 * MN; i += kBlock) obsacc[i] = 0.0;
  }
  int n = a.status[b * DAVA_STATUS_WORDS];
  n = n < 0 ? 0 : (n > K ? K : n);
  double trace = 0.0;  // sum_{j > k} a_j . g_j with every a_j final (needed at k = 1: gamma's adjoint)
  int buf = 0;
  __syncthreads();
  const double gamma = sc[3 * K];

  for (int k = n - 1; k >= 0; --k) {
    const double alpha = sc[k];
    // ---- s_k = alpha d_k, x_{k+1} = x_k + s_k (alpha is a constant of the line search) ----
    if (k == 0) {
      for (int i = tid; i < Pv; i += kBlock) {
        const double d = alpha * (xb[i] + sbp[i]);
        db[i] = d;
        gk[i] = gbp[i] - d;  // d_0 = -g_0
      }
    } else {
      const double* gk1 = Gr + (size_t)(k - 1) * Pv;
      const double* gkr = Gr + (size_t)k * Pv;
      const double* srow = S + (size_t)(k - 1) * Pv;
      const double* wrow = W + (size_t)(k - 1) * Pv;
      double* ak = Ar + (size_t)k * Pv;
      for (int i = tid; i < Pv; i += kBlock) {
        const double d = alpha * (xb[i] + sbp[i]);
        const double g1 = i < P ? gkr[i] : 0.0, g0 = i < P ? gk1[i] : 0.0;
        db[i] = d;
        gv[i] = g1;
        yv[i] = g1 - g0;
        sv[i] = i < P ? srow[i] : 0.0;
        wv[i] = i < P ? wrow[i] : 0.0;
        const double a0 = anl[i] - d;  // d_k = -H_k g_k adds -dbar_k g_k^T to H_k's adjoint
        akl[i] = a0;
        ak[i] = a0;  // row k as the pass below reads it; its final value replaces it at the end of the step
      }
      __syncthreads();
      const double rho = sc[K + k - 1], c = sc[2 * K + k - 1];
      // P1 = (A + A^T) s, P2 = (A + A^T) w over rows (a_j, g_j), j = k .. n-1
      const auto acoef = [](int, double as, double gs, double aw, double gw, double& k1, double& k2, double& k3,
                            double& k4) {
        k1 = gs; k2 = as; k3 = gw; k4 = aw;
      };
      pair_pass(P, Pv, k, n, Ar, Gr, sv, wv, 0.0, acoef, p1, p2, cf);
      double r[7] = {0, 0, 0, 0, 0, 0, 0};
      for (int i = tid; i < P; i += kBlock) {
        const double si = sv[i], wi = wv[i], yi = yv[i], di = db[i];
        r[0] += si * p1[i]; r[1] += si * p2[i]; r[2] += yi * wi; r[3] += si * di; r[4] += wi * di;
        r[5] += yi * yi; r[6] += si * yi;
      }
      block_sum<7>(r, scratch, buf);
      buf ^= 1;
      const double sAs = 0.5 * r[0], sAw = r[1], yw = r[2], sd = r[3], wd = r[4], yy = r[5], t = r[6];
      const double cbar = rho * sAs;
      const double rhobar = c * sAs - sAw + cbar * yw;
      const double tbar = rho > 0.0 ? -(rho * rho) * rhobar : 0.0;  // inverse_curvature backward
      for (int i = tid; i < Pv; i += kBlock) {
        const double q1 = p1[i], q2 = p2[i], yi = yv[i];
        wb[i] = -rho * q1 + (cbar * rho) * yi;
        p2[i] = (cbar * rho) * wv[i] + tbar * sv[i];  // ybar, direct terms
        sbp[i] = (c * rho) * q1 - rho * q2 + tbar * yi;
      }
      __syncthreads();
      // H_{k-1} dbar and H_{k-1} wbar: one pass over history entries 0 .. k-2, plus gamma I
      if (k >= 2) {
        const double* hrho = sc + K;
        const double* hc = sc + 2 * K;
        const auto hcoef = [hrho, hc](int j, double sdv, double wdv, double swv, double wwv, double& k1, double& k2,
                                      double& k3, double& k4) {
          const double rj = hrho[j], cr = hc[j] * rj;
          k1 = cr * sdv - rj * wdv; k2 = -rj * sdv;
          k3 = cr * swv - rj * wwv; k4 = -rj * swv;
        };
        pair_pass(P, Pv, 0, k - 1, S, W, db, wb, gamma, hcoef, hd, hw, cf);
      } else {
        for (int i = tid; i < Pv; i += kBlock) {
          hd[i] = gamma * db[i];
          hw[i] = gamma * wb[i];
        }
      }
      // H_k dbar = H_{k-1} dbar + entry k-1's rank-2 term;  gbar_k, a_k, a_{k-1}
      const double e1 = c * rho * sd - rho * wd, e2 = -rho * sd;
      double tr[1] = {0.0};
      for (int i = tid; i < Pv; i += kBlock) {
        const double ybar = p2[i] + hw[i];  // (hw aliases gk: read before gk is written)
        const double hk = hd[i] + e1 * sv[i] + e2 * wv[i];
        const double w = wb[i];
        gk[i] = gbp[i] - hk + ybar;
        gbp[i] = -ybar;
        const double af = akl[i] + w;
        ak[i] = af;  // final a_k (read by the passes of steps < k)
        anl[i] = -w;
        tr[0] += af * gv[i];
        if (k == 1 && i < P) tr[0] -= w * Gr[i];  // a_0 = -wbar_1
      }
      block_sum<1>(tr, scratch, buf);
      buf ^= 1;
      trace += tr[0];
      if (k == 1) {
        // gamma = clamp(q, min 1e-4), q = t / clamp(yy, min 1e-5); its adjoint is tr(H_0' adjoint)
        const double yyc = clamp_min(yy, 1e-5);
        const double q = t / yyc;
        const double qbar = q >= 1e-4 ? trace : 0.0;  // clamp backward passes where input >= min
        const double tg = qbar / yyc;
        const double yybar = yy >= 1e-5 ? -qbar * q / yyc : 0.0;
        for (int i = tid; i < Pv; i += kBlock) {
          const double yi = yv[i];
          const double extra = tg * sv[i] + 2.0 * yybar * yi;
          sbp[i] += tg * yi;
          gk[i] += extra;
          gbp[i] -= extra;
        }
      }
    }
    // ---- g_k = dE/dx(x_k): xbar += Hess E gbar_k, obsbar += (d2E/dobs dx) gbar_k ----
    // (s, w, y, g_k live in the dual vectors' space: every thread is done with them before it is overwritten)
    __syncthreads();
    const double* xk = X + (size_t)k * Pv;
    for (int i = tid; i < Pv; i += kBlock) {
      xd[i] = i < P ? Dual64(xk[i], gk[i]) : Dual64(0.0);
      gd[i] = Dual64(0.0);
    }
    __syncthreads();
    Dual64 E(0.0), unused(0.0);
    ba_eval<true, false, false, false, false, RES, Dual64>(L, xd, nullptr, 0.0, obs, vis, gd, views, vpart, scratch,
                                                           buf, E, unused, nullptr, obsacc);
    for (int i = tid; i < P; i += kBlock) xb[i] += gd[i].t;
    __syncthreads();
  }
  for (int i = tid; i < P; i += kBlock) a.x0_grad[b * P + i] = xb[i];
  if constexpr (FORM == 0) {
    if (a.obs_grad && a.obs_lds)
      for (int i = tid; i < 2 * MN; i += kBlock) a.obs_grad[b * 2 * MN + i] = obsacc[i];
  }
}

// The form the adjoint takes: the lowest whose image fits 160 KiB (form 0: with the cotangent in LDS or in the
// output), raised (never lowered) by the F64_FORM override as choose_form (solve_f64.hpp) raises the solve's;
// -1 where not even form 2's image (the dual view constants and partials) fits.
inline int choose_adjoint_form(int M, int N, int Pv) {
  int form = 2;
  if (carve_adjoint(M, N, Pv, false).total_bytes <= kMaxLdsBytes) form = 0;
  else if (carve_adjoint_large(M, Pv, 1).total_bytes <= kMaxLdsBytes) form = 1;
  const long long forced = debug_knob(kDbgF64Form);
  if ((forced == 1 || forced == 2) && forced > form) form = (int)forced;
  if (form == 2 && carve_adjoint_large(M, Pv, 2).total_bytes > kMaxLdsBytes) return -1;
  return form;
}

// ---- host side (the conventions of dava_f64.hpp) ----
struct AdjointPlan {
  int status;
  bool launch;  // false: return `status` (a refusal, or DAVA_OK for an empty batch)
  int form, lds, batch, residual;
  bool obs_lds;         // form 0: the observation cotangent accumulates in LDS (where that fits too)
  size_t row_bytes;     // rows a_j: B x K x Pv
  size_t vector_bytes;  // form 2: B x 14 x Pv doubles, else 0
  TapeLayout tape;
  LargeAdjointArgs args;  // the form-0 kernel takes its base
  size_t workspace_bytes() const { return row_bytes + vector_bytes + kTailBytes; }  // [rows | form 2: vectors | tail]
};

// The first checks of the adjoint's entry points and all of its queries (no data pointer is looked at): what a
// scene and a config need, from the shapes alone.
inline AdjointPlan adjoint_shape(const DavaSceneF64* scene, const DavaSolverConfigF64* c, bool any_form) {
  AdjointPlan p{};
  p.form = -1;
  DavaScene sc;
  p.status = check_scene_f64(scene, false, sc);  // (the launch checks the data pointers itself)
  if (p.status != DAVA_OK) return p;
  p.status = DAVA_ERR_INVALID_ARGUMENT;
  if (!c || c->iterations < 0) return p;
  p.status = DAVA_ERR_UNSUPPORTED;
  if (c->iterations < 1 || c->iterations > kMaxIterations) return p;
  const int M = sc.num_views, N = sc.num_points, Pv = round_up(sc.num_parameters, 4);
  const bool fits0 = carve_adjoint(M, N, Pv, false).total_bytes <= kMaxLdsBytes;
  p.form = any_form ? choose_adjoint_form(M, N, Pv) : fits0 ? 0 : -1;
  if (p.form < 0) return p;
  p.status = DAVA_OK;
  p.obs_lds = p.form == 0 && carve_adjoint(M, N, Pv, true).total_bytes <= kMaxLdsBytes;
  p.lds = (int)(p.form == 0 ? carve_adjoint(M, N, Pv, p.obs_lds) : carve_adjoint_large(M, Pv, p.form)).total_bytes;
  p.batch = sc.batch;
  p.residual = sc.residual;
  p.args.L = make_layout(&sc);
  p.tape = tape_layout_f64(sc.batch, sc.num_parameters, c->iterations);
  p.row_bytes = (size_t)sc.batch * p.tape.K * p.tape.Pv * sizeof(double);
  p.vector_bytes = p.form == 2 ? (size_t)sc.batch * (kAdjVectors + 4) * p.tape.Pv * sizeof(double) : 0;
  return p;
}

// the checks of both entry points, in their order
inline AdjointPlan plan_adjoint(const DavaSceneF64* scene, const DavaSolverConfigF64* c, const void* tape,
                                size_t tape_bytes, const int32_t* status, const double* x_out_grad, double* x0_grad,
                                double* observations_grad, void* workspace, size_t workspace_bytes, bool any_form) {
  AdjointPlan p = adjoint_shape(scene, c, any_form);
  const auto refuse = [&p](int st) {
    p.status = st;
    return p;
  };
  if (p.status != DAVA_OK || p.batch == 0) return p;
  if (!scene->observations || !scene->visibility || !tape || !status || !x_out_grad || !x0_grad)
    return refuse(DAVA_ERR_INVALID_ARGUMENT);
  const TapeLayout& tl = p.tape;
  if (tape_bytes < tl.queue_byte) return refuse(DAVA_ERR_WORKSPACE);
  if (!workspace || workspace_bytes < p.row_bytes + p.vector_bytes) return refuse(DAVA_ERR_WORKSPACE);  // (no tail)
  LargeAdjointArgs& a = p.args;
  a.Pv = tl.Pv;
  a.K = tl.K;
  a.tl = tl;
  a.tape = static_cast<const double*>(tape);
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.status = status;
  a.xbar = x_out_grad;
  a.x0_grad = x0_grad;
  a.obs_grad = observations_grad;
  a.arows = static_cast<double*>(workspace);
  a.obs_lds = p.obs_lds ? 1 : 0;
  a.vecs = p.form == 2 ? reinterpret_cast<double*>(static_cast<char*>(workspace) + p.row_bytes) : nullptr;
  p.launch = true;
  return p;
}

template <int FORM>
int launch_adjoint(const AdjointPlan& p, void* stream) {
  const adjoint_args_t<FORM>& a = p.args;
  with_flag(p.residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
    constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
    const auto kernel = bfgs_ba_adjoint_f64_kernel<kRes, FORM>;
    set_dynamic_lds(kernel, p.lds);
    hipLaunchKernelGGL(kernel, dim3(p.batch), dim3(kBlock), p.lds, static_cast<hipStream_t>(stream), a);
  });
  return launched();
}

// A plan's outcome where it asks for no launch, else the form-0 launch: instantiated in bfgs_adjoint_f64.hip, and
// reached from bfgs_adjoint_large_f64.hip for a scene whose whole image fits LDS.
int adjoint_form0(const AdjointPlan& p, void* stream);

}  // namespace f64
}  // namespace dava
