// The device passes of the fused solve (bfgs_solve.hip) over the inverse Hessian -- the dense sweep, the
// hybrid fold and the compact-history products in their two-pass, wide (global-vector) and fused (LDS-mode)
// forms -- with their helpers, constants and measurement notes.  Device code only: the solve kernel and
// the microbenchmarks (tools/micro/solve_pass_stream.hip, wide_pass_stream.hip) include it.
#pragma once

#include <type_traits>

#include "solve_plan.hpp"

namespace dava {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// LDS-mode fused pass: rows of at most this many float4 groups per lane go through buffer loads (bitwise
// equal; C1, C2: C2 +2.5%, profiles/r03_ab_fused_buffer_loads_small.log; all rows, i.e. 4: C3 -6%,
// profiles/r03_ab_buffer_loads.log).  (The GV wide pass through buffer loads: C5 -2.5 .. +1.8% across
// boxes, not kept.)
constexpr int kFusedBufferLoadsGM = 2;
constexpr int kSweepRows = 4;  // DENSE sweep: matrix rows in flight per lane

// Streaming access to the inverse Hessian: every element is read once and written once per BFGS
// iteration, never reused by another workgroup (non-temporal loads and stores measured no better,
// profiles/r01_ab_sweep_variants.log).
__device__ __forceinline__ f4v h_load(const float* p) { return *reinterpret_cast<const f4v*>(p); }
__device__ __forceinline__ void h_store(float* p, f4v v) { *reinterpret_cast<f4v*>(p) = v; }

// Apply the pending rank-2 term to one element (bfgs_solver.py:298-303 order:
// ((H + (s_rho_i s_j) c) - s_rho_i yH_j) - Hy_i s_rho_j, no FMA contraction).
__device__ __forceinline__ float rank2(float h, float sri, float sj, float c, float hyj, float hyi, float srj) {
  float t = __fadd_rn(h, __fmul_rn(__fmul_rn(sri, sj), c));
  t = __fsub_rn(t, __fmul_rn(sri, hyj));
  return __fsub_rn(t, __fmul_rn(hyi, srj));
}

// One sweep over the dense inverse Hessian of this problem.
//   H' = Hs + pending,  Hs = stored matrix (or gamma0*I if not materialised)
//   hy_out[j] = sum_i H'_ij y_i,  hg_out[j] = sum_i H'_ij g_i   (y = g - gp)
// Writes H' back.  Column ownership: the ceil(P/4) float4 column groups are
// split evenly over the 4 waves (wave w owns groups [w*Gw, (w+1)*Gw)), one
// group per lane per 64-group block, so every wave streams and every global
// access is a contiguous row piece of up to 1 KiB.  Lane = column means the
// column sums need no cross-lane reduction.  U rows are loaded before any is
// consumed to keep U KiB per wave in flight.
template <int NW, bool PIPE>
__device__ __forceinline__ void dense_sweep(const Layout& L, int Pld, float* __restrict__ H, bool materialized, float gamma0,
                            const float* ps, const float* phy, float prho, float pc, const float* g,
                            const float* gp, float* hy_out, float* hg_out) {
  constexpr int U = kSweepRows;
  const int P = L.P;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int G = (P + 3) / 4;                      // float4 column groups
  const int Gw = (G + NW - 1) / NW;       // groups per wave
  const int g_end = min(G, (wave + 1) * Gw);
  for (int gb = wave * Gw; gb < g_end; gb += kWave) {
    const int grp = gb + lane;
    const bool act = grp < g_end;
    const int j0 = grp * 4;
    float sj[4] = {0, 0, 0, 0}, hj[4] = {0, 0, 0, 0}, srj[4] = {0, 0, 0, 0};
    if (act) {
      const float4 a = ld4(ps + j0), b = ld4(phy + j0);
      sj[0] = a.x; sj[1] = a.y; sj[2] = a.z; sj[3] = a.w;
      hj[0] = b.x; hj[1] = b.y; hj[2] = b.z; hj[3] = b.w;
#pragma unroll
      for (int k = 0; k < 4; ++k) srj[k] = __fmul_rn(sj[k], prho);
    }
    float ay[4] = {0, 0, 0, 0}, ag[4] = {0, 0, 0, 0};
    float* col = H + j0;
    auto row_update = [&](int r, f4v h) {
      const float gi = g[r], yi = gi - gp[r];
      const float sri = __fmul_rn(ps[r], prho), hyi = phy[r];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        h[k] = rank2(h[k], sri, sj[k], pc, hj[k], hyi, srj[k]);
        ay[k] += h[k] * yi;
        ag[k] += h[k] * gi;
      }
      if (act) h_store(col + (size_t)r * Pld, h);
    };
    auto synth = [&](int r) {  // row r of gamma0 * I restricted to this lane's 4 columns
      f4v h;
      h[0] = r == j0 ? gamma0 : 0.f; h[1] = r == j0 + 1 ? gamma0 : 0.f;
      h[2] = r == j0 + 2 ? gamma0 : 0.f; h[3] = r == j0 + 3 ? gamma0 : 0.f;
      return h;
    };
    int i = 0;
    // (the buffer descriptor's range is 32-bit: matrices past 2 GiB, P > 23,170, take the loop below)
    if (PIPE && materialized && (size_t)P * Pld * sizeof(float) < (1ull << 31)) {
      // Global-vector mode (one problem per CU, rows of thousands of groups): software-pipelined,
      // two batches of U rows in flight per wave, through buffer loads / stores (a lane past the
      // wave's groups gets an offset past the descriptor's range: its load returns 0 and its store
      // is dropped, no branch).  Without branches around the memory operations the compiler waits
      // vmcnt(8..11) before a row instead of the vmcnt(0) the predicated loads force (a full round
      // trip plus the previous batch's stores per batch).  The batches ahead are clamped to row P - 1
      // (a few redundant loads at the end, never consumed).  Same arithmetic, same order: bitwise.
      // C5 dense +4.9%; the LDS-mode kernels keep the predicated loop below: there (C3, two problems
      // per CU) the same change measured -2.8%, one batch ahead -0.4%, and 8 or 16 rows per batch
      // -0.4 / -2.7% (profiles/r05_ab_dense_sweep_pipe.log, r01_ab_sweep_variants.log).
      const auto rs = make_rsrc(H, (int)((size_t)P * Pld * sizeof(float)));
      const unsigned rowb = (unsigned)Pld * 4u;
      const unsigned base = act ? (unsigned)j0 * 4u : 0x80000000u;
      auto ldrow = [&](int r) {
        return __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(base + (unsigned)r * rowb), 0, 0));
      };
      auto strow = [&](int r, f4v h) {
        typedef unsigned u4v __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, h), rs, (int)(base + (unsigned)r * rowb), 0, 0);
      };
      auto update = [&](int r, f4v h, float gi, float gpi, float psi, float phyi) {
        const float yi = gi - gpi;
        const float sri = __fmul_rn(psi, prho), hyi = phyi;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          h[k] = rank2(h[k], sri, sj[k], pc, hj[k], hyi, srj[k]);
          ay[k] += h[k] * yi;
          ag[k] += h[k] * gi;
        }
        strow(r, h);
      };
      static_assert(U == 4, "the row scalars are read as float4");
      auto consume = [&](int r0, const f4v* h) {
        const float4 g4 = ld4(g + r0), gp4 = ld4(gp + r0), ps4 = ld4(ps + r0), phy4 = ld4(phy + r0);
        update(r0, h[0], g4.x, gp4.x, ps4.x, phy4.x);
        update(r0 + 1, h[1], g4.y, gp4.y, ps4.y, phy4.y);
        update(r0 + 2, h[2], g4.z, gp4.z, ps4.z, phy4.z);
        update(r0 + 3, h[3], g4.w, gp4.w, ps4.w, phy4.w);
      };
      auto tail = [&](int r0, const f4v* h) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (r0 + u < P) update(r0 + u, h[u], g[r0 + u], gp[r0 + u], ps[r0 + u], phy[r0 + u]);
      };
      // two batches in flight, rotated without register copies (a copy would wait for the loads)
      f4v A[U], Bq[U];
#pragma unroll
      for (int u = 0; u < U; ++u) A[u] = ldrow(min(u, P - 1));
#pragma unroll
      for (int u = 0; u < U; ++u) Bq[u] = ldrow(min(U + u, P - 1));
      for (; i + 2 * U <= P; i += 2 * U) {
        consume(i, A);
#pragma unroll
        for (int u = 0; u < U; ++u) A[u] = ldrow(min(i + 2 * U + u, P - 1));
        consume(i + U, Bq);
#pragma unroll
        for (int u = 0; u < U; ++u) Bq[u] = ldrow(min(i + 3 * U + u, P - 1));
      }
      if (i + U <= P) {
        consume(i, A);
        tail(i + U, Bq);
      } else {
        tail(i, A);
      }
    } else if (materialized) {
      for (; i + U <= P; i += U) {
        f4v h[U];
#pragma unroll
        for (int u = 0; u < U; ++u) h[u] = act ? h_load(col + (size_t)(i + u) * Pld) : f4v{0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < U; ++u) row_update(i + u, h[u]);
      }
      for (; i < P; ++i) row_update(i, act ? h_load(col + (size_t)i * Pld) : f4v{0, 0, 0, 0});
    } else {
      for (; i < P; ++i) row_update(i, synth(i));
    }
    if (act) {
      st4(hy_out + j0, make_float4(ay[0], ay[1], ay[2], ay[3]));
      st4(hg_out + j0, make_float4(ag[0], ag[1], ag[2], ag[3]));
    }
  }
}

// HYBRID: COMPACT until the history is full (kcap = 1024 entries), then the dense matrix.  A problem
// still running at iteration kcap + 1 folds its history into H once,
//   H_ij = gamma0 delta_ij + sum_e [ s_ei (c_e rho_e s_ej - rho_e w_ej) - w_ei (rho_e s_ej) ]
// (the rank-2 terms U_e the history stands for, compact_products), and continues with dense_sweep.  The
// iteration cap alone never pays for the dense matrix: with the reference's stopping rules problems stop
// long before 1025 iterations, in the compact phase.  Same mapping as dense_sweep (lane = float4 column
// group, the wave's share of the groups), kFoldRows rows per pass in registers, every history entry streamed
// once per pass.  Entries e < lcap are the LDS-resident ones (LH: S row then W row).  The fold is a sum in
// entry order, not the reference's sequence of rank-2 updates: the same matrix up to rounding, as COMPACT
// itself.  Its cost is P / kFoldRows passes over the whole history, and per entry and pass 2 kFoldRows row
// values every lane needs: loaded once, coalesced, by 2 kFoldRows lanes and broadcast through SGPRs
// (v_readlane; kFoldReadlane) rather than as wave-uniform vector loads.  K = 1,100 fixed (every problem folds;
// interleaved, bitwise equal, profiles/r06j_fold_rows_readlane_ab.log): 8 rows with uniform loads (r05) C3
// 8.33 s, C5 41.9 s (the fold ~34 s of it); 16 / 32 rows with uniform loads C5 19.3 / 47.0 s; readlane 16 / 32
// rows C5 **17.3** / 14.4 s, C3 **7.64** / 7.17 s.  16 rows: at 32 (128 accumulators) the LDS-mode ray-angle
// hybrid kernel -- already at 256 VGPRs with ~300 SGPRs spilled -- returned wrong results
// (test_hybrid_switch_ray_angle_matches_oracle, rel 0.83; 16 and 8 rows pass,
// profiles/r06l_fold_variants_hybrid_ray_test.log).  (One column per lane, 32 rows, uniform loads: C5 67.7 s,
// profiles/r06i_fold_column_lanes_rejected.log.)
#ifndef DAVA_FOLD_ROWS
#define DAVA_FOLD_ROWS 16
#endif
constexpr int kFoldRows = DAVA_FOLD_ROWS;
static_assert(kFoldRows == 8 || kFoldRows == 16,
              "fold_history: 8 or 16 rows per pass; 32 rows gave wrong results in the LDS-mode ray-angle hybrid kernel "
              "(profiles/r06l_fold_variants_hybrid_ray_test.log, ADVICE.md item 3) and the cause is not known yet");
#ifndef DAVA_FOLD_READLANE
#define DAVA_FOLD_READLANE 1
#endif
constexpr bool kFoldReadlane = DAVA_FOLD_READLANE != 0;
template <int NW>
__device__ void fold_history(int P, int Pv, int Pld, int nh, const float* __restrict__ S, const float* __restrict__ W,
                             const float* LH, int lcap, const float* hrho, const float* hc, float gamma0,
                             float* __restrict__ H) {
  constexpr int R = kFoldRows;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int G = (P + 3) / 4;
  const int Gw = (G + NW - 1) / NW;
  const int g_end = min(G, (wave + 1) * Gw);
  for (int gb = wave * Gw; gb < g_end; gb += kWave) {
    const int grp = gb + lane;
    const bool act = grp < g_end;
    const int j0 = grp * 4;
    for (int i0 = 0; i0 < P; i0 += R) {
      float h[R][4];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) h[r][q] = i0 + r == j0 + q ? gamma0 : 0.f;
      for (int e = 0; e < nh; ++e) {
        const float* sr = e < lcap ? LH + (size_t)2 * e * Pv : S + (size_t)e * Pv;
        const float* wr = e < lcap ? sr + Pv : W + (size_t)e * Pv;
        const float rho = hrho[e], crho = hc[e] * rho;
        float u[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0};
        if (act) {
          const float4 s4 = ld4(sr + j0), w4 = ld4(wr + j0);
          const float sj[4] = {s4.x, s4.y, s4.z, s4.w}, wj[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            u[q] = crho * sj[q] - rho * wj[q];
            v[q] = rho * sj[q];
          }
        }
        if constexpr (kFoldReadlane) {
          // the pass's 2R row values in one coalesced load (lane r: s_e[i0 + r], lane R + r: w_e[i0 + r]), then
          // broadcast to every lane through SGPRs (v_readlane) instead of 2R wave-uniform vector loads
          static_assert(2 * R <= kWave, "one row value per lane");
          float rv = 0.f;
          if (lane < 2 * R) {
            const int rr = lane < R ? lane : lane - R;
            rv = (lane < R ? sr : wr)[min(i0 + rr, P - 1)];
          }
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const float si = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rv), r));
            const float wi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rv), R + r));
#pragma unroll
            for (int q = 0; q < 4; ++q) h[r][q] += si * u[q] - wi * v[q];
          }
        } else {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int i = min(i0 + r, P - 1);  // (rows past P are computed and dropped)
            const float si = sr[i], wi = wr[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) h[r][q] += si * u[q] - wi * v[q];
          }
        }
      }
      if (act)
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (i0 + r < P) {
            f4v o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = j0 + q < P ? h[r][q] : 0.f;
            h_store(H + (size_t)(i0 + r) * Pld + j0, o);
          }
    }
  }
}

// COMPACT mode: the inverse Hessian is never formed.  The exact BFGS history
//   H_k = gamma0 I + sum_j U_j,   U_j v = c_j rho_j (s_j.v) s_j - rho_j (w_j.v) s_j - rho_j (s_j.v) w_j
// (w_j = H_{j-1} y_j, the same rank-2 terms the reference adds to its dense H,
// bfgs_solver.py:263-303) is kept in HBM as rows S[j], W[j] of Pv floats, so
// a product H v costs 2 passes over 2 nh P floats instead of a P^2 sweep.
// Pass 1: 4 dots per entry (s.y, w.y, s.g, w.g) -> coefficients in LDS.
// Pass 2: a = H y and b = H g as coefficient-weighted sums of the rows.
template <int U, int NW>  // U: column groups of both rows in flight per lane in pass 1
__device__ __forceinline__ void compact_products(int P, int Pv, int nh, const float* __restrict__ S, const float* __restrict__ W,
                                 float* coef, const float* hrho, const float* hc, float gamma0, const float* g,
                                 const float* gp, float* a_out, float* b_out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);  // scalar: row addresses wave-uniform
  const int G = (P + 3) / 4;
  for (int j = wave; j < nh; j += NW) {
    const float* sr = S + (size_t)j * Pv;
    const float* wr = W + (size_t)j * Pv;
    float sy = 0.f, wy = 0.f, sg = 0.f, wg = 0.f;
    auto dots = [&](int q, const f4v& s4, const f4v& w4) {
      const float4 g4 = ld4(g + 4 * q), p4 = ld4(gp + 4 * q);
      const float y0 = g4.x - p4.x, y1 = g4.y - p4.y, y2 = g4.z - p4.z, y3 = g4.w - p4.w;
      sy += s4[0] * y0 + s4[1] * y1 + s4[2] * y2 + s4[3] * y3;
      wy += w4[0] * y0 + w4[1] * y1 + w4[2] * y2 + w4[3] * y3;
      sg += s4[0] * g4.x + s4[1] * g4.y + s4[2] * g4.z + s4[3] * g4.w;
      wg += w4[0] * g4.x + w4[1] * g4.y + w4[2] * g4.z + w4[3] * g4.w;
    };
    int q = lane;
    for (; q + (U - 1) * kWave < G; q += U * kWave) {
      f4v s4[U], w4[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s4[u] = *reinterpret_cast<const f4v*>(sr + 4 * (q + u * kWave));
        w4[u] = *reinterpret_cast<const f4v*>(wr + 4 * (q + u * kWave));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) dots(q + u * kWave, s4[u], w4[u]);
    }
    for (; q < G; q += kWave)
      dots(q, *reinterpret_cast<const f4v*>(sr + 4 * q), *reinterpret_cast<const f4v*>(wr + 4 * q));
    sy = wave_sum(sy); wy = wave_sum(wy); sg = wave_sum(sg); wg = wave_sum(wg);
    if (lane == 0) {
      const float rho = hrho[j], cr = hc[j] * rho;
      coef[4 * j + 0] = cr * sy - rho * wy;
      coef[4 * j + 1] = -rho * sy;
      coef[4 * j + 2] = cr * sg - rho * wg;
      coef[4 * j + 3] = -rho * sg;
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < G; q += (kWave * NW)) {
    const float4 g4 = ld4(g + 4 * q), p4 = ld4(gp + 4 * q);
    f4v y4 = {g4.x - p4.x, g4.y - p4.y, g4.z - p4.z, g4.w - p4.w};
    f4v gg = {g4.x, g4.y, g4.z, g4.w};
    f4v a4 = gamma0 * y4, b4 = gamma0 * gg;
    const float* sr = S + 4 * q;
    const float* wr = W + 4 * q;
    int j = 0;
    for (; j + 4 <= nh; j += 4) {
      f4v s4[4], w4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s4[u] = *reinterpret_cast<const f4v*>(sr + (size_t)(j + u) * Pv);
        w4[u] = *reinterpret_cast<const f4v*>(wr + (size_t)(j + u) * Pv);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 cf = ld4(coef + 4 * (j + u));
        a4 += cf.x * s4[u] + cf.y * w4[u];
        b4 += cf.z * s4[u] + cf.w * w4[u];
      }
    }
    for (; j < nh; ++j) {
      const f4v s4 = *reinterpret_cast<const f4v*>(sr + (size_t)j * Pv);
      const f4v w4 = *reinterpret_cast<const f4v*>(wr + (size_t)j * Pv);
      const float4 cf = ld4(coef + 4 * j);
      a4 += cf.x * s4 + cf.y * w4;
      b4 += cf.z * s4 + cf.w * w4;
    }
    st4(a_out + 4 * q, make_float4(a4[0], a4[1], a4[2], a4[3]));
    st4(b_out + 4 * q, make_float4(b4[0], b4[1], b4[2], b4[3]));
  }
}

// COMPACT mode, GV (long rows, 8-wave workgroup): one pass over the history, workgroup-wide.
// Thread t owns float4 column groups t, t + 512, ... (GT of them) and keeps its columns of
// y, g and of the two running sums in registers.  E entries per round (2 while GT <= 4, else
// 1 so that s, w, y, g and the sums fit in 256 VGPRs): every thread loads its columns of the
// entries' s and w rows, forms its partial dots with y and g, one block reduction gives the
// 4E dots to every thread in the same order, and each thread adds the entries'
// contributions to its own columns of H y and H g.  Rows cross HBM once per iteration (the
// two-pass variant reads them twice).
template <int GT, int NW>
__device__ __forceinline__ void compact_products_wide(int P, int Pv, int nh, const float* __restrict__ S,
                                                      const float* __restrict__ W, const float* hrho, const float* hc,
                                                      float gamma0, const float* g, const float* gp, float* a_out,
                                                      float* b_out, float* scratch, int& buf) {
  constexpr int BLOCK = kWave * NW;
  constexpr int E = GT <= 2 ? 2 : kGvEntries;
  const int tid = threadIdx.x;
  const int G = (P + 3) / 4;
  const f4v z = f4v{0, 0, 0, 0};
  f4v y[GT], gg[GT], pa[GT], pb[GT];
#pragma unroll
  for (int u = 0; u < GT; ++u) {
    const int q = tid + u * BLOCK;
    y[u] = gg[u] = pa[u] = pb[u] = z;
    if (q < G) {
      gg[u] = *reinterpret_cast<const f4v*>(g + 4 * q);
      y[u] = gg[u] - *reinterpret_cast<const f4v*>(gp + 4 * q);
    }
  }
  auto dot4 = [](f4v a, f4v b) { const f4v t = a * b; return (t[0] + t[1]) + (t[2] + t[3]); };
  for (int j = 0; j < nh; j += E) {
    const int ne = min(E, nh - j);  // uniform
    f4v s4[E][GT], w4[E][GT];
    float d[4 * E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
#pragma unroll
      for (int u = 0; u < GT; ++u) {
        const int q = tid + u * BLOCK;
        if (u < GT - 1 && (E == 1 || e < ne)) {  // groups 0 .. GT-2 lie inside the row for every thread
          s4[e][u] = *reinterpret_cast<const f4v*>(S + (size_t)(j + e) * Pv + 4 * q);
          w4[e][u] = *reinterpret_cast<const f4v*>(W + (size_t)(j + e) * Pv + 4 * q);
          continue;
        }
        s4[e][u] = w4[e][u] = z;
        if (e < ne && q < G) {
          s4[e][u] = *reinterpret_cast<const f4v*>(S + (size_t)(j + e) * Pv + 4 * q);
          w4[e][u] = *reinterpret_cast<const f4v*>(W + (size_t)(j + e) * Pv + 4 * q);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      d[4 * e] = d[4 * e + 1] = d[4 * e + 2] = d[4 * e + 3] = 0.0f;
#pragma unroll
      for (int u = 0; u < GT; ++u) {
        d[4 * e] += dot4(s4[e][u], y[u]);
        d[4 * e + 1] += dot4(w4[e][u], y[u]);
        d[4 * e + 2] += dot4(s4[e][u], gg[u]);
        d[4 * e + 3] += dot4(w4[e][u], gg[u]);
      }
    }
    block_sum<4 * E, NW>(d, scratch, buf);
    buf ^= 1;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (e < ne) {
        const float rho = hrho[j + e], cr = hc[j + e] * rho;
        const float ay = cr * d[4 * e] - rho * d[4 * e + 1], by = -rho * d[4 * e];
        const float ag = cr * d[4 * e + 2] - rho * d[4 * e + 3], bg = -rho * d[4 * e + 2];
#pragma unroll
        for (int u = 0; u < GT; ++u) {
          pa[u] += ay * s4[e][u] + by * w4[e][u];
          pb[u] += ag * s4[e][u] + bg * w4[e][u];
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < GT; ++u) {
    const int q = tid + u * BLOCK;
    if (q < G) {
      *reinterpret_cast<f4v*>(a_out + 4 * q) = pa[u] + gamma0 * y[u];
      *reinterpret_cast<f4v*>(b_out + 4 * q) = pb[u] + gamma0 * gg[u];
    }
  }
}

// GV mode, COMPACT, iteration k >= 2: the workgroup-wide history pass of compact_products_wide and
// everything up to the line search in ONE sweep over this thread's float4 column groups, from
// registers: H'y and H'g stay in registers (never written to the workspace), s_{k-1} is loaded
// once, the four curvature dots go through one block reduction, then d = -H_k g (same per-element
// formula as the generic tail), phi'(0)'s partial d.g, and the history append (W row <- H'y,
// S row <- s) -- instead of four more passes over workspace vectors (C5: the direction phase was
// 9% of the solve, profiles/r02_phase_cycles_c5.log).  Returns this thread's d.g partial.
// Per entry the four dots are packed 2-wide FMA chains over this thread's groups (v_pk_fma_f32,
// as the LDS-mode pass does) and the contributions to H'y, H'g packed FMAs: at C5 (GT = 7) ~250
// VALU ops per entry and wave instead of ~420.  (Rejected, interleaved A/B,
// profiles/r03_ab_c5_park_yg_lds.log: parking y and g in the dead LDS gradient / direction slots to
// free registers for two entries per reduction -- bitwise equal, but the per-entry LDS re-reads and
// the spills cost 14% with one entry and 19% with two.  Forming only H'g from the history and
// H'y = H'g + d_prev: two entries per reduction, +0.5..0.9% at C5 but a different rounding that moved
// a C2 problem 2.1e-5 from the oracle, profiles/r03_ab_hy_from_d.log.  r05, in the microbenchmark
// tools/micro/wide_pass_stream.hip: each wave owning a contiguous segment of every row instead of the
// strided groups t, t + BLOCK, ... -- 4.68 vs 4.76 us per entry staged, 4.74 vs 4.71 in registers at
// B = 256, another rounding; not adopted, profiles/r05_micro_wide_pass_ownership.log.)
template <int GT, int NW, bool STAGED = false, int ROWSLOTS = 2>
__device__ __forceinline__ float wide_direction(int P, int Pv, int nh, const float* __restrict__ S,
                                                const float* __restrict__ W, float* hrho, float* hc, float gamma0,
                                                const float* g, const float* gp, const float* s_cur, float* d,
                                                float* s_row, float* w_row, float* scratch, int& buf, int entry,
                                                float* tape_rho, float* tape_c, float* stage = nullptr,
                                                size_t row_stride = 0) {
  constexpr int BLOCK = kWave * NW;
  constexpr int E = GT <= 2 ? 2 : kGvEntries;
  const size_t RSd = row_stride ? row_stride : (size_t)Pv;  // floats from one history row to the next
  const int tid = threadIdx.x;
  const int G = (P + 3) / 4;
  const f4v z = f4v{0, 0, 0, 0};
  f4v y[GT], gg[GT], pa[GT], pb[GT];
#pragma unroll
  for (int u = 0; u < GT; ++u) {
    const int q = tid + u * BLOCK;
    y[u] = gg[u] = pa[u] = pb[u] = z;
    if (q < G) {
      gg[u] = *reinterpret_cast<const f4v*>(g + 4 * q);
      y[u] = gg[u] - *reinterpret_cast<const f4v*>(gp + 4 * q);
    }
  }
  // STAGED (XL images: stage = the dead LDS slots of d and the objective's gradient, 2 Pv floats): every
  // entry's rows come HBM -> LDS by global_load_lds (no registers in flight), issued for entry j + 1 as
  // soon as this thread has read entry j's groups back, so the copy runs under entry j's dots, block
  // reduction and accumulation.  Each thread copies and reads back only its own float4 groups (the copy's
  // lane-linear LDS layout is this pass's column ownership), so the staging buffer needs no barrier; the
  // copy is issued from inline asm so that the compiler's wait accounting does not stall the LDS traffic
  // of the reduction behind it, and its completion is waited for explicitly (vmcnt(0)) before the read.
  // The same rows, dots and sums in the same order: bitwise the register path's result
  // (profiles/r04_dma_stream_bitwise.log); C5 +4.5% (profiles/r04_ab_c5_dma_stream_rotmat.log).  M0 (the
  // copy's LDS base) is saved and restored around each copy, so the compiler's view of it stays true.
  constexpr bool staged = STAGED && E == 1;
  if constexpr (staged) {
    {
      typedef __attribute__((address_space(3))) float lds_float;
      const int wave = tid / kWave;
      const unsigned stage_off = __builtin_amdgcn_readfirstlane(
          (unsigned)(uintptr_t)((lds_float*)stage) + 16u * (unsigned)(wave * kWave));
      const unsigned lane_off = 16u * (unsigned)(tid % kWave);  // this lane's 16 B within a wave's group
      // copies address the rows as a wave-uniform 64-bit base (SGPRs) plus this thread's 32-bit byte
      // offset 16 (tid + u BLOCK), so a copy costs one VGPR, not a 64-bit address per group
      auto uniform_ptr64 = [](const float* p) {  // wave-uniform 64-bit address, in SGPRs
        const unsigned long long v = (unsigned long long)(uintptr_t)p;
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
        return ((unsigned long long)hi << 32) | lo;
      };
      const unsigned w_bytes = __builtin_amdgcn_readfirstlane(4u * (unsigned)Pv);
      const unsigned voff = 16u * (unsigned)tid;  // one VGPR for every group: the group's step is in the base
      // The stage holds ROWSLOTS rows (Pv floats each; the solve's XL image has room for 2, one entry): the
      // rows stream as S_0, W_0, S_1, W_1, ..., row r into slot r % ROWSLOTS, each issued as soon as the row
      // ROWSLOTS before it (same slot) has been read back.  ROWSLOTS = 2 is one entry: entry j + 1 copied
      // while entry j is consumed.
      const int nrows = 2 * nh;
      auto copy_row = [&](int r) {  // row r (entry r / 2, S or W) -> slot r % ROWSLOTS, this thread's groups
        const float* row = ((r & 1) ? W : S) + (size_t)(r >> 1) * RSd;
        const unsigned slot_off = __builtin_amdgcn_readfirstlane(4u * (unsigned)Pv * (unsigned)(r % ROWSLOTS));
#pragma unroll
        for (int u = 0; u < GT; ++u) {
          const int q = tid + u * BLOCK;
          const unsigned long long row_u = uniform_ptr64(row + 4 * u * BLOCK);
          const unsigned ds = __builtin_amdgcn_readfirstlane(stage_off + slot_off + 16u * (unsigned)(u * BLOCK));
          if (q < G) {
            unsigned saved;
            asm volatile(
                "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                "s_mov_b32 m0, %0"
                : "=&s"(saved)
                : "v"(voff), "s"(row_u), "s"(ds)
                : "memory");
          }
        }
      };
      (void)lane_off;
      (void)w_bytes;
#pragma unroll
      for (int r = 0; r < ROWSLOTS; ++r)
        if (r < nrows) copy_row(r);
      // (the last group's copies are issued only by waves with lanes in it)
      const bool hl = __builtin_amdgcn_readfirstlane(tid / kWave) * kWave + (GT - 1) * BLOCK < G;
      for (int j = 0; j < nh; ++j) {
        // rows 2j and 2j + 1 must have landed; rows issued after them may stay in flight
        if (ROWSLOTS > 2 && 2 * j + 2 < nrows) {
          if (hl) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GT * (ROWSLOTS - 2)) : "memory");
          else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((GT - 1) * (ROWSLOTS - 2)) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's copies of entry j have landed
        }
        const float* st_s = stage + Pv * ((2 * j) % ROWSLOTS) + 4 * tid;  // this thread's groups: + 4 u BLOCK
        const float* st_w = stage + Pv * ((2 * j + 1) % ROWSLOTS) + 4 * tid;
        f4v s4[GT], w4[GT];
#pragma unroll
        for (int u = 0; u < GT; ++u) {
          const int q = tid + u * BLOCK;
          s4[u] = w4[u] = z;
          if (u < GT - 1 || q < G) {
            s4[u] = *reinterpret_cast<const f4v*>(st_s + 4 * u * BLOCK);
            w4[u] = *reinterpret_cast<const f4v*>(st_w + 4 * u * BLOCK);
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // read back before the next copies overwrite it
        if (2 * j + ROWSLOTS < nrows) copy_row(2 * j + ROWSLOTS);
        if (2 * j + 1 + ROWSLOTS < nrows) copy_row(2 * j + 1 + ROWSLOTS);
        f2v sy2 = {0.f, 0.f}, wy2 = {0.f, 0.f}, sg2 = {0.f, 0.f}, wg2 = {0.f, 0.f};
#pragma unroll
        for (int u = 0; u < GT; ++u) {
          sy2 = pk_fma(s4[u].lo, y[u].lo, sy2); sy2 = pk_fma(s4[u].hi, y[u].hi, sy2);
          wy2 = pk_fma(w4[u].lo, y[u].lo, wy2); wy2 = pk_fma(w4[u].hi, y[u].hi, wy2);
          sg2 = pk_fma(s4[u].lo, gg[u].lo, sg2); sg2 = pk_fma(s4[u].hi, gg[u].hi, sg2);
          wg2 = pk_fma(w4[u].lo, gg[u].lo, wg2); wg2 = pk_fma(w4[u].hi, gg[u].hi, wg2);
        }
        float dd[4] = {sy2.x + sy2.y, wy2.x + wy2.y, sg2.x + sg2.y, wg2.x + wg2.y};
#if DAVA_MICRO_NOSYNC  // (tools/micro/wide_pass_stream.hip only: the wave's own partial dots, no barrier -- timing)
        wave_sums<4>(dd);
#else
        block_sum<4, NW, true>(dd, scratch, buf);
        buf ^= 1;
#endif
        const float rho = hrho[j], cr = hc[j] * rho;
        const float ay = fmaf(cr, dd[0], -(rho * dd[1])), by = -rho * dd[0];
        const float ag = fmaf(cr, dd[2], -(rho * dd[3])), bg = -rho * dd[2];
#pragma unroll
        for (int u = 0; u < GT; ++u) {
          pa[u] = pk_fma4(by, w4[u], pk_fma4(ay, s4[u], pa[u]));
          pb[u] = pk_fma4(bg, w4[u], pk_fma4(ag, s4[u], pb[u]));
        }
      }
    }
  }
  for (int j = 0; j < (staged ? 0 : nh); j += E) {  // (the register path)
    const int ne = min(E, nh - j);  // uniform
    f4v s4[E][GT], w4[E][GT];
    float dd[4 * E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
#pragma unroll
      for (int u = 0; u < GT; ++u) {
        const int q = tid + u * BLOCK;
        if (u < GT - 1 && (E == 1 || e < ne)) {  // groups 0 .. GT-2 lie inside the row for every thread
          s4[e][u] = *reinterpret_cast<const f4v*>(S + (size_t)(j + e) * RSd + 4 * q);
          w4[e][u] = *reinterpret_cast<const f4v*>(W + (size_t)(j + e) * RSd + 4 * q);
          continue;
        }
        s4[e][u] = w4[e][u] = z;
        if (e < ne && q < G) {
          s4[e][u] = *reinterpret_cast<const f4v*>(S + (size_t)(j + e) * RSd + 4 * q);
          w4[e][u] = *reinterpret_cast<const f4v*>(W + (size_t)(j + e) * RSd + 4 * q);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      f2v sy2 = {0.f, 0.f}, wy2 = {0.f, 0.f}, sg2 = {0.f, 0.f}, wg2 = {0.f, 0.f};
#pragma unroll
      for (int u = 0; u < GT; ++u) {
        sy2 = pk_fma(s4[e][u].lo, y[u].lo, sy2); sy2 = pk_fma(s4[e][u].hi, y[u].hi, sy2);
        wy2 = pk_fma(w4[e][u].lo, y[u].lo, wy2); wy2 = pk_fma(w4[e][u].hi, y[u].hi, wy2);
        sg2 = pk_fma(s4[e][u].lo, gg[u].lo, sg2); sg2 = pk_fma(s4[e][u].hi, gg[u].hi, sg2);
        wg2 = pk_fma(w4[e][u].lo, gg[u].lo, wg2); wg2 = pk_fma(w4[e][u].hi, gg[u].hi, wg2);
      }
      dd[4 * e] = sy2.x + sy2.y;
      dd[4 * e + 1] = wy2.x + wy2.y;
      dd[4 * e + 2] = sg2.x + sg2.y;
      dd[4 * e + 3] = wg2.x + wg2.y;
    }
    block_sum<4 * E, NW>(dd, scratch, buf);
    buf ^= 1;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (e < ne) {
        const float rho = hrho[j + e], cr = hc[j + e] * rho;
        const float ay = fmaf(cr, dd[4 * e], -(rho * dd[4 * e + 1])), by = -rho * dd[4 * e];
        const float ag = fmaf(cr, dd[4 * e + 2], -(rho * dd[4 * e + 3])), bg = -rho * dd[4 * e + 2];
#pragma unroll
        for (int u = 0; u < GT; ++u) {
          pa[u] = pk_fma4(by, w4[e][u], pk_fma4(ay, s4[e][u], pa[u]));
          pb[u] = pk_fma4(bg, w4[e][u], pk_fma4(ag, s4[e][u], pb[u]));
        }
      }
    }
  }
  // H'y, H'g in registers; s_{k-1}; the curvature dots (s.y, H'y.y, s.g, H'y.g)
  f4v sv[GT];
  float r[4] = {0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < GT; ++u) {
    const int q = tid + u * BLOCK;
    const f4v yu = y[u], gu = gg[u];
    pa[u] += gamma0 * yu;
    pb[u] += gamma0 * gu;
    sv[u] = q < G ? *reinterpret_cast<const f4v*>(s_cur + 4 * q) : z;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[0] += sv[u][e] * yu[e]; r[1] += pa[u][e] * yu[e];
      r[2] += sv[u][e] * gu[e]; r[3] += pa[u][e] * gu[e];
    }
  }
  block_sum<4, NW>(r, scratch, buf);
  buf ^= 1;
  const float rho = r[0] <= 0.f ? 0.f : 1.0f / r[0];  // inverse_curvature (func_inverse_curvature.py:24-28)
  const float c = 1.0f + rho * r[1];
  const float sg = r[2], hyg = r[3];
  const float rsg = rho * sg;
  float dg = 0.f;
#pragma unroll
  for (int u = 0; u < GT; ++u) {
    const int q = tid + u * BLOCK;
    if (q < G) {
      const f4v gu = gg[u];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * q + e;
        if (i < P) {
          const float sri = sv[u][e] * rho;
          const float di = -1.0f * (pb[u][e] + sri * (c * sg) - sri * hyg - pa[u][e] * rsg);
          d[i] = di;
          dg += di * gu[e];
        } else if constexpr (staged) {
          // the staged copies filled whole groups of d's slot with the last entry's W-row pads: the
          // pads [P, Pv) of d are zero again before the objective reads x + alpha d in float4 groups
          d[i] = 0.f;
        }
      }
      *reinterpret_cast<f4v*>(s_row + 4 * q) = sv[u];  // history entry `entry` = (s, H'y, rho, c)
      *reinterpret_cast<f4v*>(w_row + 4 * q) = pa[u];
    }
  }
  if (tid == 0) {
    hrho[entry] = rho;
    hc[entry] = c;
    if (tape_rho) { *tape_rho = rho; *tape_c = c; }
  }
  return dg;
}

// COMPACT mode, single pass (P <= 1024, i.e. at most GM <= 4 float4 groups per lane):
// the coefficients of entry j depend only on entry j's own dots, so one wave
// loads the two rows of an entry into registers, reduces its 4 dots in-wave
// (no barrier), and immediately accumulates the entry's contribution to
// H y and H g -- every history row crosses HBM once per iteration.  Entries
// are dealt round-robin to the 4 waves; the per-wave partial sums are then
// added in a fixed tree ((w0 + w2) + (w1 + w3)) through 4 spare LDS vectors,
// so the result is deterministic.  a_out / b_out / spare0..3 are Pv-float LDS vectors.
// Entries j < lcap are read from the LDS-resident history LH (S row at LH + 2 j Pv, W row
// Pv floats later) -- the same values in the same per-wave order, so the result is
// bitwise the same as with every entry in HBM.
// Wave priorities (s_setprio): the two workgroups on a CU put one wave on each SIMD, and
// VALU issue between them goes by priority, then age.  A wave streaming its history (HBM-
// latency-bound, few VALU ops per byte) drops to 0 so the partner's objective evaluation or
// line-search step (VALU/LDS-latency-bound, the critical path) issues first: C3 +1.0%
// (interleaved A/B, profiles/r01c_ab_wave_priority.log; levels 1..3 within noise of
// each other).  Re-measured on the r04 kernel (profiles/r04_ab_c2_history.log): the drop still
// pays for the short rows of four problems per CU (C2: without it -2%) but no longer for C3's
// rows of four groups (without it +1.3%), so only rows of <= 2 groups per lane drop.
constexpr int kBasePrio = 2;
constexpr int kHistPrio = 0;
template <int GM>
constexpr bool kHistDropsPrio = GM <= 2;
// EF: history entries in flight per wave (each holds 2 GM float4 rows in registers).  More
// entries in flight = more bytes outstanding per wave, which is what the history stream of a
// problem with few waves (or few problems per CU) is bound by.  (Interleaved A/B,
// profiles/r02_ab_entries_in_flight.log: 3 / 5 for short rows and 3 for long rows are slower or
// within noise -- 3 costs C3 8%.)
// Rejected, r03: LDS-DMA staging of 1-3 more entries per wave by global_load_lds_dwordx4 (no VGPRs),
// in the LDS the resident entries use -- bitwise equal, but C2 -2..-5% and C1 (B = 8192) -3..-5%
// (profiles/r03_ab_c2_lds_dma_staging.log).  Rejected, r02: refilling each entry slot as soon as it
// is consumed (a register ring) -- at the 256-VGPR cap the spills (scratch ops 26 -> 201) cost C3 33%,
// C2 13% (profiles/r02_ab_history_ring.log).
template <int GM>
constexpr bool kBatchAllEntries = GM <= 2;  // compact_products_fused: on-chip entries in batches too
template <int GM>
__host__ __device__ constexpr int fused_inflight() {
  return GM <= 2 ? 4 : 2;  // rows of <= 2 float4 groups per lane (P <= 512: C1, C2) : 3-4 groups (C3)
}
template <int GM, int NW>
__device__ __forceinline__ void compact_products_fused(int P, int Pv, int nh, const float* __restrict__ S,
                                       const float* __restrict__ W, const float* LH, int lcap,
                                       const float* hrho, const float* hc,
                                       float gamma0, const float* g, const float* gp, float* a_out, float* b_out,
                                       float* spare0, float* spare1, float* spare2, float* spare3) {
  static_assert(NW == 1 || NW == 2 || NW == 4, "the cross-wave combine is written for 1, 2 or 4 waves");
  constexpr int EF = fused_inflight<GM>();
  const int lane = threadIdx.x & (kWave - 1);
  // the wave index as a scalar: the entry index j (and so each row's buffer descriptor) is then
  // provably wave-uniform; from threadIdx.x / 64 the compiler cannot tell, keeps the descriptor in
  // VGPRs and wraps every buffer load in a waterfall loop (readfirstlane x 4, compares, exec juggling)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int G = (P + 3) / 4;
  f4v pa[GM], pb[GM];
  bool ok[GM];
#pragma unroll
  for (int m = 0; m < GM; ++m) {
    // (exec-masked for every group: telling the compiler that groups 0 .. GM-2 are full -- they are,
    // GM = ceil(G / 64) -- dropped 14 instructions per 4-entry batch and cost C3 2.3%, C2 0.9%,
    // interleaved A/B profiles/r04_ab_full_groups_and_phase_scan.log)
    ok[m] = lane + kWave * m < G;
    pa[m] = f4v{0, 0, 0, 0};
    pb[m] = f4v{0, 0, 0, 0};
  }
  // y and g stay in LDS (re-read per entry: cheap ds_read_b128, saves 8 GM VGPRs)
  auto gvec = [&](int m) {
    const float4 t = ld4(g + 4 * (lane + kWave * m));
    return f4v{t.x, t.y, t.z, t.w};
  };
  auto yvec = [&](int m) {
    const int q = lane + kWave * m;
    const float4 t = ld4(g + 4 * q), u = ld4(gp + 4 * q);
    return f4v{t.x - u.x, t.y - u.y, t.z - u.z, t.w - u.w};
  };
  // One entry: its four dots with y and g (per lane: packed 2-wide FMA chains, v_pk_fma_f32),
  // one transposed wave reduction of the four (wave_sum4: uniform results), then the entry's
  // contribution to H y and H g as packed FMAs.  ~90 VALU ops per entry at GM = 4 (the round-1
  // form, per-element products + one wave_sum per dot: ~210).
  auto consume = [&](int j, const f4v (&s4)[GM], const f4v (&w4)[GM]) {
    f2v sy2 = {0.f, 0.f}, wy2 = {0.f, 0.f}, sg2 = {0.f, 0.f}, wg2 = {0.f, 0.f};
#pragma unroll
    for (int m = 0; m < GM; ++m) {
      const f4v y = yvec(m), gm = gvec(m);
      sy2 = pk_fma(s4[m].lo, y.lo, sy2); sy2 = pk_fma(s4[m].hi, y.hi, sy2);
      wy2 = pk_fma(w4[m].lo, y.lo, wy2); wy2 = pk_fma(w4[m].hi, y.hi, wy2);
      sg2 = pk_fma(s4[m].lo, gm.lo, sg2); sg2 = pk_fma(s4[m].hi, gm.hi, sg2);
      wg2 = pk_fma(w4[m].lo, gm.lo, wg2); wg2 = pk_fma(w4[m].hi, gm.hi, wg2);
    }
    const float4 t = wave_sum4(sy2.x + sy2.y, wy2.x + wy2.y, sg2.x + sg2.y, wg2.x + wg2.y);
    const float sy = t.x, wy = t.y, sg = t.z, wg = t.w;
    // coefficients with the FMA written out: both call sites (LDS- and HBM-resident entries) must
    // round them identically, and left to itself the compiler contracted cr sy - rho wy into an
    // FMA at one site and not the other (hip's __fmul_rn / __fsub_rn do not stop contraction)
    const float rho = hrho[j], cr = hc[j] * rho;
    const float ay = fmaf(cr, sy, -(rho * wy)), by = -rho * sy;
    const float ag = fmaf(cr, sg, -(rho * wg)), bg = -rho * sg;
#pragma unroll
    for (int m = 0; m < GM; ++m) {
      pa[m] = pk_fma4(by, w4[m], pk_fma4(ay, s4[m], pa[m]));
      pb[m] = pk_fma4(bg, w4[m], pk_fma4(ag, s4[m], pb[m]));
    }
  };
  // buffer loads (rows of <= kFusedBufferLoadsGM groups per lane): a descriptor per row (range =
  // the row), lane offsets loop-invariant, the groups past P read zeros through the range check
  // instead of an exec-mask branch (bitwise equal)
  constexpr bool kBufferLoads = GM <= kFusedBufferLoadsGM;
  const float* Su = uniform_ptr(S);
  const float* Wu = uniform_ptr(W);
  auto load = [&](int j, f4v (&s4)[GM], f4v (&w4)[GM]) {
    if constexpr (kBufferLoads) {
      const auto rs = make_rsrc(Su + (size_t)j * Pv, 4 * Pv);
      const auto rw = make_rsrc(Wu + (size_t)j * Pv, 4 * Pv);
#pragma unroll
      for (int m = 0; m < GM; ++m) {
        s4[m] = buf_ld4(rs, 16 * (lane + kWave * m));
        w4[m] = buf_ld4(rw, 16 * (lane + kWave * m));
      }
    } else {
      const float* sr = S + (size_t)j * Pv;
      const float* wr = W + (size_t)j * Pv;
#pragma unroll
      for (int m = 0; m < GM; ++m) {
        const int q = lane + kWave * m;
        s4[m] = ok[m] ? *reinterpret_cast<const f4v*>(sr + 4 * q) : f4v{0, 0, 0, 0};
        w4[m] = ok[m] ? *reinterpret_cast<const f4v*>(wr + 4 * q) : f4v{0, 0, 0, 0};
      }
    }
  };
  if constexpr (kHistDropsPrio<GM>) __builtin_amdgcn_s_setprio(kHistPrio);
  int j = wave;
  if constexpr (kBatchAllEntries<GM>) {
  // Rows of <= 2 groups (C1, C2): the on-chip entries and the HBM remainder go through batches too (up to
  // EF entries loaded, then consumed in order), so their consume chains (dots, wave reduction,
  // coefficients, accumulation) interleave instead of running one entry at a time.  Same entries in the
  // same order: bitwise the one-at-a-time form (profiles/r05_ab_batch_serial.log: 1024 / 1024 C2 and
  // 2048 / 2048 C3 rows equal; C1 shape +1.2%, C2 at B = 256 +1.1%, C2 at B = 1024 +-0; rows of 4 groups,
  // C3: -0.7%, so they keep the one-at-a-time form).
  auto lds_load = [&](int jj, f4v (&s4)[GM], f4v (&w4)[GM]) {
    const float* sr = LH + (size_t)2 * jj * Pv;
    const float* wr = sr + Pv;
#pragma unroll
    for (int m = 0; m < GM; ++m) {
      const int q = lane + kWave * m;
      s4[m] = ok[m] ? *reinterpret_cast<const f4v*>(sr + 4 * q) : f4v{0, 0, 0, 0};
      w4[m] = ok[m] ? *reinterpret_cast<const f4v*>(wr + 4 * q) : f4v{0, 0, 0, 0};
    }
  };
  auto batch = [&](auto count, int jj, auto&& loader) {
    constexpr int C = decltype(count)::value;
    f4v s[C][GM], w[C][GM];
#pragma unroll
    for (int e = 0; e < C; ++e) loader(jj + e * NW, s[e], w[e]);
#pragma unroll
    for (int e = 0; e < C; ++e) consume(jj + e * NW, s[e], w[e]);
  };
  auto batch_of = [&](int cnt, int jj, auto&& loader) {  // cnt: 1 .. EF, wave-uniform
    if (cnt >= 4 && EF >= 4) batch(std::integral_constant<int, (EF >= 4 ? 4 : 1)>{}, jj, loader);
    else if (cnt == 3 && EF >= 3) batch(std::integral_constant<int, (EF >= 3 ? 3 : 1)>{}, jj, loader);
    else if (cnt >= 2) batch(std::integral_constant<int, 2>{}, jj, loader);
    else batch(std::integral_constant<int, 1>{}, jj, loader);
  };
  for (const int nl = min(lcap, nh); j < nl;) {
    const int cnt = min(EF, (nl - j + NW - 1) / NW);
    batch_of(cnt, j, lds_load);
    j += cnt * NW;
  }
  for (; j + (EF - 1) * NW < nh; j += EF * NW) batch(std::integral_constant<int, EF>{}, j, load);
  if (j < nh) batch_of((nh - j + NW - 1) / NW, j, load);
  } else {
  // on-chip entries first (wave-uniform).  (Rejected, r05, profiles/r05_ab_c2_stagger_prefetch.log,
  // profiles/r05_ab_c3_prefetch.log: issuing the first HBM batch before consuming these, so its latency
  // runs under them -- bitwise the same sums, C2 +0.1%, C3 -0.5%, 26 VGPRs spilled.)
  for (const int nl = min(lcap, nh); j < nl; j += NW) {
    f4v s0[GM], w0[GM];
    const float* sr = LH + (size_t)2 * j * Pv;
    const float* wr = sr + Pv;
#pragma unroll
    for (int m = 0; m < GM; ++m) {
      const int q = lane + kWave * m;
      s0[m] = ok[m] ? *reinterpret_cast<const f4v*>(sr + 4 * q) : f4v{0, 0, 0, 0};
      w0[m] = ok[m] ? *reinterpret_cast<const f4v*>(wr + 4 * q) : f4v{0, 0, 0, 0};
    }
    consume(j, s0, w0);
  }
  // EF entries of this wave in flight: all loads issued before any is consumed.  (Rejected, r04,
  // profiles/r04_ab_variants_c2.log: two register batches, the next batch's loads issued before this
  // one is consumed -- C2 -2..-8%.)
  for (; j + (EF - 1) * NW < nh; j += EF * NW) {
    f4v s[EF][GM], w[EF][GM];
#pragma unroll
    for (int e = 0; e < EF; ++e) load(j + e * NW, s[e], w[e]);
#pragma unroll
    for (int e = 0; e < EF; ++e) consume(j + e * NW, s[e], w[e]);
  }
  for (; j < nh; j += NW) {  // the rest, one entry in flight
    f4v s0[GM], w0[GM];
    load(j, s0, w0);
    consume(j, s0, w0);
  }
  }
  if constexpr (kHistDropsPrio<GM>) __builtin_amdgcn_s_setprio(kBasePrio);
  // deterministic cross-wave sum: ((w0 + w2) + (w1 + w3)) + gamma0 * (y | g)  (NW = 4),
  // (w0 + w1) + gamma0 * (y | g)  (NW = 2), w0 + gamma0 * (y | g)  (NW = 1).  With NW > 1 the last
  // adds are left to the caller's block-wide pass after its barrier (same operations, same order):
  // (w0 + w2) | w0 in spare0/1 and (w1 + w3) | w1 in spare2/3.
  auto put = [&](float* A, float* B) {
#pragma unroll
    for (int m = 0; m < GM; ++m)
      if (ok[m]) {
        const int q = lane + kWave * m;
        *reinterpret_cast<f4v*>(A + 4 * q) = pa[m];
        *reinterpret_cast<f4v*>(B + 4 * q) = pb[m];
      }
  };
  auto add = [&](const float* A, const float* B) {
#pragma unroll
    for (int m = 0; m < GM; ++m)
      if (ok[m]) {
        const int q = lane + kWave * m;
        pa[m] += *reinterpret_cast<const f4v*>(A + 4 * q);
        pb[m] += *reinterpret_cast<const f4v*>(B + 4 * q);
      }
  };
  if constexpr (NW == 1) {  // + gamma0 (y | g), into the outputs
#pragma unroll
    for (int m = 0; m < GM; ++m)
      if (ok[m]) {
        pa[m] += gamma0 * yvec(m);
        pb[m] += gamma0 * gvec(m);
      }
    put(a_out, b_out);
    return;
  }
  if constexpr (NW == 2) {
    if (wave == 0) put(spare0, spare1);
    if (wave == 1) put(spare2, spare3);
    return;
  }
  if (wave == 2) put(spare0, spare1);
  if (wave == 3) put(spare2, spare3);
  __syncthreads();
  if (wave == 0) { add(spare0, spare1); put(spare0, spare1); }
  if (wave == 1) { add(spare2, spare3); put(spare2, spare3); }
}

}  // namespace dava
