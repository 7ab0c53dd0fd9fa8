// Fused eval-mode BFGS + strong-Wolfe bundle-adjustment solve on gfx950.
//
// Replaces, for the squared reprojection objective:
//   BFGSSolver.forward                      autograd_solvers/bfgs_solver.py:80-215
//   BFGSSolver.scale_initial_inverse_hessian bfgs_solver.py:217-233
//   BFGSSolver.update_inverse_hessian        bfgs_solver.py:235-303
//   line_search_wolfe_conditions(strong=True) autograd_solvers/line_search/wolfe_conditions.py:23-239
//
// Design (DESIGN.md has the numbers):
//  * one problem per 256-thread workgroup for the WHOLE solve: every host sync
//    of the reference (bfgs_solver.py:144,206, wolfe_conditions.py:120) and
//    every boolean-mask gather/scatter disappears; problems that stop early
//    just retire their workgroup.
//  * all O(P) state (x, g, g_prev, d, s, H y, H g, pending update) and the
//    scene (obs, vis) live in LDS; the only HBM stream is the inverse Hessian.
//  * DENSE mode keeps the reference's dense P x P fp32 inverse Hessian per
//    problem in HBM, with the rank-2 update DEFERRED: iteration k reads
//    H_{k-2}, applies U_{k-1} on the fly, writes H_{k-1} back and in the same
//    sweep forms H_{k-1} y and H_{k-1} g (column sums: lane = column, so no
//    cross-lane reduction).  H_k g then follows algebraically from the rank-2
//    terms, so each BFGS iteration costs exactly one read + one write of H
//    (8 P^2 bytes), the minimum for a materialised dense H.  H_0 = gamma I is
//    never stored (the first sweep synthesises it).
//  * the line search runs in-kernel; trial slopes come from forward-mode
//    (JVP) derivatives, gradients at accepted points from reverse mode.
#include <algorithm>
#include <cstring>
#include <vector>


#include "ba_objective.hpp"
#include "dava_debug.hpp"
#include "dava_tape.hpp"
#include "solve_passes.hpp"

namespace dava {

struct SolveArgs {
  Layout L;
  int B, Pv, Pld;
  const float* obs;
  const uint8_t* vis;
  const float* x0;
  float* x_out;
  float* err_out;
  int32_t* status;
  float* hess;
  float* hess_dense;  // HYBRID: B x P x Pld dense matrices after the histories (else null)
  float c1, c2, thr, min_step;
  int iters, max_trials, strong, mode;
  int kcap;       // COMPACT: history capacity (entries)
  int lcap;       // COMPACT, LDS mode: entries 0 .. lcap-1 live in LDS instead of HBM
  float* vecs;    // GV mode: B slices of vstride floats (kVectors x Pv, then rho_j / c_j if scal_slice)
  int vstride;
  int scal_slice;  // GV, wide pass: rho_j, c_j in the workspace slice instead of LDS
  int kcap_lds;    // history entries whose rho_j, c_j (and product coefficients) the LDS image holds
  unsigned long long* phase_cycles;  // DAVA_PHASE_TIMING builds: B x kPhases (else null)
  int* queue;     // work-queue counter (zeroed before the launch), or null: problem = blockIdx.x
  // recording solve (dava_ba_solve_record, dava_tape.hpp): x_k and g_k rows, (alpha, rho, c, gamma)
  float* tape_x;  // (B, K, Pv) or null
  float* tape_g;  // (B, K, Pv)
  float* tape_s;  // (B, tape_T)
  int tape_T;
  int stagger;    // shader cycles per start level (0: none)
  int stagger_levels;  // <= 1: odd workgroups wait `stagger`; L > 1: level (b / 8) mod L waits level x stagger
  float drop_p;   // training-mode drop path probability (0: eval mode)
  unsigned long long drop_seed;
  int second_last;  // training mode's return_second_last: a minimum-step stop keeps x_k
};

// (Training mode's drop path draws drop_uniform, dava_common.hpp.)
// Trial slopes phi'(alpha) of the full trials (the ones that also form the gradient): forward mode (a JVP
// riding on the trial's evaluation) in LDS mode, where the reverse-mode form d . grad measured -1% at C3
// (profiles/r01b_ab_variants.log, `dot`); d . grad in global-vector mode, where it saves the pair sweep's
// tangent registers (C5 +4%, r03 interleaved A/B).  In the kernel: kTrialDot = GV.
// Lean trials (r06): a line search's trials from index kLeanFrom on are evaluated for E and the forward-mode
// slope alone -- all the Wolfe tests read (wolfe_conditions.py:116-237) -- without the reverse-mode gradient.
// If the accepted trial was lean, it is evaluated once more in the full trial form (below), so x_{k+1}'s
// objective and gradient are bit for bit what the full-trial path keeps.  The first trials (alpha = 1, accepted
// ~89% of the time at C3) stay full.  DAVA_LEAN_TRIALS (LDS mode) / DAVA_LEAN_TRIALS_GV: the first trial index
// evaluated lean, 0 = none.  LDS mode from the third trial: a search of two trials (reject, accept) would pay
// the lean trial and its full re-evaluation; interleaved A/B (profiles/r06f_lean_index_dot_gvlean_ab.log):
// from the 2nd / 3rd / 4th trial C2 0.514 / 0.514 / 0.505, C2 ray-angle 0.683 / 0.691 / 0.695, C3 0.895 for all
// (no lean trials: C2 0.46).  GV mode keeps full trials: lean from the 2nd / 3rd trial C5 -1.5% / -1.2% (its
// searches are short, and a lean trial's forward-mode tangents cost the packed sweep registers).  First
// trials with d . grad in LDS mode too: C3 -1.1%, C2 -0.5%, not kept.
#ifndef DAVA_LEAN_TRIALS
#define DAVA_LEAN_TRIALS 2
#endif
#ifndef DAVA_LEAN_TRIALS_GV
#define DAVA_LEAN_TRIALS_GV 0
#endif
constexpr int kLeanFromLds = DAVA_LEAN_TRIALS;
constexpr int kLeanFromGv = DAVA_LEAN_TRIALS_GV;
// Runs of known no-move zoom trials iterated as the scalar recurrence they are (r06; bitwise invisible).
#ifndef DAVA_NOMOVE_RUNS
#define DAVA_NOMOVE_RUNS 1
#endif
constexpr bool kNoMoveRuns = DAVA_NOMOVE_RUNS != 0;
// Diagnostic builds only (make variant FLAGS=-DDAVA_PHASE_TIMING=1): thread 0 of every
// workgroup accumulates shader-clock cycles per solver phase; dava_ba_solve prints the
// batch averages to stderr after the launch (and synchronises -- never in a product build).
#ifndef DAVA_PHASE_TIMING
#define DAVA_PHASE_TIMING 0
#endif
#if DAVA_PHASE_TIMING
constexpr int kPhases = 7;  // eval at x, history products, direction, trial evals, search logic, step, total
#define DAVA_PHASE(i)                          \
  do {                                         \
    const unsigned long long t1_ = clock64(); \
    ph_acc[i] += t1_ - ph_t0;                  \
    ph_t0 = t1_;                               \
  } while (0)
#else
#define DAVA_PHASE(i) \
  do {                \
  } while (0)
#endif

// XL: GV mode with x, d and the objective's gradient in LDS.  PPT > 0: the objective keeps
// each thread's (<= PPT) points in registers across the view sweep (ba_eval).
// NW: waves per workgroup -- 8 in GV mode; 4 (default) or 2 in LDS mode (two-wave workgroups put
// twice as many small problems on a CU at once, DESIGN.md 3.1 Launch).
// SLICE: the GV wide pass's rho_j, c_j in the workspace slice (gv_scalar_stride), a kernel of its own:
// chosen at run time inside one kernel, the two forms cost both 1-10% to register allocation
// (profiles/r05_ab_c5_scalar_slice.log).  (The LDS image's scalar capacity stays a run-time argument,
// kcap_lds: with the constant 0 in the SLICE kernels this compiler rejects the kernel with an illegal
// V_CMP_NE_U32 on src_shared_base.)
template <int MODE, bool GV, int RES, bool XL, int PPT, int NW, bool SLICE = false>
__global__ __launch_bounds__(kWave * NW, kSolveWavesPerEU) void bfgs_ba_solve_kernel(SolveArgs a) {
  static_assert(!XL || GV, "XL is a global-vector-mode variant");
  static_assert(!SLICE || (GV && MODE != DAVA_HESSIAN_DENSE), "SLICE is a global-vector history variant");
  static_assert(GV ? NW == solve_waves(true) : (NW == 1 || NW == 2 || NW == 4), "LDS mode runs 1-, 2- or 4-wave workgroups");
  constexpr int BLOCK = kWave * NW;
  constexpr bool kTrialDot = GV;  // full trials' slope as d . grad (above)
  constexpr int kLeanFrom = GV ? kLeanFromGv : kLeanFromLds;
  constexpr bool kLean = kLeanFrom > 0;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __builtin_amdgcn_s_setprio(kBasePrio);
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N;
  const int Pv = a.Pv;
  const int tid = threadIdx.x;
  // Work queue (a.queue != null): the grid holds as many workgroups as are resident at once and
  // each takes the next problem when it finishes one, so a problem that stops early or runs a
  // long line search never leaves its slot idle.  Without a queue: problem = blockIdx.x.
  __shared__ int queued_problem;
  // Staggered start (a.stagger > 0: every problem of the launch is resident at once): the odd
  // workgroups -- dealt round-robin, so the odd XCDs -- start a.stagger shader cycles (~8 us) late.
  // Problems that start together stay in phase for the whole solve, so every CU streams history
  // rows at the same time (HBM-bound) and evaluates the objective at the same time (VALU-bound);
  // offsetting half the chip by part of an iteration lets one half's stream run while the other
  // half evaluates.  C2 (B = 1024): +6% on two boxes, +0.4% on a third; C3 (16 problems per slot)
  // gets no stagger
  // (profiles/r02_ab_stagger.log).  Results are unchanged (timing only).
  // Spread start (a.stagger_levels = L > 1; GV launches, one long problem per CU): within each XCD
  // (workgroups are dealt round-robin, so b / 8 numbers them inside their XCD) the problems start at
  // L evenly spaced offsets.  Every problem alternates an HBM-bound history stream with a VALU-bound
  // objective evaluation; started together, all CUs stream at once and then all compute at once.
  // (Rejected, r05, profiles/r05_ab_c2_stagger_prefetch.log: levels by (b >> 8) mod L, i.e. the
  // problems sharing one CU started a quarter or half of an iteration apart -- C2 within +-1%.)
  const int level = a.stagger_levels > 1 ? (int)((blockIdx.x >> 3) % (unsigned)a.stagger_levels) : (blockIdx.x & 1);
  if (a.stagger > 0 && level > 0) {
    const unsigned long long t0 = clock64();
    const unsigned long long wait = (unsigned long long)a.stagger * (unsigned long long)level;
    while (clock64() - t0 < wait) __builtin_amdgcn_s_sleep(8);
  }
  for (int b = blockIdx.x;;) {
    if (a.queue) {
      __syncthreads();  // every thread is done with the previous problem's LDS image
      if (tid == 0) queued_problem = atomicAdd(a.queue, 1);
      __syncthreads();
      b = queued_problem;
      if (b >= a.B) break;
    }
    constexpr bool kHistory = MODE != DAVA_HESSIAN_DENSE;  // COMPACT, or HYBRID's compact phase
    const int lcap = kHistory && !GV ? a.lcap : 0;
    constexpr bool gvs = SLICE;  // rho_j, c_j in the workspace slice
    const LdsCarve cv = carve_lds(M, N, Pv, kHistory ? a.kcap_lds : 0, GV, lcap, XL, NW);
    float* LH = lds + cv.hist;  // LDS-resident history entries 0 .. lcap-1
    float* vb0 = GV ? a.vecs + (size_t)b * a.vstride : lds;
    float* x = (GV && !XL ? vb0 : lds) + cv.x;
    float* d = (GV && !XL ? vb0 : lds) + cv.d;
    float* ge = lds + cv.ge;  // XL: the objective's gradient output, copied to g / gp after each evaluation
    // the objective's gradient target and its publication to the workspace vector `dst`
    auto grad_buf = [&](float* dst) { return XL ? ge : dst; };
    auto publish = [&](float* dst) {
      if constexpr (XL) {
        for (int i = tid; i < P; i += BLOCK) dst[i] = ge[i];
        __syncthreads();
      }
    };
    float* g = vb0 + cv.g0;
    float* gp = vb0 + cv.g1;
    float* hcoef = lds + cv.hcoef;
    float* hrho = gvs ? vb0 + kVectors * Pv : lds + cv.hrho;
    float* hc = gvs ? hrho + gv_scalar_stride(a.kcap) : lds + cv.hc;
    float* s_cur = vb0 + cv.s0;
    float* s_pend = vb0 + cv.s1;
    float* hy_new = vb0 + cv.hy0;
    float* hy_pend = vb0 + cv.hy1;
    float* hg = vb0 + cv.hg;
    float* views = lds + cv.views;
    float* vpart = lds + cv.vpart;
    float* scratch = lds + cv.scratch;
    const int MN = M * N;
    const float* obs = GV ? a.obs + (size_t)b * 2 * MN : lds + cv.obs;
    const uint8_t* vis = GV ? a.vis + (size_t)b * MN : reinterpret_cast<uint8_t*>(lds) + cv.vis_bytes_off;

    // ---- stage the problem into LDS (zero the vector pads) ----
    const float* x0 = a.x0 + (size_t)b * P;
    for (int i = tid; i < Pv; i += BLOCK) {
      x[i] = i < P ? x0[i] : 0.f;
      d[i] = g[i] = gp[i] = s_cur[i] = s_pend[i] = hy_new[i] = hy_pend[i] = hg[i] = 0.f;
    }
    if (!GV) {
      float* o = lds + cv.obs;
      uint8_t* v = reinterpret_cast<uint8_t*>(lds) + cv.vis_bytes_off;
      const float* ob = a.obs + (size_t)b * 2 * MN;
      for (int i = tid; i < 2 * MN; i += BLOCK) o[i] = ob[i];
      const uint8_t* vbb = a.vis + (size_t)b * MN;
      for (int i = tid; i < MN; i += BLOCK) v[i] = vbb[i] ? 1 : 0;
    }
    __syncthreads();

    float* H = nullptr;   // DENSE (and HYBRID's dense phase): this problem's P x Pld inverse Hessian
    float* SH = nullptr;  // COMPACT: history rows S[kcap][Pv], W[kcap][Pv]
    float* WH = nullptr;
    if (MODE == DAVA_HESSIAN_DENSE) {
      H = a.hess ? a.hess + (size_t)b * P * a.Pld : nullptr;
    } else if (a.hess) {
      SH = a.hess + (size_t)b * 2 * a.kcap * Pv;
      WH = SH + (size_t)a.kcap * Pv;
      if (MODE == kHybrid) H = a.hess_dense + (size_t)b * P * a.Pld;
    }
    int buf = 0;
    bool materialized = false;
    float gamma0 = 1.f, pend_rho = 0.f, pend_c = 1.f;
    int steps = 0, reason = DAVA_STOP_ITERATIONS, evals = 0, trials = 0;
    float E = 0.f, unused = 0.f;

    // When the line search accepts the step it evaluated last, that trial (which also
    // formed the full gradient) IS the evaluation at x_{k+1} = x_k + alpha d: same point,
    // bit for bit, so the next iteration's objective + gradient are taken from it.
    bool have_next = false;
    float E_next = 0.f;
  #if DAVA_PHASE_TIMING
    unsigned long long ph_acc[kPhases] = {0, 0, 0, 0, 0, 0, 0};
    const unsigned long long ph_start = clock64();
    unsigned long long ph_t0 = ph_start;
  #endif
    // training mode: the drop path stops this problem at the top of iteration kend (a.iters: never).
    // Drawn once here and used as the loop's bound, so the solve loop carries nothing extra (a
    // per-iteration test cost C3 6% through register allocation, profiles/r02_ab_drop_check.log).
    int kend = a.iters;
    if (a.drop_p > 0.f) {
      kend = 0;
      while (kend < a.iters && drop_uniform(a.drop_seed, b, kend) > a.drop_p) ++kend;
    }
    int k = 0;
    for (; k < kend; ++k) {
      { float* t = g; g = gp; gp = t; }  // gp <- previous gradient; g <- (trial) gradient buffer
      if (a.tape_x) {  // recording: x_k (the same threads wrote x[i] when the last step was taken)
        float* r = a.tape_x + ((size_t)b * a.iters + k) * Pv;
        for (int i = tid; i < Pv; i += BLOCK) r[i] = x[i];  // (pads are zero)
      }
      if (have_next) {
        E = E_next;
      } else {
        ba_eval<true, false, false, false, false, RES, float, NW, PPT, GV>(L, x, nullptr, 0.f, obs, vis, grad_buf(g), views, vpart,
                                                                  scratch, buf, E, unused);
        publish(g);
        ++evals;
      }
      DAVA_PHASE(0);
      if (a.tape_g) {  // recording: g_k
        float* r = a.tape_g + ((size_t)b * a.iters + k) * Pv;
        for (int i = tid; i < Pv; i += BLOCK) r[i] = g[i];
      }
      if (!(E > a.thr)) { reason = DAVA_STOP_ERROR; break; }

      // phi'(0) = d . g is accumulated where d is formed (same per-thread order as a separate
      // pass over d); its block reduction below is also the barrier that publishes d
      float dg = 0.f;
      if (k == 0) {
        // first step: no inverse Hessian yet, d = -g (bfgs_solver.py:152-155)
        for (int i = tid; i < P; i += BLOCK) {
          const float di = -1.0f * g[i];
          d[i] = di;
          dg += di * g[i];
        }
      } else {
        float r[4] = {0, 0, 0, 0};
        float rho = 0.f, c = 1.f, sg = 0.f, hyg = 0.f;
        bool deferred = false;  // the fused pass left its last cross-wave add to the pass below
        bool tail_done = false;  // GV: wide_direction formed d and appended the history entry itself
        if (k == 1) {
          // H_0 = gamma I, gamma from N&W eq. 6.20 (bfgs_solver.py:159-167, 217-233)
          for (int i = tid; i < P; i += BLOCK) {
            const float gi = g[i], yi = gi - gp[i], si = s_cur[i];
            r[0] += si * yi; r[1] += yi * yi; r[2] += si * gi; r[3] += yi * gi;
          }
          block_sum<4, NW>(r, scratch, buf); buf ^= 1;
          const float gamma = clamp_min(r[0] / clamp_min(r[1], 1e-5f), 1e-4f);
          gamma0 = gamma;
          if (a.tape_s && tid == 0) a.tape_s[(size_t)b * a.tape_T + 3 * a.iters] = gamma;
          rho = r[0] <= 0.f ? 0.f : 1.0f / r[0];
          c = 1.0f + rho * (gamma * r[1]);
          sg = r[2];
          hyg = gamma * r[3];
          for (int i = tid; i < P; i += BLOCK) {
            const float gi = g[i], yi = gi - gp[i];
            hy_new[i] = gamma * yi;
            hg[i] = gamma * gi;
          }
          // (no barrier needed: each thread reads back only its own hy_new / hg below)
        } else {
          if constexpr (MODE == DAVA_HESSIAN_DENSE) {
            dense_sweep<NW, GV>(L, a.Pld, H, materialized, gamma0, s_pend, hy_pend, pend_rho, pend_c, g, gp, hy_new, hg);
            materialized = true;
          } else if (MODE == kHybrid && k - 1 >= a.kcap) {
            // the history is full: fold it into H (once), then sweep H as DENSE does.  The fold is
            // H' itself, so this first sweep applies no pending update (zero rows, rho 0: exact).
            if (!materialized) {
              for (int i = tid; i < Pv; i += BLOCK) s_pend[i] = hy_pend[i] = 0.f;
              fold_history<NW>(P, Pv, a.Pld, a.kcap, SH, WH, LH, lcap, hrho, hc, gamma0, H);
              pend_rho = 0.f;
              pend_c = 1.f;
              __syncthreads();
            }
            dense_sweep<NW, GV>(L, a.Pld, H, true, gamma0, s_pend, hy_pend, pend_rho, pend_c, g, gp, hy_new, hg);
            materialized = true;
          } else {
            const int G4 = (P + 3) / 4;
            const int GM = (G4 + kWave - 1) / kWave;
            deferred = !GV && NW > 1 && GM <= 4;
            if constexpr (GV) {  // workgroup-wide single pass, else two passes
              const int GT = (G4 + kWave * NW - 1) / (kWave * NW);
              const int nh = k - 1;
              float* tr = a.tape_s ? a.tape_s + (size_t)b * a.tape_T + a.iters + k - 1 : nullptr;
              float* tcp = tr ? tr + a.iters : nullptr;
              float* srow = SH + (size_t)(k - 1) * Pv;
              float* wrow = WH + (size_t)(k - 1) * Pv;
              const bool fuse = wide_history_pass(Pv, a.kcap, GV) && k - 1 < a.kcap;
              if (fuse) {
                tail_done = true;
                if (GT <= 1) dg = wide_direction<1, NW, XL>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, s_cur, d, srow, wrow, scratch, buf, k - 1, tr, tcp, XL ? lds + cv.d : nullptr);
                else if (GT == 2) dg = wide_direction<2, NW, XL>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, s_cur, d, srow, wrow, scratch, buf, k - 1, tr, tcp, XL ? lds + cv.d : nullptr);
                else if (GT == 3) dg = wide_direction<3, NW, XL>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, s_cur, d, srow, wrow, scratch, buf, k - 1, tr, tcp, XL ? lds + cv.d : nullptr);
                else if (GT == 4) dg = wide_direction<4, NW, XL>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, s_cur, d, srow, wrow, scratch, buf, k - 1, tr, tcp, XL ? lds + cv.d : nullptr);
                else if (GT == 5) dg = wide_direction<5, NW, XL>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, s_cur, d, srow, wrow, scratch, buf, k - 1, tr, tcp, XL ? lds + cv.d : nullptr);
                else if (GT == 6) dg = wide_direction<6, NW, XL>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, s_cur, d, srow, wrow, scratch, buf, k - 1, tr, tcp, XL ? lds + cv.d : nullptr);
                else dg = wide_direction<7, NW, XL>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, s_cur, d, srow, wrow, scratch, buf, k - 1, tr, tcp, XL ? lds + cv.d : nullptr);
              } else if (!wide_history_pass(Pv, a.kcap, GV))
                compact_products<GV ? 8 : 1, NW>(P, Pv, nh, SH, WH, hcoef, hrho, hc, gamma0, g, gp, hy_new, hg);
              else if (GT <= 1) compact_products_wide<1, NW>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, hy_new, hg, scratch, buf);
              else if (GT == 2) compact_products_wide<2, NW>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, hy_new, hg, scratch, buf);
              else if (GT == 3) compact_products_wide<3, NW>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, hy_new, hg, scratch, buf);
              else if (GT == 4) compact_products_wide<4, NW>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, hy_new, hg, scratch, buf);
              else if (GT == 5) compact_products_wide<5, NW>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, hy_new, hg, scratch, buf);
              else if (GT == 6) compact_products_wide<6, NW>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, hy_new, hg, scratch, buf);
              else compact_products_wide<7, NW>(P, Pv, nh, SH, WH, hrho, hc, gamma0, g, gp, hy_new, hg, scratch, buf);
            } else
            if (GM <= 1) compact_products_fused<1, NW>(P, Pv, k - 1, SH, WH, LH, lcap, hrho, hc, gamma0, g, gp, hy_new, hg, s_pend, hy_pend, d, hg);
            else if (GM == 2) compact_products_fused<2, NW>(P, Pv, k - 1, SH, WH, LH, lcap, hrho, hc, gamma0, g, gp, hy_new, hg, s_pend, hy_pend, d, hg);
            else if (GM == 3) compact_products_fused<3, NW>(P, Pv, k - 1, SH, WH, LH, lcap, hrho, hc, gamma0, g, gp, hy_new, hg, s_pend, hy_pend, d, hg);
            else if (GM == 4) compact_products_fused<4, NW>(P, Pv, k - 1, SH, WH, LH, lcap, hrho, hc, gamma0, g, gp, hy_new, hg, s_pend, hy_pend, d, hg);
            else
            // GV mode (very long rows, few resident waves): 8 column groups in flight per lane;
            // the LDS-mode kernel keeps the lean loop (its register budget is the fused pass's)
            compact_products<GV ? 8 : 1, NW>(P, Pv, k - 1, SH, WH, hcoef, hrho, hc, gamma0, g, gp, hy_new, hg);
          }
          if (!tail_done) {
          __syncthreads();
          DAVA_PHASE(1);
          if (deferred) {  // finish the fused pass's cross-wave sum here, all threads at once
            for (int i = tid; i < P; i += BLOCK) {
              const float gi = g[i], yi = gi - gp[i], si = s_cur[i];
              float hi, gh;
              hi = s_pend[i] + d[i];
              gh = hy_pend[i] + hg[i];
              hi += gamma0 * yi;
              gh += gamma0 * gi;
              hy_new[i] = hi;
              hg[i] = gh;
              r[0] += si * yi; r[1] += hi * yi; r[2] += si * gi; r[3] += hi * gi;
            }
          } else
          for (int i = tid; i < P; i += BLOCK) {
            const float gi = g[i], yi = gi - gp[i], si = s_cur[i], hi = hy_new[i];
            r[0] += si * yi; r[1] += hi * yi; r[2] += si * gi; r[3] += hi * gi;
          }
          block_sum<4, NW>(r, scratch, buf); buf ^= 1;
          rho = r[0] <= 0.f ? 0.f : 1.0f / r[0];  // inverse_curvature (func_inverse_curvature.py:24-28)
          c = 1.0f + rho * r[1];
          sg = r[2];
          hyg = r[3];
          }
        }
        // d = -H_k g,  H_k = H' + c (rho s) s^T - (rho s) (H'y)^T - (H'y) (rho s)^T
        const float rsg = rho * sg;
        if (!tail_done)
        for (int i = tid; i < P; i += BLOCK) {
          const float sri = s_cur[i] * rho;
          const float di = -1.0f * (hg[i] + sri * (c * sg) - sri * hyg - hy_new[i] * rsg);
          d[i] = di;
          dg += di * g[i];
        }
        if (MODE == DAVA_HESSIAN_DENSE || (MODE == kHybrid && k - 1 >= a.kcap)) {
          // the new update becomes the pending one; recycle the old buffers
          { float* t = s_pend; s_pend = s_cur; s_cur = t; }
          { float* t = hy_pend; hy_pend = hy_new; hy_new = t; }
          pend_rho = rho;
          pend_c = c;
        } else if (k - 1 < a.kcap && !tail_done) {
          // append U_k = (s, H y, rho, c) to the history (entry k-1), on-chip if it is one of the first lcap
          if (k - 1 < lcap) {
            float* sr = LH + (size_t)2 * (k - 1) * Pv;
            for (int i = tid; i < Pv; i += BLOCK) { sr[i] = s_cur[i]; sr[Pv + i] = hy_new[i]; }
            if (a.tape_x) {  // recording: the tape keeps every entry (the reads stay on chip)
              float* tsr = SH + (size_t)(k - 1) * Pv;
              float* twr = WH + (size_t)(k - 1) * Pv;
              for (int i = tid; i < Pv; i += BLOCK) { tsr[i] = s_cur[i]; twr[i] = hy_new[i]; }
            }
          } else {
            float* sr = SH + (size_t)(k - 1) * Pv;
            float* wr = WH + (size_t)(k - 1) * Pv;
            for (int i = tid; i < Pv; i += BLOCK) { sr[i] = s_cur[i]; wr[i] = hy_new[i]; }
          }
          if (tid == 0) {
            hrho[k - 1] = rho;
            hc[k - 1] = c;
            if (a.tape_s) {
              a.tape_s[(size_t)b * a.tape_T + a.iters + k - 1] = rho;
              a.tape_s[(size_t)b * a.tape_T + 2 * a.iters + k - 1] = c;
            }
          }
        }
      }

      // ---- strong-Wolfe line search (wolfe_conditions.py:23-239) ----
      float dphi0;
      {
        float r[1] = {dg};
        block_sum<1, NW>(r, scratch, buf); buf ^= 1;
        dphi0 = r[0];
      }
      DAVA_PHASE(2);
      float a_lo = 0.f, a_hi = 0.f, al = 1.f, f_lo = E, f_hi = E, fa = E, dfa = dphi0;
      float last_al = 0.f, last_fa = 0.f;
      // Largest alpha seen whose trial point rounded back to x.  Rounding is monotone
      // (0 <= a' <= a => |fl(a' d_i)| <= |fl(a d_i)| and fl(x_i + .) stays x_i), so every smaller
      // trial is a no-move point too and needs neither evaluation nor the check: at fp32
      // stagnation a bisection towards 0 runs ~150 such trials per line search (C2's slowest
      // problems: thousands per solve).
      float nomove_al = -1.0f;
      bool widen = true, zoom = false, evaluated = false, last_same = false;
      bool last_grad = false;  // the last evaluated trial formed its gradient (reusable at x_{k+1})
      // trial gradients go into gp's buffer (g_prev is dead once d is formed)
      const float lim = (-a.c2) * dphi0;
      for (int t = 0; t < a.max_trials; ++t) {
        if (!(widen || zoom)) break;
        if (t > 0) {
          if (widen) { a_hi = al; f_hi = fa; al = 2.0f * al; }
          if (zoom) al = 0.5f * (a_lo + a_hi);
        }
        DAVA_PHASE(4);
        // Trial points that round back to x exactly (tiny alpha, e.g. bisecting an uphill
        // direction at fp32 stagnation) need no evaluation: the reference's closure would
        // return f(x) and, via autograd w.r.t. alpha, (d * g).sum() -- exactly f0 and
        // phi'(0).  The check rides on the objective's first reduction (CHECK).  Otherwise
        // E and the full gradient at the trial point are formed (kept for reuse as the
        // next iterate's gradient) and phi'(alpha) = d . grad (DOT) -- for the first trial;
        // later ones form E and phi'(alpha) only (kLean).
        const bool known_same = al <= nomove_al;  // uniform
        if (kNoMoveRuns && known_same && zoom && E >= f_lo) {
          // A run of known no-move trials in the zoom phase: each trial point is x itself (f = E, phi' =
          // phi'(0)), and with E >= f_lo every one fails the sufficient-decrease test, so a_hi <- alpha and
          // the next bisection point is tried.  That is a scalar recurrence: iterate it here, without the
          // trial machinery, until the interval closes, the next point needs an evaluation (above
          // nomove_al) or the trial budget ends -- the same states and counts as the general path below,
          // trial by trial (uniform; C2's slowest problems run thousands of these per solve).
          for (;;) {
            a_hi = al;
            f_hi = E;
            ++trials;
            if (a_lo == a_hi) { zoom = false; break; }
            if (t + 1 >= a.max_trials) break;
            const float nx = 0.5f * (a_lo + a_hi);
            if (!(nx <= nomove_al)) break;
            al = nx;
            ++t;
          }
          evaluated = true;
          last_same = true;
          last_al = al;
          last_fa = fa = E;
          dfa = dphi0;
          continue;
        }
        const bool lean = kLean && t >= kLeanFrom;  // uniform
        bool moved = false;
        if (!known_same) {
          if (lean)
            moved = ba_eval<false, true, true, false, true, RES, float, NW, PPT, GV>(
                L, x, d, al, obs, vis, nullptr, views, vpart, scratch, buf, fa, dfa);
          else
            moved = ba_eval<true, !kTrialDot, true, kTrialDot, true, RES, float, NW, PPT, GV>(
                L, x, d, al, obs, vis, grad_buf(gp), views, vpart, scratch, buf, fa, dfa);
        }
        if (moved) {
          ++evals;
          last_same = false;
          last_grad = !lean;
          if (kLean && lean && !(isfinite(fa) && isfinite(dfa))) {
            // overflowed lean trial: the rule below needs the reverse-mode gradient (rare): the full trial form
            ba_eval<true, !kTrialDot, true, kTrialDot, false, RES, float, NW, PPT, GV>(
                L, x, d, al, obs, vis, grad_buf(gp), views, vpart, scratch, buf, fa, dfa);
            ++evals;
            last_grad = true;
          }
          // Overflowed trial (fp32 at a wild step): the reference's phi'(alpha) is autograd w.r.t.
          // alpha, i.e. (grad E(x + alpha d) * d).sum() (wolfe_conditions.py:134-143) -- NaN as
          // soon as the reverse-mode gradient holds a NaN or infinities of both signs, where the
          // forward-mode tangent may come out as +-Inf.  The NaN-blind Wolfe comparisons branch on
          // that class (a -Inf slope passes `phi' (a_hi - a_lo) >= 0` when a_hi < a_lo, NaN does
          // not), so here the slope is re-formed from the trial's reverse-mode gradient.  Finite
          // trials keep the forward-mode slope bit for bit.  Uniform branch (fa, dfa are
          // block-reduced); ba_eval<GRAD> ends with a barrier, so the gradient is complete.
          if (!(isfinite(fa) && isfinite(dfa))) {
            const float* gt = grad_buf(gp);
            float r[1] = {0.f};
            for (int i = tid; i < P; i += BLOCK) r[0] += gt[i] * d[i];
            block_sum<1, NW>(r, scratch, buf); buf ^= 1;
            dfa = r[0];
          }
        } else {
          fa = E;
          dfa = dphi0;
          last_same = true;
          if (!known_same) nomove_al = al;
        }
        DAVA_PHASE(3);
        ++trials;
        evaluated = true;
        last_al = al;
        last_fa = fa;
        bool fail = fa > E + (a.c1 * al) * dphi0;
        if (zoom) fail = fail || (fa >= f_lo);
        if (t > 0 && widen) fail = fail || (fa >= f_hi);
        const bool curv = a.strong ? (fabsf(dfa) <= lim) : (-1.0f * dfa <= lim);
        const bool up = widen ? (dfa >= 0.f) : (dfa * (a_hi - a_lo) >= 0.f);
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
      const float alpha = a_hi;
      if (a.tape_s && tid == 0) a.tape_s[(size_t)b * a.tape_T + k] = alpha;
      if constexpr (kLean) {
        if (evaluated && last_al == alpha && !last_same && !last_grad) {  // uniform
          // The accepted trial was lean: evaluate it again in the full trial form (the same point, formed
          // the same way, the same instantiation as a first trial), so x_{k+1}'s objective and gradient are
          // bit for bit those the full-trial path keeps -- the trajectory does not depend on which trial of
          // the search was accepted.  Rejected trials (the zoom tails of C2's slowest problems) stay lean.
          float f2, s2;
          ba_eval<true, !kTrialDot, true, kTrialDot, true, RES, float, NW, PPT, GV>(
              L, x, d, alpha, obs, vis, grad_buf(gp), views, vpart, scratch, buf, f2, s2);
          ++evals;
          last_fa = f2;
          last_grad = true;
        }
      }
      have_next = evaluated && last_al == alpha && (last_same || last_grad);
      E_next = last_fa;
      if (have_next && last_same) {  // x_{k+1} == x_k bitwise: its gradient is g itself
        for (int i = tid; i < P; i += BLOCK) gp[i] = g[i];
      } else if (have_next) {
        publish(gp);  // XL: only the trial that is kept needs its gradient in the workspace
      }
      DAVA_PHASE(4);

      // ---- take the step (bfgs_solver.py:191-199) and test its length (:203-207) ----
      {
        float r[1] = {0.f};
        if (a.second_last) {  // x moves only once the step has passed the test (uniform branch)
          for (int i = tid; i < P; i += BLOCK) {
            const float si = __fmul_rn(alpha, d[i]);
            s_cur[i] = si;
            r[0] += si * si;
          }
        } else {
          for (int i = tid; i < P; i += BLOCK) {
            const float si = __fmul_rn(alpha, d[i]);
            s_cur[i] = si;
            x[i] = __fadd_rn(x[i], si);
            r[0] += si * si;
          }
        }
        block_sum<1, NW>(r, scratch, buf); buf ^= 1;
        ++steps;
        DAVA_PHASE(5);
        if (!(sqrtf(r[0]) > a.min_step)) { reason = DAVA_STOP_STEP; break; }
        if (a.second_last) {  // the same additions, after the test (bfgs_solver.py:208-212)
          for (int i = tid; i < P; i += BLOCK) x[i] = __fadd_rn(x[i], s_cur[i]);
          __syncthreads();
        }
      }
    }
    if (k == kend && kend < a.iters) reason = DAVA_STOP_DROP;  // uniform
  #if DAVA_PHASE_TIMING
    ph_acc[kPhases - 1] = clock64() - ph_start;
    if (tid == 0 && a.phase_cycles)
      for (int i = 0; i < kPhases; ++i) a.phase_cycles[(size_t)b * kPhases + i] = ph_acc[i];
  #endif

    // ---- outputs ----
    __syncthreads();
    float* xo = a.x_out + (size_t)b * P;
    for (int i = tid; i < P; i += BLOCK) xo[i] = x[i];
    if (a.err_out) {
      float e2 = 0.f;
      ba_eval<false, false, false, false, false, RES, float, NW, PPT, GV>(L, x, nullptr, 0.f, obs, vis, nullptr, views, vpart, scratch, buf,
                                                     e2, unused);
      if (tid == 0) a.err_out[b] = e2;
    }
    if (a.status && tid == 0) {
      int32_t* st = a.status + (size_t)b * DAVA_STATUS_WORDS;
      st[0] = steps; st[1] = reason; st[2] = evals; st[3] = trials;
    }
    if (!a.queue) break;
  }
}

// ---- single evaluation kernel (dava_ba_evaluate) ----
struct EvalArgs {
  Layout L;
  int Pv;
  const float* obs;
  const uint8_t* vis;
  const float* x;
  const float* dir;
  const float* alpha;
  float* err;
  float* grad;
  float* slope;
};

// The evaluation the solve runs per line-search trial, as one launch (dava_ba_evaluate), with the solve's
// own layout per mode so that it measures -- and, as the generic path's closure, runs -- the same sweep:
//   LDS mode (P fits on-chip): x, d, gradient, observations and visibility staged in LDS, NW = 4 waves,
//     PPT = 1 when every point has a thread (C1-C3: each thread's point in registers across the views);
//   GV + XL (C5: 8 waves, one problem per CU): x, d and the gradient in LDS (3 Pv floats), observations
//     and visibility read in place, the packed pair sweep (two points per step) -- the in-solve trial;
//   GV without XL (an image past the LDS): x, d and the gradient in place in HBM.
// (Before r05 the GV form ran 4 waves with the vectors in HBM: at C5 VALUBusy 40% and 4.2x the
// algorithmic bytes from the per-view read-modify-write of the point gradients, profiles/r05_eval_*.)
template <bool GRAD, bool SLOPE, bool TRIAL, bool GV, int RES, bool XL = false, int NW = kWaves, int PPT = 0>
__global__ __launch_bounds__(kWave * NW) void ba_evaluate_kernel(EvalArgs a) {
  static_assert(!XL || GV, "XL is a global-vector-mode variant");
  constexpr int BLOCK = kWave * NW;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Layout L = a.L;
  const int P = L.P, M = L.M, N = L.N, Pv = a.Pv;
  const int b = blockIdx.x, tid = threadIdx.x;
  const LdsCarve cv = carve_lds(M, N, Pv, 0, GV, 0, XL, NW);
  const int MN = M * N;
  float* views = lds + cv.views;
  float* vpart = lds + cv.vpart;
  float* scratch = lds + cv.scratch;
  const float* x;
  const float* d;
  float* g;
  const float* obs;
  const uint8_t* vis;
  if (GV && !XL) {  // an image past the LDS: work on the caller's buffers in place
    x = a.x + (size_t)b * P;
    d = a.dir ? a.dir + (size_t)b * P : nullptr;
    g = a.grad ? a.grad + (size_t)b * P : nullptr;
    obs = a.obs + (size_t)b * 2 * MN;
    vis = a.vis + (size_t)b * MN;
  } else {
    float* xl = lds + cv.x;
    float* dl = lds + cv.d;
    float* gl = lds + (XL ? cv.ge : cv.g0);
    for (int i = tid; i < Pv; i += BLOCK) {
      xl[i] = i < P ? a.x[(size_t)b * P + i] : 0.f;
      dl[i] = (a.dir && i < P) ? a.dir[(size_t)b * P + i] : 0.f;
      gl[i] = 0.f;
    }
    if constexpr (GV) {  // XL: the scene stays in HBM, read in place as the solve does
      obs = a.obs + (size_t)b * 2 * MN;
      vis = a.vis + (size_t)b * MN;
    } else {
      float* ol = lds + cv.obs;
      uint8_t* vl = reinterpret_cast<uint8_t*>(lds) + cv.vis_bytes_off;
      for (int i = tid; i < 2 * MN; i += BLOCK) ol[i] = a.obs[(size_t)b * 2 * MN + i];
      for (int i = tid; i < MN; i += BLOCK) vl[i] = a.vis[(size_t)b * MN + i] ? 1 : 0;
      obs = ol; vis = vl;
    }
    x = xl; d = dl; g = gl;
  }
  __syncthreads();
  const float al = (TRIAL && a.alpha) ? a.alpha[b] : 0.f;
  int buf = 0;
  float E = 0.f, sl = 0.f;
  ba_eval<GRAD, SLOPE, TRIAL, false, false, RES, float, NW, PPT, GV>(L, x, d, al, obs, vis, g, views, vpart, scratch,
                                                                     buf, E, sl);
  if (tid == 0) {
    a.err[b] = E;
    if (SLOPE && a.slope) a.slope[b] = sl;
  }
  if (GRAD && a.grad && (!GV || XL))
    for (int i = tid; i < P; i += BLOCK) a.grad[(size_t)b * P + i] = g[i];
}

}  // namespace dava

using namespace dava;

// ---- debug overrides (dava_debug.hpp): set only through the two calls below, never from the environment ----
namespace dava {
static long long g_debug_knobs[kDbgKnobs] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                                                 -1, -1};
static const char* const kDebugKnobNames[kDbgKnobs] = {
    "FORCE_GV", "GV_NO_XL", "SOLVE_WAVES", "WG_PER_CU", "LDS_HISTORY", "STAGGER", "STAGGER_LEVELS",
    "NO_PPT", "NO_QUEUE", "ADJ_GV_WAVES", "ADJ_FORCE_GV", "ADJ_LDS_ENTRIES", "ADJ_GD_HBM",
    "COMPACT_SWITCH", "GV_SCALAR_SLICE", "ADJ_SC_GLOBAL", "F64_FORM", "F32_DUAL_FORM",
    "L1_SOLVE_FORM"};
long long debug_knob(int k) { return k >= 0 && k < kDbgKnobs ? g_debug_knobs[k] : -1; }
}  // namespace dava

extern "C" int dava_debug_set_override(const char* name, int64_t value) {
  if (!name) return DAVA_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < kDbgKnobs; ++k)
    if (strcmp(name, kDebugKnobNames[k]) == 0) {
      g_debug_knobs[k] = value < 0 ? -1 : value;
      return DAVA_OK;
    }
  return DAVA_ERR_INVALID_ARGUMENT;
}

extern "C" void dava_debug_clear_overrides(void) {
  for (int k = 0; k < kDbgKnobs; ++k) g_debug_knobs[k] = -1;
}

extern "C" size_t dava_ba_solve_workspace_bytes(const DavaScene* scene, const DavaSolverConfig* config) {
  const SolvePlan p = plan_solve(scene, config, false);
  return p.sized ? p.state_bytes + kQueueBytes : 0;
}

extern "C" int dava_ba_solve_plan(const DavaScene* scene, const DavaSolverConfig* config, DavaSolvePlan* plan) {
  const SolvePlan p = plan_solve(scene, config, false);
  if (!p.sized) return p.status;
  if (!plan || config->iterations < 0) return DAVA_ERR_INVALID_ARGUMENT;
  plan->global_vectors = p.gv ? 1 : 0;
  plan->workgroup_threads = kWave * p.nw;
  plan->lds_bytes = p.lds_bytes;
  plan->lds_history_entries = p.lcap;
  return p.status;
}

extern "C" size_t dava_ba_solve_tape_bytes(const DavaScene* scene, const DavaSolverConfig* config) {
  const SolvePlan p = plan_solve(scene, config, false);
  return p.sized && p.tape_ok ? p.tape.total_bytes : 0;
}

constexpr int kStaggerCycles = 20000;  // ~8 us at the shader clock; one C2 iteration is ~47 us

template <int MODE, bool GV, int RES, bool XL, int PPT, int NW, bool SLICE = false>
static void launch_solve_ppt(const SolveArgs& a, int B, int lds, hipStream_t s) {
  const auto kernel = bfgs_ba_solve_kernel<MODE, GV, RES, XL, PPT, NW, SLICE>;
  constexpr int threads = kWave * NW;
  set_dynamic_lds(kernel, lds);
  int grid = B;
  SolveArgs args = a;
  int slots = 0;  // workgroups resident at once (host queries only; nothing synchronises)
  {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds) == hipSuccess && per_cu > 0 &&
        cus > 0)
      slots = per_cu * cus;
  }
  // stagger only a launch whose problems all run at once (one round, B <= slots)
  args.stagger = slots > 0 && B <= slots && B > 1 ? kStaggerCycles : 0;
  args.stagger_levels = 1;
  if (debug_knob(kDbgStagger) >= 0) args.stagger = (int)debug_knob(kDbgStagger);  // A/B (cycles)
  if (debug_knob(kDbgStaggerLevels) >= 1) args.stagger_levels = (int)debug_knob(kDbgStaggerLevels);
  if (args.queue) {  // one workgroup per resident slot
    if (slots > 0) grid = min(B, slots);
    // The hardware already refills a slot as soon as its workgroup retires, but only from its
    // own XCD's share of the grid (workgroups are dealt round-robin over the 8 XCDs): the
    // queue pays where per-problem work is uneven -- stopping rules active, or few problems
    // per slot so one long line search decides an XCD's finish (C2: +10%, C3 to convergence:
    // +4.5%).  With fixed K and >= 8 problems per slot (C3: 16) it measured -1%: plain grid.
    const bool fixed_k = !(args.thr >= 0.f) && !(args.min_step >= 0.f);
    if (grid == B || (fixed_k && B >= 8 * grid)) {
      args.queue = nullptr;
      grid = B;
    }
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, s, args);
}

// Points per thread held in registers by the objective: one for the LDS-mode kernels (C1-C3:
// N <= 256; C3 +12% over re-reading x, d and the gradient from LDS per view).  Larger N, GV
// mode and the kDbgNoPPT override take the re-reading variant: eight points per thread at C5 spill
// (1 KB of scratch per lane) and ran 42% slower.
// One-wave workgroups (one problem per wave) hold two points per lane (N <= 128).
template <bool GV, bool XL, int NW>
constexpr int kRegisterPoints = GV ? 0 : (NW == 1 ? 2 : 1);

template <int MODE, bool GV, int RES, bool XL, int NW, bool SLICE = false>
static void launch_solve_nw(const SolveArgs& a, int B, int lds, hipStream_t s) {
  constexpr int R = kRegisterPoints<GV, XL, NW>;
  if constexpr (SLICE)  // (GV: no points in registers)
    launch_solve_ppt<MODE, GV, RES, XL, 0, NW, SLICE>(a, B, lds, s);
  else if (R > 0 && a.L.N <= R * kWave * NW && !debug_flag(kDbgNoPPT))
    launch_solve_ppt<MODE, GV, RES, XL, R, NW>(a, B, lds, s);
  else
    launch_solve_ppt<MODE, GV, RES, XL, 0, NW>(a, B, lds, s);
}

template <int MODE, bool GV, int RES, bool XL, bool SLICE = false>
static void launch_solve_res(const SolveArgs& a, int B, int lds, hipStream_t s, int nw) {
  if constexpr (GV) launch_solve_nw<MODE, GV, RES, XL, solve_waves(true), SLICE>(a, B, lds, s);
  else if (nw == 1) launch_solve_nw<MODE, GV, RES, XL, 1>(a, B, lds, s);
  else if (nw == 2) launch_solve_nw<MODE, GV, RES, XL, 2>(a, B, lds, s);
  else launch_solve_nw<MODE, GV, RES, XL, 4>(a, B, lds, s);
}

template <int MODE, bool GV, bool XL = false, bool SLICE = false>
static void launch_solve(const SolveArgs& a, int B, int lds, hipStream_t s, int residual, int nw) {
  with_flag(residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
    constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
    launch_solve_res<MODE, GV, kRes, XL, SLICE>(a, B, lds, s, nw);
  });
}

// The kernel of a plan: MODE from plan.mode, then SLICE (history modes only), XL, GV or LDS mode.
template <int MODE>
static void launch_solve_mode(const SolveArgs& a, const SolvePlan& p, int residual, hipStream_t s) {
  if constexpr (MODE != DAVA_HESSIAN_DENSE) {
    if (p.xl && p.scal_slice) return launch_solve<MODE, true, true, true>(a, a.B, p.lds_bytes, s, residual, p.nw);
  }
  if (p.xl) launch_solve<MODE, true, true>(a, a.B, p.lds_bytes, s, residual, p.nw);
  else if (p.gv) launch_solve<MODE, true>(a, a.B, p.lds_bytes, s, residual, p.nw);
  else launch_solve<MODE, false>(a, a.B, p.lds_bytes, s, residual, p.nw);
}

static int solve_impl(const DavaScene* scene, const DavaSolverConfig* config, const float* x0, float* x_out,
                      float* error_out, int32_t* status_out, void* workspace, size_t workspace_bytes, bool record,
                      void* stream) {
  const int st = check_scene(scene, true);
  if (st != DAVA_OK) return st;
  if (!config || config->iterations < 0 || config->max_line_search_trials < 0) return DAVA_ERR_INVALID_ARGUMENT;
  if (!(config->drop_path_p >= 0.f && config->drop_path_p <= 1.f)) return DAVA_ERR_INVALID_ARGUMENT;
  const SolvePlan p = plan_solve(scene, config, record);
  if (!p.sized) return p.status;  // (the Hessian mode)
  if (record && !p.tape_ok) return DAVA_ERR_UNSUPPORTED;
  if (scene->batch == 0) return DAVA_OK;
  if (!x0 || !x_out) return DAVA_ERR_INVALID_ARGUMENT;
  if (p.status != DAVA_OK) return p.status;  // (the LDS image does not fit)
  const int mode = config->hessian_mode;
  const size_t need = p.state_bytes;
  const bool uses_ws = record || p.gv || (mode == DAVA_HESSIAN_DENSE ? config->iterations > 2 : config->iterations > 1);
  if (uses_ws && (!workspace || workspace_bytes < need)) return DAVA_ERR_WORKSPACE;
  // the work queue needs its counter in the workspace's tail (dava_ba_solve_workspace_bytes
  // includes it); a workspace sized without it runs one workgroup per problem instead
  const bool queue = workspace && workspace_bytes >= need + kQueueBytes && !debug_flag(kDbgNoQueue);
  char* const ws = static_cast<char*>(workspace);
  SolveArgs a;
  a.L = make_layout(scene);
  a.B = scene->batch;
  a.Pv = p.Pv;
  a.Pld = p.Pld;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.x0 = x0;
  a.x_out = x_out;
  a.err_out = error_out;
  a.status = status_out;
  a.vecs = p.gv ? reinterpret_cast<float*>(ws + p.vec_offset) : nullptr;
  a.scal_slice = p.scal_slice ? 1 : 0;
  a.vstride = p.vstride;
  a.kcap_lds = p.kcap_lds;
  a.hess = ws ? reinterpret_cast<float*>(ws + p.hist_offset) : nullptr;
  a.hess_dense = p.hybrid && ws ? reinterpret_cast<float*>(ws + p.dense_offset) : nullptr;
  a.c1 = config->sufficient_decrease;
  a.c2 = config->curvature;
  a.thr = config->error_threshold;
  a.min_step = config->minimum_step;
  a.iters = config->iterations;
  a.max_trials = config->max_line_search_trials;
  a.strong = config->strong_wolfe;
  a.mode = mode;
  a.kcap = p.kcap;
  a.lcap = p.lcap;
  a.phase_cycles = nullptr;
  a.stagger = 0;
  a.stagger_levels = 1;
  a.drop_p = config->drop_path_p;
  a.drop_seed = ((unsigned long long)config->drop_seed_hi << 32) | config->drop_seed_lo;
  a.second_last = config->return_second_last ? 1 : 0;
  a.queue = queue ? reinterpret_cast<int*>(ws + need) : nullptr;
  a.tape_x = a.tape_g = a.tape_s = nullptr;
  a.tape_T = p.tape.T;
  if (record) {  // (the plan's history and vector offsets are the tape's)
    float* t = static_cast<float*>(workspace);
    a.tape_x = t + p.tape.x;
    a.tape_g = t + p.tape.g;
    a.tape_s = t + p.tape.scal;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (a recording zeroes its whole queue tail: the tape tensor handed back includes it)
  if (record && workspace_bytes >= need + kQueueBytes) {
    if (hipMemsetAsync(ws + need, 0, kQueueBytes, s) != hipSuccess) return DAVA_ERR_LAUNCH;
  } else if (queue && hipMemsetAsync(a.queue, 0, sizeof(int), s) != hipSuccess) {
    return DAVA_ERR_LAUNCH;
  }
  // the tape's scalar rows have slots no solve writes (rho / c of step K, padding): zero them so a
  // tape is a deterministic function of the inputs, byte for byte (B x T floats, small)
  if (record && hipMemsetAsync(a.tape_s, 0, (size_t)scene->batch * p.tape.T * sizeof(float), s) != hipSuccess)
    return DAVA_ERR_LAUNCH;
#if DAVA_PHASE_TIMING
  const size_t ph_bytes = (size_t)scene->batch * kPhases * sizeof(unsigned long long);
  if (hipMalloc(&a.phase_cycles, ph_bytes) != hipSuccess) return DAVA_ERR_LAUNCH;
  (void)hipMemsetAsync(a.phase_cycles, 0, ph_bytes, s);
  {
    const unsigned long long zero[kEvalSections] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_eval_cycles), zero, sizeof(zero));
  }
#endif
  if (p.mode == DAVA_HESSIAN_DENSE) launch_solve_mode<DAVA_HESSIAN_DENSE>(a, p, scene->residual, s);
  else if (p.mode == kHybrid) launch_solve_mode<kHybrid>(a, p, scene->residual, s);
  else launch_solve_mode<DAVA_HESSIAN_COMPACT>(a, p, scene->residual, s);
  const int result = launched();
#if DAVA_PHASE_TIMING
  {
    unsigned long long* h = static_cast<unsigned long long*>(malloc(ph_bytes));
    (void)hipStreamSynchronize(s);
    (void)hipMemcpy(h, a.phase_cycles, ph_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(a.phase_cycles);
    static const char* names[kPhases] = {"eval_at_x", "history", "direction", "trial_evals", "search_logic", "step",
                                         "total"};
    double avg[kPhases] = {0};
    for (int b = 0; b < scene->batch; ++b)
      for (int i = 0; i < kPhases; ++i) avg[i] += (double)h[(size_t)b * kPhases + i] / scene->batch;
    fprintf(stderr, "[dava phase cycles / problem]");
    for (int i = 0; i < kPhases; ++i) fprintf(stderr, " %s=%.0f (%.1f%%)", names[i], avg[i], 100.0 * avg[i] / avg[kPhases - 1]);
    fprintf(stderr, "\n");
    // per-problem distribution (a launch lasts as long as its slowest problems): p50 / p99 / max per phase
    {
      std::vector<unsigned long long> col(scene->batch);
      fprintf(stderr, "[dava phase cycles distribution]");
      for (int i = 0; i < kPhases; ++i) {
        for (int b = 0; b < scene->batch; ++b) col[b] = h[(size_t)b * kPhases + i];
        std::sort(col.begin(), col.end());
        const size_t n = col.size();
        fprintf(stderr, " %s=p50:%llu,p99:%llu,max:%llu", names[i], col[n / 2], col[std::min(n - 1, (size_t)(0.99 * n))],
                col[n - 1]);
      }
      fprintf(stderr, "\n");
    }
    unsigned long long ev[kEvalSections] = {};
    (void)hipMemcpyFromSymbol(ev, HIP_SYMBOL(g_eval_cycles), sizeof(ev));
    static const char* enames[kEvalSections] = {"view_constants", "point_sums", "setup", "pair_sweep", "final_sums",
                                                "gradient_assembly"};
    fprintf(stderr, "[dava objective cycles / problem]");
    for (int i = 0; i < kEvalSections; ++i) fprintf(stderr, " %s=%.0f", enames[i], (double)ev[i] / scene->batch);
    fprintf(stderr, "\n");
    free(h);
  }
#endif
  return result;
}

extern "C" int dava_ba_solve(const DavaScene* scene, const DavaSolverConfig* config, const float* x0,
                             float* x_out, float* error_out, int32_t* status_out, void* workspace,
                             size_t workspace_bytes, void* stream) {
  return solve_impl(scene, config, x0, x_out, error_out, status_out, workspace, workspace_bytes, false, stream);
}

extern "C" int dava_ba_solve_record(const DavaScene* scene, const DavaSolverConfig* config, const float* x0,
                                    float* x_out, float* error_out, int32_t* status_out, void* tape,
                                    size_t tape_bytes, void* stream) {
  if (!status_out && scene && scene->batch > 0) return DAVA_ERR_INVALID_ARGUMENT;  // the adjoint needs the steps
  return solve_impl(scene, config, x0, x_out, error_out, status_out, tape, tape_bytes, true, stream);
}

// The instantiation for a plan's form -- GV in place or GV + XL (8 waves), LDS mode with or without a point per
// thread in registers -- the outputs asked for (gradient, slope, trial point x + alpha d) and the residual
static int launch_eval(const EvalArgs& a, int B, const EvalPlan& p, int residual, hipStream_t s) {
  auto go = [&](auto kernel) { launch_lds(kernel, B, kWave * p.nw, p.lds_bytes, s, a); };
  with_flag(a.grad != nullptr, [&](auto grad) {
    with_flag(a.slope != nullptr, [&](auto slope) {
      with_flag(a.dir != nullptr && a.alpha != nullptr, [&](auto trial) {
        with_flag(residual == DAVA_RESIDUAL_RAY_ANGLE, [&](auto ray) {
          constexpr int kRes = decltype(ray)::value ? DAVA_RESIDUAL_RAY_ANGLE : DAVA_RESIDUAL_SQUARED_REPROJECTION;
          constexpr bool G = decltype(grad)::value, S = decltype(slope)::value, T = decltype(trial)::value;
          constexpr int GVW = solve_waves(true);
          if (p.gv && !p.xl) go(ba_evaluate_kernel<G, S, T, true, kRes, false, GVW, 0>);
          else if (p.gv) go(ba_evaluate_kernel<G, S, T, true, kRes, true, GVW, 0>);
          else if (p.ppt) go(ba_evaluate_kernel<G, S, T, false, kRes, false, kWaves, 1>);
          else go(ba_evaluate_kernel<G, S, T, false, kRes, false, kWaves, 0>);
        });
      });
    });
  });
  return launched();
}

extern "C" int dava_ba_evaluate(const DavaScene* scene, const float* x, const float* direction, const float* alpha,
                                float* error_out, float* grad_out, float* slope_out, void* stream) {
  const int st = check_scene(scene, true);
  if (st != DAVA_OK) return st;
  if (scene->batch == 0) return DAVA_OK;
  if (!x || !error_out) return DAVA_ERR_INVALID_ARGUMENT;
  if (slope_out && !direction) return DAVA_ERR_INVALID_ARGUMENT;
  const EvalPlan p = plan_eval(scene);
  if (p.status != DAVA_OK) return p.status;
  EvalArgs a;
  a.L = make_layout(scene);
  a.Pv = p.Pv;
  a.obs = scene->observations;
  a.vis = scene->visibility;
  a.x = x;
  a.dir = direction;
  a.alpha = alpha;
  a.err = error_out;
  a.grad = grad_out;
  a.slope = slope_out;
  return launch_eval(a, scene->batch, p, scene->residual, static_cast<hipStream_t>(stream));
}
