// The geometry of a fused-solve launch (bfgs_solve.hip): how one problem's state is carved out of LDS and
// of its workspace slice, and -- host only, below -- the one derivation of everything a launch and the
// size queries need from (scene, config): SolvePlan, and EvalPlan for the objective evaluation.
//
// The __host__ __device__ part is what the kernels themselves call (carve_lds): the host sizes the image
// with the same code the device indexes it with.
#pragma once

#include "ba_objective.hpp"
#include "dava_debug.hpp"
#include "dava_tape.hpp"

namespace dava {

struct LdsCarve {
  int x, d, ge, g0, g1, s0, s1, hy0, hy1, hg, obs, views, vpart, scratch, hcoef, hrho, hc, hist, vis_bytes_off,
      total_bytes;
};

constexpr int kVectors = 9;  // x d g g_prev s s_pend Hy Hy_pend Hg

// Waves per solve workgroup: 4 when the problem lives in LDS (two workgroups per CU);
// 8 in global-vector mode, where problems are few and long (C5: B = 256 on 256 CUs) and
// one workgroup per CU would otherwise leave each SIMD a single wave to hide latency with.
__host__ __device__ constexpr int solve_waves(bool gv) { return gv ? 8 : 4; }
constexpr int kSolveWavesPerEU = 2;  // <= 256 VGPRs: two 4-wave workgroups per CU
constexpr int kHybrid = 2;  // kernel MODE (internal; callers ask for DAVA_HESSIAN_COMPACT)

// GV mode, COMPACT: the workgroup-wide single history pass keeps at most this many float4
// column groups per thread in registers (P <= 7 * 512 * 4 = 14336); longer rows use two passes.
constexpr int kWideMaxGroups = 7;
// History entries per block reduction in the wide pass for rows of > 2 groups per thread (two
// entries' rows do not fit the registers beside y, g and the sums there).
#ifndef DAVA_GV_ENTRIES
#define DAVA_GV_ENTRIES 1  // (microbenchmark builds only: tools/micro/wide_pass_stream.hip)
#endif
constexpr int kGvEntries = DAVA_GV_ENTRIES;
__host__ __device__ inline bool wide_history_pass(int Pv, int kcap, bool gv) {
  return gv && kcap > 0 && (Pv / 4 + kWave * solve_waves(gv) - 1) / (kWave * solve_waves(gv)) <= kWideMaxGroups;
}
// GV mode, wide pass: where each history entry's rho_j and c_j live.  In LDS (8 B per entry) while the XL
// image (x, d and the objective's gradient, 149 KB at C5) still fits beside them; past that (C5: ~950
// iterations, e.g. the reference's default cap of 1000) in the problem's workspace slice, after its
// kVectors vectors (round_up(kcap, 64) floats each), so that the XL image stays: without it the solve ran
// at 4.80k against 7.22k problems/s at K = 100 (profiles/r05_ab_c5_xl.log).  Measured before the product
// coefficients left the LDS image (when the slice took over at ~320 iterations): K = 400 689 against 539
// problems/s, the reference's defaults 323 against 264, K = 100 unchanged (profiles/r05_ab_c5_scalar_slice.log).
// The pass reads entry j's pair with one uniform load each, issued at the entry's start and needed only
// after its block reduction.
__host__ __device__ inline int gv_scalar_stride(int kcap) { return round_up(kcap, 64); }
__host__ __device__ inline int gv_slice_floats(int Pv, int kcap, bool scalars_in_slice) {
  return kVectors * Pv + (scalars_in_slice ? 2 * gv_scalar_stride(kcap) : 0);
}

// LDS image of one problem.  In global-vector (GV) mode -- large P, where the O(P)
// vectors cannot live on-chip -- the nine vectors sit in a per-problem slice of the
// workspace instead (offsets index that slice) and obs / vis are read in place.
// COMPACT LDS mode may keep the OLDEST lcap history entries on-chip (S row then W row,
// 2 Pv floats per entry): entry j is read by every iteration k > j + 1, so the first
// entries carry the most traffic (lcap = 6 at C3 removes 12% of the history reads).
// GV mode with xl ("x local"): x, d and the objective's gradient output (ge) still fit in
// LDS (3 Pv floats; C5: 149 KB), so the objective -- whose per-(view, point) work reads x
// and d and accumulates point gradients view after view, one dependent access per pair --
// runs on-chip; the other vectors stay in the workspace slice (its x and d slots unused).
__host__ __device__ inline LdsCarve carve_lds(int M, int N, int Pv, int kcap = 0, bool gv = false, int lcap = 0,
                                              bool xl = false, int nw = 0) {
  if (nw <= 0) nw = solve_waves(gv);
  LdsCarve c;
  int off = 0;
  int voff = 0;
  int& o = gv ? voff : off;
  int& ox = gv && !xl ? voff : off;
  c.x = ox; ox += Pv;
  c.d = ox; ox += Pv;
  if (gv && xl) voff += 2 * Pv;
  c.ge = gv && xl ? off : 0;
  off += gv && xl ? Pv : 0;
  c.g0 = o; o += Pv;
  c.g1 = o; o += Pv;
  c.s0 = o; o += Pv;
  c.s1 = o; o += Pv;
  c.hy0 = o; o += Pv;
  c.hy1 = o; o += Pv;
  c.hg = o; o += Pv;
  c.obs = off; off += gv ? 0 : round_up(2 * M * N, 4);
  c.views = off; off += round_up(views_floats(M), 4);
  c.vpart = off; off += round_up(vpart_floats(M, nw), 4);
  c.scratch = off; off += 2 * nw * 32;
  // COMPACT: per-entry product coefficients, for the two-pass products only (compact_products: GV rows
  // past the wide pass, LDS-mode rows of more than 4 float4 groups per lane); the single-pass forms form
  // each entry's coefficients on the fly (r05: 16 B per entry returned to the on-chip history entries /
  // the XL image)
  const bool two_pass = gv ? !wide_history_pass(Pv, kcap, true) : (Pv / 4 + kWave - 1) / kWave > 4;
  c.hcoef = off; off += two_pass ? 4 * kcap : 0;
  c.hrho = off; off += round_up(kcap, 4);
  c.hc = off; off += round_up(kcap, 4);
  c.hist = off; off += gv ? 0 : 2 * lcap * Pv;
  c.vis_bytes_off = off * 4;
  c.total_bytes = c.vis_bytes_off + (gv ? 0 : round_up(M * N, 16));
  return c;
}

// ---- host only: the launch plan ----
// Global-vector mode when the all-in-LDS image would cost more than two workgroups
// per CU (e.g. C5: P = 12381 -> 446 KB of vectors per problem).
constexpr int kLdsModeBudget = 72 * 1024;
// only rows of >= 6 float4 groups per thread have the slice form instantiated (wide_direction SLICE):
// narrower rows leave room for the scalars beside their XL image at any cap
constexpr int kSliceMinGroups = 6;
// History entries the COMPACT mode keeps: one per iteration k = 1 .. iterations-1, at most
// kMaxCompactEntries; a longer solve is HYBRID (fold_history: the dense matrix after the history fills).
// The kDbgCompactSwitch override lowers the capacity (tests: the switch at K = 30 instead of 1025).
constexpr int kMaxCompactEntries = 1024;
// The work-queue counter follows the solve's state (vectors in GV mode + inverse-Hessian state), in the
// last kQueueBytes of the workspace.
constexpr size_t kQueueBytes = 256;
// A recording solve (the tape of dava_tape.hpp) needs COMPACT mode and P <= 14336: the adjoint kernel
// runs P <= 1024 with its O(P) vectors in LDS and larger P (the forward's global-vector mode, e.g. C5)
// with them in its workspace, both over rows of at most 14 float4 groups per thread.  A GV-mode
// recording also needs the forward's wide single-pass history products (the ones that write the tape).
constexpr int kTapeMaxParameters = 14336;

// Everything the solve's entry points derive from (scene, config): the size queries read fields, the
// launch fills SolveArgs from them, so the bytes a caller allocated and the offsets the kernel uses come
// from the same derivation.
struct SolvePlan {
  // DAVA_OK, or why a launch is refused: the scene (check_scene), the config pointer or the Hessian mode
  // -- then `sized` is false and no other field is set -- or DAVA_ERR_UNSUPPORTED for an LDS image that
  // does not fit, with every field set (the size queries still answer).
  int status;
  bool sized;
  int mode;  // the kernel's MODE: DAVA_HESSIAN_DENSE, DAVA_HESSIAN_COMPACT or kHybrid
  bool hybrid, gv, xl, scal_slice;
  int kcap;      // COMPACT: history capacity (entries), else 0
  int kcap_lds;  // entries whose rho_j, c_j the LDS image holds (0 with scal_slice)
  int nw, lcap, lds_bytes;
  int Pv, Pld;
  int vstride;  // floats per problem in the GV vector slices
  // Workspace, in bytes: [GV vectors | history | dense matrices | queue counter]; a recording's tape puts
  // the history first and the vectors last (TapeLayout).  state_bytes is also the queue counter's offset.
  size_t vec_bytes, hist_bytes, dense_bytes, state_bytes;
  size_t vec_offset, hist_offset, dense_offset;
  bool tape_ok;  // a recording solve exists for this (scene, config)
  TapeLayout tape;
};

inline SolvePlan plan_solve(const DavaScene* s, const DavaSolverConfig* c, bool record) {
  SolvePlan p{};
  p.status = check_scene(s, false);
  if (p.status != DAVA_OK) return p;
  p.status = DAVA_ERR_INVALID_ARGUMENT;
  if (!c || (c->hessian_mode != DAVA_HESSIAN_DENSE && c->hessian_mode != DAVA_HESSIAN_COMPACT)) return p;
  p.sized = true;
  const bool compact = c->hessian_mode == DAVA_HESSIAN_COMPACT;
  const int M = s->num_views, N = s->num_points, P = s->num_parameters;
  const int Pv = p.Pv = round_up(P, 4);
  p.Pld = round_up(P, 32);
  const int gm = (Pv / 4 + kWave - 1) / kWave;  // float4 groups per lane of one wave
  const int gvw = solve_waves(true);
  const int gt = (Pv / 4 + kWave * gvw - 1) / (kWave * gvw);  // float4 groups per thread of a GV workgroup
  auto image = [&](int kcap_lds, bool gv, int lcap, bool xl, int nw) {
    return carve_lds(M, N, Pv, kcap_lds, gv, lcap, xl, nw).total_bytes;
  };

  // history capacity; past it COMPACT is HYBRID
  {
    const int need = c->iterations > 1 ? c->iterations - 1 : 1;
    const long long sw = debug_knob(kDbgCompactSwitch);
    const int cap = sw >= 1 && sw < kMaxCompactEntries ? (int)sw : kMaxCompactEntries;
    p.kcap = compact ? min(need, cap) : 0;
  }
  p.hybrid = compact && c->iterations - 1 > p.kcap;
  p.mode = p.hybrid ? kHybrid : c->hessian_mode;

  // Global-vector mode: by the LDS-mode image of a FOUR-wave workgroup with every rho_j, c_j in it and no
  // on-chip entries, whatever wave count an LDS-mode launch then takes (below).
  p.gv = debug_flag(kDbgForceGV) || image(p.kcap, false, 0, false, solve_waves(false)) > kLdsModeBudget;

  // GV mode, wide pass: rho_j, c_j move to the workspace slice when that keeps the XL image on-chip (see
  // gv_scalar_stride).  Decided on the EIGHT-wave XL image, and before XL itself: XL is then judged on the
  // image without the scalars, and the slice is used only if XL holds.
  bool slice = false;
  if (wide_history_pass(Pv, p.kcap, true) && gt >= kSliceMinGroups) {
    if (debug_knob(kDbgGvScalarSlice) >= 0) slice = debug_knob(kDbgGvScalarSlice) > 0;  // tests
    else slice = image(p.kcap, true, 0, true, gvw) > kMaxLds && image(0, true, 0, true, gvw) <= kMaxLds;
  }
  // GV mode: run the objective on LDS copies of x and d (carve_lds `xl`) whenever they fit beside the rest
  // of the image.  The kDbgGVNoXL override forces the in-workspace variant (tests).
  p.xl = p.gv && !debug_flag(kDbgGVNoXL) && image(slice ? 0 : p.kcap, true, 0, true, gvw) <= kMaxLds;
  p.scal_slice = p.xl && slice;  // (the slice form exists with XL only: bfgs_ba_solve_kernel SLICE)
  p.kcap_lds = p.scal_slice ? 0 : p.kcap;

  // Waves per LDS-mode workgroup (GV mode: always 8).  The register budget (256 VGPRs) holds two
  // waves per SIMD, eight per CU, whatever the split, so the choice is how many waves share one
  // problem: two waves while a history row is at most 2 x 64 float4 column groups (P <= 512), else
  // four, so small problems do not pay for barriers and cross-wave sums over idle waves
  // (interleaved A/B, profiles/r02_ab_waves.log: C2 +19%, 8192 two-view 64-point problems +49%,
  // C3 -17% at two).  One wave per problem measured another +9% on the 64-point shape but put one
  // K = 100 run-to-stagnation problem 3e-5 from the oracle (30x the reference's own 1-ulp
  // sensitivity), so it stays opt-in.  DENSE keeps 4.  The kDbgSolveWaves override (1 | 2 | 4) is for
  // A/B runs and tests.
  p.nw = gvw;
  if (!p.gv) {
    const long long w = debug_knob(kDbgSolveWaves);
    if (w == 1 || w == 2 || w == 4) p.nw = (int)w;
    else p.nw = compact && gm <= 2 ? 2 : 4;
  }

  // COMPACT, LDS mode, single-pass products: how many of the oldest history entries to keep
  // on-chip.  Default: whatever fits beside the problem image without lowering the number of
  // workgroups a CU holds at the register limit (4 SIMDs x kSolveWavesPerEU waves / nw:
  // two 4-wave workgroups of 80 KiB, or four 2-wave workgroups of 40 KiB); the kDbgLdsHistory override
  // sets the count (A/B and tests; 0 = all in HBM; values past one workgroup's LDS are clamped).
  // (A recording keeps them too, and every entry in HBM besides: bitwise the same run.)
  p.lcap = 0;
  if (compact && !p.gv && p.kcap > 0 && gm <= 4) {
    const int base = image(p.kcap, false, 0, false, p.nw);
    const int per = 2 * Pv * (int)sizeof(float);
    int per_cu = 4 * kSolveWavesPerEU / p.nw;  // workgroups per CU at the register limit
    if (debug_knob(kDbgWgPerCu) > 0) per_cu = (int)debug_knob(kDbgWgPerCu);  // A/B: LDS budget = 160 KB / this
    int n = (kMaxLds / per_cu - base) / per;
    // rows of <= 2 groups per lane consume the on-chip entries in batches, entries dealt round-robin to the
    // waves: a multiple of the waves keeps the waves' batches equal (C2 at K = 100: 7 entries measured -1.2%
    // against 6; the C1 shape 18 against 17 also -1.2%, so for these short rows an on-chip entry past the
    // first few is worth little either way, profiles/r05_ab_lds_coefficients.log)
    if (gm <= 2) n -= n % p.nw;
    if (debug_knob(kDbgLdsHistory) >= 0) n = (int)debug_knob(kDbgLdsHistory);
    n = min(n, (kMaxLds - base) / per);
    p.lcap = max(0, min(n, p.kcap));
  }
  p.lds_bytes = image(p.kcap_lds, p.gv, p.lcap, p.xl, p.nw);

  // workspace
  const size_t B = (size_t)s->batch;
  p.vstride = gv_slice_floats(Pv, p.kcap, p.scal_slice);
  p.vec_bytes = p.gv ? B * (size_t)p.vstride * sizeof(float) : 0;
  p.hist_bytes = compact ? B * 2 * (size_t)p.kcap * (size_t)Pv * sizeof(float) : 0;
  p.dense_bytes = !compact || p.hybrid ? B * (size_t)P * (size_t)p.Pld * sizeof(float) : 0;
  p.tape_ok = compact && c->iterations >= 1 && !p.hybrid && P <= kTapeMaxParameters &&
              (!p.gv || wide_history_pass(Pv, p.kcap, true));
  p.tape = tape_layout(s->batch, P, c->iterations, p.gv ? p.vstride : 0);
  if (record) {
    p.vec_offset = p.tape.vecs * sizeof(float);
    p.hist_offset = p.tape.hist * sizeof(float);
    p.state_bytes = p.tape.queue_byte;
  } else {
    p.vec_offset = 0;
    p.hist_offset = p.vec_bytes;
    p.state_bytes = p.vec_bytes + p.hist_bytes + p.dense_bytes;
  }
  p.dense_offset = p.hist_offset + p.hist_bytes;  // HYBRID: the dense matrices follow the histories
  p.status = p.lds_bytes > kMaxLds ? DAVA_ERR_UNSUPPORTED : DAVA_OK;
  return p;
}

// ---- host only: the objective evaluation's form (dava_ba_evaluate; the gradient descent takes gv and ppt) ----
// The solve's own choices (plan_solve) for an image without history: GV mode by the four-wave LDS-mode image, XL
// by the eight-wave one; LDS mode holds a point per thread in registers (ppt) while N <= kBlock.  The kDbgForceGV,
// kDbgGVNoXL and kDbgNoPPT overrides apply as in the solve.  check_scene(s, ...) must have passed.
struct EvalPlan {
  int status;  // DAVA_OK, or DAVA_ERR_UNSUPPORTED for an image that does not fit
  bool gv, xl, ppt;
  int nw, lds_bytes, Pv;
};
inline EvalPlan plan_eval(const DavaScene* s) {
  EvalPlan p{};
  const int M = s->num_views, N = s->num_points;
  p.Pv = round_up(s->num_parameters, 4);
  p.gv = debug_flag(kDbgForceGV) || carve_lds(M, N, p.Pv).total_bytes > kLdsModeBudget;
  p.nw = p.gv ? solve_waves(true) : kWaves;
  p.xl = p.gv && !debug_flag(kDbgGVNoXL) && carve_lds(M, N, p.Pv, 0, true, 0, true, p.nw).total_bytes <= kMaxLds;
  p.ppt = !p.gv && N <= kBlock && !debug_flag(kDbgNoPPT);
  p.lds_bytes = carve_lds(M, N, p.Pv, 0, p.gv, 0, p.xl, p.nw).total_bytes;
  p.status = p.lds_bytes > kMaxLds ? DAVA_ERR_UNSUPPORTED : DAVA_OK;
  return p;
}

}  // namespace dava
