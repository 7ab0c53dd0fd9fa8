// The geometry of an adjoint launch (bfgs_adjoint.hip): carve_adjoint, which the kernel indexes its LDS and its
// workspace slice with and the host sizes them with, and -- host only -- AdjointPlan, the one derivation of
// everything the launch and the size queries need from (scene, config).
#pragma once

#include "ba_objective.hpp"
#include "dava_debug.hpp"
#include "dava_tape.hpp"

namespace dava {

constexpr int kAdjWaves = 4;
constexpr int kAdjBlock = kWave * kAdjWaves;
constexpr int kAdjMaxGroups = 14;  // GV mode: float4 groups per thread (P <= 14 * 256 * 4 = 14336)
constexpr int kAdjLdsBytes = 160 * 1024;
// LDS mode: two workgroups per CU (registers <= 256 VGPRs, LDS <= 80 KB each), so one problem's
// dual-number evaluation overlaps the other's row passes: C3 solve + gradient 51.7k -> 63.0k problems/s
// (r03, profiles/r03_ab_adjoint_two_wg_per_cu.log; in r02 the same register cap spilled 100-165
// registers and one workgroup per CU was faster, since then the passes' register use went down).
constexpr int kAdjLdsWpe = 2;

struct AdjointCarve {
  int xb, sbp, gbp, db, gk, p1, p2, wb, sv, wv, yv, gv, ak, an, sc, xd, gd, views, vpart, obs, obsacc, lh, scratch,
      vis_bytes_off, total_bytes;
  int gv_floats;  // global-vector mode: floats of one problem's workspace slice (the 14 vectors and 2 Dual ones)
};

// lcap: the oldest history entries' rows (s_j, w_j interleaved) kept on chip for the whole reverse
// sweep -- every H pass reads them again, so each one held saves 2 Pv floats of HBM per step.
// gv (global-vector mode, P too large for the LDS image, e.g. C5): the O(P) vectors are offsets into
// the problem's workspace slice instead, the scene is read in place and the observation cotangent is
// accumulated straight into the output; LDS keeps the scalars, view constants and reduction scratch.
// gdl (global-vector mode): the dual gradient vector of the HVP evaluation in LDS instead of the slice
// -- the evaluation accumulates it view after view, one dependent read-modify-write per pair.
__host__ __device__ inline AdjointCarve carve_adjoint(int M, int N, int Pv, int T, int lcap = 0, bool gv = false,
                                                     int nw = kAdjWaves, bool gdl = false) {
  AdjointCarve c;
  int off = 0, voff = 0;
  int& o = gv ? voff : off;
  int* vec[] = {&c.xb, &c.sbp, &c.gbp, &c.db, &c.gk, &c.p1, &c.p2, &c.wb, &c.sv, &c.wv, &c.yv, &c.gv, &c.ak, &c.an};
  for (int* v : vec) { *v = o; o += Pv; }
  c.sc = off; off += T;
  c.xd = o; o += 2 * Pv;  // Dual
  int& og = gv && gdl ? off : o;
  c.gd = og; og += 2 * Pv;  // Dual
  c.gv_floats = gv ? voff : 0;
  c.views = off; off += 2 * round_up(views_floats(M), 4);
  c.vpart = off; off += 2 * round_up(vpart_floats(M, nw), 4);
  c.obs = off; off += gv ? 0 : round_up(2 * M * N, 4);
  c.obsacc = off; off += gv ? 0 : round_up(2 * M * N, 4);
  c.lh = off; off += gv ? 0 : 2 * lcap * Pv;
  c.scratch = off; off += 2 * nw * 32;
  c.vis_bytes_off = off * 4;
  c.total_bytes = c.vis_bytes_off + (gv ? 0 : round_up(M * N, 16));
  return c;
}

// ---- host only: the launch plan ----
// The size queries read fields and the launch fills AdjointArgs from them, so the bytes a caller allocated and the
// image the kernel carves come from one derivation.
struct AdjointPlan {
  // DAVA_OK, or why no launch runs (then the other fields are unset).  The data pointers, the empty batch, the
  // tape's and the workspace's sizes are the launch's own checks, after the plan's.
  int status;
  bool gv, sc_global, gd_lds;  // global-vector mode; the kernel's SCG (LDS mode); carve_adjoint's gdl (GV mode)
  int nw, gm, gt;  // waves; float4 groups per lane of a wave (pair_pass) / per thread of a GV workgroup (else 0)
  int lcap, lds_bytes;  // history entries held in LDS; the image
  TapeLayout tl;
  size_t rows_bytes, gv_bytes;  // workspace: the a rows (B, K, Pv), then in GV mode the per-problem vector slices
};

inline AdjointPlan plan_adjoint(const DavaScene* s, const DavaSolverConfig* c) {
  AdjointPlan p{};
  p.status = DAVA_ERR_INVALID_ARGUMENT;
  if (!c) return p;
  p.status = check_scene(s, false);  // (the launch checks the data pointers itself)
  if (p.status != DAVA_OK) return p;
  p.status = DAVA_ERR_UNSUPPORTED;
  if (c->hessian_mode != DAVA_HESSIAN_COMPACT || c->iterations < 1 || c->iterations > 1025) return p;
  const int M = s->num_views, N = s->num_points;
  const TapeLayout tl = p.tl = tape_layout(s->batch, s->num_parameters, c->iterations);
  const int Pv = tl.Pv;
  auto image = [&](int T, int lcap = 0, bool gv = false, int nw = kAdjWaves, bool gdl = false) {
    return carve_adjoint(M, N, Pv, T, lcap, gv, nw, gdl).total_bytes;
  };
  constexpr int kPerWg = kAdjLdsBytes / kAdjLdsWpe;
  const int full = image(tl.T);  // LDS mode, the scalar row staged, no entries
  // Global-vector mode when the LDS image does not fit one CU (or P > 1024, past pair_pass's 4 groups
  // per lane); the kDbgAdjForceGV override forces it (tests: the same tape through both kernels).
  p.gv = debug_flag(kDbgAdjForceGV) || s->num_parameters > 1024 || full > kAdjLdsBytes;
  p.nw = kAdjWaves;
  if (p.gv) {
    if ((Pv / 4 + kAdjBlock - 1) / kAdjBlock > kAdjMaxGroups) return p;
    // Global-vector mode: waves per workgroup (one workgroup per CU).  Eight: the row passes hold up to 7
    // float4 groups per thread and two waves per SIMD hide their latency; the dual-number evaluation then
    // runs at the 256-VGPR budget.  Four: up to 14 groups per thread, one wave per SIMD with 512 registers.
    // Eight unless the eight-wave LDS image (per-wave view partials and reduction scratch grow with the
    // waves) does not fit -- many views -- or the kDbgAdjGVWaves override asks for four.
    p.nw = debug_knob(kDbgAdjGVWaves) != 4 && image(tl.T, 0, true, 8) <= kAdjLdsBytes ? 8 : 4;
    // the image of the launch that will run
    if (image(tl.T, 0, true, p.nw) > kAdjLdsBytes) return p;
  } else {
    // LDS mode: the tape's scalar row stays in place (SCG) when staging it would push the image past the two
    // workgroups per CU that the rest of it allows
    if (debug_knob(kDbgAdjScGlobal) >= 0) p.sc_global = debug_knob(kDbgAdjScGlobal) > 0;  // tests
    else p.sc_global = full > kPerWg && image(0) <= kPerWg;
    // As many history entries on chip as the CU's LDS leaves room for (two workgroups per CU), at most
    // the K - 1 a solve can make; the kDbgAdjLdsEntries override caps it (0: none) for A/B runs.  None in GV mode.
    const int room = kPerWg - (p.sc_global ? image(0) : full), per = 2 * Pv * (int)sizeof(float);
    int n = room < per ? 0 : min(room / per, tl.K - 1);
    if (debug_knob(kDbgAdjLdsEntries) >= 0) n = max(0, min(n, (int)debug_knob(kDbgAdjLdsEntries)));
    p.lcap = n;
  }
  // GV mode: the dual gradient vector in LDS where it fits beside the rest (the passes stage their rows through
  // it, bfgs_ba_adjoint_kernel `stage`); the kDbgAdjGdHbm override keeps it in the slice
  p.gd_lds = p.gv && !debug_flag(kDbgAdjGdHbm) && image(tl.T, 0, true, p.nw, true) <= kAdjLdsBytes;
  p.lds_bytes = image(p.sc_global ? 0 : tl.T, p.lcap, p.gv, p.nw, p.gd_lds);
  p.gm = (Pv / 4 + kWave - 1) / kWave;
  p.gt = p.gv ? (Pv / 4 + kWave * p.nw - 1) / (kWave * p.nw) : 0;
  p.rows_bytes = (size_t)s->batch * tl.K * Pv * sizeof(float);
  p.gv_bytes = p.gv ? (size_t)s->batch * carve_adjoint(M, N, Pv, tl.T, 0, true).gv_floats * sizeof(float) : 0;
  p.status = DAVA_OK;
  return p;
}

}  // namespace dava
