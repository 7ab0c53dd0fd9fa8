// LDS image of the dual-number (forward-over-reverse) evaluation of one problem: shared by the second
// derivatives (ba_second_order.hip) and the adjoint of the fused gradient descent (sgd_adjoint.hip), which
// appends its float accumulator for dL/dobs after it -- and, host only, what both derive from a scene: SecondPlan.
// Beyond that image both kernels take the forms of the float64 ones (ba_second_order_f64.hip):
//   form 0  everything in LDS (carve_second)
//   form 1  the dual x and gradient in LDS, the scene read in place, the dual dE/dobs in a workspace
//   form 2  as form 1, the dual x and gradient in a per-problem workspace slice of 4 Pv floats
// carve_second_large is the LDS image of forms 1 and 2, choose_second_form the form a scene takes.
#pragma once

#include "ba_objective.hpp"
#include "dava_debug.hpp"

namespace dava {

struct SecondCarve {
  int x, g, views, vpart, obsd, scratch, obs, vis_bytes_off, total_bytes;  // offsets in floats
};

__host__ __device__ inline SecondCarve carve_second(int M, int N, int Pv) {
  SecondCarve c;
  int off = 0;
  c.x = off; off += 2 * Pv;                                  // Dual
  c.g = off; off += 2 * Pv;                                  // Dual
  c.views = off; off += 2 * round_up(views_floats(M), 4);    // Dual
  c.vpart = off; off += 2 * round_up(vpart_floats(M), 4);    // Dual
  c.obsd = off; off += 2 * 2 * M * N;                        // Dual dE/dobs
  c.scratch = off; off += 2 * kWaves * 32;
  c.obs = off; off += round_up(2 * M * N, 4);
  c.vis_bytes_off = off * 4;
  c.total_bytes = c.vis_bytes_off + round_up(M * N, 16);
  return c;
}

// The LDS image of forms 1 and 2: no scene, no dE/dobs and in form 2 no x / g either.  x and g are relative to
// the vectors' base (LDS, or the problem's slice), the others to the LDS base.  total_bytes saturates past
// kMaxLds (the offsets are meaningful only for an image that fits).
__host__ __device__ inline SecondCarve carve_second_large(int M, int Pv, int form) {
  SecondCarve c{};
  const long long floats = (form == 1 ? 4LL * Pv : 0) + 2LL * round_up(views_floats(M), 4) +
                           2LL * round_up(vpart_floats(M), 4) + 2 * kWaves * 32;
  c.total_bytes = floats * 4 > kMaxLds ? kMaxLds + 1 : (int)(floats * 4);
  if (c.total_bytes > kMaxLds) return c;
  int off = 0;
  c.x = off; off += 2 * Pv;                                  // Dual
  c.g = off; off += 2 * Pv;                                  // Dual
  if (form != 1) off = 0;
  c.views = off; off += 2 * round_up(views_floats(M), 4);    // Dual
  c.vpart = off; off += 2 * round_up(vpart_floats(M), 4);    // Dual
  c.scratch = off; off += 2 * kWaves * 32;
  return c;
}

constexpr size_t kSecondTailBytes = 256;  // the tail the float64 workspaces keep (dava_f64.hpp kTailBytes)

// ---- host only: check_scene(s, ...) must have passed ----
// (a size whose images and slices cannot be indexed in 32-bit offsets is refused)
inline bool second_sizes_sane(const DavaScene* s) {
  return (long long)s->num_views * s->num_points <= (1 << 24) && s->num_parameters <= (1 << 24);
}

// The form a scene takes: the lowest whose image fits kMaxLds -- form 0's is carve_second's plus `extra0` bytes
// (the descent's adjoint appends its accumulator) -- raised (never lowered) by the F32_DUAL_FORM override; -1
// where not even form 2's image (the dual view constants and partials) fits.
inline int choose_second_form(const DavaScene* s, int extra0 = 0) {
  if (!second_sizes_sane(s)) return -1;
  const int M = s->num_views, N = s->num_points, Pv = round_up(s->num_parameters, 4);
  int form = 2;
  if ((long long)carve_second(M, N, Pv).total_bytes + extra0 <= kMaxLds) form = 0;
  else if (carve_second_large(M, Pv, 1).total_bytes <= kMaxLds) form = 1;
  const long long forced = debug_knob(kDbgF32DualForm);
  if ((forced == 1 || forced == 2) && forced > form) form = (int)forced;
  if (form == 1 && carve_second_large(M, Pv, 1).total_bytes > kMaxLds) form = 2;  // (raised past its fit)
  if (form == 2 && carve_second_large(M, Pv, 2).total_bytes > kMaxLds) return -1;
  return form;
}

struct SecondPlan {
  int status;  // DAVA_OK, or DAVA_ERR_UNSUPPORTED for an image that does not fit
  int Pv, lds_bytes;
};
inline SecondPlan plan_second(const DavaScene* s) {
  SecondPlan p{};
  p.Pv = round_up(s->num_parameters, 4);
  p.lds_bytes = carve_second(s->num_views, s->num_points, p.Pv).total_bytes;
  p.status = p.lds_bytes > kMaxLds ? DAVA_ERR_UNSUPPORTED : DAVA_OK;
  return p;
}

}  // namespace dava
