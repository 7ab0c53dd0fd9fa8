// LDS image of the float64 dual-number (forward-over-reverse) evaluation of one problem: shared by the float64
// second derivatives (ba_second_order_f64.hip) and the adjoint of the float64 gradient descent
// (sgd_adjoint_f64.hip), which appends its accumulator of dL/dobs after form 0's image.  Forms as in solve_f64.hpp:
//   form 0  the dual x and gradient, the dual dE/dobs, the observations and visibility in LDS (carve_second)
//   form 1  the dual x and gradient in LDS, the scene read in place, the dual dE/dobs in a workspace
//   form 2  as form 1, the dual x and gradient in a per-problem workspace slice of 4 Pv doubles
// carve_second_large is the LDS image of forms 1 and 2, choose_second_form the form a scene takes.
#pragma once

#include "ba_objective.hpp"
#include "dava_debug.hpp"
#include "dava_f64.hpp"

namespace dava {
namespace f64 {

using Dual64 = DualT<double>;

struct SecondCarve {
  int x, g, views, vpart, obsd, scratch, obs, vis_bytes_off;  // offsets in doubles
  long long total_bytes;
};

__host__ __device__ inline SecondCarve carve_second(int M, int N, int Pv) {
  SecondCarve c{};
  const long long MN = (long long)M * N;
  const long long doubles = 4LL * Pv + 2LL * views_floats(M) + 2LL * vpart_floats(M) + 4 * MN + 2 * kWaves * 32 + 2 * MN;
  c.total_bytes = doubles * 8 + round_up((int)(MN < (1 << 30) ? MN : (1 << 30)), 16);
  if (c.total_bytes > kMaxLdsBytes) return c;  // (offsets are meaningful only for an image that fits)
  int off = 0;
  c.x = off; off += 2 * Pv;                  // Dual64
  c.g = off; off += 2 * Pv;                  // Dual64
  c.views = off; off += 2 * views_floats(M);  // Dual64
  c.vpart = off; off += 2 * vpart_floats(M);  // Dual64
  c.obsd = off; off += 4 * (int)MN;          // Dual64 dE/dobs
  c.scratch = off; off += 2 * kWaves * 32;
  c.obs = off; off += 2 * (int)MN;
  c.vis_bytes_off = off * 8;
  return c;
}

// The LDS image of forms 1 and 2: no scene, no dE/dobs and in form 2 no x / g either.  x and g are relative to
// the vectors' base (LDS, or the problem's slice), the others to the LDS base.
__host__ __device__ inline SecondCarve carve_second_large(int M, int Pv, int form) {
  SecondCarve c{};
  const long long doubles = (form == 1 ? 4LL * Pv : 0) + 2LL * views_floats(M) + 2LL * vpart_floats(M) + 2 * kWaves * 32;
  c.total_bytes = doubles * 8;
  if (c.total_bytes > kMaxLdsBytes) return c;
  int off = 0;
  c.x = off; off += 2 * Pv;
  c.g = off; off += 2 * Pv;
  if (form != 1) off = 0;
  c.views = off; off += 2 * views_floats(M);
  c.vpart = off; off += 2 * vpart_floats(M);
  c.scratch = off; off += 2 * kWaves * 32;
  return c;
}

// The form a scene takes: the lowest whose image fits -- form 0's is carve_second's plus `extra0` bytes (the
// descent's adjoint appends its accumulator) -- raised (never lowered) by the F64_FORM override; -1 where not even
// form 2's image (the dual view constants and partials) fits.
inline int choose_second_form(int M, int N, int Pv, long long extra0 = 0) {
  int form = 2;
  if (carve_second(M, N, Pv).total_bytes + extra0 <= kMaxLdsBytes) form = 0;
  else if (carve_second_large(M, Pv, 1).total_bytes <= kMaxLdsBytes) form = 1;
  const long long forced = debug_knob(kDbgF64Form);
  if ((forced == 1 || forced == 2) && forced > form) form = (int)forced;
  if (form == 2 && carve_second_large(M, Pv, 2).total_bytes > kMaxLdsBytes) return -1;
  return form;
}

}  // namespace f64
}  // namespace dava
