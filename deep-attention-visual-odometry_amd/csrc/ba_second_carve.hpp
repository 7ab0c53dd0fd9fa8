// LDS image of the dual-number (forward-over-reverse) evaluation of one problem: shared by the second
// derivatives (ba_second_order.hip) and the adjoint of the fused gradient descent (sgd_adjoint.hip), which
// appends its float accumulator for dL/dobs after it -- and, host only, what both derive from a scene: SecondPlan.
#pragma once

#include "ba_objective.hpp"

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

// ---- host only: check_scene(s, ...) must have passed ----
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
