// LDS image of the dual-number (forward-over-reverse) evaluation of one problem: shared by the second
// derivatives (ba_second_order.hip) and the adjoint of the fused gradient descent (sgd_adjoint.hip), which
// appends its float accumulator for dL/dobs after it.
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

}  // namespace dava
