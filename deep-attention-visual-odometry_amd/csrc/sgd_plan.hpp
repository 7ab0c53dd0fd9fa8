// The geometry of the float32 fused gradient descent (sgd_solve.hip): the LDS image, the tape its adjoint
// (sgd_adjoint.hpp) replays, and -- host only -- what the entry points and the size queries derive from
// (scene, config).  The kernels index their LDS with the same code the host sizes it with.  The adjoint's image
// is the dual one of dual_image.hpp, followed by dual_acc_bytes of accumulator.
#pragma once

#include "dual_image.hpp"
#include "solve_plan.hpp"

namespace dava {

// Forward image: x, the gradient, (LDS form) the observations, the view constants and per-wave view partials
// of ba_eval, its reduction scratch, and (LDS form) the visibility bytes.
struct SgdCarve {
  int x, g, obs, views, vpart, scratch, vis_bytes_off, total_bytes;  // offsets in floats
};

__host__ __device__ inline SgdCarve carve_sgd(int M, int N, int Pv, bool gv, int nw) {
  SgdCarve c;
  int off = 0;
  c.x = off; off += Pv;
  c.g = off; off += Pv;
  c.obs = off; off += gv ? 0 : round_up(2 * M * N, 4);
  c.views = off; off += round_up(views_floats(M), 4);
  c.vpart = off; off += round_up(vpart_floats(M, nw), 4);
  c.scratch = off; off += 2 * nw * 32;
  c.vis_bytes_off = off * 4;
  c.total_bytes = c.vis_bytes_off + (gv ? 0 : round_up(M * N, 16));
  return c;
}

// The tape: x_k for k = 0 .. K-1, rows of Pv = round_up(P, 4) floats, laid out (B, K, Pv).  No header.
inline size_t sgd_tape_bytes(int B, int K, int Pv) { return (size_t)B * (size_t)K * (size_t)Pv * sizeof(float); }

// ---- host only ----
struct SgdPlan {
  int status;  // DAVA_OK, or why no launch runs (then the other fields are unset)
  bool gv;     // large form
  bool ppt;    // LDS form with a point per thread in registers
  int Pv, lds_bytes;
};

// check_scene(scene, ...) must have passed.
inline SgdPlan plan_sgd(const DavaScene* scene, const DavaSgdConfig* config) {
  SgdPlan p{};
  if (!config || config->iterations < 0) {
    p.status = DAVA_ERR_INVALID_ARGUMENT;
    return p;
  }
  p.status = DAVA_ERR_UNSUPPORTED;
  if (!sizes_sane(*scene)) return p;
  const EvalPlan e = plan_eval(scene);  // the evaluation's form; the image is the descent's own
  p.gv = e.gv;
  p.ppt = e.ppt;
  p.Pv = e.Pv;
  p.lds_bytes = carve_sgd(scene->num_views, scene->num_points, p.Pv, p.gv, e.nw).total_bytes;
  if (p.lds_bytes > kMaxLds) return p;
  p.status = DAVA_OK;
  return p;
}

}  // namespace dava
