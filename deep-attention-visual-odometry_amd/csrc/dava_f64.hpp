// What the float64 sources share (bfgs_solve_f64.hip, ba_second_order_f64.hip, bfgs_adjoint_f64.hip): the
// limits of the one-workgroup-per-problem LDS images and the host-side scene check.
#pragma once

#include "dava_common.hpp"

namespace dava {
namespace f64 {

constexpr long long kMaxLdsBytes = 160 * 1024;
constexpr int kMaxIterations = 1025;  // at most 1024 history entries, as the fp32 COMPACT mode
constexpr size_t kTailBytes = 256;    // kept for a queue counter (none is used)

// DavaSceneF64 has DavaScene's fields; the shared host checks (check_scene) read no observation
inline int check_scene_f64(const DavaSceneF64* s, bool need_data, DavaScene& as32) {
  if (!s) return DAVA_ERR_INVALID_ARGUMENT;
  as32 = DavaScene{s->batch,      s->num_views, s->num_points, s->distortion, s->num_parameters,
                   reinterpret_cast<const float*>(s->observations), s->visibility, s->residual};
  return check_scene(&as32, need_data);
}

inline int history_capacity(int iterations) { return iterations - 1 > 1 ? iterations - 1 : 1; }

}  // namespace f64
}  // namespace dava
