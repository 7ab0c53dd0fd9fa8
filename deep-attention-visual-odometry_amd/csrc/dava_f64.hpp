// What the float64 sources share (solve_f64.hpp, adjoint_f64.hpp, dual_image.hpp): the limits of the
// one-workgroup-per-problem LDS images, and the host-side scene check.
#pragma once

#include "dava_common.hpp"

namespace dava {
namespace f64 {

constexpr long long kMaxLdsBytes = kMaxLds;  // (the one limit, in the type the float64 images are sized in)
constexpr int kMaxIterations = 1025;  // at most 1024 history entries, as the fp32 COMPACT mode

// DavaSceneF64 has DavaScene's fields; the shared host checks (check_scene) read no observation
inline int check_scene_f64(const DavaSceneF64* s, bool need_data, DavaScene& as32) {
  if (!s) return DAVA_ERR_INVALID_ARGUMENT;
  as32 = DavaScene{s->batch,      s->num_views, s->num_points, s->distortion, s->num_parameters,
                   reinterpret_cast<const float*>(s->observations), s->visibility, s->residual};
  return check_scene(&as32, need_data);
}

inline int history_capacity(int iterations) { return iterations - 1 > 1 ? iterations - 1 : 1; }

// The host side of every float64 operation is a plan and a launcher.  A plan is pure host code
// -- no HIP call, no data pointer dereferenced -- that runs the entry point's checks in their one order and
// leaves the status, the form, the LDS bytes, the workspace blocks and the filled kernel argument.  `any_form`
// tells the entry points apart: false for the symbols of the LDS image (form 0 by fit alone, the F64_FORM override
// ignored, everything else DAVA_ERR_UNSUPPORTED); true for the *_large_* symbols and the form queries, which take
// the form choose_form / choose_adjoint_form / choose_dual_form (dual_image.hpp) name.

}  // namespace f64
}  // namespace dava
