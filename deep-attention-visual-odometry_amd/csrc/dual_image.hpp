// LDS image of the dual-number (forward-over-reverse) evaluation of one problem, for float and double: shared by
// the second derivatives (ba_second_order.hpp) and the adjoint of the fused gradient descent (sgd_adjoint.hpp),
// which appends its accumulator of dL/dobs after form 0's image.  Forms as in solve_f64.hpp:
//   form 0  the dual x and gradient, the dual dE/dobs, the observations and visibility in LDS
//   form 1  the dual x and gradient in LDS, the scene read in place, the dual dE/dobs in a workspace
//   form 2  as form 1, the dual x and gradient in a per-problem workspace slice of 4 Pv elements
// carve_dual is the image of a form, choose_dual_form the form a scene takes.  Everything in which the float32
// and the float64 kernels differ is in DualTraits and descend; the kernels and the host planning are one template
// over them.
#pragma once

#include "ba_objective.hpp"
#include "dava_debug.hpp"
#include "sgd_f64.hpp"

namespace dava {

// Where the two types differ.  Each entry is what that type's kernels and entry points did before they shared one
// body; the comments are on the float specialisation.
template <class T>
struct DualTraits;

template <>
struct DualTraits<float> {
  // Sub-images start on 16 bytes.  A dual sub-image holds 2 n floats, so n is rounded up to 4 (as is the
  // observations' 2MN); 2 n doubles are a multiple of 16 bytes as they are.
  static constexpr int kAlign = 4;
  // Second __launch_bounds__ argument.  0 compiles to what leaving it out does, which is what the float32
  // kernels did; the float64 ones ask for one workgroup per CU like every float64 kernel.
  static constexpr int kMinBlocks = 0;
  // The float32 kernels hold the block index in an int and widen it at each use, the float64 ones hold a size_t.
  // Either would do for both; each is kept because the register allocation follows it.
  using block_index = int;
  // One override per precision, so that a test can raise one type's form and leave the other's alone.
  static constexpr DebugKnob kFormKnob = kDbgF32DualForm;
  // The float32 form choice refuses M N > 2^24 (sizes_sane).  The float64 second derivatives never did, and
  // their recorded statuses hold them to it: form 2's image does not depend on N.  (The descent's adjoint
  // checks sizes_sane for both types before it asks for a form.)
  static constexpr bool kGuardSizes = true;
  // Whether form 0's carve returns zero offsets for an image that does not fit, as forms 1 and 2 do for both
  // types.  A kernel never runs with such an image, but the test is compiled into it: with it the float32
  // form-0 kernels allocate other registers (fewer VGPRs), so it stays out until that is measured.  On the host
  // float32's form-0 offsets are therefore meaningful only where sizes_sane holds.
  static constexpr bool kForm0Checked = false;
};

template <>
struct DualTraits<double> {
  static constexpr int kAlign = 1;
  static constexpr int kMinBlocks = 1;
  using block_index = size_t;
  static constexpr DebugKnob kFormKnob = kDbgF64Form;
  static constexpr bool kGuardSizes = false;
  static constexpr bool kForm0Checked = true;
};

// The adjoint's update a - lr * b.  In float32 a plain expression, which the compiler may contract into one FMA
// (the float32 descent it differentiates is compiled the same way); in float64 f64::descend, as torch forms it:
// the product rounded, then the difference.
__device__ __forceinline__ float descend(float a, float lr, float b) { return a - lr * b; }
using f64::descend;

// The workgroup's dynamic LDS.  Declared once, as bytes: two arrays of different element types under one name
// do not coexist across the instantiations of a kernel template.
template <class T>
__device__ __forceinline__ T* dual_lds() {
  extern __shared__ __attribute__((aligned(16))) unsigned char dual_lds_bytes[];
  return reinterpret_cast<T*>(dual_lds_bytes);
}

constexpr long long round_up_ll(long long v, int m) { return (v + m - 1) / m * m; }
// (a count of elements rounded up to the type's alignment)
template <class T>
__host__ __device__ inline int dual_align(int v) {
  if constexpr (DualTraits<T>::kAlign == 1) return v;
  else return round_up(v, DualTraits<T>::kAlign);
}

struct DualCarve {
  int x, g, views, vpart, obsd, scratch, obs, vis_bytes_off;  // offsets in elements of T (the last in bytes)
  long long total_bytes;
};

// x and g are relative to the vectors' base (LDS, or in form 2 the problem's slice), the others to the LDS base.
// Forms 1 and 2 hold no scene and no dE/dobs, form 2 no x / g either.  total_bytes is computed in 64 bits for
// any scene; the offsets are meaningful only for an image that fits.  The kernels know their form when they are
// compiled, the host asks with the form as an argument (below).
template <class T, int form>
__host__ __device__ inline DualCarve carve_dual(int M, int N, int Pv) {
  DualCarve c{};
  const long long MN = (long long)M * N;
  const long long elems = (form == 2 ? 0 : 4LL * Pv) + 2LL * dual_align<T>(views_floats(M)) +
                          2LL * dual_align<T>(vpart_floats(M)) + (form == 0 ? 4 * MN : 0) + 2 * kWaves * 32 +
                          (form == 0 ? round_up_ll(2 * MN, DualTraits<T>::kAlign) : 0);
  // (the visibility bytes: M N clamped so that its rounding stays in an int)
  c.total_bytes = elems * (long long)sizeof(T) + (form == 0 ? round_up((int)(MN < (1 << 30) ? MN : (1 << 30)), 16) : 0);
  if ((form != 0 || DualTraits<T>::kForm0Checked) && c.total_bytes > kMaxLds) return c;
  int off = 0;
  c.x = off; off += 2 * Pv;  // Dual
  c.g = off; off += 2 * Pv;  // Dual
  if (form == 2) off = 0;
  c.views = off; off += 2 * dual_align<T>(views_floats(M));  // Dual
  c.vpart = off; off += 2 * dual_align<T>(vpart_floats(M));  // Dual
  if (form == 0) { c.obsd = off; off += 4 * (int)MN; }  // Dual dE/dobs
  c.scratch = off; off += 2 * kWaves * 32;
  if (form == 0) {
    c.obs = off; off += dual_align<T>(2 * (int)MN);
    c.vis_bytes_off = off * (int)sizeof(T);
  }
  return c;
}
template <class T>
inline DualCarve carve_dual(int M, int N, int Pv, int form) {
  return form == 0 ? carve_dual<T, 0>(M, N, Pv) : form == 1 ? carve_dual<T, 1>(M, N, Pv) : carve_dual<T, 2>(M, N, Pv);
}

// The descent's adjoint keeps its accumulator of dL/dobs (2MN elements) after form 0's image
template <class T>
inline long long dual_acc_bytes(int M, int N) {
  return round_up_ll(2LL * M * N, DualTraits<T>::kAlign) * (long long)sizeof(T);
}

// ---- host only ----
// The scene step of a plan: check_scene on either scene type, leaving the float32 view of it that the shared
// host code reads (no observation is read through it)
inline int check_dual_scene(const DavaScene* s, bool need_data, DavaScene& sc) {
  const int st = check_scene(s, need_data);
  if (st == DAVA_OK) sc = *s;
  return st;
}
inline int check_dual_scene(const DavaSceneF64* s, bool need_data, DavaScene& sc) {
  return f64::check_scene_f64(s, need_data, sc);
}

// Whether form 0's image and `extra0` bytes after it fit: what the symbols of the LDS image (any_form = false) ask
template <class T>
inline bool dual_fits_form0(const DavaScene& s, long long extra0 = 0) {
  if (DualTraits<T>::kGuardSizes && !sizes_sane(s)) return false;
  return carve_dual<T, 0>(s.num_views, s.num_points, round_up(s.num_parameters, 4)).total_bytes + extra0 <= kMaxLds;
}

// The form a scene takes: the lowest whose image fits kMaxLds -- form 0's is carve_dual's plus `extra0` bytes (the
// descent's adjoint appends its accumulator) -- raised (never lowered) by the type's override; -1 where not even
// form 2's image (the dual view constants and partials) fits.  (A form the override raises to always fits if the
// lower one did: each image is part of the one below.)
template <class T>
inline int choose_dual_form(const DavaScene& s, long long extra0 = 0) {
  if (DualTraits<T>::kGuardSizes && !sizes_sane(s)) return -1;
  const int M = s.num_views, N = s.num_points, Pv = round_up(s.num_parameters, 4);
  int form = 2;
  if (dual_fits_form0<T>(s, extra0)) form = 0;
  else if (carve_dual<T>(M, N, Pv, 1).total_bytes <= kMaxLds) form = 1;
  const long long forced = debug_knob(DualTraits<T>::kFormKnob);
  if ((forced == 1 || forced == 2) && forced > form) form = (int)forced;
  if (form == 2 && carve_dual<T>(M, N, Pv, 2).total_bytes > kMaxLds) return -1;
  return form;
}

}  // namespace dava
