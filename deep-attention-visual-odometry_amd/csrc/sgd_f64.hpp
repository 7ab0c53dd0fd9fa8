// What the float64 gradient descent (sgd_solve_f64.hip) and its adjoint (sgd_adjoint.hpp, through dual_image.hpp)
// share: the config check, the tape, and the update's arithmetic.
#pragma once

#include "ba_objective.hpp"
#include "dava_debug.hpp"
#include "dava_f64.hpp"

namespace dava {
namespace f64 {

// a - lr * b as torch forms it in float64: the product rounded, then the difference (never one FMA)
__device__ __forceinline__ double descend(double a, double lr, double b) {
#pragma clang fp contract(off)
  const double step = __dmul_rn(lr, b);
  return __dsub_rn(a, step);
}

inline int sgd_config_status(const DavaSgdConfigF64* c) {
  return !c || c->iterations < 0 ? DAVA_ERR_INVALID_ARGUMENT : DAVA_OK;
}

// The tape: x_k for k = 0 .. K-1, rows of Pv = round_up(P, 4) doubles, laid out (B, K, Pv) in every form.  No header.
inline size_t sgd_tape_bytes(int B, int K, int Pv) { return (size_t)B * (size_t)K * (size_t)Pv * sizeof(double); }

}  // namespace f64
}  // namespace dava
