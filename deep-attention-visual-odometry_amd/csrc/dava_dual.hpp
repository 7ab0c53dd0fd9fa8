// Forward-mode dual numbers for second derivatives of the BA objectives.
//
// The objective's reverse-mode gradient code (ba_objective.hpp) is templated on
// its scalar type; instantiated with Dual {value, tangent} and the parameters
// seeded with a direction v, the same code returns grad E (values) and the
// Hessian-vector product H v (tangents) -- forward-over-reverse, exactly the
// second derivative of the first derivative the solver uses.  This is what
// differentiating THROUGH a solve needs from the objective (the reference gets
// it from autograd's double backward, bfgs_solver.py:133-135 create_graph).
//
// The dual number is generic in its real type: Dual = DualT<float> for the fp32 kernels, Dual64 =
// DualT<double> for the float64 ones (ba_second_order.hpp and sgd_adjoint.hpp instantiate both;
// bfgs_adjoint_f64.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "dava_common.hpp"

namespace dava {

// ---- elementary functions of the real types (float, double); the dual ones below build on them ----
__device__ __forceinline__ float sqrt_(float x) { return sqrtf(x); }
__device__ __forceinline__ float sin_(float x) { return sinf(x); }
__device__ __forceinline__ float cos_(float x) { return cosf(x); }
__device__ __forceinline__ float fabs_(float x) { return fabsf(x); }
__device__ __forceinline__ float exp_(float x) { return expf(x); }
__device__ __forceinline__ float expm1_(float x) { return expm1f(x); }
__device__ __forceinline__ float atan2_(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ float fmul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float fadd_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float value_of(float x) { return x; }
// sin and cos of one argument through one range reduction
__device__ __forceinline__ void sincos_(float x, float& s, float& c) { sincosf(x, &s, &c); }

// double (the float64 objective): the correctly rounded add / multiply for trial points, as for float
__device__ __forceinline__ double sqrt_(double x) { return sqrt(x); }
__device__ __forceinline__ double sin_(double x) { return sin(x); }
__device__ __forceinline__ double cos_(double x) { return cos(x); }
__device__ __forceinline__ double fabs_(double x) { return fabs(x); }
__device__ __forceinline__ double exp_(double x) { return exp(x); }
__device__ __forceinline__ double expm1_(double x) { return expm1(x); }
__device__ __forceinline__ double atan2_(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ double fmul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double fadd_rn(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double value_of(double x) { return x; }
__device__ __forceinline__ void sincos_(double x, double& s, double& c) { sincos(x, &s, &c); }

// The operators are friends defined in the class (not templates), so a constant of another arithmetic type
// converts to R as it would for a plain struct: `1.0f - x` works for DualT<double> x as for DualT<float>.
template <typename R>
struct DualT {
  R v, t;
  __device__ __forceinline__ DualT() = default;
  __device__ __forceinline__ constexpr DualT(R value) : v(value), t(R(0)) {}  // NOLINT: constants
  __device__ __forceinline__ constexpr DualT(R value, R tangent) : v(value), t(tangent) {}

  friend __device__ __forceinline__ DualT operator+(DualT a, DualT b) { return {a.v + b.v, a.t + b.t}; }
  friend __device__ __forceinline__ DualT operator-(DualT a, DualT b) { return {a.v - b.v, a.t - b.t}; }
  friend __device__ __forceinline__ DualT operator-(DualT a) { return {-a.v, -a.t}; }
  friend __device__ __forceinline__ DualT operator*(DualT a, DualT b) { return {a.v * b.v, a.t * b.v + a.v * b.t}; }
  friend __device__ __forceinline__ DualT operator/(DualT a, DualT b) {
    const R q = a.v / b.v;
    return {q, (a.t - q * b.t) / b.v};
  }
  friend __device__ __forceinline__ DualT operator+(DualT a, R b) { return {a.v + b, a.t}; }
  friend __device__ __forceinline__ DualT operator+(R a, DualT b) { return {a + b.v, b.t}; }
  friend __device__ __forceinline__ DualT operator-(DualT a, R b) { return {a.v - b, a.t}; }
  friend __device__ __forceinline__ DualT operator-(R a, DualT b) { return {a - b.v, -b.t}; }
  friend __device__ __forceinline__ DualT operator*(DualT a, R b) { return {a.v * b, a.t * b}; }
  friend __device__ __forceinline__ DualT operator*(R a, DualT b) { return {a * b.v, a * b.t}; }
  friend __device__ __forceinline__ DualT operator/(DualT a, R b) { return {a.v / b, a.t / b}; }
  friend __device__ __forceinline__ DualT operator/(R a, DualT b) {
    const R q = a / b.v;
    return {q, -q * b.t / b.v};
  }
  friend __device__ __forceinline__ DualT& operator+=(DualT& a, DualT b) { return a = a + b; }
  friend __device__ __forceinline__ DualT& operator-=(DualT& a, DualT b) { return a = a - b; }
  friend __device__ __forceinline__ DualT& operator*=(DualT& a, DualT b) { return a = a * b; }
  // branches and clamps follow the value (their derivative is the taken branch's)
  friend __device__ __forceinline__ bool operator<(DualT a, DualT b) { return a.v < b.v; }
  friend __device__ __forceinline__ bool operator>(DualT a, DualT b) { return a.v > b.v; }
  friend __device__ __forceinline__ bool operator<=(DualT a, DualT b) { return a.v <= b.v; }
  friend __device__ __forceinline__ bool operator>=(DualT a, DualT b) { return a.v >= b.v; }
  friend __device__ __forceinline__ bool operator==(DualT a, DualT b) { return a.v == b.v; }
};
using Dual = DualT<float>;
using Dual64 = DualT<double>;

// The real type a scalar is built on: float for float and Dual, double for double and DualT<double>.  Step
// sizes, observations, reduction scratch and constants of the objective code have this type.
template <typename S>
struct RealOf {
  using type = float;
};
template <>
struct RealOf<double> {
  using type = double;
};
template <>
struct RealOf<DualT<double>> {
  using type = double;
};
template <typename S>
using real_t = typename RealOf<S>::type;

template <typename S>
struct IsDual {
  static constexpr bool value = false;
};
template <typename R>
struct IsDual<DualT<R>> {
  static constexpr bool value = true;
};

// ---- elementary functions of dual numbers ----
template <typename R>
__device__ __forceinline__ DualT<R> sqrt_(DualT<R> x) {
  const R r = sqrt_(x.v);
  return {r, r > R(0) ? x.t / (R(2) * r) : R(0)};  // torch: 0 subgradient handled by callers' norms
}
template <typename R>
__device__ __forceinline__ DualT<R> sin_(DualT<R> x) { return {sin_(x.v), cos_(x.v) * x.t}; }
template <typename R>
__device__ __forceinline__ DualT<R> cos_(DualT<R> x) { return {cos_(x.v), -sin_(x.v) * x.t}; }
template <typename R>
__device__ __forceinline__ DualT<R> fabs_(DualT<R> x) { return {fabs_(x.v), sgn(x.v) * x.t}; }
template <typename R>
__device__ __forceinline__ DualT<R> exp_(DualT<R> x) {
  const R e = exp_(x.v);
  return {e, e * x.t};
}
template <typename R>
__device__ __forceinline__ DualT<R> expm1_(DualT<R> x) { return {expm1_(x.v), exp_(x.v) * x.t}; }
template <typename R>
__device__ __forceinline__ DualT<R> atan2_(DualT<R> y, DualT<R> x) {
  const R den = x.v * x.v + y.v * y.v;
  return {atan2_(y.v, x.v), (x.v * y.t - y.v * x.t) / den};
}
template <typename R>
__device__ __forceinline__ void sincos_(DualT<R> x, DualT<R>& s, DualT<R>& c) {
  R sv, cv;
  sincos_(x.v, sv, cv);
  s = {sv, cv * x.t};
  c = {cv, -sv * x.t};
}
template <typename R>
__device__ __forceinline__ DualT<R> fmul_rn(DualT<R> a, DualT<R> b) { return a * b; }
template <typename R>
__device__ __forceinline__ DualT<R> fadd_rn(DualT<R> a, DualT<R> b) { return a + b; }
template <typename R>
__device__ __forceinline__ R value_of(DualT<R> x) { return x.v; }
// sign(x) as torch.abs backward uses it: piecewise constant, zero derivative
template <typename R>
__device__ __forceinline__ DualT<R> sgn(DualT<R> x) { return DualT<R>(sgn(x.v)); }
// (the bound in the dual's real type: a float constant such as kRayEps widens exactly)
__device__ __forceinline__ Dual clamp_min(Dual v, float lo) { return v.v < lo ? Dual(lo) : v; }
__device__ __forceinline__ DualT<double> clamp_min(DualT<double> v, double lo) {
  return v.v < lo ? DualT<double>(lo) : v;
}

template <>
__device__ __forceinline__ Dual wave_sum<Dual>(Dual x) {
  return {wave_sum<float>(x.v), wave_sum<float>(x.t)};
}
template <>
__device__ __forceinline__ DualT<double> wave_sum<DualT<double>>(DualT<double> x) {
  return {wave_sum<double>(x.v), wave_sum<double>(x.t)};
}

// block_sum over R duals = block_sum over the 2R floats they are made of
template <int R, int NW = kWaves>
__device__ __forceinline__ void block_sum(Dual (&v)[R], float* scratch, int buf) {
  static_assert(2 * R <= 32, "scratch rows hold 32 floats");
  block_sum<2 * R, NW>(reinterpret_cast<float(&)[2 * R]>(v), scratch, buf);
}
// ... and over R double duals = the deterministic double block_sum over their 2R doubles
template <int R, int NW = kWaves>
__device__ __forceinline__ void block_sum(DualT<double> (&v)[R], double* scratch, int buf) {
  static_assert(2 * R <= 32, "scratch rows hold 32 doubles");
  block_sum<2 * R, NW>(reinterpret_cast<double(&)[2 * R]>(v), scratch, buf);
}

}  // namespace dava
