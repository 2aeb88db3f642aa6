// bbq_jsmath.h - Math.min / Math.max / Math.round as V8 evaluates them, for the kernels that follow the JavaScript number model
// (the row quantizer of bbq_build_kernels.hip, the query quantizer of bbq_query_kernels.hip).  jmin / jmax are associative and
// commutative on everything but NaN payloads, signed zeros included: -0 wins a minimum, +0 a maximum.
#pragma once
#include <hip/hip_runtime.h>

namespace bbq {

__device__ __forceinline__ double jmin(double a, double b) {
  if (a != a || b != b) return __longlong_as_double(0x7ff8000000000000ll);
  if (a == 0.0 && b == 0.0) return (__double_as_longlong(a) < 0 || __double_as_longlong(b) < 0) ? -0.0 : 0.0;
  return a < b ? a : b;
}
__device__ __forceinline__ double jmax(double a, double b) {
  if (a != a || b != b) return __longlong_as_double(0x7ff8000000000000ll);
  if (a == 0.0 && b == 0.0) return (__double_as_longlong(a) < 0 && __double_as_longlong(b) < 0) ? -0.0 : 0.0;
  return a > b ? a : b;
}
__device__ __forceinline__ double jclamp(double x, double lo, double hi) { return jmin(jmax(x, lo), hi); }
__device__ __forceinline__ double jround(double x) {
  if (x != x || fabs(x) == __longlong_as_double(0x7ff0000000000000ll)) return x;
  double r = floor(x);
  if (x - r >= 0.5) r += 1.0;
  return r;
}

}  // namespace bbq
