// bbq_query_kernels.hip - searchNearestNeighbors' query preparation for a batch of raw fp32 queries on the device (gfx950), bit-exact:
// normalizeVector twice under COSINE (src/binaryQuantizationFormat.ts:337-347, src/vectorOperations.ts:11-34), the NaN / Infinity check
// and OptimizedScalarQuantizer.scalarQuantize at queryBits (src/optimizedScalarQuantizer.ts:108-227, getInitialInterval :245-265,
// optimizeIntervals :280-353, computeLoss :373-407) - what bbq_quantize_queries computes on host threads.
//
// One wave - a workgroup of 64 threads - per query; the query is read row-major as uploaded.  The reference accumulates every sum in
// index order in f64, and that order is part of the answer: each sum is a serial chain of `dim` dependent adds.  The TERMS of a chain do
// not depend on each other, so the kernel separates the two (chain_pass):
//   terms    lane l evaluates the terms of the elements 64 j + l of round j - the conversions, the clamp, jround, s, the products - and
//            stores them to LDS, one row of 64 f64 per chain of the phase
//   chains   lane c adds row c's values in index order into chain c's accumulator: the up to five chains of a phase advance in one
//            instruction stream, and every sum is the reference's sum.  The elements behind `dim` in the last round take part in no chain
//            (adding a zero is not neutral: -0 + 0 is +0)
// Only the minimum and the maximum of the f64 differences are wave reductions: jmin / jmax are associative on the finite values the
// validation leaves, signed zeros included (bbq_jsmath.h).  The centred vector - the reference's Float32Array - is computed once and stays
// in LDS.  Every exit of optimizeIntervals depends on chain results only, which every lane holds: no lane diverges.
//
// All arithmetic follows the JavaScript number model; -ffp-contract=off, IEEE f64 division and sqrt, f32 denormals kept.
#include <hip/hip_runtime.h>
#include <float.h>
#include "bbq_device.h"
#include "bbq_jsmath.h"
#include "bbq_launch.h"

#pragma clang fp contract(off)

namespace bbq {

// NC chains over the elements [0, dim): term(i, t) fills the NC terms of element i; returns with chain c's sum in EVERY lane's sums[c].
// rows: kQueryQuantChains rows of kQueryQuantRowStride f64.  Called by the whole wave.
template <int NC, class Term>
__device__ __forceinline__ void chain_pass(double *__restrict__ rows, int dim, int lane, Term term, double (&sums)[NC]) {
  double acc = 0.0;  // lane c < NC: chain c
  for (int i0 = 0; i0 < dim; i0 += 64) {
    double t[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = 0.0;
    if (i0 + lane < dim) term(i0 + lane, t);
#pragma unroll
    for (int c = 0; c < NC; ++c) rows[c * kQueryQuantRowStride + lane] = t[c];
    __syncthreads();
    if (lane < NC) {
      const double *__restrict__ row = rows + lane * kQueryQuantRowStride;
      if (dim - i0 >= 64) {
#pragma unroll 16
        for (int k = 0; k < 64; ++k) acc += row[k];
      } else {
        for (int k = 0; k < dim - i0; ++k) acc += row[k];
      }
    }
    __syncthreads();  // the next round overwrites the rows
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) sums[c] = __shfl(acc, c, 64);
}

// the quantization step of an element against the interval [a, b]: round((clamp(x) - a) * step_inv)
__device__ __forceinline__ double step_of(double xi, double a, double b, double step_inv) { return jround((jclamp(xi, a, b) - a) * step_inv); }

// computeLoss (:373-407) over the centred vector; pm1 = points - 1
__device__ __forceinline__ double loss_pass(double *rows, const float *w, int dim, int lane, double a, double b, double norm2, double lambda, double pm1) {
  const double step = (b - a) / pm1;
  const double step_inv = 1.0 / step;
  double s[2];
  chain_pass<2>(rows, dim, lane, [&](int i, double (&t)[2]) {
    const double xi = (double)w[i];
    const double xiq = a + step * step_of(xi, a, b, step_inv);
    t[0] = xi * (xi - xiq);
    t[1] = (xi - xiq) * (xi - xiq);
  }, s);
  return (1.0 - lambda) * s[0] * s[0] / norm2 + lambda * s[1];
}

// element store into a Uint8Array: ToUint8 (NaN and the infinities 0, otherwise the truncated value modulo 256)
__device__ __forceinline__ uint8_t to_uint8(double x) {
  if (!(fabs(x) <= DBL_MAX)) return 0;
  double m = fmod(trunc(x), 256.0);
  if (m < 0) m += 256.0;
  return (uint8_t)m;
}

__global__ __launch_bounds__(64) void bbq_quantize_queries_kernel(QueryQuantArgs a) {
  extern __shared__ double s_lds[];
  double *rows = s_lds;
  float *w = reinterpret_cast<float *>(s_lds + kQueryQuantChains * kQueryQuantRowStride);  // [ceil(dim / 64) * 64]
  const int lane = threadIdx.x, dim = a.dim;
  const int64_t q = blockIdx.x;
  const float *__restrict__ src = a.queries + q * (int64_t)dim;
  const float *__restrict__ cen = a.centroid;
  for (int i = lane; i < (dim + 63) / 64 * 64; i += 64) w[i] = i < dim ? src[i] : 0.f;  // lane l owns the elements 64 j + l from here on
  __syncthreads();

  // normalizeVector, twice on the search path (COSINE)
  if (a.sim == 1) {
    for (int r = 0; r < 2; ++r) {
      double n2[1];
      chain_pass<1>(rows, dim, lane, [&](int i, double (&t)[1]) { t[0] = (double)w[i] * (double)w[i]; }, n2);
      const double norm = sqrt(n2[0]);
      for (int i = lane; i < dim; i += 64) w[i] = norm == 0 ? 0.f : (float)((double)w[i] / norm);
    }
  }

  // scalarQuantize's validation (:138-148): the first NaN / Infinity of the vector it reads.  A lane meets its elements in ascending order
  uint32_t bad = 0xffffffffu;
  for (int i = lane; i < dim && bad == 0xffffffffu; i += 64) {
    const float v = w[i];
    if (!(fabsf(v) <= FLT_MAX)) bad = ((uint32_t)i << 1) | (v != v ? 0u : 1u);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, d, 64));
  if (bad != 0xffffffffu) {  // uniform: a bad query writes nothing else
    if (lane == 0) a.status[q] = ((bad & 1u ? kQueryQuantInf : kQueryQuantNaN) << 30) | (bad >> 1);
    return;
  }

  // :155-178: the centroid dot on the uncentred input, min / max of the f64 differences, the centred vector, the sum of its values
  const double ddim = (double)dim;
  double mn = DBL_MAX, mx = -DBL_MAX, s1[2];
  chain_pass<2>(rows, dim, lane, [&](int i, double (&t)[2]) {
    const double vd = (double)w[i], cd = (double)cen[i];
    t[0] = vd * cd;
    const double diff = vd - cd;
    mn = jmin(mn, diff);
    mx = jmax(mx, diff);
    const float wi = (float)diff;
    w[i] = wi;
    t[1] = (double)wi;
  }, s1);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = jmin(mn, __shfl_xor(mn, d, 64));
    mx = jmax(mx, __shfl_xor(mx, d, 64));
  }
  const double cdot = s1[0], mean = s1[1] / ddim;
  // :181-183: std and L2 norm of the centred vector
  double s2[2];
  chain_pass<2>(rows, dim, lane, [&](int i, double (&t)[2]) {
    const double wi = (double)w[i], dd = wi - mean;
    t[0] = dd * dd;
    t[1] = wi * wi;
  }, s2);
  const double sd = sqrt(s2[0] / ddim);
  const double norm2 = sqrt(s2[1]);
  const double kGrid[8] = {0.798, 1.493, 2.051, 2.514, 2.916, 3.278, 3.611, 3.922};  // MINIMUM_MSE_GRID, src/constants.ts:38-47
  const double g = kGrid[a.bits - 1];
  const double pm1 = (double)((1 << a.bits) - 1);  // points - 1
  const double lambda = a.lambda;
  double iv0 = jclamp(-g * sd + mean, mn, mx), iv1 = jclamp(g * sd + mean, mn, mx);

  // optimizeIntervals (:280-353); the 2 x 2 solve in the operation order of Quantizer::optimize (bbq_quantizer.cpp)
  {
    double best = loss_pass(rows, w, dim, lane, iv0, iv1, norm2, lambda, pm1);
    const double scale = (1.0 - lambda) / norm2;
    bool active = fabs(scale) <= DBL_MAX;  // isFinite(scale)
    for (int it = 0; it < a.iters && active; ++it) {
      const double lo = iv0, hi = iv1;
      const double step_inv = pm1 / (hi - lo);
      double d[5];  // daa, dab, dbb, dax, dbx
      chain_pass<5>(rows, dim, lane, [&](int i, double (&t)[5]) {
        const double xi = (double)w[i];
        const double s = step_of(xi, lo, hi, step_inv) / pm1;
        t[0] = (1.0 - s) * (1.0 - s);
        t[1] = (1.0 - s) * s;
        t[2] = s * s;
        t[3] = xi * (1.0 - s);
        t[4] = xi * s;
      }, d);
      const double m0 = scale * d[3] * d[3] + lambda * d[0];
      const double m1 = scale * d[3] * d[4] + lambda * d[1];
      const double m2 = scale * d[4] * d[4] + lambda * d[2];
      const double det = m0 * m2 - m1 * m1;
      if (fabs(det) < 1e-12) break;
      const double a_opt = (m2 * d[3] - m1 * d[4]) / det;
      const double b_opt = (m0 * d[4] - m1 * d[3]) / det;
      if (fabs(iv0 - a_opt) < 1e-8 && fabs(iv1 - b_opt) < 1e-8) break;
      const double nl = loss_pass(rows, w, dim, lane, a_opt, b_opt, norm2, lambda, pm1);
      if (nl > best) break;
      iv0 = a_opt;
      iv1 = b_opt;
      best = nl;
    }
  }

  // final pass (:192-216), the query form: one byte per dimension for every queryBits, the component sum adds the assignment as it is
  const double lo = iv0, hi = iv1;
  const double step = (hi - lo) / pm1;
  const double step_inv = step > 0 ? 1.0 / step : 0.0;
  const double thr = (lo + hi) / 2;
  const bool one_bit = a.bits == 1;
  uint8_t *__restrict__ dst = a.qquant + q * (int64_t)dim;
  double qsum[1];
  chain_pass<1>(rows, dim, lane, [&](int i, double (&t)[1]) {
    const double xi = (double)w[i];
    if (one_bit) {
      const int qv = jclamp(xi, lo, hi) >= thr ? 1 : 0;
      dst[i] = (uint8_t)qv;
      t[0] = (double)qv;
    } else {
      const double assignment = step_of(xi, lo, hi, step_inv);
      dst[i] = to_uint8(jmin(assignment, pm1));
      t[0] = assignment;
    }
  }, qsum);
  if (lane == 0) {
    double *cm = a.qcorr + q * 4;
    cm[0] = iv0; cm[1] = iv1; cm[2] = a.sim == 0 ? norm2 : cdot; cm[3] = qsum[0];
    a.status[q] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ launch wrapper

hipError_t launch_quantize_queries(const QueryQuantArgs &a, int n_queries, hipStream_t s) {
  if (n_queries <= 0) return hipSuccess;
  if (a.dim <= 0 || a.dim > kQueryQuantMaxDim || a.bits < 1 || a.bits > 8 || a.sim < 0 || a.sim > 2 || a.iters < 0) return hipErrorInvalidValue;
  if (!a.queries || !a.centroid || !a.qquant || !a.qcorr || !a.status) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bbq_quantize_queries_kernel, dim3((unsigned)n_queries), dim3(64), (size_t)query_quant_lds_bytes(a.dim), s, a);
  return hipGetLastError();
}

}  // namespace bbq
