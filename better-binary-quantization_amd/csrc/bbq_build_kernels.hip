// bbq_build_kernels.hip - every kernel that builds an index on the device (gfx950), and with that every kernel that WRITES tile records
// (their layout: bbq_device.h).  BinaryQuantizationFormat.quantizeVectors (reference src/binaryQuantizationFormat.ts:165-263) for every
// indexBits, bit-exact:
//
//   transpose_in   [n][dim] f32 (as uploaded)  ->  vT4[dim/4][npad] float4   (lane = vector => every later access is coalesced)
//   normalize      COSINE: normalizeVector (src/vectorOperations.ts:11-34), one thread per vector, f64 sum in index order
//   validate       first NaN / Infinity in row-major order (src/binaryQuantizationFormat.ts:196-211)
//   centroid       computeCentroid (src/vectorOperations.ts:126-163): the Float32Array accumulator is rounded after EVERY
//                  += and the sum runs over the vectors in order, so it is a serial chain per dimension; one wave per
//                  4 dimensions streams its vT4 row with coalesced 1 KiB loads and walks the 64 values through LDS broadcasts
//   quantize       OptimizedScalarQuantizer.scalarQuantize (src/optimizedScalarQuantizer.ts:108-227, getInitialInterval
//                  :245-265, optimizeIntervals :280-353, computeLoss :373-407), one thread per vector, every reduction in
//                  the reference's index order, f64 without FMA contraction; the last pass packs the bits
//                  (packAsBinary :420-446) straight into the scan kernel's tile records and writes the corrections
//   untile         tile records -> row-major packed rows (only when the host asks for the codes)
// and rows that arrive quantized, in the caller's shape:
//   retile         row-major rows (packed 1-bit, or one byte per dimension) + corrections -> tile records
//   check_x1       is every quantizedComponentSum the implied one (popcount / code sum)?   check_code_range: every multi-bit code in range?
//   scatter_rows   the same rows -> the lanes of the ords they replace, in place (bbq_index_update*)
//   tile_add_range compact layout: each tile's {min, max} of additionalCorrection, over a tile range or a tile list
//   tile_row_sums  compact layout: each row's popcount / code sum from its stored codes, over the same tile range or tile list
// and rows that are in tile records already:
//   compact_tiles  the records gathered down to the rows a filter accepts, out of place (bbq_index_compact)
// Every writer takes its destination as a TileDest and writes a row's corrections through write_corrections.
//
// All arithmetic follows the JavaScript number model; -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include "bbq_device.h"
#include "bbq_launch.h"

#pragma clang fp contract(off)

namespace bbq {

// Math.min / Math.max / Math.round as V8 evaluates them
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

// ------------------------------------------------------------------------------------------------ transpose_in
// block 256 threads: tile of 64 vectors x 16 float4 (64 dims) through LDS, both sides coalesced
__global__ __launch_bounds__(256) void bbq_transpose_in_kernel(const float *__restrict__ in, int64_t n, int32_t dim, int32_t dim4,
                                                              int64_t npad, f32x4 *__restrict__ vT4) {
  __shared__ f32x4 tile[64][17];
  const int64_t v0 = (int64_t)blockIdx.x * 64;
  const int i40 = blockIdx.y * 16;
  const int t = threadIdx.x;
  {
    const int c = t & 15;  // float4 column inside the tile
    const int i4 = i40 + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int vr = (t >> 4) + 16 * r;
      const int64_t vec = v0 + vr;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (vec < n && i4 < dim4) {
        const float *src = in + vec * (int64_t)dim + 4 * i4;
        if ((dim & 3) == 0) {
          x = *reinterpret_cast<const f32x4 *>(src);
        } else {
          if (4 * i4 + 0 < dim) x.x = src[0];
          if (4 * i4 + 1 < dim) x.y = src[1];
          if (4 * i4 + 2 < dim) x.z = src[2];
          if (4 * i4 + 3 < dim) x.w = src[3];
        }
      }
      tile[vr][c] = x;
    }
  }
  __syncthreads();
  {
    const int vr = t & 63;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = (t >> 6) + 4 * r;
      const int i4 = i40 + c;
      if (i4 < dim4 && v0 + vr < npad) vT4[(int64_t)i4 * npad + v0 + vr] = tile[vr][c];
    }
  }
}

// ------------------------------------------------------------------------------------------------ normalize (COSINE)
__global__ __launch_bounds__(256) void bbq_normalize_kernel(f32x4 *__restrict__ vT4, int64_t n, int32_t dim, int32_t dim4, int64_t npad) {
  const int64_t vec = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (vec >= n) return;
  double n2 = 0;
  for (int i4 = 0; i4 < dim4; ++i4) {
    const f32x4 v = vT4[(int64_t)i4 * npad + vec];
    n2 += (double)v.x * (double)v.x;
    if (4 * i4 + 1 < dim) n2 += (double)v.y * (double)v.y;
    if (4 * i4 + 2 < dim) n2 += (double)v.z * (double)v.z;
    if (4 * i4 + 3 < dim) n2 += (double)v.w * (double)v.w;
  }
  const double norm = sqrt(n2);
  for (int i4 = 0; i4 < dim4; ++i4) {
    f32x4 v = vT4[(int64_t)i4 * npad + vec];
    if (norm == 0) {
      v = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      v.x = (float)((double)v.x / norm);
      v.y = (4 * i4 + 1 < dim) ? (float)((double)v.y / norm) : 0.f;
      v.z = (4 * i4 + 2 < dim) ? (float)((double)v.z / norm) : 0.f;
      v.w = (4 * i4 + 3 < dim) ? (float)((double)v.w / norm) : 0.f;
    }
    vT4[(int64_t)i4 * npad + vec] = v;
  }
}

// ------------------------------------------------------------------------------------------------ validate
__global__ __launch_bounds__(256) void bbq_validate_kernel(const f32x4 *__restrict__ vT4, int64_t n, int32_t dim, int32_t dim4,
                                                          int64_t npad, unsigned long long *__restrict__ first_bad) {
  const int64_t vec = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int i4 = blockIdx.y;
  if (vec >= n) return;
  const f32x4 v = vT4[(int64_t)i4 * npad + vec];
  const float c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = 4 * i4 + k;
    if (d < dim && !(fabsf(c[k]) <= FLT_MAX)) {  // NaN or +-Infinity
      atomicMin(first_bad, (unsigned long long)(vec * (int64_t)dim + d));
      return;
    }
  }
}

// ------------------------------------------------------------------------------------------------ centroid
// one wave per float4 row (4 dimensions): serial, exactly rounded f32 accumulation over the vectors in order.
// The wave loads 64 consecutive vectors' values with one coalesced 1 KiB load, parks them in LDS and every lane walks
// them in order (uniform LDS reads broadcast); the next 1 KiB is already in flight while the chain runs.
__global__ __launch_bounds__(64) void bbq_centroid_kernel(const f32x4 *__restrict__ vT4, int64_t n, int32_t dim, int64_t npad,
                                                         float *__restrict__ centroid) {
  __shared__ f32x4 s_buf[2][64];
  const int i4 = blockIdx.x;
  const int lane = threadIdx.x;
  const f32x4 *__restrict__ row = vT4 + (int64_t)i4 * npad;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
  f32x4 x = row[lane];  // npad is a multiple of 64: always in bounds
  int pb = 0;
  for (int64_t j0 = 0; j0 < n; j0 += 64, pb ^= 1) {
    s_buf[pb][lane] = x;
    if (j0 + 64 < n) x = row[j0 + 64 + lane];  // prefetch
    __syncthreads();
    const int cnt = (int)((n - j0) < 64 ? (n - j0) : 64);
    for (int t = 0; t < cnt; ++t) {
      const f32x4 a = s_buf[pb][t];
      if (j0 == 0 && t == 0) {  // centroid[i] = vectors[0][i]
        c0 = a.x; c1 = a.y; c2 = a.z; c3 = a.w;
      } else {                  // centroid[i] += val  (Float32Array element: f64 add, then round to f32)
        c0 = (float)((double)c0 + (double)a.x);
        c1 = (float)((double)c1 + (double)a.y);
        c2 = (float)((double)c2 + (double)a.z);
        c3 = (float)((double)c3 + (double)a.w);
      }
    }
    // the other buffer is overwritten next iteration; every lane has finished reading it one iteration ago
  }
  if (lane == 0) {
    const double dn = (double)n;
    if (4 * i4 + 0 < dim) centroid[4 * i4 + 0] = (float)((double)c0 / dn);
    if (4 * i4 + 1 < dim) centroid[4 * i4 + 1] = (float)((double)c1 / dn);
    if (4 * i4 + 2 < dim) centroid[4 * i4 + 2] = (float)((double)c2 / dn);
    if (4 * i4 + 3 < dim) centroid[4 * i4 + 3] = (float)((double)c3 / dn);
  }
}

// ------------------------------------------------------------------------------------------------ the corrections of one row
// THE writer of a row's corrections (the tile record, bbq_device.h): lane row % 64 of the corrections block of tile row / 64.  Inline:
// {lower, upper}, additionalCorrection and - where the geometry stores it - the component sum.  Compact: the compact word, and the exact
// values in the side row exact[row] (the tiles' ranges of the additive term follow from there: bbq_tile_add_range_kernel).
__device__ __forceinline__ void write_corrections(const TileDest &out, int64_t row, f64x2 lu, double add, double x1) {
  const int r = (int)(row % kTileRows);
  uint8_t *cr = out.tiles + (row / kTileRows) * (int64_t)out.geom.tile_stride + tile_corr_offset(out.geom.w16);
  if (out.geom.layout == kLayoutCompact) {
    reinterpret_cast<uint32_t *>(cr)[r] = compact_word(lu.x, lu.y);
    double *e = out.exact + row * 4;
    e[0] = lu.x; e[1] = lu.y; e[2] = add; e[3] = 0.0;
  } else {
    reinterpret_cast<f64x2 *>(cr)[r] = lu;
    reinterpret_cast<double *>(cr + kCorrAddOffset)[r] = add;
    if (out.geom.has_x1) reinterpret_cast<double *>(cr + kCorrSumOffset)[r] = x1;
  }
}

// ------------------------------------------------------------------------------------------------ quantize (1 bit)

// one pass of computeLoss over the vector (src/optimizedScalarQuantizer.ts:373-407); pm1 = points - 1 = 2^bits - 1
__device__ __forceinline__ double loss_pass(const f32x4 *__restrict__ col, int64_t npad, const float *__restrict__ s_cen, int dim,
                                            int dim4, double a, double b, double norm2, double lambda, double pm1) {
  const double step = (b - a) / pm1;
  const double step_inv = 1.0 / step;
  double xe = 0.0, e = 0.0;
  for (int i4 = 0; i4 < dim4; ++i4) {
    const f32x4 v = col[(int64_t)i4 * npad];
    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = 4 * i4 + k;
      if (d < dim) {
        const double xi = (double)(float)((double)vv[k] - (double)s_cen[d]);
        const double kq = jround((jclamp(xi, a, b) - a) * step_inv);
        const double xiq = a + step * kq;
        xe += xi * (xi - xiq);
        e += (xi - xiq) * (xi - xiq);
      }
    }
  }
  return (1.0 - lambda) * xe * xe / norm2 + lambda * e;
}

// bits == 1 packs the row straight into the scan layout; bits > 1 writes what the reference keeps for such an index - one byte per
// dimension (src/binaryQuantizationFormat.ts:241-245) - to codes_rm, and the caller builds the tile records from that.
// Vector i becomes row row0 + i of the storage (row0 > 0: an append into the partly filled last tile; lanes below row0 are not
// touched).  n_out threads write: the n vectors and the padding lanes up to the end of the last tile - with row0 > 0 that can be
// more than npad, the columns of vT4, which only the valid threads read.
__global__ __launch_bounds__(256) void bbq_quantize1_kernel(const f32x4 *__restrict__ vT4, int64_t n, int32_t dim, int32_t dim4,
                                                           int64_t npad, const float *__restrict__ centroid, int32_t sim,
                                                           double lambda, int32_t iters, int32_t bits, TileDest out, double *__restrict__ corr_rm,
                                                           uint8_t *__restrict__ codes_rm, int64_t row0, int64_t n_out) {
  extern __shared__ float s_cen[];
  for (int i = threadIdx.x; i < dim4 * 4; i += 256) s_cen[i] = i < dim ? centroid[i] : 0.f;
  __syncthreads();
  const int64_t vec = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (vec >= n_out) return;
  const bool valid = vec < n;
  const f32x4 *__restrict__ col = vT4 + vec;
  const double ddim = (double)dim;

  // pass 1 (:155-178): centroid dot on the uncentred input, min/max of the f64 differences, sum of the f32 centred values
  double cdot = 0, mn = DBL_MAX, mx = -DBL_MAX, sum = 0;
  if (valid) {
    for (int i4 = 0; i4 < dim4; ++i4) {
      const f32x4 v = col[(int64_t)i4 * npad];
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int d = 4 * i4 + k;
        if (d < dim) {
          const double vd = (double)vv[k], cd = (double)s_cen[d];
          if (sim != 0) cdot += vd * cd;
          const double diff = vd - cd;
          mn = jmin(mn, diff);
          mx = jmax(mx, diff);
          sum += (double)(float)diff;
        }
      }
    }
  }
  const double mean = sum / ddim;
  // pass 2 (:181-183): std and L2 norm of the centred vector
  double var = 0, n2 = 0;
  if (valid) {
    for (int i4 = 0; i4 < dim4; ++i4) {
      const f32x4 v = col[(int64_t)i4 * npad];
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int d = 4 * i4 + k;
        if (d < dim) {
          const double w = (double)(float)((double)vv[k] - (double)s_cen[d]);
          const double dd = w - mean;
          var += dd * dd;
          n2 += w * w;
        }
      }
    }
  }
  const double sd = sqrt(var / ddim);
  const double norm2 = sqrt(n2);
  const double kGrid[8] = {0.798, 1.493, 2.051, 2.514, 2.916, 3.278, 3.611, 3.922};  // MINIMUM_MSE_GRID, src/constants.ts:38-47
  const double g = kGrid[bits - 1];
  const double pm1 = (double)((1 << bits) - 1);  // points - 1
  double iv0 = jclamp(-g * sd + mean, mn, mx), iv1 = jclamp(g * sd + mean, mn, mx);

  // optimizeIntervals (:280-353)
  {
    double best = valid ? loss_pass(col, npad, s_cen, dim, dim4, iv0, iv1, norm2, lambda, pm1) : 0.0;
    const double scale = (1.0 - lambda) / norm2;
    bool active = valid && (fabs(scale) <= DBL_MAX);  // isFinite(scale)
    for (int it = 0; it < iters; ++it) {
      if (!__any(active)) break;
      if (active) {
        const double a = iv0, b = iv1;
        const double step_inv = pm1 / (b - a);  // (points - 1) / (b - a)
        double daa = 0, dab = 0, dbb = 0, dax = 0, dbx = 0;
        for (int i4 = 0; i4 < dim4; ++i4) {
          const f32x4 v = col[(int64_t)i4 * npad];
          const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int d = 4 * i4 + k;
            if (d < dim) {
              const double xi = (double)(float)((double)vv[k] - (double)s_cen[d]);
              const double kq = jround((jclamp(xi, a, b) - a) * step_inv);
              const double s = kq / pm1;
              daa += (1.0 - s) * (1.0 - s);
              dab += (1.0 - s) * s;
              dbb += s * s;
              dax += xi * (1.0 - s);
              dbx += xi * s;
            }
          }
        }
        const double m0 = scale * dax * dax + lambda * daa;
        const double m1 = scale * dax * dbx + lambda * dab;
        const double m2 = scale * dbx * dbx + lambda * dbb;
        const double det = m0 * m2 - m1 * m1;
        if (fabs(det) < 1e-12) {
          active = false;
        } else {
          const double a_opt = (m2 * dax - m1 * dbx) / det;
          const double b_opt = (m0 * dbx - m1 * dax) / det;
          if (fabs(iv0 - a_opt) < 1e-8 && fabs(iv1 - b_opt) < 1e-8) {
            active = false;
          } else {
            const double nl = loss_pass(col, npad, s_cen, dim, dim4, a_opt, b_opt, norm2, lambda, pm1);
            if (nl > best) {
              active = false;
            } else {
              iv0 = a_opt;
              iv1 = b_opt;
              best = nl;
            }
          }
        }
      }
    }
  }

  if (bits > 1) {
    // final pass (:192-216) for more than one bit: assignment = round((clamp(x) - a) * stepInv), dest = min(assignment, nSteps), the
    // component sum adds the assignment as it is
    const double a = iv0, b = iv1;
    const double step = (b - a) / pm1;
    const double step_inv = step > 0 ? 1.0 / step : 0.0;
    double qsum = 0;
    if (valid) {
      uint8_t *__restrict__ dst = codes_rm + vec * (int64_t)dim;
      for (int i4 = 0; i4 < dim4; ++i4) {
        const f32x4 v = col[(int64_t)i4 * npad];
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int d = 4 * i4 + k;
          if (d < dim) {
            const double xi = (double)(float)((double)vv[k] - (double)s_cen[d]);
            const double assignment = jround((jclamp(xi, a, b) - a) * step_inv);
            qsum += assignment;
            const double capped = jmin(assignment, pm1);
            // Uint8Array store of a double: ToUint8 (NaN -> 0, otherwise modulo 256 of the truncated value)
            dst[d] = (capped != capped) ? (uint8_t)0 : (uint8_t)(unsigned int)(long long)capped;
          }
        }
      }
      double *cm = corr_rm + vec * 4;
      cm[0] = iv0; cm[1] = iv1; cm[2] = (sim == 0) ? norm2 : cdot; cm[3] = qsum;
    }
    return;
  }

  // final pass (:192-216): 1-bit threshold at the interval midpoint, packed MSB-first (packAsBinary :420-446) straight into
  // the row's code chunks of its tile record
  const int64_t row = row0 + vec;
  const int r = (int)(row % kTileRows);
  uint8_t *tp = out.tiles + (row / kTileRows) * (int64_t)out.geom.tile_stride;
  const double a = iv0, b = iv1;
  const double thr = (a + b) / 2;
  double qsum = 0;
  uint32_t wcur = 0;
  u32x4 chunk = {0, 0, 0, 0};
  for (int i4 = 0; i4 < out.geom.w16 * 32; ++i4) {
    if (valid && i4 < dim4) {
      const f32x4 v = col[(int64_t)i4 * npad];
      const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int d = 4 * i4 + k;
        if (d < dim) {
          const double xi = (double)(float)((double)vv[k] - (double)s_cen[d]);
          if (jclamp(xi, a, b) >= thr) {
            wcur |= 1u << (8 * ((d >> 3) & 3) + 7 - (d & 7));
            qsum += 1.0;
          }
        }
      }
    }
    if ((i4 & 7) == 7) {  // 32 dims = one little-endian 32-bit word of the packed row
      const int wi = (i4 >> 3) & 3;
      if (wi == 0) chunk.x = wcur; else if (wi == 1) chunk.y = wcur; else if (wi == 2) chunk.z = wcur; else chunk.w = wcur;
      wcur = 0;
      if (wi == 3) {
        reinterpret_cast<u32x4 *>(tp)[tile_chunk_index(i4 >> 5, r)] = chunk;
        chunk = u32x4{0, 0, 0, 0};
      }
    }
  }
  f64x2 lu = {0.0, 0.0};
  double add = 0;
  if (valid) {
    lu.x = iv0;
    lu.y = iv1;
    add = (sim == 0) ? norm2 : cdot;  // :219
  }
  write_corrections(out, row, lu, add, qsum);  // the component sum of a freshly quantized row is its popcount: a geometry with has_x1 = 0 drops it
  if (corr_rm && valid) {
    double *cm = corr_rm + vec * 4;
    cm[0] = lu.x; cm[1] = lu.y; cm[2] = add; cm[3] = qsum;
  }
}

// ------------------------------------------------------------------------------------------------ retile (rows in the caller's shape)
// row-major rows (StagedRows) -> tile records.  One thread per (row, chunk), one more per row for its corrections.
// The rows handed over are the global rows [row0, n_rows) (row0 = 0: a creation; row0 = the old size: an append, DESIGN.md
// "Appending rows"): thread (i, j) owns global row row0 + i, lanes below row0 are not touched, lanes from n_rows up to the end of the
// last tile are written as padding.  The two row shapes differ only in how a 16-byte chunk is packed: a packed 1-bit row is copied,
// a multi-bit row (one byte per dimension) is packed into store_bits-wide fields, and a code that is not below 2^index_bits raises
// *bad (the index is refused).
__global__ __launch_bounds__(256) void bbq_retile_kernel(TileDest out, StagedRows in, int64_t n_rows, int64_t n_rows_padded, int64_t row0,
                                                        int32_t index_bits, uint32_t *__restrict__ bad) {
  const int w16 = out.geom.w16;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = row0 + gid / (w16 + 1);
  const int j = (int)(gid % (w16 + 1));
  if (row >= n_rows_padded) return;
  const bool valid = row < n_rows;
  if (j == w16) {
    f64x2 lu = {0.0, 0.0};
    double add = 0.0, x1 = 0.0;
    if (valid) {
      const double *c = in.corr + (row - row0) * 4;
      lu.x = c[0]; lu.y = c[1]; add = c[2]; x1 = c[3];
    }
    write_corrections(out, row, lu, add, x1);
    return;
  }
  uint32_t w[4] = {0, 0, 0, 0};
  if (valid && out.geom.store_bits == 1) {
    const int pb = pb_of(out.geom);
    const uint8_t *src = in.codes + (row - row0) * (int64_t)pb;
    for (int b = 0; b < 16; ++b) {
      const int byte = j * 16 + b;
      if (byte < pb) w[b >> 2] |= (uint32_t)src[byte] << (8 * (b & 3));
    }
  } else if (valid) {
    const int dim = out.geom.dim, store_bits = out.geom.store_bits, per_dword = 32 / store_bits;
    const uint8_t *src = in.codes + (row - row0) * (int64_t)dim;
    const uint32_t limit = 1u << index_bits, field = (1u << store_bits) - 1u;  // values of an indexBits-bit quantizer are < 2^indexBits (include/bbq.h)
    for (int t = 0; t < 4; ++t)
      for (int f = 0; f < per_dword; ++f) {
        const int d = (j * 4 + t) * per_dword + f;
        if (d < dim) {
          const uint32_t v = src[d];
          if (v >= limit) atomicOr(bad, 1u);
          w[t] |= (v & field) << (f * store_bits);
        }
      }
  }
  const u32x4 v = {w[0], w[1], w[2], w[3]};
  reinterpret_cast<u32x4 *>(out.tiles + (row / kTileRows) * (int64_t)out.geom.tile_stride)[tile_chunk_index(j, (int)(row % kTileRows))] = v;
}

// ------------------------------------------------------------------------------------------------ scatter (rows replaced in place)
// bbq_retile_kernel with a row map (DESIGN.md "Replacing rows"): staged row pos[i] becomes row ords[pos[i]] of the storage.  pos lists
// the block's winners - one per distinct ord, ascending by ord (bbq_update_winners) - so every destination lane has exactly one writer
// and no ordering between workgroups is needed; neighbouring threads write neighbouring lanes of one tile wherever neighbouring ords are
// updated.  Thread (i, j) writes chunk j, one more thread per row its corrections.  Only the winners' lanes are written: no padding
// lane, no lane of a row that is not named.  The host has validated the ords and, for multi-bit rows, the code range before the launch
// (nothing of a refused block reaches the index): `bad` is the packer's and stays clear.
// 16-byte chunk j of staged row i, as the tile records hold it (w starts as zeros): a packed 1-bit row is copied, a multi-bit row (one
// byte per dimension) is packed into store_bits-wide fields, and a code that is not below 2^index_bits raises *bad.  The packing of
// bbq_retile_kernel, which keeps its own copy: called from there the function changed that kernel's instruction stream (DESIGN.md
// "Replacing rows").
__device__ __forceinline__ void pack_row_chunk(const TileGeom &g, const StagedRows &in, int64_t i, int j, int32_t index_bits,
                                               uint32_t *__restrict__ bad, uint32_t (&w)[4]) {
  if (g.store_bits == 1) {
    const int pb = pb_of(g);
    const uint8_t *src = in.codes + i * (int64_t)pb;
    for (int b = 0; b < 16; ++b) {
      const int byte = j * 16 + b;
      if (byte < pb) w[b >> 2] |= (uint32_t)src[byte] << (8 * (b & 3));
    }
  } else {
    const int dim = g.dim, store_bits = g.store_bits, per_dword = 32 / store_bits;
    const uint8_t *src = in.codes + i * (int64_t)dim;
    const uint32_t limit = 1u << index_bits, field = (1u << store_bits) - 1u;  // values of an indexBits-bit quantizer are < 2^indexBits (include/bbq.h)
    for (int t = 0; t < 4; ++t)
      for (int f = 0; f < per_dword; ++f) {
        const int d = (j * 4 + t) * per_dword + f;
        if (d < dim) {
          const uint32_t v = src[d];
          if (v >= limit) atomicOr(bad, 1u);
          w[t] |= (v & field) << (f * store_bits);
        }
      }
  }
}

__global__ __launch_bounds__(256) void bbq_scatter_rows_kernel(TileDest out, StagedRows in, const int32_t *__restrict__ ords,
                                                              const int64_t *__restrict__ pos, int64_t n_winners, int32_t index_bits,
                                                              uint32_t *__restrict__ bad) {
  const int w16 = out.geom.w16;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = gid / (w16 + 1);
  const int j = (int)(gid % (w16 + 1));
  if (i >= n_winners) return;
  const int64_t p = pos[i], row = ords[p];
  if (j == w16) {
    const double *c = in.corr + p * 4;
    write_corrections(out, row, f64x2{c[0], c[1]}, c[2], c[3]);
    return;
  }
  uint32_t w[4] = {0, 0, 0, 0};
  pack_row_chunk(out.geom, in, p, j, index_bits, bad, w);
  const u32x4 v = {w[0], w[1], w[2], w[3]};
  *reinterpret_cast<u32x4 *>(out.tiles + (row / kTileRows) * (int64_t)out.geom.tile_stride + tile_chunk_offset(j, (int)(row % kTileRows))) = v;
}

// does quantizedComponentSum equal the row's implied sum everywhere (then it need not be stored)?  The implied sum of a packed 1-bit row
// is its popcount, of a multi-bit row (one byte per dimension) the sum of its codes: over the row_bytes bytes of the row either way
__global__ __launch_bounds__(256) void bbq_check_x1_kernel(StagedRows in, int64_t n_rows, int32_t row_bytes, int32_t popcount,
                                                          uint32_t *__restrict__ mismatch) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  const uint8_t *src = in.codes + row * (int64_t)row_bytes;
  uint32_t sum = 0;
  for (int b = 0; b < row_bytes; ++b) sum += popcount ? (uint32_t)__popc((uint32_t)src[b]) : (uint32_t)src[b];
  if (!(in.corr[row * 4 + 3] == (double)sum)) atomicOr(mismatch, 1u);
}

// compact layout: {min, max} of additionalCorrection over the valid rows of each tile, as f32 (one wave per tile; the f32
// rounding is inside the bound's allowance for the additive term).  A NaN anywhere makes both ends NaN: no bound, exact path.
// The per-tile body, one wave per tile, shared by the two kernels below.
__device__ __forceinline__ void tile_add_range(const double *__restrict__ exact, int64_t n_rows, float *__restrict__ add_range, int64_t tile, int lane) {
  const int64_t row = tile * kTileRows + lane;
  const bool valid = row < n_rows;
  const double v = valid ? exact[row * 4 + 2] : 0.0;
  bool nan = valid && (v != v);
  double lo = valid ? v : __longlong_as_double(0x7ff0000000000000ll), hi = valid ? v : __longlong_as_double(0xfff0000000000000ll);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, d, 64));
    hi = fmax(hi, __shfl_xor(hi, d, 64));
  }
  nan = __any(nan);
  if (lane == 0) {
    add_range[tile * 2] = nan ? __uint_as_float(0x7fc00000u) : (float)lo;
    add_range[tile * 2 + 1] = nan ? __uint_as_float(0x7fc00000u) : (float)hi;
  }
}
// Runs over the tiles [tile0, ceil(n_rows / 64)): an append starts at the tile its first new row lands in.
__global__ __launch_bounds__(256) void bbq_tile_add_range_kernel(const double *__restrict__ exact, int64_t n_rows, float *__restrict__ add_range,
                                                                 int64_t tile0) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = tile0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t n_tiles = (n_rows + kTileRows - 1) / kTileRows;
  if (tile >= n_tiles) return;
  tile_add_range(exact, n_rows, add_range, tile, lane);
}
// the same for the tiles listed (an update: the distinct tiles of the rows it replaced, each below ceil(n_rows / 64)); one wave per tile
__global__ __launch_bounds__(256) void bbq_tile_add_range_list_kernel(const double *__restrict__ exact, int64_t n_rows, float *__restrict__ add_range,
                                                                      const int64_t *__restrict__ tiles, int64_t n_listed) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_listed) return;  // uniform per wave
  tile_add_range(exact, n_rows, add_range, tiles[t], threadIdx.x & 63);
}

// compact layout: row_sums[row] = the row's popcount (1-bit rows) or the sum of its store_bits-wide fields, over all w16 chunks of the
// stored record (the padding behind the last dimension is zero) - the integer the sweep's own sum chain returns for the row
// (tile_popcounts, tile_dot_multibit), as uint16: the array exists only where every sum fits (row_sums_fit).  One wave per tile, lane l
// owns row 64 tile + l; lanes at and beyond n_rows get 0.
__device__ __forceinline__ void tile_row_sums(const TileDest &src, int64_t n_rows, uint16_t *__restrict__ row_sums, int64_t tile, int lane) {
  const u32x4 *__restrict__ cp = reinterpret_cast<const u32x4 *>(src.tiles + tile * (int64_t)src.geom.tile_stride);
  const int sb = src.geom.store_bits;
  const uint32_t mask = (1u << sb) - 1u;
  uint32_t sum = 0;
  for (int j = 0; j < src.geom.w16; ++j) {
    const u32x4 c = cp[tile_chunk_index(j, lane)];
    const uint32_t x[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (sb == 1) sum += (uint32_t)__popc(x[t]);
      else
        for (int f = 0; f < 32; f += sb) sum += (x[t] >> f) & mask;
    }
  }
  const int64_t row = tile * kTileRows + lane;
  row_sums[row] = row < n_rows ? (uint16_t)sum : (uint16_t)0;
}
__global__ __launch_bounds__(256) void bbq_tile_row_sums_kernel(TileDest src, int64_t n_rows, uint16_t *__restrict__ row_sums, int64_t tile0) {
  const int64_t tile = tile0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= (n_rows + kTileRows - 1) / kTileRows) return;
  tile_row_sums(src, n_rows, row_sums, tile, threadIdx.x & 63);
}
__global__ __launch_bounds__(256) void bbq_tile_row_sums_list_kernel(TileDest src, int64_t n_rows, uint16_t *__restrict__ row_sums,
                                                                     const int64_t *__restrict__ tiles, int64_t n_listed) {
  const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n_listed) return;  // uniform per wave
  tile_row_sums(src, n_rows, row_sums, tiles[t], threadIdx.x & 63);
}

// is every code of these multi-bit rows below 2^index_bits?  What bbq_retile_kernel reports while it writes, asked BEFORE
// anything is written: an append that fails leaves the index as it was
__global__ __launch_bounds__(256) void bbq_check_code_range_kernel(const uint8_t *__restrict__ codes, int64_t count, uint32_t limit,
                                                                   uint32_t *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count && codes[i] >= limit) atomicOr(bad, 1u);
}

// ------------------------------------------------------------------------------------------------ untile (codes for the host)
__global__ __launch_bounds__(256) void bbq_untile_kernel(TileDest src, int64_t n, uint8_t *__restrict__ codes_rm, int64_t row0) {
  const int w16 = src.geom.w16, pb = pb_of(src.geom);
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i = gid / w16;  // row row0 + i of the storage -> row i of codes_rm
  const int j = (int)(gid % w16);
  if (i >= n) return;
  const int64_t row = row0 + i;
  const uint8_t *tp = src.tiles + (row / kTileRows) * (int64_t)src.geom.tile_stride;
  const u32x4 c = reinterpret_cast<const u32x4 *>(tp)[tile_chunk_index(j, (int)(row % kTileRows))];
  const uint32_t w[4] = {c.x, c.y, c.z, c.w};
  uint8_t *dst = codes_rm + i * (int64_t)pb;
  for (int b = 0; b < 16; ++b) {
    const int byte = j * 16 + b;
    if (byte < pb) dst[byte] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
  }
}

// ------------------------------------------------------------------------------------------------ compact (tile records -> tile records)
// The records of `src` gathered down to the rows a filter accepts (DESIGN.md "Removing rows"), out of place: a destination row never
// lies behind its source row, so in place one workgroup would overwrite a tile another still has to read.  One wave per destination
// tile, lane l owns new row 64 T + l: it finds its old row (compact_source_row, bbq_device.h), gathers the row's w16 code chunks -
// 16-byte loads that are neighbours in the source wherever neighbours are kept, read once and therefore non-temporal; each store
// is 1 KiB per wave, coalesced - and its corrections, which go out through write_corrections: the compact word is the same function of
// {lower, upper} it was when the row was first written.  Lanes from `kept` to the end of the last tile are padding, as
// bbq_retile_kernel leaves them.  src and out share one geometry.
__global__ __launch_bounds__(256) void bbq_compact_tiles_kernel(TileDest out, TileDest src, CompactMap map) {
  const int lane = threadIdx.x & 63, w16 = out.geom.w16;
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t R0 = tile * kTileRows, R = R0 + lane;
  if (R0 >= map.kept) return;  // uniform per wave: grid padding
  const bool valid = R < map.kept;
  const int64_t srow = valid ? compact_source_row(map, R0, R) : 0;
  const uint8_t *sp = src.tiles + (srow / kTileRows) * (int64_t)src.geom.tile_stride;
  const int sl = (int)(srow % kTileRows);
  u32x4 *dp = reinterpret_cast<u32x4 *>(out.tiles + tile * (int64_t)out.geom.tile_stride);
  for (int j = 0; j < w16; ++j) {
    u32x4 c = {0, 0, 0, 0};
    if (valid) c = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(sp) + tile_chunk_index(j, sl));
    dp[tile_chunk_index(j, lane)] = c;
  }
  f64x2 lu = {0.0, 0.0};
  double add = 0.0, x1 = 0.0;
  if (valid) {
    if (src.geom.layout == kLayoutCompact) {
      const double *e = src.exact + srow * 4;
      lu = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(e));
      add = __builtin_nontemporal_load(e + 2);
    } else {
      const uint8_t *cr = sp + tile_corr_offset(w16);
      lu = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(cr) + sl);
      add = __builtin_nontemporal_load(reinterpret_cast<const double *>(cr + kCorrAddOffset) + sl);
      if (src.geom.has_x1) x1 = __builtin_nontemporal_load(reinterpret_cast<const double *>(cr + kCorrSumOffset) + sl);
    }
  }
  write_corrections(out, R, lu, add, x1);
}

// ------------------------------------------------------------------------------------------------ launch wrappers

hipError_t launch_build_transpose(const float *in, int64_t n, int32_t dim, int64_t npad, float *vT4, hipStream_t s) {
  const int dim4 = (dim + 3) / 4;
  dim3 grid((unsigned)(npad / 64), (unsigned)((dim4 + 15) / 16));
  hipLaunchKernelGGL(bbq_transpose_in_kernel, grid, dim3(256), 0, s, in, n, dim, dim4, npad, reinterpret_cast<f32x4 *>(vT4));
  return hipGetLastError();
}
hipError_t launch_build_normalize(float *vT4, int64_t n, int32_t dim, int64_t npad, hipStream_t s) {
  const int dim4 = (dim + 3) / 4;
  hipLaunchKernelGGL(bbq_normalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<f32x4 *>(vT4), n, dim, dim4, npad);
  return hipGetLastError();
}
hipError_t launch_build_validate(const float *vT4, int64_t n, int32_t dim, int64_t npad, unsigned long long *first_bad, hipStream_t s) {
  const int dim4 = (dim + 3) / 4;
  dim3 grid((unsigned)((n + 255) / 256), (unsigned)dim4);
  hipLaunchKernelGGL(bbq_validate_kernel, grid, dim3(256), 0, s, reinterpret_cast<const f32x4 *>(vT4), n, dim, dim4, npad, first_bad);
  return hipGetLastError();
}
hipError_t launch_build_centroid(const float *vT4, int64_t n, int32_t dim, int64_t npad, float *centroid, hipStream_t s) {
  const int dim4 = (dim + 3) / 4;
  hipLaunchKernelGGL(bbq_centroid_kernel, dim3((unsigned)dim4), dim3(64), 0, s, reinterpret_cast<const f32x4 *>(vT4), n, dim, npad, centroid);
  return hipGetLastError();
}
hipError_t launch_build_quantize1(const float *vT4, int64_t n, int64_t npad, const float *centroid, int32_t sim, double lambda, int32_t iters,
                                  const TileDest &out, double *corr_rm, hipStream_t s, int64_t row0) {
  const int dim = out.geom.dim, dim4 = (dim + 3) / 4;
  const int64_t n_out = (row0 + n + kTileRows - 1) / kTileRows * kTileRows - row0;  // row0 = 0: npad
  hipLaunchKernelGGL(bbq_quantize1_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), (size_t)dim4 * 16, s,
                     reinterpret_cast<const f32x4 *>(vT4), n, dim, dim4, npad, centroid, sim, lambda, iters, 1, out, corr_rm, (uint8_t *)nullptr, row0, n_out);
  return hipGetLastError();
}
hipError_t launch_build_quantize_bits(const float *vT4, int64_t n, int32_t dim, int64_t npad, const float *centroid, int32_t sim,
                                      double lambda, int32_t iters, int32_t bits, uint8_t *codes_rm, double *corr_rm, hipStream_t s) {
  const int dim4 = (dim + 3) / 4;
  hipLaunchKernelGGL(bbq_quantize1_kernel, dim3((unsigned)(npad / 256 + (npad % 256 ? 1 : 0))), dim3(256), (size_t)dim4 * 16, s,
                     reinterpret_cast<const f32x4 *>(vT4), n, dim, dim4, npad, centroid, sim, lambda, iters, bits, TileDest{}, corr_rm, codes_rm, (int64_t)0, npad);
  return hipGetLastError();
}
hipError_t launch_build_untile(const TileDest &src, int64_t n, uint8_t *codes_rm, hipStream_t s, int64_t row0) {
  const int64_t threads = n * src.geom.w16;
  if (threads <= 0) return hipSuccess;
  hipLaunchKernelGGL(bbq_untile_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, src, n, codes_rm, row0);
  return hipGetLastError();
}

hipError_t launch_retile(const TileDest &out, const StagedRows &in, int64_t n_rows, int64_t row0, int32_t index_bits, uint32_t *bad, hipStream_t s) {
  const int64_t n_pad = (n_rows + kTileRows - 1) / kTileRows * kTileRows;
  const int64_t threads = (n_pad - row0) * (out.geom.w16 + 1);
  if (threads <= 0) return hipSuccess;
  hipLaunchKernelGGL(bbq_retile_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, out, in, n_rows, n_pad, row0, index_bits, bad);
  return hipGetLastError();
}

hipError_t launch_compact_tiles(const TileDest &out, const TileDest &src, const CompactMap &map, hipStream_t s) {
  const int64_t n_tiles = (map.kept + kTileRows - 1) / kTileRows;
  if (n_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(bbq_compact_tiles_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, s, out, src, map);
  return hipGetLastError();
}

hipError_t launch_check_x1(const StagedRows &in, int64_t n_rows, const TileGeom &g, uint32_t *mismatch, hipStream_t s) {
  if (n_rows == 0) return hipSuccess;
  const bool packed = g.store_bits == 1;
  hipLaunchKernelGGL(bbq_check_x1_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, in, n_rows, packed ? pb_of(g) : g.dim, packed ? 1 : 0, mismatch);
  return hipGetLastError();
}

hipError_t launch_tile_add_range(const double *exact, int64_t n_rows, float *add_range, hipStream_t s, int64_t tile0) {
  const int64_t n_tiles = (n_rows + kTileRows - 1) / kTileRows - tile0;
  if (n_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(bbq_tile_add_range_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, s, exact, n_rows, add_range, tile0);
  return hipGetLastError();
}

hipError_t launch_scatter_rows(const TileDest &out, const StagedRows &in, const int32_t *ords, const int64_t *pos, int64_t n_winners,
                               int32_t index_bits, uint32_t *bad, hipStream_t s) {
  const int64_t threads = n_winners * (out.geom.w16 + 1);
  if (threads <= 0) return hipSuccess;
  hipLaunchKernelGGL(bbq_scatter_rows_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, out, in, ords, pos, n_winners, index_bits, bad);
  return hipGetLastError();
}

hipError_t launch_tile_add_range_list(const double *exact, int64_t n_rows, float *add_range, const int64_t *tiles, int64_t n_listed, hipStream_t s) {
  if (n_listed <= 0) return hipSuccess;
  hipLaunchKernelGGL(bbq_tile_add_range_list_kernel, dim3((unsigned)((n_listed + 3) / 4)), dim3(256), 0, s, exact, n_rows, add_range, tiles, n_listed);
  return hipGetLastError();
}

hipError_t launch_tile_row_sums(const TileDest &src, int64_t n_rows, uint16_t *row_sums, hipStream_t s, int64_t tile0) {
  const int64_t n_tiles = (n_rows + kTileRows - 1) / kTileRows - tile0;
  if (n_tiles <= 0 || !row_sums) return hipSuccess;
  hipLaunchKernelGGL(bbq_tile_row_sums_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, s, src, n_rows, row_sums, tile0);
  return hipGetLastError();
}

hipError_t launch_tile_row_sums_list(const TileDest &src, int64_t n_rows, uint16_t *row_sums, const int64_t *tiles, int64_t n_listed, hipStream_t s) {
  if (n_listed <= 0 || !row_sums) return hipSuccess;
  hipLaunchKernelGGL(bbq_tile_row_sums_list_kernel, dim3((unsigned)((n_listed + 3) / 4)), dim3(256), 0, s, src, n_rows, row_sums, tiles, n_listed);
  return hipGetLastError();
}

hipError_t launch_check_code_range(const uint8_t *codes, int64_t count, int32_t index_bits, uint32_t *bad, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(bbq_check_code_range_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, codes, count, 1u << index_bits, bad);
  return hipGetLastError();
}

}  // namespace bbq
