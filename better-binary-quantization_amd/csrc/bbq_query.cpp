// bbq_query.cpp - query staging: bit-planes and multi-bit dwords, the int8 and FP6 MFMA operands, and the checks of a call's query
// arguments.
#include <float.h>
#include <math.h>
#include <string.h>
#include "bbq_search.h"

namespace bbq {

// per query: bit-planes (up to 8) + digit masks (4-plane queries) + int8 values in MFMA fragment order + score uniforms + group maxima
int64_t qbuf_bytes_per_query_w(int w16) {
  return (int64_t)w16 * 8 * 16 + digit_bytes_per_query_w(w16) + (int64_t)w16 * 128 + (int64_t)sizeof(QueryParams) + 16;
}
int64_t digit_bytes_per_query_w(int w16) { return (int64_t)w16 * kDigitMasks * 16; }

int max_value(const uint8_t *q, int64_t count) {
  uint8_t m = 0;
  for (int64_t i = 0; i < count; ++i) m = std::max(m, q[i]);
  return m;
}

static int planes_for(const uint8_t *q, int64_t count) {
  uint8_t m = 0;
  for (int64_t i = 0; i < count; ++i) m |= q[i];
  if (m <= 1) return 1;
  if (m <= 3) return 2;
  if (m <= 15) return 4;
  return 8;
}

// bytes of staged query data per query (bit-planes, or the nibble / byte dwords of a multi-bit index)
int64_t query_data_bytes(const bbq_index *ix, int planes) { return (int64_t)ix->geom.w16 * query_units_per_chunk(planes, ix->geom.store_bits) * 16; }

// kernel variant for a call: 1-bit index -> number of bit-planes the query values need; multi-bit index -> 4 (values <= 15: low
// nibbles only) or 8
int planes_of_call(const bbq_index *ix, const uint8_t *q, int64_t count, int one_bit) {
  if (ix->geom.store_bits == 1) return one_bit ? 1 : planes_for(q, count);
  if (ix->geom.store_bits == 8) return 8;
  return max_value(q, count) <= 15 ? 4 : 8;
}

// a finite float that is zero or inside f32's normal range: an image the f32 bound can compute with under any denormal mode
static bool f32_image_ok(double v, float f) { return fabs(v) <= DBL_MAX && fabsf(f) <= FLT_MAX && (f == 0.0f ? v == 0.0 : fabsf(f) >= FLT_MIN); }
// the float at or above v > 0 (v far inside f32's range)
static float f32_up(double v) {
  const float f = (float)v;
  return (double)f >= v ? f : nextafterf(f, INFINITY);
}
// The f32 images of a query for the f32 form of the compact layout's score bound (compact_bound_passes, bbq_kernel_common.h, which
// holds the error budget these serve), each computed in f64 and rounded once; x1max / qcmax bound a row's component sum and qcDist.
// fast_bound = 0 - the query keeps the f64 bound - when the option is off, or an image is non-finite, overflows f32 or is a nonzero value
// below f32's normal range, or the magnitude M is outside [2^-80, 2^100] (below: a result flushed to zero would not stay inside the
// allowance; above: the allowance itself overflows and every row would pass).
void fast_bound_images(QueryParams *pp, double x1max, double qcmax, bool enable) {
  const double c1 = pp->ay * pp->dimd + pp->ly * pp->y1;
  const double M = (fabs(pp->ay) * pp->dimd + fabs(pp->ly * pp->y1) + 2.0 * (fabs(pp->ay) * x1max + fabs(pp->ly) * qcmax)) * 1.000001;
  pp->ayf = (float)pp->ay;
  pp->lyf = (float)pp->ly;
  pp->c1f = (float)c1;
  pp->csf = pp->sim == 0 ? 2.0f : 1.0f;
  pp->caf = pp->sim == 0 ? -1.0f : 1.0f;
  pp->digit_k = 0;
  const bool ok = enable && f32_image_ok(pp->ay, pp->ayf) && f32_image_ok(pp->ly, pp->lyf) && f32_image_ok(c1, pp->c1f) && M >= 0x1p-80 && M <= 0x1p100;
  pp->k2mf = ok ? f32_up(M * 0x1p-20) : 0.0f;
  pp->tinyf = ok ? f32_up(std::max(0x1p-100, M * 0x1p-120)) : 0.0f;
  if (!ok) pp->ayf = pp->lyf = pp->c1f = 0.0f;
  pp->fast_bound = ok ? 1 : 0;
}

// writes the query data and the score uniforms of one query into the staging buffer.
// 1-bit index: bit-planes ([j][p] 16-byte blocks, packed like the rows: dim d -> byte d>>3, bit 7-(d&7)).
// multi-bit index: per row dword w the dwords the kernel multiplies its unfolded fields with (dot_chunk_multibit):
//   store_bits 2: {lo nibbles of dims 16w+0,2,..,14 | lo nibbles of dims 16w+1,3,..,15 [| hi nibbles of the same, planes == 8]}
//   store_bits 4: {lo nibbles of dims 8w..8w+7 [| hi nibbles]}          store_bits 8: {bytes of dims 4w..4w+3}
void fill_query(const bbq_index *ix, uint8_t *planes_dst, QueryParams *pp, const uint8_t *q, const double *qc, int planes,
                int one_bit, int sim) {
  memset(planes_dst, 0, (size_t)query_data_bytes(ix, planes));
  if (ix->geom.store_bits == 1) {
    // eight dimensions (one byte of every plane) at a time: bit p of the eight query bytes, gathered MSB-first by one multiply -
    // source bit 8i (dimension 8*byte + i) goes to bit 63 - i of the product, no two partial products share a position
    const int full = ix->geom.dim >> 3;
    for (int byte = 0; byte < full; ++byte) {
      uint64_t x;
      memcpy(&x, q + (size_t)byte * 8, 8);
      if (!x) continue;
      const int j = byte >> 4, b = byte & 15;
      for (int p = 0; p < planes; ++p)
        planes_dst[((size_t)j * planes + p) * 16 + b] = (uint8_t)((((x >> p) & 0x0101010101010101ull) * 0x8040201008040201ull) >> 56);
    }
    for (int d = full * 8; d < ix->geom.dim; ++d) {  // the last, partial byte
      const uint8_t v = q[d];
      if (!v) continue;
      const int byte = d >> 3, j = byte >> 4, b = byte & 15;
      const uint8_t bit = (uint8_t)(0x80u >> (d & 7));
      for (int p = 0; p < planes; ++p)
        if ((v >> p) & 1) planes_dst[((size_t)j * planes + p) * 16 + b] |= bit;
    }
  } else {
    const int sb = ix->geom.store_bits, per = 32 / sb, qn = query_units_per_chunk(planes, sb);
    uint32_t *dst = reinterpret_cast<uint32_t *>(planes_dst);
    for (int d = 0; d < ix->geom.dim; ++d) {
      const uint32_t v = q[d];
      if (!v) continue;
      const int w = d / per, f = d % per;
      uint32_t *qw = dst + (size_t)w * qn;
      if (sb == 2) {
        const int half = f & 1, nib = f >> 1;
        qw[half] |= (v & 15u) << (4 * nib);
        if (planes > 4) qw[2 + half] |= (v >> 4) << (4 * nib);
      } else if (sb == 4) {
        qw[0] |= (v & 15u) << (4 * f);
        if (planes > 4) qw[1] |= (v >> 4) << (4 * f);
      } else {
        qw[0] |= v << (8 * f);
      }
    }
  }
  const double FBS = 1.0 / 15.0;  // src/constants.ts:20
  pp->ay = qc[0];
  pp->ly = one_bit ? (qc[1] - qc[0]) : (qc[1] - qc[0]) * FBS;  // src/batchDotProduct.ts:498 / :574
  pp->y1 = qc[3];
  pp->qadd = qc[2];
  // multi-bit index: the reference's batch scorer throws on unpacked rows and its per-row scorer answers
  // (src/binaryQuantizedScorer.ts:403-419): centroidDP is 0 for every query width but 1 (searchNearestNeighbors passes no
  // original query, :290) and MAXIMUM_INNER_PRODUCT is not divided by FOUR_BIT_SCALE (:207-209)
  const bool per_row_form = ix->geom.store_bits > 1;
  pp->cdp = (per_row_form && !one_bit) ? 0.0 : ix->centroid_dp;
  pp->dimd = (double)ix->geom.dim;
  pp->sim = sim;
  pp->one_bit = one_bit;
  pp->mip_plain = per_row_form ? 1 : 0;
  // the largest component sum and the largest qcDist a stored row can have, whatever y1 the caller passed
  const double vmax = (double)((1 << ix->geom.store_bits) - 1), qmax = ix->geom.store_bits == 1 ? (double)((1 << planes) - 1) : (planes > 4 ? 255.0 : 15.0);
  fast_bound_images(pp, pp->dimd * vmax, pp->dimd * vmax * qmax, ix->opt_fast_bound != 0 && !ix->geom.has_x1);
}

// The digit form of a 4-plane query against a 1-bit index (bbq_device.h, kDigitTable): the masks [j][kDigitMasks] = {P0, N0, P1, N1, P2},
// 16 bytes each and packed like the rows and the bit-planes (dim d -> byte d >> 3, bit 7 - (d & 7)), and K = pop(N0) + 3 pop(N1) into
// pp->digit_k.  Staged in addition to the bit-planes fill_query writes: every kernel but the digit twin of the sparse sweep reads those.
// Every value of q is at most 15 (planes == 4).
// A PADDING position (dim .. w16 * 128 - 1) is staged as the value 0, digits (-1, -1, 0): bits in N0 and N1.  The form's 4 * ones counts
// every bit the row stores, also one a caller left behind the last dimension of a partly used byte (the library stores a row's bytes as
// they come, and such a bit is part of the row's sum wherever the compact layout holds it); as a 0 of the query it contributes
// 4 - 1 - 3 = 0, as it does in the plane form, whose planes are 0 there.  A clear row bit there adds 1 + 3 to a0 + 3 a1 and to K alike.
void fill_query_digits(const bbq_index *ix, uint8_t *digits_dst, QueryParams *pp, const uint8_t *q) {
  static const struct Lut {
    uint8_t of[16];
    constexpr Lut() : of{} { for (int v = 0; v < 16; ++v) of[v] = (uint8_t)digit_mask_bits(v); }
  } lut;
  const int dim = ix->geom.dim;
  uint32_t n0 = 0, n1 = 0;
  for (int byte = 0; byte < ix->geom.w16 * 16; ++byte) {
    // the mask bits of the byte's eight dimensions side by side, then bit m of all eight gathered MSB-first by one multiply (fill_query)
    uint64_t x = 0;
    const int nd = std::max(0, std::min(8, dim - byte * 8));
    for (int i = 0; i < nd; ++i) x |= (uint64_t)lut.of[q[(size_t)byte * 8 + i] & 15] << (8 * i);
    for (int i = nd; i < 8; ++i) x |= (uint64_t)lut.of[0] << (8 * i);  // padding: the value 0
    uint8_t *dst = digits_dst + (size_t)(byte >> 4) * kDigitMasks * 16 + (byte & 15);
    for (int m = 0; m < kDigitMasks; ++m) dst[m * 16] = (uint8_t)((((x >> m) & 0x0101010101010101ull) * 0x8040201008040201ull) >> 56);
    n0 += (uint32_t)__builtin_popcount(dst[1 * 16]);
    n1 += (uint32_t)__builtin_popcount(dst[3 * 16]);
  }
  pp->digit_k = n0 + 3u * n1;
}

// MFMA shared sweep, int8 form (query values up to 127): the int8 query values in the order the code bits fall out of the packed
// words.  For 32-dim word g, half h, dword c, byte i the kernel extracts bit p = 4h + c + 8i of the little-endian word, which is row
// byte 4g + (p >> 3), bit (p & 7), i.e. dimension 32g + 8*(p >> 3) + 7 - (p & 7) (MSB-first packing,
// src/optimizedScalarQuantizer.ts:420-446).  Layout: [group][g][h][n][16 B], n = query in its group of 32.
static void fill_query_mfma(const bbq_index *ix, uint8_t *dst, int q_in_batch, const uint8_t *q) {
  const int words = ix->geom.w16 * 4, group = q_in_batch / 32, n = q_in_batch % 32;
  uint8_t *gb = dst + (size_t)group * mfma_query_bytes_per_group(ix->geom.w16, false);
  for (int g = 0; g < words; ++g)
    for (int h = 0; h < 2; ++h) {
      uint8_t *o = gb + (((size_t)g * 2 + h) * 32 + n) * 16;
      for (int cc = 0; cc < 4; ++cc)
        for (int i = 0; i < 4; ++i) {
          const int p = 4 * h + cc + 8 * i;
          const int d = 32 * g + 8 * (p >> 3) + 7 - (p & 7);
          o[4 * cc + i] = d < ix->geom.dim ? q[d] : 0;
        }
    }
}

// FP form (query values <= 15): v_mfma_f32_32x32x64_f8f6f4 with the rows as FP4 and the queries as FP6 (e2m3).  Step g covers the
// code words 2g (lower half-wave) and 2g + 1 (upper); element i of a lane is bit p = 4 (i & 7) + (i >> 3) of its word - the kernel
// masks bit c = i >> 3 of every nibble where it stands, an FP4 number of 0.5, 1.0, 2.0 and (bit 3, shifted down) 0.5 - and the query
// value carries 1/2, 1/4, 1/8, 1/2 against it: every product is q / 4 (q / 2 or q for smaller query values, see below).  e2m3 holds q / 2, q / 4 and q / 8 exactly for q <= 15
// (exponent 0: m / 8; exponent e: (1 + m / 8) 2^(e-1)).  A lane's 32 six-bit codes are 24 bytes: the first 16 in [g][h][n][16 B],
// the last 8 in [g][h][n][8 B] behind all of them (two aligned LDS reads per lane and step).
static uint32_t fp6_code_of_eighths(int eighths) {
  if (eighths < 8) return (uint32_t)eighths;                   // exponent field 0: m / 8
  int e = 1;
  while (eighths >= (8 << e)) ++e;                             // 2^(e-1) <= value < 2^e
  return ((uint32_t)e << 3) | (uint32_t)((eighths >> (e - 1)) - 8);   // exact: the low e - 1 bits of eighths are zero for q <= 15
}

static void fill_query_mfma_fp(const bbq_index *ix, uint8_t *dst, int q_in_batch, const uint8_t *q, int scale8) {
  const int steps = ix->geom.w16 * 2, group = q_in_batch / 32, n = q_in_batch % 32;
  uint8_t *gb = dst + (size_t)group * mfma_query_bytes_per_group(ix->geom.w16, true);
  uint8_t *gb2 = gb + (size_t)steps * 2 * 32 * 16;
  // the value x 8: q/2, q/4, q/8, q/2 at scale8 = 2 (products q/4: values up to 15); twice that for values up to 7 (scale8 = 4,
  // products q/2), four times for values up to 3 (scale8 = 8, products q): the finest grain e2m3's range (7.5) allows
  uint8_t lut[4][16];
  for (int cls = 0; cls < 4; ++cls)
    for (int v = 0; v < 16; ++v) lut[cls][v] = (uint8_t)fp6_code_of_eighths(v * (cls == 1 ? 2 : cls == 2 ? 1 : 4) * (scale8 / 2));
  // element i = 8 cls + j of a lane is bit p = 4 j + cls of its word: row byte j >> 1, bit 4 (j & 1) + cls, i.e. dimension
  // 8 (j >> 1) + 7 - 4 (j & 1) - cls of the word's 32.  The eight six-bit codes of a class are 48 bits: bytes [6 cls, 6 cls + 6)
  static const int off[8] = {7, 3, 15, 11, 23, 19, 31, 27};
  for (int g = 0; g < steps; ++g)
    for (int h = 0; h < 2; ++h) {
      const int base = 32 * (2 * g + h);
      uint8_t bits[24];
      for (int cls = 0; cls < 4; ++cls) {
        uint64_t v48 = 0;
        if (base + 32 <= ix->geom.dim) {
          for (int j = 0; j < 8; ++j) v48 |= (uint64_t)lut[cls][q[base + off[j] - cls] & 15] << (6 * j);
        } else {
          for (int j = 0; j < 8; ++j) {
            const int d = base + off[j] - cls;
            v48 |= (uint64_t)lut[cls][d < ix->geom.dim ? (q[d] & 15) : 0] << (6 * j);
          }
        }
        for (int b = 0; b < 6; ++b) bits[6 * cls + b] = (uint8_t)(v48 >> (8 * b));
      }
      memcpy(gb + (((size_t)g * 2 + h) * 32 + n) * 16, bits, 16);
      memcpy(gb2 + (((size_t)g * 2 + h) * 32 + n) * 8, bits + 16, 8);
    }
}

// second copy of a sub-batch's queries as MFMA operands in fragment order + per-group maxima for the rows' magnitude budget
MfmaStage stage_queries_mfma(const SearchCall &c, uint8_t *h_qbuf, const QueryParams *hq, int64_t q_first, int nq, size_t bytes) {
  const bbq_index *ix = c.ix;
  MfmaStage m{};
  m.fp = c.maxq <= 15;  // queryBits <= 4: rows as FP4, queries as FP6 - 64 dimensions per MFMA in the time the int8 form takes for 32
  m.scale8 = c.maxq <= 3 ? 8 : c.maxq <= 7 ? 4 : 2;  // products of scale8 / 8 * q: the accumulator's quarter-unit grain is 1, 1/2 or 1/4 of a qcDist unit
  const int groups = (nq + 31) / 32;
  m.off_qbytes = (bytes + 15) / 16 * 16;
  const size_t qbytes_len = (size_t)groups * (size_t)mfma_query_bytes_per_group(ix->geom.w16, m.fp);
  m.off_qmax = m.off_qbytes + qbytes_len;
  m.bytes = m.off_qmax + (size_t)groups * 16;
  memset(h_qbuf + m.off_qbytes, 0, qbytes_len);
  float *qm = reinterpret_cast<float *>(h_qbuf + m.off_qmax);
  for (int i = 0; i < 4 * groups; ++i) qm[i] = 0.f;
  for (int i = 0; i < nq; ++i) {
    const uint8_t *qv = c.qquant + (size_t)(q_first + i) * ix->geom.dim;
    if (m.fp) fill_query_mfma_fp(ix, h_qbuf + m.off_qbytes, i, qv, m.scale8);
    else fill_query_mfma(ix, h_qbuf + m.off_qbytes, i, qv);
    float *g = qm + 4 * (i / 32);
    // upper bounds (rounded up) of the group's |ay / ly|, |y1|, 1 / (cs * ly) and of the sum of a query's values (the largest
    // qcDist there can be, whatever y1 the caller passed)
    double qsum = 0;
    for (int d = 0; d < ix->geom.dim; ++d) qsum += qv[d];
    g[0] = std::max(g[0], (float)(fabs(hq[i].ay / hq[i].ly) * 1.000001));
    g[1] = std::max(g[1], (float)(fabs(hq[i].y1) * 1.000001));
    g[2] = std::max(g[2], (float)(1.0 / ((c.sim == 0 ? 2.0 : 1.0) * hq[i].ly) * 1.000001));
    g[3] = std::max(g[3], (float)(qsum * 1.000001));
  }
  return m;
}

// The matrix-core sweep tests "score > threshold" as an inequality on the integer dot product (bbq_mfma_kernels.hip), which divides by
// the query's interval width: it takes queries with a positive, finite width and finite corrections; any other sub-batch sweeps on
// the vector ALUs.
bool mfma_query_ok(const QueryParams &p) {
  return p.ly > 0.0 && p.ly < 1e30 && 1.0 / p.ly < 1e30 && fabs(p.ay) < 1e30 && fabs(p.y1) < 1e30 && fabs(p.qadd) < 1e30 && fabs(p.cdp) < 1e30;
}

int validate_query_args(const bbq_index *ix, int32_t nq, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                        int32_t sim, int64_t k, bool values_pending) {
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  if (nq < 0) return fail(BBQ_ERR_INVALID_ARG, "n_queries < 0");
  if (nq > 0 && (!qquant || !qcorr)) return fail(BBQ_ERR_INVALID_ARG, "查询向量不能为空");
  if (k < 0) return fail(BBQ_ERR_NEGATIVE_K, "k值不能为负数");
  if (query_bits < 1 || query_bits > 8) return fail(BBQ_ERR_INVALID_ARG, "queryBits必须在1-8之间");
  if (sim < 0 || sim > 2) return fail(BBQ_ERR_INVALID_ARG, "不支持的相似性函数: %d", sim);
  if (query_bits == 1 && !values_pending)  // (values_pending: the library's own quantizer is still producing them)
    for (int64_t i = 0; i < (int64_t)nq * ix->geom.dim; ++i)
      if (qquant[i] > 1) return fail(BBQ_ERR_INVALID_ARG, "1位量化值必须为0或1");
  return BBQ_OK;
}

}  // namespace bbq
