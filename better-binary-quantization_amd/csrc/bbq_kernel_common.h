// bbq_kernel_common.h - device functions shared by the sweep kernels of bbq_kernels.hip, bbq_latency_kernels.hip and
// bbq_mfma_kernels.hip (gfx950 only): the reference's float64 score formulas, the per-tile popcount loop, the score bound of the
// compact layout, the per-row candidate test and the ways candidates leave a workgroup, block-wide scan and order-statistic
// selection.  Everything here is __forceinline__: each kernel file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include "bbq_device.h"

#pragma clang fp contract(off)

namespace bbq {

// streamed, read-once data: non-temporal loads (A/B on MI355X: see DESIGN.md); -DBBQ_PLAIN_LOADS for the experiment
#ifdef BBQ_PLAIN_LOADS
#define BBQ_STREAM_LOAD(p) (*(p))
#else
#define BBQ_STREAM_LOAD(p) __builtin_nontemporal_load(p)
#endif

// a tile's bytes: default cache policy for the resident part of the index (IndexView::resident_tiles), streamed otherwise.
// `resident` must be wave-uniform (chunk_is_resident: decided per workgroup from blockIdx): a scalar branch, never both loads
template <class T> __device__ __forceinline__ const T *stream_ptr(const T *p, int64_t nt_delta) {
  return reinterpret_cast<const T *>(reinterpret_cast<const char *>(p) + nt_delta);
}
// the compiler merges the loads of two branches that differ only in the cache policy into ONE plain load (also through a phi of
// the two addresses): the streamed branch is fenced with compiler barriers, which its loads cannot be hoisted or sunk across
#define BBQ_BRANCH_FENCE() asm volatile("" ::: "memory")
__device__ __forceinline__ bool chunk_is_resident(int64_t chunk, const IndexView &v) {  // chunk comes from blockIdx: scalar
  return v.resident_share >= 0 ? (chunk & 63) < v.resident_share : chunk * kTilesPerChunk < v.resident_tiles;
}

// ALL loads of a wave's tile in ONE two-way branch (W > 0): the W code chunks of the lane's row and its corrections - CORR 0: none,
// 1: the compact word, 2: the inline f64 corrections (lower, upper | additional | component sum if stored).  Loads that are
// already in flight when the branch is reached make the compiler wait for them inside it (it assumes either arm may follow them).
// RS: the lane's entry of the row_sums side array (rs points at it) is one more load of the tile, under the arm's cache policy -> rsum.
// (A caller that uses the value behind a barrier passes rs as the aligned PAIR of entries the lane's own lies in, a uint32_t, and picks its half
// there: a 16-bit value that lives across blocks is widened by the compiler where it is loaded, and that instruction waits for the load.)
// `first` is called at the head of whichever arm is taken, in front of its loads: a load of the caller's own that has to be the oldest one in
// flight (the sweep's query masks).  Issued in front of the branch instead, it is "just issued" on the path into either arm, and the
// compiler's count at the join behind the arms makes whoever needs it wait for all of the tile's loads but the last.
struct NoFirstLoad { __device__ __forceinline__ void operator()() const {} };
template <int W, int CORR, bool RS = false, class RSrc = uint16_t, class First = NoFirstLoad>
__device__ __forceinline__ void load_tile(const uint8_t *__restrict__ tp, int lane, bool has_x1, bool resident, int64_t nt_delta,
                                          u32x4 (&c)[W], uint32_t &cw, f64x2 &lu, double &xadd, double &x1,
                                          const RSrc *__restrict__ rs = nullptr, uint32_t *rsum = nullptr, First first = First()) {
  const u32x4 *__restrict__ cp = reinterpret_cast<const u32x4 *>(tp) + lane;
  const uint8_t *__restrict__ cr = tp + tile_corr_offset(W);
  if (resident) {  // scalar branch
    first();
#pragma unroll
    for (int j = 0; j < W; ++j) c[j] = cp[j * kTileRows];
    if constexpr (CORR == 1) cw = *(reinterpret_cast<const uint32_t *>(cr) + lane);
    if constexpr (RS) *rsum = *rs;
    if constexpr (CORR == 2) {
      lu = *(reinterpret_cast<const f64x2 *>(cr) + lane);
      xadd = *(reinterpret_cast<const double *>(cr + kCorrAddOffset) + lane);
      if (has_x1) x1 = *(reinterpret_cast<const double *>(cr + kCorrSumOffset) + lane);
    }
  } else {
    BBQ_BRANCH_FENCE();
    first();
    const u32x4 *__restrict__ cs = stream_ptr(cp, nt_delta);
    const uint8_t *__restrict__ crs = stream_ptr(cr, nt_delta);
#pragma unroll
    for (int j = 0; j < W; ++j) c[j] = BBQ_STREAM_LOAD(cs + j * kTileRows);
    if constexpr (CORR == 1) cw = BBQ_STREAM_LOAD(reinterpret_cast<const uint32_t *>(crs) + lane);
    if constexpr (RS) *rsum = BBQ_STREAM_LOAD(stream_ptr(rs, nt_delta));
    if constexpr (CORR == 2) {
      lu = BBQ_STREAM_LOAD(reinterpret_cast<const f64x2 *>(crs) + lane);
      xadd = BBQ_STREAM_LOAD(reinterpret_cast<const double *>(crs + kCorrAddOffset) + lane);
      if (has_x1) x1 = BBQ_STREAM_LOAD(reinterpret_cast<const double *>(crs + kCorrSumOffset) + lane);
    }
    BBQ_BRANCH_FENCE();
  }
}

__device__ __forceinline__ uint32_t popc4(u32x4 v) { return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }
// acc + popcount(x) in ONE instruction (v_bcnt_u32_b32 has the addend built in).  Written as `acc += popc4(...)` the compiler sums the
// four counts of a 16-byte chunk in a tree of v_add3_u32 first: 56 extra vector instructions per 768-d row, 14 % of the sweep's
// vector work - and the sweep is bound by vector issue whenever its bytes come out of a cache (scan kernel).
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}
__device__ __forceinline__ uint32_t popc4_acc(u32x4 v, uint32_t acc) { return bcnt_acc(v.w, bcnt_acc(v.z, bcnt_acc(v.y, bcnt_acc(v.x, acc)))); }

// Math.max(x, 0) of the reference: NaN propagates, -0 -> +0
__device__ __forceinline__ double js_max0(double x) { return (x != x) ? x : (x > 0.0 ? x : 0.0); }

// src/batchDotProduct.ts:478-541 (one_bit) / :554-617 (every other queryBits); SURVEY App. A.4.
// Parenthesised exactly as JavaScript evaluates the reference's expressions; no FMA contraction.
__device__ __forceinline__ double score_f64(double qc, double ax, double ux, double xadd, double x1, const QueryParams &p) {
  const double lx = ux - ax;
  const double t1 = (ax * p.ay) * p.dimd;
  const double t2 = (p.ay * lx) * x1;
  const double t3 = (ax * p.ly) * p.y1;
  const double t4 = (lx * p.ly) * qc;
  const double s = ((t1 + t2) + t3) + t4;
  if (p.sim == 0) {  // EUCLIDEAN
    const double e = (p.qadd + xadd) - (2.0 * s);
    return js_max0(1.0 / (1.0 + e));
  }
  const double t = p.one_bit ? (s + ((p.qadd + xadd) - p.cdp)) : (((s + p.qadd) + xadd) - p.cdp);
  if (p.sim == 1) return js_max0((1.0 + t) / 2.0);  // COSINE
  // scaleMaxInnerProductScore (src/utils.ts:171-176): the 1-bit batch form (:527-533) and the per-row scorer's form for
  // every query width (src/binaryQuantizedScorer.ts:148-153, :207-209), which is what answers for multi-bit indexes
  if (p.one_bit || p.mip_plain) return t < 0.0 ? 1.0 / (1.0 - t) : t + 1.0;
  const double FBS = 1.0 / 15.0;  // FOUR_BIT_SCALE, src/constants.ts:20 - a true division by it, not *15
  return t < 0.0 ? 1.0 / (1.0 - t / FBS) : t / FBS + 1.0;
}

// qcDist of a 1-bit row from the popcounts of its AND with the query's bit-planes: plane p weighs 2^p
template <int QB> __device__ __forceinline__ uint32_t plane_dot(const uint32_t (&acc)[QB]) {
  uint32_t qc = 0;
#pragma unroll
  for (int p = 0; p < QB; ++p) qc += acc[p] << p;
  return qc;
}

// One tile = 64 rows, one row per lane.  W = compile-time number of 16-byte chunks per row: the chunks come in registers (load_tile).
// Returns qcDist; `ones` = the row's popcount - left alone with ONES false: the caller has it from the row_sums side array
template <int QB, int W, bool ONES = true>
__device__ __forceinline__ uint32_t tile_popcounts(const u32x4 (&c)[W], const u32x4 *__restrict__ s_planes, uint32_t &ones) {
  uint32_t acc[QB];
#pragma unroll
  for (int p = 0; p < QB; ++p) acc[p] = 0;
  if constexpr (ONES) ones = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) {
#pragma unroll
    for (int p = 0; p < QB; ++p) acc[p] = popc4_acc(c[j] & s_planes[j * QB + p], acc[p]);
    if constexpr (ONES) ones = popc4_acc(c[j], ones);
  }
  return plane_dot<QB>(acc);
}
// any width (w16 chunks, known at run time): streamed chunk by chunk
template <int QB, bool ONES = true>
__device__ __forceinline__ uint32_t tile_popcounts_any(const uint8_t *__restrict__ tp, int lane, int w16, const u32x4 *__restrict__ s_planes,
                                                       uint32_t &ones) {
  const u32x4 *__restrict__ cp = reinterpret_cast<const u32x4 *>(tp) + lane;
  uint32_t acc[QB];
#pragma unroll
  for (int p = 0; p < QB; ++p) acc[p] = 0;
  if constexpr (ONES) ones = 0;
  for (int j = 0; j < w16; ++j) {
    const u32x4 c = BBQ_STREAM_LOAD(cp + j * kTileRows);
#pragma unroll
    for (int p = 0; p < QB; ++p) acc[p] += popc4(c & s_planes[j * QB + p]);
    if constexpr (ONES) ones += popc4(c);
  }
  return plane_dot<QB>(acc);
}

// The digit form of a 4-plane query (bbq_device.h, kDigitMasks): qcDist of a 1-bit row from THREE planes of ternary digits instead of four
// bit-planes.  s_digits holds {P0, N0, P1, N1, P2} per chunk; (x & P) | (~x & N) is one v_bfi_b32 with the row word as the selector, the top
// digit a plain AND; `ones` = the row's popcount from the row_sums side array, k = QueryParams::digit_k.  u32 arithmetic on a value below 2^32.
__device__ __forceinline__ u32x4 digit_select(u32x4 x, u32x4 p, u32x4 n) { return (x & p) | (~x & n); }
__device__ __forceinline__ uint32_t digit_dot(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t ones, uint32_t k) {
  return ((ones << 2) - k) + a0 + 3u * a1 + 9u * a2;
}
// same shape as tile_popcounts: the chunks in registers, the masks from LDS through wave-uniform addresses, the sums inside v_bcnt
template <int W>
__device__ __forceinline__ uint32_t tile_digit_dot(const u32x4 (&c)[W], const u32x4 *__restrict__ s_digits, uint32_t ones, uint32_t k) {
  uint32_t a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const u32x4 *__restrict__ m = s_digits + j * kDigitMasks;
    a0 = popc4_acc(digit_select(c[j], m[0], m[1]), a0);
    a1 = popc4_acc(digit_select(c[j], m[2], m[3]), a1);
    a2 = popc4_acc(c[j] & m[4], a2);
    // 12 chunks: left alone, the compiler reads the masks of many chunks ahead of their use - 82 vector registers and 5 waves where the plane
    // form has 69 and 7.  A compiler barrier behind each chunk keeps a chunk's five reads next to its use: 68 registers, 7 waves
    if constexpr (W >= 12) BBQ_BRANCH_FENCE();
  }
  return digit_dot(a0, a1, a2, ones, k);
}
// any width: streamed chunk by chunk
__device__ __forceinline__ uint32_t tile_digit_dot_any(const uint8_t *__restrict__ tp, int lane, int w16, const u32x4 *__restrict__ s_digits,
                                                       uint32_t ones, uint32_t k) {
  const u32x4 *__restrict__ cp = reinterpret_cast<const u32x4 *>(tp) + lane;
  uint32_t a0 = 0, a1 = 0, a2 = 0;
  for (int j = 0; j < w16; ++j) {
    const u32x4 c = BBQ_STREAM_LOAD(cp + j * kTileRows);
    const u32x4 *__restrict__ m = s_digits + j * kDigitMasks;
    a0 += popc4(digit_select(c, m[0], m[1]));
    a1 += popc4(digit_select(c, m[2], m[3]));
    a2 += popc4(c & m[4]);
  }
  return digit_dot(a0, a1, a2, ones, k);
}

// Upper bound of the score when only the COMPACT corrections are known (kLayoutCompact).
// The raw score s is linear in (lower, upper): with x1 and qcDist fixed,
//     s(lower, upper) = lower * A + upper * B,   A = ay*(dim - x1) + ly*(y1 - qc),   B = ay*x1 + ly*qc,
// so replacing (lower, upper, add) by their compact values (al, au, aadd) changes s by exactly
// (lower-al)*A + (upper-au)*B and the additive term by (add-aadd).  |lower-al| <= |al|*kBf16Rel + kAbsSlack
// (f32 rounding + truncation to the upper 16 bits), |add-aadd| <= |aadd|*2^-23 + kAbsSlack.  All three similarity
// transforms are monotone in s (resp. in t), and a generous rounding allowance (kRoundRel, ~7 orders of magnitude
// above the real f64 round-off of these ~20 operations) covers the difference between exact-arithmetic reasoning and
// IEEE evaluation.  Returns a value U with  exact f64 score <= U  (NaN or +inf when no finite bound can be given:
// the caller then takes the exact path).  tests/test_bound_math_cpu.py restates this in numpy and checks dominance.
constexpr double kBf16Rel = 0.0078125 * (1.0 + 1.0 / 65536.0);  // 2^-7 (1 + 2^-16)
constexpr double kF32Rel = 1.1920928955078125e-07;             // 2^-23
constexpr double kAbsSlack = 1e-37;
constexpr double kRoundRel = 1e-9;

__device__ __forceinline__ double score_upper_bound(double qc, double al, double au, double aadd, double x1, const QueryParams &p) {
  const double lx = au - al;
  const double t1 = (al * p.ay) * p.dimd;
  const double t2 = (p.ay * lx) * x1;
  const double t3 = (al * p.ly) * p.y1;
  const double t4 = (lx * p.ly) * qc;
  const double s = ((t1 + t2) + t3) + t4;
  const double A = p.ay * (p.dimd - x1) + p.ly * (p.y1 - qc);
  const double B = p.ay * x1 + p.ly * qc;
  const double mag = fabs(t1) + fabs(t2) + fabs(t3) + fabs(t4) + fabs(p.qadd) + fabs(aadd) + fabs(p.cdp) + 1.0;
  if (!(mag < 1e290)) return __longlong_as_double(0x7ff8000000000000ll);  // non-finite / huge: no bound
  const double es = fabs(A) * (fabs(al) * kBf16Rel + kAbsSlack) + fabs(B) * (fabs(au) * kBf16Rel + kAbsSlack);
  const double eadd = fabs(aadd) * kF32Rel + kAbsSlack;
  const double slop = kRoundRel * (mag + fabs(A) + fabs(B));
  if (p.sim == 0) {  // EUCLIDEAN: score = max(1/(1+e), 0), decreasing in e while 1+e > 0
    const double e_low = ((p.qadd + aadd) - (2.0 * s)) - (2.0 * es + eadd + slop);
    const double den = 1.0 + e_low;
    if (!(den > 0.0)) return __longlong_as_double(0x7ff0000000000000ll);  // +inf: cannot exclude a tiny positive denominator
    const double u = 1.0 / den;
    return u + kRoundRel * (u + 1.0);
  }
  const double t_up = (((s + p.qadd) + aadd) - p.cdp) + (es + eadd + slop);
  double u;
  if (p.sim == 1) u = js_max0((1.0 + t_up) / 2.0);
  else if (p.one_bit || p.mip_plain) u = t_up < 0.0 ? 1.0 / (1.0 - t_up) : t_up + 1.0;
  else {
    const double FBS = 1.0 / 15.0;
    u = t_up < 0.0 ? 1.0 / (1.0 - t_up / FBS) : t_up / FBS + 1.0;
  }
  return u + kRoundRel * (fabs(u) + 1.0);
}

// ---- one row of a sweep ----------------------------------------------------------------------------------------------------------
// the tile's additive-correction range in the compact layout: EUCLIDEAN scores fall with it (take the minimum), the others rise (maximum)
__device__ __forceinline__ float tile_add_bound(const IndexView &v, int64_t tile, int sim) { return v.add_range[tile * 2 + (sim == 0 ? 0 : 1)]; }

// ---- the threshold in the linear space of the score formula ------------------------------------------------------------------------
// conservative lower edge, in z-space, of "score > theta" for one query.
//   COSINE / MIP: z = s + xadd,  score = f(z + qadd - cdp) with f increasing
//   EUCLIDEAN   : z = 2s - xadd, score = 1/(1 + qadd - z)  increasing in z while the denominator is positive
// Returns zmin with:  exact f32 score > theta_score  =>  z > zmin.   -DBL_MAX accepts everything.
__device__ __forceinline__ double z_threshold(uint32_t theta_key, const QueryParams &p) {
  if (theta_key == 0u) return -DBL_MAX;
  const uint32_t bits = bits_of_key(theta_key);
  const double th = (double)__uint_as_float(bits);  // the threshold score (a float the reference produced)
  if (!(th == th)) return -DBL_MAX;
  double z;
  if (p.sim == 1) {                 // max((1+t)/2, 0) > th  =>  t > 2 th - 1        (th >= 0 always for scores)
    if (th < 0.0) return -DBL_MAX;
    z = (2.0 * th - 1.0) - (p.qadd - p.cdp);
  } else if (p.sim == 2) {
    double t;
    if (p.one_bit || p.mip_plain) t = th >= 1.0 ? th - 1.0 : (th > 0.0 ? 1.0 - 1.0 / th : -DBL_MAX);  // the two forms score_f64 has
    else {
      const double FBS = 1.0 / 15.0;
      t = th >= 1.0 ? (th - 1.0) * FBS : (th > 0.0 ? (1.0 - 1.0 / th) * FBS : -DBL_MAX);
    }
    if (t == -DBL_MAX) return -DBL_MAX;
    z = t - (p.qadd - p.cdp);
  } else {                          // 1/(1+e) > th, e = qadd + xadd - 2s = qadd - z   =>  z > qadd + 1 - 1/th
    if (!(th > 0.0)) return -DBL_MAX;
    z = p.qadd + 1.0 - 1.0 / th;
  }
  if (!(fabs(z) <= DBL_MAX)) return -DBL_MAX;
  return z - 1e-9 * (fabs(z) + fabs(p.qadd) + fabs(p.cdp) + 1.0);  // rounding allowance of this inversion
}
// ... rounded DOWN to f32: the z image of a threshold key (-inf accepts everything)
__device__ __forceinline__ float z_threshold_f32(uint32_t theta_key, const QueryParams &p) {
  const double z = z_threshold(theta_key, p);
  const float zf = (float)z;  // to nearest; -DBL_MAX becomes -inf
  if (!((double)zf > z)) return zf;
  const uint32_t b = __float_as_uint(zf);  // the next float below zf (zf is no NaN and not -inf here)
  return __uint_as_float((b << 1) == 0u ? 0x80000001u : (b & 0x80000000u) ? b + 1u : b - 1u);
}
// THE writer of a query's threshold: the key and its z image, one 8-byte store
__device__ __forceinline__ void store_threshold(Threshold *dst, uint32_t key, const QueryParams &p) { *dst = make_threshold(key, z_threshold_f32(key, p)); }

// compact layout: the row's bf16 {lower, upper} word and the tile's additive bound give an upper bound of its score.  NaN (no bound)
// passes; otherwise the row can only matter if even its upper bound beats the threshold.  `ones` = x1: the compact layout exists only
// for indexes whose component sums are the rows' popcounts / code sums (set_index_geometry).
//
// Two forms of one test, chosen per query by a scalar branch (QueryParams::fast_bound, set by the host: fast_bound_images):
//  * f64, through the similarity transform: score_upper_bound against the key;
//  * f32, in z-space, against the threshold's z image (z_threshold_f32).  With g = ay x1 + ly qc and c1 = ay dim + ly y1 the raw score of
//    the compact corrections is s = al (c1 - g) + au g, and  z = cs s + ca add.  99.9 % of the rows of a sweep exist only to fail this
//    test, and in f64 it was a fifth of the sweep's vector instructions.
// Error budget of the f32 form (u = 2^-24; M >= |ay| dim + |ly y1| + 2 (|ay| x1max + |ly| qcmax), so |g|, |c1 - g|, and every
// term of the reference's sum t1..t4 per unit of |lower| + |upper|, are at most M; W = |al| + |au|, E = |al (c1 - g)| + |au g| <= W M):
//  * the images ayf, lyf, c1f are within u of their values, (float)qc within u (exact below 2^24), (float)ones exact: the computed g is
//    within 2.1 u M of g, the computed A = c1 - g within 5.1 u M, the two products and their sum add 3 u E: |s_f32 - s| <= 9.1 u W M;
//  * the exact corrections differ from the compact ones by |lower - al| <= |al| kBf16Rel + 2^-132 (f32 rounding, truncation to bf16; the
//    absolute part is what a subnormal f32 loses), so the exact row's s differs by at most kBf16Rel E + 2^-131 M - with E taken from the
//    computed products (within u + 6 u W M / E of the true ones, the latter 2^-7 * 6 u W M more);
//  * the reference's own f64 evaluation (2^-50 W M) and the z-space sums vanish beside these.
//  Allowance: K1 E + 2^-20 W M + tiny, K1 = kBf16Rel (1 + 2^-18) (the 2^-18 pays the roundings of E and of the allowance itself),
//  2^-20 = 16 u against the 9.2 u needed, tiny = max(2^-100, 2^-120 M) for the absolute parts: the 2^-131 M above, kAbsSlack of the
//  additive term, and every f32 operation here whose result leaves the normal range (at most 2^-126 each, also with subnormals
//  flushed; the host refuses images below the normal range and M < 2^-80, so that a flushed g or A, times |au| or |al|, stays inside
//  the 2^-20 W M).  The additive term: ca add <= ca aadd + 2^-23 |aadd| (add_range is rounded to nearest), given 2^-21 |aadd|; the last
//  line pays the roundings of the z-space sums.  Overflow or NaN anywhere ends as +inf or NaN: the row passes, as in the f64 form.
//  tests/test_bound_f32_cpu.py restates this in numpy f32 and checks dominance over the exact score, fused and unfused.
constexpr float kFastK1 = (float)(kBf16Rel * (1.0 + 1.0 / 262144.0));
constexpr float kFastAddRel = 4.76837158203125e-07f;  // 2^-21
// (P: QueryParams, or the f32 images alone - the sweep of several tiles per wave keeps nothing else of the query in its tile loop)
template <class P>
__device__ __forceinline__ bool fast_bound_passes(bool valid, uint32_t qc, uint32_t cw, float aadd, uint32_t ones, const P &p, const Threshold &th) {
  const float al = compact_lower(cw), au = compact_upper(cw);  // bf16 -> f32 is exact
  const float g = fmaf(p.lyf, (float)qc, p.ayf * (float)ones);
  const float A = p.c1f - g;
  const float pa = al * A, pb = au * g;
  const float s = pa + pb;
  const float e = fabsf(pa) + fabsf(pb);
  const float w = fabsf(al) + fabsf(au);
  const float slack = fmaf(kFastK1, e, fmaf(w, p.k2mf, p.tinyf));
  const float zc = fmaf(p.csf, s, p.caf * aadd);
  const float zs = fmaf(p.csf, slack, kFastAddRel * fabsf(aadd));
  const float z0 = zc + zs;
  const float zup = fmaf(kFastAddRel, fabsf(z0), z0);
  return valid && !(zup <= threshold_z(th));  // NaN anywhere passes -> exact path
}
__device__ __forceinline__ bool f64_bound_passes(bool valid, uint32_t qc, uint32_t cw, float aadd, double x1, const QueryParams &p, uint32_t theta) {
  const double al = (double)compact_lower(cw);
  const double au = (double)compact_upper(cw);
  const double ub = score_upper_bound((double)qc, al, au, (double)aadd, x1, p);
  const float ub32 = (float)ub;
  return valid && ((ub32 != ub32) || key_of_bits(__float_as_uint(ub32)) > theta);
}
__device__ __forceinline__ bool compact_bound_passes(bool valid, uint32_t qc, uint32_t cw, float aadd, uint32_t ones, double x1, const QueryParams &p,
                                                     const Threshold &th) {
  return p.fast_bound ? fast_bound_passes(valid, qc, cw, aadd, ones, p, th) : f64_bound_passes(valid, qc, cw, aadd, x1, p, th.key);  // per query: a scalar branch
}
// the row's exact corrections from the compact layout's side array: {lower, upper} and additionalCorrection.  STREAM: the dense paths,
// which read every row once (non-temporal loads)
template <bool STREAM = false>
__device__ __forceinline__ void exact_corrections(const double *exact, int64_t row, f64x2 &lu, double &xadd) {
  const f64x2 *__restrict__ ex = reinterpret_cast<const f64x2 *>(exact + row * 4);
  if constexpr (STREAM) {
    lu = BBQ_STREAM_LOAD(ex);
    xadd = BBQ_STREAM_LOAD(reinterpret_cast<const double *>(ex + 1));
  } else {
    lu = ex[0];
    xadd = reinterpret_cast<const double *>(ex + 1)[0];
  }
}

// the candidate test on the exact score, rounded to f32 as the reference stores it (Float32Array, src/binaryQuantizationFormat.ts:353,378):
// a valid row is a candidate iff its score is no NaN and its key beats the threshold.  A valid row with a NaN score sets `nan_seen`.
__device__ __forceinline__ bool exact_key_passes(bool valid, float s32, uint32_t theta, bool &nan_seen) {
  if (valid && (s32 != s32)) nan_seen = true;
  return valid && (s32 == s32) && key_of_bits(__float_as_uint(s32)) > theta;
}
// a candidate entry (bbq_entry.h) of a row and its f32 score
__device__ __forceinline__ uint64_t candidate_entry(int64_t row_id, float s32) { return make_entry((uint32_t)row_id, __float_as_uint(s32)); }

// ---- candidates leaving a workgroup ------------------------------------------------------------------------------------------------
// the cnt staged entries of a chunk into its slot, row-ordered: rows are distinct, so ranking by counting puts them in row order
// (thread `t` of `nt` takes entries t, t + nt, ...)
__device__ __forceinline__ void write_ranked(const uint64_t *__restrict__ src, uint32_t cnt, uint64_t *__restrict__ out, int t, int nt) {
  for (uint32_t i = t; i < cnt; i += nt) {
    const uint64_t e = src[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < cnt; ++j) rank += (src[j] < e) ? 1u : 0u;
    out[rank] = e;
  }
}

// the workgroup's cnt > 0 staged entries (workgroup-uniform) into the query's list behind the `base` entries of the earlier segments,
// unordered: ONE atomic on the query's append counter reserves the room for all of them, handed to the workgroup through the LDS word
// s_at.  A list without that room flags the query (kFlagOverflow) and takes none of them.
template <int NT>
__device__ __forceinline__ void append_to_list(const uint64_t *s_ent, uint32_t cnt, uint32_t *counter, int64_t base, uint64_t *__restrict__ list,
                                               int64_t list_cap, uint32_t *flags, uint32_t *s_at) {
  const int tid = threadIdx.x;
  if (tid == 0) *s_at = atomicAdd(counter, cnt);
  __syncthreads();
  const int64_t at = base + *s_at;
  if (at + cnt > list_cap) {
    if (tid == 0) atomicOr(flags, kFlagOverflow);
    return;
  }
  for (uint32_t i = tid; i < cnt; i += NT) list[at + i] = s_ent[i];
}

__device__ __forceinline__ uint32_t block_exclusive_scan_1024(uint32_t v, uint32_t *s_wave, uint32_t &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t n = __shfl_up(incl, d, 64);
    if (lane >= d) incl += n;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  uint32_t wave_off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const uint32_t x = s_wave[w];
    if (w < wave) wave_off += x;
    tot += x;
  }
  total = tot;
  __syncthreads();
  return wave_off + incl - v;
}

// k-th largest of the M keys in LDS (M >= k >= 1): radix select over the key bytes that actually vary, one 1024-thread workgroup;
// every thread returns it.  s_hist: 2 x 256 words, s_wave: 16 words, s_scr: 8 words of scratch owned by this function.
// Barriers are what this costs (16 waves: ~0.4 us each), so there are two per pass: the histogram of a pass is built in one of two
// buffers while the other is being cleared, and every pass leaves its result in words of its own.
template <int NT>
__device__ __forceinline__ uint32_t block_select_kth_largest_t(const uint32_t *s_keys, uint32_t M, uint32_t k, uint32_t *s_hist, uint32_t *s_wave,
                                                               uint32_t *s_scr) {
  const int tid = threadIdx.x;
  // Scores of one query live in a narrow range: the upper bytes of their keys are the same for (nearly) all of them, and a
  // histogram pass over such a byte is thousands of atomic adds on ONE LDS word (measured: 10 us per pass at 6 K keys).
  // Bytes that are constant over all keys are therefore skipped: they belong to the answer as they are.
  uint32_t vary = 0;
  {
    const uint32_t key0 = s_keys[0];
#pragma unroll 4
    for (uint32_t i = tid; i < M; i += NT) vary |= s_keys[i] ^ key0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) vary |= __shfl_xor(vary, d, 64);
    if ((tid & 63) == 0) s_wave[tid >> 6] = vary;
    for (int i = tid; i < 512; i += NT) s_hist[i] = 0;
    __syncthreads();
    vary = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) vary |= s_wave[w];
  }
  uint32_t prefix = 0, mask = 0, kk = k;
  int buf = 0;
  for (int pass = 3; pass >= 0; --pass) {
    const int sh = pass * 8;
    if (((vary >> sh) & 255u) == 0u) {  // uniform: every key has the same byte here
      prefix |= s_keys[0] & (255u << sh);
      mask |= 255u << sh;
      continue;
    }
    uint32_t *__restrict__ hist = s_hist + 256 * buf;
    // The pass is latency-bound per wave (a wave walks M / NT keys one after the other), so nothing in a step may wait: the keys of
    // four steps are loaded before any of them is used, the first active lane's bin is read with v_readlane (an LDS-routed shuffle
    // was a round trip per key) and the histogram adds return nothing.
    for (uint32_t i0 = 0; i0 < M; i0 += 4 * NT) {  // whole waves iterate together (ballots below)
      uint32_t kv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t i = i0 + (uint32_t)u * NT + tid;
        kv[u] = s_keys[i < M ? i : 0];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t i = i0 + (uint32_t)u * NT + tid;
        const bool in = i < M && (kv[u] & mask) == prefix;
        const uint32_t bin = in ? (kv[u] >> sh) & 255u : 256u;
        // a byte with few distinct values would still pile the adds on a few words: the lanes that share the first active lane's
        // bin add once for all of them
        const unsigned long long act = __ballot(in);
        if (act) {
          const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, __ffsll((long long)act) - 1);
          const unsigned long long same = __ballot(in && bin == b0);
          if (in && bin == b0) {
            if ((tid & 63) == __ffsll((long long)same) - 1) atomicAdd(&hist[b0], (uint32_t)__popcll(same));
          } else if (in) {
            atomicAdd(&hist[bin], 1u);
          }
        }
      }
    }
    __syncthreads();
    if (tid < 64) {
      // wave 0 finds the bin: lane l owns bins 4l..4l+3; suffix sums over lanes by shuffles (no LDS round trips)
      const uint32_t h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
      uint32_t suf = h0 + h1 + h2 + h3;  // becomes the sum over bins >= 4*tid
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t n = __shfl_down(suf, d, 64);
        if (tid + d < 64) suf += n;
      }
      const uint32_t above = suf - (h0 + h1 + h2 + h3);  // bins > 4*tid+3
      if (suf >= kk && above < kk) {                     // exactly one lane: the k-th largest lies in its 4 bins
        uint32_t cum = above;
        int b = 4 * tid + 3;
        if (cum + h3 < kk) { cum += h3; b = 4 * tid + 2;
          if (cum + h2 < kk) { cum += h2; b = 4 * tid + 1;
            if (cum + h1 < kk) { cum += h1; b = 4 * tid; } } }
        s_scr[2 * pass] = (uint32_t)b;
        s_scr[2 * pass + 1] = kk - cum;
      }
    } else if (tid >= NT - 256) {
      s_hist[256 * (buf ^ 1) + (tid - (NT - 256))] = 0;  // the other buffer, for the next pass
    }
    __syncthreads();
    prefix |= s_scr[2 * pass] << sh;
    mask |= 255u << sh;
    kk = s_scr[2 * pass + 1];
    buf ^= 1;
  }
  __syncthreads();  // the caller may reuse the scratch words and the keys
  return prefix;
}

__device__ __forceinline__ uint32_t block_select_kth_largest(const uint32_t *s_keys, uint32_t M, uint32_t k, uint32_t *s_hist, uint32_t *s_wave,
                                                             uint32_t *s_scr) {
  return block_select_kth_largest_t<kFinalizeThreads>(s_keys, M, k, s_hist, s_wave, s_scr);
}

}  // namespace bbq
