// bbq_mfma_common.h - the device pieces the matrix-core kernels share (bbq_mfma_kernels.hip: the top-k shared sweep;
// bbq_range_mfma_kernels.hip: the count pass of the range search): the number formats of the accumulator's start value, a row's
// constants, the start-value contraction, one k-step of the FP form, the tile registers and their loads.  Included behind the
// including file's `#pragma clang fp contract(off)`; the derivations stand where they stood, at the pieces themselves.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "bbq_device.h"
#include "bbq_kernel_common.h"

namespace bbq {

typedef int i32x4m __attribute__((ext_vector_type(4)));
typedef int i32x16m __attribute__((ext_vector_type(16)));
typedef float f32x16m __attribute__((ext_vector_type(16)));
typedef int i32x8m __attribute__((ext_vector_type(8)));
// the accept words of a filtered sweep as the kernel reads them: through the constant address space, so that a wave-uniform read is a
// scalar load wherever it stands (a kernel that writes memory - this one appends candidates - reads a plain global pointer through the
// vector unit once it has stored anything, and waits for every vector load in flight, the next tile's among them, to do it)
typedef const __attribute__((address_space(4))) uint64_t *AcceptWords;

constexpr int kMfmaQueries = 32;
// The accumulator's start value lies in a binade whose ulp is the grain of the threshold:
//   int8 form (S = 1):          [2^23, 2^24), ulp 1; the i32 accumulator holds the float's bits, 0x4B000000 + its integer distance from 2^23
//   FP form  (S = 1/4, 1/2, 1): [2^19, 2^20), ulp 1/16; the f32 accumulator holds the value.  The products are multiples of S, the start
//                               value a multiple of 1/16: every partial sum is a multiple of 1/16 below 2^20, i.e. exact in f32
// "bias" is the middle of the binade (1.5 x its lower end); the sum of the terms must stay below a quarter of the binade's lower end
// so that every partial sum stays inside it.
// "pass_none" (the filtered family: the start value of a row its filter rejects) mirrors pass_all below the bias: a value inside the
// binade, a quarter of the binade's lower end below its middle.  The row's constants are zero, so its accumulator ends at exactly
// pass_none + S * qcDist, and the largest S * qcDist a form admits is far below that margin:
//   int8 form: 1536 dimensions x 127 = 195 072 < 2 097 152 (2^21), and 10 485 760 = pass_none >= 2^23: the sum stays in [2^23, bias)
//   FP form:   1536 x 15 x S <= 23 040 for S = 1 (5 760 at S = 1/4, where 15 is reached; the values a larger S goes with are smaller)
//              < 131 072 (2^17), and 655 360 = pass_none >= 2^19: the sum stays in [2^19, bias)
// so no pair of a rejected row ends above the bias, whatever the query (tests/test_prefilter_reject_cpu.py restates this in numpy).
template <bool FP> struct MfmaNum;
template <> struct MfmaNum<false> {
  static constexpr float S = 1.0f, ulp = 1.0f, bias = 12582912.0f, mag_limit = 4000000.0f, pass_all = 12582912.0f + 2097152.0f,
                         pass_none = 12582912.0f - 2097152.0f;
};
template <> struct MfmaNum<true> {   // S is chosen per call: 1/4 for query values up to 15, 1/2 up to 7, 1 up to 3 (MfmaArgs::fp_scale)
  static constexpr float S = 0.25f, ulp = 0.0625f, bias = 786432.0f, mag_limit = 110000.0f, pass_all = 786432.0f + 131072.0f,
                         pass_none = 786432.0f - 131072.0f;
};

// (z_threshold - the conservative lower edge, in z-space, of "score > theta" for one query - lives in bbq_kernel_common.h)

// ---- the threshold on the integer ------------------------------------------------------------------------------------------------
// With ax = lower, lx = upper - lower of the row, x1 its component sum, D the dimension, and ay, ly, y1 of the query
// (src/batchDotProduct.ts:478-617):
//     s = ay * (ax * D + lx * x1) + ly * (ax * y1 + lx * qc),       z = cs * s + ca * add      (cs, ca) = (2, -1) EUCLIDEAN, (1, 1) otherwise
// so for lx > 0 and ly > 0 (beta = cs * ly):
//     z > zth   <=>   qc > T = (zth / beta) * (1 / lx)  -  (ay / ly) * (rho * D + x1)  -  y1 * rho  -  (1 / beta) * (ca * add / lx),    rho = ax / lx.
// Per query (prologue, f64 -> f32):  qk = -S * {zth / beta, ay / ly, y1, 1 / beta}.   Per row (f32):  rk = {1 / lx, -(rho * D + x1), -rho, -ca * add / lx}.
// The accumulator starts at  K + qk . rk  with K = bias + slack: K first, then the four products one by one, the one with the row's
// popcount in it last (start_values(): the MFMAs that do not need the popcount are issued in front of it).
//
// Slack.  Let mag = S * sum_j max_q |q_j| * |r_j| (the row's magnitude budget, with |rho| * D + (a bound of |x1|) standing for |r_1|, plus
// S * the largest possible qcDist so that every term of s is covered).
//  * the sum: four fused multiply-adds onto K, each result inside the binade (guaranteed by mag < mag_limit, else the row is "weird"):
//    4 * 0.5 ulp (tests/test_prefilter_math_cpu.py checks this order, the products-first order and a plain FMA chain);
//  * the f32 images of the constants: q_j within 2^-24 (one rounding of an f64), 1 / lx within 2^-22 (v_rcp_f32 is good to 1 ulp, lx
//    itself is rounded once), rho and add / lx within 2^-21.4, r_1 within 2^-21.3 of |rho| * D + |x1|: every product within 2^-21 of its
//    magnitude, together below 2^-21 * mag;  the f64 evaluation of the reference score itself (~2^-50 of the same magnitudes) and
//    the inversion of the similarity transform (z_threshold's own allowance) are far inside.
// slack = (2.25 ulp + 2^-20 * mag) rounded up to whole ulps: above 2 ulp + twice the bound of the images.  A weird row (lx <= 0, non-finite, mag too large)
// gets zero constants and K = pass_all, a value inside the binade that no threshold reaches: every one of its pairs passes and is
// scored exactly, and the difference to the start value is still qcDist.  A query that accepts everything (no threshold yet) is not
// swept here at all: the prologue flags it, as its candidates would overflow every list of this kernel anyway.
// A row that the filter of a filtered sweep rejects (FILT, `accepted` false) gets zero constants as well, and K = pass_none: none of
// its pairs passes.  The reject comes last, so it holds for a weird row too: a rejected row is never scored, whatever it holds.
struct RowK {
  float r0, r1, r2, r3, K;
};
// `x1` is what r1 is made of; `x1_bound` >= |x1| is what the magnitude budget uses - the dimension for a row whose component sum is
// its popcount: every constant but r1 is then known before the popcount, and the start-value MFMAs that do not need r1 run in front
// of it (start_values: K first)
template <bool FP, bool FILT = false>
__device__ __forceinline__ RowK row_constants_early(double al, double au, double add, float x1_bound, float D, int sim, const float *__restrict__ gmax, float &rho_out, bool &ok_out,
                                                    bool accepted = true) {
  using N = MfmaNum<FP>;
  const float lxf = (float)(au - al), alf = (float)al, addf = (float)add;
  const float r0 = __builtin_amdgcn_rcpf(lxf);
  const float rho = alf * r0;
  RowK k;
  k.r0 = r0;
  k.r1 = 0.0f;
  k.r2 = -rho;
  k.r3 = (sim == 0 ? addf : -addf) * r0;
  // gmax: S * max over the workgroup's queries of |zth / beta|, |ay / ly|, |y1|, 1 / beta, and S * max sum of query values
  const float mag = fmaf(gmax[0], fabsf(r0), fmaf(gmax[1], fmaf(fabsf(rho), D, x1_bound), fmaf(gmax[2], fabsf(rho), fmaf(gmax[3], fabsf(k.r3), gmax[4]))));
  bool ok = lxf > 0.0f && mag < N::mag_limit;  // NaN anywhere: not ok
  if constexpr (FILT) ok = ok && accepted;     // (a rejected row's r1 stays zero with the others: the caller sets it by `ok`)
  if (ok) {
    k.K = N::bias + N::ulp * ceilf(fmaf(mag, 9.5367431640625e-07f / N::ulp, 2.25f));  // whole ulps above 2.25 ulp + 2^-20 * mag: 3 for an ordinary row
  } else {
    k.r0 = k.r2 = k.r3 = 0.0f;
    k.K = N::pass_all;
    if constexpr (FILT) k.K = accepted ? N::pass_all : N::pass_none;
  }
  rho_out = rho;
  ok_out = ok;
  return k;
}

template <int W, bool COMPACT>
struct TileRegs {
  u32x4 c[W];     // this lane's row: its code words
  f64x2 lu;       // {lower, upper}
  double add;      // additionalCorrection
  double x1;       // explicit quantizedComponentSum (has_x1 only)
};

template <int W, bool COMPACT>
__device__ __forceinline__ void load_tile_regs(TileRegs<W, COMPACT> &t, const IndexView &idx, int64_t tile, int lane) {
  const uint8_t *__restrict__ tp = idx.tiles + tile * (int64_t)idx.geom.tile_stride;
#pragma unroll
  for (int j = 0; j < W; ++j) t.c[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(tp) + lane + j * kTileRows);
  const uint8_t *__restrict__ cr = tp + tile_corr_offset(W);
  if constexpr (COMPACT) {
    const double *__restrict__ ex = idx.exact + (tile * kTileRows + lane) * 4;
    t.lu = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(ex));
    t.add = __builtin_nontemporal_load(ex + 2);
    t.x1 = 0.0;
  } else {
    t.lu = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(cr) + lane);
    t.add = __builtin_nontemporal_load(reinterpret_cast<const double *>(cr + kCorrAddOffset) + lane);
    t.x1 = idx.geom.has_x1 ? __builtin_nontemporal_load(reinterpret_cast<const double *>(cr + kCorrSumOffset) + lane) : 0.0;
  }
}

__device__ __forceinline__ int abits(float v) { return (int)__float_as_uint(v); }
__device__ __forceinline__ int abits(int v) { return v; }

// the 16 start values of a lane (16 queries x its row-group row): K + qk . rk as three chained v_mfma_f32_32x32x2_f32 on C = 0, K first
// (every addition rounds at the binade's ulp: four roundings, which the slack covers).  The same call on the same operands gives the
// same bits: the survivors' path calls it again.
__device__ __forceinline__ f32x16m start_values_early(float aq0, float aq1, float b0, float b1) {   // the two steps without the popcount
  f32x16m c = {0};
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(aq0, b0, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(aq1, b1, c, 0, 0, 0);
  return c;
}
template <bool FP>
__device__ __forceinline__ typename std::conditional<FP, f32x16m, i32x16m>::type start_values_finish(f32x16m c, float aq2, float b2) {
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(aq2, b2, c, 0, 0, 0);
  if constexpr (FP) return c;
  else return __builtin_bit_cast(i32x16m, c);   // the int8 form accumulates onto the float's bits
}
template <bool FP>
__device__ __forceinline__ typename std::conditional<FP, f32x16m, i32x16m>::type start_values(float aq0, float aq1, float aq2, float b0, float b1, float b2) {
  return start_values_finish<FP>(start_values_early(aq0, aq1, b0, b1), aq2, b2);
}

// ---- one k-step of the FP form, as a template over the step index: the fragment reads are inline asm (ds_read with an immediate
// offset, waited for by hand) because they must stay where they are written - one step ahead of their use.  Left to the compiler
// every step's fragment is read ahead of the loop (12 x 6 registers at 768-d: spills); volatile reads leave the LDS address space.
template <int G, int STEPS, int W>
__device__ __forceinline__ void fp_step(f32x16m &acc0, f32x16m &acc1, const u32x4 (&c)[W], u32x4 &bq, u32x2 &bq2, uint32_t addr16, uint32_t addr8) {
  // a lane supplies 32 of a step's 64 dimensions: ONE code word - word 2G of its row group's row n in the lower half-wave, word
  // 2G + 1 in the upper.  The tile's words were swapped in place for that (swap_code_words): [0] = {row n: 2G | row n: 2G + 1}, [1] =
  // the same of row 32 + n
  const uint32_t sw[2] = {(G & 1) == 0 ? c[G >> 1].x : c[G >> 1].z, (G & 1) == 0 ? c[G >> 1].y : c[G >> 1].w};
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bq), "+v"(bq2));   // this step's fragment has arrived
  i32x8m Q, R0, R1;   // 8 dwords wide for the builtin; FP6 uses 6 of them and FP4 4: the others stay undefined
  Q[0] = (int)bq.x; Q[1] = (int)bq.y; Q[2] = (int)bq.z; Q[3] = (int)bq.w; Q[4] = (int)bq2.x; Q[5] = (int)bq2.y;
  if constexpr (G + 1 < STEPS) {  // the next step's fragment, one step ahead: the read is issued BEFORE this step's MFMAs (their operand
                                  // passes through an asm behind it, or the compiler issues them first to reuse the registers)
    asm volatile("ds_read_b128 %0, %2 offset:%4\n\tds_read_b64 %1, %3 offset:%5"
                 : "=v"(bq), "=v"(bq2) : "v"(addr16), "v"(addr8), "n"((G + 1) * 1024), "n"((G + 1) * 512));
    asm volatile("" : "+v"(Q));
  }
  // bits 0, 1, 2 of every nibble where they stand are the FP4 numbers 0.5, 1.0, 2.0; bit 3 would be the sign: it moves to bit 0
  R0[0] = (int)(sw[0] & 0x11111111u); R0[1] = (int)(sw[0] & 0x22222222u); R0[2] = (int)(sw[0] & 0x44444444u); R0[3] = (int)((sw[0] >> 3) & 0x11111111u);
  R1[0] = (int)(sw[1] & 0x11111111u); R1[1] = (int)(sw[1] & 0x22222222u); R1[2] = (int)(sw[1] & 0x44444444u); R1[3] = (int)((sw[1] >> 3) & 0x11111111u);
  // A = queries (FP6 e2m3, cbsz 2), B = rows (FP4 e2m1, blgp 4), block scales 2^0
  acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(Q, R0, acc0, 2, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
  acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(Q, R1, acc1, 2, 4, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
  asm volatile("" : "+v"(acc0), "+v"(acc1));  // ordered with the reads: this step's MFMAs are issued before the next step begins
  if constexpr (G + 1 < STEPS) fp_step<G + 1, STEPS, W>(acc0, acc1, c, bq, bq2, addr16, addr8);
}

// FP form: swap(word 2s, word 2s + 1) of every lane's own row, in place, ONCE per tile: afterwards the first register of each pair
// holds {rows 0..31: word 2s | rows 0..31: word 2s + 1}, the second the same of rows 32..63 - the B operands of step s for the two row
// groups, for every group of queries the workgroup serves (per group and step it was a swap and, for all but the last group, two
// copies: the swap overwrites both of its operands)
template <int W>
__device__ __forceinline__ void swap_code_words(u32x4 (&c)[W]) {
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const auto s0 = __builtin_amdgcn_permlane32_swap(c[j].x, c[j].y, false, false);
    const auto s1 = __builtin_amdgcn_permlane32_swap(c[j].z, c[j].w, false, false);
    c[j].x = s0[0]; c[j].y = s0[1]; c[j].z = s1[0]; c[j].w = s1[1];
  }
}

// bytes of one group's staged query operands
__host__ __device__ constexpr int mfma_query_bytes(int w16, bool fp) { return fp ? w16 * 2 * 2 * 32 * 24 : w16 * 4 * 2 * 32 * 16; }

}  // namespace bbq
