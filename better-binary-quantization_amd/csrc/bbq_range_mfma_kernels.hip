// bbq_range_mfma_kernels.hip - the count pass of the range search on the matrix cores (sweep_share 32; gfx950).
//
// bbq_range_kernel counts one query per workgroup: 64 queries are 64 sweeps of the index.  Here a workgroup loads a tile once for 32 or
// 64 queries, as bbq_scan_mfma_kernel does for the top-k search (bbq_mfma_kernels.hip, whose derivations this file relies on and whose
// device pieces it shares through bbq_mfma_common.h): the queries' thresholds are known before the launch, so "score >= threshold" is the
// start value of the accumulator, the contraction runs as FP6 x FP4 on v_mfma_f32_32x32x64_f8f6f4 (query values <= 15) or on
// v_mfma_i32_32x32x32_i8 (<= 127), and only the pairs that end above the bias are scored - by score_f64 and exact_key_passes, the two
// functions bbq_range_kernel decides with.  The pre-filter is conservative and a weird row passes it for every query, so the same rows
// pass and every chunk's count is the per-query kernel's.
//
// What is this kernel's own: it emits nothing but counts.  No candidate entries, no staged lists, no append lists, no flush at the end.
// A survivor that passes the exact test bumps an LDS counter [wave][query slot]; behind the last group of a tile the lanes that own a
// slot add their counter to counts[query][chunk] with a u32 atomicAdd whose result nobody reads (eight waves share a chunk's word;
// integer addition does not depend on the order of arrival, so the counts are the same bytes from run to run - the host clears them in
// front of the launch).  A query the pre-filter cannot serve is not counted here but FLAGGED in recount[]: by the host before the launch
// (no positive finite interval width: mfma_query_ok), by the prologue (a key below every score: every row passes, nothing to pre-filter)
// or by a wave whose survivor queue is full (a loose threshold).  A flagged query's counts are garbage; the host overwrites them with
// bbq_range_kernel's (bbq_range.cpp).  A query flagged at entry or by the prologue is absent: its lane gets the start values of a lane
// without a query, and a weird row's pairs of it are dropped as those of a slot beyond the last query are.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <algorithm>
#include <type_traits>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_launch.h"

#pragma clang fp contract(off)

#include "bbq_mfma_common.h"

namespace bbq {

struct RangeMfmaArgs {
  IndexView idx;
  const QueryParams *qparams;  // [Q]
  const Threshold *theta;      // [Q] bbq_range_theta_kernel's
  uint32_t *counts;            // [Q][n_chunks], cleared by the host
  uint32_t *recount;           // [Q] not zero: the query's counts are not this kernel's to give
  const uint8_t *qbytes;       // the queries as matrix-core operands, as MfmaArgs::qbytes (stage_queries_mfma, bbq_query.cpp)
  const float *qmax;           // [groups][4] as MfmaArgs::qmax
  int32_t n_chunks;            // chunks of idx
  int32_t nq_total;
  int32_t chunks_per_block;    // consecutive chunks one workgroup walks with the same staged queries
  float fp_scale;              // FP form: every product is fp_scale * q
  int32_t queue_cap;           // survivors per wave, tile and group that wait for their exact scores
};

// Grid (runs of chunks_per_block chunks, groups of G x 32 queries); a workgroup is kChunkRows / 64 waves and a wave is one tile of each
// chunk of its run.  W / COMPACT / FP / G / Accept as bbq_scan_mfma_kernel takes them: with the accept words of a filter a wave walks
// only the tiles of its slot whose word is not zero, and a rejected row of a tile it sweeps starts at pass_none.
template <int W, bool COMPACT, bool FP, int G, class... Accept>
__global__ __launch_bounds__(kChunkRows, W <= 8 ? 4 : 2) void bbq_range_mfma_kernel(const RangeMfmaArgs a, const Accept... accept_arg) {
  constexpr bool FILT = sizeof...(Accept) > 0;
  static_assert(sizeof...(Accept) <= 1, "at most the accept words");
  const uint64_t *__restrict__ accept = nullptr;
  if constexpr (FILT) accept = (accept_arg, ...);
  (void)accept;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using N = MfmaNum<FP>;
  using Acc = typename std::conditional<FP, f32x16m, i32x16m>::type;
  constexpr int NT = kChunkRows;
  constexpr int NW = kChunkRows / 64;
  constexpr int WORDS = W * 4;
  constexpr int STEPS = FP ? WORDS / 2 : WORDS;
  constexpr int QBYTES = mfma_query_bytes(W, FP);
  constexpr int nqb = G * kMfmaQueries;                                              // query slots of this workgroup
  const float S = FP ? a.fp_scale : 1.0f;
  const int qcap = a.queue_cap;
  // (range_mfma_smem_bytes restates this layout)
  f32x4 *s_qk = reinterpret_cast<f32x4 *>(smem + (size_t)G * QBYTES);               // [nqb] -S * {zth/beta, ay/ly, y1, 1/beta}
  f64x2 *s_lu = reinterpret_cast<f64x2 *>(s_qk + nqb);                               // [NW][64] {lower, upper} of every tile row ...
  f64x2 *s_ax = s_lu + NW * 64;                                                      // [NW][64] ... and {additionalCorrection, component sum}
  uint32_t *s_queue = reinterpret_cast<uint32_t *>(s_ax + NW * 64);                  // [NW][qcap]
  uint32_t *s_qcount = s_queue + NW * qcap;                                          // [NW]
  QueryParams *s_qp = reinterpret_cast<QueryParams *>(s_qcount + 8);                 // [nqb]
  float *s_gmax = reinterpret_cast<float *>(s_qp + nqb);                             // [8]
  uint32_t *s_key = reinterpret_cast<uint32_t *>(s_gmax + 8);                        // [nqb] the queries' threshold keys
  uint32_t *s_cnt = s_key + nqb;                                                     // [NW][nqb] passing rows of the wave's current tile
  uint32_t *s_present = s_cnt + NW * nqb;                                            // [2] bit s: slot s holds a query this kernel counts

  const int q0 = blockIdx.y * nqb;
  const int nb = min(nqb, a.nq_total - q0);                                          // queries present here
  const int ng = (nb + kMfmaQueries - 1) / kMfmaQueries;                             // groups present here
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 31, h = lane >> 5;
  const int64_t n_tiles = (a.idx.n_rows + kTileRows - 1) / kTileRows;
  const int cpb = a.chunks_per_block;
  const int lc0 = blockIdx.x * cpb;
  TileRegs<W, COMPACT> t;
  // FILT: the walk over the slot's tiles with an accepted row, as in bbq_scan_mfma_kernel - all wave-uniform
  int ci_first = 0, ci_step = 0, cend = 0;
  uint64_t aw = 0;
  AcceptWords awords = nullptr;
  (void)ci_first, (void)ci_step, (void)cend, (void)aw, (void)awords;
  if constexpr (FILT) {
    const int64_t t0 = (int64_t)lc0 * kTilesPerChunk + __builtin_amdgcn_readfirstlane(wave);
    cend = (int)max((int64_t)0, min((int64_t)min(cpb, a.n_chunks - lc0), (n_tiles - t0 + kTilesPerChunk - 1) / kTilesPerChunk));
    awords = (AcceptWords)accept + t0;
    for (; ci_first < cend; ++ci_first) {
      aw = awords[(int64_t)ci_first * kTilesPerChunk];
      if (aw != 0) break;
    }
    int lane_first = lane;
    asm volatile("" : "+v"(lane_first));
    if (ci_first < cend) load_tile_regs<W, COMPACT>(t, a.idx, t0 + (int64_t)ci_first * kTilesPerChunk, lane_first);
  } else {
    const int64_t t0 = (int64_t)lc0 * kTilesPerChunk + wave;
    if (lc0 < a.n_chunks && t0 < n_tiles) load_tile_regs<W, COMPACT>(t, a.idx, t0, lane);
  }
  // prologue: wave 0 derives the queries' constants while the other waves stage the query fragments and clear the counters
  if (wave == 0) {
    if (lane < 8) s_gmax[lane] = 0.0f;   // same wave as the atomicMax below: LDS operations of a wave execute in order
    if (lane < NW) s_qcount[lane] = 0;
    bool present = false;
    if (lane < nqb) {
      QueryParams p{};
      uint32_t key = 0xFFFFFFFFu;
      f32x4 qk;
      // a slot without a query: the largest finite threshold - nothing of an ordinary row passes (a weird row's pairs are dropped later)
      qk.x = -3.0e38f; qk.y = 0.0f; qk.z = 0.0f; qk.w = 0.0f;
      if (lane < nb) {
        p = a.qparams[q0 + lane];   // (also of a flagged query: slot 0's similarity is the call's)
        if (a.recount[q0 + lane] == 0u) {
          key = a.theta[q0 + lane].key;
          const double zt = z_threshold(key, p);
          const double beta = (p.sim == 0 ? 2.0 : 1.0) * p.ly;   // > 0 and finite: the host has flagged every other query (mfma_query_ok)
          const double A = -(double)S * (zt / beta);
          if (A < 1.0e30) {  // (also false for NaN)
            qk.x = A > -3.0e38 ? (float)A : -3.0e38f;            // a threshold beyond every score: nothing passes
            // kept finite: mfma_query_ok admits |ay / ly| up to 1e60, an infinite f32.  Every row is weird for such a query (its magnitude
            // budget is infinite), so this constant only ever meets r1 = 0 - where inf x 0 would make the start value NaN
            qk.y = fminf(fmaxf((float)(-(double)S * (p.ay / p.ly)), -3.0e38f), 3.0e38f);
            qk.z = (float)(-(double)S * p.y1);
            qk.w = (float)(-(double)S / beta);
            if (fabsf(qk.x) < 1.0e30f) atomicMax(reinterpret_cast<uint32_t *>(s_gmax), __float_as_uint(fabsf(qk.x) * 1.0000002f));
            present = true;
          } else {
            // a key below every score (-inf is one): every row passes and there is nothing to pre-filter - the per-query kernel counts it
            a.recount[q0 + lane] = 1u;
          }
        }
      }
      s_qp[lane] = p;
      s_key[lane] = key;
      s_qk[lane] = qk;
      if (lane == 0) {  // the host's maxima are S-free and rounded up; the workgroup's groups share one budget
        float g1 = 0.0f, g2 = 0.0f, g3 = 0.0f, g4 = 0.0f;
        for (int g = 0; g < ng; ++g) {
          const float *__restrict__ gm = a.qmax + (size_t)(blockIdx.y * G + g) * 4;
          g1 = fmaxf(g1, gm[0]); g2 = fmaxf(g2, gm[1]); g3 = fmaxf(g3, gm[2]); g4 = fmaxf(g4, gm[3]);
        }
        s_gmax[1] = S * g1;
        s_gmax[2] = S * g2;
        s_gmax[3] = S * g3;
        s_gmax[4] = S * g4;
      }
    }
    const unsigned long long pm = __ballot(present);
    if (lane == 0) { s_present[0] = (uint32_t)pm; s_present[1] = (uint32_t)(pm >> 32); }
  } else {
    const u32x4 *__restrict__ gb = reinterpret_cast<const u32x4 *>(a.qbytes + (size_t)blockIdx.y * G * QBYTES);
    u32x4 *__restrict__ sb = reinterpret_cast<u32x4 *>(smem);
    for (int i = tid - 64; i < ng * (QBYTES / 16); i += NT - 64) sb[i] = gb[i];
    for (int i = tid - 64; i < NW * nqb; i += NT - 64) s_cnt[i] = 0;
  }
  __syncthreads();

  const int sim = s_qp[0].sim;                  // uniform over the call
  const float Df = (float)a.idx.geom.dim;
  // the slots that hold a query of this kernel's, per group: wave-uniform
  uint32_t present_of[G];
#pragma unroll
  for (int g = 0; g < G; ++g) present_of[g] = __builtin_amdgcn_readfirstlane(s_present[g]);
#pragma unroll 1
  for (int ci = FILT ? ci_first : 0; ci < (FILT ? cend : cpb); ci = FILT ? ci_step : ci + 1) {
  const int lc = lc0 + ci;
  if (lc >= a.n_chunks) break;       // block-uniform
  const int64_t tile_v = (int64_t)lc * kTilesPerChunk + wave;
  const int64_t tile = ((int64_t)__builtin_amdgcn_readfirstlane((int)(tile_v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)tile_v);
  uint64_t aw_next = 0, aw_ahead = 0;
  (void)aw_next, (void)aw_ahead;
  if constexpr (FILT) ci_step = cend;
  if constexpr (FILT) aw_ahead = awords[(int64_t)min(ci + 1, cend - 1) * kTilesPerChunk];

  if (tile < n_tiles) {  // wave-uniform: a wave's tile of the last chunk may not exist
    // ---- my row's constants (tile row `lane`), every one but r1 first: the start-value MFMAs that do not need the popcount run in front of it
    float rho;
    bool row_ok;
    RowK mine = row_constants_early<FP, FILT>(t.lu.x, t.lu.y, t.add, a.idx.geom.has_x1 ? fabsf((float)t.x1) * 1.0000002f : Df, Df, sim, s_gmax, rho, row_ok,
                                              !FILT || ((aw >> lane) & 1ull) != 0);
    const auto b0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine.K), __float_as_uint(mine.r0), false, false);
    const auto b1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine.r2), __float_as_uint(mine.r3), false, false);
    int lds_off0;
    asm volatile("v_mov_b32 %0, 0" : "=v"(lds_off0));
    float aqf[3];
    {
      const f32x4 qkm = s_qk[n + lds_off0];
      aqf[0] = h ? qkm.x : 1.0f;    // step 0: K x 1 + qk[0] r0
      aqf[1] = h ? qkm.w : qkm.z;   // step 1: qk[2] r2 + qk[3] r3
      aqf[2] = h ? 0.0f : qkm.y;    // step 2: qk[1] r1 (the row's popcount is in r1)
    }
    f32x16m e0 = start_values_early(aqf[0], aqf[1], __uint_as_float(b0[0]), __uint_as_float(b1[0]));
    f32x16m e1 = start_values_early(aqf[0], aqf[1], __uint_as_float(b0[1]), __uint_as_float(b1[1]));
#pragma unroll
    for (int j = 0; j < W; ++j) asm volatile("" : "+v"(e0), "+v"(e1), "+v"(t.c[j]));
    uint32_t ones = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) ones += __popc(t.c[j].x) + __popc(t.c[j].y) + __popc(t.c[j].z) + __popc(t.c[j].w);
    double x1row = (double)ones;                 // quantizedComponentSum of a 1-bit row is its popcount ...
    if (a.idx.geom.has_x1) x1row = t.x1;         // ... unless the index says otherwise
    mine.r1 = row_ok ? -fmaf(rho, Df, (float)x1row) : 0.0f;
    s_lu[wave * 64 + lane] = t.lu;               // for the survivors' exact scores (any lane may score any row of the tile)
    {
      f64x2 ax;
      ax.x = t.add; ax.y = x1row;
      s_ax[wave * 64 + lane] = ax;
    }
    const auto b2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine.r1), 0u, false, false);
    float rb[2][3];
#pragma unroll
    for (int rg = 0; rg < 2; ++rg) { rb[rg][0] = __uint_as_float(b0[rg]); rb[rg][1] = __uint_as_float(b1[rg]); rb[rg][2] = __uint_as_float(b2[rg]); }
    const int rows_here = (int)min((int64_t)kTileRows, a.idx.n_rows - tile * kTileRows);
    uint32_t *__restrict__ queue = s_queue + (size_t)wave * qcap;
    bool counted = false;                        // wave-uniform: a survivor of this tile went through the exact test
    if constexpr (FP) swap_code_words<W>(t.c);   // (the popcount above wanted the words as they were loaded)
#pragma unroll
    for (int g = 0; g < G; ++g) {
    int lds_off;
    asm volatile("v_mov_b32 %0, 0" : "=v"(lds_off));
    const int gq = g * kMfmaQueries;             // first query slot of this group
    const u32x4 *__restrict__ s_B = reinterpret_cast<const u32x4 *>(smem + (size_t)g * QBYTES);
    const u32x2 *__restrict__ s_B2 = reinterpret_cast<const u32x2 *>(smem + (size_t)g * QBYTES + (size_t)STEPS * 2 * 32 * 16);
    float aq0, aq1, aq2;
    Acc acc0, acc1;
    if (g == 0) {   // (compile time: the groups are unrolled) begun in front of the popcount
      aq0 = aqf[0]; aq1 = aqf[1]; aq2 = aqf[2];
      acc0 = start_values_finish<FP>(e0, aq2, rb[0][2]);
      acc1 = start_values_finish<FP>(e1, aq2, rb[1][2]);
    } else {
      const f32x4 qkm = s_qk[gq + n + lds_off];
      aq0 = h ? qkm.x : 1.0f;
      aq1 = h ? qkm.w : qkm.z;
      aq2 = h ? 0.0f : qkm.y;
      acc0 = start_values<FP>(aq0, aq1, aq2, rb[0][0], rb[0][1], rb[0][2]);
      acc1 = start_values<FP>(aq0, aq1, aq2, rb[1][0], rb[1][1], rb[1][2]);
    }
    // ---- the contraction: C[m = query][n = row of the group] += sum over the k-steps
    if constexpr (FP) {
      int hq = h, nq = n;
      if constexpr (FILT) asm volatile("" : "+v"(hq), "+v"(nq));
      const uint32_t addr16 = (uint32_t)(uintptr_t)(s_B + hq * 32 + nq + lds_off), addr8 = (uint32_t)(uintptr_t)(s_B2 + hq * 32 + nq + lds_off);
      u32x4 bq;
      u32x2 bq2;
#pragma unroll
      for (int j = 0; j < W; ++j) asm volatile("" : "+v"(t.c[j]));
      asm volatile("ds_read_b128 %0, %2\n\tds_read_b64 %1, %3" : "=v"(bq), "=v"(bq2) : "v"(addr16), "v"(addr8));
      fp_step<0, STEPS, W>(acc0, acc1, t.c, bq, bq2, addr16, addr8);
    } else {
#pragma unroll
      for (int w8 = 0; w8 < WORDS; ++w8) {
        const uint32_t w = (w8 & 3) == 0 ? t.c[w8 >> 2].x : (w8 & 3) == 1 ? t.c[w8 >> 2].y : (w8 & 3) == 2 ? t.c[w8 >> 2].z : t.c[w8 >> 2].w;
        const auto sw = __builtin_amdgcn_permlane32_swap(w, w >> 4, false, false);
        const u32x4 bq = s_B[(w8 * 2 + h) * 32 + n + lds_off];
        i32x4m Q;
        Q.x = (int)bq.x; Q.y = (int)bq.y; Q.z = (int)bq.z; Q.w = (int)bq.w;
        i32x4m R0, R1;
        R0.x = (int)(sw[0] & 0x01010101u); R0.y = (int)((sw[0] >> 1) & 0x01010101u); R0.z = (int)((sw[0] >> 2) & 0x01010101u); R0.w = (int)((sw[0] >> 3) & 0x01010101u);
        R1.x = (int)(sw[1] & 0x01010101u); R1.y = (int)((sw[1] >> 1) & 0x01010101u); R1.z = (int)((sw[1] >> 2) & 0x01010101u); R1.w = (int)((sw[1] >> 3) & 0x01010101u);
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(Q, R0, acc0, 0, 0, 0);   // A = queries (m), B = rows (n)
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(Q, R1, acc1, 0, 0, 0);
      }
    }
    // ---- the codes are consumed by the last group: the next tile of this wave slot goes into the same registers while this one is tested
    if (g + 1 == G) {
      const int64_t tn = tile + kTilesPerChunk;
      int lane_here = lane;
      asm volatile("" : "+v"(lane_here));
      if constexpr (FILT) {
        int cn = ci + 1;
        uint64_t wn = aw_ahead;
        while (cn < cend && wn == 0) {
          ++cn;
          wn = awords[(int64_t)min(cn, cend - 1) * kTilesPerChunk];
        }
        if (cn < cend) {
          load_tile_regs<W, COMPACT>(t, a.idx, tile + (int64_t)(cn - ci) * kTilesPerChunk, lane_here);
        } else {
          t.lu.x = t.lu.y = t.add = t.x1 = 0.0;
        }
        ci_step = cn;
        aw_next = wn;
      } else {
        if (ci + 1 < cpb && lc + 1 < a.n_chunks && tn < n_tiles) load_tile_regs<W, COMPACT>(t, a.idx, tn, lane_here);
      }
    }
    // ---- any accumulator above the bias?  (compared as integers in both forms, one v_max3_i32 per two accumulators)
    int mx = max(max(abits(acc0[0]), abits(acc0[1])), abits(acc0[2]));
#pragma unroll
    for (int r = 3; r < 15; r += 2) mx = max(max(mx, abits(acc0[r])), abits(acc0[r + 1]));
    mx = max(max(mx, abits(acc0[15])), abits(acc1[0]));
#pragma unroll
    for (int r = 1; r < 15; r += 2) mx = max(max(mx, abits(acc1[r])), abits(acc1[r + 1]));
    mx = max(mx, abits(acc1[15]));
    const bool any_lane = mx > (int)__float_as_uint(N::bias);
    if (__any(any_lane)) {
      // survivors: qcDist from the difference to the start value, derived again from operands that pass through an empty asm
      float rc[2][3];
#pragma unroll
      for (int rg = 0; rg < 2; ++rg)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          rc[rg][j] = rb[rg][j];
          asm volatile("" : "+v"(rc[rg][j]));
        }
      int h2 = h, n2 = n;
      asm volatile("" : "+v"(h2), "+v"(n2));
      const uint32_t pres = present_of[g];
#pragma unroll
      for (int rg = 0; rg < 2; ++rg) {
        const int rit = 32 * rg + n2;
        const Acc &accv = rg == 0 ? acc0 : acc1;
        bool any_rg = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) any_rg = any_rg || abits(accv[r]) > (int)__float_as_uint(N::bias);
        if (!__any(any_rg)) continue;  // wave-uniform
        const Acc init = start_values<FP>(aq0, aq1, aq2, rc[rg][0], rc[rg][1], rc[rg][2]);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const auto av = accv[r];
          const bool above = abits(av) > (int)__float_as_uint(N::bias);
          if (__any(above)) {  // wave-uniform: most accumulators have no survivor in any lane
            const int m = (r & 3) + 8 * (r >> 2) + 4 * h2;
            // (a slot without a query of this kernel's: only a weird row's pairs get here.  FILT: the accept bit as a second guard)
            if (above && ((pres >> m) & 1u) != 0 && rit < rows_here && (!FILT || ((aw >> rit) & 1ull) != 0)) {
              uint32_t qc;
              if constexpr (FP) qc = (uint32_t)((av - init[r]) * (1.0f / S));   // both on the 1/16 grid inside one binade: exact
              else qc = (uint32_t)(av - init[r]);
              const uint32_t slot = atomicAdd(&s_qcount[wave], 1u);
              if (slot < (uint32_t)qcap) queue[slot] = qc | ((uint32_t)rit << 20) | ((uint32_t)m << 26);
              else a.recount[q0 + gq + m] = 1u;  // more survivors than the queue holds: this query is counted on its own
            }
          }
        }
      }
      // ---- the exact test of the survivors (same-wave LDS traffic: program order is enough)
      const uint32_t n_pass = min(s_qcount[wave], (uint32_t)qcap);
      for (uint32_t i = lane; i < n_pass; i += 64) {
        const uint32_t e = queue[i];
        const int qc = (int)(e & 0xFFFFFu), rit = (int)((e >> 20) & 63u), qn = gq + (int)(e >> 26);
        const QueryParams pq = s_qp[qn];
        const f64x2 lu = s_lu[wave * 64 + rit], ax = s_ax[wave * 64 + rit];
        const float s32 = (float)score_f64((double)qc, lu.x, lu.y, ax.x, ax.y, pq);
        bool nan = false;  // a NaN score is in no answer and raises nothing here
        if (exact_key_passes(true, s32, s_key[qn], nan)) atomicAdd(&s_cnt[__builtin_amdgcn_readfirstlane(wave) * nqb + qn], 1u);
      }
      s_qcount[wave] = 0;  // this wave's queue is its own: ready for its next group or tile
      counted = true;
    }
    }  // groups of this workgroup
    // ---- the tile's counts: the lane that owns a slot adds what its wave counted to the chunk's word of that query.  Nothing waits for
    // the atomic's result, and the sum does not depend on the order the chunk's waves arrive in
    if (counted) {  // (the lane through an empty asm: the counter's address is derived here, not carried around the loop)
      int lane_c = lane;
      asm volatile("" : "+v"(lane_c));
      if (lane_c < nqb) {
        uint32_t *__restrict__ mine_c = s_cnt + __builtin_amdgcn_readfirstlane(wave) * nqb + lane_c;
        const uint32_t c = *mine_c;
        if (c != 0u) {
          atomicAdd(a.counts + (size_t)(q0 + lane_c) * a.n_chunks + lc, c);
          *mine_c = 0u;
        }
      }
    }
  }
  if constexpr (FILT) aw = aw_next;
  }  // chunks of this workgroup
}

// ---------------------------------------------------------------------------------------------------------------------

namespace {

size_t range_mfma_smem_bytes(int w16, bool fp, int gpb, int queue_cap) {
  constexpr size_t NW = kChunkRows / 64;
  const size_t nqb = (size_t)gpb * kMfmaQueries;
  return (size_t)gpb * mfma_query_bytes(w16, fp) + nqb * 16 + NW * 64 * 32 + NW * queue_cap * 4 + 32 + nqb * sizeof(QueryParams) + 32 + nqb * 4 + NW * nqb * 4 + 16;
}

constexpr int kMaxChunksPerBlock = 16;  // as the top-k launch's

// (the int8 form up to 1024-d has one group per workgroup, as in bbq_scan_mfma_kernel: with two its fragment reads spill)
constexpr bool two_groups_built(int w16, bool fp) { return fp || w16 > 8; }

// two groups per tile load where the call has them and the LDS fits the CU as the top-k kernel's does: two workgroups per CU up to
// 1024-d, one beyond
int groups_per_block(int w16, int groups, bool fp) {
  if (groups < 2 || !two_groups_built(w16, fp)) return 1;
  const size_t two = range_mfma_smem_bytes(w16, fp, 2, mfma_queue_cap(2));
  const size_t lds_alloc = (two + 1279) / 1280 * 1280;  // LDS is handed out in 1280-byte blocks
  return (w16 <= 8 ? 2 * lds_alloc <= 160 * 1024 : two <= 150 * 1024) ? 2 : 1;
}

template <int W, bool COMPACT, bool FP, int G>
hipError_t launch_g(const RangeMfmaArgs &a, const uint64_t *accept, dim3 grid, size_t smem, hipStream_t s) {
  dim3 block(kChunkRows, 1, 1);
  if (accept) {
    auto kern = bbq_range_mfma_kernel<W, COMPACT, FP, G, const uint64_t *>;
    if (smem > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, block, smem, s, a, accept);
    return hipGetLastError();
  }
  auto kern = bbq_range_mfma_kernel<W, COMPACT, FP, G>;
  if (smem > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, grid, block, smem, s, a);
  return hipGetLastError();
}

template <int W, bool COMPACT, bool FP>
hipError_t launch_t(RangeMfmaArgs a, const uint64_t *accept, hipStream_t s) {
  const int groups = (a.nq_total + kMfmaQueries - 1) / kMfmaQueries;
  const int gpb = groups_per_block(W, groups, FP);
  a.queue_cap = mfma_queue_cap(gpb);
  const size_t smem = range_mfma_smem_bytes(W, FP, gpb, a.queue_cap);
  // chunks per workgroup by the top-k launch's rule (launch_mfma_t, bbq_mfma_kernels.hip): one round of resident workgroups up to 12
  // chunks each, beyond that about sqrt(2 x prologue x chunks / slots)
  const int grid_y = (groups + gpb - 1) / gpb;
  const int64_t units = (int64_t)a.n_chunks * grid_y;
  int64_t cpb = (units + 511) / 512;
  if (cpb > 12) cpb = std::min<int64_t>(kMaxChunksPerBlock, std::max<int64_t>(4, (int64_t)llround(sqrt((double)units / 220.0))));
  a.chunks_per_block = (int)cpb;
  dim3 grid((unsigned)((a.n_chunks + a.chunks_per_block - 1) / a.chunks_per_block), (unsigned)grid_y, 1);
  if constexpr (two_groups_built(W, FP)) {
    if (gpb == 2) return launch_g<W, COMPACT, FP, 2>(a, accept, grid, smem, s);
  }
  return launch_g<W, COMPACT, FP, 1>(a, accept, grid, smem, s);
}

template <int W>
hipError_t launch_w(const RangeMfmaArgs &a, const uint64_t *accept, bool compact, bool fp, hipStream_t s) {
  if (compact) return fp ? launch_t<W, true, true>(a, accept, s) : launch_t<W, true, false>(a, accept, s);
  return fp ? launch_t<W, false, true>(a, accept, s) : launch_t<W, false, false>(a, accept, s);
}

}  // namespace

bool range_mfma_supported(const TileGeom &g) {
  if (g.store_bits != 1 || !(g.w16 == 1 || g.w16 == 6 || g.w16 == 8 || g.w16 == 12)) return false;
  return range_mfma_smem_bytes(g.w16, false, 1, mfma_queue_cap(1)) <= 150 * 1024;
}

int range_mfma_queries_per_tile_load(const TileGeom &g, int n_queries, bool fp) {
  return kMfmaQueries * groups_per_block(g.w16, (n_queries + kMfmaQueries - 1) / kMfmaQueries, fp);
}

hipError_t launch_range_count_mfma(const RangeArgs &ra, const uint8_t *qbytes, const float *qmax, float fp_scale, uint32_t *recount, int n_queries, hipStream_t s) {
  if (!range_mfma_supported(ra.idx.geom) || !recount || ra.q_first != 0) return hipErrorInvalidValue;
  if (n_queries <= 0 || ra.n_chunks <= 0) return hipSuccess;
  const bool fp = fp_scale > 0.0f;
  const RangeMfmaArgs a{ra.idx, ra.qparams, ra.theta, ra.counts, recount, qbytes, qmax, ra.n_chunks, n_queries, 1, fp_scale, mfma_queue_cap(1)};
  const bool compact = ra.idx.geom.layout == kLayoutCompact;
  switch (ra.idx.geom.w16) {
    case 1: return launch_w<1>(a, ra.accept, compact, fp, s);
    case 6: return launch_w<6>(a, ra.accept, compact, fp, s);
    case 8: return launch_w<8>(a, ra.accept, compact, fp, s);
    case 12: return launch_w<12>(a, ra.accept, compact, fp, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bbq
