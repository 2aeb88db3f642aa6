// bbq_rowlist.h - what the row-list score passes share (gfx950): span, group, range (a row addressed by tile and lane), gather and MaxSim
// over chosen groups (a row addressed by its ord), the fused MaxSim kernel (the group kernel's tile, once for a block of tokens).  One
// definition each of the row's terms, the query staging, the segmented maximum with its edge fold, and - host side - the ladder from an
// index's geometry and a call's plane count to a kernel's <QB, W, SB>.  Rows are scored with the sweep's own functions
// (bbq_kernel_common.h, bbq_scan_body.h), so every score is bit for bit what the dense sweep writes for that row.
// Everything device-side is __forceinline__: each kernel file gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_scan_body.h"

#pragma clang fp contract(off)

namespace bbq {

// ---- query staging ------------------------------------------------------------------------------------------------------------------

// The source addresses are the caller's: computed in here from the query's number, range and candidate kernels came out of this build's
// compiler with other register counts (profiles/rowlist_score_body_resources.txt).

// stage a query's planes (gp: `units` = w16 * QU 16-byte units) once per workgroup of NT threads, tid the thread's number
template <int NT>
__device__ __forceinline__ void stage_query_planes(u32x4 *s_planes, const u32x4 *gp, int units, int tid) {
  for (int i = tid; i < units; i += NT) s_planes[i] = gp[i];
}

// stage the planes (gp, `units` each) and uniforms (qp) of n tokens once per workgroup of NT threads: the tokens of a query lie back to back
constexpr int kParamUnits = sizeof(QueryParams) / 16;
template <int NT>
__device__ __forceinline__ void stage_token_block(u32x4 *s_planes, QueryParams *s_params, const u32x4 *gp, const QueryParams *qp, int n,
                                                  int units, int tid) {
  for (int i = tid; i < n * units; i += NT) s_planes[i] = gp[i];
  const u32x4 *gq = reinterpret_cast<const u32x4 *>(qp);
  u32x4 *sq = reinterpret_cast<u32x4 *>(s_params);
  for (int i = tid; i < n * kParamUnits; i += NT) sq[i] = gq[i];
}

// token t's uniforms out of LDS, those the score branches on made scalar: the same in every lane, the score's branches stay scalar
__device__ __forceinline__ QueryParams token_params(const QueryParams *s_params, int t) {
  QueryParams p = s_params[t];
  p.sim = __builtin_amdgcn_readfirstlane(p.sim);
  p.one_bit = __builtin_amdgcn_readfirstlane(p.one_bit);
  p.mip_plain = __builtin_amdgcn_readfirstlane(p.mip_plain);
  return p;
}

// ---- the row's terms ----------------------------------------------------------------------------------------------------------------

// what score_f64 (and, for the compact layout, the bound in front of it) takes of a row
struct RowTerms {
  f64x2 lu;        // the interval's lower and upper end
  double xadd, x1;  // the additional correction; the component sum
  uint32_t cw;     // the compact correction word (BOUND_FIRST alone)
  uint32_t qc, ones;
};

// The terms of lane `lane`'s row of the tile at tp (row = its ord), for the query staged at s_planes.  QB / W / SB as bbq_scan_kernel
// takes them; COMPACT: the corrections layout of the index - every row's exact corrections come from the side array, as in the dense
// sweep.  The row's component sum comes from the row_sums side array where the launch's view carries it and is counted otherwise - the
// same value either way.  `resident` as load_tile takes it.
// BOUND_FIRST (COMPACT alone; range search): the bound's terms first - the compact word -> cw, and the exact corrections are left to the
// caller, behind its bound.  Otherwise they are fetched here, up front.
template <int QB, int W, int SB, bool COMPACT, bool BOUND_FIRST = false>
__device__ __forceinline__ RowTerms tile_row_terms(const IndexView &idx, const uint8_t *__restrict__ tp, int64_t row, int lane, int w16,
                                                   bool resident, const u32x4 *__restrict__ s_planes) {
  const uint8_t *__restrict__ cr = tp + tile_corr_offset(w16);
  const bool rs = COMPACT && idx.row_sums != nullptr;  // uniform over the launch
  constexpr bool EXACT = COMPACT && !BOUND_FIRST;
  constexpr int CORR = COMPACT ? (BOUND_FIRST ? 1 : 0) : 2;
  RowTerms t = {{0.0, 0.0}, 0.0, 0.0, 0, 0, 0};
  if constexpr (W > 0) {
    u32x4 c[W];
    if (rs) {
      load_tile<W, CORR, true>(tp, lane, false, resident, idx.nt_delta, c, t.cw, t.lu, t.xadd, t.x1, idx.row_sums + row, &t.ones);
      if constexpr (EXACT) exact_corrections<true>(idx.exact, row, t.lu, t.xadd);
      if constexpr (SB == 1) t.qc = tile_popcounts<QB, W, false>(c, s_planes, t.ones);
      else tile_dot_multibit<QB, W, SB, false>(c, s_planes, t.qc, t.ones);
    } else {
      load_tile<W, CORR>(tp, lane, idx.geom.has_x1 != 0, resident, idx.nt_delta, c, t.cw, t.lu, t.xadd, t.x1);
      if constexpr (EXACT) exact_corrections<true>(idx.exact, row, t.lu, t.xadd);
      if constexpr (SB == 1) t.qc = tile_popcounts<QB, W>(c, s_planes, t.ones);
      else tile_dot_multibit<QB, W, SB>(c, s_planes, t.qc, t.ones);
    }
  } else {  // a row width without a compiled kernel: streamed chunk by chunk
    if constexpr (!COMPACT) {
      t.lu = BBQ_STREAM_LOAD(reinterpret_cast<const f64x2 *>(cr) + lane);
      t.xadd = BBQ_STREAM_LOAD(reinterpret_cast<const double *>(cr + kCorrAddOffset) + lane);
      if (idx.geom.has_x1) t.x1 = BBQ_STREAM_LOAD(reinterpret_cast<const double *>(cr + kCorrSumOffset) + lane);
    } else if constexpr (BOUND_FIRST) {
      t.cw = BBQ_STREAM_LOAD(reinterpret_cast<const uint32_t *>(cr) + lane);
    } else {
      exact_corrections<true>(idx.exact, row, t.lu, t.xadd);
    }
    if (rs) {
      t.ones = BBQ_STREAM_LOAD(idx.row_sums + row);
      if constexpr (SB == 1) t.qc = tile_popcounts_any<QB, false>(tp, lane, w16, s_planes, t.ones);
      else tile_dot_multibit_any<QB, SB, false>(tp, lane, w16, s_planes, t.qc, t.ones);
    } else {
      if constexpr (SB == 1) t.qc = tile_popcounts_any<QB>(tp, lane, w16, s_planes, t.ones);
      else tile_dot_multibit_any<QB, SB>(tp, lane, w16, s_planes, t.qc, t.ones);
    }
  }
  if (COMPACT || !idx.geom.has_x1) t.x1 = (double)t.ones;  // quantizedComponentSum of a freshly quantized row is its popcount / component sum
  return t;
}

// The loads of ord r's row, row-addressed: r is lane lr = r & 63 of the tile at tp = tiles + (r >> 6) * tile_stride (bbq_device.h), so
// its code chunks sit 1 KiB apart inside that tile's record and its corrections in the record's inline block or, for the compact layout,
// in exact[r].  Plain loads, default cache policy (bbq_gather_kernels.hip says why).  W > 0: the W code chunks -> c, in front of the
// corrections; rs: the row's component sum from the side array -> ones.  The caller puts its scheduling barrier behind the call, so that
// every load of the row is issued before the first is used.
template <int W, bool COMPACT>
__device__ __forceinline__ void load_row(const IndexView &idx, const uint8_t *__restrict__ tp, int lr, int64_t r, int w16, bool rs,
                                         u32x4 (&c)[W > 0 ? W : 1], f64x2 &lu, double &xadd, double &x1, uint32_t &ones) {
  if constexpr (W > 0) {
#pragma unroll
    for (int j = 0; j < W; ++j) c[j] = *reinterpret_cast<const u32x4 *>(tp + tile_chunk_offset(j, lr));
  }
  if constexpr (COMPACT) {
    exact_corrections(idx.exact, r, lu, xadd);
  } else {
    const uint8_t *__restrict__ cr = tp + tile_corr_offset(w16);
    lu = *(reinterpret_cast<const f64x2 *>(cr) + lr);
    xadd = *(reinterpret_cast<const double *>(cr + kCorrAddOffset) + lr);
    if (idx.geom.has_x1) x1 = *(reinterpret_cast<const double *>(cr + kCorrSumOffset) + lr);
  }
  if (rs) ones = idx.row_sums[r];
}

// the row's popcount does not depend on the token: counted once where the codes stay in registers over a block of tokens
template <int W>
__device__ __forceinline__ uint32_t row_popcount(const u32x4 (&c)[W], uint32_t ones) {
#pragma unroll
  for (int j = 0; j < W; ++j) ones = popc4_acc(c[j], ones);
  return ones;
}

// ---- the segmented maximum and the edge fold ----------------------------------------------------------------------------------------

// A wave's segments are the runs of lanes between two set bits of its heads word (bit 0 is always set: lane 0 opens one).
// the first lane of this lane's segment
__device__ __forceinline__ int segment_head(uint64_t heads, int lane) { return 63 - __clzll((long long)(heads & (~0ull >> (63 - lane)))); }
// (the last: lane == kTileRows - 1 || ((heads >> (lane + 1)) & 1ull), written out by the callers - as a function of this header the
// candidate kernel's run-time-width forms came out with two to six vector registers fewer)
// the inclusive segmented maximum: lane l takes the keys of the lanes between its segment's first lane and itself, so the last lane of a
// segment holds the segment's
__device__ __forceinline__ unsigned long long segment_max(unsigned long long key, int head, int lane) {
#pragma unroll
  for (int d = 1; d < kTileRows; d <<= 1) {
    const unsigned long long o = __shfl_up(key, (unsigned)d, kTileRows);
    if (lane - d >= head && o > key) key = o;
  }
  return key;
}

constexpr int kGroupEdges = 2 * kTilesPerChunk;  // LDS slots of a workgroup's edge segments (per token): two per wave
static_assert(kGroupEdges <= 64, "one wave merges the edge segments");

// Behind the barrier, one wave: the edge segments of the workgroup in row order, lane l < kGroupEdges holding slot l's key mk (0: none;
// 0 in the lanes beyond) and group mg - those of one group folded into the first of them, and each stored plainly into rep[slot] unless
// the group crosses the chunk's first or last row: those two, at most, are raised with atomicMax, as the neighbouring chunk's workgroup
// raises them.  (mk and mg as values, read by the caller: read in here, the group kernels came out with other register counts.)
__device__ __forceinline__ void fold_group_edges(const GroupScoreArgs &a, unsigned long long mk, uint32_t mg, unsigned long long *__restrict__ rep,
                                                 int64_t first_tile, int64_t n_tiles, int lane) {
  unsigned long long best = mk;
  bool leader = mk != 0ull;
#pragma unroll
  for (int j = 0; j < kGroupEdges; ++j) {
    const unsigned long long kj = __shfl(mk, j, kTileRows);
    const uint32_t gj = (uint32_t)__shfl((int)mg, j, kTileRows);
    if (mk != 0ull && kj != 0ull && gj == mg) {
      if (kj > best) best = kj;
      if (j < lane) leader = false;
    }
  }
  if (leader) {
    const int64_t next_tile = first_tile + kTilesPerChunk < n_tiles ? first_tile + kTilesPerChunk : n_tiles;
    const bool cut_lo = !(a.starts[first_tile] & 1ull) && mg == a.first_group[first_tile];  // the group began in front of the chunk
    const bool cut_hi = !(a.starts[next_tile] & 1ull) && mg == a.first_group[next_tile];    // ... goes on behind it
    unsigned long long *dst = rep + a.slot[mg];
    if (cut_lo || cut_hi) atomicMax(dst, best);
    else *dst = best;
  }
}

// ---- the launch ladder (host) -------------------------------------------------------------------------------------------------------

// (geom.store_bits, planes, geom.w16) -> <QB, W, SB> as bbq_scan_kernel takes them: f(Int<QB>, Int<W>, Int<SB>) is called with the
// three as types and its hipError_t returned; hipErrorInvalidValue for an unknown store_bits.  W = 0 is the run-time width.
// The compiled row widths are the sweep's (launch_scan_w, launch_scan_mb_w); tests/test_rowlist_cells_cpu.py reads the arms below and
// holds the width matrix of the row-list tests to them.
// MultiBitRows: whether multi-bit rows have compiled widths - not for a kernel whose compiled form is that of 1-bit rows alone
// (bbq_maxsim_cand_kernel): it takes every multi-bit row at W = 0, and no other <QB, W, SB> is instantiated for it.
template <int N> using Int = std::integral_constant<int, N>;
enum class MultiBitRows { kCompiledWidths, kRunTimeWidth };

template <int QB, class F>
hipError_t rowlist_width(int w16, F &f) {
  switch (w16) {
    case 1: return f(Int<QB>{}, Int<1>{}, Int<1>{});    // dim <= 128
    case 6: return f(Int<QB>{}, Int<6>{}, Int<1>{});    // dim 768
    case 8: return f(Int<QB>{}, Int<8>{}, Int<1>{});    // dim 1024
    case 12: return f(Int<QB>{}, Int<12>{}, Int<1>{});  // dim 1536
    default: return f(Int<QB>{}, Int<0>{}, Int<1>{});
  }
}
template <int QB, int SB, MultiBitRows MB, class F>
hipError_t rowlist_width_mb(int w16, F &f) {
  if constexpr (MB == MultiBitRows::kCompiledWidths) {
    switch (w16) {
      case 12: return f(Int<QB>{}, Int<12>{}, Int<SB>{});
      case 16: return f(Int<QB>{}, Int<16>{}, Int<SB>{});
      default: return f(Int<QB>{}, Int<0>{}, Int<SB>{});
    }
  } else {
    return f(Int<QB>{}, Int<0>{}, Int<SB>{});
  }
}
template <MultiBitRows MB = MultiBitRows::kCompiledWidths, class F>
hipError_t rowlist_ladder(const TileGeom &geom, int planes, F f) {
  switch (geom.store_bits) {
    case 1:
      switch (planes) {
        case 1: return rowlist_width<1>(geom.w16, f);
        case 2: return rowlist_width<2>(geom.w16, f);
        case 4: return rowlist_width<4>(geom.w16, f);
        default: return rowlist_width<8>(geom.w16, f);
      }
    case 2: return planes > 4 ? rowlist_width_mb<8, 2, MB>(geom.w16, f) : rowlist_width_mb<4, 2, MB>(geom.w16, f);
    case 4: return planes > 4 ? rowlist_width_mb<8, 4, MB>(geom.w16, f) : rowlist_width_mb<4, 4, MB>(geom.w16, f);
    case 8: return f(Int<8>{}, Int<0>{}, Int<8>{});
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bbq
