// bbq_group_kernels.hip - grouped search (gfx950): bbq_search_grouped_batch.
//
// The k best groups of rows, each through its best accepted row.  Groups are contiguous runs of rows (a document's chunks); a group set
// (bbq_group.cpp) describes them once, in three small tables.  Two passes of this file stand in front of the span search's select pass.
// The score pass streams the whole index for every query of a sub-batch - a workgroup is one chunk for one query, a wave one tile, a
// lane one row, scored with the sweep's own functions (bbq_kernel_common.h, bbq_scan_body.h: bit for bit what the dense sweep writes) -
// and reduces the rows of each group to ONE packed key, the representative's (group_key, bbq_device.h): a segmented maximum inside the
// wave, the segments that cross a tile's edge merged in LDS by one wave, and a 64-bit atomic maximum in global memory only for the at
// most two groups that cross the chunk's edges.  A maximum does not depend on the order its operands arrive in: the result is the same
// on every run.  The unpack pass turns the keys into the scores[] / ords[] arrays of the live groups, ascending by ord, which
// bbq_span_select_kernel<true> (bbq_span_kernels.hip) takes as they are.
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_launch.h"
#include "bbq_rowlist.h"
#include "bbq_scan_body.h"

#pragma clang fp contract(off)

namespace bbq {

namespace {

constexpr int kGroupUnpackThreads = 256;

// grid = sweep_grid_x(n_chunks, s) x sweep_grid_y(n_queries, s), decoded by sweep_coord as bbq_scan_kernel decodes it (s = a.l2_shift:
// 2^s queries of a chunk dispatched next to each other); block = kChunkRows / 64 waves: wave w takes tile w of the chunk.  QB / W / SB /
// COMPACT and the row_sums view as bbq_span_score_kernel takes them.  FILT: a.accept holds the filter's word of every tile; without one
// the accepted rows of a tile are its rows below n_rows.  A wave whose tile lies behind the last one or holds no accepted row loads
// nothing and goes straight to the barrier.
// The wave's segments are the runs of lanes between two set bits of its starts word (lane 0 opens one too).  After an inclusive
// segmented maximum over the packed keys the last lane of a segment holds the segment's; a rejected lane contributes 0, and a segment
// that is 0 has no accepted row and is dropped.  A segment whose group begins and ends inside the tile is the whole group: its key is
// stored plainly.  The others - the tile's first and last, at most - go to the wave's two LDS slots with their group; behind the
// barrier wave 0 folds the slots of equal group and stores each plainly unless the group crosses the chunk's first or last row: those
// two, at most, are raised with atomicMax, as the neighbouring chunk's workgroup raises them.
template <int QB, int W, int SB, bool COMPACT, bool FILT>
__global__ __launch_bounds__(kChunkRows) void bbq_group_score_kernel(const GroupScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = kChunkRows;
  constexpr int QU = query_units_per_chunk(QB, SB);
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  u32x4 *s_planes = reinterpret_cast<u32x4 *>(smem);
  unsigned long long *s_key = reinterpret_cast<unsigned long long *>(smem + (size_t)w16 * QU * 16);
  uint32_t *s_grp = reinterpret_cast<uint32_t *>(s_key + kGroupEdges);
  const SweepCoord wg = sweep_coord(blockIdx.x, blockIdx.y, a.l2_shift);
  if (wg.chunk_local >= a.n_chunks || wg.query >= a.n_queries) return;  // workgroup-uniform: the grid's padding
  const int q = wg.query;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  stage_query_planes<NT>(s_planes, reinterpret_cast<const u32x4 *>(a.qplanes) + (size_t)q * w16 * QU, w16 * QU, tid);
  if (tid < kGroupEdges) s_key[tid] = 0ull;
  const QueryParams p = a.qparams[q];
  __syncthreads();

  const int64_t n_tiles = (a.idx.n_rows + kTileRows - 1) / kTileRows;
  const int64_t first_tile = (int64_t)wg.chunk_local * kTilesPerChunk;
  const int64_t tile = first_tile + __builtin_amdgcn_readfirstlane(wave);
  unsigned long long *__restrict__ rep = a.rep + (size_t)q * (size_t)a.live;
  uint64_t mine = 0;  // the wave's accepted rows, bit l = lane l: wave-uniform
  if (tile < n_tiles) {
    if constexpr (FILT) {
      mine = a.accept[tile];
    } else {
      const int64_t left = a.idx.n_rows - tile * kTileRows;  // > 0
      mine = left < kTileRows ? (1ull << left) - 1ull : ~0ull;
    }
  }
  if (mine != 0) {  // wave-uniform
    const int64_t row = tile * kTileRows + lane;
    const uint8_t *__restrict__ tp = a.idx.tiles + tile * (int64_t)a.idx.geom.tile_stride;
    const bool resident = chunk_is_resident(tile / kTilesPerChunk, a.idx);
    const RowTerms rt = tile_row_terms<QB, W, SB, COMPACT>(a.idx, tp, row, lane, w16, resident, s_planes);

    const float s32 = (float)score_f64((double)rt.qc, rt.lu.x, rt.lu.y, rt.xadd, rt.x1, p);
    unsigned long long key = ((mine >> lane) & 1ull) ? group_key(__float_as_uint(s32), s32 != s32, (uint32_t)row) : 0ull;

    const uint64_t st = a.starts[tile];  // wave-uniform
    const uint64_t heads = st | 1ull;
    const int head = segment_head(heads, lane);
    key = segment_max(key, head, lane);
    const bool is_end = lane == kTileRows - 1 || ((heads >> (lane + 1)) & 1ull);
    if (is_end && key != 0ull) {
      const uint32_t grp = a.first_group[tile] + (uint32_t)__popcll((st >> 1) & ((1ull << lane) - 1ull));
      const bool begins_here = (st >> head) & 1ull;
      const bool ends_here = lane < kTileRows - 1 || (a.starts[tile + 1] & 1ull);
      if (begins_here && ends_here) {
        rep[a.slot[grp]] = key;  // the whole group: no other lane of the launch writes its slot for this query
      } else {
        const int e = 2 * wave + (head == 0 ? 0 : 1);  // the tile's first segment, or its last
        s_key[e] = key;
        s_grp[e] = grp;
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;

  const unsigned long long mk = lane < kGroupEdges ? s_key[lane] : 0ull;
  const uint32_t mg = lane < kGroupEdges ? s_grp[lane] : 0u;
  fold_group_edges(a, mk, mg, rep, first_tile, n_tiles, lane);
}

__global__ __launch_bounds__(kGroupUnpackThreads) void bbq_group_unpack_kernel(const unsigned long long *__restrict__ rep, float *__restrict__ scores,
                                                                               uint32_t *__restrict__ ords, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kGroupUnpackThreads + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = rep[i];
  scores[i] = __uint_as_float(group_key_score_bits(k));
  ords[i] = group_key_ord(k);
}

template <int QB, int W, int SB>
hipError_t launch_group_score_t(const GroupScoreArgs &args, hipStream_t s) {
  GroupScoreArgs a = args;  // the map's parameter: what the kernel decodes its block index with is what the grid is built from
  a.l2_shift = sweep_shift_for(args.l2_shift, a.n_queries, a.n_chunks);
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  const size_t smem = (size_t)w16 * query_units_per_chunk(QB, SB) * 16 + (size_t)kGroupEdges * (8 + 4);
  dim3 grid(sweep_grid_x(a.n_chunks, a.l2_shift), sweep_grid_y(a.n_queries, a.l2_shift), 1), block(kChunkRows, 1, 1);
  const bool compact = a.idx.geom.layout == kLayoutCompact;
  if (a.accept) {
    if (compact) hipLaunchKernelGGL((bbq_group_score_kernel<QB, W, SB, true, true>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_group_score_kernel<QB, W, SB, false, true>), grid, block, smem, s, a);
  } else {
    if (compact) hipLaunchKernelGGL((bbq_group_score_kernel<QB, W, SB, true, false>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_group_score_kernel<QB, W, SB, false, false>), grid, block, smem, s, a);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_group_score(const GroupScoreArgs &a, int planes, hipStream_t s) {
  if (a.n_chunks <= 0 || a.n_queries <= 0 || a.live <= 0) return hipSuccess;
  if (a.n_queries > 65535 || a.idx.n_rows > kGroupMaxRows || !a.starts || !a.first_group || !a.slot || !a.rep) return hipErrorInvalidValue;
  if ((int64_t)a.n_chunks != (a.idx.n_rows + kChunkRows - 1) / kChunkRows) return hipErrorInvalidValue;  // the tables are those of the whole index
  return rowlist_ladder(a.idx.geom, planes, [&](auto qb, auto w, auto sb) { return launch_group_score_t<qb(), w(), sb()>(a, s); });
}

hipError_t launch_group_unpack(const unsigned long long *rep, float *scores, uint32_t *ords, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + kGroupUnpackThreads - 1) / kGroupUnpackThreads;
  if (blocks > 0x7fffffffll || (uint64_t)blocks * kGroupUnpackThreads > kGridWorkItemsMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bbq_group_unpack_kernel, dim3((unsigned)blocks, 1, 1), dim3(kGroupUnpackThreads, 1, 1), 0, s, rep, scores, ords, n);
  return hipGetLastError();
}

}  // namespace bbq
