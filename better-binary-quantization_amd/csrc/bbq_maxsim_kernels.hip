// bbq_maxsim_kernels.hip - MaxSim search (gfx950): bbq_search_maxsim_batch.
//
// A query is a run of token vectors; a live group of rows scores S = (float)((double)m_0 + (double)m_1 + ...), m_t the f32 score of
// token t's representative of the group (the grouped search's, bbq_group_kernels.hip), the f64 adds strictly in ascending t.  Two
// passes of this file stand between a token block's keys and the span search's select pass.
// The FUSED score pass is the grouped search's score pass with one difference: a workgroup is one chunk for ALL tokens of one query's
// token block.  A wave loads its tile once - codes and corrections stay in registers - and what belongs to the tile (addresses, the
// accept word, the starts word, the segments' group numbers and slots) is computed once; per token it pays the popcounts, the score,
// the packed key, the six-step segmented maximum and the stores.  Every other shape takes the grouped search's own kernel with the
// block's token vectors as its queries (bbq_maxsim.cpp): the keys land in the same rep[token][slot] either way.
// The ACCUMULATE pass adds a block's keys, unpacked, into an f64 per (query, slot) that lives across the blocks of a query.
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_launch.h"
#include "bbq_rowlist.h"
#include "bbq_scan_body.h"

#pragma clang fp contract(off)

namespace bbq {

namespace {

constexpr int kMaxSimAccThreads = 256;

// LDS of a fused workgroup: [TB][W * QU] planes | [TB] QueryParams | [TB][kGroupEdges] keys | [kGroupEdges] groups
constexpr size_t maxsim_lds_bytes(int w16, int qu) {
  return (size_t)kMaxSimTokenBlock * ((size_t)w16 * qu * 16 + sizeof(QueryParams) + (size_t)kGroupEdges * 8) + (size_t)kGroupEdges * 4;
}
static_assert(maxsim_lds_bytes(12, 4) <= 40 * 1024, "four workgroups per CU (kMaxSimTokenBlock, bbq_device.h)");

// grid and block as bbq_group_score_kernel's, the grid's query axis over a.queries: workgroup = (chunk, query, the launch's token block).
// The segments, the plain store of a whole group, the two LDS slots per wave and the fold behind the barrier are the group kernel's, per
// token: token t's keys go to rep[vec_first + t][slot], its edge segments to s_key[t][..]; the groups of the edge slots do not depend
// on the token.  Behind the barrier wave w folds the tokens w, w + 8, ...
template <int QB, int W, bool COMPACT, bool FILT>
__global__ __launch_bounds__(kChunkRows) void bbq_maxsim_score_kernel(const MaxSimScoreArgs ma) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = kChunkRows;
  constexpr int QU = query_units_per_chunk(QB, 1);
  constexpr int PU = W * QU;  // 16-byte units of a token's planes
  const GroupScoreArgs &a = ma.g;
  u32x4 *s_planes = reinterpret_cast<u32x4 *>(smem);
  QueryParams *s_params = reinterpret_cast<QueryParams *>(smem + (size_t)kMaxSimTokenBlock * PU * 16);
  unsigned long long *s_key = reinterpret_cast<unsigned long long *>(s_params + kMaxSimTokenBlock);
  uint32_t *s_grp = reinterpret_cast<uint32_t *>(s_key + kMaxSimTokenBlock * kGroupEdges);
  const SweepCoord wg = sweep_coord(blockIdx.x, blockIdx.y, a.l2_shift);
  if (wg.chunk_local >= a.n_chunks || wg.query >= a.n_queries) return;  // workgroup-uniform: the grid's padding
  const MaxSimQuery mq = ma.queries[wg.query];
  const int n_tok = mq.n_tok < kMaxSimTokenBlock ? mq.n_tok : kMaxSimTokenBlock;  // the LDS holds no more
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  stage_token_block<NT>(s_planes, s_params, reinterpret_cast<const u32x4 *>(a.qplanes) + (size_t)mq.vec_first * PU, a.qparams + mq.vec_first,
                        n_tok, PU, tid);  // the block's
  for (int i = tid; i < n_tok * kGroupEdges; i += NT) s_key[i] = 0ull;
  __syncthreads();

  const int64_t n_tiles = (a.idx.n_rows + kTileRows - 1) / kTileRows;
  const int64_t first_tile = (int64_t)wg.chunk_local * kTilesPerChunk;
  const int64_t tile = first_tile + __builtin_amdgcn_readfirstlane(wave);
  unsigned long long *__restrict__ rep = a.rep + (size_t)mq.vec_first * (size_t)a.live;  // token 0 of the block; token t: + t * live
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
    const bool rs = COMPACT && a.idx.row_sums != nullptr;  // uniform over the launch

    // the tile, once: codes and corrections stay in registers over the tokens
    f64x2 lu = {0.0, 0.0};
    double xadd = 0.0, x1 = 0.0;
    uint32_t cw = 0;
    uint32_t ones = 0;
    constexpr int CORR = COMPACT ? 0 : 2;
    u32x4 c[W];
    if (rs) {
      load_tile<W, CORR, true>(tp, lane, false, resident, a.idx.nt_delta, c, cw, lu, xadd, x1, a.idx.row_sums + row, &ones);
    } else {
      load_tile<W, CORR>(tp, lane, a.idx.geom.has_x1 != 0, resident, a.idx.nt_delta, c, cw, lu, xadd, x1);
    }
    if constexpr (COMPACT) exact_corrections<true>(a.idx.exact, row, lu, xadd);
    if (!rs) ones = row_popcount(c, ones);
    if (COMPACT || !a.idx.geom.has_x1) x1 = (double)ones;  // quantizedComponentSum of a freshly quantized row is its popcount

    // the lane's segment, once: its first lane, whether it ends here, where its key goes
    const bool accepted = (mine >> lane) & 1ull;
    const uint64_t st = a.starts[tile];  // wave-uniform
    const uint64_t heads = st | 1ull;
    const int head = segment_head(heads, lane);
    const bool is_end = lane == kTileRows - 1 || ((heads >> (lane + 1)) & 1ull);
    bool whole = false;
    int32_t slot = -1;
    int e = 0;
    if (is_end) {
      const uint32_t grp = a.first_group[tile] + (uint32_t)__popcll((st >> 1) & ((1ull << lane) - 1ull));
      const bool begins_here = (st >> head) & 1ull;
      const bool ends_here = lane < kTileRows - 1 || (a.starts[tile + 1] & 1ull);
      whole = begins_here && ends_here;
      e = 2 * wave + (head == 0 ? 0 : 1);  // the tile's first segment, or its last
      if (whole) slot = a.slot[grp];       // -1 for a group without an accepted row, whose key stays 0: never used
      else s_grp[e] = grp;                 // read only where a key of the slot is not 0
    }

    for (int t = 0; t < n_tok; ++t) {
      const QueryParams p = token_params(s_params, t);
      uint32_t unused = 0;
      const uint32_t qc = tile_popcounts<QB, W, false>(c, s_planes + t * PU, unused);
      const float s32 = (float)score_f64((double)qc, lu.x, lu.y, xadd, x1, p);
      const unsigned long long key = segment_max(accepted ? group_key(__float_as_uint(s32), s32 != s32, (uint32_t)row) : 0ull, head, lane);
      if (is_end && key != 0ull) {
        if (whole) rep[(size_t)t * (size_t)a.live + slot] = key;  // the whole group: no other lane of the launch writes its slot for this token
        else s_key[t * kGroupEdges + e] = key;
      }
    }
  }
  __syncthreads();

  // per token the edge segments of the workgroup, in row order: those of one group folded into the first of them
  const uint32_t mg = lane < kGroupEdges ? s_grp[lane] : 0u;
  for (int t = wave; t < n_tok; t += kTilesPerChunk) {
    const unsigned long long mk = lane < kGroupEdges ? s_key[t * kGroupEdges + lane] : 0ull;
    fold_group_edges(a, mk, mg, rep + (size_t)t * (size_t)a.live, first_tile, n_tiles, lane);
  }
}

// grid = (ceil(live / kMaxSimAccThreads), the block's queries); a thread is one (query, slot).  The adds run in ascending token, in f64,
// from the first token's score - not from 0.0: a single -0.0 stays -0.0 - and a NaN score (a key whose score half is 0) makes the sum NaN
__global__ __launch_bounds__(kMaxSimAccThreads) void bbq_maxsim_accumulate_kernel(const MaxSimAccArgs a) {
  const int64_t slot = (int64_t)blockIdx.x * kMaxSimAccThreads + threadIdx.x;
  if (slot >= a.live) return;
  const MaxSimQuery mq = a.queries[blockIdx.y];
  const unsigned long long *__restrict__ k = a.rep + (size_t)mq.vec_first * (size_t)a.live + slot;
  const size_t at = (size_t)mq.query * (size_t)a.live + slot;
  int t = 0;
  double acc;
  if (mq.flags & kMaxSimFirst) {
    acc = (double)__uint_as_float(group_key_score_bits(k[0]));
    t = 1;
  } else {
    acc = a.acc[at];
  }
  for (; t < mq.n_tok; ++t) acc = acc + (double)__uint_as_float(group_key_score_bits(k[(size_t)t * (size_t)a.live]));
  if (mq.flags & kMaxSimLast) {
    a.scores[at] = (float)acc;
    if (a.live_group) a.ords[at] = (uint32_t)a.live_group[slot];  // null: the caller's entries are not slots of the group set
  } else {
    a.acc[at] = acc;
  }
}

template <int W>
hipError_t launch_maxsim_score_t(const MaxSimScoreArgs &args, hipStream_t s) {
  constexpr int QB = 4;
  MaxSimScoreArgs a = args;  // the map's parameter: what the kernel decodes its block index with is what the grid is built from
  a.g.l2_shift = sweep_shift_for(args.g.l2_shift, a.g.n_queries, a.g.n_chunks);
  const size_t smem = maxsim_lds_bytes(W, query_units_per_chunk(QB, 1));
  dim3 grid(sweep_grid_x(a.g.n_chunks, a.g.l2_shift), sweep_grid_y(a.g.n_queries, a.g.l2_shift), 1), block(kChunkRows, 1, 1);
  const bool compact = a.g.idx.geom.layout == kLayoutCompact;
  if (a.g.accept) {
    if (compact) hipLaunchKernelGGL((bbq_maxsim_score_kernel<QB, W, true, true>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_maxsim_score_kernel<QB, W, false, true>), grid, block, smem, s, a);
  } else {
    if (compact) hipLaunchKernelGGL((bbq_maxsim_score_kernel<QB, W, true, false>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_maxsim_score_kernel<QB, W, false, false>), grid, block, smem, s, a);
  }
  return hipGetLastError();
}

}  // namespace

bool maxsim_fused_exists(const TileGeom &geom, int planes) {
  return geom.store_bits == 1 && planes == 4 && (geom.w16 == 6 || geom.w16 == 8 || geom.w16 == 12);
}

hipError_t launch_maxsim_score(const MaxSimScoreArgs &a, int planes, hipStream_t s) {
  const GroupScoreArgs &g = a.g;
  if (g.n_chunks <= 0 || g.n_queries <= 0 || g.live <= 0) return hipSuccess;
  if (!maxsim_fused_exists(g.idx.geom, planes) || !a.queries) return hipErrorInvalidValue;
  if (g.n_queries > 65535 || g.idx.n_rows > kGroupMaxRows || !g.starts || !g.first_group || !g.slot || !g.rep) return hipErrorInvalidValue;
  if ((int64_t)g.n_chunks != (g.idx.n_rows + kChunkRows - 1) / kChunkRows) return hipErrorInvalidValue;  // the tables are those of the whole index
  switch (g.idx.geom.w16) {
    case 6: return launch_maxsim_score_t<6>(a, s);    // dim 641..768
    case 8: return launch_maxsim_score_t<8>(a, s);    // dim 897..1024
    default: return launch_maxsim_score_t<12>(a, s);  // dim 1409..1536
  }
}

hipError_t launch_maxsim_accumulate(const MaxSimAccArgs &a, int n_queries, hipStream_t s) {
  if (n_queries <= 0 || a.live <= 0) return hipSuccess;
  const int64_t blocks = (a.live + kMaxSimAccThreads - 1) / kMaxSimAccThreads;
  if (n_queries > 65535 || blocks > 0x7fffffffll || (uint64_t)blocks * kMaxSimAccThreads > kGridWorkItemsMax) return hipErrorInvalidValue;
  if (!a.rep || !a.queries || !a.acc || !a.scores || (a.live_group && !a.ords)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bbq_maxsim_accumulate_kernel, dim3((unsigned)blocks, n_queries, 1), dim3(kMaxSimAccThreads, 1, 1), 0, s, a);
  return hipGetLastError();
}

}  // namespace bbq
