// bbq_maxsim_mfma_kernels.hip - the MaxSim search's score pass on the matrix cores (gfx950; maxsim_fused 2).
//
// The fused score pass (bbq_maxsim_score_kernel, bbq_maxsim_kernels.hip) loads a tile once for a block of up to 32 tokens and pays, per
// token and row, the four bit-plane popcounts in front of the score.  A token block is exactly one query group of the matrix-core shared
// sweep (kMaxSimTokenBlock == kMfmaQueries): here the block's token vectors are the FP6 A operands of v_mfma_scale_f32_32x32x64_f8f6f4
// and the tile's 1-bit codes its FP4 B operands where they stand (fp_step, bbq_mfma_common.h, whose layout and derivations this file
// relies on).  MaxSim prunes nothing, so nothing of the sweep's threshold half is here: the accumulator starts at 0 and ends at
// S * qcDist with S = 1/4 - a multiple of 1/4 below 2^20, exact in f32 - for all 32 x 64 (token, row) pairs of the tile after 2 W
// steps.  What stays per pair is the f64 score in the reference's operation order, the packed key and the group maximum, and those run
// as in the fused kernel: the keys land in the same rep[token][slot] and the same edge slots, and the accumulate and select passes take
// them untouched.
//
// What is this kernel's own is the shape the maximum is taken in.  Behind the contraction a lane (h = lane >> 5, n = lane & 31) holds
// tile row n in acc0 and tile row 32 + n in acc1, each against the 16 tokens m = (r & 3) + 8 (r >> 2) + 4 h of accumulator entry r: the
// 64 rows of a token lie across the 32 lanes of ONE half-wave in TWO registers, and the two half-waves work on different tokens at the
// same time.  The segmented maximum is five steps inside a half-wave per register and then the seam between row 31 and row 32.
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_launch.h"
#include "bbq_rowlist.h"

#pragma clang fp contract(off)

#include "bbq_mfma_common.h"

namespace bbq {

namespace {

static_assert(kMaxSimTokenBlock == kMfmaQueries, "a token block is one query group of the matrix cores");

// LDS of a workgroup: the block's operand bytes | [TB] QueryParams | [TB][kGroupEdges] keys | [kGroupEdges] groups
constexpr size_t maxsim_mfma_lds_bytes(int w16) {
  return (size_t)mfma_query_bytes(w16, true) + (size_t)kMaxSimTokenBlock * (sizeof(QueryParams) + (size_t)kGroupEdges * 8) + (size_t)kGroupEdges * 4;
}
static_assert(maxsim_mfma_lds_bytes(12) <= 64 * 1024, "no opt-in to large dynamic LDS; two workgroups per CU at the widest row");

// both halves of a lane's value: [0] = the value of tile row n = lane & 31, [1] = that of row 32 + n, in both half-waves
struct RowPair { uint32_t v[2]; };
__device__ __forceinline__ RowPair both_rows(uint32_t mine) {
  const auto s = __builtin_amdgcn_permlane32_swap(mine, mine, false, false);
  return RowPair{{s[0], s[1]}};
}
__device__ __forceinline__ void both_rows(double mine, double (&out)[2]) {
  const RowPair lo = both_rows((uint32_t)__double2loint(mine)), hi = both_rows((uint32_t)__double2hiint(mine));
  out[0] = __hiloint2double((int)hi.v[0], (int)lo.v[0]);
  out[1] = __hiloint2double((int)hi.v[1], (int)lo.v[1]);
}

// what does not depend on the token, of one of the lane's two rows (tile row R = 32 rg + n)
struct RowSeg {
  bool accepted, is_end, whole, open;  // open: no segment begins in rows 32 .. R (rg = 1 alone) - the row continues row 31's segment
  int head;                            // the first lane, in the half-wave, of the row's segment inside its register
  int32_t slot;
  int e;
};

// the inclusive segmented maximum over the 32 lanes of a half-wave (the two half-waves at once, each on its own token)
__device__ __forceinline__ unsigned long long half_segment_max(unsigned long long key, int head, int n) {
#pragma unroll
  for (int d = 1; d < 32; d <<= 1) {
    const unsigned long long o = __shfl_up(key, (unsigned)d, 32);
    if (n - d >= head && o > key) key = o;
  }
  return key;
}

// Grid and workgroup are bbq_maxsim_score_kernel's: workgroup = (chunk, query, the launch's token block), eight waves, a wave = one tile.
// A wave whose accept word is 0, or that lies beyond the last tile, loads and multiplies nothing.  A tile with only one accepted half
// still runs both halves: the two MFMAs of a step share the A operand and the reads that feed it, and the branch would have to be
// taken per step.
template <int W, bool COMPACT, bool FILT>
__global__ __launch_bounds__(kChunkRows) void bbq_maxsim_mfma_kernel(const MaxSimScoreArgs ma) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = kChunkRows;
  constexpr int STEPS = 2 * W;
  constexpr int QBYTES = mfma_query_bytes(W, true);
  const GroupScoreArgs &a = ma.g;
  QueryParams *s_params = reinterpret_cast<QueryParams *>(smem + QBYTES);
  unsigned long long *s_key = reinterpret_cast<unsigned long long *>(s_params + kMaxSimTokenBlock);
  uint32_t *s_grp = reinterpret_cast<uint32_t *>(s_key + kMaxSimTokenBlock * kGroupEdges);
  const SweepCoord wg = sweep_coord(blockIdx.x, blockIdx.y, a.l2_shift);
  if (wg.chunk_local >= a.n_chunks || wg.query >= a.n_queries) return;  // workgroup-uniform: the grid's padding
  const MaxSimQuery mq = ma.queries[wg.query];
  const int n_tok = mq.n_tok < kMaxSimTokenBlock ? mq.n_tok : kMaxSimTokenBlock;  // the LDS holds no more
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int n = lane & 31, h = lane >> 5;
  {  // the block's operands (a missing token's bytes are zero: the host's), its tokens' uniforms, no edge key yet
    const u32x4 *__restrict__ gb = reinterpret_cast<const u32x4 *>(ma.qops + (size_t)wg.query * QBYTES);
    u32x4 *__restrict__ sb = reinterpret_cast<u32x4 *>(smem);
    for (int i = tid; i < QBYTES / 16; i += NT) sb[i] = gb[i];
    const u32x4 *__restrict__ gq = reinterpret_cast<const u32x4 *>(a.qparams + mq.vec_first);
    u32x4 *__restrict__ sq = reinterpret_cast<u32x4 *>(s_params);
    for (int i = tid; i < n_tok * kParamUnits; i += NT) sq[i] = gq[i];
    for (int i = tid; i < n_tok * kGroupEdges; i += NT) s_key[i] = 0ull;
  }
  __syncthreads();

  const int64_t n_tiles = (a.idx.n_rows + kTileRows - 1) / kTileRows;
  const int64_t first_tile = (int64_t)wg.chunk_local * kTilesPerChunk;
  const int64_t tile = first_tile + __builtin_amdgcn_readfirstlane(wave);
  unsigned long long *__restrict__ rep = a.rep + (size_t)mq.vec_first * (size_t)a.live;  // token 0 of the block; token t: + t * live
  uint64_t mine = 0;  // the wave's accepted rows, bit l = tile row l: wave-uniform
  if (tile < n_tiles) {
    if constexpr (FILT) {
      mine = a.accept[tile];
    } else {
      const int64_t left = a.idx.n_rows - tile * kTileRows;  // > 0
      mine = left < kTileRows ? (1ull << left) - 1ull : ~0ull;
    }
  }
  if (mine != 0) {  // wave-uniform
    // the tile, once: lane l loads row l, as the matrix-core sweeps load it (load_tile_regs).  A choice, and not the fused kernel's: every
    // load is non-temporal from the index's one mapping - the fused kernel reads a resident chunk under the default cache policy and a
    // streamed one through nt_delta (chunk_is_resident, load_tile) - and a compact row's corrections come from the side array by the two
    // streamed loads exact_corrections<true> makes, issued with the codes and not behind them.  The bytes are the same; against a
    // partly resident index the cache policy is the sweep's, not the fused kernel's
    TileRegs<W, COMPACT> t;
    load_tile_regs<W, COMPACT>(t, a.idx, tile, lane);
    const bool rs = COMPACT && a.idx.row_sums != nullptr;  // uniform over the launch
    uint32_t ones = 0;
    if (rs) ones = __builtin_nontemporal_load(a.idx.row_sums + tile * kTileRows + lane);
    else ones = row_popcount(t.c, 0u);  // in front of swap_code_words: of the lane's own row
    if (COMPACT || !a.idx.geom.has_x1) t.x1 = (double)ones;  // quantizedComponentSum of a freshly quantized row is its popcount

    // ---- the contraction: C[m = token][row of the half] over 2 W steps of 64 dimensions, from 0
    swap_code_words<W>(t.c);
    // The zeros are held in registers, opaque to the compiler.  Started from the inline constant 0, step 0's MFMAs are the untied form
    // and its destination was allocated over its own A and B sources (v[2:17] <- v[4:9] x v[14:17]): a 16-pass MFMA still reads its
    // sources while it writes, and the widest compact form then gave a few groups per hundred calls a second-best row.  With C in
    // registers every step is the tied form (destination = C), which no source can share
    f32x16m acc0 = {0}, acc1 = {0};
    asm volatile("" : "+v"(acc0), "+v"(acc1));
    {
      // the priming read of fp_step<0>, as the sweeps carry it.  Their opaque LDS offset and the empty asms that pin the code words in
      // front of it keep the read inside their loops over chunks and query groups; here a wave has one tile and one group, and the read
      // stands behind the barrier with nothing to be hoisted over
      const u32x4 *__restrict__ s_B = reinterpret_cast<const u32x4 *>(smem);
      const u32x2 *__restrict__ s_B2 = reinterpret_cast<const u32x2 *>(smem + (size_t)STEPS * 2 * 32 * 16);
      const uint32_t addr16 = (uint32_t)(uintptr_t)(s_B + h * 32 + n), addr8 = (uint32_t)(uintptr_t)(s_B2 + h * 32 + n);
      u32x4 bq;
      u32x2 bq2;
      asm volatile("ds_read_b128 %0, %2\n\tds_read_b64 %1, %3" : "=v"(bq), "=v"(bq2) : "v"(addr16), "v"(addr8));
      fp_step<0, STEPS, W>(acc0, acc1, t.c, bq, bq2, addr16, addr8);
    }

    // ---- the constants of the lane's two rows: once per tile, across the half-waves
    double lo[2], up[2], xadd[2], x1[2];
    both_rows(t.lu.x, lo);
    both_rows(t.lu.y, up);
    both_rows(t.add, xadd);
    both_rows(t.x1, x1);

    // ---- the two rows' segments, once: where each begins inside its register, whether it ends at the row, where its key goes
    const uint64_t st = a.starts[tile];  // wave-uniform
    const uint64_t heads = st | 1ull;
    RowSeg sg[2];
#pragma unroll
    for (int rg = 0; rg < 2; ++rg) {
      const int R = 32 * rg + n;
      RowSeg &s = sg[rg];
      s.accepted = (mine >> R) & 1ull;
      const int head = segment_head(heads, R);  // in the tile
      s.open = rg == 1 && head < 32;
      s.head = s.open ? 0 : head - 32 * rg;
      s.is_end = R == kTileRows - 1 || ((heads >> (R + 1)) & 1ull);
      s.whole = false;
      s.slot = -1;
      s.e = 0;
      if (s.is_end) {
        const uint32_t grp = a.first_group[tile] + (uint32_t)__popcll((st >> 1) & ((1ull << R) - 1ull));
        const bool begins_here = (st >> head) & 1ull;
        const bool ends_here = R < kTileRows - 1 || (a.starts[tile + 1] & 1ull);
        s.whole = begins_here && ends_here;
        s.e = 2 * wave + (head == 0 ? 0 : 1);  // the tile's first segment, or its last
        if (s.whole) s.slot = a.slot[grp];     // -1 for a group without an accepted row, whose key stays 0: never used
        else s_grp[s.e] = grp;                 // (both half-waves write the same value) read only where a key of the slot is not 0
      }
    }
    const uint32_t row0 = (uint32_t)(tile * kTileRows) + (uint32_t)n;

    // ---- per accumulator entry: the half-wave's token against the lane's two rows
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mb = (r & 3) + 8 * (r >> 2);  // the lower half-wave's token; the upper's is mb + 4
      if (mb >= n_tok) continue;              // wave-uniform: neither half has a token
      const int m = mb + 4 * h;
      const bool has_tok = m < n_tok;         // (a half-wave without a token reads uniforms nobody staged and stores nothing)
      const QueryParams p = token_params(s_params, m);
      const uint32_t qc0 = (uint32_t)(acc0[r] * 4.0f), qc1 = (uint32_t)(acc1[r] * 4.0f);  // exact: multiples of 1/4 below 2^20
      const float s0 = (float)score_f64((double)qc0, lo[0], up[0], xadd[0], x1[0], p);
      const float s1 = (float)score_f64((double)qc1, lo[1], up[1], xadd[1], x1[1], p);
      unsigned long long k0 = has_tok && sg[0].accepted ? group_key(__float_as_uint(s0), s0 != s0, row0) : 0ull;
      unsigned long long k1 = has_tok && sg[1].accepted ? group_key(__float_as_uint(s1), s1 != s1, row0 + 32u) : 0ull;
      k0 = half_segment_max(k0, sg[0].head, n);
      k1 = half_segment_max(k1, sg[1].head, n);
      // the seam: row 31's value is the maximum of its segment's rows of the lower register; the rows of the upper register in front of
      // which no segment begins continue that segment
      const unsigned long long seam = __shfl(k0, 31, 32);
      if (sg[1].open && seam > k1) k1 = seam;
#pragma unroll
      for (int rg = 0; rg < 2; ++rg) {
        const unsigned long long key = rg == 0 ? k0 : k1;
        if (sg[rg].is_end && key != 0ull) {
          if (sg[rg].whole) rep[(size_t)m * (size_t)a.live + sg[rg].slot] = key;  // the whole group: no other lane of the launch writes its slot for this token
          else s_key[m * kGroupEdges + sg[rg].e] = key;
        }
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

template <int W>
hipError_t launch_maxsim_mfma_t(const MaxSimScoreArgs &args, hipStream_t s) {
  MaxSimScoreArgs a = args;  // the map's parameter: what the kernel decodes its block index with is what the grid is built from
  a.g.l2_shift = sweep_shift_for(args.g.l2_shift, a.g.n_queries, a.g.n_chunks);
  const size_t smem = maxsim_mfma_lds_bytes(W);
  dim3 grid(sweep_grid_x(a.g.n_chunks, a.g.l2_shift), sweep_grid_y(a.g.n_queries, a.g.l2_shift), 1), block(kChunkRows, 1, 1);
  const bool compact = a.g.idx.geom.layout == kLayoutCompact;
  if (a.g.accept) {
    if (compact) hipLaunchKernelGGL((bbq_maxsim_mfma_kernel<W, true, true>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_maxsim_mfma_kernel<W, false, true>), grid, block, smem, s, a);
  } else {
    if (compact) hipLaunchKernelGGL((bbq_maxsim_mfma_kernel<W, true, false>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_maxsim_mfma_kernel<W, false, false>), grid, block, smem, s, a);
  }
  return hipGetLastError();
}

}  // namespace

// 4 planes: every token's quantized value is at most 15 (planes_of_call) - what FP6 at S = 1/4 holds exactly
bool maxsim_mfma_exists(const TileGeom &geom, int planes) { return maxsim_fused_exists(geom, planes); }

hipError_t launch_maxsim_mfma(const MaxSimScoreArgs &a, int planes, hipStream_t s) {
  const GroupScoreArgs &g = a.g;
  if (g.n_chunks <= 0 || g.n_queries <= 0 || g.live <= 0) return hipSuccess;
  if (!maxsim_mfma_exists(g.idx.geom, planes) || !a.queries || !a.qops) return hipErrorInvalidValue;
  if (g.n_queries > 65535 || g.idx.n_rows > kGroupMaxRows || !g.starts || !g.first_group || !g.slot || !g.rep) return hipErrorInvalidValue;
  if ((int64_t)g.n_chunks != (g.idx.n_rows + kChunkRows - 1) / kChunkRows) return hipErrorInvalidValue;  // the tables are those of the whole index
  switch (g.idx.geom.w16) {
    case 6: return launch_maxsim_mfma_t<6>(a, s);    // dim 641..768
    case 8: return launch_maxsim_mfma_t<8>(a, s);    // dim 897..1024
    default: return launch_maxsim_mfma_t<12>(a, s);  // dim 1409..1536
  }
}

}  // namespace bbq
