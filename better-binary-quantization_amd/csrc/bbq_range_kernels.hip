// bbq_range_kernels.hip - range search (gfx950): bbq_count_range_batch, bbq_search_range_batch.
//
// Every row whose f32 score is >= the caller's threshold, ascending by row.  The threshold comes from the host as a key (bbq_range_key:
// key(score) > key  <=>  score >= threshold) and the answer has no fixed size, so the sweep is count-then-fill: one pass counts the passing
// rows of every chunk, one workgroup per query scans the counts into offsets and lists the chunks that hold a row, and a second pass over
// those chunks alone writes each passing row where the offsets put it.  Both passes are the same kernel and score a row with the sweep's
// own functions (bbq_kernel_common.h, bbq_scan_body.h), so they pass the same rows and every score is bit for bit what the dense sweep
// writes.  No global atomics, no candidate slots, no overflow tier: the output is deterministic.
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_launch.h"
#include "bbq_rowlist.h"
#include "bbq_scan_body.h"

#pragma clang fp contract(off)

namespace bbq {

namespace {

// one thread per query: the key and its z image through the one writer of a threshold
__global__ void bbq_range_theta_kernel(Threshold *__restrict__ theta, const uint32_t *__restrict__ keys, const QueryParams *__restrict__ qparams, int n_queries) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n_queries) store_threshold(theta + q, keys[q], qparams[q]);
}

// one workgroup per query: counts[q][*] -> its exclusive prefix (in place), totals[q], and the ascending list of the chunks whose count
// is not zero with its length
__global__ __launch_bounds__(kRangeOffsetsThreads) void bbq_range_offsets_kernel(uint32_t *__restrict__ counts, uint32_t *__restrict__ nonempty,
                                                                                 uint32_t *__restrict__ totals, uint32_t *__restrict__ n_nonempty, int n_chunks) {
  __shared__ uint32_t s_wave[16];
  const int q = blockIdx.x;
  uint32_t *__restrict__ c = counts + (size_t)q * n_chunks;
  uint32_t *__restrict__ ne = nonempty + (size_t)q * n_chunks;
  uint32_t rows = 0, listed = 0;  // of the chunks in front of this round's: workgroup-uniform
  for (int i0 = 0; i0 < n_chunks; i0 += kRangeOffsetsThreads) {
    const int i = i0 + (int)threadIdx.x;
    const uint32_t v = i < n_chunks ? c[i] : 0u;
    uint32_t round_rows, round_listed;
    const uint32_t at = block_exclusive_scan_1024(v, s_wave, round_rows);
    const uint32_t slot = block_exclusive_scan_1024(v != 0u ? 1u : 0u, s_wave, round_listed);
    if (i < n_chunks) c[i] = rows + at;
    if (v != 0u) ne[listed + slot] = (uint32_t)i;
    rows += round_rows;
    listed += round_listed;
  }
  if (threadIdx.x == 0) {
    totals[q] = rows;
    n_nonempty[q] = listed;
  }
}

// grid = (chunks of kChunkRows rows, queries) for the count pass (FILL false), (longest list of non-empty chunks among the launch's
// queries, queries) for the fill pass; block = kChunkRows / 64 waves: wave w handles tile w of its chunk, one row per lane.  QB / W / SB
// as bbq_scan_kernel takes them; COMPACT: the corrections layout of the index - its score bound stands in front of the exact gather, an
// inline index scores every row.  The accept bitset is a run-time pointer (null: every row): a wave reads its tile's word through a
// wave-uniform address and a wave whose word is 0 loads nothing.  The row's component sum comes from the row_sums side array where the
// launch's view carries it and is counted otherwise - the same value either way.
template <int QB, int W, int SB, bool COMPACT, bool FILL>
__global__ __launch_bounds__(kChunkRows) void bbq_range_kernel(const RangeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = kChunkRows;
  constexpr int QU = query_units_per_chunk(QB, SB);
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  u32x4 *s_planes = reinterpret_cast<u32x4 *>(smem);
  uint32_t *s_wave = reinterpret_cast<uint32_t *>(smem + (size_t)w16 * QU * 16);  // FILL: [kTilesPerChunk] passing rows per wave; else word 0: of the chunk
  const int q = a.q_first + (int)blockIdx.y;
  int64_t chunk = blockIdx.x;
  if constexpr (FILL) {
    if (blockIdx.x >= a.n_nonempty[q]) return;  // workgroup-uniform: beyond this query's list, before anything is loaded
    chunk = a.nonempty[(size_t)q * a.n_chunks + blockIdx.x];
  }
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t n_tiles = (a.idx.n_rows + kTileRows - 1) / kTileRows;
  const int64_t tile = chunk * kTilesPerChunk + __builtin_amdgcn_readfirstlane(wave);

  // the tile's accept word first, as in the filtered sweep: the scalar load travels while the planes are staged
  uint64_t aw = 0;
  if (tile < n_tiles) aw = a.accept ? a.accept[tile] : ~0ull;
  stage_query_planes<NT>(s_planes, reinterpret_cast<const u32x4 *>(a.qplanes) + (size_t)q * w16 * QU, w16 * QU, tid);
  if (!FILL && tid == 0) s_wave[0] = 0;
  const QueryParams p = a.qparams[q];
  const Threshold th = a.theta[q];
  __syncthreads();

  const int64_t row = tile * kTileRows + lane;
  bool pass = false;
  float s32 = 0.0f;
  if (aw != 0) {  // wave-uniform
    const uint8_t *__restrict__ tp = a.idx.tiles + tile * (int64_t)a.idx.geom.tile_stride;
    const bool valid = row < a.idx.n_rows && ((aw >> lane) & 1ull) != 0;
    const bool resident = chunk_is_resident(chunk, a.idx);
    RowTerms rt = tile_row_terms<QB, W, SB, COMPACT, true>(a.idx, tp, row, lane, w16, resident, s_planes);

    bool need_exact = true;
    if constexpr (COMPACT) {
      const float aadd = tile_add_bound(a.idx, tile, p.sim);
      need_exact = compact_bound_passes(valid, rt.qc, rt.cw, aadd, rt.ones, rt.x1, p, th);
      if (need_exact) exact_corrections(a.idx.exact, row, rt.lu, rt.xadd);
    }
    if (need_exact) {
      s32 = (float)score_f64((double)rt.qc, rt.lu.x, rt.lu.y, rt.xadd, rt.x1, p);
      bool nan_seen = false;  // a NaN score is in no answer and raises nothing here
      pass = exact_key_passes(valid, s32, th.key, nan_seen);
    }
  }

  const unsigned long long m = __ballot(pass);
  if constexpr (!FILL) {
    if (lane == 0 && m != 0) atomicAdd(s_wave, (uint32_t)__popcll(m));
    __syncthreads();
    if (tid == 0) a.counts[(size_t)q * a.n_chunks + chunk] = s_wave[0];
  } else {
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (pass) {
      // the passing rows of the chunk below this one: the waves in front through LDS, the lanes in front through the ballot mask
      uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      for (int w = 0; w < wave; ++w) rank += s_wave[w];
      a.out[a.base[q] + a.chunk_off[(size_t)q * a.n_chunks + chunk] + rank] = candidate_entry(row, s32);
    }
  }
}

template <int QB, int W, int SB>
hipError_t launch_range_t(const RangeArgs &a, bool fill, unsigned gx, int n_queries, hipStream_t s) {
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  const size_t smem = (size_t)w16 * query_units_per_chunk(QB, SB) * 16 + kTilesPerChunk * 4;
  dim3 grid(gx, (unsigned)n_queries, 1), block(kChunkRows, 1, 1);
  const bool compact = a.idx.geom.layout == kLayoutCompact;
  if (fill) {
    if (compact) hipLaunchKernelGGL((bbq_range_kernel<QB, W, SB, true, true>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_range_kernel<QB, W, SB, false, true>), grid, block, smem, s, a);
  } else {
    if (compact) hipLaunchKernelGGL((bbq_range_kernel<QB, W, SB, true, false>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_range_kernel<QB, W, SB, false, false>), grid, block, smem, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_range(const RangeArgs &a, int planes, bool fill, int64_t gx, int n_queries, hipStream_t s) {
  if (n_queries <= 0 || gx <= 0) return hipSuccess;
  if (n_queries > 65535 || gx > a.n_chunks || (uint64_t)gx * kChunkRows > kGridWorkItemsMax) return hipErrorInvalidValue;  // grid.y, and grid.x in work-items
  return rowlist_ladder(a.idx.geom, planes,
                        [&](auto qb, auto w, auto sb) { return launch_range_t<qb(), w(), sb()>(a, fill, (unsigned)gx, n_queries, s); });
}

}  // namespace

hipError_t launch_range_theta(Threshold *theta, const uint32_t *keys, const QueryParams *qparams, int n_queries, hipStream_t s) {
  if (n_queries <= 0) return hipSuccess;
  hipLaunchKernelGGL(bbq_range_theta_kernel, dim3((unsigned)((n_queries + 255) / 256), 1, 1), dim3(256, 1, 1), 0, s, theta, keys, qparams, n_queries);
  return hipGetLastError();
}

hipError_t launch_range_count(const RangeArgs &a, int planes, int n_queries, hipStream_t s) {
  return launch_range(a, planes, false, a.n_chunks, n_queries, s);
}

hipError_t launch_range_offsets(uint32_t *counts, uint32_t *nonempty, uint32_t *totals, uint32_t *n_nonempty, int n_chunks, int n_queries, hipStream_t s) {
  if (n_queries <= 0) return hipSuccess;
  hipLaunchKernelGGL(bbq_range_offsets_kernel, dim3((unsigned)n_queries, 1, 1), dim3(kRangeOffsetsThreads, 1, 1), 0, s, counts, nonempty, totals, n_nonempty, n_chunks);
  return hipGetLastError();
}

hipError_t launch_range_fill(const RangeArgs &a, int planes, int n_queries, int64_t max_nonempty, hipStream_t s) {
  return launch_range(a, planes, true, max_nonempty, n_queries, s);
}

}  // namespace bbq
