// bbq_gather_kernels.hip - scoring chosen rows (gfx950): bbq_score_ords*, bbq_search_ords_batch.
//
// computeBatchQuantizedScores (reference src/binaryQuantizedScorer.ts:315-420) for an arbitrary list of ords per query.  One lane
// scores one list entry: ord r is lane r & 63 of tile r >> 6 (bbq_device.h), so its w16 code chunks sit 1 KiB apart inside that tile's
// record and its corrections in the record's inline block or, for the compact layout, in exact[r].  A workgroup serves kGatherThreads
// entries of ONE query and stages that query's planes in LDS once, as the sweep does; the grid is the rerank kernel's: x = pieces
// of the longest list of the launch, y = query, and a workgroup whose piece lies beyond its query's list leaves before it loads
// anything.  The row is scored by the sweep's own functions - tile_popcounts / tile_dot_multibit or their _any forms, score_f64 - so
// an entry's outputs are bit for bit what the dense sweep writes for that row.
//
// This is a gather and latency is what it costs: for the compiled row widths every load of the row - its code chunks and its
// corrections - is issued before the first is used; the other widths walk their chunks in the sweep's run-time loop.
// Cache policy: the gathered loads of the compiled widths take the DEFAULT policy.  A 16-byte chunk brings in a line that holds the
// same chunk of the neighbouring rows of its tile, and a caller's list is seldom uniform: sorted lists, duplicates, graph
// neighbourhoods and one tenant's rows name rows of the same tiles again, within one call and from one call to the next; a
// non-temporal load would give those lines up first.  Not measured (DESIGN.md "Scoring chosen rows").
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_launch.h"
#include "bbq_rowlist.h"
#include "bbq_scan_body.h"

#pragma clang fp contract(off)

namespace bbq {

namespace {

// grid = (pieces of kGatherThreads entries of the longest list, queries); SB / QB / W as bbq_scan_kernel takes them; COMPACT: the
// corrections layout of the index
template <int QB, int W, int SB, bool COMPACT>
__global__ __launch_bounds__(kGatherThreads) void bbq_score_ords_kernel(const GatherArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int QU = query_units_per_chunk(QB, SB);
  const int q = blockIdx.y;
  const int64_t beg = a.offsets[q], end = a.offsets[q + 1];
  const int64_t c0 = beg + (int64_t)blockIdx.x * kGatherThreads;
  if (c0 >= end) return;  // workgroup-uniform: this piece lies beyond the query's list
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  const int tid = threadIdx.x;
  u32x4 *s_planes = reinterpret_cast<u32x4 *>(smem);
  // the lane's entry, asked for first: the row's address hangs on it.  An idle lane of the list's last wave shadows the workgroup's
  // first entry, so every address stays in bounds
  const int64_t i = c0 + tid;
  const bool valid = i < end;
  const int64_t r = a.ords[valid ? i : c0];
  stage_query_planes<kGatherThreads>(s_planes, reinterpret_cast<const u32x4 *>(a.qplanes) + (size_t)q * w16 * QU, w16 * QU, tid);
  const QueryParams p = a.qparams[q];
  __syncthreads();
  if (c0 + (tid & ~63) >= end) return;  // wave-uniform: a whole wave beyond the list

  const uint8_t *__restrict__ tp = a.idx.tiles + (r >> 6) * (int64_t)a.idx.geom.tile_stride;
  const int lr = (int)(r & 63);
  f64x2 lu = {0.0, 0.0};
  double xadd = 0.0, x1 = 0.0;
  uint32_t qc, ones;
  u32x4 c[W > 0 ? W : 1];
  load_row<W, COMPACT>(a.idx, tp, lr, r, w16, false, c, lu, xadd, x1, ones);  // (the sum is counted: no side array here)
  if constexpr (W > 0) {
    // nothing crosses this line: left to itself the scheduler issues the later chunks behind the first popcounts, which wait for
    // the first chunk - a second round trip for the row
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SB == 1) qc = tile_popcounts<QB, W>(c, s_planes, ones);
    else tile_dot_multibit<QB, W, SB>(c, s_planes, qc, ones);
  } else {  // a row width without a compiled kernel: the sweep's chunk loop
    if constexpr (SB == 1) qc = tile_popcounts_any<QB>(tp, lr, w16, s_planes, ones);
    else tile_dot_multibit_any<QB, SB>(tp, lr, w16, s_planes, qc, ones);
  }
  if (COMPACT || !a.idx.geom.has_x1) x1 = (double)ones;  // quantizedComponentSum of a freshly quantized row is its popcount / component sum

  const double s64 = score_f64((double)qc, lu.x, lu.y, xadd, x1, p);
  if (valid) {
    if (a.out_qcdist) a.out_qcdist[i] = (int32_t)qc;
    if (a.out_score64) a.out_score64[i] = s64;
    if (a.out_score32) a.out_score32[i] = (float)s64;
  }
}

template <int QB, int W, int SB>
hipError_t launch_gather_t(const GatherArgs &a, int n_queries, int64_t max_count, hipStream_t s) {
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  const size_t smem = (size_t)w16 * query_units_per_chunk(QB, SB) * 16;
  dim3 grid((unsigned)((max_count + kGatherThreads - 1) / kGatherThreads), (unsigned)n_queries, 1), block(kGatherThreads, 1, 1);
  if (a.idx.geom.layout == kLayoutCompact) hipLaunchKernelGGL((bbq_score_ords_kernel<QB, W, SB, true>), grid, block, smem, s, a);
  else hipLaunchKernelGGL((bbq_score_ords_kernel<QB, W, SB, false>), grid, block, smem, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_score_ords(const GatherArgs &a, int planes, int n_queries, int64_t max_count, hipStream_t s) {
  if (n_queries <= 0 || max_count <= 0) return hipSuccess;
  if (n_queries > 65535 || (uint64_t)max_count + kGatherThreads > kGridWorkItemsMax) return hipErrorInvalidValue;  // grid.y, and grid.x in work-items
  return rowlist_ladder(a.idx.geom, planes,
                        [&](auto qb, auto w, auto sb) { return launch_gather_t<qb(), w(), sb()>(a, n_queries, max_count, s); });
}

}  // namespace bbq
