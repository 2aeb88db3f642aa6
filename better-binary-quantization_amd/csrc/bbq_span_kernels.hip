// bbq_span_kernels.hip - span search (gfx950): bbq_search_spans_batch, bbq_search_spans_filtered_batch.
//
// The k best rows among a few contiguous runs of rows that differ from query to query.  Two passes.  The score pass streams every span as
// whole tiles - a work item is up to kChunkRows rows of one span of one query - and leaves the f32 score of each visited row at the row's
// position in the query's visiting order: no threshold, no bound, no atomic, the array the reference's heap would be fed.  The select pass,
// one workgroup per query, finds the exact (k + 1)-th largest score key of that array - in LDS where the keys fit the finalize kernel's key
// buffer, by a radix select over the scores in global memory otherwise - and writes the k rows above it when there are exactly k and no
// score is NaN: the case in which the heap provably ends up with those rows whatever its history was (DESIGN.md "Exact top-k").  The host
// sorts them, checks them for equal scores and replays the heap over the scores where the device could not prove the answer.
// With a row filter (FILT / ORDS below) only the accepted rows of the spans are visited: the score pass compacts them - an accepted row's
// score and ord go to its position among the query's accepted rows, a position computed from the filter's words alone - and the select
// pass, unchanged over the compacted scores, takes the ords of its k winners from that parallel array.
// Rows are scored with the sweep's own functions (bbq_kernel_common.h, bbq_scan_body.h): every score is bit for bit what the dense sweep
// writes for that row.
#include <hip/hip_runtime.h>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_launch.h"
#include "bbq_rowlist.h"
#include "bbq_scan_body.h"

#pragma clang fp contract(off)

namespace bbq {

namespace {

// grid = work items of the launch; block = kChunkRows / 64 waves: wave w takes tile item.first_tile + w, one row per lane, and a wave
// whose tile holds no row of [row_lo, row_hi) loads nothing.  QB / W / SB as bbq_scan_kernel takes them; COMPACT: the corrections layout
// of the index - every row's exact corrections come from the side array, as in the dense sweep.  The row's component sum comes from the
// row_sums side array where the launch's view carries it and is counted otherwise - the same value either way.
// FILT: a.accept holds one word per tile, bit l = lane l.  The wave's rows are those of its filter word that lie in [row_lo, row_hi) - a
// bit of the same tile outside the span counts nowhere - and a wave without one returns before any tile load.  An accepted row's position
// is item.out + the item's accepted rows in the tiles in front of the wave's + the accepted rows of the tile below the lane: words read at
// wave-uniform addresses and popcounts, no atomic, the same positions on every run.  Rejected lanes write nothing.
template <int QB, int W, int SB, bool COMPACT, bool FILT>
__global__ __launch_bounds__(kChunkRows) void bbq_span_score_kernel(const SpanScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = kChunkRows;
  constexpr int QU = query_units_per_chunk(QB, SB);
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  u32x4 *s_planes = reinterpret_cast<u32x4 *>(smem);
  const SpanItem it = a.items[blockIdx.x];  // workgroup-uniform
  const int q = (int)it.query;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  {  // stage the query's planes once per workgroup.  (Written out, not stage_query_planes: with no branch of the kernel's own between the
     // wave number and its readfirstlane, this build's compiler moves the shift behind it and the 24 unfiltered kernels of the inline layout
     // at a compiled width come out with 52 scalar registers for 54 - harmless, but not the kernel it was)
    const u32x4 *__restrict__ gp = reinterpret_cast<const u32x4 *>(a.qplanes) + (size_t)q * w16 * QU;
    for (int i = tid; i < w16 * QU; i += NT) s_planes[i] = gp[i];
  }
  const QueryParams p = a.qparams[q];
  __syncthreads();

  const int64_t tile = (int64_t)it.first_tile + __builtin_amdgcn_readfirstlane(wave);
  if (tile * kTileRows >= (int64_t)it.row_hi) return;  // wave-uniform: no row of the item in this tile (row_hi <= n_rows: the tile exists otherwise)
  const int64_t row = tile * kTileRows + lane;
  uint64_t mine = 0;    // FILT: the wave's accepted rows of the item, bit l = lane l, and how many the item has in front of this tile:
  uint32_t before = 0;  // wave-uniform both, kept in scalar registers until the score is there
  if constexpr (FILT) {
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const uint64_t from_lo = ~0ull << (it.row_lo & 63u);  // the lanes of the item's first tile at or behind row_lo
    const int64_t left = (int64_t)it.row_hi - tile * kTileRows;  // > 0; every tile in front of this one lies below row_hi as a whole
    mine = a.accept[tile] & (left < kTileRows ? (1ull << left) - 1ull : ~0ull);
    if (wave_u == 0) mine &= from_lo;
    if (mine == 0) return;  // wave-uniform: no accepted row of the item in this tile
#pragma unroll
    for (int t = 0; t < kTilesPerChunk - 1; ++t)
      if (t < wave_u) before += (uint32_t)__popcll(a.accept[(int64_t)it.first_tile + t] & (t == 0 ? from_lo : ~0ull));
  }
  const uint8_t *__restrict__ tp = a.idx.tiles + tile * (int64_t)a.idx.geom.tile_stride;
  const bool resident = chunk_is_resident(tile / kTilesPerChunk, a.idx);
  const RowTerms rt = tile_row_terms<QB, W, SB, COMPACT>(a.idx, tp, row, lane, w16, resident, s_planes);

  const float s32 = (float)score_f64((double)rt.qc, rt.lu.x, rt.lu.y, rt.xadd, rt.x1, p);
  if constexpr (FILT) {
    if ((mine >> lane) & 1ull) {
      const int64_t out = it.out + before + __popcll(mine & ((1ull << lane) - 1ull));
      a.scores[out] = s32;
      a.ords[out] = (uint32_t)row;
    }
  } else {
    if (row >= (int64_t)it.row_lo && row < (int64_t)it.row_hi) a.scores[it.out + (row - (int64_t)it.row_lo)] = s32;
  }
}

template <int QB, int W, int SB>
hipError_t launch_span_score_t(const SpanScoreArgs &a, unsigned n_items, hipStream_t s) {
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  const size_t smem = (size_t)w16 * query_units_per_chunk(QB, SB) * 16;
  dim3 grid(n_items, 1, 1), block(kChunkRows, 1, 1);
  const bool compact = a.idx.geom.layout == kLayoutCompact;
  if (a.accept) {
    if (compact) hipLaunchKernelGGL((bbq_span_score_kernel<QB, W, SB, true, true>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_span_score_kernel<QB, W, SB, false, true>), grid, block, smem, s, a);
  } else {
    if (compact) hipLaunchKernelGGL((bbq_span_score_kernel<QB, W, SB, true, false>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_span_score_kernel<QB, W, SB, false, false>), grid, block, smem, s, a);
  }
  return hipGetLastError();
}

// ---- the select pass ----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t key_of_score(float s) { return key_of_bits(__float_as_uint(s)); }

// one histogram step of a radix pass for the whole wave: the lanes that share the first active lane's bin add once for all of them (the
// upper bytes of one query's score keys are nearly constant: thousands of adds on one LDS word otherwise, block_select_kth_largest_t)
__device__ __forceinline__ void hist_add(uint32_t *hist, bool in, uint32_t bin, int lane) {
  const unsigned long long act = __ballot(in);
  if (!act) return;
  const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, __ffsll((long long)act) - 1);
  const unsigned long long same = __ballot(in && bin == b0);
  if (in && bin == b0) {
    if (lane == __ffsll((long long)same) - 1) atomicAdd(&hist[b0], (uint32_t)__popcll(same));
  } else if (in) {
    atomicAdd(&hist[bin], 1u);
  }
}

// k-th largest key (L >= k >= 1) of the L scores in global memory, one kFinalizeThreads workgroup; every thread returns it.  Four 8-bit
// passes from the top byte down, each a histogram in LDS over the keys that match the prefix found so far.  The scores of sixteen steps
// are loaded before any of them is used: a pass is bound by the latency of its loads (one workgroup walks the whole array), so the array
// is read as few times as possible - the first pass also looks for NaN scores (-> nan_seen, per thread; the result means nothing then), and
// rank_in_cut, the answer's rank among the keys equal to it, makes k - rank_in_cut the number of keys above it without another pass.
// s_hist: 256 words, s_scr: 2 words.
__device__ __forceinline__ uint32_t global_select_kth_largest(const float *__restrict__ sc, int64_t L, uint32_t k, uint32_t *s_hist, uint32_t *s_scr,
                                                              bool &nan_seen, uint32_t &rank_in_cut) {
  constexpr int NT = kFinalizeThreads;
  constexpr int U = 16;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  uint32_t prefix = 0, mask = 0, kk = k;
  for (int pass = 3; pass >= 0; --pass) {
    const int sh = pass * 8;
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (int64_t i0 = 0; i0 < L; i0 += (int64_t)U * NT) {  // whole waves iterate together (ballots in hist_add)
      uint32_t kv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + (int64_t)u * NT + tid;
        const float s = sc[i < L ? i : 0];
        if (pass == 3) nan_seen |= s != s;
        kv[u] = key_of_score(s);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = i0 + (int64_t)u * NT + tid;
        const bool in = i < L && (kv[u] & mask) == prefix;
        hist_add(s_hist, in, (kv[u] >> sh) & 255u, lane);
      }
    }
    __syncthreads();
    if (tid < 64) {  // wave 0 finds the bin: lane l owns bins 4l..4l+3, suffix sums over lanes by shuffles
      const uint32_t h0 = s_hist[4 * tid], h1 = s_hist[4 * tid + 1], h2 = s_hist[4 * tid + 2], h3 = s_hist[4 * tid + 3];
      uint32_t suf = h0 + h1 + h2 + h3;  // becomes the sum over bins >= 4 * tid
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t n = __shfl_down(suf, d, 64);
        if (tid + d < 64) suf += n;
      }
      const uint32_t above = suf - (h0 + h1 + h2 + h3);  // bins > 4 * tid + 3
      if (suf >= kk && above < kk) {                     // exactly one lane: the k-th largest lies in its 4 bins
        uint32_t cum = above;
        int b = 4 * tid + 3;
        if (cum + h3 < kk) { cum += h3; b = 4 * tid + 2;
          if (cum + h2 < kk) { cum += h2; b = 4 * tid + 1;
            if (cum + h1 < kk) { cum += h1; b = 4 * tid; } } }
        s_scr[0] = (uint32_t)b;
        s_scr[1] = kk - cum;
      }
    }
    __syncthreads();
    prefix |= s_scr[0] << sh;
    mask |= 255u << sh;
    kk = s_scr[1];
    // (the next pass clears the histogram behind this barrier and writes s_scr behind two more)
  }
  __syncthreads();
  rank_in_cut = kk;
  return prefix;
}

// the ord at position i of a query's visiting order: its non-empty spans as {first position, first row}, ascending in both
__device__ __forceinline__ int64_t span_ord(const SpanRun *__restrict__ runs, int n_runs, int64_t i) {
  int lo = 0, hi = n_runs - 1;  // the last run that starts at or in front of i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (runs[mid].pos <= i) lo = mid; else hi = mid - 1;
  }
  return runs[lo].begin + (i - runs[lo].pos);
}

// one kFinalizeThreads workgroup per selected query (the host selects those with len > k and 1 <= k <= kSpanSelectMax).  Leaves in the
// query's block of a.out: word 0 = {rows whose key lies above the cut | flags << 32}, word 1 = the cut's f32 score bits, and - when
// exactly k rows lie above the cut and no score is NaN - those k rows as entries, in any order.  ORDS: the scores are the compacted ones
// of a filtered query and a winner's ord is a.ords' at its position; the runs are not read.
template <bool ORDS>
__global__ __launch_bounds__(kFinalizeThreads) void bbq_span_select_kernel(const SpanSelectArgs a) {
  constexpr int NT = kFinalizeThreads;
  __shared__ uint32_t s_keys[kFinalizeKeyCap];
  __shared__ uint32_t s_hist[512];
  __shared__ uint32_t s_wave[16];
  __shared__ uint32_t s_scr[8];
  __shared__ uint32_t s_red[4];  // 0: a NaN was seen, 1: keys above the cut, 2: entries written so far
  const SpanQuery sq = a.sel[blockIdx.x];
  const float *__restrict__ sc = a.scores + sq.score_off;
  const int64_t L = sq.len;
  const uint32_t k = (uint32_t)a.k;
  uint64_t *__restrict__ out = a.out + (size_t)blockIdx.x * (size_t)a.out_stride;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const bool in_lds = L <= kFinalizeKeyCap;  // workgroup-uniform
  if (tid < 4) s_red[tid] = 0;
  __syncthreads();

  // the cut = the (k + 1)-th largest key, and the number of keys above it (<= k).  A NaN anywhere: order statistics mean nothing, the
  // host replays the heap
  bool nan = false;
  uint32_t cut = 0, above = 0;
  if (in_lds) {
    for (int64_t i = tid; i < L; i += NT) {
      const float s = sc[i];
      nan |= s != s;
      s_keys[i] = key_of_score(s);
    }
    if (__any(nan) && lane == 0) s_red[0] = 1u;
    __syncthreads();
    if (s_red[0] == 0u) {  // workgroup-uniform
      cut = block_select_kth_largest(s_keys, (uint32_t)L, k + 1u, s_hist, s_wave, s_scr);
      uint32_t cnt = 0;
      for (int64_t i = tid; i < L; i += NT) cnt += s_keys[i] > cut ? 1u : 0u;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
      if (lane == 0 && cnt != 0) atomicAdd(&s_red[1], cnt);
      __syncthreads();
      above = s_red[1];
    }
  } else {
    uint32_t rank_in_cut = 0;
    cut = global_select_kth_largest(sc, L, k + 1u, s_hist, s_scr, nan, rank_in_cut);
    if (__any(nan) && lane == 0) s_red[0] = 1u;
    __syncthreads();
    above = k + 1u - rank_in_cut;
  }
  if (s_red[0] != 0u) {  // workgroup-uniform
    if (tid == 0) {
      out[0] = header_word(0u, kFlagNaN);
      out[1] = 0;
    }
    return;
  }
  if (tid == 0) {
    out[0] = header_word(above, 0u);
    out[1] = bits_of_key(cut);
  }
  if (above != k) return;  // fewer: scores equal to the cut among the k + 1 largest - the host replays the heap

  constexpr int U = 8;  // as in the radix passes: the loads of several steps in flight
  for (int64_t i0 = 0; i0 < L; i0 += (int64_t)U * NT) {  // whole waves iterate together
    float sv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + (int64_t)u * NT + tid;
      sv[u] = sc[i < L ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = i0 + (int64_t)u * NT + tid;
      const bool in = i < L && key_of_score(sv[u]) > cut;
      const unsigned long long m = __ballot(in);
      if (m == 0) continue;
      uint32_t base = 0;
      if (lane == __ffsll((long long)m) - 1) base = atomicAdd(&s_red[2], (uint32_t)__popcll(m));
      base = (uint32_t)__builtin_amdgcn_readlane((int)base, __ffsll((long long)m) - 1);
      const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (in && slot < k) {  // (slot < k: there are `above` of them)
        int64_t ord;
        if constexpr (ORDS) ord = (int64_t)a.ords[sq.score_off + i];
        else ord = span_ord(a.runs + sq.run_first, sq.n_runs, i);
        out[2 + slot] = candidate_entry(ord, sv[u]);
      }
    }
  }
}

}  // namespace

hipError_t launch_span_score(const SpanScoreArgs &a, int planes, int64_t n_items, hipStream_t s) {
  if (n_items <= 0) return hipSuccess;
  if (a.accept && !a.ords) return hipErrorInvalidValue;
  if ((uint64_t)n_items * kChunkRows > kGridWorkItemsMax) return hipErrorInvalidValue;  // grid.x in work-items
  const unsigned n = (unsigned)n_items;
  return rowlist_ladder(a.idx.geom, planes, [&](auto qb, auto w, auto sb) { return launch_span_score_t<qb(), w(), sb()>(a, n, s); });
}

hipError_t launch_span_select(const SpanSelectArgs &a, int n_selected, hipStream_t s) {
  if (n_selected <= 0) return hipSuccess;
  if (a.k < 1 || a.k > kSpanSelectMax || a.out_stride < a.k + 2) return hipErrorInvalidValue;
  if (a.ords) hipLaunchKernelGGL(bbq_span_select_kernel<true>, dim3((unsigned)n_selected, 1, 1), dim3(kFinalizeThreads, 1, 1), 0, s, a);
  else hipLaunchKernelGGL(bbq_span_select_kernel<false>, dim3((unsigned)n_selected, 1, 1), dim3(kFinalizeThreads, 1, 1), 0, s, a);
  return hipGetLastError();
}

}  // namespace bbq
