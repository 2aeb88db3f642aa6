// bbq_maxsim_cand_kernels.hip - MaxSim over chosen groups (gfx950): bbq_score_maxsim_groups_batch, bbq_search_maxsim_groups_batch.
//
// The MaxSim score S = (float)((double)m_0 + (double)m_1 + ...) of bbq_search_maxsim_batch (bbq_maxsim_kernels.hip), for the groups a
// query NAMES - its candidate list, groups of a group set in any order, duplicates included - instead of every live group of the index.
// The score pass of this file is a gather shaped like bbq_score_ords_kernel (bbq_gather_kernels.hip) with the fused MaxSim kernel's
// token loop inside: a lane is one row of the query's EXPANDED rows - the rows of its candidates back to back in list order - and finds
// its candidate by binary search over the prefix records the host staged (MaxSimCand, bbq_device.h: one per candidate, never a row
// list), once per token block.  It loads its row once - for the compiled widths every load of the row is issued before the first is used
// and codes and corrections stay in registers - and per token of the block staged in LDS pays the popcounts, the score, the packed key
// (group_key: a rejected row's is 0) and the six-step segmented maximum over the lanes of one candidate.  A candidate that lies wholly
// inside the wave is stored plainly into rep[token][entry]; one that a wave's or a workgroup's edge cuts is raised with the 64-bit
// atomicMax into the cleared rep: a maximum does not depend on the order its operands arrive in, so the result is the same on every
// run.  A wave none of whose rows is accepted loads nothing.  The other widths, and the multi-bit rows, walk their chunks in the sweep's
// run-time loop per token: their row comes from the cache, not from registers.
// The keys of a block are then added by bbq_maxsim_accumulate_kernel (bbq_maxsim_kernels.hip) with the entry as its slot.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "bbq_device.h"
#include "bbq_kernel_common.h"
#include "bbq_launch.h"
#include "bbq_rowlist.h"
#include "bbq_scan_body.h"

#pragma clang fp contract(off)

namespace bbq {

namespace {

constexpr size_t kCandLdsMax = 64 * 1024;  // what a launch asks for without an attribute; four workgroups of a CU's 160 KB at the default shapes

// LDS of a workgroup: [tok_pass][w16 * QU] planes | [tok_pass] QueryParams
constexpr size_t cand_token_bytes(int w16, int qu) { return (size_t)w16 * qu * 16 + sizeof(QueryParams); }
static_assert(kMaxSimTokenBlock * cand_token_bytes(12, 8) <= kCandLdsMax && kMaxSimTokenBlock * cand_token_bytes(6, 4) <= 16 * 1024,
              "every compiled width stages a whole token block; 768-d x 4 planes leaves room for eight workgroups a CU");

// grid = (pieces of kMaxSimCandThreads expanded rows of the longest list of the launch, the block's queries); QB / W / SB / COMPACT as
// bbq_score_ords_kernel takes them (W > 0: 1-bit rows only), FILT: a.accept holds the group set's accept words.
template <int QB, int W, int SB, bool COMPACT, bool FILT>
__global__ __launch_bounds__(kMaxSimCandThreads) void bbq_maxsim_cand_kernel(const MaxSimCandArgs a) {
  static_assert(W == 0 || SB == 1, "the register-resident form is that of 1-bit rows");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int NT = kMaxSimCandThreads;
  constexpr int QU = query_units_per_chunk(QB, SB);
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  const int PU = w16 * QU;  // 16-byte units of a token's planes
  const MaxSimQuery mq = a.queries[blockIdx.y];
  const MaxSimCandQuery cq = a.cq[mq.query];
  const int64_t x0 = (int64_t)blockIdx.x * NT;
  if (x0 >= cq.total) return;  // workgroup-uniform: this piece lies beyond the query's expanded rows
  const int n_tok = mq.n_tok < kMaxSimTokenBlock ? mq.n_tok : kMaxSimTokenBlock;
  const int tok_pass = a.tok_pass;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  u32x4 *s_planes = reinterpret_cast<u32x4 *>(smem);
  QueryParams *s_params = reinterpret_cast<QueryParams *>(smem + (size_t)tok_pass * PU * 16);

  // the lane's expanded row and its candidate: the last record at or in front of it.  A lane beyond the list shadows the list's last
  // row, so every address stays in bounds; it is a segment of its own whose key is 0
  const int64_t x = x0 + tid;
  const bool valid = x < cq.total;
  const uint32_t xc = (uint32_t)(valid ? x : (int64_t)cq.total - 1);
  const MaxSimCand *__restrict__ recs = a.recs + cq.rec_first;
  int e = 0;
  {
    int hi = cq.n_cand - 1;
    while (e < hi) {
      const int mid = (e + hi + 1) >> 1;
      if (recs[mid].pos <= xc) e = mid;
      else hi = mid - 1;
    }
  }
  const MaxSimCand rc = recs[e];
  const uint32_t next_pos = recs[e + 1].pos;  // the terminator's for the last candidate
  const int64_t r = (int64_t)rc.first_row + (xc - rc.pos);
  bool accepted = valid;
  if constexpr (FILT) accepted = valid && ((a.accept[r >> 6] >> (r & 63)) & 1ull);
  const bool active = __ballot(accepted) != 0ull;  // wave-uniform

  // the lane's segment, once: the lanes of its candidate inside this wave
  const uint64_t heads = __ballot(!valid || xc == rc.pos) | 1ull;
  const int head = segment_head(heads, lane);
  const bool is_end = valid && (lane == kTileRows - 1 || ((heads >> (lane + 1)) & 1ull));
  const int64_t wave_x = x - lane;
  const bool whole = (int64_t)rc.pos >= wave_x && (int64_t)next_pos <= wave_x + kTileRows;  // no other wave of the launch sees this entry

  // the row, once: codes and corrections stay in registers over the tokens
  const uint8_t *__restrict__ tp = a.idx.tiles + (r >> 6) * (int64_t)a.idx.geom.tile_stride;
  const int lr = (int)(r & 63);
  const bool rs = COMPACT && a.idx.row_sums != nullptr;  // uniform over the launch
  f64x2 lu = {0.0, 0.0};
  double xadd = 0.0, x1 = 0.0;
  uint32_t ones = 0;
  u32x4 c[W > 0 ? W : 1];
  (void)c;
  if (active) {
    load_row<W, COMPACT>(a.idx, tp, lr, r, w16, rs, c, lu, xadd, x1, ones);
    // nothing crosses this line: every load of the row is in flight before the staging below and the first popcount wait for anything
    __builtin_amdgcn_sched_barrier(0);
  }

  unsigned long long *__restrict__ rep = a.rep + (size_t)mq.vec_first * (size_t)a.stride + (size_t)e;  // token 0 of the block; token t: + t * stride
  for (int t0 = 0; t0 < n_tok; t0 += tok_pass) {  // one pass for every compiled width
    const int np = n_tok - t0 < tok_pass ? n_tok - t0 : tok_pass;
    if (t0 > 0) __syncthreads();  // the last pass's readers are done
    stage_token_block<NT>(s_planes, s_params, reinterpret_cast<const u32x4 *>(a.qplanes) + (size_t)(mq.vec_first + t0) * PU,
                          a.qparams + mq.vec_first + t0, np, PU, tid);  // the pass's
    __syncthreads();
    if (!active) continue;  // wave-uniform; the barriers above are reached by every wave
    if constexpr (W > 0) {
      if (t0 == 0 && !rs) ones = row_popcount(c, ones);
    }
    for (int t = 0; t < np; ++t) {
      const QueryParams p = token_params(s_params, t);
      const u32x4 *pl = s_planes + t * PU;
      uint32_t qc;
      if constexpr (W > 0) {
        uint32_t unused = 0;
        qc = tile_popcounts<QB, W, false>(c, pl, unused);
      } else if (rs) {
        if constexpr (SB == 1) qc = tile_popcounts_any<QB, false>(tp, lr, w16, pl, ones);
        else tile_dot_multibit_any<QB, SB, false>(tp, lr, w16, pl, qc, ones);
      } else {
        if constexpr (SB == 1) qc = tile_popcounts_any<QB>(tp, lr, w16, pl, ones);
        else tile_dot_multibit_any<QB, SB>(tp, lr, w16, pl, qc, ones);
      }
      const double xs = (COMPACT || !a.idx.geom.has_x1) ? (double)ones : x1;  // quantizedComponentSum of a freshly quantized row is its popcount / component sum
      const float s32 = (float)score_f64((double)qc, lu.x, lu.y, xadd, xs, p);
      const unsigned long long key = segment_max(accepted ? group_key(__float_as_uint(s32), s32 != s32, (uint32_t)r) : 0ull, head, lane);
      if (is_end && key != 0ull) {
        unsigned long long *dst = rep + (size_t)(t0 + t) * (size_t)a.stride;
        if (whole) *dst = key;
        else atomicMax(dst, key);
      }
    }
  }
}

template <int QB, int W, int SB>
hipError_t launch_cand_t(const MaxSimCandArgs &args, int n_queries, int64_t longest, hipStream_t s) {
  MaxSimCandArgs a = args;
  const int w16 = W > 0 ? W : a.idx.geom.w16;
  const size_t per = cand_token_bytes(w16, query_units_per_chunk(QB, SB));
  if (per > kCandLdsMax) return hipErrorInvalidValue;  // a row of more than 64 KB of staged query data
  a.tok_pass = (int32_t)std::min<size_t>(kMaxSimTokenBlock, kCandLdsMax / per);
  const size_t smem = (size_t)a.tok_pass * per;
  dim3 grid((unsigned)((longest + kMaxSimCandThreads - 1) / kMaxSimCandThreads), (unsigned)n_queries, 1), block(kMaxSimCandThreads, 1, 1);
  const bool compact = a.idx.geom.layout == kLayoutCompact;
  if (a.accept) {
    if (compact) hipLaunchKernelGGL((bbq_maxsim_cand_kernel<QB, W, SB, true, true>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_maxsim_cand_kernel<QB, W, SB, false, true>), grid, block, smem, s, a);
  } else {
    if (compact) hipLaunchKernelGGL((bbq_maxsim_cand_kernel<QB, W, SB, true, false>), grid, block, smem, s, a);
    else hipLaunchKernelGGL((bbq_maxsim_cand_kernel<QB, W, SB, false, false>), grid, block, smem, s, a);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_maxsim_cand_score(const MaxSimCandArgs &a, int planes, int n_queries, int64_t longest, hipStream_t s) {
  if (n_queries <= 0 || longest <= 0) return hipSuccess;
  if (n_queries > 65535 || longest > kMaxSimCandMaxRows || a.idx.n_rows > kGroupMaxRows) return hipErrorInvalidValue;  // grid.y; grid.x in work-items; the key's ord
  if (!a.queries || !a.cq || !a.recs || !a.rep || a.stride <= 0) return hipErrorInvalidValue;
  // the register-resident widths are those of 1-bit rows: a multi-bit row takes the run-time width
  return rowlist_ladder<MultiBitRows::kRunTimeWidth>(
      a.idx.geom, planes, [&](auto qb, auto w, auto sb) { return launch_cand_t<qb(), w(), sb()>(a, n_queries, longest, s); });
}

}  // namespace bbq
