// bbq_latency.cpp - the two launch chains of a single-query call (kernels: bbq_latency_kernels.hip): the query travels in the kernel
// arguments, the answer comes back through mapped host memory.
#include <string.h>
#include "bbq_search.h"

using namespace bbq;

namespace {

// behind the last launch of a chain: the event that ends it, then the wait for the sequence word that launch raises in mapped host
// memory (polling: no copy) - the answer block it left is there when this returns BBQ_OK
int await_latency_answer(DeviceCtx *ctx, Slot &s, uint64_t seq) {
  HIPCHK(hipEventRecord(s.ev_done, s.stream));
  s.fl.timed = false;
  volatile uint64_t *flag = ctx->h_lat;
  for (int64_t spin = 0; spin < (1ll << 31); ++spin) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return BBQ_OK;
    if ((spin & 0xffff) == 0xffff && hipEventQuery(s.ev_done) != hipErrorNotReady) break;  // the launch chain is over (or failed)
    __builtin_ia32_pause();
  }
  const hipError_t e = hipEventSynchronize(s.ev_done);
  if (e == hipSuccess && __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return BBQ_OK;
  s.ctrl_clean = false;  // whatever the chain left behind
  if (e != hipSuccess) return fail(BBQ_ERR_HIP, "latency path: %s", hipGetErrorString(e));
  return fail(BBQ_ERR_HIP, "latency path: the device finished without an answer");
}

// what both latency chains sweep the main storage with: the slot's control words and list, the query (*resident_bytes: of a sweep over all rows)
static LatScanArgs lat_scan_args(const SearchCall &c, Slot &s, int64_t *resident_bytes = nullptr) {
  bbq_index *ix = c.ix;
  LatScanArgs a{};
  const LaunchView lv = launch_view(ix, ix->main);
  if (resident_bytes) *resident_bytes = lv.resident_bytes;
  a.idx = lv.view;
  a.row_id_base = ix->main.row_id_base;
  a.theta = s.d_theta;
  a.flags = s.d_flags;
  a.list_counts = s.d_list_counts;
  a.append_count = s.d_append_counts;
  a.list = s.d_lists;
  a.list_cap = s.list_cap;
  fill_query(ix, reinterpret_cast<uint8_t *>(a.planes), &a.p, c.qquant, c.qcorr, c.planes, c.one_bit, c.sim);
  return a;
}

// the answer the device proved (the entries behind header h of the block in mapped host memory) goes to the caller
void take_answer(bbq_index *ix, const uint64_t *block, const AnswerHeader &h, int32_t *out_idx, float *out_score, int64_t *out_n, bool *done) {
  unpack_entries(block + 2, h.count, out_idx, out_score);
  out_n[0] = h.count;
  ix->stats.candidates += h.listed;
  *done = true;
}

// the chain's slot gets the workspace of the plan at hand and all-zero control words
int prepare_latency_slot(const SearchCall &c, Slot &s) {
  int rc = ensure_slot(c, s, 1, true);
  if (rc != BBQ_OK) return rc;
  if (!s.ctrl_clean) {  // the slot's last user was not a latency chain
    HIPCHK(hipMemsetAsync(s.d_block, 0, (size_t)s.ctrl_bytes, s.stream));
    s.ctrl_clean = true;
  }
  return BBQ_OK;
}

// makes `f` the answering finalize launch of a chain: the answer to mapped host memory, then the sequence word
void answer_to_host(FinalizeArgs &f, DeviceCtx *ctx, int64_t final_k, uint64_t seq) {
  f.final_out = ctx->d_lat + kLatAnswerOffset;
  f.final_stride = kFinalSelectMax + 2;
  f.final_k = (int32_t)final_k;
  f.done_flag = ctx->d_lat;
  f.seq = seq;
}

}  // namespace

namespace bbq {

// The single-query call on a large index: threshold from a pre-sampled prefix (bbq_lat_pre_kernel + bbq_lat_select_kernel: two small
// launches), ONE sweep over all rows with it, final selection on the list alone - four launches where the segmented chain has six,
// and nothing in front of the large sweep but the two small ones.  The list is every row above the threshold, not a heap history: a
// query whose answer the device cannot prove (equal scores, NaN, more candidates than the selection holds) is handed to the
// segmented chain (*done = false), which replays it exactly.
int search_latency_presampled(const SearchCall &c, int32_t *out_idx, float *out_score, int64_t *out_n, bool *done) {
  bbq_index *ix = c.ix;
  const Plan &p = *c.plan;
  *done = false;
  const int64_t N = ix->main.view.n_rows, k2 = p.final_k;
  if (!ix->opt_latency_presample || !ix->opt_latency_fused || ix->has_pilot || c.share != 1 || !p.latency ||
      k2 < 1 || k2 > kFinalSelectMax || N < 262144 || !latency_path_supported(ix->main.view, c.planes))
    return BBQ_OK;
  // sample enough rows for ~6000 candidates in the sweep (the selection holds kFinalizeKeyCap of them)
  int64_t P = ((k2 + 2) * N / 6000 + kChunkRows - 1) / kChunkRows * kChunkRows;
  P = std::max<int64_t>(P, 8192);
  if (P > N / 4) return BBQ_OK;
  // Keys per wave of the sample: ONE (the wave's maximum) when the sample has at least eight times as many waves as the rank asks for -
  // two of the rank's best rows then rarely share a wave, the threshold is all but the prefix's true order statistic, and the selection
  // launch has a quarter of the keys to go through (10 M rows, k = 100: 2 656 instead of 10 624 keys, select 11.6 -> 6.6 us, pre-sample
  // 9.4 -> 8.0 us); four otherwise.  Either way the threshold is an order statistic of a SUBSET of the rows: a valid lower bound.
  int per_wave = (P / kTileRows >= 8 * (k2 + 2)) ? 1 : 4;
  if (P / kTileRows * per_wave > kLatPreKeys) per_wave = 1;
  const int64_t n_keys = P / kTileRows * per_wave;
  if (n_keys > kLatPreKeys || n_keys < k2 + 2) return BBQ_OK;
  Slot &s = ix->slots[0];
  int rc = prepare_latency_slot(c, s);
  if (rc != BBQ_OK) return rc;
  DeviceCtx *ctx = ix->ctx;
  hipStream_t st = s.stream;
  LatScanArgs a = lat_scan_args(c, s, &ix->stats.resident_bytes);  // of the one sweep over all rows, not sweep + prefix
  LatPreArgs pre{};
  pre.idx = launch_view(ix, ix->main).view;
  pre.rows = (int32_t)P;
  pre.per_wave = per_wave;
  pre.pre_keys = ctx->d_pre_keys;
  pre.flags = s.d_flags;
  pre.p = a.p;
  memcpy(pre.planes, a.planes, sizeof pre.planes);
  HIPCHK(launch_lat_pre(pre, c.planes, st));
  // rank k2 + 2: the sweep must list at least k2 + 1 rows for the selection to see the boundary of the answer
  HIPCHK(launch_lat_select(ctx->d_pre_keys, (int)n_keys, (int)(k2 + 2), s.d_theta, a.p, st));
  a.chunk_begin = 0;
  a.n_chunks = (int32_t)ix->main.n_chunks();
  a.first = 0;
  HIPCHK(launch_lat_scan(a, c.planes, st));
  const uint64_t seq = ++ctx->lat_seq;
  FinalizeArgs f = slot_finalize_args(s, s.d_lists, s.d_list_counts, s.list_cap, true, c.k_dev);
  f.qp1 = a.p;
  f.emit = 1;
  answer_to_host(f, ctx, k2, seq);
  HIPCHK(launch_finalize(f, 1, st));
  rc = await_latency_answer(ctx, s, seq);
  if (rc != BBQ_OK) return rc;
  const AnswerHeader r(ctx->h_lat + kLatAnswerOffset);
  // The list holds the rows ABOVE the sampled threshold only, so the selection's "take every listed row" case (total <= k2) proves
  // nothing here: equal keys at ranks k2+1 / k2+2 of the sample can leave fewer than k2 rows above it (N >= 262144 > k2, so a
  // complete answer has exactly k2 entries).  Anything else goes to the segmented chain.
  if (r.flags != 0 || r.needs_replay != 0 || r.count != (uint32_t)k2) return BBQ_OK;
  take_answer(ix, ctx->h_lat + kLatAnswerOffset, r, out_idx, out_score, out_n, done);
  return BBQ_OK;
}

// one query, no copies: every sweep takes the query from its kernel arguments (bbq_latency_kernels.hip), the last finalize launch
// writes the answer to mapped host memory and raises the sequence word this thread polls.  Returns BBQ_OK with *done = false when the
// call has to take the general path (index shape without an instantiation).
int search_latency_chain(const SearchCall &c, int32_t *out_idx, float *out_score, int64_t *out_n, bool *done) {
  bbq_index *ix = c.ix;
  const Plan &p = *c.plan;
  *done = false;
  if (!ix->opt_latency_fused || !ix->opt_append_last || ix->has_pilot || c.share != 1 || !p.latency ||
      p.final_k < 1 || p.final_k > kFinalSelectMax || p.segs.empty() || !p.segs[0].dense || !latency_path_supported(ix->main.view, c.planes))
    return BBQ_OK;
  for (size_t i = 1; i < p.segs.size(); ++i)
    if (p.segs[i].dense || p.segs[i].storage != 1) return BBQ_OK;
  Slot &s = ix->slots[0];
  int rc = prepare_latency_slot(c, s);
  if (rc != BBQ_OK) return rc;
  DeviceCtx *ctx = ix->ctx;
  hipStream_t st = s.stream;
  LatScanArgs a = lat_scan_args(c, s);
  const uint64_t seq = ++ctx->lat_seq;
  for (size_t i = 0; i < p.segs.size(); ++i) {
    const Segment &g = p.segs[i];
    a.chunk_begin = g.chunk_begin;
    a.n_chunks = (int32_t)g.n_chunks;
    a.first = i == 0 ? 1 : 0;
    HIPCHK(launch_lat_scan(a, c.planes, st));
    FinalizeArgs f = slot_finalize_args(s, s.d_lists, s.d_list_counts, s.list_cap, true, c.k_dev);
    f.qp1 = a.p;  // (qparams stays null: the query is in no device buffer)
    f.emit = 1;
    f.need_theta = i + 1 < p.segs.size() ? 1 : 0;
    if (i + 1 == p.segs.size()) answer_to_host(f, ctx, p.final_k, seq);
    HIPCHK(launch_finalize(f, 1, st));
  }
  rc = await_latency_answer(ctx, s, seq);
  if (rc != BBQ_OK) return rc;
  const AnswerHeader r(ctx->h_lat + kLatAnswerOffset);
  if (r.flags == 0 && r.needs_replay == 0) {  // answered on the device
    take_answer(ix, ctx->h_lat + kLatAnswerOffset, r, out_idx, out_score, out_n, done);
    return BBQ_OK;
  }
  // equal scores in or at the edge of the answer (or a flagged query): the general path's collection steps for this one query - the
  // list on the device is complete and it is this slot's
  rc = replay_listed_query(c, s, r.listed, r.flags, out_idx, out_score, out_n);
  if (rc != BBQ_OK) return rc;
  *done = true;
  return BBQ_OK;
}

}  // namespace bbq
