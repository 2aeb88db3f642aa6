// bbq_shard.cpp - the scan of one shard of a row-sharded index: candidate lists packed for the host framework, synchronous or as
// up to two batches in flight (bbq_shard_scan_begin / _wait).
#include "bbq_search.h"

using namespace bbq;

namespace bbq {

int settle_shard_slots(DeviceCtx *ctx, bbq_index *owner) {
  for (int i = 0; i < kMaxSlots; ++i) {
    Slot &s = ctx->slots[i];
    if (!s.fl.busy || !s.fl.shard_owner || (owner && s.fl.shard_owner != owner)) continue;
    HIPCHK(hipEventSynchronize(s.ev_done));
    s.fl.busy = false;
    account_timing(s.fl.shard_owner, s);
    s.fl.shard_owner = nullptr;
  }
  return BBQ_OK;
}

}  // namespace bbq

extern "C" {

int64_t bbq_shard_list_cap(const bbq_index *ix, int64_t k) {
  if (!ix || k <= 0 || ix->multi) return 0;
  // the scan runs with rank k + 1 whenever it can leave shard-local answers (k <= kFinalSelectMax): size for that plan
  const int64_t keff = std::min<int64_t>(k, kMaxFastK);
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  return (keff <= kFinalSelectMax ? build_plan(ix, keff + 1, keff) : build_plan(ix, keff)).list_cap;
}

int bbq_shard_scan_begin(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                         int64_t k, void *dev_packed, int64_t packed_cap, void *dev_offsets, void *dev_flags, void *dev_answers,
                         int64_t answers_stride) {
  clear_error();
  int rc = validate_query_args(ix, n_queries, qquant, qcorr, query_bits, sim, k);
  if (rc != BBQ_OK) return rc;
  if (n_queries <= 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_shard_scan: n_queries must be positive");
  if (!dev_packed || !dev_offsets || !dev_flags || packed_cap <= 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_shard_scan: null output buffers");
  if (k == 0 || k > kMaxFastK) return fail(BBQ_ERR_UNSUPPORTED, "bbq_shard_scan: k must be in 1..%lld", (long long)kMaxFastK);
  if (dev_answers && answers_stride < k + 3) return fail(BBQ_ERR_INVALID_ARG, "bbq_shard_scan: answers_stride must be at least k + 3");
  if (dev_answers && k > kFinalSelectMax)
    return fail(BBQ_ERR_UNSUPPORTED, "bbq_shard_scan: shard-local answers exist for k <= %d (pass dev_answers = NULL and merge the lists)", kFinalSelectMax);
  if (ix->multi) return fail(BBQ_ERR_INVALID_ARG, "bbq_shard_scan: the handle is a multi-device index (it shards by itself)");
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  if (ix->shard_begun - ix->shard_waited >= 2) return fail(BBQ_ERR_INVALID_ARG, "bbq_shard_scan_begin: two batches are already in flight on this index (wait for one first)");
  SearchCall c(ix, qquant, qcorr, planes_of_call(ix, qquant, (int64_t)n_queries * ix->geom.dim, query_bits == 1), query_bits, sim, k);
  // with answers the shard runs with rank k + 1, like the single index does: its last finalize launch then knows the (k + 1)-th largest
  // key of everything it has seen (the cut) and the rows above it.  Lists for rank k + 1 are supersets of the lists for rank k where
  // both ranks plan the same segments (4 k and 4 (k + 1) can round to different first segments); either list replays to the same answer.
  const bool answers = dev_answers != nullptr;
  c.k_dev = answers ? k + 1 : k;
  const Plan plan = build_plan(ix, c.k_dev, answers ? k : 0);
  c.plan = &plan;
  bbq_index::ShardSet &set = ix->shard_set[ix->shard_begun & 1];
  if (!set.h_total) {
    HIPCHK(set.done.create(hipEventDisableTiming));
    HIPCHK(set.h_total.alloc(1));
  }
  // per-query lists with room for a flood (rows stored cluster by cluster); what travels is packed, so the headroom costs
  // device memory only
  const int64_t list_cap = plan.list_cap + std::min<int64_t>(plan.flood_cap, 65536);
  if (set.q_cap < n_queries || set.list_cap < list_cap) {  // per-query lists the finalize kernels build (the set is idle: its last batch was waited for)
    set.q_cap = 0;  // until both are in place
    HIPCHK(set.d_lists.alloc((size_t)n_queries * (size_t)list_cap));
    HIPCHK(set.d_counts.alloc((size_t)n_queries * 2 + 4));
    set.q_cap = n_queries;
    set.list_cap = list_cap;
  }
  const int Q = effective_batch(ix, n_queries);
  const int nslots = std::min(std::max(1, ix->opt_slots), kMaxSlots);
  const int64_t nsub = ((int64_t)n_queries + Q - 1) / Q;
  auto bail = [&](int code) {
    (void)settle_shard_slots(ix->ctx, nullptr);
    drain(ix);
    return code;
  };
  // slots other indexes (or the previous batch of this one) have left busy are retired one by one as they are needed: the device
  // keeps working on them while this batch is being enqueued behind
  for (int64_t i = 0; i < nsub; ++i) {
    Slot &s = ix->slots[i % nslots];
    if (s.fl.busy) {
      const hipError_t e = hipEventSynchronize(s.ev_done);
      if (e != hipSuccess) return bail(fail(BBQ_ERR_HIP, "bbq_shard_scan_begin: %s", hipGetErrorString(e)));
      s.fl.busy = false;
      account_timing(s.fl.shard_owner ? s.fl.shard_owner : ix, s);
      s.fl.shard_owner = nullptr;
    }
    const int nq = (int)std::min<int64_t>(Q, n_queries - i * Q);
    rc = ensure_slot(c, s, nq, false);
    if (rc != BBQ_OK) return bail(rc);
    ExtOut ext;
    ext.lists = set.d_lists + (size_t)(i * Q) * list_cap;
    ext.list_cap = list_cap;
    ext.counts = set.d_counts + (size_t)(i * Q) * 2;
    if (answers) {
      ext.answers = reinterpret_cast<uint64_t *>(dev_answers) + (size_t)(i * Q) * (size_t)answers_stride;
      ext.answers_stride = answers_stride;
    }
    rc = enqueue_subbatch(c, s, i * Q, nq, &ext);
    if (rc != BBQ_OK) return bail(rc);
    s.fl.shard_owner = ix;
  }
  // the packing runs on the auxiliary stream behind the last sub-batch of every slot this batch has used
  hipStream_t aux = ix->ctx->aux_stream;
  for (int j = 0; j < nslots; ++j)
    if (ix->slots[j].fl.busy && ix->slots[j].fl.shard_owner == ix) HIPCHK(hipStreamWaitEvent(aux, ix->slots[j].ev_done, 0));
  // pack: [nq][list_cap] -> contiguous entries + offsets, what the host framework sends over RCCL
  int64_t *d_total = reinterpret_cast<int64_t *>(set.d_counts + (size_t)n_queries * 2);
  d_total = reinterpret_cast<int64_t *>(((uintptr_t)d_total + 7) & ~(uintptr_t)7);
  HIPCHK(launch_pack(set.d_counts, set.d_lists, list_cap, plan.list_cap, n_queries, reinterpret_cast<int64_t *>(dev_offsets),
                     reinterpret_cast<int32_t *>(dev_flags), d_total, reinterpret_cast<uint64_t *>(dev_packed), packed_cap, aux));
  HIPCHK(hipMemcpyAsync(set.h_total, d_total, 8, hipMemcpyDeviceToHost, aux));
  HIPCHK(hipEventRecord(set.done, aux));
  set.packed_cap = packed_cap;
  ix->shard_begun += 1;
  return BBQ_OK;
}

int bbq_shard_scan_wait(bbq_index *ix, int64_t *out_total) {
  clear_error();
  if (!ix || ix->multi || !ix->ctx) return fail(BBQ_ERR_INVALID_ARG, "bbq_shard_scan_wait: not a shard handle");
  if (out_total) *out_total = 0;
  hipEvent_t ev = nullptr;
  bbq_index::ShardSet *set = nullptr;
  {
    std::lock_guard<std::mutex> lk(ix->ctx->mu);
    if (ix->shard_begun == ix->shard_waited) return fail(BBQ_ERR_INVALID_ARG, "bbq_shard_scan_wait: no batch in flight");
    set = &ix->shard_set[ix->shard_waited & 1];
    ev = set->done;
  }
  // outside the device mutex: the next batch is being enqueued by another thread meanwhile
  hipError_t e = hipEventSynchronize(ev);
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  ix->shard_waited += 1;
  if (e != hipSuccess) return fail(BBQ_ERR_HIP, "bbq_shard_scan_wait: %s", hipGetErrorString(e));
  const int64_t total = *set->h_total;
  if (out_total) *out_total = total;
  if (total > set->packed_cap) return fail(BBQ_ERR_OOM, "bbq_shard_scan: %lld candidates do not fit packed_cap %lld", (long long)total, (long long)set->packed_cap);
  return BBQ_OK;
}

int bbq_shard_scan(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                   int32_t sim, int64_t k, void *dev_packed, int64_t packed_cap, void *dev_offsets, void *dev_flags,
                   int64_t *out_total) {
  if (out_total) *out_total = 0;
  if (n_queries == 0) {
    clear_error();
    return validate_query_args(ix, n_queries, qquant, qcorr, query_bits, sim, k);
  }
  if (!out_total) return fail(BBQ_ERR_INVALID_ARG, "bbq_shard_scan: null output buffers");
  int rc = bbq_shard_scan_begin(ix, n_queries, qquant, qcorr, query_bits, sim, k, dev_packed, packed_cap, dev_offsets, dev_flags, nullptr, 0);
  if (rc != BBQ_OK) return rc;
  rc = bbq_shard_scan_wait(ix, out_total);
  if (rc != BBQ_OK) return rc;
  std::lock_guard<std::mutex> lk(ix->ctx->mu);  // the synchronous form leaves nothing in flight: timings are booked when it returns
  return settle_shard_slots(ix->ctx, ix);
}

}  // extern "C"
