// bbq_range.cpp - range search: bbq_range_key, bbq_count_range_batch, bbq_search_range_batch (kernels: bbq_range_kernels.hip).  The
// host turns every threshold into a key, checks everything before the first launch and works through the call in sub-batches: stage
// the queries, launch theta, count and offsets, bring back each query's total and the length of its list of non-empty chunks - where
// the count entry point stops - then fill in launches of bounded size and unpack their entries into the caller's arrays.
#include <string.h>
#include "bbq_search.h"

using namespace bbq;

namespace {

// A sub-batch takes at most this many queries and this much scratch for its per-chunk arrays (8 B per chunk and query: the counts,
// scanned in place into offsets, and the list of non-empty chunks), and always at least one query: 64 MiB is one query over 2^32 rows.
// A fill launch takes consecutive queries while their entries stay within kRangeMaxEntries, and always at least one query, so its
// output is max(8 MiB, 8 B x the rows of the index) at most.  The sub-batch scratch is the context's (DeviceCtx::d_range) and only
// grows; the fill output lives for the call.
constexpr int kRangeMaxQueries = 1024;
constexpr int64_t kRangeChunkBytes = 64ll << 20;
constexpr int64_t kRangeMaxEntries = 1 << 20;

// where a sub-batch of nq queries keeps what in the scratch: [query data | query uniforms | keys] come from the host in one copy,
// [totals | list lengths] go back in one
struct Layout {
  size_t qdata, qparams, keys, head_bytes, theta, base, totals, n_nonempty, counts, nonempty, bytes;
  Layout(size_t nq, size_t qb, size_t n_chunks) {
    qdata = 0;
    qparams = qdata + nq * qb;
    keys = qparams + nq * sizeof(QueryParams);
    head_bytes = keys + nq * 4;
    theta = align16(head_bytes);
    base = align16(theta + nq * sizeof(Threshold));
    totals = align16(base + nq * 8);
    n_nonempty = totals + nq * 4;
    counts = align16(n_nonempty + nq * 4);
    nonempty = counts + nq * n_chunks * 4;
    bytes = nonempty + nq * n_chunks * 4;
  }
};

// the arguments of both entry points, checked: the handle, the filter's device and every threshold (-> keys)
int check_range_args(const char *who, bbq_index *ix, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                     int32_t sim, const float *thresholds, std::vector<uint32_t> &keys) {
  int rc = validate_query_args(ix, n_queries, qquant, qcorr, query_bits, sim, 0);
  if (rc != BBQ_OK) return rc;
  if (ix->multi) return fail(BBQ_ERR_UNSUPPORTED, "range search is not supported on a multi-device index");
  if (ix->has_pilot || ix->row_base != 0) return fail(BBQ_ERR_UNSUPPORTED, "range search is not supported on a row shard or an index with a pilot replica");
  if (n_queries > 0 && !thresholds) return fail(BBQ_ERR_INVALID_ARG, "%s: thresholds is null", who);
  keys.resize((size_t)n_queries);
  for (int32_t q = 0; q < n_queries; ++q)
    if (bbq_range_key(thresholds[q], &keys[(size_t)q]) != BBQ_OK) return fail(BBQ_ERR_INVALID_ARG, "%s: thresholds[%d] is NaN", who, q);
  return BBQ_OK;
}

// one call under the context's lock
struct RangeRun {
  bbq_index *ix;
  const uint8_t *qquant;
  const double *qcorr;
  const uint32_t *keys;
  int planes, one_bit, sim;
  size_t qb;
  int64_t n_chunks;
  RangeArgs a{};
  std::vector<uint8_t> head;
  int64_t *d_base = nullptr;   // RangeArgs::base of the sub-batch counted last, for the host to fill
  std::vector<uint32_t> back;  // [totals | list lengths] of the sub-batch counted last

  // queries [q0, q0 + nq) counted: the device holds their offsets and lists, `back` their totals and list lengths
  int count(int64_t q0, int nq) {
    const Layout lo((size_t)nq, qb, (size_t)n_chunks);
    uint8_t *d = ix->ctx->d_range;
    hipStream_t st = ix->ctx->aux_stream;
    head.resize(lo.head_bytes);
    for (int s = 0; s < nq; ++s)
      fill_query(ix, head.data() + lo.qdata + (size_t)s * qb, reinterpret_cast<QueryParams *>(head.data() + lo.qparams) + s,
                 qquant + (size_t)(q0 + s) * ix->geom.dim, qcorr + (size_t)(q0 + s) * 4, planes, one_bit, sim);
    memcpy(head.data() + lo.keys, keys + q0, (size_t)nq * 4);
    HIPCHK(hipMemcpyAsync(d, head.data(), lo.head_bytes, hipMemcpyHostToDevice, st));
    a.qplanes = reinterpret_cast<const uint4 *>(d + lo.qdata);
    a.qparams = reinterpret_cast<const QueryParams *>(d + lo.qparams);
    a.theta = reinterpret_cast<const Threshold *>(d + lo.theta);
    a.q_first = 0;
    a.counts = reinterpret_cast<uint32_t *>(d + lo.counts);
    a.chunk_off = a.counts;
    a.nonempty = reinterpret_cast<const uint32_t *>(d + lo.nonempty);
    a.n_nonempty = reinterpret_cast<const uint32_t *>(d + lo.n_nonempty);
    d_base = reinterpret_cast<int64_t *>(d + lo.base);
    a.base = d_base;
    HIPCHK(launch_range_theta(reinterpret_cast<Threshold *>(d + lo.theta), reinterpret_cast<const uint32_t *>(d + lo.keys), a.qparams, nq, st));
    HIPCHK(launch_range_count(a, planes, nq, st));
    HIPCHK(launch_range_offsets(a.counts, reinterpret_cast<uint32_t *>(d + lo.nonempty), reinterpret_cast<uint32_t *>(d + lo.totals),
                                reinterpret_cast<uint32_t *>(d + lo.n_nonempty), (int)n_chunks, nq, st));
    back.resize((size_t)nq * 2);
    HIPCHK(hipMemcpyAsync(back.data(), d + lo.totals, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // the staging vector is free for the next sub-batch
    return BBQ_OK;
  }
};

// the fill launch that starts at query i0 of a sub-batch with these totals: queries [i0, *i1) and their entries
int64_t fill_launch_of(const int64_t *totals, int64_t i0, int64_t nq, int64_t *i1) {
  int64_t i = i0 + 1, cnt = totals[i0];
  while (i < nq && cnt + totals[i] <= kRangeMaxEntries) cnt += totals[i++];
  *i1 = i;
  return cnt;
}

// Both entry points behind their argument checks.  out_counts: the count entry point; otherwise out_offsets and, within cap, the entries.
int range_locked(bbq_index *ix, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                 const uint32_t *keys, int64_t *out_counts, int64_t cap, int64_t *out_offsets, int32_t *out_idx, float *out_score) {
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  // under the lock: the rows the filter was made for are the rows the kernel reads (a compaction on another thread comes before or after)
  const int64_t n = ix->main.view.n_rows;
  if (f && (f->device != ix->device || f->n_rows != n))
    return fail(BBQ_ERR_INVALID_ARG, "the filter was made for an index of %lld rows on device %d, this one has %lld rows on device %d",
                (long long)f->n_rows, f->device, (long long)n, ix->device);
  std::vector<int64_t> totals((size_t)n_queries, 0);
  auto deliver_totals = [&] {
    if (out_counts) {
      for (int32_t q = 0; q < n_queries; ++q) out_counts[q] = totals[(size_t)q];
    } else {
      out_offsets[0] = 0;
      for (int32_t q = 0; q < n_queries; ++q) out_offsets[q + 1] = out_offsets[q] + totals[(size_t)q];
    }
  };
  if (n == 0 || (f && f->count == 0)) {  // nothing to sweep
    deliver_totals();
    return BBQ_OK;
  }

  RangeRun r{ix, qquant, qcorr, keys};
  r.one_bit = query_bits == 1 ? 1 : 0;
  r.sim = sim;
  r.planes = planes_of_call(ix, qquant, (int64_t)n_queries * ix->geom.dim, r.one_bit);
  r.qb = (size_t)query_data_bytes(ix, r.planes);
  r.n_chunks = ix->main.n_chunks();
  r.a.idx = main_launch_view(ix);
  r.a.accept = f ? f->d_bits.get() : nullptr;
  r.a.n_chunks = (int32_t)r.n_chunks;
  const int64_t sub = std::min<int64_t>({(int64_t)n_queries, (int64_t)kRangeMaxQueries, std::max<int64_t>(1, kRangeChunkBytes / (r.n_chunks * 8))});
  const int rc_scratch = reserve_scratch(ix->ctx->d_range, Layout((size_t)sub, r.qb, (size_t)r.n_chunks).bytes, "range search");
  if (rc_scratch != BBQ_OK) return rc_scratch;
  const bool one_sub = sub >= n_queries;
  // every query's total first: the count entry point's answer, and what the caller's cap is held against before anything is filled.  A
  // call of several sub-batches counts each of them again in front of its fill (the scratch holds one sub-batch's offsets)
  for (int64_t q0 = 0; q0 < n_queries; q0 += sub) {
    const int nq = (int)std::min<int64_t>(sub, n_queries - q0);
    const int rc = r.count(q0, nq);
    if (rc != BBQ_OK) return rc;
    for (int s = 0; s < nq; ++s) totals[(size_t)(q0 + s)] = r.back[(size_t)s];
  }
  deliver_totals();
  if (out_counts) return BBQ_OK;
  if (out_offsets[n_queries] > cap)
    return fail(BBQ_ERR_INVALID_ARG, "bbq_search_range_batch: %lld entries, room for %lld", (long long)out_offsets[n_queries], (long long)cap);
  if (out_offsets[n_queries] == 0) return BBQ_OK;

  // the output of the largest fill launch, before the first one writes to the caller's arrays
  int64_t max_entries = 0;
  for (int64_t q0 = 0; q0 < n_queries; q0 += sub) {
    const int64_t nq = std::min<int64_t>(sub, n_queries - q0);
    for (int64_t i0 = 0, i1; i0 < nq; i0 = i1) max_entries = std::max(max_entries, fill_launch_of(totals.data() + q0, i0, nq, &i1));
  }
  DevBuf<uint64_t> d_out;
  {
    const hipError_t e = d_out.alloc((size_t)max_entries);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "range search: %lld entries of output: %s", (long long)max_entries, hipGetErrorString(e)); }
  }
  std::vector<uint64_t> h_ent((size_t)max_entries);
  std::vector<int64_t> base;
  hipStream_t st = ix->ctx->aux_stream;
  r.a.out = d_out;
  for (int64_t q0 = 0; q0 < n_queries; q0 += sub) {
    const int64_t nq = std::min<int64_t>(sub, n_queries - q0);
    if (out_offsets[q0 + nq] == out_offsets[q0]) continue;  // nothing in this sub-batch
    if (!one_sub) {
      const int rc = r.count(q0, (int)nq);
      if (rc != BBQ_OK) return rc;
    }
    const int64_t *tot = totals.data() + q0;
    base.assign((size_t)nq, 0);
    for (int64_t i0 = 0, i1; i0 < nq; i0 = i1) {
      fill_launch_of(tot, i0, nq, &i1);
      for (int64_t i = i0 + 1; i < i1; ++i) base[(size_t)i] = base[(size_t)i - 1] + tot[i - 1];
    }
    HIPCHK(hipMemcpyAsync(r.d_base, base.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
    for (int64_t i0 = 0, i1; i0 < nq; i0 = i1) {
      const int64_t cnt = fill_launch_of(tot, i0, nq, &i1);
      if (cnt == 0) continue;
      int64_t longest = 0;
      for (int64_t i = i0; i < i1; ++i) longest = std::max<int64_t>(longest, r.back[(size_t)(nq + i)]);
      r.a.q_first = (int32_t)i0;
      HIPCHK(launch_range_fill(r.a, r.planes, (int)(i1 - i0), longest, st));
      HIPCHK(hipMemcpyAsync(h_ent.data(), d_out, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));  // also: `base` and the output are free for the next launch
      const int64_t at = out_offsets[q0 + i0];
      unpack_entries(h_ent.data(), cnt, out_idx + at, out_score + at);
    }
  }
  return BBQ_OK;
}

}  // namespace

extern "C" {

int bbq_range_key(float threshold, uint32_t *out_key) {
  clear_error();
  if (!out_key) return fail(BBQ_ERR_INVALID_ARG, "bbq_range_key: out_key is null");
  if (threshold != threshold) return fail(BBQ_ERR_INVALID_ARG, "bbq_range_key: the threshold is NaN");
  if (threshold == 0.0f) threshold = -0.0f;  // +0 and -0 compare equal: both scores pass either threshold
  uint32_t b;
  memcpy(&b, &threshold, 4);
  *out_key = key_of_bits(b) - 1u;  // the key of the largest float below the threshold (of -inf: below every score's key)
  return BBQ_OK;
}

int bbq_count_range_batch(bbq_index *ix, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                          int32_t sim, const float *thresholds, int64_t *out_counts) {
  clear_error();
  std::vector<uint32_t> keys;
  const int rc = check_range_args("bbq_count_range_batch", ix, f, n_queries, qquant, qcorr, query_bits, sim, thresholds, keys);
  if (rc != BBQ_OK) return rc;
  if (n_queries == 0) return BBQ_OK;
  if (!out_counts) return fail(BBQ_ERR_INVALID_ARG, "bbq_count_range_batch: out_counts is null");
  return range_locked(ix, f, n_queries, qquant, qcorr, query_bits, sim, keys.data(), out_counts, 0, nullptr, nullptr, nullptr);
}

int bbq_search_range_batch(bbq_index *ix, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                           int32_t sim, const float *thresholds, int64_t cap, int64_t *out_offsets, int32_t *out_idx, float *out_score) {
  clear_error();
  std::vector<uint32_t> keys;
  const int rc = check_range_args("bbq_search_range_batch", ix, f, n_queries, qquant, qcorr, query_bits, sim, thresholds, keys);
  if (rc != BBQ_OK) return rc;
  if (cap < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_range_batch: cap < 0");
  if (cap > 0 && (!out_idx || !out_score)) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_range_batch: null output");
  if (n_queries == 0) {
    if (out_offsets) out_offsets[0] = 0;
    return BBQ_OK;
  }
  if (!out_offsets) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_range_batch: out_offsets is null");
  return range_locked(ix, f, n_queries, qquant, qcorr, query_bits, sim, keys.data(), nullptr, cap, out_offsets, out_idx, out_score);
}

}  // extern "C"
