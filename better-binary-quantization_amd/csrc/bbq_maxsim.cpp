// bbq_maxsim.cpp - MaxSim search: bbq_search_maxsim_batch, bbq_maxsim_reduce, bbq_maxsim_token_block (kernels: bbq_maxsim_kernels.hip, the
// grouped search's score pass and the span search's select pass).  A query is a run of token vectors and a live group of a group set
// (bbq_group.cpp) scores the ordered f64 sum of its representatives' f32 scores.  A call works through sub-batches
// bounded by scratch, and inside a sub-batch the queries' tokens in blocks of at most kMaxSimTokenBlock - a block's vectors staged in one
// copy (stage_maxsim_token_block, which MaxSim over chosen groups shares), its keys cleared, the score pass (fused where the option and
// the shape allow, the grouped search's kernel with the block's vectors as its queries otherwise) and the accumulate pass - then the
// select pass over the sums, the answer blocks back in one copy, and the end every select-pass search has (finish_selected,
// bbq_select.cpp): the device's k proven, the reference's heap replayed over the other queries' sums.
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include "bbq_search.h"

using namespace bbq;

namespace {

constexpr int kMaxSimMaxQueries = 1024;  // of a sub-batch: 32 768 vectors in a score launch at the most
// maxsim_fused -1: the fused kernel wherever it exists.  At 1 M rows of 768, 1024 and 1536 dimensions (profiles/maxsim_search*.json) the
// slowest of its three runs beat the fastest of the unfused path's by more than that path's spread on every leg: 1.4 to 1.7 times faster
constexpr bool kMaxSimFusedDefault = true;

// where a sub-batch of nq queries whose widest token block has nv vectors keeps what in the scratch: [query data | query uniforms | the
// block's queries | selected queries] come from the host in one copy per block, the answer blocks go back in one; the keys of a block,
// the sums, the scores and the group numbers stay unless a query's heap is replayed
struct Layout {
  size_t qdata, qparams, mq, sel, head_bytes, out, rep, acc, scores, ords, bytes;
  Layout(int nq, int64_t nv, int n_sel, int64_t live, size_t qb, size_t out_stride) {
    qdata = 0;
    qparams = qdata + (size_t)nv * qb;
    mq = qparams + (size_t)nv * sizeof(QueryParams);
    sel = mq + (size_t)nq * sizeof(MaxSimQuery);
    head_bytes = sel + (size_t)n_sel * sizeof(SpanQuery);
    out = align16(head_bytes);
    rep = align16(out + (size_t)n_sel * out_stride * 8);
    acc = rep + (size_t)nv * (size_t)live * 8;
    scores = acc + (size_t)nq * (size_t)live * 8;
    ords = align16(scores + (size_t)nq * (size_t)live * 4);
    bytes = ords + (size_t)nq * (size_t)live * 4;
  }
};
static_assert(sizeof(MaxSimQuery) == 16 && sizeof(SpanQuery) == 32 && sizeof(QueryParams) % 16 == 0, "every staged array starts 8-byte aligned");

// the call behind its argument checks, under the context's lock
int maxsim_locked(bbq_index *ix, const bbq_groups *gs, int32_t n_queries, const int64_t *voff, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                  int32_t sim, int64_t k, int32_t *out_group, float *out_score, int64_t *out_n, uint8_t *out_status) {
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  // under the lock: the rows the check sees are the rows the kernel reads (an append or a compaction on another thread comes before or after)
  if (gs->device != ix->device || gs->n_rows != ix->main.view.n_rows)
    return fail(BBQ_ERR_INVALID_ARG, "bbq_search_maxsim_batch: the group set was made for an index of %lld rows on device %d, this one has %lld rows on device %d",
                (long long)gs->n_rows, gs->device, (long long)ix->main.view.n_rows, ix->device);
  const int64_t L = gs->live;
  if (k > 0 && L > 0 && (!out_group || !out_score)) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_maxsim_batch: null output");
  if (k == 0 || L == 0) {  // nothing to score
    for (int32_t q = 0; q < n_queries; ++q) out_n[q] = 0;
    if (out_status) memset(out_status, 0, (size_t)n_queries);
    return BBQ_OK;
  }

  constexpr int TB = kMaxSimTokenBlock;
  const int64_t n_vectors = voff[n_queries];
  const int one_bit = query_bits == 1 ? 1 : 0;
  const int planes = planes_of_call(ix, qquant, n_vectors * ix->geom.dim, one_bit);
  const size_t qb = (size_t)query_data_bytes(ix, planes);
  const size_t out_stride = (size_t)std::min<int64_t>(k, kSpanSelectMax) + 2;
  const bool sel = k >= 1 && k <= kSpanSelectMax && L > k;  // does the select pass run?  The same for every query of the call
  const bool fused = maxsim_fused_exists(ix->geom, planes) && (ix->opt_maxsim_fused == 1 || (ix->opt_maxsim_fused < 0 && kMaxSimFusedDefault));

  // the plan: sub-batches of equal size, the last one shorter; a query costs the keys of one token block, its sum, its score and its group
  const int64_t budget = (int64_t)ix->opt_group_scratch_mb << 20;
  const int per = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kMaxSimMaxQueries, n_queries), budget / ((8 * TB + 16) * L)));
  int64_t widest = 0;  // vectors of the widest token block of any sub-batch
  for (int64_t q0 = 0; q0 < n_queries; q0 += per) {
    int64_t nv = 0;
    for (int64_t q = q0; q < std::min<int64_t>(q0 + per, n_queries); ++q) nv += std::min<int64_t>(TB, voff[q + 1] - voff[q]);
    widest = std::max(widest, nv);
  }
  const Layout big(per, widest, sel ? per : 0, L, qb, out_stride);
  // everything large, before anything is written to the caller's arrays
  const int rc_scratch = reserve_scratch(ix->ctx->d_span, big.bytes, "MaxSim search");
  if (rc_scratch != BBQ_OK) return rc_scratch;
  const size_t back_words = sel ? (size_t)per * out_stride : 0;
  const size_t host_rows = (size_t)per * (size_t)L;
  std::unique_ptr<uint8_t[]> head(new (std::nothrow) uint8_t[std::max<size_t>(big.head_bytes, 1)]);
  std::unique_ptr<uint64_t[]> back(new (std::nothrow) uint64_t[std::max<size_t>(back_words, 1)]);
  std::unique_ptr<float[]> h_scores(new (std::nothrow) float[host_rows]);      // touched only where a heap is replayed
  std::unique_ptr<uint32_t[]> h_ords(new (std::nothrow) uint32_t[host_rows]);  // the same
  if (!head || !back || !h_scores || !h_ords)
    return fail(BBQ_ERR_OOM, "MaxSim search: host staging for %zu + %zu + %zu bytes", big.head_bytes, back_words * 8, host_rows * 8);

  uint8_t *d = ix->ctx->d_span;
  hipStream_t st = ix->ctx->aux_stream;
  MaxSimScoreArgs ma{};
  GroupScoreArgs &ga = ma.g;
  ga = group_score_args(ix, gs);
  const MaxSimTokens tk{voff, qquant, qcorr, planes, one_bit, sim};
  std::vector<SelectQuery> sq((size_t)per);  // every query of a sub-batch: L sums from s * L on, and block s where the select pass runs
  SelectTail t{};
  t.back = back.get();
  t.h_scores = h_scores.get();
  t.h_ords = h_ords.get();
  t.k = k;
  t.out_stride = out_stride;
  t.stream = st;
  t.threads = ix->opt_replay_threads;

  for (int64_t q0 = 0; q0 < n_queries; q0 += per) {
    const int nq = (int)std::min<int64_t>(per, n_queries - q0);
    int64_t nv = 0, longest = 0;
    for (int s = 0; s < nq; ++s) {
      nv += std::min<int64_t>(TB, voff[q0 + s + 1] - voff[q0 + s]);
      longest = std::max(longest, voff[q0 + s + 1] - voff[q0 + s]);
    }
    const Layout lo(nq, nv, sel ? nq : 0, L, qb, out_stride);  // nv: the sub-batch's first block is its widest
    float *d_scores = reinterpret_cast<float *>(d + lo.scores);
    uint32_t *d_ords = reinterpret_cast<uint32_t *>(d + lo.ords);
    SpanQuery *h_sel = reinterpret_cast<SpanQuery *>(head.get() + lo.sel);
    for (int s = 0; sel && s < nq; ++s) h_sel[s] = SpanQuery{(int64_t)s * L, L, 0, 0, 0};

    for (int64_t t0 = 0; t0 < longest; t0 += TB) {  // the token block [t0, t0 + TB) of every query that has one
      int n_mq = 0;
      const int32_t v = stage_maxsim_token_block(ix, tk, q0, nq, t0, [](int) { return true; }, head.get() + lo.qdata, qb,
                                                 reinterpret_cast<QueryParams *>(head.get() + lo.qparams), reinterpret_cast<MaxSimQuery *>(head.get() + lo.mq), &n_mq);
      HIPCHK(hipMemcpyAsync(d, head.get(), lo.head_bytes, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(d + lo.rep, 0, (size_t)v * (size_t)L * 8, st));
      ga.qplanes = reinterpret_cast<const uint4 *>(d + lo.qdata);
      ga.qparams = reinterpret_cast<const QueryParams *>(d + lo.qparams);
      ga.rep = reinterpret_cast<unsigned long long *>(d + lo.rep);
      ma.queries = reinterpret_cast<const MaxSimQuery *>(d + lo.mq);
      if (fused) {
        ga.n_queries = n_mq;
        HIPCHK(launch_maxsim_score(ma, planes, st));
      } else {
        ga.n_queries = v;  // every token vector of the block is a query of the grouped search's score pass
        HIPCHK(launch_group_score(ga, planes, st));
      }
      MaxSimAccArgs aa{};
      aa.rep = ga.rep;
      aa.queries = ma.queries;
      aa.acc = reinterpret_cast<double *>(d + lo.acc);
      aa.scores = d_scores;
      aa.ords = d_ords;
      aa.live_group = gs->d_live_group.get();
      aa.live = L;
      HIPCHK(launch_maxsim_accumulate(aa, n_mq, st));
      if (t0 + TB < longest) HIPCHK(hipStreamSynchronize(st));  // the staging is free for the next block
    }
    if (sel) {
      SpanSelectArgs se{};
      se.scores = d_scores;
      se.sel = reinterpret_cast<const SpanQuery *>(d + lo.sel);
      se.runs = nullptr;
      se.ords = d_ords;
      se.out = reinterpret_cast<uint64_t *>(d + lo.out);
      se.k = (int32_t)k;
      se.out_stride = (int32_t)out_stride;
      HIPCHK(launch_span_select(se, nq, st));
      HIPCHK(hipMemcpyAsync(back.get(), d + lo.out, (size_t)nq * out_stride * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // also: the staging is free for the next sub-batch

    for (int s = 0; s < nq; ++s) sq[(size_t)s] = SelectQuery{L, (int64_t)s * L, sel ? s : -1};
    t.queries = sq.data();
    t.nq = nq;
    t.d_scores = d_scores;
    t.d_ords = d_ords;
    t.out_tag = out_group + q0 * k;
    t.out_score = out_score + q0 * k;
    t.out_n = out_n + q0;
    t.out_status = out_status ? out_status + q0 : nullptr;
    const int rc = finish_selected(t);  // the sums of a replayed query over the live groups in ascending group number
    if (rc != BBQ_OK) return rc;
  }
  return BBQ_OK;
}

}  // namespace

int32_t bbq::stage_maxsim_token_block(const bbq_index *ix, const MaxSimTokens &tk, int64_t q0, int nq, int64_t t0, const std::function<bool(int)> &takes_part,
                                      uint8_t *h_qdata, size_t qb, QueryParams *h_qparams, MaxSimQuery *h_mq, int *n_mq) {
  int32_t v = 0;  // vectors staged so far
  *n_mq = 0;
  for (int s = 0; s < nq; ++s) {
    const int64_t first = tk.voff[q0 + s], T = tk.voff[q0 + s + 1] - first;
    if (T <= t0 || !takes_part(s)) continue;
    const int n_tok = (int)std::min<int64_t>(kMaxSimTokenBlock, T - t0);
    h_mq[(*n_mq)++] = MaxSimQuery{v, n_tok, s, (t0 == 0 ? kMaxSimFirst : 0) | (t0 + n_tok == T ? kMaxSimLast : 0)};
    for (int t = 0; t < n_tok; ++t, ++v) {
      const int64_t vec = first + t0 + t;
      fill_query(ix, h_qdata + (size_t)v * qb, h_qparams + v, tk.qquant + (size_t)vec * ix->geom.dim, tk.qcorr + (size_t)vec * 4, tk.planes, tk.one_bit, tk.sim);
    }
  }
  return v;
}

extern "C" {

int32_t bbq_maxsim_token_block(void) { return kMaxSimTokenBlock; }

int bbq_maxsim_reduce(const float *rep_scores, int64_t n_vectors, int64_t n_groups, float *out) {
  clear_error();
  if (n_vectors < 1 || n_groups < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_maxsim_reduce: at least one vector, no negative group count");
  if (n_groups > 0 && (!rep_scores || !out)) return fail(BBQ_ERR_INVALID_ARG, "bbq_maxsim_reduce: null argument");
  for (int64_t s = 0; s < n_groups; ++s) {
    double acc = (double)rep_scores[s];  // from m_0, not from 0.0
    for (int64_t t = 1; t < n_vectors; ++t) acc = acc + (double)rep_scores[t * n_groups + s];
    out[s] = (float)acc;
  }
  return BBQ_OK;
}

int bbq_search_maxsim_batch(bbq_index *ix, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets, const uint8_t *qquant, const double *qcorr,
                            int32_t query_bits, int32_t sim, int64_t k, int32_t *out_group, float *out_score, int64_t *out_n, uint8_t *out_status) {
  clear_error();
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  if (n_queries < 0) return fail(BBQ_ERR_INVALID_ARG, "n_queries < 0");
  const int rcv = check_maxsim_vec_offsets("bbq_search_maxsim_batch", n_queries, vec_offsets);
  if (rcv != BBQ_OK) return rcv;
  const int32_t n_vectors = n_queries > 0 ? (int32_t)vec_offsets[n_queries] : 0;
  const int rc = validate_query_args(ix, n_vectors, qquant, qcorr, query_bits, sim, k);
  if (rc != BBQ_OK) return rc;
  const int rc2 = check_group_index(ix);
  if (rc2 != BBQ_OK) return rc2;
  if (!g) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_maxsim_batch: the group set is null");
  if (n_queries == 0) return BBQ_OK;
  if (!out_n) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_maxsim_batch: out_n is null");
  return maxsim_locked(ix, g, n_queries, vec_offsets, qquant, qcorr, query_bits, sim, k, out_group, out_score, out_n, out_status);
}

}  // extern "C"
