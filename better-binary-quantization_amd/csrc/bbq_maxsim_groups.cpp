// bbq_maxsim_groups.cpp - MaxSim over chosen groups: bbq_score_maxsim_groups_batch, bbq_search_maxsim_groups_batch (kernels:
// bbq_maxsim_cand_kernels.hip and the MaxSim search's accumulate pass).  A query is a run of token vectors and a list of candidate
// groups of a group set, in the caller's order, duplicates included; every list entry scores the MaxSim sum bbq_search_maxsim_batch
// defines for its group.  The host checks every list - a group number out of range or a group that is not live - under the context's
// lock before the first launch, stages ONE record per candidate (the group's first row and its position among the query's expanded
// rows) and never a row list, and works through sub-batches bounded by scratch, and inside a sub-batch the queries' tokens in blocks of at
// most kMaxSimTokenBlock - a block's vectors (the MaxSim search's stage_maxsim_token_block, bbq_maxsim.cpp) and the records staged in one
// copy, its keys cleared, the score pass and the accumulate pass - then the f32 sums back in one copy.  The search call replays the
// reference's heap over the sums in list order (replay_lists, bbq_replay.cpp), as bbq_search_ords_batch does over its scores.
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include "bbq_search.h"

using namespace bbq;

namespace {

constexpr int kCandMaxQueries = 1024;  // of a sub-batch

// where a sub-batch of nq queries with n_rec records whose widest token block has nv vectors keeps what in the scratch: [query data |
// query uniforms | the block's queries | the queries' lists | records] come from the host in one copy per block; the keys of a block
// and the sums stay on the device, the scores go back in one copy.  E: entries per query = the longest list of the sub-batch
struct Layout {
  size_t qdata, qparams, mq, cq, recs, head_bytes, rep, acc, scores, bytes;
  Layout(int nq, int64_t nv, int64_t n_rec, int64_t E, size_t qb) {
    qdata = 0;
    qparams = qdata + (size_t)nv * qb;
    mq = qparams + (size_t)nv * sizeof(QueryParams);
    cq = mq + (size_t)nq * sizeof(MaxSimQuery);
    recs = cq + (size_t)nq * sizeof(MaxSimCandQuery);
    head_bytes = recs + (size_t)n_rec * sizeof(MaxSimCand);
    rep = align16(head_bytes);
    acc = rep + (size_t)nv * (size_t)E * 8;
    scores = acc + (size_t)nq * (size_t)E * 8;
    bytes = scores + (size_t)nq * (size_t)E * 4;
  }
};
static_assert(sizeof(MaxSimQuery) == 16 && sizeof(MaxSimCandQuery) == 16 && sizeof(MaxSimCand) == 8 && sizeof(QueryParams) % 16 == 0, "every staged array starts 8-byte aligned");

// the call behind its argument checks, under the context's lock.  out == null: the lists are checked and nothing is launched
int score_locked(const char *fn, bbq_index *ix, const bbq_groups *gs, int32_t n_queries, const int64_t *voff, const uint8_t *qquant, const double *qcorr,
                 int32_t query_bits, int32_t sim, const int64_t *coff, const int32_t *cand, float *out) {
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  // under the lock: the rows the check sees are the rows the kernel reads (an append or a compaction on another thread comes before or after)
  if (gs->device != ix->device || gs->n_rows != ix->main.view.n_rows)
    return fail(BBQ_ERR_INVALID_ARG, "%s: the group set was made for an index of %lld rows on device %d, this one has %lld rows on device %d", fn,
                (long long)gs->n_rows, gs->device, (long long)ix->main.view.n_rows, ix->device);
  // every list, in call order, before anything is launched or written
  int64_t longest_list = 0;
  const int rc = check_maxsim_cand_lists(fn, gs, n_queries, coff, cand, &longest_list);
  if (rc != BBQ_OK) return rc;
  if (!out) return BBQ_OK;

  constexpr int TB = kMaxSimTokenBlock;
  const int64_t n_vectors = voff[n_queries];
  const int one_bit = query_bits == 1 ? 1 : 0;
  const int planes = planes_of_call(ix, qquant, n_vectors * ix->geom.dim, one_bit);
  const size_t qb = (size_t)query_data_bytes(ix, planes);

  // the plan: sub-batches of equal size, the last one shorter; a query costs the keys of one token block, its sum and its score per
  // entry, and every query of the call is given the entries of the longest list
  const int64_t budget = (int64_t)ix->opt_group_scratch_mb << 20;
  const int per = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kCandMaxQueries, n_queries), budget / ((8 * TB + 12) * longest_list)));
  int64_t widest = 0, most_rec = 0;  // vectors of the widest token block, and records, of any sub-batch
  for (int64_t q0 = 0; q0 < n_queries; q0 += per) {
    const int64_t q1 = std::min<int64_t>(q0 + per, n_queries);
    int64_t nv = 0;
    for (int64_t q = q0; q < q1; ++q) nv += std::min<int64_t>(TB, voff[q + 1] - voff[q]);
    widest = std::max(widest, nv);
    most_rec = std::max(most_rec, coff[q1] - coff[q0] + (q1 - q0));
  }
  const Layout big(per, widest, most_rec, longest_list, qb);
  // everything large, before anything is written to the caller's array
  const int rc_scratch = reserve_scratch(ix->ctx->d_span, big.bytes, "MaxSim over chosen groups");
  if (rc_scratch != BBQ_OK) return rc_scratch;
  const size_t host_scores = (size_t)per * (size_t)longest_list;
  std::unique_ptr<uint8_t[]> head(new (std::nothrow) uint8_t[std::max<size_t>(big.head_bytes, 1)]);
  std::unique_ptr<float[]> h_scores(new (std::nothrow) float[host_scores]);
  if (!head || !h_scores) return fail(BBQ_ERR_OOM, "MaxSim over chosen groups: host staging for %zu + %zu bytes", big.head_bytes, host_scores * 4);

  uint8_t *d = ix->ctx->d_span;
  hipStream_t st = ix->ctx->aux_stream;
  MaxSimCandArgs ca{};
  ca.idx = main_launch_view(ix);
  ca.accept = gs->filtered ? gs->d_words.get() + tiles_of(gs->n_rows) + 1 : nullptr;
  const MaxSimTokens tk{voff, qquant, qcorr, planes, one_bit, sim};

  for (int64_t q0 = 0; q0 < n_queries; q0 += per) {
    const int nq = (int)std::min<int64_t>(per, n_queries - q0);
    int64_t nv = 0, longest_tok = 0, E = 0, longest_rows = 0;
    for (int s = 0; s < nq; ++s) {
      nv += std::min<int64_t>(TB, voff[q0 + s + 1] - voff[q0 + s]);
      longest_tok = std::max(longest_tok, voff[q0 + s + 1] - voff[q0 + s]);
      E = std::max(E, coff[q0 + s + 1] - coff[q0 + s]);
    }
    if (E == 0) continue;  // every list of the sub-batch is empty
    const int64_t n_rec = coff[q0 + nq] - coff[q0] + nq;
    const Layout lo(nq, nv, n_rec, E, qb);  // nv: the sub-batch's first block is its widest
    // the lists, once per sub-batch: a record per candidate and a terminator per query
    MaxSimCandQuery *h_cq = reinterpret_cast<MaxSimCandQuery *>(head.get() + lo.cq);
    MaxSimCand *h_rec = reinterpret_cast<MaxSimCand *>(head.get() + lo.recs);
    longest_rows = stage_maxsim_cand_records(gs, nq, coff + q0, cand, h_cq, h_rec);
    float *d_scores = reinterpret_cast<float *>(d + lo.scores);

    for (int64_t t0 = 0; t0 < longest_tok; t0 += TB) {  // the token block [t0, t0 + TB) of every query that has one and a candidate
      int n_mq = 0;
      const int32_t v = stage_maxsim_token_block(ix, tk, q0, nq, t0, [&](int s) { return h_cq[s].n_cand != 0; }, head.get() + lo.qdata, qb,
                                                 reinterpret_cast<QueryParams *>(head.get() + lo.qparams), reinterpret_cast<MaxSimQuery *>(head.get() + lo.mq), &n_mq);
      HIPCHK(hipMemcpyAsync(d, head.get(), lo.head_bytes, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(d + lo.rep, 0, (size_t)v * (size_t)E * 8, st));
      ca.qplanes = reinterpret_cast<const uint4 *>(d + lo.qdata);
      ca.qparams = reinterpret_cast<const QueryParams *>(d + lo.qparams);
      ca.queries = reinterpret_cast<const MaxSimQuery *>(d + lo.mq);
      ca.cq = reinterpret_cast<const MaxSimCandQuery *>(d + lo.cq);
      ca.recs = reinterpret_cast<const MaxSimCand *>(d + lo.recs);
      ca.rep = reinterpret_cast<unsigned long long *>(d + lo.rep);
      ca.stride = E;
      HIPCHK(launch_maxsim_cand_score(ca, planes, n_mq, longest_rows, st));
      MaxSimAccArgs aa{};
      aa.rep = ca.rep;
      aa.queries = ca.queries;
      aa.acc = reinterpret_cast<double *>(d + lo.acc);
      aa.scores = d_scores;
      aa.live = E;  // no ords: an entry is a position of the caller's list
      HIPCHK(launch_maxsim_accumulate(aa, n_mq, st));
      if (t0 + TB < longest_tok) HIPCHK(hipStreamSynchronize(st));  // the staging is free for the next block
    }
    HIPCHK(hipMemcpyAsync(h_scores.get(), d_scores, (size_t)nq * (size_t)E * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // also: the staging is free for the next sub-batch
    for (int s = 0; s < nq; ++s) {
      const int64_t beg = coff[q0 + s], n = coff[q0 + s + 1] - beg;
      if (n > 0) memcpy(out + beg, h_scores.get() + (size_t)s * (size_t)E, (size_t)n * 4);
    }
  }
  return BBQ_OK;
}

// the checks both calls share, in the MaxSim search's order and wording; *total = cand_offsets[n_queries].  *done: the call is answered
int check_call(const char *fn, bbq_index *ix, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets, const uint8_t *qquant, const double *qcorr,
               int32_t query_bits, int32_t sim, int64_t k, const int64_t *cand_offsets, int64_t *total, bool *done) {
  *done = false;
  *total = 0;
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  if (n_queries < 0) return fail(BBQ_ERR_INVALID_ARG, "n_queries < 0");
  const int rcv = check_maxsim_vec_offsets(fn, n_queries, vec_offsets);
  if (rcv != BBQ_OK) return rcv;
  const int32_t n_vectors = n_queries > 0 ? (int32_t)vec_offsets[n_queries] : 0;
  const int rc = validate_query_args(ix, n_vectors, qquant, qcorr, query_bits, sim, k);
  if (rc != BBQ_OK) return rc;
  const int rc2 = check_group_index(ix);
  if (rc2 != BBQ_OK) return rc2;
  if (!g) return fail(BBQ_ERR_INVALID_ARG, "%s: the group set is null", fn);
  if (n_queries == 0) {
    *done = true;
    return BBQ_OK;
  }
  const int rc3 = check_maxsim_cand_offsets(fn, n_queries, cand_offsets);
  if (rc3 != BBQ_OK) return rc3;
  *total = cand_offsets[n_queries];
  return BBQ_OK;
}

}  // namespace

// ---- what the exact MaxSim rerank (bbq_maxsim_rerank.cpp) shares with the calls of this file

int bbq::check_maxsim_vec_offsets(const char *fn, int32_t n_queries, const int64_t *vec_offsets) {
  if (n_queries > 0) {
    if (!vec_offsets) return fail(BBQ_ERR_INVALID_ARG, "%s: vec_offsets is null", fn);
    if (vec_offsets[0] != 0) return fail(BBQ_ERR_INVALID_ARG, "%s: vec_offsets[0] must be 0 (query 0)", fn);
    for (int32_t q = 0; q < n_queries; ++q)
      if (vec_offsets[q + 1] <= vec_offsets[q])
        return fail(BBQ_ERR_INVALID_ARG, "%s: query %d has no token vector or vec_offsets descends: [%lld, %lld)", fn, q, (long long)vec_offsets[q],
                    (long long)vec_offsets[q + 1]);
    if (vec_offsets[n_queries] > 0x7fffffffll) return fail(BBQ_ERR_INVALID_ARG, "%s: more than 2^31 - 1 token vectors", fn);
  }
  return BBQ_OK;
}

int bbq::check_maxsim_cand_offsets(const char *fn, int32_t n_queries, const int64_t *cand_offsets) {
  if (!cand_offsets) return fail(BBQ_ERR_INVALID_ARG, "%s: cand_offsets is null", fn);
  if (cand_offsets[0] != 0) return fail(BBQ_ERR_INVALID_ARG, "%s: cand_offsets[0] must be 0 (query 0)", fn);
  for (int32_t q = 0; q < n_queries; ++q)
    if (cand_offsets[q + 1] < cand_offsets[q])
      return fail(BBQ_ERR_INVALID_ARG, "%s: cand_offsets descends at query %d: [%lld, %lld)", fn, q, (long long)cand_offsets[q], (long long)cand_offsets[q + 1]);
  return BBQ_OK;
}

int bbq::check_maxsim_cand_lists(const char *fn, const bbq_groups *gs, int32_t n_queries, const int64_t *coff, const int32_t *cand, int64_t *longest) {
  int64_t longest_list = 0;
  for (int32_t q = 0; q < n_queries; ++q) {
    int64_t rows = 0;
    for (int64_t i = coff[q]; i < coff[q + 1]; ++i) {
      const int32_t g = cand[i];
      if (g < 0 || g >= gs->n_groups)
        return fail(BBQ_ERR_INVALID_ARG, "%s: query %d, position %lld: group %d is not a group of the set (%lld groups)", fn, q, (long long)(i - coff[q]), g,
                    (long long)gs->n_groups);
      if (gs->slot[(size_t)g] < 0)
        return fail(BBQ_ERR_INVALID_ARG, "%s: query %d, position %lld: group %d is not live (it is empty or its rows are all filtered out)", fn, q,
                    (long long)(i - coff[q]), g);
      rows += gs->offsets[(size_t)g + 1] - gs->offsets[(size_t)g];
    }
    if (rows > kMaxSimCandMaxRows)
      return fail(BBQ_ERR_INVALID_ARG, "%s: query %d: its candidates hold %lld rows, more than %lld", fn, q, (long long)rows, (long long)kMaxSimCandMaxRows);
    longest_list = std::max(longest_list, coff[q + 1] - coff[q]);
  }
  *longest = longest_list;
  return BBQ_OK;
}

int64_t bbq::stage_maxsim_cand_records(const bbq_groups *gs, int nq, const int64_t *coff, const int32_t *cand, MaxSimCandQuery *h_cq, MaxSimCand *h_rec) {
  int64_t longest_rows = 0, at = 0;
  for (int s = 0; s < nq; ++s) {
    const int64_t beg = coff[s], n = coff[s + 1] - beg;
    int64_t pos = 0;
    h_cq[s].rec_first = at;
    for (int64_t i = 0; i < n; ++i) {
      const size_t g = (size_t)cand[beg + i];
      h_rec[at++] = MaxSimCand{(uint32_t)gs->offsets[g], (uint32_t)pos};
      pos += gs->offsets[g + 1] - gs->offsets[g];
    }
    h_rec[at++] = MaxSimCand{0u, (uint32_t)pos};
    h_cq[s].n_cand = (int32_t)n;
    h_cq[s].total = (int32_t)pos;
    longest_rows = std::max(longest_rows, pos);
  }
  return longest_rows;
}

extern "C" {

int bbq_score_maxsim_groups_batch(bbq_index *ix, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets, const uint8_t *qquant, const double *qcorr,
                                  int32_t query_bits, int32_t sim, const int64_t *cand_offsets, const int32_t *cand_groups, float *out_score) {
  static const char fn[] = "bbq_score_maxsim_groups_batch";
  clear_error();
  int64_t total = 0;
  bool done = false;
  const int rc = check_call(fn, ix, g, n_queries, vec_offsets, qquant, qcorr, query_bits, sim, 0, cand_offsets, &total, &done);
  if (rc != BBQ_OK || done || total == 0) return rc;
  if (!cand_groups) return fail(BBQ_ERR_INVALID_ARG, "%s: cand_groups is null", fn);
  if (!out_score) return fail(BBQ_ERR_INVALID_ARG, "%s: null output", fn);
  return score_locked(fn, ix, g, n_queries, vec_offsets, qquant, qcorr, query_bits, sim, cand_offsets, cand_groups, out_score);
}

int bbq_search_maxsim_groups_batch(bbq_index *ix, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets, const uint8_t *qquant, const double *qcorr,
                                   int32_t query_bits, int32_t sim, int64_t k, const int64_t *cand_offsets, const int32_t *cand_groups, int32_t *out_group,
                                   float *out_score, int64_t *out_n) {
  static const char fn[] = "bbq_search_maxsim_groups_batch";
  clear_error();
  int64_t total = 0;
  bool done = false;
  int rc = check_call(fn, ix, g, n_queries, vec_offsets, qquant, qcorr, query_bits, sim, k, cand_offsets, &total, &done);
  if (rc != BBQ_OK || done) return rc;
  if (!out_n) return fail(BBQ_ERR_INVALID_ARG, "%s: out_n is null", fn);
  if (total > 0 && !cand_groups) return fail(BBQ_ERR_INVALID_ARG, "%s: cand_groups is null", fn);
  if (total > 0 && k > 0 && (!out_group || !out_score)) return fail(BBQ_ERR_INVALID_ARG, "%s: null output", fn);
  std::unique_ptr<float[]> s32(new (std::nothrow) float[(size_t)std::max<int64_t>(total, 1)]);
  if (!s32) return fail(BBQ_ERR_OOM, "%s: host staging for %lld scores", fn, (long long)total);
  if (total > 0) {  // also for k == 0: a candidate that names no live group is an error whatever k is
    rc = score_locked(fn, ix, g, n_queries, vec_offsets, qquant, qcorr, query_bits, sim, cand_offsets, cand_groups, k > 0 ? s32.get() : nullptr);
    if (rc != BBQ_OK) return rc;
  }
  replay_lists(n_queries, cand_offsets, cand_groups, s32.get(), k, ix->opt_replay_threads, out_group, out_score, out_n);  // in the order given
  return BBQ_OK;
}

}  // extern "C"
