// bbq_maxsim_rerank.cpp - exact MaxSim rerank: bbq_maxsim_reduce_true, bbq_rerank_maxsim_groups_batch, bbq_search_maxsim_rerank_batch
// (kernels: bbq_maxsim_rerank_kernels.hip).  A query is a run of RAW fp32 token vectors and a list of candidate groups of a group set;
// every list entry scores T = M_0 + M_1 + ..., M_t the greatest computeSimilarity of token t against the group's accepted fp32 rows,
// which stay resident in HBM (bbq_vectors).  The lists are checked and staged by the functions MaxSim over chosen groups uses
// (bbq_maxsim_groups.cpp): one 8-byte record per candidate goes to the device, never a row list, and one f64 per candidate comes back.
// The host path has that file's shape: sub-batches bounded by scratch, inside a sub-batch the queries' tokens in blocks of at most
// kMaxSimTokenBlock - a block's token vectors and the records staged in one copy, its keys cleared, the score pass and the accumulate
// pass.  The recipe call composes the MaxSim search, this rerank and the two selectors of bbq_search_rerank_batch (bbq_rerank.cpp).
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include "bbq_search.h"

using namespace bbq;

namespace {

constexpr int kRerankMaxQueries = 1024;  // of a sub-batch
constexpr int TB = kMaxSimTokenBlock;
constexpr int TG = kMaxSimRerankTokenGroup;

inline int64_t slots_of(int64_t n_tok) { return (n_tok + TG - 1) / TG * TG; }  // of one query's token block

// where a sub-batch of nq queries with n_rec records whose widest token block has nv vector slots keeps what in the scratch: [the block's
// queries | the queries' lists | records | squared norms | token vectors] come from the host in one copy per block; the keys of a block
// and the sums stay on the device, the sums go back in one copy.  E: entries per query = the longest list of the sub-batch
struct Layout {
  size_t mq, cq, recs, na, tokens, head_bytes, rep, acc, bytes;
  Layout(int nq, int64_t nv, int64_t n_rec, int64_t E, int32_t dim) {
    mq = 0;
    cq = mq + (size_t)nq * sizeof(MaxSimQuery);
    recs = cq + (size_t)nq * sizeof(MaxSimCandQuery);
    na = recs + (size_t)n_rec * sizeof(MaxSimCand);
    tokens = align16(na + (size_t)nv * 8);  // the kernel copies them 16 bytes at a time
    head_bytes = tokens + (size_t)nv * (size_t)dim * 8;
    rep = align16(head_bytes);
    acc = rep + (size_t)nv * (size_t)E * 8;
    bytes = acc + (size_t)nq * (size_t)E * 8;
  }
};
static_assert(sizeof(MaxSimQuery) == 16 && sizeof(MaxSimCandQuery) == 16 && sizeof(MaxSimCand) == 8, "every staged array starts 8-byte aligned");

}  // namespace

int bbq::rerank_maxsim_groups(const char *fn, bbq_vectors *v, const bbq_groups *gs, int32_t n_queries, const int64_t *voff, const float *queries,
                              int32_t true_sim, const int64_t *coff, const int32_t *cand, double *out, int scratch_mb) {
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  HIPCHK(hipSetDevice(v->device));
  // under the lock: the rows the check sees are the rows the kernel reads (an append or a compaction on another thread comes before or after)
  if (gs->device != v->device || gs->n_rows != v->n)
    return fail(BBQ_ERR_INVALID_ARG, "%s: the group set was made for %lld rows on device %d, the vectors are %lld rows on device %d", fn, (long long)gs->n_rows,
                gs->device, (long long)v->n, v->device);
  int64_t longest_list = 0;
  const int rc = check_maxsim_cand_lists(fn, gs, n_queries, coff, cand, &longest_list);
  if (rc != BBQ_OK) return rc;
  if (longest_list == 0) return BBQ_OK;

  const int32_t dim = v->dim;
  // the plan: sub-batches of equal size, the last one shorter; a query costs the keys of one token block and its sum per entry - every
  // query of the call is given the entries of the longest list - and the f64 image of one token block
  const int64_t budget = (int64_t)scratch_mb << 20;
  const int64_t per_query = (8 * TB + 8) * longest_list + (int64_t)TB * 8 * ((int64_t)dim + 1);
  const int per = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kRerankMaxQueries, n_queries), budget / per_query));
  int64_t widest = 0, most_rec = 0;  // vector slots of the widest token block, and records, of any sub-batch
  for (int64_t q0 = 0; q0 < n_queries; q0 += per) {
    const int64_t q1 = std::min<int64_t>(q0 + per, n_queries);
    int64_t nv = 0;
    for (int64_t q = q0; q < q1; ++q) nv += slots_of(std::min<int64_t>(TB, voff[q + 1] - voff[q]));
    widest = std::max(widest, nv);
    most_rec = std::max(most_rec, coff[q1] - coff[q0] + (q1 - q0));
  }
  const Layout big(per, widest, most_rec, longest_list, dim);
  // everything large, before anything is written to the caller's array
  const int rc_scratch = reserve_scratch(v->ctx->d_span, big.bytes, "exact MaxSim rerank");
  if (rc_scratch != BBQ_OK) return rc_scratch;
  const size_t host_sums = (size_t)per * (size_t)longest_list;
  std::unique_ptr<uint8_t[]> head(new (std::nothrow) uint8_t[std::max<size_t>(big.head_bytes, 1)]);
  std::unique_ptr<double[]> h_sums(new (std::nothrow) double[host_sums]);
  if (!head || !h_sums) return fail(BBQ_ERR_OOM, "exact MaxSim rerank: host staging for %zu + %zu bytes", big.head_bytes, host_sums * 8);

  uint8_t *d = v->ctx->d_span;
  hipStream_t st = v->ctx->aux_stream;
  MaxSimRerankArgs ra{};
  ra.vecs = v->d;
  ra.dim = dim;
  ra.sim = true_sim;
  ra.accept = gs->filtered ? gs->d_words.get() + tiles_of(gs->n_rows) + 1 : nullptr;

  for (int64_t q0 = 0; q0 < n_queries; q0 += per) {
    const int nq = (int)std::min<int64_t>(per, n_queries - q0);
    int64_t nv = 0, longest_tok = 0, E = 0;
    for (int s = 0; s < nq; ++s) {
      nv += slots_of(std::min<int64_t>(TB, voff[q0 + s + 1] - voff[q0 + s]));
      longest_tok = std::max(longest_tok, voff[q0 + s + 1] - voff[q0 + s]);
      E = std::max(E, coff[q0 + s + 1] - coff[q0 + s]);
    }
    if (E == 0) continue;  // every list of the sub-batch is empty
    const int64_t n_rec = coff[q0 + nq] - coff[q0] + nq;
    const Layout lo(nq, nv, n_rec, E, dim);  // nv: the sub-batch's first block is its widest
    // the lists, once per sub-batch: a record per candidate and a terminator per query
    MaxSimCandQuery *h_cq = reinterpret_cast<MaxSimCandQuery *>(head.get() + lo.cq);
    MaxSimCand *h_rec = reinterpret_cast<MaxSimCand *>(head.get() + lo.recs);
    const int64_t longest_rows = stage_maxsim_cand_records(gs, nq, coff + q0, cand, h_cq, h_rec);
    double *d_acc = reinterpret_cast<double *>(d + lo.acc);

    for (int64_t t0 = 0; t0 < longest_tok; t0 += TB) {  // the token block [t0, t0 + TB) of every query that has one and a candidate
      MaxSimQuery *h_mq = reinterpret_cast<MaxSimQuery *>(head.get() + lo.mq);
      double *h_na = reinterpret_cast<double *>(head.get() + lo.na);
      double *h_tok = reinterpret_cast<double *>(head.get() + lo.tokens);
      int n_mq = 0;
      int32_t slot = 0;  // vector slots staged so far
      for (int s = 0; s < nq; ++s) {
        const int64_t first = voff[q0 + s], T = voff[q0 + s + 1] - first;
        if (T <= t0 || h_cq[s].n_cand == 0) continue;
        const int n_tok = (int)std::min<int64_t>(TB, T - t0);
        const int tp = (int)slots_of(n_tok);
        h_mq[n_mq++] = MaxSimQuery{slot, n_tok, s, (t0 == 0 ? kMaxSimFirst : 0) | (t0 + n_tok == T ? kMaxSimLast : 0)};
        // column j's tokens side by side, widened (exactly) to f64, the padding slots 0.0; and each token's squared norm, the
        // reference's na chain: na += a * a in index order, the product exact in f64
        double *dst = h_tok + (size_t)slot * (size_t)dim;
        for (int t = 0; t < tp; ++t) {
          if (t >= n_tok) {
            for (int32_t j = 0; j < dim; ++j) dst[(size_t)j * tp + t] = 0.0;
            h_na[slot + t] = 0.0;
            continue;
          }
          const float *src = queries + (size_t)(first + t0 + t) * (size_t)dim;
          double na = 0.0;
          for (int32_t j = 0; j < dim; ++j) {
            const double a = (double)src[j];
            dst[(size_t)j * tp + t] = a;
            na += a * a;
          }
          h_na[slot + t] = na;
        }
        slot += tp;
      }
      HIPCHK(hipMemcpyAsync(d, head.get(), lo.tokens + (size_t)slot * (size_t)dim * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemsetAsync(d + lo.rep, 0, (size_t)slot * (size_t)E * 8, st));
      ra.tokens = reinterpret_cast<const double *>(d + lo.tokens);
      ra.na = reinterpret_cast<const double *>(d + lo.na);
      ra.queries = reinterpret_cast<const MaxSimQuery *>(d + lo.mq);
      ra.cq = reinterpret_cast<const MaxSimCandQuery *>(d + lo.cq);
      ra.recs = reinterpret_cast<const MaxSimCand *>(d + lo.recs);
      ra.rep = reinterpret_cast<unsigned long long *>(d + lo.rep);
      ra.stride = E;
      HIPCHK(launch_maxsim_rerank_score(ra, n_mq, longest_rows, st));
      MaxSimTrueAccArgs aa{};
      aa.rep = ra.rep;
      aa.queries = ra.queries;
      aa.acc = d_acc;
      aa.stride = E;
      HIPCHK(launch_maxsim_true_accumulate(aa, n_mq, st));
      if (t0 + TB < longest_tok) HIPCHK(hipStreamSynchronize(st));  // the staging is free for the next block
    }
    HIPCHK(hipMemcpyAsync(h_sums.get(), d_acc, (size_t)nq * (size_t)E * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // also: the staging is free for the next sub-batch
    for (int s = 0; s < nq; ++s) {
      const int64_t beg = coff[q0 + s], n = coff[q0 + s + 1] - beg;
      if (n > 0) memcpy(out + beg, h_sums.get() + (size_t)s * (size_t)E, (size_t)n * 8);
    }
  }
  return BBQ_OK;
}

namespace {

constexpr int kDefaultScratchMb = 256;  // bbq_index's default for group_scratch_mb: the budget of a call that has no index

// the checks of bbq_rerank_maxsim_groups_batch in front of the lock; *done: the call is answered
int check_rerank_call(const char *fn, bbq_vectors *v, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets, const float *queries, int32_t true_sim,
                      const int64_t *cand_offsets, const int32_t *cand_groups, double *out_true, bool *done) {
  *done = false;
  if (true_sim < 0 || true_sim > 2) return fail(BBQ_ERR_INVALID_ARG, "不支持的相似性函数: %d", true_sim);  // needs no handle
  if (!v) return fail(BBQ_ERR_INVALID_ARG, "%s: vectors handle is null", fn);
  if (!g) return fail(BBQ_ERR_INVALID_ARG, "%s: the group set is null", fn);
  if (n_queries < 0) return fail(BBQ_ERR_INVALID_ARG, "n_queries < 0");
  int rc = check_maxsim_vec_offsets(fn, n_queries, vec_offsets);
  if (rc != BBQ_OK) return rc;
  if (n_queries == 0) {
    *done = true;
    return BBQ_OK;
  }
  if (!queries) return fail(BBQ_ERR_INVALID_ARG, "%s: queries is null", fn);
  rc = check_maxsim_cand_offsets(fn, n_queries, cand_offsets);
  if (rc != BBQ_OK) return rc;
  if (cand_offsets[n_queries] == 0) {
    *done = true;
    return BBQ_OK;
  }
  if (!cand_groups) return fail(BBQ_ERR_INVALID_ARG, "%s: cand_groups is null", fn);
  if (!out_true) return fail(BBQ_ERR_INVALID_ARG, "%s: null output", fn);
  return BBQ_OK;
}

}  // namespace

extern "C" {

int bbq_maxsim_reduce_true(const double *rep_true, int64_t n_vectors, int64_t n_groups, double *out) {
  clear_error();
  if (n_vectors < 1 || n_groups < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_maxsim_reduce_true: at least one vector, no negative group count");
  if (n_groups > 0 && (!rep_true || !out)) return fail(BBQ_ERR_INVALID_ARG, "bbq_maxsim_reduce_true: null argument");
  for (int64_t s = 0; s < n_groups; ++s) {
    double acc = rep_true[s];  // from M_0, not from 0.0
    for (int64_t t = 1; t < n_vectors; ++t) acc = acc + rep_true[t * n_groups + s];
    if (acc != acc) {  // one NaN, whatever the operands' payloads were
      const uint64_t nan_bits = kTrueNaNBits;
      memcpy(&acc, &nan_bits, 8);
    }
    out[s] = acc;
  }
  return BBQ_OK;
}

int bbq_rerank_maxsim_groups_batch(bbq_vectors *v, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets, const float *queries, int32_t true_sim,
                                   const int64_t *cand_offsets, const int32_t *cand_groups, double *out_true) {
  static const char fn[] = "bbq_rerank_maxsim_groups_batch";
  clear_error();
  bool done = false;
  const int rc = check_rerank_call(fn, v, g, n_queries, vec_offsets, queries, true_sim, cand_offsets, cand_groups, out_true, &done);
  if (rc != BBQ_OK || done) return rc;
  return rerank_maxsim_groups(fn, v, g, n_queries, vec_offsets, queries, true_sim, cand_offsets, cand_groups, out_true, kDefaultScratchMb);
}

int bbq_search_maxsim_rerank_batch(bbq_index *ix, bbq_vectors *v, const bbq_groups *g, int32_t n_queries, const int64_t *vec_offsets, const float *queries,
                                   const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t k, int32_t factor, int32_t selector,
                                   int32_t true_sim, int32_t *out_group, float *out_quantized, double *out_true, int64_t *out_n) {
  static const char fn[] = "bbq_search_maxsim_rerank_batch";
  clear_error();
  if (true_sim < 0 || true_sim > 2) return fail(BBQ_ERR_INVALID_ARG, "不支持的相似性函数: %d", true_sim);  // needs no handle
  if (!ix || !v) return fail(BBQ_ERR_INVALID_ARG, "%s: null handle", fn);
  if (k < 0) return fail(BBQ_ERR_INVALID_ARG, "k必须是非负数");
  if (factor < 1) return fail(BBQ_ERR_INVALID_ARG, "%s: factor must be >= 1", fn);
  if (selector != 0 && selector != 1) return fail(BBQ_ERR_INVALID_ARG, "%s: selector must be 0 (heap) or 1 (sort)", fn);
  if (v->dim != ix->geom.dim) return fail(BBQ_ERR_DIM_MISMATCH, "%s: vectors are %d-d, index is %d-d", fn, v->dim, ix->geom.dim);
  if (n_queries > 0 && (!out_n || !queries)) return fail(BBQ_ERR_INVALID_ARG, "%s: null argument", fn);
  if (k > 0 && k * (int64_t)factor / factor != k) return fail(BBQ_ERR_INVALID_ARG, "%s: k*factor overflows", fn);
  const int64_t kk = k * (int64_t)factor;
  // the search strides its outputs by its k
  std::vector<int32_t> cgrp((size_t)std::max(n_queries, 0) * (size_t)std::max<int64_t>(kk, 1));
  std::vector<float> csc(cgrp.size());
  std::vector<int64_t> cn((size_t)std::max(n_queries, 1));
  int rc = bbq_search_maxsim_batch(ix, g, n_queries, vec_offsets, qquant, qcorr, query_bits, sim, kk, cgrp.data(), csc.data(), cn.data(), nullptr);
  if (rc != BBQ_OK) return rc;
  for (int32_t q = 0; q < n_queries; ++q) out_n[q] = 0;
  if (n_queries == 0 || k == 0) return BBQ_OK;
  if (!out_group || !out_quantized || !out_true) return fail(BBQ_ERR_INVALID_ARG, "output arrays are null");
  // each query's returned groups, in returned order, are its candidate list
  std::vector<int64_t> off((size_t)n_queries + 1, 0);
  for (int32_t q = 0; q < n_queries; ++q) off[q + 1] = off[q] + cn[q];
  std::vector<int32_t> cand((size_t)off[n_queries]);
  for (int32_t q = 0; q < n_queries; ++q) std::copy(cgrp.begin() + (int64_t)q * kk, cgrp.begin() + (int64_t)q * kk + cn[q], cand.begin() + off[q]);
  std::vector<double> ts(cand.size());
  if (!cand.empty()) {
    rc = rerank_maxsim_groups(fn, v, g, n_queries, vec_offsets, queries, true_sim, off.data(), cand.data(), ts.data(), ix->opt_group_scratch_mb);
    if (rc != BBQ_OK) return rc;
  }
  std::vector<Ranked> r;
  for (int32_t q = 0; q < n_queries; ++q) {
    rerank_select(selector, k, ts.data() + off[q], cn[q], r);
    for (size_t j = 0; j < r.size(); ++j) {
      out_group[(int64_t)q * k + j] = cgrp[(int64_t)q * kk + r[j].pos];
      out_quantized[(int64_t)q * k + j] = csc[(int64_t)q * kk + r[j].pos];
      out_true[(int64_t)q * k + j] = r[j].score;
    }
    out_n[q] = (int64_t)r.size();
  }
  return BBQ_OK;
}

}  // extern "C"
