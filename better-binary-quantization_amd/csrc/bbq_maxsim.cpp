// bbq_maxsim.cpp - MaxSim search: bbq_search_maxsim_batch, bbq_maxsim_reduce, bbq_maxsim_token_block (kernels: bbq_maxsim_kernels.hip, the
// grouped search's score pass and the span search's select pass).  A query is a run of token vectors and a live group of a group set
// (bbq_group.cpp) scores the ordered f64 sum of its representatives' f32 scores.  A call follows the grouped search's host path: sub-batches
// bounded by scratch, and inside a sub-batch the queries' tokens in blocks of at most kMaxSimTokenBlock - a block's vectors staged in one
// copy, its keys cleared, the score pass (fused where the option and the shape allow, the grouped search's kernel with the block's
// vectors as its queries otherwise) and the accumulate pass - then the select pass over the sums, the answer blocks back in one copy, the
// device's k sorted and proven, and the reference's heap replayed over the sums of the queries it could not prove.
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include <thread>
#include "bbq_search.h"

using namespace bbq;

namespace {

constexpr int kMaxSimMaxQueries = 1024;  // of a sub-batch: 32 768 vectors in a score launch at the most
// maxsim_fused -1: the fused kernel wherever it exists.  At 1 M rows of 768, 1024 and 1536 dimensions (profiles/maxsim_search*.json) the
// slowest of its three runs beat the fastest of the unfused path's by more than that path's spread on every leg: 1.4 to 1.7 times faster
constexpr bool kMaxSimFusedDefault = true;

inline size_t align16(size_t b) { return (b + 15) / 16 * 16; }

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
  {
    const hipError_t e = ix->ctx->d_span.reserve(big.bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "MaxSim search: %zu bytes of scratch: %s", big.bytes, hipGetErrorString(e)); }
  }
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
  const int64_t n_tiles = tiles_of(gs->n_rows);
  MaxSimScoreArgs ma{};
  GroupScoreArgs &ga = ma.g;
  ga.idx = launch_view(ix, ix->main).view;
  ga.idx.row_sums = row_sums_for_launch(ix) ? ix->main.view.row_sums : nullptr;
  ga.starts = gs->d_words.get();
  ga.accept = gs->filtered ? gs->d_words.get() + n_tiles + 1 : nullptr;
  ga.first_group = gs->d_index.get();
  ga.slot = reinterpret_cast<const int32_t *>(gs->d_index.get() + n_tiles + 1);
  ga.live = L;
  ga.n_chunks = (int32_t)ix->main.n_chunks();
  ga.l2_shift = l2_share_shift(ix);
  std::vector<int64_t> replay;  // the queries of the sub-batch whose heap the host replays
  std::vector<uint64_t> ent;

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
      MaxSimQuery *h_mq = reinterpret_cast<MaxSimQuery *>(head.get() + lo.mq);
      int n_mq = 0;
      int32_t v = 0;  // vectors staged so far
      for (int s = 0; s < nq; ++s) {
        const int64_t first = voff[q0 + s], T = voff[q0 + s + 1] - first;
        if (T <= t0) continue;
        const int n_tok = (int)std::min<int64_t>(TB, T - t0);
        h_mq[n_mq++] = MaxSimQuery{v, n_tok, s, (t0 == 0 ? kMaxSimFirst : 0) | (t0 + n_tok == T ? kMaxSimLast : 0)};
        for (int t = 0; t < n_tok; ++t, ++v) {
          const int64_t vec = first + t0 + t;
          fill_query(ix, head.get() + lo.qdata + (size_t)v * qb, reinterpret_cast<QueryParams *>(head.get() + lo.qparams) + v,
                     qquant + (size_t)vec * ix->geom.dim, qcorr + (size_t)vec * 4, planes, one_bit, sim);
        }
      }
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

    // what the device selected: exactly k sums above the cut and no NaN - sorted by descending score; two equal sums among them, or one
    // equal to the cut, and the heap's history decides: replayed like the queries the device could not prove
    replay.clear();
    for (int s = 0; s < nq; ++s) {
      const int64_t q = q0 + s;
      bool proven = false;
      if (sel) {
        const uint64_t *blk = back.get() + (size_t)s * out_stride;
        if ((uint32_t)(blk[0] >> 32) == 0u && (int64_t)(uint32_t)blk[0] == k) {
          ent.assign(blk + 2, blk + 2 + k);
          std::sort(ent.begin(), ent.end(), [](uint64_t x, uint64_t y) { return entry_score(x) > entry_score(y); });
          proven = entry_score(ent[(size_t)k - 1]) != entry_score(blk[1]);
          for (int64_t i = 1; proven && i < k; ++i) proven = entry_score(ent[(size_t)i - 1]) != entry_score(ent[(size_t)i]);
          if (proven) {
            unpack_entries(ent.data(), k, out_group + q * k, out_score + q * k);
            out_n[q] = k;
          }
        }
      }
      if (out_status) out_status[q] = proven ? 0 : 1;
      if (!proven) replay.push_back(s);
    }
    if (!replay.empty()) {
      // the reference loop (src/binaryQuantizationFormat.ts:383-411) over the live groups in ascending group number: the literal heap of
      // min(k, L) (the sums come back query by query, or in one copy where they are at least half of the sub-batch's)
      auto bring_back = [&](int64_t first, int64_t rows) {
        hipError_t e = hipMemcpyAsync(h_scores.get() + first, d_scores + first, (size_t)rows * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_ords.get() + first, d_ords + first, (size_t)rows * 4, hipMemcpyDeviceToHost, st);
        return e;
      };
      if (2 * (int64_t)replay.size() >= nq) {
        HIPCHK(bring_back(0, (int64_t)nq * L));
      } else {
        for (int64_t s : replay) HIPCHK(bring_back(s * L, L));
      }
      HIPCHK(hipStreamSynchronize(st));
      auto work = [&](size_t t, size_t T) {
        for (size_t i = t; i < replay.size(); i += T) {
          const int64_t s = replay[i], q = q0 + s;
          const float *sc = h_scores.get() + s * L;
          const uint32_t *od = h_ords.get() + s * L;
          HeapReplay hr(k, L);
          for (int64_t r = 0; r < L; ++r) hr.offer(sc[r], (int32_t)od[r]);
          out_n[q] = hr.finish(out_group + q * k, out_score + q * k);
        }
      };
      const size_t T = std::min<size_t>((size_t)std::max(ix->opt_replay_threads, 1), replay.size());
      if (T <= 1 || (int64_t)replay.size() * L < 4096) {
        work(0, 1);
      } else {
        std::vector<std::thread> th;
        for (size_t t = 0; t < T; ++t) th.emplace_back(work, t, T);
        for (std::thread &x : th) x.join();
      }
    }
  }
  return BBQ_OK;
}

}  // namespace

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
  if (n_queries > 0) {
    if (!vec_offsets) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_maxsim_batch: vec_offsets is null");
    if (vec_offsets[0] != 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_maxsim_batch: vec_offsets[0] must be 0 (query 0)");
    for (int32_t q = 0; q < n_queries; ++q)
      if (vec_offsets[q + 1] <= vec_offsets[q])
        return fail(BBQ_ERR_INVALID_ARG, "bbq_search_maxsim_batch: query %d has no token vector or vec_offsets descends: [%lld, %lld)", q, (long long)vec_offsets[q],
                    (long long)vec_offsets[q + 1]);
    if (vec_offsets[n_queries] > 0x7fffffffll) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_maxsim_batch: more than 2^31 - 1 token vectors");
  }
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
