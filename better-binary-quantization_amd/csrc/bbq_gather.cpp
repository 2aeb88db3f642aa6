// bbq_gather.cpp - scoring and ranking chosen rows: bbq_score_ords, bbq_score_ords_batch, bbq_search_ords_batch (kernel:
// bbq_gather_kernels.hip).  The host checks every list before the first launch, stages queries, offsets and ords, works through a
// long call in launches of bounded size and brings back only the outputs asked for; the search replays the reference's heap over the
// f32 scores in list order (replay_lists, bbq_replay.cpp).
#include <string.h>
#include "bbq_search.h"

using namespace bbq;

namespace {

// One launch takes at most this many list entries and this many queries, so the device scratch of a call of any size stays below
// kGatherMaxEntries * 20 B (ords + the three outputs) + kGatherMaxQueries staged queries: 20 MiB + 0.9 MiB at 768-d.  The scratch is
// the context's (DeviceCtx::d_gather) and only grows.
constexpr int64_t kGatherMaxEntries = 1 << 20;
constexpr int kGatherMaxQueries = 1024;

// entries [beg, end) of the call's ords: a whole list, or a piece of one longer than a launch takes
struct ListPiece { int32_t q; int64_t beg, end; };

// offsets as bbq_rerank_scores takes them; *total = offsets[n_queries]
int check_offsets(const char *who, int32_t n_queries, const int64_t *offsets, int64_t *total) {
  if (!offsets) return fail(BBQ_ERR_INVALID_ARG, "%s: offsets is null", who);
  if (offsets[0] != 0) return fail(BBQ_ERR_INVALID_ARG, "%s: offsets[0] must be 0", who);
  for (int32_t q = 0; q < n_queries; ++q)
    if (offsets[q + 1] < offsets[q]) return fail(BBQ_ERR_INVALID_ARG, "%s: offsets must ascend", who);
  *total = offsets[n_queries];
  return BBQ_OK;
}

// the first entry, in list order, that names no row: what the reference's loop throws on (src/binaryQuantizedScorer.ts:389-400)
int check_ords(const int32_t *ords, int64_t total, int64_t n_rows) {
  for (int64_t i = 0; i < total; ++i)
    if (ords[i] < 0 || ords[i] >= n_rows) return fail(BBQ_ERR_INVALID_ARG, "向量索引 %d 不存在", ords[i]);
  return BBQ_OK;
}

// a single-device index: lists checked, then launch by launch on the auxiliary stream.  Takes the context's lock.
int score_ords_single(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                      const int64_t *offsets, const int32_t *ords, int32_t *out_qcdist, double *out_score64, float *out_score32) {
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  const int64_t total = offsets[n_queries];
  // under the lock: the rows the check sees are the rows the kernel reads (a compaction on another thread comes before or after)
  int rc = check_ords(ords, total, ix->main.view.n_rows);
  if (rc != BBQ_OK) return rc;
  if (!out_qcdist && !out_score64 && !out_score32) return BBQ_OK;
  const int one_bit = query_bits == 1 ? 1 : 0;
  const int planes = planes_of_call(ix, qquant, (int64_t)n_queries * ix->geom.dim, one_bit);
  const size_t qb = (size_t)query_data_bytes(ix, planes);

  std::vector<ListPiece> pieces;
  for (int32_t q = 0; q < n_queries; ++q)
    for (int64_t b = offsets[q]; b < offsets[q + 1]; b += kGatherMaxEntries) pieces.push_back(ListPiece{q, b, std::min(b + kGatherMaxEntries, offsets[q + 1])});
  // the scratch of the largest launch: [offsets | query data | query uniforms] [ords] [qcDist] [f32] [f64]
  const size_t max_q = std::min<size_t>(pieces.size(), (size_t)kGatherMaxQueries), max_e = (size_t)std::min<int64_t>(total, kGatherMaxEntries);
  const size_t head_cap = align16((max_q + 1) * 8) + max_q * (qb + sizeof(QueryParams));
  const size_t at_ords = align16(head_cap), at_qc = at_ords + align16(max_e * 4), at_32 = at_qc + align16(max_e * 4), at_64 = at_32 + align16(max_e * 4);
  rc = reserve_scratch(ix->ctx->d_gather, at_64 + max_e * 8, "bbq_score_ords");
  if (rc != BBQ_OK) return rc;
  uint8_t *d = ix->ctx->d_gather;
  hipStream_t st = ix->ctx->aux_stream;
  std::vector<uint8_t> head(head_cap);

  for (size_t p0 = 0; p0 < pieces.size();) {
    // consecutive pieces are consecutive in ords (an empty list has no piece): one launch covers the entries [g0, g1)
    size_t p1 = p0;
    int64_t longest = 0;
    const int64_t g0 = pieces[p0].beg;
    while (p1 < pieces.size() && p1 - p0 < (size_t)kGatherMaxQueries && pieces[p1].end - g0 <= kGatherMaxEntries) {
      longest = std::max(longest, pieces[p1].end - pieces[p1].beg);
      ++p1;
    }
    const int nq = (int)(p1 - p0);
    const int64_t cnt = pieces[p1 - 1].end - g0;
    const size_t at_qdata = align16((size_t)(nq + 1) * 8), at_qparams = at_qdata + (size_t)nq * qb, head_bytes = at_qparams + (size_t)nq * sizeof(QueryParams);
    int64_t *loc_off = reinterpret_cast<int64_t *>(head.data());
    for (int s = 0; s < nq; ++s) {
      const ListPiece &lp = pieces[p0 + (size_t)s];
      loc_off[s] = lp.beg - g0;
      fill_query(ix, head.data() + at_qdata + (size_t)s * qb, reinterpret_cast<QueryParams *>(head.data() + at_qparams) + s,
                 qquant + (size_t)lp.q * ix->geom.dim, qcorr + (size_t)lp.q * 4, planes, one_bit, sim);
    }
    loc_off[nq] = cnt;
    HIPCHK(hipMemcpyAsync(d, head.data(), head_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d + at_ords, ords + g0, (size_t)cnt * 4, hipMemcpyHostToDevice, st));
    GatherArgs a{};
    a.idx = ix->main.view;
    a.qplanes = reinterpret_cast<const uint4 *>(d + at_qdata);
    a.qparams = reinterpret_cast<const QueryParams *>(d + at_qparams);
    a.offsets = reinterpret_cast<const int64_t *>(d);
    a.ords = reinterpret_cast<const int32_t *>(d + at_ords);
    a.out_qcdist = out_qcdist ? reinterpret_cast<int32_t *>(d + at_qc) : nullptr;
    a.out_score32 = out_score32 ? reinterpret_cast<float *>(d + at_32) : nullptr;
    a.out_score64 = out_score64 ? reinterpret_cast<double *>(d + at_64) : nullptr;
    HIPCHK(launch_score_ords(a, planes, nq, longest, st));
    if (out_qcdist) HIPCHK(hipMemcpyAsync(out_qcdist + g0, d + at_qc, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    if (out_score32) HIPCHK(hipMemcpyAsync(out_score32 + g0, d + at_32, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    if (out_score64) HIPCHK(hipMemcpyAsync(out_score64 + g0, d + at_64, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // the staging vector and the scratch are free for the next launch
    p0 = p1;
  }
  return BBQ_OK;
}

// arguments checked (everything but the ords of a single-device index, which are checked under its lock): the scores of every entry
int score_ords_checked(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                       const int64_t *offsets, const int32_t *ords, int32_t *out_qcdist, double *out_score64, float *out_score32) {
  if (ix->multi) {
    const int rc = check_ords(ords, offsets[n_queries], ix->n_rows);
    if (rc != BBQ_OK) return rc;
    return multi_score_ords(ix, n_queries, qquant, qcorr, query_bits, sim, offsets, ords, out_qcdist, out_score64, out_score32);
  }
  return score_ords_single(ix, n_queries, qquant, qcorr, query_bits, sim, offsets, ords, out_qcdist, out_score64, out_score32);
}

}  // namespace

extern "C" {

int bbq_score_ords_batch(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                         const int64_t *offsets, const int32_t *ords, int32_t *out_qcdist, double *out_score64, float *out_score32) {
  clear_error();
  int rc = validate_query_args(ix, n_queries, qquant, qcorr, query_bits, sim, 0);
  if (rc != BBQ_OK) return rc;
  if (n_queries == 0) return BBQ_OK;
  int64_t total = 0;
  rc = check_offsets("bbq_score_ords_batch", n_queries, offsets, &total);
  if (rc != BBQ_OK) return rc;
  if (total == 0) return BBQ_OK;
  if (!ords) return fail(BBQ_ERR_INVALID_ARG, "bbq_score_ords_batch: ords is null");
  return score_ords_checked(ix, n_queries, qquant, qcorr, query_bits, sim, offsets, ords, out_qcdist, out_score64, out_score32);
}

int bbq_score_ords(bbq_index *ix, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, const int32_t *ords, int64_t n,
                   int32_t *out_qcdist, double *out_score64, float *out_score32) {
  if (n < 0) {
    clear_error();
    return fail(BBQ_ERR_INVALID_ARG, "bbq_score_ords: n < 0");
  }
  const int64_t offsets[2] = {0, n};
  return bbq_score_ords_batch(ix, 1, qquant, qcorr, query_bits, sim, offsets, ords, out_qcdist, out_score64, out_score32);
}

int bbq_search_ords_batch(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t k,
                          const int64_t *offsets, const int32_t *ords, int32_t *out_idx, float *out_score, int64_t *out_n) {
  clear_error();
  int rc = validate_query_args(ix, n_queries, qquant, qcorr, query_bits, sim, k);
  if (rc != BBQ_OK) return rc;
  if (n_queries == 0) return BBQ_OK;
  int64_t total = 0;
  rc = check_offsets("bbq_search_ords_batch", n_queries, offsets, &total);
  if (rc != BBQ_OK) return rc;
  if (!out_n) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_ords_batch: out_n is null");
  if (total > 0 && !ords) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_ords_batch: ords is null");
  if (total > 0 && k > 0 && (!out_idx || !out_score)) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_ords_batch: null output");
  std::vector<float> s32((size_t)std::max<int64_t>(total, 1));
  if (total > 0) {  // also for k == 0: an ord that names no row is an error whatever k is, as in the reference's loop
    rc = score_ords_checked(ix, n_queries, qquant, qcorr, query_bits, sim, offsets, ords, nullptr, nullptr, k > 0 ? s32.data() : nullptr);
    if (rc != BBQ_OK) return rc;
  }
  replay_lists(n_queries, offsets, ords, s32.data(), k, ix->opt_replay_threads, out_idx, out_score, out_n);  // in the order given
  return BBQ_OK;
}

}  // extern "C"
