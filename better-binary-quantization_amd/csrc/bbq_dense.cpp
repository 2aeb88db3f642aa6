// bbq_dense.cpp - the dense path: every score of one query, for the queries the sparse path cannot bound, for large k, for the
// shards of a multi-device index, and for bbq_score_rows.
#include "bbq_search.h"

using namespace bbq;

namespace {

// query qi of the call into the device's auxiliary query buffer, on the auxiliary stream; returns when it is there
int stage_aux_query(const SearchCall &c, int64_t qi) {
  bbq_index *ix = c.ix;
  int rc = ensure_aux_qbuf(ix->ctx, qbuf_bytes_per_query_w(ix->geom.w16));
  if (rc != BBQ_OK) return rc;
  const int64_t qb = query_data_bytes(ix, c.planes);
  std::vector<uint8_t> hb((size_t)qb + sizeof(QueryParams));
  fill_query(ix, hb.data(), reinterpret_cast<QueryParams *>(hb.data() + qb), c.qquant + (size_t)qi * ix->geom.dim, c.qcorr + (size_t)qi * 4,
             c.planes, c.one_bit, c.sim);
  hipStream_t st = ix->ctx->aux_stream;
  HIPCHK(hipMemcpyAsync(ix->ctx->d_aux_qbuf, hb.data(), hb.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return BBQ_OK;
}

// a dense sweep of the main storage from chunk_begin on with the staged query; the caller adds where the scores go
ScanArgs dense_scan_args(const SearchCall &c, int64_t chunk_begin) {
  bbq_index *ix = c.ix;
  ScanArgs a{};
  a.idx = launch_view(ix, ix->main).view;
  a.qplanes = reinterpret_cast<const uint4 *>(ix->ctx->d_aux_qbuf.get());
  a.qparams = reinterpret_cast<const QueryParams *>(ix->ctx->d_aux_qbuf + query_data_bytes(ix, c.planes));
  a.chunk_begin = chunk_begin;
  a.row_id_base = ix->main.row_id_base;
  a.flags = ix->ctx->d_aux_flags;
  return a;
}

// every f32 score of one query to the host (out [n_rows] of this index)
int dense_scores_one(const SearchCall &c, int64_t qi, float *out) {
  bbq_index *ix = c.ix;
  const int64_t n = ix->main.view.n_rows;
  const int64_t chunks = ix->main.n_chunks();
  HIPCHK(ix->d_dense_all.reserve((size_t)std::max<int64_t>(n, 1)));
  int rc = stage_aux_query(c, qi);
  if (rc != BBQ_OK) return rc;
  hipStream_t st = ix->ctx->aux_stream;
  ScanArgs a = dense_scan_args(c, 0);
  a.dense_score32 = ix->d_dense_all;
  a.dense_stride = n;
  // gridDim.x is limited to 2^31-1: fine for any index that fits in HBM
  HIPCHK(launch_scan(a, c.planes, true, 1, (int)chunks, st));
  HIPCHK(hipMemcpyAsync(out, ix->d_dense_all, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BBQ_OK;
}

}  // namespace

namespace bbq {

// dense path for one query: every f32 score to the host, full replay of the reference loop - of a filtered call: over the accepted
// rows only, ascending, which is the loop the filter's contract names
int dense_search_one(const SearchCall &c, int64_t qi, int32_t *out_idx, float *out_score, int64_t *out_n) {
  bbq_index *ix = c.ix;
  const int64_t n = ix->main.view.n_rows;
  std::vector<float> h((size_t)std::max<int64_t>(n, 1));
  int rc = dense_scores_one(c, qi, h.data());
  if (rc != BBQ_OK) return rc;
  HeapReplay hr(c.k_out, c.filter ? c.n_eff : n);
  if (c.filter) {
    for (size_t w = 0; w < c.filter->h_bits.size(); ++w)
      for (uint64_t bits = c.filter->h_bits[w]; bits; bits &= bits - 1) {
        const int64_t i = (int64_t)w * 64 + __builtin_ctzll(bits);
        hr.offer(h[(size_t)i], (int32_t)(ix->main.row_id_base + i));
      }
  } else {
    for (int64_t i = 0; i < n; ++i) hr.offer(h[(size_t)i], (int32_t)(ix->main.row_id_base + i));
  }
  *out_n = hr.finish(out_idx, out_score);
  ix->stats.dense_fallbacks += 1;
  ix->stats.candidates += c.filter ? c.n_eff : n;
  return BBQ_OK;
}

// every f32 score of one query on this index (shard), to host memory: the dense path of a multi-device index
int dense_scores_host(bbq_index *ix, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, float *out) {
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  if (ix->n_rows == 0) return BBQ_OK;
  const SearchCall c(ix, qquant, qcorr, planes_of_call(ix, qquant, ix->geom.dim, query_bits == 1), query_bits, sim, 0);
  ix->stats.dense_fallbacks += 1;
  return dense_scores_one(c, 0, out);
}

}  // namespace bbq

extern "C" {

int bbq_score_rows(bbq_index *ix, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                   int64_t row_begin, int64_t row_count, int32_t *out_qcdist, double *out_score64, float *out_score32) {
  clear_error();
  int rc = validate_query_args(ix, 1, qquant, qcorr, query_bits, sim, 0);
  if (rc != BBQ_OK) return rc;
  if (row_begin < 0 || row_count < 0 || row_begin + row_count > ix->n_rows)
    return fail(BBQ_ERR_INVALID_ARG, "向量索引 %lld 不存在", (long long)(row_begin + row_count - 1));
  if (row_count == 0) return BBQ_OK;
  if (ix->multi) return multi_score_rows(ix, qquant, qcorr, query_bits, sim, row_begin, row_count, out_qcdist, out_score64, out_score32);
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  const SearchCall c(ix, qquant, qcorr, planes_of_call(ix, qquant, ix->geom.dim, query_bits == 1), query_bits, sim, 0);
  rc = stage_aux_query(c, 0);
  if (rc != BBQ_OK) return rc;
  hipStream_t st = ix->ctx->aux_stream;
  const int64_t piece_chunks = 1024;  // 1M rows per piece
  const int64_t c_first = row_begin / kChunkRows, c_last = (row_begin + row_count + kChunkRows - 1) / kChunkRows;
  const int64_t piece_rows = std::min(piece_chunks, c_last - c_first) * kChunkRows;
  DevBuf<float> d32;
  DevBuf<int32_t> dqc;
  DevBuf<double> d64;
  HIPCHK(d32.alloc((size_t)piece_rows));
  HIPCHK(dqc.alloc((size_t)piece_rows));
  HIPCHK(d64.alloc((size_t)piece_rows));
  std::vector<float> h32((size_t)piece_rows);
  std::vector<int32_t> hqc((size_t)piece_rows);
  std::vector<double> h64((size_t)piece_rows);
  rc = BBQ_OK;
  for (int64_t cb = c_first; cb < c_last && rc == BBQ_OK; cb += piece_chunks) {
    const int64_t nc = std::min(piece_chunks, c_last - cb);
    ScanArgs a = dense_scan_args(c, cb);
    a.dense_score32 = d32;
    a.dense_qcdist = dqc;
    a.dense_score64 = d64;
    a.dense_stride = piece_rows;
    hipError_t e = launch_scan(a, c.planes, true, 1, (int)nc, st);
    const int64_t r0 = cb * kChunkRows, r1 = std::min((cb + nc) * kChunkRows, ix->main.view.n_rows);
    if (e == hipSuccess) e = hipMemcpyAsync(h32.data(), d32, (size_t)(r1 - r0) * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hqc.data(), dqc, (size_t)(r1 - r0) * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h64.data(), d64, (size_t)(r1 - r0) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { rc = fail(BBQ_ERR_HIP, "bbq_score_rows: %s", hipGetErrorString(e)); break; }
    const int64_t lo = std::max(r0, row_begin), hi = std::min(r1, row_begin + row_count);
    for (int64_t r = lo; r < hi; ++r) {
      if (out_score32) out_score32[r - row_begin] = h32[(size_t)(r - r0)];
      if (out_qcdist) out_qcdist[r - row_begin] = hqc[(size_t)(r - r0)];
      if (out_score64) out_score64[r - row_begin] = h64[(size_t)(r - r0)];
    }
  }
  return rc;
}

}  // extern "C"
