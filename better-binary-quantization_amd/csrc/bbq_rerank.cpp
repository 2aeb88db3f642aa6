// bbq_rerank.cpp - oversample + exact rerank: fp32 vectors resident in HBM, true scores on the device (bbq_rerank_kernels.hip),
// the reference's two selectors on the host
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include "bbq_search.h"

using namespace bbq;

namespace {

// staging that a larger call outgrows is replaced with half as much again
template <class T>
hipError_t grow_staging(DevBuf<T> &b, int64_t need) {
  return (int64_t)b.size() >= need ? hipSuccess : b.alloc((size_t)(need + need / 2 + 64));
}

// Array.prototype.sort((a, b) => b.trueScore - a.trueScore), src/topKSelector.ts:75,112: stable; an element of the right
// run overtakes one of the left run only when the comparator says so (> 0), whatever it says for NaN
void sort_desc_stable(std::vector<Ranked> &v) {
  const size_t n = v.size();
  std::vector<Ranked> tmp(n);
  for (size_t w = 1; w < n; w *= 2) {
    for (size_t lo = 0; lo < n; lo += 2 * w) {
      const size_t mid = std::min(lo + w, n), hi = std::min(lo + 2 * w, n);
      size_t i = lo, j = mid, o = lo;
      while (i < mid && j < hi) tmp[o++] = (v[j].score - v[i].score) > 0 ? v[j++] : v[i++];
      while (i < mid) tmp[o++] = v[i++];
      while (j < hi) tmp[o++] = v[j++];
    }
    v.swap(tmp);
  }
}

// n rows behind those the handle holds.  The buffer grows by half as much again, at least to what is needed (an empty one gets exactly
// that), and the old rows move device to device.  Context mutex held, device current; `who` names the entry point in messages.
int append_vectors(bbq_vectors *v, const float *vectors, int64_t n, const char *who) {
  const int64_t dim = v->dim, total = v->n + n;
  DevBuf<float> grown;
  float *dst = v->d;
  if ((int64_t)v->d.size() < total * dim) {
    const int64_t cap = std::max<int64_t>(total, (int64_t)(v->d.size() / (size_t)dim) * 3 / 2);
    const hipError_t e = grown.alloc((size_t)(cap * dim));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "%s: %lld x %d fp32: %s", who, (long long)cap, v->dim, hipGetErrorString(e)); }
    if (v->n > 0) HIPCHK(hipMemcpy(grown, v->d, (size_t)(v->n * dim) * sizeof(float), hipMemcpyDeviceToDevice));
    dst = grown;
  }
  const int64_t count = n * dim, piece = 64LL << 20;  // 256 MB pieces keep the runtime's pinned staging bounded
  for (int64_t o = 0; o < count; o += piece) {
    const hipError_t e = hipMemcpy(dst + v->n * dim + o, vectors + o, (size_t)std::min(piece, count - o) * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(BBQ_ERR_HIP, "%s: copy: %s", who, hipGetErrorString(e));
  }
  HIPCHK(hipDeviceSynchronize());
  if (grown) v->d = std::move(grown);  // the old rows are released here, behind the copy
  v->n = total;
  return BBQ_OK;
}

}  // namespace

// the reference's two selectors over the true scores t[0 .. cnt) of one query -> r, best first: 0 the heap of k, drained and stably
// sorted (src/topKSelector.ts:40-76), 1 the stable descending sort, first k (:102-114)
void bbq::rerank_select(int32_t selector, int64_t k, const double *t, int64_t cnt, std::vector<Ranked> &r) {
  r.clear();
  if (selector == 0) {
    std::vector<int32_t> tag((size_t)k + 1);
    std::vector<double> tsc((size_t)k + 1);
    HeapReplay h(k, INT64_MAX);
    for (int64_t i = 0; i < cnt; ++i) h.offer64(t[i], (int32_t)i);
    const int64_t m = h.drain_ascending(tag.data(), tsc.data());
    for (int64_t j = 0; j < m; ++j) r.push_back(Ranked{tsc[j], tag[j]});
    sort_desc_stable(r);
  } else {
    for (int64_t i = 0; i < cnt; ++i) r.push_back(Ranked{t[i], (int32_t)i});
    sort_desc_stable(r);
    if ((int64_t)r.size() > k) r.resize((size_t)k);
  }
}

extern "C" {

int bbq_vectors_create(const float *vectors, int64_t n, int32_t dim, int32_t device, bbq_vectors **out) {
  clear_error();
  if (!out) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_create: out is null");
  *out = nullptr;
  if (n < 0 || dim <= 0 || (n > 0 && !vectors)) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_create: bad arguments");
  if (n > 0x7fffffffLL) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_create: more than 2^31-1 rows");
  DeviceCtx *ctx = nullptr;
  int rc = open_device(device, &ctx);
  if (rc != BBQ_OK) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  std::unique_ptr<bbq_vectors> v(new bbq_vectors());
  v->device = device;
  v->ctx = ctx;
  v->dim = dim;
  if (n > 0) {  // an empty handle, and the rows appended to it
    rc = append_vectors(v.get(), vectors, n, "bbq_vectors_create");
    if (rc != BBQ_OK) return rc;
  }
  *out = v.release();
  return BBQ_OK;
}

void bbq_vectors_destroy(bbq_vectors *v) {
  if (!v) return;
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  (void)hipSetDevice(v->device);
  delete v;
}

int bbq_vectors_append(bbq_vectors *v, const float *vectors, int64_t n) {
  clear_error();
  if (!v) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_append: vectors handle is null");
  if (n < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_append: n < 0");
  if (n == 0) return BBQ_OK;
  if (!vectors) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_append: vectors is null");
  if (v->n + n > 0x7fffffffLL) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_append: more than 2^31-1 rows");
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  HIPCHK(hipSetDevice(v->device));
  HIPCHK(hipStreamSynchronize(v->ctx->aux_stream));  // bbq_rerank_scores reads the rows on it
  return append_vectors(v, vectors, n, "bbq_vectors_append");
}

int bbq_vectors_compact(bbq_vectors *v, const bbq_filter *f) {
  clear_error();
  if (!v || !f) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_compact: null handle");
  if (f->device != v->device || f->ctx != v->ctx) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_compact: the filter lives on another device than the vectors");
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  HIPCHK(hipSetDevice(v->device));
  if (f->n_rows != v->n)
    return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_compact: the filter was made for %lld rows, the handle holds %lld", (long long)f->n_rows, (long long)v->n);
  const int64_t kept = f->count;
  if (kept == v->n) return BBQ_OK;
  HIPCHK(hipStreamSynchronize(v->ctx->aux_stream));  // bbq_rerank_scores reads the rows on it
  // out of place, as the index is compacted: exactly the kept rows afterwards, the old rows released behind the gather
  DevBuf<float> kept_rows;
  if (kept > 0) {
    const hipError_t e = kept_rows.alloc((size_t)(kept * v->dim));
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "bbq_vectors_compact: %lld x %d fp32: %s", (long long)kept, v->dim, hipGetErrorString(e)); }
    DevBuf<uint32_t> d_rank;
    CompactMap map;
    const int rc = stage_compact_map(f, d_rank, &map);
    if (rc != BBQ_OK) return rc;
    HIPCHK(launch_compact_vectors(kept_rows, v->d, v->dim, map, v->ctx->aux_stream));
    HIPCHK(hipStreamSynchronize(v->ctx->aux_stream));
  }
  v->d = std::move(kept_rows);
  v->n = kept;
  return BBQ_OK;
}

int bbq_vectors_update(bbq_vectors *v, const int32_t *ords, const float *vectors, int64_t n) {
  clear_error();
  if (!v) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_update: vectors handle is null");
  if (n < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_update: n < 0");
  if (n == 0) return BBQ_OK;
  if (!ords || !vectors) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_update: null argument");
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  HIPCHK(hipSetDevice(v->device));
  std::vector<int64_t> pos;
  int rc = update_winners(ords, n, v->n, pos);
  if (rc != BBQ_OK) return rc;
  hipStream_t st = v->ctx->aux_stream;
  HIPCHK(hipStreamSynchronize(st));  // bbq_rerank_scores reads the rows on it
  // the block staged as it came, then the winners scattered to their ords: nothing is written before every allocation has succeeded
  DevBuf<float> staged;
  DevBuf<int32_t> d_ords;
  DevBuf<int64_t> d_pos;
  const hipError_t e = staged.alloc((size_t)(n * v->dim));
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "bbq_vectors_update: %lld x %d fp32: %s", (long long)n, v->dim, hipGetErrorString(e)); }
  rc = stage_winners(st, ords, n, pos, d_ords, d_pos);
  if (rc != BBQ_OK) return rc;
  const int64_t count = n * v->dim, piece = 64LL << 20;  // 256 MB pieces keep the runtime's pinned staging bounded
  for (int64_t o = 0; o < count; o += piece)
    HIPCHK(hipMemcpyAsync(staged + o, vectors + o, (size_t)std::min(piece, count - o) * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(launch_scatter_vectors(v->d, staged, v->dim, d_ords, d_pos, (int64_t)pos.size(), st));
  HIPCHK(hipStreamSynchronize(st));
  return BBQ_OK;
}

int64_t bbq_vectors_size(const bbq_vectors *v) { return v ? v->n : 0; }
int32_t bbq_vectors_dimension(const bbq_vectors *v) { return v ? v->dim : 0; }

int bbq_rerank_scores(bbq_vectors *v, int32_t n_queries, const float *queries, const int64_t *offsets, const int32_t *rows,
                      int32_t true_sim, double *out_true) {
  clear_error();
  if (!v) return fail(BBQ_ERR_INVALID_ARG, "bbq_rerank_scores: vectors handle is null");
  if (n_queries < 0 || n_queries > 65535) return fail(BBQ_ERR_INVALID_ARG, "bbq_rerank_scores: n_queries out of range");
  if (true_sim < 0 || true_sim > 2) return fail(BBQ_ERR_INVALID_ARG, "不支持的相似性函数: %d", true_sim);
  if (n_queries == 0) return BBQ_OK;
  if (!queries || !offsets) return fail(BBQ_ERR_INVALID_ARG, "bbq_rerank_scores: null argument");
  if (offsets[0] != 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_rerank_scores: offsets[0] must be 0");
  int64_t max_count = 0;
  for (int32_t q = 0; q < n_queries; ++q) {
    const int64_t c = offsets[q + 1] - offsets[q];
    if (c < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_rerank_scores: offsets must ascend");
    max_count = std::max(max_count, c);
  }
  const int64_t total = offsets[n_queries];
  if (total == 0) return BBQ_OK;
  if (!rows || !out_true) return fail(BBQ_ERR_INVALID_ARG, "bbq_rerank_scores: null argument");
  for (int64_t i = 0; i < total; ++i)
    if (rows[i] < 0 || rows[i] >= v->n) return fail(BBQ_ERR_INVALID_ARG, "基础向量%d不存在", rows[i]);
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  HIPCHK(hipSetDevice(v->device));
  HIPCHK(grow_staging(v->d_q, (int64_t)n_queries * v->dim));
  HIPCHK(grow_staging(v->d_off, (int64_t)n_queries + 1));
  HIPCHK(grow_staging(v->d_rows, total));
  HIPCHK(grow_staging(v->d_out, total));
  hipStream_t st = v->ctx->aux_stream;
  HIPCHK(hipMemcpyAsync(v->d_q, queries, (size_t)n_queries * v->dim * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(v->d_off, offsets, (size_t)(n_queries + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(v->d_rows, rows, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, st));
  RerankArgs a{};
  a.vecs = v->d;
  a.n = v->n;
  a.dim = v->dim;
  a.sim = true_sim;
  a.queries = v->d_q;
  a.offsets = v->d_off;
  a.rows = v->d_rows;
  a.out = v->d_out;
  HIPCHK(launch_rerank(a, n_queries, max_count, st));
  HIPCHK(hipMemcpyAsync(out_true, v->d_out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BBQ_OK;
}

int bbq_search_rerank_batch(bbq_index *ix, bbq_vectors *v, int32_t n_queries, const float *queries, const uint8_t *qquant,
                            const double *qcorr, int32_t query_bits, int32_t sim, int64_t k, int32_t factor, int32_t selector,
                            int32_t true_sim, int32_t *out_idx, float *out_quantized, double *out_true, int64_t *out_n) {
  clear_error();
  if (!ix || !v) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_rerank_batch: null handle");
  if (k < 0) return fail(BBQ_ERR_INVALID_ARG, "k必须是非负数");
  if (factor < 1) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_rerank_batch: factor must be >= 1");
  if (selector != 0 && selector != 1) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_rerank_batch: selector must be 0 (heap) or 1 (sort)");
  if (v->dim != ix->geom.dim) return fail(BBQ_ERR_DIM_MISMATCH, "bbq_search_rerank_batch: vectors are %d-d, index is %d-d", v->dim, ix->geom.dim);
  if (v->n < ix->n_rows) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_rerank_batch: %lld vectors for %lld index rows", (long long)v->n, (long long)ix->n_rows);
  if (n_queries > 0 && (!out_n || !queries)) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_rerank_batch: null argument");
  if (k > 0 && k * (int64_t)factor / factor != k) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_rerank_batch: k*factor overflows");
  const int64_t kk = k * (int64_t)factor;
  const int64_t kq = std::min<int64_t>(kk, ix->n_rows);  // candidates a query can return
  std::vector<int32_t> cidx((size_t)n_queries * (size_t)std::max<int64_t>(kk, 1));
  std::vector<float> csc(cidx.size());
  std::vector<int64_t> cn((size_t)std::max(n_queries, 1));
  // the search strides its outputs by its k; ask for kk but only kq entries per query can be filled
  int rc = bbq_search_batch(ix, n_queries, qquant, qcorr, query_bits, sim, kk, cidx.data(), csc.data(), cn.data());
  if (rc != BBQ_OK) return rc;
  (void)kq;
  for (int32_t q = 0; q < n_queries; ++q) out_n[q] = 0;
  if (n_queries == 0 || k == 0) return BBQ_OK;
  if (!out_idx || !out_quantized || !out_true) return fail(BBQ_ERR_INVALID_ARG, "output arrays are null");
  std::vector<int64_t> off((size_t)n_queries + 1, 0);
  for (int32_t q = 0; q < n_queries; ++q) off[q + 1] = off[q] + cn[q];
  std::vector<int32_t> rows((size_t)off[n_queries]);
  for (int32_t q = 0; q < n_queries; ++q)
    std::copy(cidx.begin() + (int64_t)q * kk, cidx.begin() + (int64_t)q * kk + cn[q], rows.begin() + off[q]);
  std::vector<double> ts(rows.size());
  rc = bbq_rerank_scores(v, n_queries, queries, off.data(), rows.data(), true_sim, ts.data());
  if (rc != BBQ_OK) return rc;
  std::vector<Ranked> r;
  for (int32_t q = 0; q < n_queries; ++q) {
    rerank_select(selector, k, ts.data() + off[q], cn[q], r);
    for (size_t j = 0; j < r.size(); ++j) {
      out_idx[(int64_t)q * k + j] = cidx[(int64_t)q * kk + r[j].pos];
      out_quantized[(int64_t)q * k + j] = csc[(int64_t)q * kk + r[j].pos];
      out_true[(int64_t)q * k + j] = r[j].score;
    }
    out_n[q] = (int64_t)r.size();
  }
  return BBQ_OK;
}

}  // extern "C"
