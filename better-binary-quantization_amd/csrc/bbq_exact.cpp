// bbq_exact.cpp - exact search: bbq_true_topk, bbq_vectors_search_batch, bbq_vectors_set_option (kernels: bbq_exact_kernels.hip).  The
// true top-k of raw fp32 queries over the rows a bbq_vectors keeps in HBM - the reference's getTrueTopK (tests/recall-common.ts:143-149)
// - scored and selected on the device: a sub-batch of at most 1024 queries is widened to f64 and staged in one copy, the rows are worked
// through a slab at a time - the score pass leaves a slab's keys, the select pass folds them into each query's running list - and the
// lists, k x (row, key) a query, are the only thing that comes back.
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>
#include "bbq_search.h"

using namespace bbq;

namespace {

constexpr int kExactMaxQueries = 1024;          // of a sub-batch
constexpr int64_t kExactScratchBytes = 256ll << 20;  // a sub-batch's slab keys stay under it: at least one slab of kExactSlabStep rows
constexpr int64_t kExactSlabStep = 256, kExactSlabMax = 1ll << 24;
constexpr int QB = kExactQueryBlock;
constexpr int QG = kMaxSimRerankTokenGroup;

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// where a sub-batch of nq queries that keeps kk rows a query and works in slabs of S rows keeps what: [squared norms | queries] come from
// the host in one copy, [list keys | list rows | list counts] go back in one
struct Layout {
  size_t na, queries, head_bytes, list_keys, list_rows, list_count, lists_end, keys, bytes;
  int64_t slots;
  Layout(int nq, int64_t kk, int64_t S, int32_t dim) {
    slots = ((int64_t)nq + QG - 1) / QG * QG;  // every block but the last is full
    na = 0;
    queries = align16(na + (size_t)slots * 8);
    head_bytes = queries + (size_t)slots * (size_t)dim * 8;
    list_keys = align16(head_bytes);
    list_rows = list_keys + (size_t)nq * (size_t)kk * 8;
    list_count = list_rows + (size_t)nq * (size_t)kk * 4;
    lists_end = list_count + (size_t)nq * 4;
    keys = align256(lists_end);
    bytes = keys + (size_t)nq * (size_t)S * 8;
  }
};

struct KeyRow {
  unsigned long long key;
  int32_t row;
};
inline bool ranks_first(const KeyRow &a, const KeyRow &b) { return a.key > b.key || (a.key == b.key && a.row < b.row); }

}  // namespace

extern "C" {

int bbq_true_topk(const double *scores, int64_t n, const uint64_t *accept_bits, int64_t k, int32_t *out_idx, double *out_true, int64_t *out_n) {
  clear_error();
  if (!out_n) return fail(BBQ_ERR_INVALID_ARG, "bbq_true_topk: out_n is null");
  *out_n = 0;
  if (k < 0) return fail(BBQ_ERR_NEGATIVE_K, "k必须是非负数");
  if (n < 0 || n > 0x7fffffffLL) return fail(BBQ_ERR_INVALID_ARG, "bbq_true_topk: n out of range");
  if (n > 0 && !scores) return fail(BBQ_ERR_INVALID_ARG, "bbq_true_topk: scores is null");
  if (k == 0 || n == 0) return BBQ_OK;
  std::vector<KeyRow> r;
  try {
    for (int64_t i = 0; i < n; ++i) {
      if (accept_bits && !((accept_bits[i >> 6] >> (i & 63)) & 1ull)) continue;
      uint64_t bits;
      memcpy(&bits, scores + i, 8);
      r.push_back(KeyRow{true_key(bits, scores[i] != scores[i]), (int32_t)i});
    }
  } catch (const std::bad_alloc &) {
    return fail(BBQ_ERR_OOM, "bbq_true_topk: host memory for %lld rows", (long long)n);
  }
  const int64_t m = std::min<int64_t>(k, (int64_t)r.size());
  if (m == 0) return BBQ_OK;
  if (!out_idx || !out_true) return fail(BBQ_ERR_INVALID_ARG, "bbq_true_topk: output arrays are null");
  std::partial_sort(r.begin(), r.begin() + m, r.end(), ranks_first);  // a strict order: no two entries share a row
  for (int64_t j = 0; j < m; ++j) {
    const uint64_t bits = true_key_bits(r[j].key);  // a NaN as kTrueNaNBits
    out_idx[j] = r[j].row;
    memcpy(out_true + j, &bits, 8);
  }
  *out_n = m;
  return BBQ_OK;
}

int bbq_vectors_set_option(bbq_vectors *v, const char *name, int64_t value) {
  clear_error();
  if (!v || !name) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_set_option: null argument");
  if (strcmp(name, "exact_slab_rows") != 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_set_option: unknown option '%s'", name);
  if (value != 0 && (value < kExactSlabStep || value > kExactSlabMax || value % kExactSlabStep != 0))
    return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_set_option: exact_slab_rows is 0 or a multiple of %lld in %lld .. %lld, not %lld", (long long)kExactSlabStep,
                (long long)kExactSlabStep, (long long)kExactSlabMax, (long long)value);
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  v->opt_exact_slab_rows = value;
  return BBQ_OK;
}

int bbq_vectors_search_batch(bbq_vectors *v, const bbq_filter *f, int32_t n_queries, const float *queries, int32_t true_sim, int64_t k, int32_t *out_idx,
                             double *out_true, int64_t *out_n) {
  static const char fn[] = "bbq_vectors_search_batch";
  clear_error();
  if (true_sim < 0 || true_sim > 2) return fail(BBQ_ERR_INVALID_ARG, "不支持的相似性函数: %d", true_sim);  // needs no handle
  if (!v) return fail(BBQ_ERR_INVALID_ARG, "%s: vectors handle is null", fn);
  if (k < 0) return fail(BBQ_ERR_NEGATIVE_K, "k必须是非负数");
  if (n_queries < 0) return fail(BBQ_ERR_INVALID_ARG, "n_queries < 0");
  if (n_queries > 0 && !out_n) return fail(BBQ_ERR_INVALID_ARG, "%s: out_n is null", fn);
  if (f && (f->device != v->device || f->ctx != v->ctx)) return fail(BBQ_ERR_INVALID_ARG, "%s: the filter lives on another device than the vectors", fn);
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  HIPCHK(hipSetDevice(v->device));
  // under the lock: the rows the check sees are the rows the kernels read (an append or a compaction on another thread comes before or after)
  if (f && f->n_rows != v->n)
    return fail(BBQ_ERR_INVALID_ARG, "%s: the filter was made for %lld rows, the handle holds %lld", fn, (long long)f->n_rows, (long long)v->n);
  const int64_t n = v->n, accepted = f ? f->count : n;
  for (int32_t q = 0; q < n_queries; ++q) out_n[q] = 0;
  if (k == 0 || n_queries == 0 || accepted == 0) return BBQ_OK;
  const int64_t kk = std::min(k, accepted);
  if (kk > kMaxFastK)
    return fail(BBQ_ERR_UNSUPPORTED, "%s: min(k, accepted rows) = %lld is beyond %lld; score the rows with bbq_rerank_scores and rank them on the host", fn,
                (long long)kk, (long long)kMaxFastK);
  static_assert(kMaxFastK == kExactSelectMax, "the select pass takes what the call admits");
  if (!queries || !out_idx || !out_true) return fail(BBQ_ERR_INVALID_ARG, "%s: null argument", fn);

  const int32_t dim = v->dim;
  const int per = (int)std::min<int64_t>(kExactMaxQueries, n_queries);
  const int64_t n_up = (n + kExactSlabStep - 1) / kExactSlabStep * kExactSlabStep;
  int64_t S = v->opt_exact_slab_rows;
  if (S == 0) S = std::max(kExactSlabStep, std::min(kExactSlabMax, kExactScratchBytes / (8 * (int64_t)per) / kExactSlabStep * kExactSlabStep));
  S = std::min(S, n_up);
  const Layout big(per, kk, S, dim);
  // everything large, before anything is written to the caller's arrays
  {
    const hipError_t e = v->d_exact.reserve(big.bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "%s: %zu bytes of scratch: %s", fn, big.bytes, hipGetErrorString(e)); }
    const size_t back = big.lists_end - big.list_keys;
    if (v->h_exact_in.reserve(big.head_bytes) != hipSuccess || v->h_exact_out.reserve(back) != hipSuccess) {
      (void)hipGetLastError();
      return fail(BBQ_ERR_OOM, "%s: host staging for %zu + %zu bytes", fn, big.head_bytes, back);
    }
  }
  uint8_t *d = v->d_exact;
  hipStream_t st = v->ctx->aux_stream;

  for (int64_t q0 = 0; q0 < n_queries; q0 += per) {
    const int nq = (int)std::min<int64_t>(per, n_queries - q0);
    const Layout lo(nq, kk, S, dim);
    // a block's queries: column j's values side by side, widened (exactly) to f64, the padding slots 0.0; and each query's squared
    // norm, the reference's na chain: na += a * a in index order, the product exact in f64
    double *h_na = reinterpret_cast<double *>(v->h_exact_in.get() + lo.na);
    double *h_q = reinterpret_cast<double *>(v->h_exact_in.get() + lo.queries);
    for (int b0 = 0; b0 < nq; b0 += QB) {
      const int n_q = std::min(QB, nq - b0), tp = (n_q + QG - 1) / QG * QG;
      double *dst = h_q + (size_t)b0 * (size_t)dim;
      for (int t = 0; t < tp; ++t) {
        if (t >= n_q) {
          for (int32_t j = 0; j < dim; ++j) dst[(size_t)j * tp + t] = 0.0;
          h_na[b0 + t] = 0.0;
          continue;
        }
        const float *src = queries + (size_t)(q0 + b0 + t) * (size_t)dim;
        double na = 0.0;
        for (int32_t j = 0; j < dim; ++j) {
          const double a = (double)src[j];
          dst[(size_t)j * tp + t] = a;
          na += a * a;
        }
        h_na[b0 + t] = na;
      }
    }
    HIPCHK(hipMemcpyAsync(d, v->h_exact_in.get(), lo.head_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d + lo.list_count, 0, (size_t)nq * 4, st));

    ExactScoreArgs sa{};
    sa.vecs = v->d;
    sa.queries = reinterpret_cast<const double *>(d + lo.queries);
    sa.na = reinterpret_cast<const double *>(d + lo.na);
    sa.accept = f ? f->d_bits.get() : nullptr;
    sa.keys = reinterpret_cast<unsigned long long *>(d + lo.keys);
    sa.n = n;
    sa.stride = S;
    sa.n_queries = nq;
    sa.dim = dim;
    sa.sim = true_sim;
    ExactSelectArgs xa{};
    xa.keys = sa.keys;
    xa.accept = sa.accept;
    xa.list_keys = reinterpret_cast<unsigned long long *>(d + lo.list_keys);
    xa.list_rows = reinterpret_cast<int32_t *>(d + lo.list_rows);
    xa.list_count = reinterpret_cast<int32_t *>(d + lo.list_count);
    xa.n = n;
    xa.stride = S;
    xa.kk = (int32_t)kk;
    for (int64_t row0 = 0; row0 < n; row0 += S) {
      const int64_t rows = std::min(S, n - row0);
      sa.row0 = xa.row0 = row0;
      xa.rows = (int32_t)rows;
      HIPCHK(launch_exact_score(sa, rows, st));
      HIPCHK(launch_exact_select(xa, nq, st));
    }
    const size_t back = lo.lists_end - lo.list_keys;
    HIPCHK(hipMemcpyAsync(v->h_exact_out.get(), d + lo.list_keys, back, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // also: the staging is free for the next sub-batch
    const uint8_t *h = v->h_exact_out.get();
    const unsigned long long *h_keys = reinterpret_cast<const unsigned long long *>(h);
    const int32_t *h_rows = reinterpret_cast<const int32_t *>(h + (lo.list_rows - lo.list_keys));
    const int32_t *h_cnt = reinterpret_cast<const int32_t *>(h + (lo.list_count - lo.list_keys));
    for (int s = 0; s < nq; ++s)
      if (h_cnt[s] != kk) return fail(BBQ_ERR_HIP, "%s: query %lld kept %d of %lld rows", fn, (long long)(q0 + s), h_cnt[s], (long long)kk);
    for (int s = 0; s < nq; ++s) {
      int32_t *oi = out_idx + (q0 + s) * k;
      double *ot = out_true + (q0 + s) * k;
      for (int64_t j = 0; j < kk; ++j) {
        const uint64_t bits = true_key_bits(h_keys[(size_t)s * (size_t)kk + j]);  // a NaN as kTrueNaNBits
        oi[j] = h_rows[(size_t)s * (size_t)kk + j];
        memcpy(ot + j, &bits, 8);
      }
      out_n[q0 + s] = kk;
    }
  }
  return BBQ_OK;
}

}  // extern "C"
