// bbq_exact.cpp - exact search: bbq_true_topk, bbq_exact_bound, bbq_vectors_search_batch, bbq_vectors_set_option, bbq_vectors_exact_stats
// (kernels: bbq_exact_kernels.hip, bbq_exact_prefilter_kernels.hip).
// The true top-k of raw fp32 queries over the rows a bbq_vectors keeps in HBM - the reference's getTrueTopK (tests/recall-common.ts:143-149)
// - scored and selected on the device: a sub-batch of at most 1024 queries is widened to f64 and staged in one copy, the rows are worked
// through a slab at a time - the score pass leaves a slab's keys, the select pass folds them into each query's running list - and the
// lists, k x (row, key) a query, are the only thing that comes back.
// With the prefilter the slab's pass is the f32 one on the matrix cores: it leaves every pair's interval, the select pass keeps the
// k-th largest lower end, the compaction keeps the rows whose upper end reaches it, and only those run the f64 chain
// (bbq_rerank_kernel) behind the last slab; they are ranked here.  A query with more survivors than its list holds sends its
// sub-batch through the f64 sweep: the answer is the same either way.
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
static_assert(kExactSlabStep % kExactPreRows == 0, "a slab is whole prefilter tiles");
// what exact_prefilter -1 means per similarity (EUCLIDEAN, COSINE, MAXIMUM_INNER_PRODUCT): on only where every measured leg won
// (README "Exact search")
constexpr bool kExactPrefilterDefault[3] = {false, false, false};

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

// where a sub-batch of nq queries that keeps kk rows a query and works in slabs of S rows keeps what: [squared norms | queries] come from
// the host in one copy, [list keys | list rows | list counts] go back in one.  Behind them the prefilter's: the upper ends' keys,
// [sides | raw queries] from the host in one copy, the survivors' [counts | scores | rows]
struct Layout {
  size_t na, queries, head_bytes, list_keys, list_rows, list_count, lists_end, keys, bytes;
  size_t hi_keys, sides, raw, pre_end, surv_count, surv_scores, surv_rows;
  int64_t slots, cap;
  Layout(int nq, int64_t kk, int64_t S, int32_t dim, bool pre) {
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
    cap = exact_survivor_cap(kk);
    hi_keys = bytes;
    sides = align256(hi_keys + (size_t)nq * (size_t)S * 8);
    raw = sides + (size_t)nq * sizeof(ExactSide);
    pre_end = raw + (size_t)nq * (size_t)dim * 4;
    surv_count = align16(pre_end);
    surv_scores = align16(surv_count + (size_t)nq * 4);
    surv_rows = surv_scores + (size_t)nq * (size_t)cap * 8;
    if (pre) bytes = surv_rows + (size_t)nq * (size_t)cap * 4;
  }
};

struct KeyRow {
  unsigned long long key;
  int32_t row;
};
inline bool ranks_first(const KeyRow &a, const KeyRow &b) { return a.key > b.key || (a.key == b.key && a.row < b.row); }

const char fn[] = "bbq_vectors_search_batch";

// one call behind its checks
struct Call {
  bbq_vectors *v;
  const bbq_filter *f;
  const float *queries;
  int32_t true_sim;
  int64_t k, kk, S, accepted;
  int32_t *out_idx;
  double *out_true;
  int64_t *out_n;
  hipStream_t st;
};

void write_answer(const Call &c, int64_t q, const KeyRow *best) {
  int32_t *oi = c.out_idx + q * c.k;
  double *ot = c.out_true + q * c.k;
  for (int64_t j = 0; j < c.kk; ++j) {
    const uint64_t bits = true_key_bits(best[j].key);  // a NaN as kTrueNaNBits
    oi[j] = best[j].row;
    memcpy(ot + j, &bits, 8);
  }
  c.out_n[q] = c.kk;
}

// the f64 sweep: every (query, accepted row) pair through the chain, the lists selected on the device
int sweep_f64(const Call &c, int64_t q0, int nq) {
  bbq_vectors *v = c.v;
  const int32_t dim = v->dim;
  const int64_t n = v->n, kk = c.kk, S = c.S;
  uint8_t *d = v->d_exact;
  hipStream_t st = c.st;
  const Layout lo(nq, kk, S, dim, false);
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
      const float *src = c.queries + (size_t)(q0 + b0 + t) * (size_t)dim;
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
  sa.accept = c.f ? c.f->d_bits.get() : nullptr;
  sa.keys = reinterpret_cast<unsigned long long *>(d + lo.keys);
  sa.n = n;
  sa.stride = S;
  sa.n_queries = nq;
  sa.dim = dim;
  sa.sim = c.true_sim;
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
    int32_t *oi = c.out_idx + (q0 + s) * c.k;
    double *ot = c.out_true + (q0 + s) * c.k;
    for (int64_t j = 0; j < kk; ++j) {
      const uint64_t bits = true_key_bits(h_keys[(size_t)s * (size_t)kk + j]);  // a NaN as kTrueNaNBits
      oi[j] = h_rows[(size_t)s * (size_t)kk + j];
      memcpy(ot + j, &bits, 8);
    }
    c.out_n[q0 + s] = kk;
  }
  v->exact_stats[1] += (int64_t)nq * c.accepted;
  v->exact_stats[3] = std::max(v->exact_stats[3], c.accepted);
  return BBQ_OK;
}

// the prefiltered sweep.  *overflow: a query's survivors did not fit - nothing was answered, the f64 sweep serves the sub-batch
int sweep_prefiltered(const Call &c, int64_t q0, int nq, bool *overflow) {
  bbq_vectors *v = c.v;
  const int32_t dim = v->dim;
  const int64_t n = v->n, kk = c.kk, S = c.S;
  uint8_t *d = v->d_exact;
  hipStream_t st = c.st;
  const Layout lo(nq, kk, S, dim, true);
  const int64_t cap = lo.cap;
  *overflow = false;
  // the queries as they are, and what each contributes to an interval: its f32 sum of squares, summed here in index order
  ExactSide *h_sides = reinterpret_cast<ExactSide *>(v->h_exact_in.get());
  float *h_raw = reinterpret_cast<float *>(v->h_exact_in.get() + (lo.raw - lo.sides));
  const float *src = c.queries + (size_t)q0 * (size_t)dim;
  memcpy(h_raw, src, (size_t)nq * (size_t)dim * 4);
  for (int s = 0; s < nq; ++s) {
    float qq = 0.f;
    for (int32_t j = 0; j < dim; ++j) qq += src[(size_t)s * dim + j] * src[(size_t)s * dim + j];
    h_sides[s] = exact_side(dim, qq);
  }
  HIPCHK(hipMemcpyAsync(d + lo.sides, v->h_exact_in.get(), lo.pre_end - lo.sides, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d + lo.list_count, 0, (size_t)nq * 4, st));
  HIPCHK(hipMemsetAsync(d + lo.surv_count, 0, (size_t)nq * 4, st));

  ExactPrefilterArgs pa{};
  pa.vecs = v->d;
  pa.queries = reinterpret_cast<const float *>(d + lo.raw);
  pa.sides = reinterpret_cast<const ExactSide *>(d + lo.sides);
  pa.accept = c.f ? c.f->d_bits.get() : nullptr;
  pa.lo_keys = reinterpret_cast<unsigned long long *>(d + lo.keys);
  pa.hi_keys = reinterpret_cast<unsigned long long *>(d + lo.hi_keys);
  pa.n = n;
  pa.stride = S;
  pa.n_queries = nq;
  pa.dim = dim;
  pa.sim = c.true_sim;
  ExactSelectArgs xa{};
  xa.keys = pa.lo_keys;
  xa.accept = pa.accept;
  xa.list_keys = reinterpret_cast<unsigned long long *>(d + lo.list_keys);
  xa.list_rows = reinterpret_cast<int32_t *>(d + lo.list_rows);
  xa.list_count = reinterpret_cast<int32_t *>(d + lo.list_count);
  xa.n = n;
  xa.stride = S;
  xa.kk = (int32_t)kk;
  ExactCompactArgs ca{};
  ca.hi_keys = pa.hi_keys;
  ca.accept = pa.accept;
  ca.list_keys = xa.list_keys;
  ca.list_count = xa.list_count;
  ca.surv_rows = reinterpret_cast<int32_t *>(d + lo.surv_rows);
  ca.surv_count = reinterpret_cast<int32_t *>(d + lo.surv_count);
  ca.n = n;
  ca.stride = S;
  ca.kk = (int32_t)kk;
  ca.cap = (int32_t)cap;
  for (int64_t row0 = 0; row0 < n; row0 += S) {
    const int64_t rows = std::min(S, n - row0);
    pa.row0 = xa.row0 = ca.row0 = row0;
    xa.rows = ca.rows = (int32_t)rows;
    HIPCHK(launch_exact_prefilter(pa, rows, st));
    HIPCHK(launch_exact_select(xa, nq, st));
    HIPCHK(launch_exact_compact(ca, nq, st));
  }
  uint8_t *h = v->h_exact_out.get();
  HIPCHK(hipMemcpyAsync(h, d + lo.surv_count, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  v->exact_stats[0] += (int64_t)nq * c.accepted;
  const int32_t *h_cnt = reinterpret_cast<const int32_t *>(h);
  int64_t longest = 0, total = 0;
  for (int s = 0; s < nq; ++s) {
    if (h_cnt[s] > cap) {
      *overflow = true;
      return BBQ_OK;
    }
    if (h_cnt[s] < kk) return fail(BBQ_ERR_HIP, "%s: query %lld kept %d of %lld rows", fn, (long long)(q0 + s), h_cnt[s], (long long)kk);
    longest = std::max<int64_t>(longest, h_cnt[s]);
    total += h_cnt[s];
  }
  // the survivors' f64 chains, the rerank's kernel over lists of a fixed stride
  RerankArgs ra{};
  ra.vecs = v->d;
  ra.n = n;
  ra.dim = dim;
  ra.sim = c.true_sim;
  ra.queries = pa.queries;
  ra.rows = ca.surv_rows;
  ra.out = reinterpret_cast<double *>(d + lo.surv_scores);
  ra.counts = ca.surv_count;
  ra.stride = cap;
  HIPCHK(launch_rerank(ra, nq, longest, st));
  double *h_scores = reinterpret_cast<double *>(h + align16((size_t)nq * 4));
  int32_t *h_rows = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(h_scores) + (size_t)nq * (size_t)longest * 8);
  HIPCHK(hipMemcpy2DAsync(h_scores, (size_t)longest * 8, ra.out, (size_t)cap * 8, (size_t)longest * 8, (size_t)nq, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpy2DAsync(h_rows, (size_t)longest * 4, ra.rows, (size_t)cap * 4, (size_t)longest * 4, (size_t)nq, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<KeyRow> r;
  try {
    r.reserve((size_t)longest);
  } catch (const std::bad_alloc &) {
    return fail(BBQ_ERR_OOM, "%s: host memory for %lld survivors", fn, (long long)longest);
  }
  for (int s = 0; s < nq; ++s) {
    r.clear();
    for (int32_t i = 0; i < h_cnt[s]; ++i) {
      const double x = h_scores[(size_t)s * (size_t)longest + i];
      uint64_t bits;
      memcpy(&bits, &x, 8);
      r.push_back(KeyRow{true_key(bits, x != x), h_rows[(size_t)s * (size_t)longest + i]});
    }
    std::partial_sort(r.begin(), r.begin() + kk, r.end(), ranks_first);  // a strict order: a row survives once
    write_answer(c, q0 + s, r.data());
    v->exact_stats[3] = std::max<int64_t>(v->exact_stats[3], h_cnt[s]);
  }
  v->exact_stats[1] += total;
  return BBQ_OK;
}

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

int bbq_exact_bound(int32_t dim, int32_t true_sim, float dot, float query_sumsq, float row_sumsq, double *out_lo, double *out_hi) {
  clear_error();
  if (!out_lo || !out_hi) return fail(BBQ_ERR_INVALID_ARG, "bbq_exact_bound: null argument");
  if (dim < 1) return fail(BBQ_ERR_INVALID_ARG, "bbq_exact_bound: dim < 1");
  if (true_sim < 0 || true_sim > 2) return fail(BBQ_ERR_INVALID_ARG, "不支持的相似性函数: %d", true_sim);
  if (!exact_prefilter_serves(true_sim)) return fail(BBQ_ERR_UNSUPPORTED, "bbq_exact_bound: EUCLIDEAN has no interval; the exact search scores it in f64 alone");
  exact_interval(dim, true_sim, (double)dot, exact_side(dim, query_sumsq), exact_side(dim, row_sumsq), out_lo, out_hi);
  return BBQ_OK;
}

int bbq_vectors_set_option(bbq_vectors *v, const char *name, int64_t value) {
  clear_error();
  if (!v || !name) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_set_option: null argument");
  if (strcmp(name, "exact_prefilter") == 0) {
    if (value < -1 || value > 1) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_set_option: exact_prefilter is -1, 0 or 1, not %lld", (long long)value);
    std::lock_guard<std::mutex> lk(v->ctx->mu);
    v->opt_exact_prefilter = value;
    return BBQ_OK;
  }
  if (strcmp(name, "exact_slab_rows") != 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_set_option: unknown option '%s'", name);
  if (value != 0 && (value < kExactSlabStep || value > kExactSlabMax || value % kExactSlabStep != 0))
    return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_set_option: exact_slab_rows is 0 or a multiple of %lld in %lld .. %lld, not %lld", (long long)kExactSlabStep,
                (long long)kExactSlabStep, (long long)kExactSlabMax, (long long)value);
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  v->opt_exact_slab_rows = value;
  return BBQ_OK;
}

int bbq_vectors_exact_stats(bbq_vectors *v, int64_t out[4]) {
  clear_error();
  if (!v || !out) return fail(BBQ_ERR_INVALID_ARG, "bbq_vectors_exact_stats: null argument");
  std::lock_guard<std::mutex> lk(v->ctx->mu);
  for (int i = 0; i < 4; ++i) out[i] = v->exact_stats[i];
  return BBQ_OK;
}

int bbq_vectors_search_batch(bbq_vectors *v, const bbq_filter *f, int32_t n_queries, const float *queries, int32_t true_sim, int64_t k, int32_t *out_idx,
                             double *out_true, int64_t *out_n) {
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
  for (int i = 0; i < 4; ++i) v->exact_stats[i] = 0;
  if (k == 0 || n_queries == 0 || accepted == 0) return BBQ_OK;
  const int64_t kk = std::min(k, accepted);
  if (kk > kMaxFastK)
    return fail(BBQ_ERR_UNSUPPORTED, "%s: min(k, accepted rows) = %lld is beyond %lld; score the rows with bbq_rerank_scores and rank them on the host", fn,
                (long long)kk, (long long)kMaxFastK);
  static_assert(kMaxFastK == kExactSelectMax, "the select pass takes what the call admits");
  if (!queries || !out_idx || !out_true) return fail(BBQ_ERR_INVALID_ARG, "%s: null argument", fn);

  const int32_t dim = v->dim;
  const bool pre = exact_prefilter_serves(true_sim) && (v->opt_exact_prefilter == 1 || (v->opt_exact_prefilter < 0 && kExactPrefilterDefault[true_sim]));
  const int per = (int)std::min<int64_t>(kExactMaxQueries, n_queries);
  const int64_t n_up = (n + kExactSlabStep - 1) / kExactSlabStep * kExactSlabStep;
  int64_t S = v->opt_exact_slab_rows;
  const int64_t pair_bytes = pre ? 16 : 8;  // a pair's key, or the keys of its interval's two ends
  if (S == 0) S = std::max(kExactSlabStep, std::min(kExactSlabMax, kExactScratchBytes / (pair_bytes * (int64_t)per) / kExactSlabStep * kExactSlabStep));
  S = std::min(S, n_up);
  const Layout big(per, kk, S, dim, pre);
  // everything large, before anything is written to the caller's arrays
  {
    const hipError_t e = v->d_exact.reserve(big.bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "%s: %zu bytes of scratch: %s", fn, big.bytes, hipGetErrorString(e)); }
    size_t in = big.head_bytes, back = big.lists_end - big.list_keys;
    if (pre) {
      in = std::max(in, big.pre_end - big.sides);
      back = std::max(back, align16((size_t)per * 4) + (size_t)per * (size_t)big.cap * 12);
    }
    if (v->h_exact_in.reserve(in) != hipSuccess || v->h_exact_out.reserve(back) != hipSuccess) {
      (void)hipGetLastError();
      return fail(BBQ_ERR_OOM, "%s: host staging for %zu + %zu bytes", fn, in, back);
    }
  }
  const Call c{v, f, queries, true_sim, k, kk, S, accepted, out_idx, out_true, out_n, v->ctx->aux_stream};
  for (int64_t q0 = 0; q0 < n_queries; q0 += per) {
    const int nq = (int)std::min<int64_t>(per, n_queries - q0);
    bool overflow = !pre;
    if (pre) {
      const int rc = sweep_prefiltered(c, q0, nq, &overflow);
      if (rc != BBQ_OK) return rc;
      if (overflow) ++v->exact_stats[2];
    }
    if (overflow) {
      const int rc = sweep_f64(c, q0, nq);
      if (rc != BBQ_OK) return rc;
    }
  }
  return BBQ_OK;
}

}  // extern "C"
