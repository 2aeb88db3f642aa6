// bbq_span.cpp - span search: bbq_search_spans_batch, bbq_search_spans_filtered_batch (kernels: bbq_span_kernels.hip).  The host checks
// every span before the first launch, plans the call in sub-batches and allocates what the largest of them needs, then works through
// them: stage the queries, the span tables and the work items in one copy, launch the score pass and the select pass, bring back the
// answer blocks in one copy, and end as every select-pass search does (finish_selected, bbq_select.cpp): what the device selected is
// proven, the reference's heap replayed over the scores of the other queries.  With a row filter the same call is planned in ACCEPTED rows, counted from the filter's host copy: a query's length is the
// number of accepted rows in its spans, an item's `out` the position of its first accepted row among them, an item without an accepted
// row is not staged, and the device leaves each accepted row's ord beside its score - the ords a replay offers to the heap.
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include "bbq_search.h"

using namespace bbq;

namespace {

// A sub-batch takes at most this many queries and this many bytes of scores (filtered: of scores and ords), and always at least one
// query: a query whose spans hold more rows than that has a sub-batch of its own.  A score launch takes at most kSpanMaxItems work items (the grid's x extent in
// work-items is a 32-bit count).  The scratch is the context's (DeviceCtx::d_span) and only grows.
constexpr int kSpanMaxQueries = 1024;
constexpr int64_t kSpanScoreBytes = 64ll << 20;
constexpr int64_t kSpanMaxItems = 1 << 22;
static_assert((uint64_t)kSpanMaxItems * kChunkRows <= kGridWorkItemsMax, "one score launch");

// work items of the non-empty span [b, e): cut at kChunkRows-row steps from the start of b's tile
inline int64_t items_of_span(int64_t b, int64_t e) { return (e - (b & ~(int64_t)(kTileRows - 1)) + kChunkRows - 1) / kChunkRows; }

// accepted rows of [b, e), b < e: the words of the filter's host copy, the two edge words masked to the span
inline int64_t accepted_rows(const uint64_t *bits, int64_t b, int64_t e) {
  const int64_t w0 = b >> 6, w1 = (e - 1) >> 6;
  const uint64_t lo = ~0ull << (b & 63), hi = ~0ull >> (63 - ((e - 1) & 63));
  if (w0 == w1) return __builtin_popcountll(bits[w0] & lo & hi);
  int64_t n = __builtin_popcountll(bits[w0] & lo) + __builtin_popcountll(bits[w1] & hi);
  for (int64_t w = w0 + 1; w < w1; ++w) n += __builtin_popcountll(bits[w]);
  return n;
}

// the cuts of the non-empty span [sb, se), at kChunkRows-row steps from the start of sb's tile, in order: fn(row_lo, row_hi)
template <class Fn>
inline void for_each_cut(int64_t sb, int64_t se, Fn fn) {
  for (int64_t r0 = sb & ~(int64_t)(kTileRows - 1); r0 < se; r0 += kChunkRows) fn(std::max(r0, sb), std::min(r0 + kChunkRows, se));
}

// the work items of the non-empty span [sb, se) in order: fn(row_lo, row_hi, rows), rows = the rows of the item the call visits - all
// of them without a filter; with one the accepted ones, read from `acc` (one count per cut, in call order; advanced), and then a cut
// without an accepted row is no item
template <class Fn>
inline void for_each_item(int64_t sb, int64_t se, const uint16_t *&acc, Fn fn) {
  for_each_cut(sb, se, [&](int64_t r_lo, int64_t r_hi) {
    const int64_t rows = acc ? *acc++ : r_hi - r_lo;
    if (rows > 0) fn(r_lo, r_hi, rows);
  });
}
static_assert(kChunkRows <= 65535, "a cut's accepted rows as 16 bits");

// what a sub-batch of the call holds
struct SubBatch {
  int64_t q0 = 0;
  int nq = 0;
  int64_t n_items = 0, n_runs = 0, n_sel = 0, n_scores = 0;
};

// where a sub-batch keeps what in the scratch: [query data | query uniforms | selected queries | runs | items] come from the host in one
// copy, the answer blocks go back in one, the scores - and the ords of a filtered call - stay unless a query's heap is replayed
struct Layout {
  size_t qdata, qparams, sel, runs, items, head_bytes, out, scores, ords, bytes;
  Layout(const SubBatch &b, size_t qb, size_t out_stride, bool filtered) {
    qdata = 0;
    qparams = qdata + (size_t)b.nq * qb;
    sel = qparams + (size_t)b.nq * sizeof(QueryParams);
    runs = sel + (size_t)b.n_sel * sizeof(SpanQuery);
    items = runs + (size_t)b.n_runs * sizeof(SpanRun);
    head_bytes = items + (size_t)b.n_items * sizeof(SpanItem);
    out = align16(head_bytes);
    scores = align16(out + (size_t)b.n_sel * out_stride * 8);
    ords = align16(scores + (size_t)b.n_scores * 4);
    bytes = filtered ? ords + (size_t)b.n_scores * 4 : scores + (size_t)b.n_scores * 4;
  }
};
static_assert(sizeof(SpanQuery) == 32 && sizeof(SpanRun) == 16 && sizeof(QueryParams) % 16 == 0, "every staged array starts 8-byte aligned");

// every span of every query, in call order: inside the index, begin <= end, ascending and disjoint within a query.  len[q] = its rows
int check_spans(const char *fn, int32_t n_queries, const int64_t *off, const int64_t *spans, int64_t n_rows, std::vector<int64_t> &len) {
  len.assign((size_t)n_queries, 0);
  for (int32_t q = 0; q < n_queries; ++q) {
    int64_t prev_end = 0;
    for (int64_t j = off[q]; j < off[q + 1]; ++j) {
      const int64_t b = spans[2 * j], e = spans[2 * j + 1];
      if (b < 0 || e < b || e > n_rows)
        return fail(BBQ_ERR_INVALID_ARG, "%s: query %d, span %lld: [%lld, %lld) is no span of an index of %lld rows", fn, q,
                    (long long)(j - off[q]), (long long)b, (long long)e, (long long)n_rows);
      if (j > off[q] && b < prev_end)
        return fail(BBQ_ERR_INVALID_ARG, "%s: query %d, span %lld: [%lld, %lld) begins in front of the end of the span before it (%lld); spans ascend and do not overlap",
                    fn, q, (long long)(j - off[q]), (long long)b, (long long)e, (long long)prev_end);
      prev_end = e;
      len[(size_t)q] += e - b;
    }
  }
  return BBQ_OK;
}

// does the select pass run for a query of `len` rows (filtered: accepted rows)?
inline bool selected(int64_t len, int64_t k) { return k >= 1 && k <= kSpanSelectMax && len > k; }

// the call behind its argument checks, under the context's lock.  f: the row filter, or null - every row; fn: the entry point's name
int spans_locked(const char *fn, bbq_index *ix, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t k,
                 const int64_t *off, const int64_t *spans, int32_t *out_idx, float *out_score, int64_t *out_n, uint8_t *out_status) {
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  // under the lock: the rows the check sees are the rows the kernel reads (an append or a compaction on another thread comes before or after)
  if (f && (f->device != ix->device || f->n_rows != ix->main.view.n_rows))
    return fail(BBQ_ERR_INVALID_ARG, "%s: the filter was made for an index of %lld rows on device %d, this one has %lld rows on device %d", fn,
                (long long)f->n_rows, f->device, (long long)ix->main.view.n_rows, ix->device);
  std::vector<int64_t> len;
  int rc = check_spans(fn, n_queries, off, spans, ix->main.view.n_rows, len);
  if (rc != BBQ_OK) return rc;
  int64_t longest = 0;
  for (int32_t q = 0; q < n_queries; ++q) longest = std::max(longest, len[(size_t)q]);
  if (k > 0 && longest > 0 && (!out_idx || !out_score)) return fail(BBQ_ERR_INVALID_ARG, "%s: null output", fn);
  std::vector<uint16_t> cut_acc;  // filtered: the accepted rows of every cut of every non-empty span, in call order - counted once
  if (f && k > 0) {               // from here on a query's length is A_q, the accepted rows of its spans
    const uint64_t *bits = f->h_bits.data();
    longest = 0;
    for (int32_t q = 0; q < n_queries; ++q) {
      int64_t a = 0;
      for (int64_t j = off[q]; j < off[q + 1]; ++j)
        if (spans[2 * j + 1] > spans[2 * j])
          for_each_cut(spans[2 * j], spans[2 * j + 1], [&](int64_t r_lo, int64_t r_hi) {
            cut_acc.push_back((uint16_t)accepted_rows(bits, r_lo, r_hi));
            a += cut_acc.back();
          });
      longest = std::max(longest, len[(size_t)q] = a);
    }
  }
  if (k == 0 || longest == 0) {  // nothing to score
    for (int32_t q = 0; q < n_queries; ++q) out_n[q] = 0;
    if (out_status) memset(out_status, 0, (size_t)n_queries);
    return BBQ_OK;
  }

  const int one_bit = query_bits == 1 ? 1 : 0;
  const int planes = planes_of_call(ix, qquant, (int64_t)n_queries * ix->geom.dim, one_bit);
  const size_t qb = (size_t)query_data_bytes(ix, planes);
  const size_t out_stride = (size_t)std::min<int64_t>(k, kSpanSelectMax) + 2;

  // the plan: sub-batches, and the largest of everything they need
  const int64_t row_bytes = f ? 8 : 4;  // of scratch per visited row: its score, and with a filter its ord
  std::vector<SubBatch> subs;
  size_t max_bytes = 0, max_head = 0, max_back = 0;
  int64_t max_scores = 0;
  const uint16_t *acc = f ? cut_acc.data() : nullptr;
  for (int64_t q = 0; q < n_queries;) {
    SubBatch b;
    b.q0 = q;
    while (q < n_queries && b.nq < kSpanMaxQueries && (b.nq == 0 || (b.n_scores + len[(size_t)q]) * row_bytes <= kSpanScoreBytes)) {
      const int64_t L = len[(size_t)q];
      for (int64_t j = off[q]; j < off[q + 1]; ++j)
        if (spans[2 * j + 1] > spans[2 * j]) {
          if (f) for_each_item(spans[2 * j], spans[2 * j + 1], acc, [&](int64_t, int64_t, int64_t) { ++b.n_items; });
          else b.n_items += items_of_span(spans[2 * j], spans[2 * j + 1]);
          if (!f && selected(L, k)) ++b.n_runs;
        }
      if (selected(L, k)) ++b.n_sel;
      b.n_scores += L;
      ++b.nq;
      ++q;
    }
    const Layout lo(b, qb, out_stride, f != nullptr);
    max_bytes = std::max(max_bytes, lo.bytes);
    max_head = std::max(max_head, lo.head_bytes);
    max_back = std::max(max_back, (size_t)b.n_sel * out_stride);
    max_scores = std::max(max_scores, b.n_scores);
    subs.push_back(b);
  }
  // everything large, before anything is written to the caller's arrays
  rc = reserve_scratch(ix->ctx->d_span, max_bytes, "span search");
  if (rc != BBQ_OK) return rc;
  std::unique_ptr<uint8_t[]> head(new (std::nothrow) uint8_t[std::max<size_t>(max_head, 1)]);
  std::unique_ptr<uint64_t[]> back(new (std::nothrow) uint64_t[std::max<size_t>(max_back, 1)]);
  std::unique_ptr<float[]> h_scores(new (std::nothrow) float[(size_t)std::max<int64_t>(max_scores, 1)]);  // touched only where a heap is replayed
  std::unique_ptr<uint32_t[]> h_ords(new (std::nothrow) uint32_t[(size_t)std::max<int64_t>(f ? max_scores : 0, 1)]);  // the same
  if (!head || !back || !h_scores || !h_ords)
    return fail(BBQ_ERR_OOM, "span search: host staging for %zu + %zu + %lld bytes", max_head, max_back * 8, (long long)(max_scores * row_bytes));

  uint8_t *d = ix->ctx->d_span;
  hipStream_t st = ix->ctx->aux_stream;
  SpanScoreArgs sa{};
  sa.idx = main_launch_view(ix);
  sa.accept = f ? f->d_bits.get() : nullptr;
  std::vector<SelectQuery> sq;  // per query of the sub-batch: its rows, where its scores start, its block among the selected or -1
  SelectTail t{};
  t.back = back.get();
  t.h_scores = h_scores.get();
  t.h_ords = h_ords.get();
  t.k = k;
  t.out_stride = out_stride;
  t.stream = st;
  t.threads = ix->opt_replay_threads;

  acc = f ? cut_acc.data() : nullptr;
  for (const SubBatch &b : subs) {
    const Layout lo(b, qb, out_stride, f != nullptr);
    SpanQuery *h_sel = reinterpret_cast<SpanQuery *>(head.get() + lo.sel);
    SpanRun *h_runs = reinterpret_cast<SpanRun *>(head.get() + lo.runs);
    SpanItem *h_items = reinterpret_cast<SpanItem *>(head.get() + lo.items);
    sq.resize((size_t)b.nq);
    int64_t n_items = 0, n_runs = 0, n_sel = 0, n_scores = 0;
    for (int s = 0; s < b.nq; ++s) {
      const int64_t q = b.q0 + s, L = len[(size_t)q];
      fill_query(ix, head.get() + lo.qdata + (size_t)s * qb, reinterpret_cast<QueryParams *>(head.get() + lo.qparams) + s,
                 qquant + (size_t)q * ix->geom.dim, qcorr + (size_t)q * 4, planes, one_bit, sim);
      const bool sel = selected(L, k);
      sq[(size_t)s] = SelectQuery{L, n_scores, sel ? (int32_t)n_sel : -1};
      if (sel) h_sel[n_sel++] = SpanQuery{n_scores, L, n_runs, 0, 0};
      int64_t pos = 0;  // of the next item's first visited row in the query's (filtered: compacted) visiting order
      for (int64_t j = off[q]; j < off[q + 1]; ++j) {
        const int64_t sb = spans[2 * j], se = spans[2 * j + 1];
        if (se <= sb) continue;
        if (sel && !f) {
          h_runs[n_runs++] = SpanRun{pos, sb};
          ++h_sel[n_sel - 1].n_runs;
        }
        for_each_item(sb, se, acc, [&](int64_t r_lo, int64_t r_hi, int64_t rows) {
          h_items[n_items++] = SpanItem{(uint32_t)s, (uint32_t)(r_lo >> 6), (uint32_t)r_lo, (uint32_t)r_hi, n_scores + pos};
          pos += rows;
        });
      }
      n_scores += L;
    }

    if (n_scores > 0) {
      HIPCHK(hipMemcpyAsync(d, head.get(), lo.head_bytes, hipMemcpyHostToDevice, st));
      sa.qplanes = reinterpret_cast<const uint4 *>(d + lo.qdata);
      sa.qparams = reinterpret_cast<const QueryParams *>(d + lo.qparams);
      sa.scores = reinterpret_cast<float *>(d + lo.scores);
      sa.ords = f ? reinterpret_cast<uint32_t *>(d + lo.ords) : nullptr;
      for (int64_t i0 = 0; i0 < n_items; i0 += kSpanMaxItems) {
        sa.items = reinterpret_cast<const SpanItem *>(d + lo.items) + i0;
        HIPCHK(launch_span_score(sa, planes, std::min(kSpanMaxItems, n_items - i0), st));
      }
      if (n_sel > 0) {
        SpanSelectArgs se{};
        se.scores = sa.scores;
        se.sel = reinterpret_cast<const SpanQuery *>(d + lo.sel);
        se.runs = reinterpret_cast<const SpanRun *>(d + lo.runs);
        se.ords = sa.ords;
        se.out = reinterpret_cast<uint64_t *>(d + lo.out);
        se.k = (int32_t)k;
        se.out_stride = (int32_t)out_stride;
        HIPCHK(launch_span_select(se, (int)n_sel, st));
        HIPCHK(hipMemcpyAsync(back.get(), d + lo.out, (size_t)n_sel * out_stride * 8, hipMemcpyDeviceToHost, st));
      }
      HIPCHK(hipStreamSynchronize(st));  // also: the staging is free for the next sub-batch
    }

    // what the device selected is proven or replayed (bbq_select.cpp); without a filter the rows of a replayed query are its spans
    t.queries = sq.data();
    t.nq = b.nq;
    t.d_scores = sa.scores;
    t.d_ords = sa.ords;
    t.out_tag = out_idx + b.q0 * k;
    t.out_score = out_score + b.q0 * k;
    t.out_n = out_n + b.q0;
    t.out_status = out_status ? out_status + b.q0 : nullptr;
    rc = finish_selected(t, [&](int64_t s, const float *sc, HeapReplay &hr) {
      for (int64_t j = off[b.q0 + s]; j < off[b.q0 + s + 1]; ++j)
        for (int64_t r = spans[2 * j]; r < spans[2 * j + 1]; ++r) hr.offer(*sc++, (int32_t)r);
    });
    if (rc != BBQ_OK) return rc;
  }
  return BBQ_OK;
}

// the argument checks that need no lock, then the call
int spans_entry(const char *fn, bbq_index *ix, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                int64_t k, const int64_t *span_offsets, const int64_t *spans, int32_t *out_idx, float *out_score, int64_t *out_n, uint8_t *out_status) {
  clear_error();
  const int rc = validate_query_args(ix, n_queries, qquant, qcorr, query_bits, sim, k);
  if (rc != BBQ_OK) return rc;
  if (ix->multi) return fail(BBQ_ERR_UNSUPPORTED, "span search is not supported on a multi-device index");
  if (ix->has_pilot || ix->row_base != 0) return fail(BBQ_ERR_UNSUPPORTED, "span search is not supported on a row shard or an index with a pilot replica");
  if (n_queries == 0) return BBQ_OK;
  if (!span_offsets) return fail(BBQ_ERR_INVALID_ARG, "%s: span_offsets is null", fn);
  if (span_offsets[0] != 0) return fail(BBQ_ERR_INVALID_ARG, "%s: span_offsets[0] must be 0", fn);
  for (int32_t q = 0; q < n_queries; ++q)
    if (span_offsets[q + 1] < span_offsets[q]) return fail(BBQ_ERR_INVALID_ARG, "%s: span_offsets must ascend", fn);
  if (span_offsets[n_queries] > 0 && !spans) return fail(BBQ_ERR_INVALID_ARG, "%s: spans is null", fn);
  if (!out_n) return fail(BBQ_ERR_INVALID_ARG, "%s: out_n is null", fn);
  return spans_locked(fn, ix, f, n_queries, qquant, qcorr, query_bits, sim, k, span_offsets, spans, out_idx, out_score, out_n, out_status);
}

}  // namespace

extern "C" {

int bbq_search_spans_batch(bbq_index *ix, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t k,
                           const int64_t *span_offsets, const int64_t *spans, int32_t *out_idx, float *out_score, int64_t *out_n, uint8_t *out_status) {
  return spans_entry("bbq_search_spans_batch", ix, nullptr, n_queries, qquant, qcorr, query_bits, sim, k, span_offsets, spans, out_idx, out_score, out_n, out_status);
}

int bbq_search_spans_filtered_batch(bbq_index *ix, const bbq_filter *f, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits,
                                    int32_t sim, int64_t k, const int64_t *span_offsets, const int64_t *spans, int32_t *out_idx, float *out_score,
                                    int64_t *out_n, uint8_t *out_status) {
  return spans_entry("bbq_search_spans_filtered_batch", ix, f, n_queries, qquant, qcorr, query_bits, sim, k, span_offsets, spans, out_idx, out_score, out_n,
                     out_status);
}

}  // extern "C"
