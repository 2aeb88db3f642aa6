// bbq_filter.cpp - the accept set of a filtered search (bbq_filter_*, include/bbq.h): one bit per row of ONE index, resident on that
// index's device in the layout the sweep reads it in - word t = tile t, bit l = lane l, so a wave's 64 rows are one word - and the
// host-side summary the accepted-space plan is built from (build_filtered_plan, bbq_core.cpp).  Read-only after creation.
#include <memory>
#include "bbq_search.h"

using namespace bbq;

namespace {

// what a filter can be made for: a single-device root index (DESIGN.md "Filtered search", out of scope)
int check_filter_index(const bbq_index *ix) {
  if (ix->multi) return fail(BBQ_ERR_UNSUPPORTED, "filtered search is not supported on a multi-device index");
  if (ix->has_pilot || ix->row_base != 0) return fail(BBQ_ERR_UNSUPPORTED, "filtered search is not supported on a row shard or an index with a pilot replica");
  return BBQ_OK;
}

// the host-side summary of an accept set over n_rows rows: |A|, the cumulative counts per chunk, the first and last non-empty chunk
// (bits: one word per tile, tail bits already cleared; they become the filter's host copy)
void summarize(bbq_filter *f, int64_t n_rows, std::vector<uint64_t> &&bits) {
  f->n_rows = n_rows;
  const int64_t n_chunks = (n_rows + kChunkRows - 1) / kChunkRows, n_words = (int64_t)bits.size();
  f->cum.assign((size_t)n_chunks + 1, 0);
  for (int64_t c = 0; c < n_chunks; ++c) {
    int in_chunk = 0;
    for (int64_t w = c * kTilesPerChunk; w < std::min<int64_t>((c + 1) * kTilesPerChunk, n_words); ++w) in_chunk += __builtin_popcountll(bits[(size_t)w]);
    f->cum[(size_t)c + 1] = f->cum[(size_t)c] + in_chunk;
    if (in_chunk > 0) {
      if (f->first_chunk < 0) f->first_chunk = c;
      f->last_chunk = c;
    }
  }
  f->count = f->cum[(size_t)n_chunks];
  f->h_bits = std::move(bits);
}

void clear_tail(std::vector<uint64_t> &bits, int64_t n_rows) {  // bits at and beyond n_rows are ignored
  if (n_rows & 63) bits.back() &= (1ull << (n_rows & 63)) - 1;
}

int make_filter(bbq_index *ix, std::vector<uint64_t> &&bits, bbq_filter **out) {
  std::unique_ptr<bbq_filter> f(new bbq_filter());
  f->device = ix->device;
  f->ctx = ix->ctx;
  summarize(f.get(), ix->n_rows, std::move(bits));
  const int64_t n_words = (int64_t)f->h_bits.size();
  if (n_words > 0) {
    std::lock_guard<std::mutex> lk(ix->ctx->mu);
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(f->d_bits.alloc((size_t)n_words));
    HIPCHK(hipMemcpy(f->d_bits, f->h_bits.data(), (size_t)n_words * 8, hipMemcpyHostToDevice));
  }
  *out = f.release();
  return BBQ_OK;
}

}  // namespace

extern "C" {

int bbq_filter_create(bbq_index *ix, const uint64_t *accept_bits, int64_t n_words, bbq_filter **out) {
  clear_error();
  if (!out) return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_create: out is null");
  *out = nullptr;
  if (n_words < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_create: n_words < 0");
  if (n_words > 0 && !accept_bits) return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_create: accept_bits is null");
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  int rc = check_filter_index(ix);
  if (rc != BBQ_OK) return rc;
  const int64_t want = (ix->n_rows + 63) / 64;
  if (n_words != want)
    return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_create: n_words is %lld, an index of %lld rows takes %lld", (long long)n_words, (long long)ix->n_rows, (long long)want);
  std::vector<uint64_t> bits(accept_bits, accept_bits + n_words);
  clear_tail(bits, ix->n_rows);
  return make_filter(ix, std::move(bits), out);
}

int bbq_filter_create_rows(bbq_index *ix, const int32_t *rows, int64_t n, bbq_filter **out) {
  clear_error();
  if (!out) return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_create_rows: out is null");
  *out = nullptr;
  if (n < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_create_rows: n < 0");
  if (n > 0 && !rows) return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_create_rows: rows is null");
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  int rc = check_filter_index(ix);
  if (rc != BBQ_OK) return rc;
  std::vector<uint64_t> bits((size_t)((ix->n_rows + 63) / 64), 0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = rows[i];
    if (r < 0 || r >= ix->n_rows) return fail(BBQ_ERR_INVALID_ARG, "向量索引 %lld 不存在", (long long)r);
    bits[(size_t)(r >> 6)] |= 1ull << (r & 63);
  }
  return make_filter(ix, std::move(bits), out);
}

void bbq_filter_destroy(bbq_filter *f) {
  if (!f) return;
  std::lock_guard<std::mutex> lk(f->ctx->mu);
  (void)hipSetDevice(f->device);
  delete f;
}

int64_t bbq_filter_count(const bbq_filter *f) { return f ? f->count : 0; }

int bbq_filter_plan(const uint64_t *accept_bits, int64_t n_rows, int64_t k_dev, int64_t first_segment_rows, int32_t growth, int32_t max_segments,
                    int64_t *segments, int32_t *out_n) {
  clear_error();
  if (!out_n || n_rows < 0 || k_dev < 1 || max_segments < 0 || (max_segments > 0 && !segments) || (n_rows > 0 && !accept_bits))
    return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_plan: null or negative argument");
  if (first_segment_rows < 1024 || first_segment_rows > 8192 || growth < 2 || growth > 1024)
    return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_plan: first_segment_rows is 1024..8192, growth 2..1024 (bbq_set_option)");
  bbq_index ix;  // an index of n_rows rows as far as the plan looks at it: its size and its options; nothing of it is on a device
  ix.n_rows = ix.main.view.n_rows = n_rows;
  ix.opt_s0 = first_segment_rows;
  ix.opt_growth = growth;
  bbq_filter f;
  std::vector<uint64_t> bits(accept_bits, accept_bits + (n_rows + 63) / 64);
  if (n_rows > 0) clear_tail(bits, n_rows);
  summarize(&f, n_rows, std::move(bits));
  const Plan p = build_filtered_plan(&ix, f, k_dev, 0, false);
  *out_n = (int32_t)p.segs.size();
  if ((int32_t)p.segs.size() > max_segments) return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_plan: %d segments, room for %d", (int)p.segs.size(), max_segments);
  for (size_t i = 0; i < p.segs.size(); ++i) {
    segments[3 * i] = p.segs[i].chunk_begin;
    segments[3 * i + 1] = p.segs[i].n_chunks;
    segments[3 * i + 2] = p.segs[i].cap;
  }
  return BBQ_OK;
}

}  // extern "C"
