// bbq_group.cpp - grouped search: bbq_groups_*, bbq_search_grouped_batch (kernels: bbq_group_kernels.hip, and the span search's select
// pass).  A group set is made once for one index: its offsets are checked, the live groups - those with a row the bound filter accepts -
// are numbered on the host, and three small tables go to the device (GroupScoreArgs, bbq_device.h).  A call works through sub-batches
// bounded by scratch: the queries staged in one copy, the score pass, the unpack pass and the span search's select pass over the live
// groups' representatives, the answer blocks back in one copy, and the end every select-pass search has (finish_selected,
// bbq_select.cpp): the device's k proven, the reference's heap replayed over the other queries' representatives.  Every query of a
// call has the same number of representatives, L: whether the select pass runs is decided once per call.
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include "bbq_search.h"

using namespace bbq;

namespace {

// A sub-batch takes at most this many queries and - by default - this many bytes of scratch for the representatives (16 B per live
// group and query: the packed key, the score, the ord), and always at least one query.
constexpr int kGroupMaxQueries = 1024;

// accepted rows of [b, e), b < e: is there one?  bits == null: every row
inline bool any_accepted(const uint64_t *bits, int64_t b, int64_t e) {
  if (!bits) return true;
  const int64_t w0 = b >> 6, w1 = (e - 1) >> 6;
  const uint64_t lo = ~0ull << (b & 63), hi = ~0ull >> (63 - ((e - 1) & 63));
  if (w0 == w1) return (bits[w0] & lo & hi) != 0;
  if ((bits[w0] & lo) || (bits[w1] & hi)) return true;
  for (int64_t w = w0 + 1; w < w1; ++w)
    if (bits[w]) return true;
  return false;
}

int check_offsets(const char *fn, const int64_t *off, int64_t n_groups, int64_t n_rows) {
  if (n_groups < 0) return fail(BBQ_ERR_INVALID_ARG, "%s: n_groups < 0", fn);
  if (!off) return fail(BBQ_ERR_INVALID_ARG, "%s: group_offsets is null", fn);
  if (off[0] != 0) return fail(BBQ_ERR_INVALID_ARG, "%s: group_offsets[0] must be 0", fn);
  for (int64_t g = 0; g < n_groups; ++g)
    if (off[g + 1] < off[g]) return fail(BBQ_ERR_INVALID_ARG, "%s: group_offsets must ascend (group %lld: [%lld, %lld))", fn, (long long)g, (long long)off[g], (long long)off[g + 1]);
  if (off[n_groups] != n_rows)
    return fail(BBQ_ERR_INVALID_ARG, "%s: group_offsets ends at %lld, the index has %lld rows", fn, (long long)off[n_groups], (long long)n_rows);
  return BBQ_OK;
}

// the plan of checked offsets: per group its rank among the live groups or -1 (slot, may be null), L, and the number of non-empty groups
void plan_groups(const int64_t *off, int64_t n_groups, const uint64_t *bits, int32_t *slot, int64_t *live, int64_t *nonempty) {
  int64_t L = 0, ne = 0;
  for (int64_t g = 0; g < n_groups; ++g) {
    const bool is_live = off[g + 1] > off[g] && any_accepted(bits, off[g], off[g + 1]);
    if (off[g + 1] > off[g]) ++ne;
    if (slot) slot[g] = is_live ? (int32_t)L : -1;
    if (is_live) ++L;
  }
  *live = L;
  if (nonempty) *nonempty = ne;
}

}  // namespace

// what a group set can be made for, and searched on: a single-device root index (DESIGN.md "Grouped search", out of scope)
int bbq::check_group_index(const bbq_index *ix) {
  if (ix->multi) return fail(BBQ_ERR_UNSUPPORTED, "grouped search is not supported on a multi-device index");
  if (ix->has_pilot || ix->row_base != 0) return fail(BBQ_ERR_UNSUPPORTED, "grouped search is not supported on a row shard or an index with a pilot replica");
  return BBQ_OK;
}

GroupScoreArgs bbq::group_score_args(bbq_index *ix, const bbq_groups *gs) {
  const int64_t n_tiles = tiles_of(gs->n_rows);
  GroupScoreArgs ga{};
  ga.idx = main_launch_view(ix);
  ga.starts = gs->d_words.get();
  ga.accept = gs->filtered ? gs->d_words.get() + n_tiles + 1 : nullptr;
  ga.first_group = gs->d_index.get();
  ga.slot = reinterpret_cast<const int32_t *>(gs->d_index.get() + n_tiles + 1);
  ga.live = gs->live;
  ga.n_chunks = (int32_t)ix->main.n_chunks();
  ga.l2_shift = l2_share_shift(ix);
  return ga;
}

namespace {

// where a sub-batch of nq queries keeps what in the scratch: [query data | query uniforms | selected queries] come from the host in
// one copy, the answer blocks go back in one, the packed keys, the scores and the ords stay unless a query's heap is replayed
struct Layout {
  size_t qdata, qparams, sel, head_bytes, out, rep, scores, ords, bytes;
  Layout(int nq, int n_sel, int64_t live, size_t qb, size_t out_stride) {
    qdata = 0;
    qparams = qdata + (size_t)nq * qb;
    sel = qparams + (size_t)nq * sizeof(QueryParams);
    head_bytes = sel + (size_t)n_sel * sizeof(SpanQuery);
    out = align16(head_bytes);
    rep = align16(out + (size_t)n_sel * out_stride * 8);
    scores = rep + (size_t)nq * (size_t)live * 8;
    ords = align16(scores + (size_t)nq * (size_t)live * 4);
    bytes = ords + (size_t)nq * (size_t)live * 4;
  }
};

// the group of row r: the last one that begins at or in front of it (the empty groups that begin there too end there)
inline int32_t group_of(const std::vector<int64_t> &off, int64_t r) {
  return (int32_t)(std::upper_bound(off.begin(), off.end(), r) - off.begin() - 1);
}

// the call behind its argument checks, under the context's lock
int grouped_locked(bbq_index *ix, const bbq_groups *gs, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim, int64_t k,
                   int32_t *out_idx, int32_t *out_group, float *out_score, int64_t *out_n, uint8_t *out_status) {
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  // under the lock: the rows the check sees are the rows the kernel reads (an append or a compaction on another thread comes before or after)
  if (gs->device != ix->device || gs->n_rows != ix->main.view.n_rows)
    return fail(BBQ_ERR_INVALID_ARG, "bbq_search_grouped_batch: the group set was made for an index of %lld rows on device %d, this one has %lld rows on device %d",
                (long long)gs->n_rows, gs->device, (long long)ix->main.view.n_rows, ix->device);
  const int64_t L = gs->live;
  if (k > 0 && L > 0 && (!out_idx || !out_score)) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_grouped_batch: null output");
  if (k == 0 || L == 0) {  // nothing to score
    for (int32_t q = 0; q < n_queries; ++q) out_n[q] = 0;
    if (out_status) memset(out_status, 0, (size_t)n_queries);
    return BBQ_OK;
  }

  const int one_bit = query_bits == 1 ? 1 : 0;
  const int planes = planes_of_call(ix, qquant, (int64_t)n_queries * ix->geom.dim, one_bit);
  const size_t qb = (size_t)query_data_bytes(ix, planes);
  const size_t out_stride = (size_t)std::min<int64_t>(k, kSpanSelectMax) + 2;
  const bool sel = k >= 1 && k <= kSpanSelectMax && L > k;  // does the select pass run?  The same for every query of the call

  // the plan: sub-batches of equal size, the last one shorter
  const int64_t budget = (int64_t)ix->opt_group_scratch_mb << 20;
  const int per = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kGroupMaxQueries, n_queries), budget / (16 * L)));
  const Layout big(per, sel ? per : 0, L, qb, out_stride);
  // everything large, before anything is written to the caller's arrays
  const int rc_scratch = reserve_scratch(ix->ctx->d_span, big.bytes, "grouped search");
  if (rc_scratch != BBQ_OK) return rc_scratch;
  const size_t back_words = sel ? (size_t)per * out_stride : 0;
  const size_t host_rows = (size_t)per * (size_t)L;
  std::unique_ptr<uint8_t[]> head(new (std::nothrow) uint8_t[std::max<size_t>(big.head_bytes, 1)]);
  std::unique_ptr<uint64_t[]> back(new (std::nothrow) uint64_t[std::max<size_t>(back_words, 1)]);
  std::unique_ptr<float[]> h_scores(new (std::nothrow) float[host_rows]);      // touched only where a heap is replayed
  std::unique_ptr<uint32_t[]> h_ords(new (std::nothrow) uint32_t[host_rows]);  // the same
  if (!head || !back || !h_scores || !h_ords)
    return fail(BBQ_ERR_OOM, "grouped search: host staging for %zu + %zu + %zu bytes", big.head_bytes, back_words * 8, host_rows * 8);

  uint8_t *d = ix->ctx->d_span;
  hipStream_t st = ix->ctx->aux_stream;
  GroupScoreArgs ga = group_score_args(ix, gs);
  std::vector<SelectQuery> sq((size_t)per);  // every query of a sub-batch: L scores from s * L on, and block s where the select pass runs
  SelectTail t{};
  t.back = back.get();
  t.h_scores = h_scores.get();
  t.h_ords = h_ords.get();
  t.k = k;
  t.out_stride = out_stride;
  t.stream = st;
  t.threads = ix->opt_replay_threads;

  for (int64_t q0 = 0; q0 < n_queries; q0 += per) {
    const int nq = (int)std::min<int64_t>(per, n_queries - q0);
    const Layout lo(nq, sel ? nq : 0, L, qb, out_stride);
    SpanQuery *h_sel = reinterpret_cast<SpanQuery *>(head.get() + lo.sel);
    for (int s = 0; s < nq; ++s) {
      const int64_t q = q0 + s;
      fill_query(ix, head.get() + lo.qdata + (size_t)s * qb, reinterpret_cast<QueryParams *>(head.get() + lo.qparams) + s,
                 qquant + (size_t)q * ix->geom.dim, qcorr + (size_t)q * 4, planes, one_bit, sim);
      if (sel) h_sel[s] = SpanQuery{(int64_t)s * L, L, 0, 0, 0};
    }
    HIPCHK(hipMemcpyAsync(d, head.get(), lo.head_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d + lo.rep, 0, (size_t)nq * (size_t)L * 8, st));
    ga.qplanes = reinterpret_cast<const uint4 *>(d + lo.qdata);
    ga.qparams = reinterpret_cast<const QueryParams *>(d + lo.qparams);
    ga.rep = reinterpret_cast<unsigned long long *>(d + lo.rep);
    ga.n_queries = nq;
    HIPCHK(launch_group_score(ga, planes, st));
    float *d_scores = reinterpret_cast<float *>(d + lo.scores);
    uint32_t *d_ords = reinterpret_cast<uint32_t *>(d + lo.ords);
    HIPCHK(launch_group_unpack(ga.rep, d_scores, d_ords, (int64_t)nq * L, st));
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

    for (int s = 0; s < nq; ++s) sq[(size_t)s] = SelectQuery{L, (int64_t)s * L, sel ? s : -1};
    t.queries = sq.data();
    t.nq = nq;
    t.d_scores = d_scores;
    t.d_ords = d_ords;
    t.out_tag = out_idx + q0 * k;
    t.out_score = out_score + q0 * k;
    t.out_n = out_n + q0;
    t.out_status = out_status ? out_status + q0 : nullptr;
    const int rc = finish_selected(t);  // the representatives of a replayed query in ascending ord
    if (rc != BBQ_OK) return rc;
    if (out_group)
      for (int s = 0; s < nq; ++s)
        for (int64_t j = 0; j < out_n[q0 + s]; ++j) out_group[(q0 + s) * k + j] = group_of(gs->offsets, out_idx[(q0 + s) * k + j]);
  }
  return BBQ_OK;
}

}  // namespace

extern "C" {

int bbq_groups_plan(const int64_t *group_offsets, int64_t n_groups, int64_t n_rows, const uint64_t *accept_bits, int32_t *out_slot, int64_t *out_live) {
  clear_error();
  if (n_rows < 0 || !out_live || (n_groups > 0 && !out_slot)) return fail(BBQ_ERR_INVALID_ARG, "bbq_groups_plan: null or negative argument");
  if (n_groups > 0x7fffffffll) return fail(BBQ_ERR_INVALID_ARG, "bbq_groups_plan: more than 2^31 - 1 groups");
  const int rc = check_offsets("bbq_groups_plan", group_offsets, n_groups, n_rows);
  if (rc != BBQ_OK) return rc;
  std::vector<uint64_t> bits;
  if (accept_bits && n_rows > 0) {  // bits at and beyond n_rows are ignored
    bits.assign(accept_bits, accept_bits + (n_rows + 63) / 64);
    if (n_rows & 63) bits.back() &= (1ull << (n_rows & 63)) - 1;
  }
  plan_groups(group_offsets, n_groups, bits.empty() ? nullptr : bits.data(), out_slot, out_live, nullptr);
  return BBQ_OK;
}

int bbq_groups_create(bbq_index *ix, const int64_t *group_offsets, int64_t n_groups, const bbq_filter *f, bbq_groups **out) {
  clear_error();
  if (!out) return fail(BBQ_ERR_INVALID_ARG, "bbq_groups_create: out is null");
  *out = nullptr;
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  int rc = check_group_index(ix);
  if (rc != BBQ_OK) return rc;
  if (n_groups > 0x7fffffffll) return fail(BBQ_ERR_INVALID_ARG, "bbq_groups_create: more than 2^31 - 1 groups");
  std::lock_guard<std::mutex> lk(ix->ctx->mu);  // the rows the offsets are checked against are the rows of the index now
  const int64_t n_rows = ix->main.view.n_rows;
  rc = check_offsets("bbq_groups_create", group_offsets, n_groups, n_rows);
  if (rc != BBQ_OK) return rc;
  if (n_rows > kGroupMaxRows) return fail(BBQ_ERR_UNSUPPORTED, "bbq_groups_create: an index of more than %lld rows", (long long)kGroupMaxRows);
  if (f && (f->device != ix->device || f->n_rows != n_rows))
    return fail(BBQ_ERR_INVALID_ARG, "bbq_groups_create: the filter was made for an index of %lld rows on device %d, this one has %lld rows on device %d",
                (long long)f->n_rows, f->device, (long long)n_rows, ix->device);
  std::unique_ptr<bbq_groups> g(new bbq_groups());
  g->device = ix->device;
  g->ctx = ix->ctx;
  g->n_rows = n_rows;
  g->n_groups = n_groups;
  g->filtered = f != nullptr;
  g->offsets.assign(group_offsets, group_offsets + n_groups + 1);
  const uint64_t *bits = f ? f->h_bits.data() : nullptr;
  std::vector<int32_t> slot((size_t)n_groups);
  plan_groups(group_offsets, n_groups, bits, slot.data(), &g->live, &g->n_nonempty);
  g->slot = slot;
  if (n_rows == 0) {  // nothing to sweep: every call answers with nothing
    *out = g.release();
    return BBQ_OK;
  }

  // the device tables (GroupScoreArgs): the starts words and - filtered - the accept words; each tile's first group and each non-empty group's slot
  const int64_t n_tiles = tiles_of(n_rows), ne = g->n_nonempty;
  std::vector<uint64_t> words((size_t)(n_tiles + 1) + (f ? (size_t)n_tiles : 0), 0);
  std::vector<uint32_t> index((size_t)(n_tiles + 1) + (size_t)ne + 1, 0);
  int32_t *ne_slot = reinterpret_cast<int32_t *>(index.data() + n_tiles + 1);
  int64_t o = 0;  // the ordinal of the next non-empty group
  for (int64_t i = 0; i < n_groups; ++i) {
    const int64_t b = group_offsets[i], e = group_offsets[i + 1];
    if (e <= b) continue;
    words[(size_t)(b >> 6)] |= 1ull << (b & 63);
    for (int64_t t = (b + kTileRows - 1) >> 6; t <= (e - 1) >> 6; ++t) index[(size_t)t] = (uint32_t)o;  // the tiles whose first row it holds
    ne_slot[o++] = slot[(size_t)i];
  }
  ne_slot[ne] = -1;  // the rows behind the last one: no group
  std::vector<int32_t> live_group((size_t)std::max<int64_t>(g->live, 1));  // the MaxSim search's table: slot -> group number
  for (int64_t i = 0; i < n_groups; ++i)
    if (slot[(size_t)i] >= 0) live_group[(size_t)slot[(size_t)i]] = (int32_t)i;
  if (n_rows & 63) words[(size_t)(n_rows >> 6)] |= 1ull << (n_rows & 63);
  words[(size_t)n_tiles] = 1ull;
  index[(size_t)n_tiles] = (uint32_t)ne;
  if (f) std::copy(f->h_bits.begin(), f->h_bits.begin() + n_tiles, words.begin() + n_tiles + 1);
  HIPCHK(hipSetDevice(ix->device));
  if (g->d_words.alloc(words.size()) != hipSuccess || g->d_index.alloc(index.size()) != hipSuccess || g->d_live_group.alloc(live_group.size()) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "bbq_groups_create: %zu bytes of device tables", words.size() * 8 + index.size() * 4 + live_group.size() * 4);
  }
  HIPCHK(hipMemcpy(g->d_live_group, live_group.data(), live_group.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g->d_words, words.data(), words.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g->d_index, index.data(), index.size() * 4, hipMemcpyHostToDevice));
  *out = g.release();
  return BBQ_OK;
}

void bbq_groups_destroy(bbq_groups *g) {
  if (!g) return;
  std::lock_guard<std::mutex> lk(g->ctx->mu);
  (void)hipSetDevice(g->device);
  delete g;
}

int64_t bbq_groups_count(const bbq_groups *g) { return g ? g->n_groups : 0; }
int64_t bbq_groups_live(const bbq_groups *g) { return g ? g->live : 0; }

int bbq_search_grouped_batch(bbq_index *ix, const bbq_groups *g, int32_t n_queries, const uint8_t *qquant, const double *qcorr, int32_t query_bits, int32_t sim,
                             int64_t k, int32_t *out_idx, int32_t *out_group, float *out_score, int64_t *out_n, uint8_t *out_status) {
  clear_error();
  const int rc = validate_query_args(ix, n_queries, qquant, qcorr, query_bits, sim, k);
  if (rc != BBQ_OK) return rc;
  const int rc2 = check_group_index(ix);
  if (rc2 != BBQ_OK) return rc2;
  if (!g) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_grouped_batch: the group set is null");
  if (n_queries == 0) return BBQ_OK;
  if (!out_n) return fail(BBQ_ERR_INVALID_ARG, "bbq_search_grouped_batch: out_n is null");
  return grouped_locked(ix, g, n_queries, qquant, qcorr, query_bits, sim, k, out_idx, out_group, out_score, out_n, out_status);
}

}  // extern "C"
