// bbq_compact.cpp - rows taken OUT of a device-resident index (DESIGN.md "Removing rows"): bbq_index_compact keeps the rows a filter
// accepts, bbq_index_remove_rows drops the rows named, bbq_filter_kept_rows tells the host which old row each new row was.  The rows
// never leave the device: the accepted rows are gathered into new tile records (bbq_compact_tiles_kernel, bbq_build_kernels.hip)
// allocated, finished and committed by the functions of the append path (bbq_append.cpp), and the old records are released at the
// commit.  Out of place: validate and allocate first, write second, publish last - a call that fails leaves the index as it was.
#include <memory>
#include "bbq_search.h"

using namespace bbq;

namespace bbq {

int stage_compact_map(const bbq_filter *f, DevBuf<uint32_t> &d_rank, CompactMap *map) {
  const size_t n_words = f->h_bits.size();
  std::vector<uint32_t> rank(n_words + 1, 0);
  for (size_t t = 0; t < n_words; ++t) rank[t + 1] = rank[t] + (uint32_t)__builtin_popcountll(f->h_bits[t]);
  if (d_rank.alloc(n_words + 1) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "no device memory for the ranks of %lld tiles", (long long)n_words);
  }
  HIPCHK(hipMemcpy(d_rank, rank.data(), (n_words + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
  *map = CompactMap{f->d_bits, d_rank, (int64_t)n_words, f->count};
  return BBQ_OK;
}

}  // namespace bbq

extern "C" {

int bbq_index_compact(bbq_index *ix, const bbq_filter *f) {
  clear_error();
  if (!f) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_compact: filter is null");
  int rc = check_append_index(ix, 0, "bbq_index_compact");
  if (rc != BBQ_OK) return rc;
  if (f->device != ix->device || f->ctx != ix->ctx) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_compact: the filter lives on another device than the index");
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  if (f->n_rows != ix->n_rows)
    return fail(BBQ_ERR_INVALID_ARG, "bbq_index_compact: the filter was made for %lld rows, the index has %lld", (long long)f->n_rows, (long long)ix->n_rows);
  rc = quiesce(ix, "bbq_index_compact");
  if (rc != BBQ_OK) return rc;
  const int64_t kept = f->count;
  if (kept == ix->n_rows) return BBQ_OK;  // every row stays where it is, and so does the capacity
  // new records of exactly the tiles the kept rows take, as a creation over them allocates (none for no rows)
  Storage &st = ix->main;
  Room room;
  room.grown = true;
  room.cap_tiles = tiles_of(kept);
  if (kept > 0) {
    rc = alloc_tiles(ix, room.cap_tiles, room.tiles, room.exact);
    if (rc != BBQ_OK) return rc;
    room.d_tiles = room.tiles;
    room.d_exact = room.exact;
    room.d_add_range = const_cast<float *>(add_range_of(room.exact, room.cap_tiles));
    room.d_row_sums = const_cast<uint16_t *>(row_sums_of(room.exact, room.cap_tiles, ix->geom));
    DevBuf<uint32_t> d_rank;
    CompactMap map;
    rc = stage_compact_map(f, d_rank, &map);
    if (rc != BBQ_OK) return rc;
    const TileDest src{st.d_tiles, st.d_exact, ix->geom};  // the record format is not re-decided: source and destination share it
    HIPCHK(launch_compact_tiles(tile_dest(ix, room), src, map, ix->ctx->aux_stream));
    rc = finish_rows(ix, room, 0, kept);  // the device has completed behind this: d_rank may go
    if (rc != BBQ_OK) return rc;
  }
  commit(ix, st, room, kept);  // the old records are released here
  return BBQ_OK;
}

int bbq_index_remove_rows(bbq_index *ix, const int32_t *rows, int64_t n) {
  clear_error();
  int rc = check_append_index(ix, 0, "bbq_index_remove_rows");
  if (rc != BBQ_OK) return rc;
  if (n < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_remove_rows: n < 0");
  if (n > 0 && !rows) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_remove_rows: rows is null");
  const int64_t n_rows = ix->n_rows, n_words = (n_rows + 63) / 64;
  std::vector<uint64_t> keep((size_t)n_words, ~0ull);  // the complement of the rows named; bbq_filter_create clears the tail
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = rows[i];
    if (r < 0 || r >= n_rows) return fail(BBQ_ERR_INVALID_ARG, "向量索引 %lld 不存在", (long long)r);
    keep[(size_t)(r >> 6)] &= ~(1ull << (r & 63));
  }
  bbq_filter *f = nullptr;
  rc = bbq_filter_create(ix, keep.data(), n_words, &f);
  if (rc != BBQ_OK) return rc;
  rc = bbq_index_compact(ix, f);
  bbq_filter_destroy(f);
  return rc;
}

int bbq_filter_kept_rows(const uint64_t *accept_bits, int64_t n_rows, int32_t *out_rows, int64_t cap, int64_t *out_n) {
  clear_error();
  if (!out_n || n_rows < 0 || cap < 0 || (n_rows > 0 && !accept_bits) || (cap > 0 && !out_rows))
    return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_kept_rows: null or negative argument");
  if (n_rows > 0x7fffffffll) return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_kept_rows: more than 2^31-1 rows");
  const int64_t n_words = (n_rows + 63) / 64;
  const auto word = [&](int64_t t) {  // bits at and beyond n_rows are ignored
    const uint64_t w = accept_bits[t];
    return (t == n_words - 1 && (n_rows & 63)) ? w & ((1ull << (n_rows & 63)) - 1) : w;
  };
  int64_t count = 0;
  for (int64_t t = 0; t < n_words; ++t) count += __builtin_popcountll(word(t));
  *out_n = count;
  if (count > cap) return fail(BBQ_ERR_INVALID_ARG, "bbq_filter_kept_rows: %lld rows are kept, room for %lld", (long long)count, (long long)cap);
  int64_t o = 0;
  for (int64_t t = 0; t < n_words; ++t)
    for (uint64_t w = word(t); w; w &= w - 1) out_rows[o++] = (int32_t)(t * 64 + __builtin_ctzll(w));
  return BBQ_OK;
}

}  // extern "C"
