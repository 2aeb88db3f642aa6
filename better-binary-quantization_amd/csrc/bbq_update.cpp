// bbq_update.cpp - rows of a device-resident index REPLACED in place (DESIGN.md "Replacing rows"): bbq_index_update_rows (rows already
// quantized), bbq_index_update (raw fp32 rows quantized on the device against the index's centroid), bbq_update_winners (host only:
// which entries of a block take effect).  Both entry points bring the block into device memory in the caller's shape with the
// functions of the append path (bbq_append.cpp), check it there, and only then scatter the winners into their lanes
// (bbq_scatter_rows_kernel, bbq_build_kernels.hip) and recompute the add ranges of the touched tiles.  Validate and allocate first,
// write last: a call that fails has not written a byte the index can see.  The size does not change, so filters stay valid.
#include "bbq_search.h"

using namespace bbq;

namespace bbq {

int update_winners(const int32_t *ords, int64_t n, int64_t n_rows, std::vector<int64_t> &pos) {
  for (int64_t i = 0; i < n; ++i)
    if (ords[i] < 0 || ords[i] >= n_rows) return fail(BBQ_ERR_INVALID_ARG, "向量索引 %d 不存在", ords[i]);
  std::vector<int64_t> order((size_t)n);
  for (int64_t i = 0; i < n; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return ords[a] < ords[b]; });
  pos.clear();
  for (int64_t i = 0; i < n; ++i)  // stable: the last of a run of equal ords is its last occurrence in the block
    if (i + 1 == n || ords[order[(size_t)i]] != ords[order[(size_t)i + 1]]) pos.push_back(order[(size_t)i]);
  return BBQ_OK;
}

int stage_winners(hipStream_t s, const int32_t *ords, int64_t n, const std::vector<int64_t> &pos, DevBuf<int32_t> &d_ords, DevBuf<int64_t> &d_pos) {
  if (d_ords.alloc((size_t)n) != hipSuccess || d_pos.alloc(pos.size()) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "no device memory for the ords of %lld rows", (long long)n);
  }
  HIPCHK(hipMemcpyAsync(d_ords, ords, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_pos, pos.data(), pos.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
  return BBQ_OK;
}

}  // namespace bbq

namespace {

// what both entry points ask before they take the lock: the scope of an append
int check_update(const bbq_index *ix, const int32_t *ords, int64_t n, const char *who) {
  const int rc = check_append_index(ix, 0, who);
  if (rc != BBQ_OK) return rc;
  if (n < 0) return fail(BBQ_ERR_INVALID_ARG, "%s: n < 0", who);
  if (n > 0 && !ords) return fail(BBQ_ERR_INVALID_ARG, "%s: ords is null", who);
  return BBQ_OK;
}

// The n checked rows staged in device memory, in the caller's shape, replace the rows ords[] names: the winners `pos` go to their
// lanes, then each touched tile's add range and row sums are recomputed as a creation computes them (compact layout).  Everything
// that can fail without the device failing - the allocations - comes before the first write.
int scatter_device_rows(bbq_index *ix, const int32_t *ords, int64_t n, const std::vector<int64_t> &pos, const uint8_t *d_codes, const double *d_corr) {
  hipStream_t s = ix->ctx->aux_stream;
  Storage &st = ix->main;
  const bool compact = ix->geom.layout == kLayoutCompact;
  DevBuf<int32_t> d_ords;
  DevBuf<int64_t> d_pos, d_tiles;
  DevBuf<uint32_t> d_bad;
  std::vector<int64_t> tiles;  // the distinct tiles of the winners: they are sorted by ord
  if (compact)
    for (int64_t p : pos)
      if (tiles.empty() || tiles.back() != ords[p] / kTileRows) tiles.push_back(ords[p] / kTileRows);
  int rc = stage_winners(s, ords, n, pos, d_ords, d_pos);
  if (rc != BBQ_OK) return rc;
  if (d_bad.alloc(1) != hipSuccess || (compact && d_tiles.alloc(tiles.size()) != hipSuccess)) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "no device memory for the tiles of %lld rows", (long long)n);
  }
  HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));
  if (compact) HIPCHK(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
  Room room;  // the records as they stand: an update never grows them
  rc = make_room(ix, st, tiles_of(st.view.n_rows), room);
  if (rc != BBQ_OK) return rc;
  HIPCHK(launch_scatter_rows(tile_dest(ix, room), StagedRows{d_codes, d_corr}, d_ords, d_pos, (int64_t)pos.size(), ix->index_bits, d_bad, s));
  if (compact) {
    HIPCHK(launch_tile_add_range_list(room.d_exact, st.view.n_rows, room.d_add_range, d_tiles, (int64_t)tiles.size(), s));
    HIPCHK(launch_tile_row_sums_list(tile_dest(ix, room), st.view.n_rows, room.d_row_sums, d_tiles, (int64_t)tiles.size(), s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return BBQ_OK;
}

}  // namespace

extern "C" {

int bbq_update_winners(const int32_t *ords, int64_t n, int64_t n_rows, int64_t *out_pos, int64_t cap, int64_t *out_n) {
  clear_error();
  if (!out_n || n < 0 || n_rows < 0 || cap < 0 || (n > 0 && !ords) || (cap > 0 && !out_pos))
    return fail(BBQ_ERR_INVALID_ARG, "bbq_update_winners: null or negative argument");
  *out_n = 0;
  std::vector<int64_t> pos;
  const int rc = update_winners(ords, n, n_rows, pos);
  if (rc != BBQ_OK) return rc;
  *out_n = (int64_t)pos.size();
  if (*out_n > cap) return fail(BBQ_ERR_INVALID_ARG, "bbq_update_winners: %lld ords are distinct, room for %lld", (long long)*out_n, (long long)cap);
  std::copy(pos.begin(), pos.end(), out_pos);
  return BBQ_OK;
}

int bbq_index_update_rows(bbq_index *ix, const int32_t *ords, const uint8_t *codes, const double *corr, int64_t n) {
  clear_error();
  int rc = check_update(ix, ords, n, "bbq_index_update_rows");
  if (rc != BBQ_OK) return rc;
  if (n == 0) return BBQ_OK;
  if (!codes || !corr) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  std::vector<int64_t> pos;  // under the lock: the size the ords are held to is the size the rows are written at
  rc = update_winners(ords, n, ix->n_rows, pos);
  if (rc == BBQ_OK) rc = quiesce(ix, "bbq_index_update_rows");
  if (rc != BBQ_OK) return rc;
  DevBuf<uint8_t> d_codes;
  DevBuf<double> d_corr;
  rc = stage_rows(ix, codes, corr, n, d_codes, d_corr);
  // every row of the block is checked, losers included; the record format is never re-decided (Sums::kRequire, as for an append)
  if (rc == BBQ_OK) rc = check_device_rows(ix, d_codes, d_corr, n, Sums::kRequire);
  if (rc != BBQ_OK) return rc;
  return scatter_device_rows(ix, ords, n, pos, d_codes, d_corr);
}

int bbq_index_update(bbq_index *ix, const int32_t *ords, const float *vectors, int64_t n, const float *centroid, int32_t sim, double lambda,
                     int32_t iters, uint8_t *codes_out, double *corr_out, int64_t *bad_row, int32_t *bad_col) {
  clear_error();
  int rc = check_update(ix, ords, n, "bbq_index_update");
  if (rc != BBQ_OK) return rc;
  if (sim < 0 || sim > 2) return fail(BBQ_ERR_INVALID_ARG, "不支持的相似性函数: %d", sim);
  if (iters < 0 || lambda != lambda) return fail(BBQ_ERR_INVALID_ARG, "bad lambda/iters");
  if (n == 0) return BBQ_OK;
  if (!vectors || !centroid) return fail(BBQ_ERR_INVALID_ARG, "输入向量不能为空");
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  std::vector<int64_t> pos;  // under the lock: the size the ords are held to is the size the rows are written at
  rc = update_winners(ords, n, ix->n_rows, pos);
  if (rc == BBQ_OK) rc = quiesce(ix, "bbq_index_update");
  if (rc != BBQ_OK) return rc;
  DevBuf<float> d_vT4, d_cen;
  if (d_cen.alloc((size_t)(ix->geom.dim + 3) / 4 * 4) != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "no device memory for the centroid"); }
  HIPCHK(hipMemcpyAsync(d_cen, centroid, (size_t)ix->geom.dim * 4, hipMemcpyHostToDevice, ix->ctx->aux_stream));
  rc = stage_vectors(ix->ctx, vectors, n, ix->geom.dim, sim, d_vT4, bad_row, bad_col);
  if (rc != BBQ_OK) return rc;
  // the whole block quantized into scratch, in the caller's shape: the index stays untouched until every row has been quantized and
  // checked, and codes_out / corr_out get all n rows, duplicate losers included
  DevBuf<uint8_t> d_codes;
  DevBuf<double> d_corr;
  rc = quantize_staged(ix, d_vT4, n, d_cen, sim, lambda, iters, d_codes, d_corr, codes_out, corr_out);
  if (rc == BBQ_OK) rc = check_device_rows(ix, d_codes, d_corr, n, Sums::kRequire);
  if (rc != BBQ_OK) return rc;
  return scatter_device_rows(ix, ords, n, pos, d_codes, d_corr);
}

}  // extern "C"
