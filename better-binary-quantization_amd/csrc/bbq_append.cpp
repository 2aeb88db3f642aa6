// bbq_append.cpp - the one path that writes rows into a device-resident index (DESIGN.md "Appending rows"), and the entry points that
// grow an index in place: bbq_index_append_rows (rows already quantized), bbq_index_append (raw fp32 rows quantized on the device
// against the index's centroid), bbq_index_reserve / _capacity.  bbq_index_create*, bbq_index_build* and bbq_index_load write their
// rows through the same functions, as appends to an empty storage: the build kernels (bbq_build_kernels.hip) take a
// row offset, and a creation's is 0.  Everything here validates and allocates first, writes second and publishes the new row count
// last: an append that fails leaves the index as it was.
#include <string.h>
#include "bbq_search.h"

using namespace bbq;

namespace {

// the checked rows written behind those `st` holds, and committed
int write_device_rows(bbq_index *ix, Storage &st, const uint8_t *d_codes, const double *d_corr, int64_t n) {
  const int64_t row0 = st.view.n_rows, total = row0 + n;
  hipStream_t s = ix->ctx->aux_stream;
  Room room;
  int rc = make_room(ix, st, tiles_of(total), room);
  if (rc != BBQ_OK) return rc;
  if (n > 0) {
    uint32_t bad = 0;  // raised while multi-bit rows are re-tiled: a code that is not below 2^indexBits (an append has asked before)
    DevBuf<uint32_t> d_bad;
    if (ix->geom.store_bits > 1) {
      HIPCHK(d_bad.alloc(1));
      HIPCHK(hipMemsetAsync(d_bad, 0, 4, s));
    }
    HIPCHK(launch_retile(tile_dest(ix, room), StagedRows{d_codes, d_corr}, total, row0, ix->index_bits, d_bad, s));
    if (d_bad) HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
    rc = finish_rows(ix, room, row0, total);
    if (rc != BBQ_OK) return rc;
    if (bad) return fail(BBQ_ERR_INVALID_ARG, "indexBits=%d: a quantized value is not below %d", ix->index_bits, 1 << ix->index_bits);
  }
  commit(ix, st, room, total);
  return BBQ_OK;
}

// n rows in device memory, in the caller's shape, become the rows behind those `st` holds.  Returns after the device work has
// completed: the caller's scratch rows may go.
int append_device_rows(bbq_index *ix, Storage &st, const uint8_t *d_codes, const double *d_corr, int64_t n, Sums mode) {
  // a storage that holds neither rows nor room has nothing that would have to be re-tiled: an append to it decides as a creation does
  // (and is written into buffers of its own, so rows refused after the write have not touched the index either)
  if (st.cap_tiles == 0) mode = Sums::kDecide;
  const int32_t had_x1 = ix->geom.has_x1;
  int rc = check_device_rows(ix, d_codes, d_corr, n, mode);
  if (rc == BBQ_OK) rc = write_device_rows(ix, st, d_codes, d_corr, n);
  if (rc != BBQ_OK && ix->geom.has_x1 != had_x1) {  // rows that were refused have decided nothing
    ix->geom.has_x1 = had_x1;
    decide_layout(ix);
  }
  return rc;
}

}  // namespace

namespace bbq {

// host rows -> device scratch
int stage_rows(const bbq_index *ix, const uint8_t *codes, const double *corr, int64_t n, DevBuf<uint8_t> &d_codes, DevBuf<double> &d_corr) {
  const int64_t pb = caller_row_bytes(ix);
  hipStream_t s = ix->ctx->aux_stream;
  if (d_codes.alloc((size_t)(n * pb)) != hipSuccess || d_corr.alloc((size_t)n * 4) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "no device memory to stage %lld rows", (long long)n);
  }
  HIPCHK(hipMemcpyAsync(d_codes, codes, (size_t)(n * pb), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_corr, corr, (size_t)n * 32, hipMemcpyHostToDevice, s));
  return BBQ_OK;
}

// quantizedComponentSum of a 1-bit row is its popcount (src/optimizedScalarQuantizer.ts:204-209), of a multi-bit row its code sum; while
// that holds for every row the 8 bytes need not be stored or read.  An index that stores the sums already takes any row.  Nothing is
// written: an append that is refused here has not touched even a padding lane.
int check_device_rows(bbq_index *ix, const uint8_t *d_codes, const double *d_corr, int64_t n, Sums mode) {
  const bool multibit = ix->geom.store_bits > 1, range = multibit && mode == Sums::kRequire;
  if (n > 0 && (!ix->geom.has_x1 || range)) {
    hipStream_t s = ix->ctx->aux_stream;
    uint32_t flags[2] = {0, 0};  // a sum that is not the implied one; a code out of range
    DevBuf<uint32_t> d_flags;
    HIPCHK(d_flags.alloc(2));
    HIPCHK(hipMemsetAsync(d_flags, 0, 8, s));
    if (!ix->geom.has_x1) HIPCHK(launch_check_x1(StagedRows{d_codes, d_corr}, n, ix->geom, d_flags, s));
    if (range) HIPCHK(launch_check_code_range(d_codes, n * ix->geom.dim, ix->index_bits, d_flags + 1, s));
    HIPCHK(hipMemcpyAsync(flags, d_flags, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (flags[1]) return fail(BBQ_ERR_INVALID_ARG, "indexBits=%d: a quantized value is not below %d", ix->index_bits, 1 << ix->index_bits);
    if (flags[0] && mode == Sums::kRequire)
      return fail(BBQ_ERR_UNSUPPORTED, "a row's quantizedComponentSum is not its %s and the index stores no explicit sums: holding the row would mean "
                  "re-tiling the whole index (create it over all rows instead)", multibit ? "code sum" : "popcount");
    if (flags[0]) ix->geom.has_x1 = 1;
  }
  if (mode == Sums::kDecide) decide_layout(ix);  // decided once per index, over all its storages
  return BBQ_OK;
}

// what an append can work on: a single-device root index without a pilot replica (the scope of the filters)
int check_append_index(const bbq_index *ix, int64_t n, const char *who) {
  if (!ix) return fail(BBQ_ERR_INVALID_ARG, "%s: null handle", who);
  if (n < 0) return fail(BBQ_ERR_INVALID_ARG, "%s: n < 0", who);
  if (ix->multi) return fail(BBQ_ERR_UNSUPPORTED, "%s is not supported on a multi-device index", who);
  if (ix->has_pilot || ix->row_base != 0) return fail(BBQ_ERR_UNSUPPORTED, "%s is not supported on a row shard or an index with a pilot replica", who);
  if (ix->n_rows + n > 0xFFFFFFFFll) return fail(BBQ_ERR_UNSUPPORTED, "more than 2^32 rows");
  return BBQ_OK;
}

// the index made quiet: nothing of it in flight on the device.  Context mutex held, device current.
int quiesce(bbq_index *ix, const char *who) {
  if (ix->shard_begun != ix->shard_waited)
    return fail(BBQ_ERR_INVALID_ARG, "%s: a bbq_shard_scan_begin batch of this index has not been waited for", who);
  int rc = settle_shard_slots(ix->ctx, ix);
  if (rc != BBQ_OK) return rc;
  rc = drain(ix);
  if (rc != BBQ_OK) return rc;
  HIPCHK(hipStreamSynchronize(ix->ctx->aux_stream));
  return BBQ_OK;
}

// the one function that allocates tile records: d_tiles and, for the compact layout, the side arrays for `cap` tiles
int alloc_tiles(const bbq_index *ix, int64_t cap, DevBuf<uint8_t> &tiles, DevBuf<double> &exact) {
  if (tiles.alloc((size_t)(cap * ix->geom.tile_stride)) != hipSuccess ||
      (ix->geom.layout == kLayoutCompact && exact.alloc((size_t)compact_alloc_bytes(ix->geom, cap) / 8) != hipSuccess)) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "no device memory for %lld rows (%lld bytes of tiles)", (long long)(cap * kTileRows), (long long)(cap * ix->geom.tile_stride));
  }
  return BBQ_OK;
}

// what every write of the rows [row0, total) into `room` ends with: each touched tile's range of additive corrections and its rows'
// component sums (compact layout), then the device has completed and the rows may be committed
int finish_rows(const bbq_index *ix, const Room &room, int64_t row0, int64_t total) {
  hipStream_t s = ix->ctx->aux_stream;
  if (ix->geom.layout == kLayoutCompact) {
    HIPCHK(launch_tile_add_range(room.d_exact, total, room.d_add_range, s, row0 / kTileRows));
    HIPCHK(launch_tile_row_sums(tile_dest(ix, room), total, room.d_row_sums, s, row0 / kTileRows));
  }
  HIPCHK(hipStreamSynchronize(s));
  return BBQ_OK;
}

int make_room(bbq_index *ix, Storage &st, int64_t need_tiles, Room &r, bool geometric) {
  if (need_tiles <= st.cap_tiles) {
    r.cap_tiles = st.cap_tiles;
    r.d_tiles = st.d_tiles;
    r.d_exact = st.d_exact;
    r.d_add_range = const_cast<float *>(add_range_of(st.d_exact, st.cap_tiles));
    r.d_row_sums = const_cast<uint16_t *>(row_sums_of(st.d_exact, st.cap_tiles, ix->geom));
    return BBQ_OK;
  }
  const int64_t cap = geometric ? std::max(need_tiles, st.cap_tiles + st.cap_tiles / 2) : need_tiles;
  const int rc = alloc_tiles(ix, cap, r.tiles, r.exact);
  if (rc != BBQ_OK) return rc;
  r.cap_tiles = cap;
  r.grown = true;
  r.d_tiles = r.tiles;
  r.d_exact = r.exact;
  r.d_add_range = const_cast<float *>(add_range_of(r.exact, cap));
  r.d_row_sums = const_cast<uint16_t *>(row_sums_of(r.exact, cap, ix->geom));
  const int64_t used = tiles_of(st.view.n_rows);
  hipStream_t s = ix->ctx->aux_stream;
  if (used > 0) {
    HIPCHK(hipMemcpyAsync(r.d_tiles, st.d_tiles, (size_t)(used * ix->geom.tile_stride), hipMemcpyDeviceToDevice, s));
    if (ix->geom.layout == kLayoutCompact) {
      HIPCHK(hipMemcpyAsync(r.d_exact, st.d_exact, (size_t)(used * kTileRows) * 32, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(r.d_add_range, st.view.add_range, (size_t)used * 8, hipMemcpyDeviceToDevice, s));
      if (r.d_row_sums) HIPCHK(hipMemcpyAsync(r.d_row_sums, st.view.row_sums, (size_t)row_sums_bytes(ix->geom, used), hipMemcpyDeviceToDevice, s));
    }
  }
  return BBQ_OK;
}

void commit(bbq_index *ix, Storage &st, Room &r, int64_t n_rows) {
  if (r.grown) {
    st.d_tiles = std::move(r.tiles);
    st.d_exact = std::move(r.exact);
    st.cap_tiles = r.cap_tiles;
  }
  if (&st == &ix->main) ix->n_rows = n_rows;
  set_storage_view(ix, st, n_rows, st.row_id_base);
}

int append_host_rows(bbq_index *ix, Storage &st, const uint8_t *codes, const double *corr, int64_t n, Sums mode) {
  DevBuf<uint8_t> d_codes;
  DevBuf<double> d_corr;
  if (n > 0) {
    const int rc = stage_rows(ix, codes, corr, n, d_codes, d_corr);
    if (rc != BBQ_OK) return rc;
  }
  return append_device_rows(ix, st, d_codes, d_corr, n, mode);
}

int stage_vectors(DeviceCtx *ctx, const float *vectors, int64_t n, int32_t dim, int32_t sim, DevBuf<float> &d_vT4, int64_t *bad_row, int32_t *bad_col) {
  hipStream_t st = ctx->aux_stream;
  const int64_t npad = tiles_of(n) * kTileRows;
  DevBuf<float> d_in;
  DevBuf<unsigned long long> d_bad;
  if (d_in.alloc((size_t)n * dim) != hipSuccess || d_vT4.alloc((size_t)((dim + 3) / 4) * npad * 4) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "no device memory to stage %lld x %d fp32", (long long)n, dim);
  }
  HIPCHK(hipMemcpyAsync(d_in, vectors, (size_t)n * dim * 4, hipMemcpyHostToDevice, st));
  HIPCHK(launch_build_transpose(d_in, n, dim, npad, d_vT4, st));
  HIPCHK(hipStreamSynchronize(st));
  d_in.reset();  // the peak footprint: the transposed copy alone from here on
  if (sim == BBQ_COSINE) HIPCHK(launch_build_normalize(d_vT4, n, dim, npad, st));  // src/binaryQuantizationFormat.ts:174-176
  // :196-211 NaN / Infinity validation on the processed vectors, first offender in row-major order
  unsigned long long bad = ~0ull;
  HIPCHK(d_bad.alloc(1));
  HIPCHK(hipMemcpyAsync(d_bad, &bad, 8, hipMemcpyHostToDevice, st));
  HIPCHK(launch_build_validate(d_vT4, n, dim, npad, d_bad, st));
  HIPCHK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (bad != ~0ull) {
    const int64_t r = (int64_t)(bad / (unsigned long long)dim);
    const int c = (int)(bad % (unsigned long long)dim);
    float v = 0;
    HIPCHK(hipMemcpy(&v, d_vT4 + ((size_t)(c / 4) * npad + r) * 4 + (c & 3), 4, hipMemcpyDeviceToHost));
    if (bad_row) *bad_row = r;
    if (bad_col) *bad_col = c;
    if (v != v) return fail(BBQ_ERR_NAN_INPUT, "向量 %lld 位置 %d 包含NaN值", (long long)r, c);
    return fail(BBQ_ERR_INF_INPUT, "向量 %lld 位置 %d 包含Infinity值", (long long)r, c);
  }
  return BBQ_OK;
}

int quantize_staged(bbq_index *ix, DevBuf<float> &d_vT4, int64_t n, const float *d_cen, int32_t sim, double lambda, int32_t iters,
                    DevBuf<uint8_t> &d_codes, DevBuf<double> &d_corr, uint8_t *codes_out, double *corr_out) {
  hipStream_t st = ix->ctx->aux_stream;
  const int32_t dim = ix->geom.dim;
  const int64_t npad = tiles_of(n) * kTileRows, pb = ix->index_bits > 1 ? dim : pb_of(ix->geom);
  if (d_codes.alloc((size_t)(n * pb)) != hipSuccess || d_corr.alloc((size_t)n * 4) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "no device memory for %lld quantized rows", (long long)n);
  }
  DevBuf<uint8_t> d_tmp;  // lives until the device has completed
  if (ix->index_bits > 1) {
    // more than one bit: the kernel leaves what the reference keeps for such an index - one byte per dimension - and the corrections
    // in device memory; the tile records are built from there exactly as they are from a caller's rows
    HIPCHK(launch_build_quantize_bits(d_vT4, n, dim, npad, d_cen, sim, lambda, iters, ix->index_bits, d_codes, d_corr, st));  // :221-249
  } else {
    // 1-bit rows on the row-major path: packed codes from a scratch tile set without sums
    if (d_tmp.alloc((size_t)(npad / kTileRows) * scratch_tile_dest(ix, nullptr).geom.tile_stride) != hipSuccess) {
      (void)hipGetLastError();
      return fail(BBQ_ERR_OOM, "no device memory for %lld quantized rows", (long long)n);
    }
    const TileDest tmp = scratch_tile_dest(ix, d_tmp);
    HIPCHK(launch_build_quantize1(d_vT4, n, npad, d_cen, sim, lambda, iters, tmp, d_corr, st, 0));
    HIPCHK(launch_build_untile(tmp, n, d_codes, st, 0));
  }
  HIPCHK(hipStreamSynchronize(st));
  d_vT4.reset();  // before the caller allocates what it writes the rows into
  // the host copies first: nothing can fail behind the commit
  if (corr_out) HIPCHK(hipMemcpy(corr_out, d_corr, (size_t)n * 32, hipMemcpyDeviceToHost));
  if (codes_out) HIPCHK(hipMemcpy(codes_out, d_codes, (size_t)(n * pb), hipMemcpyDeviceToHost));
  return BBQ_OK;
}

int quantize_into(bbq_index *ix, DevBuf<float> &d_vT4, int64_t n, const float *d_cen, int32_t sim, double lambda, int32_t iters, Sums mode,
                  uint8_t *codes_out, double *corr_out) {
  hipStream_t st = ix->ctx->aux_stream;
  const int32_t pb = pb_of(ix->geom);
  const int64_t npad = tiles_of(n) * kTileRows;
  DevBuf<double> d_corr;
  DevBuf<uint8_t> d_codes;
  if (ix->index_bits > 1 || ix->geom.has_x1) {
    // multi-bit rows, and an index with explicit sums (rare: it was created from rows whose sums are not their popcounts): freshly
    // quantized rows are taken as a caller's are, from device memory in the caller's shape
    const int rc = quantize_staged(ix, d_vT4, n, d_cen, sim, lambda, iters, d_codes, d_corr, codes_out, corr_out);
    if (rc != BBQ_OK) return rc;
    return append_device_rows(ix, ix->main, d_codes, d_corr, n, mode);
  }
  if (corr_out && d_corr.alloc((size_t)n * 4) != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "no device memory for the corrections"); }
  // 1-bit: one thread per vector quantizes straight into its lane of the tile records, from the partly filled last tile on; a freshly
  // quantized row's component sum IS its popcount, so there is nothing to check
  if (codes_out && d_codes.alloc((size_t)n * pb) != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "no device memory for the codes"); }
  const int64_t row0 = ix->main.view.n_rows, total = row0 + n;
  Room room;
  int rc = make_room(ix, ix->main, tiles_of(total), room);
  if (rc != BBQ_OK) return rc;
  HIPCHK(launch_build_quantize1(d_vT4, n, npad, d_cen, sim, lambda, iters, tile_dest(ix, room), d_corr, st, row0));  // :221-249
  if (corr_out) HIPCHK(hipMemcpyAsync(corr_out, d_corr, (size_t)n * 32, hipMemcpyDeviceToHost, st));
  if (codes_out) {
    HIPCHK(launch_build_untile(tile_dest(ix, room), n, d_codes, st, row0));
    HIPCHK(hipMemcpyAsync(codes_out, d_codes, (size_t)n * pb, hipMemcpyDeviceToHost, st));
  }
  rc = finish_rows(ix, room, row0, total);
  if (rc != BBQ_OK) return rc;
  commit(ix, ix->main, room, total);
  return BBQ_OK;
}

}  // namespace bbq

extern "C" {

int64_t bbq_index_capacity(const bbq_index *ix) {
  if (!ix || ix->multi) return ix ? ix->n_rows : 0;
  return std::max<int64_t>(ix->n_rows, ix->main.cap_tiles * kTileRows);
}

int bbq_index_reserve(bbq_index *ix, int64_t rows) {
  clear_error();
  int rc = check_append_index(ix, 0, "bbq_index_reserve");
  if (rc != BBQ_OK) return rc;
  if (rows < 0) return fail(BBQ_ERR_INVALID_ARG, "bbq_index_reserve: rows < 0");
  if (rows > 0xFFFFFFFFll) return fail(BBQ_ERR_UNSUPPORTED, "more than 2^32 rows");
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  if (tiles_of(rows) <= ix->main.cap_tiles) return BBQ_OK;
  rc = quiesce(ix, "bbq_index_reserve");
  if (rc != BBQ_OK) return rc;
  // exactly what was asked for: the geometric rule is for appends that run out of room
  Room room;
  rc = make_room(ix, ix->main, tiles_of(rows), room, false);
  if (rc != BBQ_OK) return rc;
  HIPCHK(hipStreamSynchronize(ix->ctx->aux_stream));
  commit(ix, ix->main, room, ix->n_rows);
  return BBQ_OK;
}

int bbq_index_append_rows(bbq_index *ix, const uint8_t *codes, const double *corr, int64_t n) {
  clear_error();
  int rc = check_append_index(ix, n, "bbq_index_append_rows");
  if (rc != BBQ_OK) return rc;
  if (n == 0) return BBQ_OK;
  if (!codes || !corr) return fail(BBQ_ERR_INVALID_ARG, "目标向量集合不能为空");
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  rc = quiesce(ix, "bbq_index_append_rows");
  if (rc != BBQ_OK) return rc;
  return append_host_rows(ix, ix->main, codes, corr, n, Sums::kRequire);
}

int bbq_index_append(bbq_index *ix, const float *vectors, int64_t n, const float *centroid, int32_t sim, double lambda, int32_t iters,
                     uint8_t *codes_out, double *corr_out, int64_t *bad_row, int32_t *bad_col) {
  clear_error();
  int rc = check_append_index(ix, n, "bbq_index_append");
  if (rc != BBQ_OK) return rc;
  if (sim < 0 || sim > 2) return fail(BBQ_ERR_INVALID_ARG, "不支持的相似性函数: %d", sim);
  if (iters < 0 || lambda != lambda) return fail(BBQ_ERR_INVALID_ARG, "bad lambda/iters");
  if (n == 0) return BBQ_OK;
  if (!vectors || !centroid) return fail(BBQ_ERR_INVALID_ARG, "输入向量不能为空");
  std::lock_guard<std::mutex> lk(ix->ctx->mu);
  HIPCHK(hipSetDevice(ix->device));
  rc = quiesce(ix, "bbq_index_append");
  if (rc != BBQ_OK) return rc;
  // the rows are quantized against the centroid the index was built with: the caller's
  DevBuf<float> d_vT4, d_cen;
  if (d_cen.alloc((size_t)(ix->geom.dim + 3) / 4 * 4) != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "no device memory for the centroid"); }
  HIPCHK(hipMemcpyAsync(d_cen, centroid, (size_t)ix->geom.dim * 4, hipMemcpyHostToDevice, ix->ctx->aux_stream));
  rc = stage_vectors(ix->ctx, vectors, n, ix->geom.dim, sim, d_vT4, bad_row, bad_col);
  if (rc != BBQ_OK) return rc;
  return quantize_into(ix, d_vT4, n, d_cen, sim, lambda, iters, Sums::kRequire, codes_out, corr_out);
}

}  // extern "C"
