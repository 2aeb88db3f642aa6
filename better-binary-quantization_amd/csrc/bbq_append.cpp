// bbq_append.cpp - rows appended to a device-resident index in place (DESIGN.md "Appending rows"): bbq_index_append_rows (rows already
// quantized), bbq_index_append (raw fp32 rows quantized on the device against the index's centroid), bbq_index_reserve / _capacity.
// The kernels are the build's (bbq_build_kernels.hip, bbq_kernels.hip), launched at a row offset.  Every entry point validates and
// allocates first, writes second and publishes the new row count last: an append that fails leaves the index as it was.
#include <string.h>
#include "bbq_search.h"

using namespace bbq;

namespace {

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

// Room for `need_tiles` tiles.  While they fit the capacity nothing happens and the append writes in place; otherwise larger buffers
// (geometric: half as much again as the capacity, at least what is needed; otherwise exactly what is needed) are allocated HERE and
// the tiles in use copied over device to device - the storage itself only changes in commit(), so a failure on the way costs
// nothing but these buffers.
struct Room {
  DevBuf<uint8_t> tiles;
  DevBuf<double> exact;
  int64_t cap_tiles = 0;
  bool grown = false;
  uint8_t *d_tiles = nullptr;   // where the append writes
  double *d_exact = nullptr;
  float *d_add_range = nullptr;
};

int make_room(bbq_index *ix, int64_t need_tiles, Room &r, bool geometric = true) {
  Storage &st = ix->main;
  if (need_tiles <= st.cap_tiles) {
    r.cap_tiles = st.cap_tiles;
    r.d_tiles = st.d_tiles;
    r.d_exact = st.d_exact;
    r.d_add_range = const_cast<float *>(add_range_of(st.d_exact, st.cap_tiles));
    return BBQ_OK;
  }
  const int64_t cap = geometric ? std::max(need_tiles, st.cap_tiles + st.cap_tiles / 2) : need_tiles;
  const bool compact = ix->layout == kLayoutCompact;
  if (r.tiles.alloc((size_t)(cap * ix->tile_stride)) != hipSuccess || (compact && r.exact.alloc((size_t)compact_side_bytes(cap) / 8) != hipSuccess)) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "no device memory for %lld rows (%lld bytes of tiles)", (long long)(cap * kTileRows), (long long)(cap * ix->tile_stride));
  }
  r.cap_tiles = cap;
  r.grown = true;
  r.d_tiles = r.tiles;
  r.d_exact = r.exact;
  r.d_add_range = const_cast<float *>(add_range_of(r.exact, cap));
  const int64_t used = (ix->n_rows + kTileRows - 1) / kTileRows;
  hipStream_t s = ix->ctx->aux_stream;
  if (used > 0) {
    HIPCHK(hipMemcpyAsync(r.d_tiles, st.d_tiles, (size_t)(used * ix->tile_stride), hipMemcpyDeviceToDevice, s));
    if (compact) {
      HIPCHK(hipMemcpyAsync(r.d_exact, st.d_exact, (size_t)(used * kTileRows) * 32, hipMemcpyDeviceToDevice, s));
      HIPCHK(hipMemcpyAsync(r.d_add_range, st.view.add_range, (size_t)used * 8, hipMemcpyDeviceToDevice, s));
    }
  }
  return BBQ_OK;
}

// the append (or the reservation) published: called after the device has completed everything that wrote the new rows and - the index
// is quiet - everything that read the old buffers, which are released here
void commit(bbq_index *ix, Room &r, int64_t n_rows) {
  Storage &st = ix->main;
  if (r.grown) {
    st.d_tiles = std::move(r.tiles);
    st.d_exact = std::move(r.exact);
    st.cap_tiles = r.cap_tiles;
  }
  ix->n_rows = n_rows;
  set_storage_view(ix, st, n_rows, st.row_id_base);
}

// rows in device memory, in the caller's shape (bbq_index_create's), become the rows [n_rows, n_rows + n) of the index
int append_device_rows(bbq_index *ix, const uint8_t *d_codes, const double *d_corr, int64_t n) {
  const bool multibit = ix->store_bits > 1;
  const int64_t pb = multibit ? ix->dim : ix->pb;
  hipStream_t s = ix->ctx->aux_stream;
  // an index without explicit component sums cannot hold a row whose sum is not its popcount / code sum; a multi-bit code must be
  // below 2^indexBits: both asked before anything is written
  uint32_t flags[2] = {0, 0};
  DevBuf<uint32_t> d_flags;
  HIPCHK(d_flags.alloc(2));
  HIPCHK(hipMemsetAsync(d_flags, 0, 8, s));
  if (!ix->has_x1) {
    if (multibit) HIPCHK(launch_check_x1_multibit(d_codes, d_corr, n, ix->dim, d_flags, s));
    else HIPCHK(launch_check_x1(d_codes, d_corr, n, (int32_t)pb, d_flags, s));
  }
  if (multibit) HIPCHK(launch_check_code_range(d_codes, n * ix->dim, ix->index_bits, d_flags + 1, s));
  HIPCHK(hipMemcpyAsync(flags, d_flags, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (flags[1]) return fail(BBQ_ERR_INVALID_ARG, "indexBits=%d: a quantized value is not below %d", ix->index_bits, 1 << ix->index_bits);
  if (flags[0])
    return fail(BBQ_ERR_UNSUPPORTED, "a row's quantizedComponentSum is not its %s and the index stores no explicit sums: holding the row would mean "
                "re-tiling the whole index (create it over all rows instead)", multibit ? "code sum" : "popcount");
  const int64_t row0 = ix->n_rows, total = row0 + n;
  Room room;
  int rc = make_room(ix, (total + kTileRows - 1) / kTileRows, room);
  if (rc != BBQ_OK) return rc;
  if (multibit) {
    HIPCHK(launch_retile_multibit(d_codes, d_corr, total, ix->dim, ix->store_bits, ix->index_bits, room.d_tiles, ix->w16, ix->tile_stride, ix->has_x1, ix->layout,
                                  room.d_exact, d_flags + 1, s, row0));
  } else {
    HIPCHK(launch_retile(d_codes, d_corr, total, (int32_t)pb, room.d_tiles, ix->w16, ix->tile_stride, ix->has_x1, ix->layout, room.d_exact, s, row0));
  }
  if (ix->layout == kLayoutCompact) HIPCHK(launch_tile_add_range(room.d_exact, total, room.d_add_range, s, row0 / kTileRows));
  HIPCHK(hipStreamSynchronize(s));
  commit(ix, room, total);
  return BBQ_OK;
}

}  // namespace

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
  const int64_t need = (rows + kTileRows - 1) / kTileRows;
  if (need <= ix->main.cap_tiles) return BBQ_OK;
  rc = quiesce(ix, "bbq_index_reserve");
  if (rc != BBQ_OK) return rc;
  // exactly what was asked for: the geometric rule is for appends that run out of room
  Room room;
  rc = make_room(ix, need, room, false);
  if (rc != BBQ_OK) return rc;
  HIPCHK(hipStreamSynchronize(ix->ctx->aux_stream));
  commit(ix, room, ix->n_rows);
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
  const int64_t pb = ix->store_bits > 1 ? ix->dim : ix->pb;
  DevBuf<uint8_t> d_codes;
  DevBuf<double> d_corr;
  hipStream_t s = ix->ctx->aux_stream;
  if (d_codes.alloc((size_t)(n * pb)) != hipSuccess || d_corr.alloc((size_t)n * 4) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "bbq_index_append_rows: no device memory to stage %lld rows", (long long)n);
  }
  HIPCHK(hipMemcpyAsync(d_codes, codes, (size_t)(n * pb), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_corr, corr, (size_t)n * 32, hipMemcpyHostToDevice, s));
  return append_device_rows(ix, d_codes, d_corr, n);  // synchronises before the staged rows go
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
  hipStream_t st = ix->ctx->aux_stream;
  const int32_t dim = ix->dim;
  const int64_t npad = (n + kTileRows - 1) / kTileRows * kTileRows;
  const int dim4 = (dim + 3) / 4;
  DevBuf<float> d_in, d_vT4, d_cen;
  DevBuf<unsigned long long> d_bad;
  DevBuf<double> d_corr;
  DevBuf<uint8_t> d_codes;
  if (d_in.alloc((size_t)n * dim) != hipSuccess || d_vT4.alloc((size_t)dim4 * npad * 4) != hipSuccess || d_cen.alloc((size_t)dim4 * 4) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BBQ_ERR_OOM, "bbq_index_append: no device memory to stage %lld x %d fp32", (long long)n, dim);
  }
  // the build's steps without its centroid pass (bbq_build.cpp): transpose, normalizeVector (COSINE), validation
  HIPCHK(hipMemcpyAsync(d_in, vectors, (size_t)n * dim * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_cen, centroid, (size_t)dim * 4, hipMemcpyHostToDevice, st));
  HIPCHK(launch_build_transpose(d_in, n, dim, npad, d_vT4, st));
  HIPCHK(hipStreamSynchronize(st));
  d_in.reset();
  if (sim == BBQ_COSINE) HIPCHK(launch_build_normalize(d_vT4, n, dim, npad, st));
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
  if (ix->index_bits > 1) {
    // as the build does it: one byte per dimension + the corrections in device memory, tile records from there
    if (d_codes.alloc((size_t)n * dim) != hipSuccess || d_corr.alloc((size_t)n * 4) != hipSuccess) {
      (void)hipGetLastError();
      return fail(BBQ_ERR_OOM, "bbq_index_append: no device memory for %lld quantized rows", (long long)n);
    }
    HIPCHK(launch_build_quantize_bits(d_vT4, n, dim, npad, d_cen, sim, lambda, iters, ix->index_bits, d_codes, d_corr, st));
    HIPCHK(hipStreamSynchronize(st));
    d_vT4.reset();
    // the host copies first: nothing can fail behind the commit
    if (corr_out) HIPCHK(hipMemcpy(corr_out, d_corr, (size_t)n * 32, hipMemcpyDeviceToHost));
    if (codes_out) HIPCHK(hipMemcpy(codes_out, d_codes, (size_t)n * dim, hipMemcpyDeviceToHost));
    return append_device_rows(ix, d_codes, d_corr, n);
  }
  // 1-bit: one thread per vector quantizes straight into its lane of the tile records, from the partly filled last tile on
  const int64_t row0 = ix->n_rows, total = row0 + n;
  if (corr_out || ix->has_x1) {
    if (d_corr.alloc((size_t)n * 4) != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "bbq_index_append: no device memory for the corrections"); }
  }
  if (codes_out && d_codes.alloc((size_t)n * ix->pb) != hipSuccess) { (void)hipGetLastError(); return fail(BBQ_ERR_OOM, "bbq_index_append: no device memory for the codes"); }
  if (ix->has_x1) {
    // an index with explicit sums keeps a fourth corrections block the in-place kernel does not write: such rows (rare: the index was
    // created from rows whose sums are not their popcounts) take the row-major path, packed codes from a scratch tile set
    DevBuf<uint8_t> d_tmp, d_rows;
    const int32_t stride1 = tile_stride_of(ix->w16, kLayoutInline, 0);
    if (d_tmp.alloc((size_t)(npad / kTileRows) * stride1) != hipSuccess || d_rows.alloc((size_t)n * ix->pb) != hipSuccess) {
      (void)hipGetLastError();
      return fail(BBQ_ERR_OOM, "bbq_index_append: no device memory for %lld quantized rows", (long long)n);
    }
    HIPCHK(launch_build_quantize1(d_vT4, n, dim, npad, d_cen, sim, lambda, iters, d_tmp, nullptr, d_corr, ix->w16, stride1, kLayoutInline, st));
    HIPCHK(launch_build_untile(d_tmp, n, ix->pb, ix->w16, stride1, d_rows, st));
    HIPCHK(hipStreamSynchronize(st));
    if (corr_out) HIPCHK(hipMemcpy(corr_out, d_corr, (size_t)n * 32, hipMemcpyDeviceToHost));
    if (codes_out) HIPCHK(hipMemcpy(codes_out, d_rows, (size_t)n * ix->pb, hipMemcpyDeviceToHost));
    return append_device_rows(ix, d_rows, d_corr, n);
  }
  Room room;
  rc = make_room(ix, (total + kTileRows - 1) / kTileRows, room);
  if (rc != BBQ_OK) return rc;
  HIPCHK(launch_build_quantize1(d_vT4, n, dim, npad, d_cen, sim, lambda, iters, room.d_tiles, room.d_exact, d_corr, ix->w16, ix->tile_stride, ix->layout, st,
                                row0));
  if (ix->layout == kLayoutCompact) HIPCHK(launch_tile_add_range(room.d_exact, total, room.d_add_range, st, row0 / kTileRows));
  if (corr_out) HIPCHK(hipMemcpyAsync(corr_out, d_corr, (size_t)n * 32, hipMemcpyDeviceToHost, st));
  if (codes_out) {
    HIPCHK(launch_build_untile(room.d_tiles, n, ix->pb, ix->w16, ix->tile_stride, d_codes, st, row0));
    HIPCHK(hipMemcpyAsync(codes_out, d_codes, (size_t)n * ix->pb, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  commit(ix, room, total);
  return BBQ_OK;
}

}  // extern "C"
